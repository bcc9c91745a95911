/* Prints every helper of include/legion_batch_layout.h for one batch: stdin "H nc[0..15] ec[0..15]", stdout "name [arg] value" lines.
 * Built by tests/test_batch_layout_cpu.py with the host C compiler: the header is plain C and needs nothing else. */
#include "legion_batch_layout.h"
#include <stdio.h>

int main(void)
{
    int H, i;
    int32_t nc[LEGION_COUNTER_WORDS], ec[LEGION_COUNTER_WORDS];
    if (scanf("%d", &H) != 1 || H < 1 || H > LEGION_MAX_HOPS) return 2;
    for (i = 0; i < LEGION_COUNTER_WORDS; i++) if (scanf("%d", &nc[i]) != 1) return 2;
    for (i = 0; i < LEGION_COUNTER_WORDS; i++) if (scanf("%d", &ec[i]) != 1) return 2;
    printf("MAX_HOPS %d\nCOUNTER_WORDS %d\nLEVEL_WORDS %d\n", LEGION_MAX_HOPS, LEGION_COUNTER_WORDS, LEGION_LEVEL_WORDS);
    printf("NC_TOTAL %d\nNC_HOP_NEW %d\nNC_NEXT_INPUTS %d\n", LEGION_NC_TOTAL, LEGION_NC_HOP_NEW, LEGION_NC_NEXT_INPUTS);
    printf("EC_TOTAL %d\nEC_HOP %d\nEC_INPUT_OFF %d\n", LEGION_EC_TOTAL, LEGION_EC_HOP, LEGION_EC_INPUT_OFF);
    for (i = 0; i <= H; i++) {
        printf("idx_level_offset %d %d\nidx_level_size %d %d\nidx_nodes_through %d %d\n", i, legion_idx_level_offset(i), i, legion_idx_level_size(i), i, legion_idx_nodes_through(i));
        printf("idx_level %d %d\n", legion_idx_level_offset(i), legion_idx_level(legion_idx_level_offset(i)));
        printf("level_offset %d %d\nlevel_size %d %d\nnodes_through %d %d\n", i, legion_level_offset(nc, i), i, legion_level_size(nc, i), i, legion_nodes_through(nc, i));
        printf("edges_through %d %d\n", i, legion_edges_through(ec, i));
    }
    for (i = 1; i <= H; i++) {
        printf("idx_edges_through %d %d\n", i, legion_idx_edges_through(i));
        printf("hop_edges_begin %d %d\nhop_edges_end %d %d\nhop_inputs %d %d\n", i, legion_hop_edges_begin(ec, i), i, legion_hop_edges_end(ec, i), i, legion_hop_inputs(nc, ec, i));
    }
    printf("batch_nodes %d %d\nfirst_block_dst %d %d\nbatch_edges %d %d\nagg_rows %d %d\n", H, legion_batch_nodes(nc, H), H, legion_first_block_dst(nc, H), H, legion_batch_edges(ec, H), H, legion_agg_rows(nc, ec, H));
    return 0;
}
