/*
 * legion_batch_layout.h -- the layout of the two counter arrays that describe a mini-batch.
 *
 * Every batch is handed over with two int32[LEGION_COUNTER_WORDS] arrays, `nc` (node counters) and `ec` (edge counters): the
 * reference's update_counter state machine (src/Kernels.cu:112-150), stretched from 2 to H <= LEGION_MAX_HOPS hops.  The sampler
 * kernels write them, everything that sizes a buffer or views a tensor reads them -- through the functions below, which are the
 * one statement of the layout (legion1_amd/layout.py says the same for Python).  Plain C (C99 and _Static_assert), <stdint.h> only;
 * under hipcc the functions are __host__ __device__, in C++ constexpr.
 *
 * Level l = the nodes first reached after l hops (level 0 = the seeds).  Hop h (1..H) expands its input slots -- the seeds at
 * h = 1, else one slot per edge of hop h - 1 -- and finds level h.  ids[] holds the levels back to back, src_off[] / dst_off[]
 * hold the hops' edges back to back.
 *
 *   word   nc                                                   ec
 *   0      running node total (= nodes_through(H) at the end)   running edge total (= edges_through(H) at the end)
 *   1      new nodes of the hop in flight (0 between hops)      edges of the hop in flight (0 between hops)
 *   2      input slots of the next hop                          offset of the current hop's input list in agg_src_ids:
 *                                                               SCRATCH, not a total -- "edges through hop 0" is 0, not ec[2]
 *   3      offset of level 0 in ids[] (0)                       edges through hop 1
 *   4      size   of level 0 (the seeds)                        edges through hop 2
 *   5      offset of level 1 = nodes through level 0            edges through hop 3
 *   6      size   of level 1                                    edges through hop 4
 *   7      offset of level 2 = nodes through level 1            edges through hop 5
 *   ...    3 + 2l offset, 4 + 2l size of level l                2 + h: edges through hop h
 *   5+2H   nodes through level H = the batch's nodes            (2 + H is the last word in use)
 *   15     nodes through level 5 (H = 5): the last word
 *
 * nodes_through(l) = level_offset(l) + level_size(l) = level_offset(l + 1): word 5 + 2l is word 3 + 2(l + 1).
 * A failed server posts nc[] = -1 in every word (nc[LEGION_NC_TOTAL] == -1: no valid batch has it).
 */
#ifndef LEGION_BATCH_LAYOUT_H
#define LEGION_BATCH_LAYOUT_H

#include <stdint.h>

#define LEGION_MAX_HOPS 5         /* the layout's words run out behind 5 hops (asserted below) */
#define LEGION_COUNTER_WORDS 16   /* int32 words of nc and of ec */
#define LEGION_LEVEL_WORDS 2      /* nc words per level: (offset, size), level after level from word 3 */

/* the fixed words */
#define LEGION_NC_TOTAL 0         /* running node total */
#define LEGION_NC_HOP_NEW 1       /* new nodes of the hop in flight */
#define LEGION_NC_NEXT_INPUTS 2   /* input slots of the next hop */
#define LEGION_EC_TOTAL 0         /* running edge total */
#define LEGION_EC_HOP 1           /* edges of the hop in flight */
#define LEGION_EC_INPUT_OFF 2     /* offset of the current hop's input list in agg_src_ids (scratch, not a total) */

#if defined(__cplusplus)
static_assert(5 + LEGION_LEVEL_WORDS * LEGION_MAX_HOPS < LEGION_COUNTER_WORDS, "nc: nodes through level LEGION_MAX_HOPS needs a word");
static_assert(2 + LEGION_MAX_HOPS < LEGION_COUNTER_WORDS, "ec: edges through hop LEGION_MAX_HOPS needs a word");
#else
_Static_assert(5 + LEGION_LEVEL_WORDS * LEGION_MAX_HOPS < LEGION_COUNTER_WORDS, "nc: nodes through level LEGION_MAX_HOPS needs a word");
_Static_assert(2 + LEGION_MAX_HOPS < LEGION_COUNTER_WORDS, "ec: edges through hop LEGION_MAX_HOPS needs a word");
#endif

#if defined(__HIPCC__)
#define LEGION_LAYOUT_FN __host__ __device__ constexpr static inline
#elif defined(__cplusplus)
#define LEGION_LAYOUT_FN constexpr static inline
#else
#define LEGION_LAYOUT_FN static inline
#endif

/* ---- word indices (the writers and the gathers' (offset word, size word) arguments need words, not values) ---- */
LEGION_LAYOUT_FN int legion_idx_level_offset(int l) { return 3 + LEGION_LEVEL_WORDS * l; }   /* nc */
LEGION_LAYOUT_FN int legion_idx_level_size(int l) { return 4 + LEGION_LEVEL_WORDS * l; }     /* nc */
LEGION_LAYOUT_FN int legion_idx_nodes_through(int l) { return 5 + LEGION_LEVEL_WORDS * l; }  /* nc; = legion_idx_level_offset(l + 1) */
LEGION_LAYOUT_FN int legion_idx_edges_through(int h) { return 2 + h; }      /* ec; h >= 1 */
LEGION_LAYOUT_FN int legion_idx_level(int offset_word) { return (offset_word - 3) / LEGION_LEVEL_WORDS; }   /* inverse of legion_idx_level_offset */

/* ---- nodes ---- */
LEGION_LAYOUT_FN int32_t legion_level_offset(const int32_t* nc, int l) { return nc[legion_idx_level_offset(l)]; }
LEGION_LAYOUT_FN int32_t legion_level_size(const int32_t* nc, int l) { return nc[legion_idx_level_size(l)]; }
LEGION_LAYOUT_FN int32_t legion_nodes_through(const int32_t* nc, int l) { return nc[legion_idx_nodes_through(l)]; }
/* nodes of an H-hop batch: the length of ids[] and the rows of the features */
LEGION_LAYOUT_FN int32_t legion_batch_nodes(const int32_t* nc, int H) { return legion_nodes_through(nc, H); }
/* n_in: the nodes of the levels < H = the destination nodes of the first block a trainer runs */
LEGION_LAYOUT_FN int32_t legion_first_block_dst(const int32_t* nc, int H) { return legion_level_offset(nc, H); }

/* ---- edges ---- */
/* edges of the hops 1..h; 0 for h < 1 (word 2 is scratch) */
LEGION_LAYOUT_FN int32_t legion_edges_through(const int32_t* ec, int h) { return h < 1 ? 0 : ec[legion_idx_edges_through(h)]; }
/* the edges of hop h are src_off / dst_off [begin, end) */
LEGION_LAYOUT_FN int32_t legion_hop_edges_begin(const int32_t* ec, int h) { return legion_edges_through(ec, h - 1); }
LEGION_LAYOUT_FN int32_t legion_hop_edges_end(const int32_t* ec, int h) { return legion_edges_through(ec, h); }
LEGION_LAYOUT_FN int32_t legion_batch_edges(const int32_t* ec, int H) { return ec[legion_idx_edges_through(H)]; }   /* H >= 1 */

/* ---- both ---- */
/* input slots of hop h: the seeds at h = 1, else one per edge of hop h - 1 (valid once hop h - 1 is counted, and after the batch) */
LEGION_LAYOUT_FN int32_t legion_hop_inputs(const int32_t* nc, const int32_t* ec, int h)
{
    return h == 1 ? legion_level_size(nc, 0) : legion_hop_edges_end(ec, h - 1) - legion_hop_edges_begin(ec, h - 1);
}
/* rows of the feature buffer an aggregated batch fills: the rows of the levels < H, then one row of sums per input slot of hop H */
LEGION_LAYOUT_FN int32_t legion_agg_rows(const int32_t* nc, const int32_t* ec, int H)
{
    return legion_first_block_dst(nc, H) + legion_hop_inputs(nc, ec, H);
}

#endif /* LEGION_BATCH_LAYOUT_H */
