// serve_modes.cpp -- the serving modes as the environment states them: the only readers of LEGION_AGG_LAST_HOP, LEGION_AGG_NORM,
// LEGION_SAMPLING, LEGION_SAMPLING_SEED, LEGION_LP_DRAW, LEGION_WEIGHTED_DISTINCT, LEGION_SHARED_DRAWS, LEGION_EDGE_IDS, LEGION_EDGE_WEIGHTS and LEGION_AGG_EDGE_WEIGHT (ServeModes, internal.h).  Host code only: no device is touched.
#include "internal.h"

#include <cctype>
#include <cstring>

using namespace legion;

// $LEGION_SAMPLING_SEED: a decimal or 0x hex integer in [0, 2^32)
static bool parse_seed(const char* n, uint32_t& seed)
{
    const bool hex = n[0] == '0' && (n[1] == 'x' || n[1] == 'X');
    const char* digits = hex ? n + 2 : n;
    bool ok = digits[0] != 0 && strlen(digits) <= 16;
    for (const char* c = digits; ok && *c; c++) ok = hex ? isxdigit((unsigned char)*c) != 0 : isdigit((unsigned char)*c) != 0;
    unsigned long long v = 0;
    if (ok) { v = strtoull(digits, nullptr, hex ? 16 : 10); ok = v <= 0xFFFFFFFFull; }
    seed = ok ? (uint32_t)v : 0;
    return ok;
}

// LEGION_AGG_LAST_HOP: atoi, so anything non-numeric is off.  LEGION_AGG_NORM: unset / empty = plain sums, "both" only on a server that aggregates
// the last hop.  LEGION_SAMPLING: unset / empty / "replace" = with replacement, "distinct" or "weighted".  LEGION_SAMPLING_SEED: unset / empty = off.
// LEGION_LP_DRAW: unset / empty / "0" = off, "1" only under a seed (k is resolved against the meta line: serve_modes_resolve_lp_draw).
// LEGION_WEIGHTED_DISTINCT: unset / empty / "0" = off, "1" only with LEGION_SAMPLING=weighted.
// LEGION_SHARED_DRAWS: unset / empty / "0" = off, "1" only with LEGION_SAMPLING=distinct, or =weighted with LEGION_WEIGHTED_DISTINCT=1, under a seed: unseeded, every batch of every epoch
// would prefer the same nodes (the node key depends on the draw word alone), which a server must not do silently.
// LEGION_EDGE_IDS, LEGION_EDGE_WEIGHTS, LEGION_AGG_EDGE_WEIGHT: unset / empty / "0" = off, "1" = on.  Edge ids not under the alias rule (pool_apply_modes'
// reason); edge weights only with edge ids; the edge-weighted sums only with the aggregated mode, edge ids and retained weights, and without a norm.
// A switch: false with the refusal when the value is neither; `what`: what "1" means, for the refusal
static bool parse_switch(const char* var, const char* what, bool& on, std::string& why)
{
    const char* v = getenv(var);
    on = v && strcmp(v, "1") == 0;
    if (on || !v || !v[0] || strcmp(v, "0") == 0) return true;
    why = std::string(var) + "=" + v + " is not a known setting: `1` (" + what + "), `0` or unset";
    return false;
}
bool legion::serve_modes_from_env(ServeModes& m, std::string& why)
{
    m = ServeModes();
    const char* agg = getenv("LEGION_AGG_LAST_HOP");
    m.agg_last_hop = agg && atoi(agg) != 0;
    const char* norm = getenv("LEGION_AGG_NORM");
    if (norm && norm[0]) {
        if (strcmp(norm, "both") != 0) { why = std::string("LEGION_AGG_NORM=") + norm + " is not a known norm: `both` (GraphConv norm='both', out-degree rsqrt inside block 1) or unset"; return false; }
        if (!m.agg_last_hop) { why = "LEGION_AGG_NORM=both needs LEGION_AGG_LAST_HOP=1: only the last hop's neighbour sums are normalised"; return false; }
        m.agg_norm = 1;
    }
    const char* sampling = getenv("LEGION_SAMPLING");
    if (sampling && sampling[0] && strcmp(sampling, "replace") != 0) {
        if (strcmp(sampling, "weighted") == 0) m.sampling = kSamplingWeighted;
        else if (strcmp(sampling, "distinct") == 0) m.sampling = kSamplingDistinct;
        else { why = std::string("LEGION_SAMPLING=") + sampling + " is not a known sampling mode: `replace` (the default: draws with replacement) or `distinct` (min(degree, fan-out) distinct neighbours per row), or `weighted` (draws with replacement in proportion to the edge weights)"; return false; }
    }
    const char* seed = getenv("LEGION_SAMPLING_SEED");
    if (seed && seed[0]) {
        if (!parse_seed(seed, m.seed)) { why = std::string("LEGION_SAMPLING_SEED=") + seed + " is not a sampling seed: a decimal or 0x hex integer in [0, 2^32), or unset (the same batches every epoch)"; return false; }
        m.seeded = true;
    }
    const char* lp = getenv("LEGION_LP_DRAW");
    if (lp && lp[0] && strcmp(lp, "0") != 0) {
        if (strcmp(lp, "1") != 0) { why = std::string("LEGION_LP_DRAW=") + lp + " is not a known setting: `1` (the pos and neg thirds of link-prediction batches are drawn per batch), `0` or unset"; return false; }
        if (!m.seeded) { why = "LEGION_LP_DRAW=1 needs LEGION_SAMPLING_SEED: the thirds are drawn from the batch's draw word"; return false; }
        m.lp_draw = 1;
    }
    const char* wd = getenv("LEGION_WEIGHTED_DISTINCT");
    if (wd && wd[0] && strcmp(wd, "0") != 0) {
        if (strcmp(wd, "1") != 0) { why = std::string("LEGION_WEIGHTED_DISTINCT=") + wd + " is not a known setting: `1` (weighted draws without replacement: distinct columns per row, by edge weight), `0` or unset"; return false; }
        if (m.sampling != kSamplingWeighted) { why = "LEGION_WEIGHTED_DISTINCT=1 needs LEGION_SAMPLING=weighted: the flag turns the weighted draws into draws without replacement"; return false; }
        m.weighted_distinct = true;
    }
    const char* sd = getenv("LEGION_SHARED_DRAWS");
    if (sd && sd[0] && strcmp(sd, "0") != 0) {
        if (strcmp(sd, "1") != 0) { why = std::string("LEGION_SHARED_DRAWS=") + sd + " is not a known setting: `1` (distinct draws by a key of the neighbour node: rows that see the same neighbours pick the same ones), `0` or unset"; return false; }
        if (m.sampling != kSamplingDistinct && !(m.sampling == kSamplingWeighted && m.weighted_distinct)) { why = "LEGION_SHARED_DRAWS=1 needs LEGION_SAMPLING=distinct: the flag keys the distinct draws by the neighbour node"; return false; }
        if (!m.seeded) { why = "LEGION_SHARED_DRAWS=1 needs LEGION_SAMPLING_SEED: the node keys come from the batch's draw word, and without a seed every batch of every epoch would prefer the same nodes"; return false; }
        m.shared_draws = true;
    }
    if (!parse_switch("LEGION_EDGE_IDS", "every sampled edge's position in the whole CSR is served beside the COO", m.edge_ids, why)) return false;
    if (m.edge_ids && !draw_rule_facts(draw_rule_of(m)).picks_column) { why = "LEGION_EDGE_IDS=1 cannot be served under LEGION_SAMPLING=weighted without LEGION_WEIGHTED_DISTINCT=1: the alias table holds the alias neighbour's id, not its column"; return false; }
    if (!parse_switch("LEGION_EDGE_WEIGHTS", "the graph's edge weights are retained and every sampled edge's weight is served beside its id", m.edge_weights, why)) return false;
    if (m.edge_weights && !m.edge_ids) { why = "LEGION_EDGE_WEIGHTS=1 needs LEGION_EDGE_IDS=1: an edge's weight is served beside its id"; return false; }
    if (!parse_switch("LEGION_AGG_EDGE_WEIGHT", "the last hop's neighbour sums scale every row by its edge's weight", m.agg_edge_weight, why)) return false;
    if (m.agg_edge_weight) {
        std::string missing;
        if (!m.agg_last_hop) missing += " needs LEGION_AGG_LAST_HOP=1 (only neighbour sums are scaled);";
        if (!m.edge_ids) missing += " needs LEGION_EDGE_IDS=1 (the weight of a draw is the edge_w that mode hands over);";
        if (!serve_modes_retain_weights(m)) missing += " needs retained edge weights (LEGION_EDGE_WEIGHTS=1, or LEGION_SAMPLING=weighted LEGION_WEIGHTED_DISTINCT=1);";
        if (m.agg_norm) missing += " must not be combined with LEGION_AGG_NORM (GraphConv(norm='both', edge_weight=) has no kernel in this build);";
        if (!missing.empty()) { missing.pop_back(); why = "LEGION_AGG_EDGE_WEIGHT=1" + missing; return false; }
    }
    return true;
}

bool legion::serve_modes_resolve_lp_draw(ServeModes& m, bool lp_lists, int32_t raw_batch_size, std::string& why)
{
    if (!m.lp_draw) return true;
    if (!lp_lists) { why = "LEGION_LP_DRAW=1 needs link-prediction training lists (meta flag 2: [src | pos | neg] thirds per batch)"; return false; }
    if (raw_batch_size < 3 || raw_batch_size % 3 != 0) { why = "LEGION_LP_DRAW=1 needs a batch size divisible by 3 ([src | pos | neg] thirds), the meta line has " + std::to_string(raw_batch_size); return false; }
    m.lp_draw = raw_batch_size / 3;
    return true;
}

// the launcher refuses such a hop per batch (launch_sample_hop): a server that booted would fail every batch, the pre-sampling epoch first
bool legion::serve_modes_fit_fanout(const ServeModes& m, const int32_t* fanout, int32_t hops, std::string& why)
{
    const DrawRuleFacts& rule = draw_rule_facts(draw_rule_of(m));
    for (int32_t h = 0; rule.max_fanout && h < hops; h++)
        if (fanout[h] > rule.max_fanout) {
            why = std::string(rule.env_head) + " takes fan-outs of at most " + std::to_string(rule.max_fanout) + ", hop " + std::to_string(h + 1) + " has " + std::to_string(fanout[h]) + rule.env_tail;
            return false;
        }
    return true;
}
