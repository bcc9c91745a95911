// ipc_service -- the trainer-side Python module of the hand-off (drop-in for
// pytorch_extension/ipc_service.cpp:14-93 + ipc_cuda_kernel.cu:178-230 of the reference):
//   initialize() get_next(feature_dim) get_block_size() get_steps() synchronize() finalize()
// and, beyond the reference: get_next_aggregated*(feature_dim), get_edge_ids() / get_edge_weights(), one function per serving mode.
// All device work goes through the C ABI of liblegion_amd.so (legion_ipc_client_*); tensors are
// zero-copy torch::from_blob views of server-owned device memory, valid until synchronize().
// For 2 hops get_next returns the reference's 7 tensors
//   [ids, features, labels, b1_src, b1_dst, b2_src, b2_dst]   (b2_* alias the prefix of b1_*);
// for H hops it returns 3 + 2H tensors, block k covering the edges of hops 1..H-k+1.
#include <torch/extension.h>

#include <cstdint>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/legion_amd.h"

static LegionIPCClient* env = nullptr;
static int32_t h_node_counter[LEGION_COUNTER_WORDS];   // legion_batch_layout.h draws both arrays word by word
static int32_t h_edge_counter[LEGION_COUNTER_WORDS];
static int32_t g_hops = 2;
// The server's serving modes, read once, in initialize()
static struct ServerModes {
    bool aggregated = false;   // the last hop is handed over as neighbour sums (LEGION_AGG_LAST_HOP=1)
    int agg_norm = 0;          // ... normalised: 0 = plain sums, 1 = out-degree rsqrt inside block 1 (LEGION_AGG_NORM=both)
    int sampling = 0;          // how the server's sampler draws: 0 = with replacement, 1 = distinct neighbours (LEGION_SAMPLING=distinct), 2 = by edge weight (LEGION_SAMPLING=weighted)
    bool seeded = false;       // seeded sampling (LEGION_SAMPLING_SEED): fresh draws per batch, the training list reshuffled per epoch
    uint32_t seed = 0;         // ... the seed (0 is a seed: `seeded` says whether there is one)
    int lp_draw = 0;           // k > 0: the server draws the pos and neg thirds of its 3 k-seed training batches per batch (LEGION_LP_DRAW=1)
    bool weighted_distinct = false;   // the weighted draws are without replacement (LEGION_WEIGHTED_DISTINCT=1; `sampling` stays 2)
    bool shared_draws = false;        // the distinct draws go by a key of the neighbour node (LEGION_SHARED_DRAWS=1)
    bool edge_ids = false;            // every sampled edge's position in the whole CSR is served (LEGION_EDGE_IDS=1): get_edge_ids()
    bool edge_weights = false;        // ... and its weight (LEGION_EDGE_WEIGHTS=1, or weighted-distinct sampling): get_edge_weights()
    bool agg_edge_weight = false;     // the neighbour sums scale every row by its edge's weight (LEGION_AGG_EDGE_WEIGHT=1)
} g_modes;
static bool g_have_batch = false;     // a get_next* has returned a batch: the counters above are its
// ONE consumer thread per process is the contract (the reference's trainer loop, legion_graphsage.py:72-89):
// get_next / synchronize run without the GIL and share `env`, the two counter arrays and the client's current pipe, so the entry points
// are serialised by this lock -- uncontended in the reference's loop, and a second Python thread gets whole counters instead of torn ones.
static std::mutex g_mu;

static void require_env()
{
    TORCH_CHECK(env != nullptr, "ipc_service.initialize() was not called");
}

void InitializeIPC()
{
    env = legion_ipc_client_open(-1); // current device == torch.cuda.set_device(rank) (ipc_cuda_kernel.cu:41)
    TORCH_CHECK(env != nullptr, "ipc_service: cannot attach to the sampling server: ", legion_last_error());
    g_hops = legion_ipc_client_hops(env);
    g_modes.aggregated = legion_ipc_client_agg_last_hop(env) != 0;
    g_modes.agg_norm = legion_ipc_client_agg_norm(env);
    g_modes.sampling = legion_ipc_client_sampling(env);
    g_modes.seeded = legion_ipc_client_sampling_seed(env, &g_modes.seed) != 0;
    g_modes.lp_draw = legion_ipc_client_lp_draw(env);
    g_modes.weighted_distinct = legion_ipc_client_weighted_distinct(env) != 0;
    g_modes.shared_draws = legion_ipc_client_shared_draws(env) != 0;
    g_modes.edge_ids = legion_ipc_client_edge_ids(env) != 0;
    g_modes.edge_weights = legion_ipc_client_edge_weights(env) != 0;
    g_modes.agg_edge_weight = legion_ipc_client_agg_edge_weight(env) != 0;
    g_have_batch = false;
}

void FinalizeIPC()
{
    if (env) legion_ipc_client_close(env);
    env = nullptr;
    g_have_batch = false;
}

// One batch of either hand-off mode.  Default: [ids, features[n, F], labels, (src, dst) x H].  Aggregated (the server runs with
// LEGION_AGG_LAST_HOP=1): [ids, x_in[n_in, F], labels, (src, dst) x H, S[N, F]] -- feature rows of the nodes found before the last hop, and
// one row of neighbour sums per input slot of the last hop, both views of the same server buffer (INTEGRATION.md "Aggregated last hop").
// norm: what the caller expects of the sums (0 = plain, 1 = out-degree rsqrt, S_w of INTEGRATION.md "Normalised sums"): same tensors, other values.
// edge_weight: the caller expects every row of the sums scaled by its edge's weight ("Edge-weighted sums"): same tensors again.
static const char* kEdgeWeightServer = "LEGION_AGG_LAST_HOP=1 LEGION_EDGE_IDS=1 LEGION_EDGE_WEIGHTS=1 LEGION_AGG_EDGE_WEIGHT=1";
static std::vector<torch::Tensor> next_batch(int feature_dim, bool aggregated, int norm = 0, bool edge_weight = false)
{
    std::lock_guard<std::mutex> lock(g_mu);
    require_env();
    TORCH_CHECK(!edge_weight || g_modes.agg_edge_weight, "ipc_service.get_next_aggregated_edge_weight: the server does not scale the neighbour sums by edge weight (start it with ",
                kEdgeWeightServer, ") -- call ", !g_modes.aggregated ? "get_next" : g_modes.agg_norm ? "get_next_aggregated_norm" : "get_next_aggregated");
    TORCH_CHECK(edge_weight || !g_modes.agg_edge_weight, "ipc_service.", !aggregated ? "get_next" : norm ? "get_next_aggregated_norm" : "get_next_aggregated",
                ": the server scales the neighbour sums by each edge's weight (LEGION_AGG_EDGE_WEIGHT=1): every row of the sums is w_e x the neighbour's features -- call get_next_aggregated_edge_weight");
    TORCH_CHECK(!aggregated || !g_modes.aggregated || norm != 0 || g_modes.agg_norm == 0, "ipc_service.get_next_aggregated: the server normalises the neighbour sums (LEGION_AGG_NORM=both): "
                "every row is scaled by its out-degree^-1/2 inside block 1 -- call get_next_aggregated_norm");
    TORCH_CHECK(!aggregated || norm == 0 || (g_modes.aggregated && g_modes.agg_norm == norm), "ipc_service.get_next_aggregated_norm: the server does not normalise the neighbour sums (start it with "
                "LEGION_AGG_LAST_HOP=1 LEGION_AGG_NORM=both) -- call ", g_modes.aggregated ? "get_next_aggregated" : "get_next");
    TORCH_CHECK(aggregated || !g_modes.aggregated, "ipc_service.get_next: the server hands the last hop over as neighbour sums (LEGION_AGG_LAST_HOP=1): rows >= n_in of "
                "its feature buffer are sums, not features -- call get_next_aggregated");
    TORCH_CHECK(!aggregated || g_modes.aggregated, "ipc_service.get_next_aggregated: the server does not aggregate the last hop (start it with LEGION_AGG_LAST_HOP=1) -- call get_next");
    legion_ipc_client_wait(env); // env->Wait(), ipc_service.cpp:42
    g_have_batch = false;
    legion_ipc_client_read_counters(env, h_node_counter, h_edge_counter);
    // a server that failed mid-batch posts the pipe with every node-counter word at -1 (runner.cpp, post_poisoned)
    TORCH_CHECK(h_node_counter[LEGION_NC_TOTAL] >= 0, "ipc_service: the sampling server failed (poisoned batch posted)");
    const int dev = GetGPUDevice();
    const auto device = torch::Device(torch::kCUDA, dev);
    const auto i32 = torch::TensorOptions().dtype(torch::kI32).device(device);
    const auto f32 = torch::TensorOptions().dtype(torch::kF32).device(device);
    const int H = g_hops;
    const int64_t n_nodes = legion_batch_nodes(h_node_counter, H);
    const int64_t n_in = legion_first_block_dst(h_node_counter, H);
    const int64_t n_runs = legion_hop_inputs(h_node_counter, h_edge_counter, H);
    const int64_t n_rows = aggregated ? n_in + n_runs : n_nodes;       // rows of the feature buffer this batch fills
    // the feature buffer holds a bounded number of rows (1.2 x the largest pre-sampled batch, Server.cu:275): a batch that reaches more
    // nodes must not be viewed as [n, F] (the reference does, unchecked: ipc_cuda_kernel.cu:200 -- a read past the allocation)
    const int64_t rows = legion_ipc_client_feature_rows(env);
    TORCH_CHECK(rows <= 0 || n_rows <= rows, "ipc_service: the batch has ", n_rows, aggregated ? " rows (features + neighbour sums)" : " nodes", " but the server's feature buffer holds ", rows,
                " rows (sized from the pre-sampling epoch; use a training batch size >= the validation / test batch size)");
    for (int w = LEGION_BUF_IDS; w <= LEGION_BUF_AGG_DST; w++)    // legion_ipc_client_open refuses a server that has not registered its buffers; never build a tensor on a null one
        TORCH_CHECK(legion_ipc_client_buffer(env, w) != nullptr, "ipc_service: hand-off buffer ", w, " of this GPU was never registered by the server");
    std::vector<torch::Tensor> out;
    out.push_back(torch::from_blob(legion_ipc_client_buffer(env, LEGION_BUF_IDS), {n_nodes}, i32));
    out.push_back(torch::from_blob(legion_ipc_client_buffer(env, LEGION_BUF_FEATURES), {aggregated ? n_in : n_nodes, (int64_t)feature_dim}, f32));
    out.push_back(torch::from_blob(legion_ipc_client_buffer(env, LEGION_BUF_LABELS), {(int64_t)legion_nodes_through(h_node_counter, 0)}, i32));
    for (int k = 1; k <= H; k++) {
        const int64_t n_edges = legion_edges_through(h_edge_counter, H - k + 1); // block k: the hops 1..H-k+1 (ec[4], ec[3] at H = 2: ipc_cuda_kernel.cu:198-213)
        out.push_back(torch::from_blob(legion_ipc_client_buffer(env, LEGION_BUF_AGG_SRC), {n_edges}, i32));
        out.push_back(torch::from_blob(legion_ipc_client_buffer(env, LEGION_BUF_AGG_DST), {n_edges}, i32));
    }
    if (aggregated)
        out.push_back(torch::from_blob((float*)legion_ipc_client_buffer(env, LEGION_BUF_FEATURES) + n_in * (int64_t)feature_dim, {n_runs, (int64_t)feature_dim}, f32));
    g_have_batch = true;
    return out;
}

// The edge buffers of the batch the last get_next* returned: H views of the current pipe's buffer, view k of the length of block k's src / dst
// pair (the edges of hops 1..H-k+1, the same prefix rule and order).  which: 0 = edge ids (int64), 1 = edge weights (float32).
static std::vector<torch::Tensor> edge_views(int which)
{
    std::lock_guard<std::mutex> lock(g_mu);
    require_env();
    const char* name = which ? "ipc_service.get_edge_weights" : "ipc_service.get_edge_ids";
    TORCH_CHECK(g_modes.edge_ids, name, ": the server does not serve edge ids (start it with LEGION_EDGE_IDS=1", which ? " LEGION_EDGE_WEIGHTS=1)" : ")");
    TORCH_CHECK(!which || g_modes.edge_weights, name, ": the server does not serve edge weights (start it with LEGION_EDGE_IDS=1 LEGION_EDGE_WEIGHTS=1)");
    TORCH_CHECK(g_have_batch, name, ": no batch yet -- call it after get_next (it returns the edges of the batch the last get_next* returned)");
    void* buf = legion_ipc_client_edge_buffer(env, which);
    TORCH_CHECK(buf != nullptr, name, ": the edge buffer of this GPU was never registered by the server (LEGION_EDGE_IDS=1)");
    const int H = g_hops;
    const int64_t all = legion_edges_through(h_edge_counter, H), elems = legion_ipc_client_edge_elems(env);
    TORCH_CHECK(all <= elems, name, ": the batch has ", all, " edges but the server's edge buffers hold ", elems, " (LEGION_EDGE_IDS=1)");
    const auto device = torch::Device(torch::kCUDA, GetGPUDevice());
    const auto opt = torch::TensorOptions().dtype(which ? torch::kF32 : torch::kI64).device(device);
    std::vector<torch::Tensor> out;
    for (int k = 1; k <= H; k++) out.push_back(torch::from_blob(buf, {(int64_t)legion_edges_through(h_edge_counter, H - k + 1)}, opt));
    return out;
}

std::vector<torch::Tensor> get_next(int feature_dim) { return next_batch(feature_dim, false); }
std::vector<torch::Tensor> get_next_aggregated(int feature_dim) { return next_batch(feature_dim, true); }
std::vector<torch::Tensor> get_next_aggregated_norm(int feature_dim) { return next_batch(feature_dim, true, 1); }
std::vector<torch::Tensor> get_next_aggregated_edge_weight(int feature_dim) { return next_batch(feature_dim, true, 0, true); }
std::vector<torch::Tensor> get_edge_ids() { return edge_views(0); }
std::vector<torch::Tensor> get_edge_weights() { return edge_views(1); }
bool aggregated() { require_env(); return g_modes.aggregated; }
int aggregate_norm() { require_env(); return g_modes.agg_norm; }
const char* sampling() { require_env(); return g_modes.sampling == 2 ? "weighted" : g_modes.sampling ? "distinct" : "replace"; }
pybind11::object sampling_seed() { require_env(); return g_modes.seeded ? pybind11::object(pybind11::int_(g_modes.seed)) : pybind11::object(pybind11::none()); }

int lp_draw() { require_env(); return g_modes.lp_draw; }
bool weighted_distinct() { require_env(); return g_modes.weighted_distinct; }
bool shared_draws() { require_env(); return g_modes.shared_draws; }
bool edge_ids() { require_env(); return g_modes.edge_ids; }
bool edge_weights() { require_env(); return g_modes.edge_weights; }
bool aggregate_edge_weight() { require_env(); return g_modes.agg_edge_weight; }

// [b1_src_nodes, b1_dst_nodes, b2_src_nodes, b2_dst_nodes, ...] = [nc9, nc7, nc7, nc5] at H = 2
// (ipc_service.cpp:60-72)
std::vector<int> get_block_size()
{
    std::lock_guard<std::mutex> lock(g_mu);
    std::vector<int> ret;
    const int H = g_hops;
    for (int k = 1; k <= H; k++) {
        ret.push_back(legion_nodes_through(h_node_counter, H - k + 1));
        ret.push_back(legion_nodes_through(h_node_counter, H - k));
    }
    return ret;
}

std::vector<int32_t> get_steps()
{
    require_env();
    int32_t s[3];
    legion_ipc_client_steps(env, s);
    return {s[0], s[1], s[2]};
}

void Synchronize()
{
    std::lock_guard<std::mutex> lock(g_mu);
    require_env();
    // env->Post(), ipc_service.cpp:83-85.  legion_ipc_client_post waits for the device first: the reference trainers call this with
    // their optimizer step still queued (legion_graphsage.py:93-116), and a posted pipe is overwritten by the server
    legion_ipc_client_post(env);
    g_have_batch = false;        // the pipe went back: get_edge_ids / get_edge_weights have no batch until the next get_next*
}

int get_hops() { return g_hops; }

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m)
{
    // get_next blocks on the pipe's semaphore and synchronize on the trainer's device: neither touches Python state, so both run without the GIL
    // (the reference holds it: a trainer's other Python threads stall for as long as the server takes to produce a batch)
    m.def("get_next", &get_next, "dataset get next (HIP)", pybind11::call_guard<pybind11::gil_scoped_release>());
    m.def("get_next_aggregated", &get_next_aggregated, "next batch of a server that hands the last hop over as neighbour sums (extension)", pybind11::call_guard<pybind11::gil_scoped_release>());
    m.def("get_next_aggregated_norm", &get_next_aggregated_norm, "next batch of a server that hands the last hop over as out-degree-normalised neighbour sums (extension)", pybind11::call_guard<pybind11::gil_scoped_release>());
    m.def("get_next_aggregated_edge_weight", &get_next_aggregated_edge_weight, "next batch of a server that hands the last hop over as neighbour sums scaled by each edge's weight (extension)", pybind11::call_guard<pybind11::gil_scoped_release>());
    m.def("get_edge_ids", &get_edge_ids, "per block, every edge's position in the whole CSR (int64), of the batch the last get_next* returned; valid until synchronize() (LEGION_EDGE_IDS=1; extension)");
    m.def("get_edge_weights", &get_edge_weights, "per block, every edge's weight (float32), of the batch the last get_next* returned; valid until synchronize() (LEGION_EDGE_WEIGHTS=1; extension)");
    m.def("lp_draw", &lp_draw, "k: the server draws the pos and neg thirds of its 3 k-seed training batches per batch (LEGION_LP_DRAW=1), 0 = it does not (extension)");
    m.def("weighted_distinct", &weighted_distinct, "whether the server's weighted draws are without replacement (LEGION_WEIGHTED_DISTINCT=1; sampling() stays \"weighted\"); extension");
    m.def("shared_draws", &shared_draws, "whether the server's distinct draws go by a key of the neighbour node (LEGION_SHARED_DRAWS=1; extension)");
    m.def("edge_ids", &edge_ids, "whether the server serves every sampled edge's position in the whole CSR (LEGION_EDGE_IDS=1; extension)");
    m.def("edge_weights", &edge_weights, "whether the server serves every sampled edge's weight (LEGION_EDGE_WEIGHTS=1, or weighted-distinct sampling; extension)");
    m.def("aggregate_edge_weight", &aggregate_edge_weight, "whether the server scales the neighbour sums by each edge's weight (LEGION_AGG_EDGE_WEIGHT=1; extension)");
    m.def("aggregated", &aggregated, "whether the server hands the last hop over as neighbour sums (extension)");
    m.def("aggregate_norm", &aggregate_norm, "how the server normalises the neighbour sums: 0 = not, 1 = out-degree rsqrt inside block 1 (extension)");
    m.def("sampling", &sampling, "how the server's sampler draws: \"replace\" (with replacement, the default), \"distinct\" (LEGION_SAMPLING=distinct) or \"weighted\" (LEGION_SAMPLING=weighted: with replacement, by edge weight); extension");
    m.def("sampling_seed", &sampling_seed, "the server's sampling seed (LEGION_SAMPLING_SEED: fresh draws per batch, the training list reshuffled per epoch), or None: the same batches every epoch (extension)");
    m.def("get_block_size", &get_block_size, "get dgl block size");
    m.def("get_steps", &get_steps, "get steps");
    m.def("initialize", &InitializeIPC, "InitializeIPC");
    m.def("finalize", &FinalizeIPC, "FinalizeIPC");
    m.def("synchronize", &Synchronize, "synchronize", pybind11::call_guard<pybind11::gil_scoped_release>());
    m.def("get_hops", &get_hops, "number of hops the server samples (extension)");
}
