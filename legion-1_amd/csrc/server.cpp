// server.cpp -- the sampling server: meta line, dataset sources, seed split, table placement, boot, run loop
//   GPUServer   src/Server.cu:43-161    (boot, pre-sampling epoch, cache build, run loop)
//   GPUGraphStore (loader)  src/GPUGraphStore.cu:30-143,190-443  (meta_config + raw files + seed split)
// The Intel-PCM monitor of the reference (Server.h:54-135) is not rebuilt: CostModel gets its
// transaction input from the collected hotness instead (cache.cpp).
#include "internal.h"

#include <algorithm>
#include <chrono>
#include <cstring>
#include <fcntl.h>
#include <fstream>
#include <iostream>
#include <optional>
#include <sstream>
#include <sys/mman.h>
#include <sys/stat.h>
#include <thread>
#include <unistd.h>

#include "audit_hooks.h"

using namespace legion;

namespace {

// raw little-endian file -> memory (the mmap_*_read family, GPUGraphStore.cu:30-143)
bool read_file(const std::string& path, void* dst, int64_t max_bytes, int64_t* got = nullptr, bool quiet = false)
{
    int fd = open(path.c_str(), O_RDONLY);
    if (fd == -1) {
        if (!quiet) log_out() << "cannout open file: " << path << "\n";
        return false;
    }
    struct stat st;
    fstat(fd, &st);
    int64_t len = std::min<int64_t>(st.st_size, max_bytes);
    const void* buf = mmap(nullptr, (size_t)(len > 0 ? len : 1), PROT_READ, MAP_PRIVATE, fd, 0);
    if (buf == MAP_FAILED) { close(fd); return false; }
    memcpy(dst, buf, (size_t)len);
    munmap((void*)buf, (size_t)(len > 0 ? len : 1));
    close(fd);
    if (got) *got = len;
    return true;
}

struct Meta { // ReadMetaFIle, GPUGraphStore.cu:190-223
    std::string dataset_path;
    int32_t raw_batch_size = 0, node_num = 0, float_attr_len = 0, epoch = 0, partition = 0;
    int32_t set_num[kModes] = {0, 0, 0};   // seed-set sizes by mode: training, validation, testing
    int64_t edge_num = 0, cache_memory = 0;
};

// Dataset source `synth:<workload>[:<scale>[:<skew>]]` (extension): the tables of the named synthetic shape are generated on the device by
// the legion_synth_* calls bench.py uses -- 64 GB of files per start is not an option for the papers100M shape.  V, E, F of the meta line
// must be the generator's (E = 0: not checked); the seed-set sizes of the meta line take the first n ids of the generator's train / valid /
// test ranges.
struct SynthSource {
    std::string name;
    double scale = 1.0;
    int32_t skew = 205;
};

} // namespace

struct Server {
    int shard_count = 0, train_step = 0, max_step = 0;
    bool replicated = false;   // CSR + features replicated into every GPU's HBM: the cache has nothing to add
    std::string meta_path = "./meta_config";
    std::vector<int32_t> fanout{25, 10}; // Server.cu:68-69
    Meta meta;
    SynthSource synth_src;     // meta.dataset_path, when it names a synth: source
    GPUGraphStorage* graph = nullptr;
    GPUNodeStorage* noder = nullptr;
    GPUCache* cache = nullptr;
    IPCEnv* env = nullptr;
    std::vector<Runner*> runners;
    std::vector<RunnerParams*> params;
    int64_t* indptr = nullptr;
    int32_t* indices = nullptr;
    float* feats = nullptr;
    bool synth = false;        // the tables were generated in HBM (dataset source `synth:`), not read into pinned host memory
    int32_t synth_pitch = 0;   // floats between two feature rows of the generated tables
};

namespace {

// The seed lists the dataset source gives the split, by mode; from files also every node's label and, when the file exists,
// partition_<G>_bn
struct SeedLists {
    std::vector<int32_t> ids[kModes];
    std::vector<int32_t> labels, partition;
    bool have_part = false;
};

// One mode's seeds after the split: ids and labels per partition, and the per-partition views LegionBuildInfo takes of them
struct SeedSplit {
    std::vector<std::vector<int32_t>> ids, labels;
    std::vector<int32_t> num;
    std::vector<const int32_t*> id_ptr, label_ptr;
};

// The meta line, logged as the reference does.  Returns the refusal text (empty: accepted).  Host code only.
std::string read_meta(const std::string& path, Meta& m)
{
    std::ifstream f(path);
    if (!f.is_open()) { log_out() << "unable to open meta config file\n"; return "Server_Initialize: meta_config missing"; }
    std::string line;
    getline(f, line);
    std::istringstream iss(line);
    iss >> m.dataset_path >> m.raw_batch_size >> m.node_num >> m.edge_num >> m.float_attr_len >> m.set_num[LEGION_TRAINMODE] >>
        m.set_num[LEGION_VALIDMODE] >> m.set_num[LEGION_TESTMODE] >> m.cache_memory >> m.epoch >> m.partition;
    log_out() << "Dataset path:       " << m.dataset_path << "\nRaw Batchsize:      " << m.raw_batch_size
              << "\nGraph nodes num:    " << m.node_num << "\nGraph edges num:    " << m.edge_num
              << "\nFeature dim:        " << m.float_attr_len << "\nTraining set num:   " << m.set_num[LEGION_TRAINMODE]
              << "\nValidation set num: " << m.set_num[LEGION_VALIDMODE] << "\nTesting set num:    " << m.set_num[LEGION_TESTMODE]
              << "\nCache memory:       " << m.cache_memory << "\nTrain epoch:        " << m.epoch
              << "\nPartition?:         " << m.partition << "\n";
    // The reference reads the eleven fields unchecked (GPUGraphStore.cu:190-223): a short or mistyped line leaves zeros behind and the
    // first division by the batch size or the first zero-byte table ends the server without a message.  Refuse it here, by name.
    const int32_t min_set = *std::min_element(m.set_num, m.set_num + kModes), max_set = *std::max_element(m.set_num, m.set_num + kModes);
    const char* bad = nullptr;
    if (iss.fail()) bad = "fewer than eleven fields (path batch V E F n_train n_valid n_test cache_bytes epochs partition_flag)";
    else if (m.raw_batch_size < 1) bad = "batch size < 1";
    else if (m.node_num < 1) bad = "node count < 1";
    else if (m.edge_num < 0) bad = "negative edge count";
    else if (m.float_attr_len < 1) bad = "feature dim < 1";
    else if (min_set < 0) bad = "negative seed-set size";
    else if (max_set > m.node_num) bad = "a seed set larger than the node count";
    else if (m.cache_memory < 0) bad = "negative cache budget";
    else if (m.epoch < 0) bad = "negative epoch count";
    else if (m.partition < 0 || m.partition > 2) bad = "partition flag outside 0..2";
    return bad ? std::string("Server_Initialize: meta_config refused: ") + bad : std::string();
}

// `synth:<workload>[:<scale>[:<skew>]]` -> src; false for a dataset path that names files
bool parse_synth(const std::string& path, SynthSource& src)
{
    if (path.rfind("synth:", 0) != 0) return false;
    const std::string rest = path.substr(6);
    const size_t c1 = rest.find(':');
    src.name = rest.substr(0, c1);
    if (c1 != std::string::npos) {
        const std::string tail = rest.substr(c1 + 1);
        const size_t c2 = tail.find(':');
        src.scale = atof(tail.substr(0, c2).c_str());
        if (c2 != std::string::npos) src.skew = atoi(tail.substr(c2 + 1).c_str());
    }
    return true;
}

// One copy of the synthetic tables on the CURRENT device: degrees -> in-place scan -> indptr, neighbours, features.
bool synth_tables_here(const LegionSynthSpec& sp, int32_t skew, int32_t pitch, int64_t** indptr, int32_t** indices, float** feats, int64_t* E)
{
    const int32_t V = sp.V;
    HIP_CHECK(hipMalloc(indptr, ((size_t)V + 1) * sizeof(int64_t)));
    if (!*indptr) return false;
    HIP_CHECK(hipMemset(*indptr, 0, sizeof(int64_t)));
    legion_synth_degrees(nullptr, *indptr + 1, 0, V, sp.ladder);
    inclusive_scan_i64(nullptr, *indptr + 1, *indptr + 1, V);
    HIP_CHECK(hipMemcpy(E, *indptr + V, sizeof(int64_t), hipMemcpyDeviceToHost));
    HIP_CHECK(hipMalloc(indices, (size_t)std::max<int64_t>(*E, 1) * sizeof(int32_t)));
    if (!*indices) return false;
    legion_synth_neighbors_skew(nullptr, *indices, 0, *E, V, sp.M, sp.C, skew);
    HIP_CHECK(hipMalloc(feats, (size_t)V * pitch * sizeof(float)));
    if (!*feats) return false;
    if (pitch > sp.F) HIP_CHECK(hipMemset(*feats, 0, (size_t)V * pitch * sizeof(float)));
    legion_synth_features_pitched(nullptr, *feats, 0, V, sp.F, pitch);
    HIP_CHECK(hipDeviceSynchronize());
    return !error_pending();
}

// synth: source: check the meta line against the generator, generate the tables on logical GPU 0, list the seeds.
bool load_synth(Server* s, LegionSynthSpec& spec, SeedLists& lists)
{
    Meta& m = s->meta;
    const SynthSource& src = s->synth_src;
    if (legion_synth_spec(src.name.c_str(), src.scale, &spec) != 0) { LEGION_ARG_ERROR("Server_Initialize: the synth: dataset path names no known workload / scale"); return false; }
    if (spec.V != m.node_num || spec.F != m.float_attr_len || src.skew < 0 || src.skew > 256) {
        LEGION_ARG_ERROR("Server_Initialize: node count / feature dim of the meta line differ from the synth: generator's");
        return false;
    }
    const int32_t have[kModes] = {spec.n_train, spec.n_valid, spec.n_test};
    for (int mode = 0; mode < kModes; mode++)
        if (m.set_num[mode] > have[mode] || m.set_num[mode] < 0) {
            LEGION_ARG_ERROR("Server_Initialize: a seed set of the meta line is larger than the synth: generator's");
            return false;
        }
    log_out() << "Start generate graph (" << src.name << ", scale " << src.scale << ", skew " << src.skew << "/256)\n";
    s->synth = true;
    s->synth_pitch = legion_row_pitch(spec.F);
    {
        DeviceGuard guard(0);
        int64_t E = 0;
        if (!synth_tables_here(spec, src.skew, s->synth_pitch, &s->indptr, &s->indices, &s->feats, &E)) {
            LEGION_ARG_ERROR("Server_Initialize: generating the synth: tables failed");
            return false;
        }
        if (m.edge_num != 0 && m.edge_num != E) {
            LEGION_ARG_ERROR("Server_Initialize: edge count of the meta line differs from the synth: generator's");
            return false;
        }
        m.edge_num = E;
        log_out() << "Graph generated in HBM: " << E << " edges\n";
    }
    const int64_t first[kModes] = {0, spec.n_train, (int64_t)spec.n_train + spec.n_valid};   // the generator's train / valid / test ranges
    for (int mode = 0; mode < kModes; mode++) {
        lists.ids[mode].resize(m.set_num[mode]);
        for (int32_t i = 0; i < m.set_num[mode]; i++) lists.ids[mode][i] = legion_synth_seed_id_host(first[mode] + i, m.node_num, spec.M2, spec.C2);
    }
    return true;
}

// Load_Graph / Load_Feature (GPUGraphStore.cu:254-325): the tables into pinned, device-mapped host memory, then the seed lists, the labels
// and the optional partition_<G>_bn
bool load_files(Server* s, SeedLists& lists)
{
    static const char* const kSetFile[kModes] = {"trainingset", "validationset", "testingset"};
    const Meta& m = s->meta;
    const int32_t V = m.node_num, F = m.float_attr_len;
    log_out() << "Start load graph\n";
    s->indptr = (int64_t*)host_alloc_space64(((int64_t)V + 1) * 8);
    s->indices = (int32_t*)host_alloc_space64(m.edge_num * 4);
    bool ok = read_file(m.dataset_path + "edge_src", s->indptr, ((int64_t)V + 1) * 8);
    ok = read_file(m.dataset_path + "edge_dst", s->indices, m.edge_num * 4) && ok;
    log_out() << "start load node\n";
    s->feats = (float*)host_alloc_space64((int64_t)V * F * 4);
    ok = read_file(m.dataset_path + "features", s->feats, (int64_t)V * F * 4) && ok;
    lists.labels.resize(V); lists.partition.resize(V);
    for (int mode = 0; mode < kModes; mode++) {
        lists.ids[mode].resize(m.set_num[mode]);
        ok = read_file(m.dataset_path + kSetFile[mode], lists.ids[mode].data(), (int64_t)m.set_num[mode] * 4) && ok;
    }
    ok = read_file(m.dataset_path + "labels", lists.labels.data(), (int64_t)V * 4) && ok;
    // the reference only prints "cannout open file" and carries on with garbage (GPUGraphStore.cu:33-35); fail instead
    if (!ok) { LEGION_ARG_ERROR("Server_Initialize: dataset file(s) missing"); return false; }
    lists.have_part = read_file(m.dataset_path + "partition_" + std::to_string(s->shard_count) + "_bn", lists.partition.data(), (int64_t)V * 4, nullptr, true);
    return true;
}

// synth: source + flag 2: the per-GPU link-prediction lists are GENERATED (legion_synth_lp_seeds, the rule of synth.lp_trainingset): one
// triple per training id in list order, dealt by src % G with its GLOBAL number, every batch laid out as [src | pos | neg] thirds.
bool generate_lp_lists(const Server* s, const std::vector<int32_t>& training_ids, std::vector<std::vector<int32_t>>& out)
{
    const Meta& m = s->meta;
    const int G = s->shard_count;
    DeviceGuard guard(0);
    for (int g = 0; g < G; g++) {
        std::vector<int32_t> srcs;
        std::vector<int64_t> tno;
        for (int64_t t = 0; t < (int64_t)training_ids.size(); t++)
            if (training_ids[t] % G == g) { srcs.push_back(training_ids[t]); tno.push_back(t); }
        const int64_t n = (int64_t)srcs.size(), k = m.raw_batch_size / 3;
        const int64_t n_out = (n + k - 1) / k * m.raw_batch_size;
        out[g].assign((size_t)n_out, 0);
        if (n == 0) continue;
        int32_t *d_src = nullptr, *d_out = nullptr;
        int64_t* d_tno = nullptr;
        HIP_CHECK(hipMalloc(&d_src, (size_t)n * 4)); HIP_CHECK(hipMalloc(&d_tno, (size_t)n * 8)); HIP_CHECK(hipMalloc(&d_out, (size_t)n_out * 4));
        if (!d_src || !d_tno || !d_out) return false;
        HIP_CHECK(hipMemcpy(d_src, srcs.data(), (size_t)n * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(d_tno, tno.data(), (size_t)n * 8, hipMemcpyHostToDevice));
        legion_synth_lp_seeds(nullptr, d_out, d_src, d_tno, n, m.raw_batch_size, s->indptr, s->indices, m.node_num, 1);
        HIP_CHECK(hipMemcpy(out[g].data(), d_out, (size_t)n_out * 4, hipMemcpyDeviceToHost));
        (void)hipFree(d_src); (void)hipFree(d_tno); (void)hipFree(d_out);
    }
    if (error_pending()) return false;
    log_out() << "Link-prediction seed lists generated: " << out[0].size() << " seeds on GPU 0\n";
    return true;
}

// Pre-partitioned training lists (extension, not in the reference): meta flag 2 = GPU g serves the file
// trainingset_<G>_<g> verbatim.  Needed for link prediction on G > 1 GPUs: lp_sage.py:87-90 expects every
// batch as [src | pos | neg] thirds, which neither split rule below preserves (synth.lp_trainingset writes them).
bool read_lp_lists(const Meta& m, int G, std::vector<std::vector<int32_t>>& out)
{
    bool ok = true;
    for (int g = 0; g < G && ok; g++) {
        const std::string path = m.dataset_path + "trainingset_" + std::to_string(G) + "_" + std::to_string(g);
        struct stat st;
        if (stat(path.c_str(), &st) != 0) { log_out() << "cannout open file: " << path << "\n"; ok = false; break; }
        out[g].resize((size_t)st.st_size / 4);
        ok = read_file(path, out[g].data(), (int64_t)out[g].size() * 4);
        for (int32_t tid : out[g]) if (tid < 0 || tid >= m.node_num) ok = false;
    }
    if (!ok) LEGION_ARG_ERROR("Server_Initialize: pre-partitioned training lists (meta flag 2) missing or out of range");
    return ok;
}

// flags 0 / 1: training id t to partition t % G, or (flag 1) to partition_<G>_bn[t] when that file exists
bool split_training(const Meta& m, const SeedLists& lists, int G, std::vector<std::vector<int32_t>>& out)
{
    for (int32_t tid : lists.ids[LEGION_TRAINMODE]) {
        if (tid < 0 || tid >= m.node_num) { LEGION_ARG_ERROR("Server_Initialize: training id outside [0, V)"); return false; }
        int32_t part = (lists.have_part && m.partition == 1) ? lists.partition[tid] : tid % G;
        if (part >= 0 && part < G) out[part].push_back(tid); // the reference indexes unchecked (GPUGraphStore.cu:338-341)
    }
    return true;
}

// seed split, GPUGraphStore.cu:332-414: the training ids by the rule of the meta line's partition flag, the validation and test ids by
// id % G; then every id's label
bool split_seeds(const Server* s, const SeedLists& lists, const LegionSynthSpec& spec, SeedSplit* split)
{
    const Meta& m = s->meta;
    const int G = s->shard_count;
    for (int mode = 0; mode < kModes; mode++) split[mode].ids.assign(G, {});
    std::vector<std::vector<int32_t>>& train = split[LEGION_TRAINMODE].ids;
    const bool ok = m.partition != 2 ? split_training(m, lists, G, train)
                  : s->synth ? generate_lp_lists(s, lists.ids[LEGION_TRAINMODE], train)
                  : read_lp_lists(m, G, train);
    if (!ok) return false;
    for (int mode = LEGION_VALIDMODE; mode <= LEGION_TESTMODE; mode++)
        for (int32_t tid : lists.ids[mode]) { int32_t part = tid % G; if (part < G) split[mode].ids[part].push_back(tid); }
    for (int mode = 0; mode < kModes; mode++) {
        split[mode].labels.assign(G, {});
        for (int p = 0; p < G; p++)
            for (int32_t id : split[mode].ids[p])
                split[mode].labels[p].push_back(s->synth ? legion_synth_label_host(id, spec.classes) : lists.labels[id]);
    }
    return true;
}

// LegionBuildInfo of the boot (the split seeds, the tables where the dataset source left them) and what is built from it: the IPC
// environment's schedule and the two storages
void build_storages(Server* s, SeedSplit* split)
{
    const Meta& m = s->meta;
    const int G = s->shard_count;
    LegionBuildInfo info;
    memset(&info, 0, sizeof(info));
    info.partition_count = G;
    for (int mode = 0; mode < kModes; mode++) {
        SeedSplit& set = split[mode];
        for (int p = 0; p < G; p++) {
            set.num.push_back((int32_t)set.ids[p].size());
            set.id_ptr.push_back(set.ids[p].data());
            set.label_ptr.push_back(set.labels[p].data());
        }
        info.*kBuildInfoSeeds[mode].num = set.num.data();
        info.*kBuildInfoSeeds[mode].ids = set.id_ptr.data();
        info.*kBuildInfoSeeds[mode].labels = set.label_ptr.data();
    }
    info.total_num_nodes = m.node_num; info.float_attr_len = m.float_attr_len;
    const int32_t table_loc = s->synth ? LEGION_LOC_DEVICE : LEGION_LOC_HOST_PINNED;
    info.host_float_attrs = s->feats; info.features_location = table_loc;
    info.float_attr_pitch = s->synth ? s->synth_pitch : 0;
    info.csr_node_index = s->indptr; info.csr_dst_node_ids = s->indices; info.csr_location = table_loc;
    info.total_edge_num = m.edge_num; info.cache_edge_num = 0;
    info.epoch = m.epoch; info.raw_batch_size = m.raw_batch_size;

    s->env = NewIPCEnv(G);
    IPCEnv_Coordinate(s->env, &info);
    s->noder = NewGPUMemoryNodeStorage();
    GPUNodeStorage_Build(s->noder, &info);
    s->graph = NewGPUMemoryGraphStorage();
    GPUGraphStorage_Build(s->graph, &info);
}

// MI355X-first: 288 GB of HBM usually hold the whole dataset, so replicate the tables into every GPU's HBM
// instead of reading them over PCIe (the reference's UVA zero-copy).  $LEGION_TABLES = device | host | auto
// (default auto: replicate when CSR + features + 20 % fit into the free HBM of every GPU).
bool place_tables(Server* s, const LegionSynthSpec& spec)
{
    const Meta& m = s->meta;
    const int G = s->shard_count;
    const int32_t V = m.node_num, F = m.float_attr_len;
    const char* mode = getenv("LEGION_TABLES");
    const std::string tables = s->synth ? "synth" : (mode ? mode : "auto");
    const int64_t need = (((int64_t)V + 1) * 8 + m.edge_num * 4 + (int64_t)V * F * 4);
    bool replicate = tables == "device";
    if (tables == "auto") {
        replicate = true;
        for (int i = 0; i < G; i++) {
            DeviceGuard guard(i);
            size_t free_b = 0, total_b = 0;
            HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
            if ((double)need * 1.2 > (double)free_b) replicate = false;
        }
    }
    if (s->synth) {
        // generated in HBM on logical GPU 0; every other physical device of the job gets a copy of its own, generated in place
        // (the storages free them as replicas: device_leaders / free_replicas)
        const std::vector<int> leader = device_leaders(G);
        GPUGraphStorage* g = s->graph;
        for (int i = 1; i < G; i++) {
            if (leader[i] < 0) continue;
            if (leader[i] == 0) {                                  // shares GPU 0's tables and holds no replica
                LEGION_AUDIT_SHARE(s->indptr, i); LEGION_AUDIT_SHARE(s->indices, i); LEGION_AUDIT_SHARE(s->feats, i);
                continue;
            }
            if (leader[i] != i) {
                g->replica_indptr[i] = g->replica_indptr[leader[i]]; g->replica_indices[i] = g->replica_indices[leader[i]];
                s->noder->replica_attrs[i] = s->noder->replica_attrs[leader[i]];
                LEGION_AUDIT_SHARE(g->replica_indptr[i], i); LEGION_AUDIT_SHARE(g->replica_indices[i], i); LEGION_AUDIT_SHARE(s->noder->replica_attrs[i], i);
                continue;
            }
            DeviceGuard guard(i);
            int64_t E2 = 0;
            if (!synth_tables_here(spec, s->synth_src.skew, s->synth_pitch, &g->replica_indptr[i], &g->replica_indices[i],
                                   &s->noder->replica_attrs[i], &E2) || E2 != m.edge_num) {
                LEGION_ARG_ERROR("Server_Initialize: generating the synth: tables on a further GPU failed");
                return false;
            }
        }
        s->noder->replica_pitch = s->synth_pitch;
        // $LEGION_SYNTH_CACHE=1: build the hotness cache anyway (budget = the meta line's cache_memory), as if the generated tables were the
        // reference's host tables -- the cost model, FillUp and the cached gather / partitioned sampler through the server binary on a
        // synth: source (bench.py's `cached_gather.served`, tests).  Default: everything is already HBM resident, a cache has nothing to add.
        { const char* e = getenv("LEGION_SYNTH_CACHE"); s->replicated = !(e && e[0] == '1'); }
        log_out() << "Tables generated in HBM: " << need / 1e9 << " GB per GPU" << (s->replicated ? "" : " (cache built on top: LEGION_SYNTH_CACHE=1)") << "\n";
    } else if (replicate) {
        GPUGraphStorage_ReplicateToDevices(s->graph);
        GPUNodeStorage_ReplicateToDevices(s->noder);
        s->replicated = true;
        log_out() << "Tables replicated into HBM: " << need / 1e9 << " GB per GPU\n";
    } else {
        log_out() << "Tables stay in pinned host memory (" << need / 1e9 << " GB)\n";
    }
    return true;
}

// LEGION_SAMPLING=weighted: the graph's edge weights -- `edge_weights` (float32[E], one per entry of edge_dst) beside the dataset's files,
// generated on the device for a synth: source -- become the graph's alias table on every GPU of the job (GPUGraphStorage_SetEdgeWeights).
// retain (LEGION_WEIGHTED_DISTINCT=1, LEGION_EDGE_WEIGHTS=1): the weights themselves stay on every GPU beside the table (GPUGraphStorage_RetainEdgeWeights).
// LEGION_EDGE_WEIGHTS=1 takes this path under every sampling kind: under a kind that is not weighted the 8 E-byte table is built and never read.
// who: the setting that asked, for the refusal and the log
bool load_edge_weights(Server* s, bool retain, const char* who)
{
    const Meta& m = s->meta;
    const int64_t E = m.edge_num;
    if (GPUGraphStorage_RetainEdgeWeights(s->graph, retain ? 1 : 0) != 0) return false;
    if (s->synth) {
        DeviceGuard guard(0);
        float* d_w = nullptr;
        HIP_CHECK(hipMalloc(&d_w, (size_t)std::max<int64_t>(E, 1) * sizeof(float)));
        if (!d_w) return false;
        legion_synth_edge_weights(nullptr, d_w, 0, E);
        HIP_CHECK(hipDeviceSynchronize());
        const int rc = GPUGraphStorage_SetEdgeWeights(s->graph, d_w, LEGION_LOC_DEVICE);
        (void)hipFree(d_w);
        if (rc != 0) return false;
    } else {
        std::vector<float> w((size_t)std::max<int64_t>(E, 1));
        int64_t got = 0;
        const std::string path = m.dataset_path + "edge_weights";
        if (!read_file(path, w.data(), E * 4, &got) || got != E * 4) {
            LEGION_ARG_ERROR((std::string("Server_Initialize: ") + who + " needs " + path + ": float32[" + std::to_string(E) + "], one weight per entry of edge_dst (missing or short)").c_str());
            return false;
        }
        if (GPUGraphStorage_SetEdgeWeights(s->graph, w.data(), LEGION_LOC_HOST_PAGEABLE) != 0) return false;
    }
    log_out() << "Edge weights: alias table built in HBM, " << E * 8 / 1e9 << " GB per GPU\n";
    if (retain) log_out() << "Edge weights: kept in HBM beside the table, " << E * 4 / 1e9 << " GB per GPU (" << (strcmp(who, "LEGION_EDGE_WEIGHTS=1") == 0 ? who : "LEGION_WEIGHTED_DISTINCT=1") << ")\n";
    return true;
}

// the cache, then one runner per GPU (GPUServer::Initialize, Server.cu:70-81)
void start_runners(Server* s)
{
    const int G = s->shard_count;
    s->cache = NewGPUCache();
    const int32_t train_step = IPCEnv_GetTrainStep(s->env);
    GPUCache_Initialize(s->cache, s->meta.cache_memory, 0, s->meta.float_attr_len, train_step, G);
    log_out() << "Storage Initialized\n";
    s->train_step = train_step;
    s->max_step = IPCEnv_GetMaxStep(s->env);
    s->runners.resize(G);
    s->params.resize(G);
    for (int i = 0; i < G; i++) {
        RunnerParams* p = new RunnerParams();
        p->device_id = i;
        p->fanout = s->fanout.data();
        p->hops = (int32_t)s->fanout.size();
        p->cache = s->cache; p->graph = s->graph; p->noder = s->noder; p->env = s->env;
        p->global_batch_id = 0;
        p->in_memory = 1;
        s->params[i] = p;
        s->runners[i] = NewGPURunner();
        runner_set_lists_verbatim(s->runners[i], s->meta.partition == 2);
        Runner_Initialize(s->runners[i], p);
    }
}

} // namespace

extern "C" {

Server* NewGPUServer(void) { return new Server(); }
void Server_SetFanout(Server* s, const int32_t* fanout, int32_t hops)
{
    if (!s || !fanout || hops < 1 || hops > LEGION_MAX_HOPS) { LEGION_ARG_ERROR("Server_SetFanout: bad arguments"); return; }
    s->fanout.assign(fanout, fanout + hops);
}
void Server_SetMetaConfigPath(Server* s, const char* path) { if (s && path) s->meta_path = path; }

// GPUServer::Initialize (Server.cu:45-81) + GPUGraphStore::Initialze (GPUGraphStore.cu:429-470)
void Server_Initialize(Server* s, int global_shard_count)
{
    if (!s || global_shard_count < 1 || global_shard_count > kMaxParts) { LEGION_ARG_ERROR("Server_Initialize: shard count must be 1..8"); return; }
    s->shard_count = global_shard_count;
    log_out() << "HIP Device Count: " << global_shard_count << "\n";
    const std::string refused = read_meta(s->meta_path, s->meta);
    if (!refused.empty()) { LEGION_ARG_ERROR(refused.c_str()); return; }
    ServeModes modes;   // checked before any device is touched; every runner parses them for itself
    std::string why;
    if (!serve_modes_from_env(modes, why) || !serve_modes_fit_fanout(modes, s->fanout.data(), (int32_t)s->fanout.size(), why) ||
        !serve_modes_resolve_lp_draw(modes, s->meta.partition == 2, s->meta.raw_batch_size, why)) { LEGION_ARG_ERROR(("Server_Initialize: " + why).c_str()); return; }
    const Meta& m = s->meta;
    // from the first device call on the main thread works on GPU 0 unless a scope below says otherwise (the reference's main thread never
    // leaves device 0); not before the meta line and the synth: source are validated -- a refused configuration touches no device
    std::optional<DeviceGuard> boot;
    LegionSynthSpec spec{};
    SeedLists lists;
    if (parse_synth(m.dataset_path, s->synth_src)) {
        if (!load_synth(s, spec, lists)) return;
        boot.emplace(0);
        if (m.partition == 2 && m.raw_batch_size % 3 != 0) {
            LEGION_ARG_ERROR("Server_Initialize: synth: link-prediction lists (meta flag 2) need a batch size divisible by 3 ([src | pos | neg] thirds, lp_sage.py:87-90)");
            return;
        }
    } else {
        boot.emplace(0);
        if (!load_files(s, lists)) return;
    }
    log_out() << "Finish Reading All Files\n";
    SeedSplit split[kModes];
    if (!split_seeds(s, lists, spec, split)) return;
    log_out() << "Finish Partition\n";
    build_storages(s, split);
    if (!place_tables(s, spec)) return;
    if ((modes.sampling == kSamplingWeighted || modes.edge_weights) && !load_edge_weights(s, serve_modes_retain_weights(modes), modes.sampling == kSamplingWeighted ? "LEGION_SAMPLING=weighted" : "LEGION_EDGE_WEIGHTS=1")) return;
    start_runners(s);
}

// PreSc, Server.cu:83-114
void Server_PreSc(Server* s, int cache_agg_mode)
{
    DeviceGuard boot(0);
    auto t1 = std::chrono::steady_clock::now();
    std::vector<std::thread> pool;
    for (int i = 0; i < s->shard_count; i++)
        pool.emplace_back([s, i]() { // PreSCLoop, Server.cu:28-34
            for (int b = 0; b < s->train_step; b++) {
                s->params[i]->global_batch_id = b;
                Runner_RunPreSc(s->runners[i], s->params[i]);
            }
            Runner_InitializeFeaturesBuffer(s->runners[i], s->params[i]);
        });
    for (auto& th : pool) th.join();
    double t = std::chrono::duration_cast<std::chrono::duration<double>>(std::chrono::steady_clock::now() - t1).count();
    GPUCache_CandidateSelection(s->cache, cache_agg_mode, s->noder, s->graph);
    // everything already sits in each GPU's HBM: caching would only add an id -> slot indirection (option c)
    if (s->replicated) GPUCache_SetCapacity(s->cache, 0, 0);
    GPUCache_CostModel(s->cache, cache_agg_mode, s->noder, s->graph, nullptr, s->train_step);
    GPUCache_FillUp(s->cache, cache_agg_mode, s->noder, s->graph);
    log_out() << "First epoch cost: " << t << " s\n";
    log_out() << "System is ready for serving\n" << std::flush;
}

// Run, Server.cu:116-135
void Server_Run(Server* s)
{
    std::vector<std::thread> pool;
    for (int i = 0; i < s->shard_count; i++)
        pool.emplace_back([s, i]() { // RunnerLoop, Server.cu:36-41
            for (int b = 0; b < s->max_step; b++) {
                s->params[i]->global_batch_id = b;
                Runner_RunOnce(s->runners[i], s->params[i]);
            }
        });
    for (auto& th : pool) th.join();
}

// Finalize, Server.cu:137-146
void Server_Finalize(Server* s)
{
    DeviceGuard boot(0);
    for (int i = 0; i < s->shard_count; i++) {
        int64_t st[3];
        legion_peer_exchange_stats(Runner_GetMemoryPool(s->runners[i]), st);     // $LEGION_PEER_GATHER=exchange: what the bulk-copy gather did
        if (st[0] > 0) log_out() << i << " peer exchange gather: " << st[0] << " batches, " << st[1] << " rows over hipMemcpyPeerAsync, " << st[2] << " host syncs\n";
        Runner_Finalize(s->runners[i], s->params[i]);
    }
    GPUGraphStorage_Finalize(s->graph);
    GPUNodeStorage_Finalize(s->noder);
    IPCEnv_Finalize(s->env);
    log_out() << std::flush;
    (void)legion_audit_report();     // $LEGION_DEVICE_AUDIT=1: what the logical-device audit saw (server_main exits non-zero on a violation)
    log_out() << "Server Stopped\n";
}

void Server_Delete(Server* s)
{
    if (!s) return;
    DeviceGuard boot(0);
    for (auto r : s->runners) Runner_Delete(r);
    for (auto p : s->params) delete p;
    if (s->cache) GPUCache_Delete(s->cache);
    if (s->graph) GPUGraphStorage_Delete(s->graph);
    if (s->noder) GPUNodeStorage_Delete(s->noder);
    if (s->synth) {
        DeviceGuard guard(0);
        (void)hipFree(s->indptr); (void)hipFree(s->indices); (void)hipFree(s->feats);
    } else {
        if (s->indptr) host_free_space(s->indptr);
        if (s->indices) host_free_space(s->indices);
        if (s->feats) host_free_space(s->feats);
    }
    delete s;
}

} // extern "C"
