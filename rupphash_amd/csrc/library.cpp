// library.cpp -- rph_library: a grouped set of files that stays on the device (include/rupphash.h).  What rph_group_files_pdq_append
// moves, expands and re-unions on every call -- the library's hashes, its variants, its flags and its components -- is kept in HBM
// between calls: an append uploads the new files only, sweeps the pairs they add and unites the edges where the sweep left them
// (components.hip); a query sweeps without changing anything; a removal compacts the survivors into a second set of arrays and regroups
// the components that lost a file (library_kernels.hip).  A library made by rph_library_create_tree also keeps the edges its appends find,
// swept at its `top`, in global numbering (library_edges.hip): rph_library_merge_tree then needs no sweep up to that top.
#include <algorithm>
#include <cstring>
#include <vector>

#include "rph_internal.h"

struct rph_library {
    rph_ctx *ctx = nullptr;
    uint32_t similarity = 0;
    std::mutex mu;  // one call at a time
    // resident, `cap` files of room each: hashes [32], variants [8][32] (always 8 rows; files without features repeat their hash and
    // carry has_features 0, which keeps them to variant 0 on the row side), low-confidence and has_features flags, min-labels
    DevBuf d_h, d_var, d_lc, d_hf, d_lab;
    uint64_t n = 0, cap = 0, want_cap = 1024, comparisons = 0;
    // per call, kept: coefficient staging (GroupSide::upload's pieces), the edge list and its cursor, a query's hashes and flags
    DevBuf d_stage, d_edges, d_cnt, d_qh, d_qlc;
    std::vector<uint8_t> low_host;
    // rph_debug_library_stages: events around the stages of the last append (created on the first request)
    bool profile = false, staged = false;  // armed; an append has recorded all six since
    hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    // rph_library_remove: the uploaded indices; flags, index lists and hipCUB workspace; the gathered rows of the components that lost a
    // file.  What the last removal did (rph_debug_library_remove_stats) and the events around its stages, armed with the append's
    DevBuf d_rm_idx, d_rm_work, d_rm_rows;
    rph_group_lists_dev group_lists;  // rph_library_group_max_dist: the caller's group arrays and its outputs
    DevBuf d_near_idx, d_near_out;    // rph_library_nearest*: the query files' indices; the slots and, behind them, the counts
    uint64_t rm_stats[3] = {0, 0, 0};  // members regrouped, edges found among them, first edge capacity tried
    DevBuf d_tree;                     // rph_library_merge_tree: into, level and edges_at before they go to the host
    uint64_t tree_stats[2] = {0, 0};   // edges its sweep found, first edge capacity it tried
    bool rm_staged = false;
    hipEvent_t rm_ev[7] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    // rph_library_create_tree: every edge the variant sweep at `top` reports among the resident files, in the library's numbering, i < j,
    // order unspecified; n_store of them, room for store_cap, never more than max_edges.  d_united: the edges of one append within
    // `similarity`, for the union-find; d_store_nums: the store kernels' counters.  edge_stats: rph_debug_library_edge_stats
    bool keeps_edges = false;
    uint32_t top = 0;
    uint64_t max_edges = 0, n_store = 0, store_cap = 0, store_first_cap = 0;
    DevBuf d_store, d_united, d_store_nums;
    uint64_t edge_stats[5] = {0, 0, 0, 0, 0};
};

namespace {
constexpr uint64_t MAX_FILES = 0x7FFFFFFFull;  // the export's hipCUB calls count in int
constexpr uint64_t COEFF_STEP = 1u << 18;      // 256 MiB of coefficients per piece

int fail(const char *who, const char *what)
{
    rph_set_error("%s: %s", who, what);
    return RPH_ERR_INVALID_ARG;
}

// room for `need` files: geometric growth, device-to-device copy of the resident part, old buffers freed once the stream is through
// with them.  The new buffers are all allocated before anything is replaced: a failure leaves the library as it was.
int grow(rph_library *lib, uint64_t need, hipStream_t s)
{
    if (need <= lib->cap) return RPH_OK;
    uint64_t cap = std::max<uint64_t>(lib->want_cap, 1024);
    while (cap < need) cap *= 2;
    cap = std::min(cap, MAX_FILES);
    DevBuf *cur[5] = {&lib->d_h, &lib->d_var, &lib->d_lc, &lib->d_hf, &lib->d_lab};
    const size_t width[5] = {32, 256, 1, 1, 4};
    DevBuf next[5];
    for (int k = 0; k < 5; k++) RPH_TRY(next[k].alloc(cap * width[k]));
    for (int k = 0; k < 5 && lib->n; k++) RPH_HIP_CHECK(hipMemcpyAsync(next[k].data(), cur[k]->data(), lib->n * width[k], hipMemcpyDeviceToDevice, s));
    RPH_HIP_CHECK(hipStreamSynchronize(s));
    for (int k = 0; k < 5; k++) *cur[k] = std::move(next[k]);
    lib->cap = cap;
    return RPH_OK;
}

// `count` files behind the resident ones (which are not touched and whose number does not change): hashes, flags and variants
int upload_behind(rph_library *lib, const uint8_t *hashes32, const float *coeffs, const uint8_t *hf, const int32_t *quality, uint64_t count, hipStream_t s)
{
    const uint64_t at = lib->n;
    RPH_HIP_CHECK(hipMemcpyAsync(lib->d_h.data() + at * 32, hashes32, count * 32, hipMemcpyHostToDevice, s));
    if (quality) {
        lib->low_host.resize(count);
        for (uint64_t i = 0; i < count; i++) lib->low_host[i] = (uint8_t)rph_is_low_pdq_quality(quality[i]);
        RPH_HIP_CHECK(hipMemcpyAsync(lib->d_lc.data() + at, lib->low_host.data(), count, hipMemcpyHostToDevice, s));
    } else {
        RPH_HIP_CHECK(hipMemsetAsync(lib->d_lc.data() + at, 0, count, s));
    }
    if (coeffs && hf)
        RPH_HIP_CHECK(hipMemcpyAsync(lib->d_hf.data() + at, hf, count, hipMemcpyHostToDevice, s));
    else
        RPH_HIP_CHECK(hipMemsetAsync(lib->d_hf.data() + at, coeffs ? 1 : 0, count, s));
    if (coeffs) {
        RPH_TRY(lib->d_stage.reserve(std::min(COEFF_STEP, count) * 1024, s));
        for (uint64_t first = 0; first < count; first += COEFF_STEP) {
            const uint32_t m = (uint32_t)std::min(COEFF_STEP, count - first);
            RPH_HIP_CHECK(hipMemcpyAsync(lib->d_stage.data(), coeffs + first * 256, (size_t)m * 1024, hipMemcpyHostToDevice, s));
            RPH_TRY(rph_launch_pdq_from_coeffs((const float *)lib->d_stage.data(), m, nullptr, lib->d_var.data() + (at + first) * 256, s));
        }
    }
    // files without features (all of them when there are no coefficients): every row is the hash
    if (!coeffs || hf) RPH_TRY(rph_launch_featureless_variants(lib->d_h.data() + at * 32, lib->d_hf.data() + at, count, lib->d_var.data() + at * 256, s));
    return RPH_OK;
}

constexpr uint64_t STORE_FIRST_CAP = 1u << 20;     // 12 MiB: where a store starts (rph_debug_library_edge_store overrides it)
constexpr uint64_t STORE_MAX_EDGES = 1ull << 28;  // max_edges == 0: 3 GiB

// room for `need` edges in the store: geometric growth, device-to-device copy of the edges it holds.  The new buffer is allocated before
// anything is replaced: a failure leaves a valid store of the old length.  More than max_edges: RPH_ERR_CAPACITY, nothing changed.
int grow_store(rph_library *lib, uint64_t need, hipStream_t s)
{
    if (need > lib->max_edges) {
        rph_set_error("rph_library: the edge store would hold %llu edges, max_edges is %llu", (unsigned long long)need, (unsigned long long)lib->max_edges);
        return RPH_ERR_CAPACITY;
    }
    if (need <= lib->store_cap) return RPH_OK;
    uint64_t cap = std::max<uint64_t>(lib->store_first_cap ? lib->store_first_cap : STORE_FIRST_CAP, 1);
    while (cap < need) cap *= 2;
    cap = std::min(cap, lib->max_edges);
    DevBuf next;
    RPH_TRY(next.alloc(cap * sizeof(rph_edge)));
    if (lib->n_store) RPH_HIP_CHECK(hipMemcpyAsync(next.data(), lib->d_store.data(), lib->n_store * sizeof(rph_edge), hipMemcpyDeviceToDevice, s));
    RPH_HIP_CHECK(hipStreamSynchronize(s));
    lib->edge_stats[0] += lib->store_cap != 0;  // (the first allocation is no growth)
    lib->d_store = std::move(next);
    lib->store_cap = cap;
    return RPH_OK;
}

// What d_edges holds -- n_cross edges (resident file, new-local file), then (new-local, new-local) ones, over n resident and n_new new
// files -- behind the store's end in the library's numbering and, within the similarity, into d_united (*united_out of them).  The
// store's length does not advance: that is the caller's commit.  It waits for the stream.
int stage_edges(rph_library *lib, uint64_t n_found, uint64_t n_cross, uint64_t n, uint64_t n_new, hipStream_t s, unsigned long long *united_out)
{
    RPH_TRY(grow_store(lib, lib->n_store + n_found, s));
    RPH_TRY(lib->d_united.reserve(n_found * sizeof(rph_edge), s));
    if (!lib->d_store_nums.data()) RPH_TRY(lib->d_store_nums.alloc(32));
    unsigned long long nums[2] = {0, 0};
    StreamDrain drain{s};
    RPH_TRY(rph_library_launch_store_append(lib->ctx, lib->d_edges.as<rph_edge>(), n_found, n_cross, (uint32_t)n, (uint32_t)n_new, lib->similarity, lib->top,
                                            lib->d_store.as<rph_edge>() + lib->n_store, lib->d_united.as<rph_edge>(), lib->d_store_nums.as<unsigned long long>(), s));
    RPH_HIP_CHECK(hipMemcpyAsync(nums, lib->d_store_nums.data(), 16, hipMemcpyDeviceToHost, s));
    RPH_HIP_CHECK(hipStreamSynchronize(s));
    if (nums[1] || nums[0] > n_found) {
        rph_set_error("rph_library: an edge for the store names a file outside its set, is not i < j or lies above top");
        return RPH_ERR_INVALID_ARG;
    }
    *united_out = nums[0];
    return RPH_OK;
}

int mark(rph_library *lib, int k, hipStream_t s)
{
    if (lib->profile) RPH_HIP_CHECK(hipEventRecord(lib->ev[k], s));
    return RPH_OK;
}

// the two requests of rph_group_files_pdq_append: the resident files' variants against the new hashes (every pair), and the new files'
// variants against their own hashes (i < j, indices local to the new set)
rph_sweep sweep_of(const rph_library *lib, uint64_t row_first, uint64_t n_rows, uint64_t col_first, uint64_t n_cols, bool cross)
{
    rph_sweep q;
    q.rows = lib->d_var.data() + row_first * 256, q.n_variants = 8, q.n = n_rows;
    q.low_conf = lib->d_lc.data() + row_first, q.has_features = lib->d_hf.data() + row_first;
    q.cols = lib->d_h.data() + col_first * 32;
    q.threshold = lib->similarity;
    if (cross) q.cross = true, q.low_conf_cols = lib->d_lc.data() + col_first, q.n_cols = n_cols;
    return q;
}

int append(rph_library *lib, const uint8_t *hashes32, const float *coeffs, const uint8_t *hf, const int32_t *quality, uint64_t n_new, uint32_t *labels_out,
           uint64_t *new_comparisons_out)
{
    rph_ctx *ctx = lib->ctx;
    hipStream_t s = ctx->stream;
    const uint64_t n = lib->n;
    RPH_TRY(mark(lib, 0, s));
    RPH_TRY(grow(lib, n + n_new, s));
    RPH_TRY(upload_behind(lib, hashes32, coeffs, hf, quality, n_new, s));
    RPH_TRY(mark(lib, 1, s));
    rph_sweep cross = sweep_of(lib, 0, n, n, n_new, true), within = sweep_of(lib, n, n_new, n, n_new, false);
    if (lib->keeps_edges) cross.threshold = within.threshold = lib->top;  // the store's edges; the unions below take those within `similarity`
    if (!lib->d_cnt.data()) RPH_TRY(lib->d_cnt.alloc(8));
    uint64_t cap = std::max<uint64_t>(1u << 20, 32 * n_new);
    unsigned long long found[2] = {0, 0};  // behind the cross sweep, behind both
    std::vector<uint32_t> own(n_new);
    StreamDrain drain{s};
    for (int attempt = 0;; attempt++) {
        if (attempt == RPH_GROW_GROUP_FILES.attempts) {
            rph_set_error("rph_library_append: edge list kept growing (%llu)", found[1]);
            return RPH_ERR_CAPACITY;
        }
        RPH_TRY(lib->d_edges.reserve(cap * sizeof(rph_edge), s));
        cap = lib->d_edges.capacity() / sizeof(rph_edge);
        RPH_HIP_CHECK(hipMemsetAsync(lib->d_cnt.data(), 0, 8, s));
        cross.edges = within.edges = lib->d_edges.as<rph_edge>();
        cross.cap = within.cap = cap;
        cross.count = within.count = lib->d_cnt.as<unsigned long long>();
        RPH_TRY(rph_launch_hamming_sweep(ctx, cross, s, ctx->hamming_kernel));
        RPH_HIP_CHECK(hipMemcpyAsync(&found[0], lib->d_cnt.data(), 8, hipMemcpyDeviceToHost, s));
        RPH_TRY(mark(lib, 2, s));
        RPH_TRY(rph_launch_hamming_sweep(ctx, within, s, ctx->hamming_kernel));  // appends behind the cross edges: one cursor
        RPH_TRY(mark(lib, 3, s));
        RPH_HIP_CHECK(hipMemcpyAsync(&found[1], lib->d_cnt.data(), 8, hipMemcpyDeviceToHost, s));  // only the cursor comes back
        RPH_HIP_CHECK(hipStreamSynchronize(s));
        if (found[1] <= cap) break;
        cap = RPH_GROW_GROUP_FILES.next_cap(found[1]);
    }
    // The new files start as components of their own (behind the size: not part of the library yet).  Then the edges where the sweeps
    // left them, the cross edges (library index, new-local index) and the inner ones (both new-local): one range check, which is the last
    // thing that can refuse, two union launches, one flatten.  From the first union launch the resident labels change; what can still
    // fail after it is a HIP call, that is a device that is lost to this context anyway.
    // An edge-keeping library first writes all of them behind its store's end, rebased to the library's numbering, and unites the copy
    // of those within `similarity`; a store that cannot take them (max_edges, an allocation) refuses here, before any label changes.
    const rph_edge *e = lib->d_edges.as<rph_edge>();
    uint32_t *lab = lib->d_lab.as<uint32_t>();
    unsigned long long united = found[1];
    if (lib->keeps_edges) RPH_TRY(stage_edges(lib, found[1], found[0], n, n_new, s, &united));
    for (uint64_t i = 0; i < n_new; i++) own[i] = (uint32_t)(n + i);
    RPH_HIP_CHECK(hipMemcpyAsync(lab + n, own.data(), n_new * 4, hipMemcpyHostToDevice, s));
    RPH_HIP_CHECK(hipStreamSynchronize(s));
    const rph_union_edges sets[2] = {{e, found[0], 0, (uint32_t)n}, {e + found[0], found[1] - found[0], (uint32_t)n, (uint32_t)n}};
    const rph_union_edges kept{lib->d_united.as<rph_edge>(), united, 0, 0};
    RPH_TRY(rph_union_find_labels(ctx, lib->keeps_edges ? &kept : sets, lib->keeps_edges ? 1 : 2, lab, n + n_new, s));
    RPH_TRY(mark(lib, 4, s));
    if (labels_out) RPH_HIP_CHECK(hipMemcpyAsync(labels_out, lab + n, n_new * 4, hipMemcpyDeviceToHost, s));
    RPH_TRY(mark(lib, 5, s));
    RPH_HIP_CHECK(hipStreamSynchronize(s));
    lib->staged = lib->profile;
    lib->n = n + n_new;
    lib->comparisons += united;
    if (new_comparisons_out) *new_comparisons_out = united;
    if (lib->keeps_edges) lib->n_store += found[1], lib->edge_stats[1] = found[1], lib->edge_stats[2] = united;
    return RPH_OK;
}

// The tree of an edge-keeping library at t <= its top, without a sweep: the core over the store at `top`, then the cut of
// rph_merge_tree_truncate (rph_host_merge_tree_cut, in place) on the arrays as they arrive: the tree is the core's own, nothing to check
int merge_tree_from_store(rph_library *lib, uint32_t t, uint32_t *into, uint8_t *level, uint64_t *edges_at)
{
    rph_ctx *ctx = lib->ctx;
    hipStream_t s = ctx->stream;
    const uint64_t n = lib->n;
    const uint32_t top = lib->top;
    uint64_t at[RPH_MAX_SIMILARITY_256 + 1];  // rph_library_create_tree refuses a top above RPH_MAX_SIMILARITY_256
    if (top > RPH_MAX_SIMILARITY_256) return fail("rph_library_merge_tree", "the store's top is above 63");
    StreamDrain drain{s};
    Layout L;
    const size_t o_into = L.add(n * 4, 256), o_level = L.add(n, 256), o_at = L.add((size_t)(top + 1) * 8, 256);
    RPH_TRY(lib->d_tree.reserve(L.end(), s));
    uint8_t *d = lib->d_tree.data();
    RPH_TRY(rph_merge_tree_run(ctx, lib->d_store.as<rph_edge>(), lib->n_store, 0, 0, n, top, (uint32_t *)(d + o_into), d + o_level, (uint64_t *)(d + o_at), nullptr, s));
    RPH_HIP_CHECK(hipMemcpyAsync(into, d + o_into, n * 4, hipMemcpyDeviceToHost, s));
    RPH_HIP_CHECK(hipMemcpyAsync(level, d + o_level, n, hipMemcpyDeviceToHost, s));
    RPH_HIP_CHECK(hipMemcpyAsync(at, d + o_at, (size_t)(top + 1) * 8, hipMemcpyDeviceToHost, s));
    RPH_HIP_CHECK(hipStreamSynchronize(s));
    rph_host_merge_tree_cut(into, level, n, t, into, level);
    std::copy(at, at + t + 1, edges_at);
    lib->edge_stats[4] = 0;
    return RPH_OK;
}

// The resident files' rows against their own hashes (i < j) at `top`, whatever the library's similarity is, into the kept edge buffer
// with append()'s retry loop; then the merge tree of those edges (merge_tree.hip).  Nothing resident is written.
int merge_tree(rph_library *lib, uint32_t top, uint32_t *into, uint8_t *level, uint64_t *edges_at)
{
    rph_ctx *ctx = lib->ctx;
    hipStream_t s = ctx->stream;
    const uint64_t n = lib->n;
    rph_sweep all = sweep_of(lib, 0, n, 0, n, false);
    all.threshold = top;
    if (!lib->d_cnt.data()) RPH_TRY(lib->d_cnt.alloc(8));
    // (as in remove(): the capacity asked for is what the sweep may fill, not what the buffer happens to hold)
    uint64_t edge_cap = std::max<uint64_t>(1u << 20, 32 * n);
    const uint64_t first_cap = edge_cap;
    unsigned long long found = 0;
    StreamDrain drain{s};
    for (int attempt = 0; n > 1; attempt++) {
        if (attempt == RPH_GROW_GROUP_FILES.attempts) {
            rph_set_error("rph_library_merge_tree: edge list kept growing (%llu)", found);
            return RPH_ERR_CAPACITY;
        }
        RPH_TRY(lib->d_edges.reserve(edge_cap * sizeof(rph_edge), s));
        RPH_HIP_CHECK(hipMemsetAsync(lib->d_cnt.data(), 0, 8, s));
        all.edges = lib->d_edges.as<rph_edge>(), all.cap = edge_cap, all.count = lib->d_cnt.as<unsigned long long>();
        RPH_TRY(rph_launch_hamming_sweep(ctx, all, s, ctx->hamming_kernel));
        RPH_HIP_CHECK(hipMemcpyAsync(&found, lib->d_cnt.data(), 8, hipMemcpyDeviceToHost, s));
        RPH_HIP_CHECK(hipStreamSynchronize(s));
        if (found <= edge_cap) break;
        edge_cap = RPH_GROW_GROUP_FILES.next_cap(found);
    }
    lib->tree_stats[0] = found, lib->tree_stats[1] = first_cap;
    lib->edge_stats[4] = 1;
    Layout L;
    const size_t o_into = L.add(n * 4, 256), o_level = L.add(n, 256), o_at = L.add((size_t)(top + 1) * 8, 256);
    RPH_TRY(lib->d_tree.reserve(L.end(), s));
    uint8_t *t = lib->d_tree.data();
    RPH_TRY(rph_merge_tree_run(ctx, lib->d_edges.as<rph_edge>(), found, 0, 0, n, top, (uint32_t *)(t + o_into), t + o_level, (uint64_t *)(t + o_at), nullptr, s));
    RPH_HIP_CHECK(hipMemcpyAsync(into, t + o_into, n * 4, hipMemcpyDeviceToHost, s));
    RPH_HIP_CHECK(hipMemcpyAsync(level, t + o_level, n, hipMemcpyDeviceToHost, s));
    RPH_HIP_CHECK(hipMemcpyAsync(edges_at, t + o_at, (size_t)(top + 1) * 8, hipMemcpyDeviceToHost, s));
    RPH_HIP_CHECK(hipStreamSynchronize(s));
    return RPH_OK;
}

int mark_removal(rph_library *lib, int k, hipStream_t s)
{
    if (lib->profile) RPH_HIP_CHECK(hipEventRecord(lib->rm_ev[k], s));
    return RPH_OK;
}

// `indices` are checked (below the size, none twice) and `sorted` holds them ascending.  Three facts make this exact: an edge (i, j), i < j,
// depends on the two files and their order alone; every edge lies inside one component; a stable compaction keeps the order.  So the
// survivors' graph is the old one minus the edges of the removed files, components that lost nobody keep their labels (renumbered), and
// only the members of the others are swept again.  The new state is built beside the old one and moved in last: whatever fails before
// that, an allocation or a HIP call, leaves the library as it was.
int remove(rph_library *lib, const uint32_t *indices, const std::vector<uint32_t> &sorted, uint32_t *new_index_out, uint64_t *dropped_out)
{
    rph_ctx *ctx = lib->ctx;
    hipStream_t s = ctx->stream;
    const uint64_t n = lib->n, n_remove = sorted.size(), kept = n - n_remove;
    // every buffer whose size is known now: the resident twins at the same capacity, the indices, flags / lists / workspace
    const size_t width[5] = {32, 256, 1, 1, 4};
    DevBuf *cur[5] = {&lib->d_h, &lib->d_var, &lib->d_lc, &lib->d_hf, &lib->d_lab};
    DevBuf next[5];
    uint32_t host_nums[2] = {0, 0};  // what comes back from the device: survivors and members, edges found, edges dropped
    unsigned long long found = 0, dropped = 0;
    // an edge-keeping library: the twin of its store at the same capacity, and what the filter counted (kept, dropped within the
    // similarity, dropped, out of range)
    DevBuf store_twin;
    unsigned long long store_nums[4] = {0, 0, 0, 0};
    StreamDrain drain{s};
    for (int k = 0; k < 5; k++) RPH_TRY(next[k].alloc(lib->cap * width[k]));
    if (lib->keeps_edges) {
        RPH_TRY(store_twin.alloc(lib->store_cap * sizeof(rph_edge)));
        if (!lib->d_store_nums.data()) RPH_TRY(lib->d_store_nums.alloc(32));
    }
    size_t temp_bytes = 0;
    RPH_TRY(rph_library_select_temp_bytes(n, &temp_bytes));
    Layout L;
    const size_t o_removed = L.add(n, 256), o_touched = L.add(n, 256), o_keep = L.add(n, 256), o_regroup = L.add(n, 256), o_new = L.add(n * 4, 256),
                 o_survivors = L.add(n * 4, 256), o_members = L.add(n * 4, 256), o_nums = L.add(16, 256), o_temp = L.add(temp_bytes + 16, 256);
    RPH_TRY(lib->d_rm_work.reserve(L.end(), s));
    RPH_TRY(lib->d_rm_idx.reserve(n_remove * 4, s));
    if (!lib->d_cnt.data()) RPH_TRY(lib->d_cnt.alloc(8));
    uint8_t *w = lib->d_rm_work.data();
    uint8_t *removed = w + o_removed, *touched = w + o_touched, *keep = w + o_keep, *regroup = w + o_regroup;
    uint32_t *new_index = (uint32_t *)(w + o_new), *survivors = (uint32_t *)(w + o_survivors), *members = (uint32_t *)(w + o_members);
    uint32_t *nums = (uint32_t *)(w + o_nums);  // survivors, members; behind them the dropped edges (8 bytes)
    unsigned long long *d_dropped = (unsigned long long *)(w + o_nums + 8);
    const uint32_t *lab = lib->d_lab.as<uint32_t>();

    RPH_TRY(mark_removal(lib, 0, s));
    RPH_HIP_CHECK(hipMemcpyAsync(lib->d_rm_idx.data(), indices, n_remove * 4, hipMemcpyHostToDevice, s));
    RPH_TRY(rph_library_launch_mark(ctx, lib->d_rm_idx.as<uint32_t>(), n_remove, lab, n, removed, touched, keep, regroup, s));
    RPH_TRY(rph_library_launch_select(keep, regroup, n, new_index, survivors, members, nums, w + o_temp, temp_bytes, s));
    RPH_HIP_CHECK(hipMemcpyAsync(host_nums, nums, 8, hipMemcpyDeviceToHost, s));
    RPH_TRY(mark_removal(lib, 1, s));
    RPH_HIP_CHECK(hipStreamSynchronize(s));
    const uint64_t m = host_nums[1];
    if (host_nums[0] != kept || m < n_remove || m > n) {
        rph_set_error("rph_library_remove: the selection kept %u files and regroups %u (%llu of %llu stay)", host_nums[0], host_nums[1], (unsigned long long)kept,
                      (unsigned long long)n);
        return RPH_ERR_HIP;
    }

    // the members of the components that lost a file, removed ones included (their edges are what the count goes down by), in order
    Layout R;
    const size_t r_h = R.add(m * 32, 256), r_var = R.add(m * 256, 256), r_lc = R.add(m, 256), r_hf = R.add(m, 256);
    RPH_TRY(lib->d_rm_rows.reserve(R.end(), s));
    uint8_t *r = lib->d_rm_rows.data();
    const rph_library_rows resident{lib->d_h.data(), lib->d_var.data(), lib->d_lc.data(), lib->d_hf.data()}, part{r + r_h, r + r_var, r + r_lc, r + r_hf},
        twin{next[0].data(), next[1].data(), next[2].data(), next[3].data()};
    RPH_TRY(rph_library_launch_gather(ctx, members, m, resident, part, s));
    RPH_TRY(mark_removal(lib, 2, s));

    // their pairs again: the triangular variant sweep, i < j among the members being i < j in the library.  The capacity asked for is what
    // the sweep may fill, not what the buffer happens to hold: which attempt succeeds then depends on this call alone.
    rph_sweep again;
    again.rows = part.variants, again.n_variants = 8, again.n = m;
    again.low_conf = part.low_conf, again.has_features = part.has_features;
    again.cols = part.hashes;
    again.threshold = lib->similarity;
    uint64_t edge_cap = std::max<uint64_t>(1u << 20, 32 * m);
    const uint64_t first_cap = edge_cap;
    for (int attempt = 0;; attempt++) {
        if (attempt == RPH_GROW_GROUP_FILES.attempts) {
            rph_set_error("rph_library_remove: edge list kept growing (%llu)", found);
            return RPH_ERR_CAPACITY;
        }
        RPH_TRY(lib->d_edges.reserve(edge_cap * sizeof(rph_edge), s));
        RPH_HIP_CHECK(hipMemsetAsync(lib->d_cnt.data(), 0, 8, s));
        again.edges = lib->d_edges.as<rph_edge>(), again.cap = edge_cap, again.count = lib->d_cnt.as<unsigned long long>();
        RPH_TRY(rph_launch_hamming_sweep(ctx, again, s, ctx->hamming_kernel));
        RPH_HIP_CHECK(hipMemcpyAsync(&found, lib->d_cnt.data(), 8, hipMemcpyDeviceToHost, s));
        RPH_TRY(mark_removal(lib, 3, s));
        RPH_HIP_CHECK(hipStreamSynchronize(s));
        if (found <= edge_cap) break;
        edge_cap = RPH_GROW_GROUP_FILES.next_cap(found);
    }

    // edges of removed files counted and disarmed, the rest renumbered; the survivors' rows and starting labels into the twins; the kept
    // edges united over the new labels (one range check first, then union and flatten)
    RPH_TRY(rph_library_launch_split_edges(ctx, lib->d_edges.as<rph_edge>(), found, members, removed, new_index, d_dropped, s));
    RPH_HIP_CHECK(hipMemcpyAsync(&dropped, d_dropped, 8, hipMemcpyDeviceToHost, s));
    RPH_TRY(mark_removal(lib, 4, s));
    RPH_TRY(rph_library_launch_gather(ctx, survivors, kept, resident, twin, s));
    RPH_TRY(rph_library_launch_labels(ctx, lab, removed, touched, new_index, n, next[4].as<uint32_t>(), s));
    RPH_TRY(mark_removal(lib, 5, s));
    if (kept) {
        const rph_union_edges all{lib->d_edges.as<rph_edge>(), found, 0, 0};
        RPH_TRY(rph_union_find_labels(ctx, &all, 1, next[4].as<uint32_t>(), kept, s));
    }
    RPH_TRY(mark_removal(lib, 6, s));
    // the store through the same flags and numbers into its twin.  What it drops within the similarity is what the regroup counted: both
    // are the edges of the removed files, found by two different routes
    if (lib->keeps_edges) {
        RPH_TRY(rph_library_launch_store_filter(ctx, lib->d_store.as<rph_edge>(), lib->n_store, n, removed, new_index, lib->similarity, store_twin.as<rph_edge>(),
                                                lib->d_store_nums.as<unsigned long long>(), s));
        RPH_HIP_CHECK(hipMemcpyAsync(store_nums, lib->d_store_nums.data(), 32, hipMemcpyDeviceToHost, s));
    }
    RPH_HIP_CHECK(hipStreamSynchronize(s));
    if (lib->keeps_edges && (store_nums[3] || store_nums[1] != dropped || store_nums[0] + store_nums[2] != lib->n_store)) {
        rph_set_error("rph_library_remove: the edge store drops %llu edges within the similarity (%llu of %llu in all, %llu kept), the regroup counted %llu",
                      store_nums[1], store_nums[2], (unsigned long long)lib->n_store, store_nums[0], dropped);
        return RPH_ERR_HIP;
    }

    // the swap: nothing can fail from here, and the stream is through with the old arrays
    for (int k = 0; k < 5; k++) *cur[k] = std::move(next[k]);
    if (lib->keeps_edges) {
        lib->d_store = std::move(store_twin);
        lib->n_store = store_nums[0];
        lib->edge_stats[3] = store_nums[2];
    }
    lib->n = kept;
    lib->comparisons -= std::min<uint64_t>(dropped, lib->comparisons);  // (a restored count may have been lower than the files' edges)
    lib->rm_stats[0] = m, lib->rm_stats[1] = found, lib->rm_stats[2] = first_cap;
    lib->rm_staged = lib->profile;
    if (dropped_out) *dropped_out = dropped;
    if (new_index_out) {
        uint64_t gone = 0;
        for (uint64_t x = 0; x < n; x++) {
            const bool out = gone < n_remove && sorted[gone] == x;
            gone += out;
            new_index_out[x] = out ? 0xFFFFFFFFu : (uint32_t)(x - gone);
        }
    }
    return RPH_OK;
}
}  // namespace

extern "C" {

int rph_library_create(rph_ctx *ctx, uint32_t similarity, rph_library **lib_out)
{
    return rph_guarded("rph_library_create", [&]() -> int {
        if (!ctx || !lib_out) return fail("rph_library_create", "null argument");
        *lib_out = nullptr;
        if (similarity > RPH_MAX_SIMILARITY_256) return fail("rph_library_create", "Similarity distances above 63 require R=4 bit-flip checks, which are not implemented.");
        rph_library *lib = new rph_library;
        lib->ctx = ctx;
        lib->similarity = similarity;
        *lib_out = lib;
        return RPH_OK;
    });
}

int rph_library_create_tree(rph_ctx *ctx, uint32_t similarity, uint32_t top, uint64_t max_edges, rph_library **lib_out)
{
    return rph_guarded("rph_library_create_tree", [&]() -> int {
        if (!ctx || !lib_out) return fail("rph_library_create_tree", "null argument");
        *lib_out = nullptr;
        if (top > RPH_MAX_SIMILARITY_256) return fail("rph_library_create_tree", "Similarity distances above 63 require R=4 bit-flip checks, which are not implemented.");
        if (similarity > top) return fail("rph_library_create_tree", "similarity above top: the store would lack edges the groups need");
        rph_library *lib = new rph_library;
        lib->ctx = ctx;
        lib->similarity = similarity;
        lib->keeps_edges = true;
        lib->top = top;
        lib->max_edges = max_edges ? max_edges : STORE_MAX_EDGES;
        *lib_out = lib;
        return RPH_OK;
    });
}

int rph_library_edge_info(rph_library *lib, uint32_t *top_out, uint64_t *n_edges_out, uint64_t *capacity_out)
{
    if (!lib) return fail("rph_library_edge_info", "null argument");
    std::lock_guard<std::mutex> lock(lib->mu);
    if (top_out) *top_out = lib->keeps_edges ? lib->top : RPH_NO_EDGE_STORE;
    if (n_edges_out) *n_edges_out = lib->n_store;
    if (capacity_out) *capacity_out = lib->max_edges;
    return RPH_OK;
}

int rph_library_edges(rph_library *lib, rph_edge *edges_out, uint64_t cap, uint64_t *n_edges_out)
{
    return rph_guarded("rph_library_edges", [&]() -> int {
        if (!lib || !n_edges_out || (!edges_out && cap)) return fail("rph_library_edges", "null argument");
        *n_edges_out = 0;
        std::lock_guard<std::mutex> lock(lib->mu);
        if (!lib->keeps_edges) return fail("rph_library_edges", "the library keeps no edges: make it with rph_library_create_tree");
        *n_edges_out = lib->n_store;
        if (lib->n_store > cap) {
            rph_set_error("rph_library_edges: %llu edges, capacity %llu", (unsigned long long)lib->n_store, (unsigned long long)cap);
            return RPH_ERR_CAPACITY;
        }
        if (lib->n_store == 0) return RPH_OK;
        RPH_HIP_CHECK(hipSetDevice(lib->ctx->device));
        RPH_HIP_CHECK(hipMemcpyAsync(edges_out, lib->d_store.data(), lib->n_store * sizeof(rph_edge), hipMemcpyDeviceToHost, lib->ctx->stream));
        RPH_HIP_CHECK(hipStreamSynchronize(lib->ctx->stream));
        return RPH_OK;
    });
}

int rph_library_restore_edges(rph_library *lib, const uint8_t *hashes32, const float *coeffs, const uint8_t *has_features, const int32_t *quality, uint64_t n,
                              const rph_edge *edges, uint64_t n_edges)
{
    return rph_guarded("rph_library_restore_edges", [&]() -> int {
        const char *who = "rph_library_restore_edges";
        if (!lib || (!hashes32 && n) || (!edges && n_edges)) return fail(who, "null argument");
        std::lock_guard<std::mutex> lock(lib->mu);
        if (!lib->keeps_edges) return fail(who, "the library keeps no edges: make it with rph_library_create_tree");
        if (lib->n) return fail(who, "the library is not empty");
        if (n > MAX_FILES) return fail(who, "at most 2^31 - 1 files");
        // the caller's word, checked here before anything is uploaded and again by the kernel that stores it
        for (uint64_t e = 0; e < n_edges; e++)
            if (edges[e].i >= edges[e].j || edges[e].j >= n || edges[e].d > lib->top) return fail(who, "an edge is not i < j < n with d <= top");
        if (n == 0) return RPH_OK;
        rph_ctx *ctx = lib->ctx;
        RPH_HIP_CHECK(hipSetDevice(ctx->device));
        hipStream_t s = ctx->stream;
        std::vector<uint32_t> own(n);
        for (uint64_t i = 0; i < n; i++) own[i] = (uint32_t)i;
        StreamDrain drain{s};
        RPH_TRY(grow(lib, n, s));
        RPH_TRY(upload_behind(lib, hashes32, coeffs, has_features, quality, n, s));
        RPH_TRY(lib->d_edges.reserve(n_edges * sizeof(rph_edge), s));
        if (n_edges) RPH_HIP_CHECK(hipMemcpyAsync(lib->d_edges.data(), edges, n_edges * sizeof(rph_edge), hipMemcpyHostToDevice, s));
        unsigned long long united = 0;
        RPH_TRY(stage_edges(lib, n_edges, 0, 0, n, s, &united));  // as inner edges of an append to an empty library
        RPH_HIP_CHECK(hipMemcpyAsync(lib->d_lab.data(), own.data(), n * 4, hipMemcpyHostToDevice, s));
        const rph_union_edges kept{lib->d_united.as<rph_edge>(), united, 0, 0};
        RPH_TRY(rph_union_find_labels(ctx, &kept, 1, lib->d_lab.as<uint32_t>(), n, s));
        RPH_HIP_CHECK(hipStreamSynchronize(s));
        lib->n = n;
        lib->n_store = n_edges;
        lib->comparisons = united;
        return RPH_OK;
    });
}

int rph_library_destroy(rph_library *lib)
{
    if (!lib) return RPH_ERR_INVALID_ARG;
    {
        std::lock_guard<std::mutex> lock(lib->mu);
        (void)hipSetDevice(lib->ctx->device);
        (void)hipStreamSynchronize(lib->ctx->stream);
        for (hipEvent_t e : lib->ev)
            if (e) (void)hipEventDestroy(e);
        for (hipEvent_t e : lib->rm_ev)
            if (e) (void)hipEventDestroy(e);
    }
    delete lib;
    return RPH_OK;
}

int rph_library_reserve(rph_library *lib, uint64_t n_files)
{
    return rph_guarded("rph_library_reserve", [&]() -> int {
        if (!lib) return fail("rph_library_reserve", "null argument");
        if (n_files > MAX_FILES) return fail("rph_library_reserve", "at most 2^31 - 1 files");
        std::lock_guard<std::mutex> lock(lib->mu);
        RPH_HIP_CHECK(hipSetDevice(lib->ctx->device));
        const uint64_t before = lib->want_cap;
        lib->want_cap = std::max(before, n_files);  // grow() sizes the first allocation by it
        const int rc = grow(lib, n_files, lib->ctx->stream);
        if (rc != RPH_OK) lib->want_cap = before;
        return rc;
    });
}

int rph_library_size(rph_library *lib, uint64_t *n_files_out, uint64_t *comparisons_out)
{
    if (!lib) return fail("rph_library_size", "null argument");
    std::lock_guard<std::mutex> lock(lib->mu);
    if (n_files_out) *n_files_out = lib->n;
    if (comparisons_out) *comparisons_out = lib->comparisons;
    return RPH_OK;
}

int rph_library_append(rph_library *lib, const uint8_t *hashes32, const float *coeffs, const uint8_t *has_features, const int32_t *quality, uint64_t n_new,
                       uint32_t *labels_out, uint64_t *new_comparisons_out)
{
    return rph_guarded("rph_library_append", [&]() -> int {
        if (!lib || (!hashes32 && n_new)) return fail("rph_library_append", "null argument");
        if (new_comparisons_out) *new_comparisons_out = 0;
        if (n_new == 0) return RPH_OK;
        std::lock_guard<std::mutex> lock(lib->mu);
        if (n_new > MAX_FILES || lib->n + n_new > MAX_FILES) return fail("rph_library_append", "at most 2^31 - 1 files");
        RPH_HIP_CHECK(hipSetDevice(lib->ctx->device));
        return append(lib, hashes32, coeffs, has_features, quality, n_new, labels_out, new_comparisons_out);
    });
}

int rph_library_remove(rph_library *lib, const uint32_t *indices, uint64_t n_remove, uint32_t *new_index_out, uint64_t *dropped_comparisons_out)
{
    return rph_guarded("rph_library_remove", [&]() -> int {
        if (!lib || (!indices && n_remove)) return fail("rph_library_remove", "null argument");
        std::lock_guard<std::mutex> lock(lib->mu);
        if (n_remove > lib->n) return fail("rph_library_remove", "more indices than files: one is listed twice or lies outside the library");
        std::vector<uint32_t> sorted(indices, indices + n_remove);
        std::sort(sorted.begin(), sorted.end());
        if (n_remove && sorted.back() >= lib->n) return fail("rph_library_remove", "an index is not below the size");
        if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end()) return fail("rph_library_remove", "an index is listed twice");
        if (n_remove == 0) {  // nothing changes; the map is the identity
            if (dropped_comparisons_out) *dropped_comparisons_out = 0;
            for (uint64_t x = 0; x < lib->n && new_index_out; x++) new_index_out[x] = (uint32_t)x;
            return RPH_OK;
        }
        RPH_HIP_CHECK(hipSetDevice(lib->ctx->device));
        return remove(lib, indices, sorted, new_index_out, dropped_comparisons_out);
    });
}

int rph_library_restore(rph_library *lib, const uint8_t *hashes32, const float *coeffs, const uint8_t *has_features, const int32_t *quality, uint64_t n,
                        const uint32_t *members, const uint32_t *offsets, uint32_t n_groups, uint64_t comparisons)
{
    return rph_guarded("rph_library_restore", [&]() -> int {
        if (!lib || (!hashes32 && n) || ((!members || !offsets) && n_groups)) return fail("rph_library_restore", "null argument");
        std::lock_guard<std::mutex> lock(lib->mu);
        if (lib->keeps_edges) return fail("rph_library_restore", "groups alone cannot fill an edge store: use rph_library_restore_edges");
        if (lib->n) return fail("rph_library_restore", "the library is not empty");
        if (n > MAX_FILES) return fail("rph_library_restore", "at most 2^31 - 1 files");
        // the groups through the checks of rph_union_find_groups_append (no edges); what it lists has its smallest member first
        std::vector<uint32_t> m(std::max<uint64_t>(n, 1)), o(n / 2 + 2), labels(n);
        uint32_t ng = 0;
        RPH_TRY(rph_host_union_find_append(members, offsets, n_groups, nullptr, 0, n, m.data(), o.data(), &ng));
        for (uint64_t i = 0; i < n; i++) labels[i] = (uint32_t)i;
        for (uint32_t g = 0; g < ng; g++)
            for (uint32_t t = o[g]; t < o[g + 1]; t++) labels[m[t]] = m[o[g]];
        if (n) {
            RPH_HIP_CHECK(hipSetDevice(lib->ctx->device));
            hipStream_t s = lib->ctx->stream;
            RPH_TRY(grow(lib, n, s));
            RPH_TRY(upload_behind(lib, hashes32, coeffs, has_features, quality, n, s));
            RPH_HIP_CHECK(hipMemcpyAsync(lib->d_lab.data(), labels.data(), n * 4, hipMemcpyHostToDevice, s));
            RPH_HIP_CHECK(hipStreamSynchronize(s));
        }
        lib->n = n;
        lib->comparisons = comparisons;
        return RPH_OK;
    });
}

int rph_library_groups(rph_library *lib, uint32_t *members, uint32_t *offsets, uint32_t *n_groups_out)
{
    return rph_guarded("rph_library_groups", [&]() -> int {
        if (!lib || !members || !offsets || !n_groups_out) return fail("rph_library_groups", "null argument");
        std::lock_guard<std::mutex> lock(lib->mu);
        return rph_groups_from_labels_dev(lib->ctx, lib->d_lab.data(), lib->n, members, offsets, n_groups_out, lib->ctx->stream);
    });
}

int rph_library_labels(rph_library *lib, uint64_t first, uint64_t count, uint32_t *labels_out)
{
    return rph_guarded("rph_library_labels", [&]() -> int {
        if (!lib || (!labels_out && count)) return fail("rph_library_labels", "null argument");
        std::lock_guard<std::mutex> lock(lib->mu);
        if (first > lib->n || count > lib->n - first) return fail("rph_library_labels", "first + count exceeds the size");
        if (count == 0) return RPH_OK;
        RPH_HIP_CHECK(hipSetDevice(lib->ctx->device));
        RPH_HIP_CHECK(hipMemcpyAsync(labels_out, lib->d_lab.as<uint32_t>() + first, count * 4, hipMemcpyDeviceToHost, lib->ctx->stream));
        RPH_HIP_CHECK(hipStreamSynchronize(lib->ctx->stream));
        return RPH_OK;
    });
}

int rph_library_query(rph_library *lib, const uint8_t *hashes32_q, const int32_t *quality_q, uint64_t n_q, rph_edge *edges, uint64_t cap,
                      uint64_t *n_edges_out)
{
    return rph_guarded("rph_library_query", [&]() -> int {
        if (!lib || (!hashes32_q && n_q) || !n_edges_out || (!edges && cap)) return fail("rph_library_query", "null argument");
        *n_edges_out = 0;
        if (n_q > 0xFFFFFFFFull) return fail("rph_library_query", "at most 2^32 - 1 queries");
        std::lock_guard<std::mutex> lock(lib->mu);
        if (n_q == 0 || lib->n == 0) return RPH_OK;
        rph_ctx *ctx = lib->ctx;
        RPH_HIP_CHECK(hipSetDevice(ctx->device));
        hipStream_t s = ctx->stream;
        RPH_TRY(lib->d_qh.reserve(n_q * 32, s));
        RPH_HIP_CHECK(hipMemcpyAsync(lib->d_qh.data(), hashes32_q, n_q * 32, hipMemcpyHostToDevice, s));
        rph_sweep q = sweep_of(lib, 0, lib->n, 0, n_q, true);
        q.cols = lib->d_qh.data();
        q.low_conf_cols = nullptr;
        if (quality_q) {
            lib->low_host.resize(n_q);
            for (uint64_t i = 0; i < n_q; i++) lib->low_host[i] = (uint8_t)rph_is_low_pdq_quality(quality_q[i]);
            RPH_TRY(lib->d_qlc.reserve(n_q, s));
            RPH_HIP_CHECK(hipMemcpyAsync(lib->d_qlc.data(), lib->low_host.data(), n_q, hipMemcpyHostToDevice, s));
            q.low_conf_cols = lib->d_qlc.data();
        }
        if (!lib->d_cnt.data()) RPH_TRY(lib->d_cnt.alloc(8));
        RPH_TRY(lib->d_edges.reserve(cap * sizeof(rph_edge), s));
        RPH_HIP_CHECK(hipMemsetAsync(lib->d_cnt.data(), 0, 8, s));
        q.edges = lib->d_edges.as<rph_edge>(), q.cap = cap, q.count = lib->d_cnt.as<unsigned long long>();
        RPH_TRY(rph_launch_hamming_sweep(ctx, q, s, ctx->hamming_kernel));
        unsigned long long found = 0;
        RPH_HIP_CHECK(hipMemcpyAsync(&found, lib->d_cnt.data(), 8, hipMemcpyDeviceToHost, s));
        RPH_HIP_CHECK(hipStreamSynchronize(s));
        *n_edges_out = found;
        const uint64_t n_take = std::min<uint64_t>(found, cap);
        if (n_take) RPH_HIP_CHECK(hipMemcpy(edges, lib->d_edges.data(), n_take * sizeof(rph_edge), hipMemcpyDeviceToHost));
        if (found > cap) {
            rph_set_error("rph_library_query: %llu edges found, capacity %llu", found, (unsigned long long)cap);
            return RPH_ERR_CAPACITY;
        }
        return RPH_OK;
    });
}

int rph_library_group_max_dist(rph_library *lib, const uint32_t *members, const uint32_t *offsets, uint32_t n_groups, const uint32_t *pivots,
                               uint32_t *max_dist_out, uint32_t *member_dist_out)
{
    return rph_guarded("rph_library_group_max_dist", [&]() -> int {
        if (!lib) return fail("rph_library_group_max_dist", "null argument");
        std::lock_guard<std::mutex> lock(lib->mu);
        RPH_TRY(rph_host_group_lists_check("rph_library_group_max_dist", lib->d_h.data(), lib->n, members, offsets, n_groups, pivots, max_dist_out));
        if (n_groups == 0) return RPH_OK;
        RPH_HIP_CHECK(hipSetDevice(lib->ctx->device));
        hipStream_t s = lib->ctx->stream;
        StreamDrain drain{s};
        RPH_TRY(lib->group_lists.upload(members, offsets, n_groups, pivots, member_dist_out != nullptr, s));
        // the resident rows as they are: a file without features repeats its hash in all 8, which is the plain distance
        rph_group_dist q;
        q.hashes = lib->d_h.data(), q.n = lib->n, q.rows = lib->d_var.data(), q.row_mode = RPH_ROWS_PER_FILE, q.has_features = lib->d_hf.data();
        lib->group_lists.fill(q);
        RPH_TRY(rph_group_max_dist_run(lib->ctx, q, lib->group_lists.total, s));
        return lib->group_lists.download(max_dist_out, member_dist_out, s);
    });
}

// rph_library_nearest and rph_library_nearest_files: the queries are hashes of the caller's (uploaded into d_qh) or resident files
// (their indices uploaded; the kernel gathers their hashes from d_h and skips each in its own list)
static int library_nearest(const char *who, rph_library *lib, const uint8_t *hashes32_q, const uint32_t *indices, uint64_t n_q, uint32_t k, uint32_t max_dist,
                           rph_edge *out, uint32_t *counts_out)
{
    if (!lib) return fail(who, "null argument");
    std::lock_guard<std::mutex> lock(lib->mu);
    const void *queries = indices ? (const void *)indices : (const void *)hashes32_q;
    RPH_TRY(rph_nearest_check(who, lib->d_var.data(), 8, lib->n, queries, n_q, k, out));
    for (uint64_t t = 0; t < n_q && indices; t++)
        if (indices[t] >= lib->n) return fail(who, "an index is not below the size");
    if (n_q == 0) return RPH_OK;
    rph_ctx *ctx = lib->ctx;
    RPH_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    StreamDrain drain{s};
    const size_t slot_bytes = align_up(n_q * k * sizeof(rph_edge), 256);
    RPH_TRY(lib->d_near_out.reserve(slot_bytes + n_q * 4, s));
    rph_nearest q;
    q.rows = lib->d_var.data(), q.has_features = lib->d_hf.data(), q.n_variants = 8, q.n_lib = lib->n;
    q.k = k, q.max_dist = max_dist, q.n_q = n_q;
    if (indices) {
        RPH_TRY(lib->d_near_idx.reserve(n_q * 4, s));
        RPH_HIP_CHECK(hipMemcpyAsync(lib->d_near_idx.data(), indices, n_q * 4, hipMemcpyHostToDevice, s));
        q.hashes_q = lib->d_h.data(), q.gather = lib->d_near_idx.as<uint32_t>();
    } else {
        RPH_TRY(lib->d_qh.reserve(n_q * 32, s));
        RPH_HIP_CHECK(hipMemcpyAsync(lib->d_qh.data(), hashes32_q, n_q * 32, hipMemcpyHostToDevice, s));
        q.hashes_q = lib->d_qh.data();
    }
    q.out = lib->d_near_out.as<rph_edge>(), q.counts = (uint32_t *)(lib->d_near_out.data() + slot_bytes);
    RPH_TRY(rph_nearest_run(ctx, q, s));
    RPH_HIP_CHECK(hipMemcpyAsync(out, q.out, n_q * k * sizeof(rph_edge), hipMemcpyDeviceToHost, s));
    if (counts_out) RPH_HIP_CHECK(hipMemcpyAsync(counts_out, q.counts, n_q * 4, hipMemcpyDeviceToHost, s));
    RPH_HIP_CHECK(hipStreamSynchronize(s));
    return RPH_OK;
}

int rph_library_nearest(rph_library *lib, const uint8_t *hashes32_q, uint64_t n_q, uint32_t k, uint32_t max_dist, rph_edge *out, uint32_t *counts_out)
{
    return rph_guarded("rph_library_nearest", [&]() -> int { return library_nearest("rph_library_nearest", lib, hashes32_q, nullptr, n_q, k, max_dist, out, counts_out); });
}

int rph_library_nearest_files(rph_library *lib, const uint32_t *indices, uint64_t n_q, uint32_t k, uint32_t max_dist, rph_edge *out, uint32_t *counts_out)
{
    return rph_guarded("rph_library_nearest_files", [&]() -> int {
        if (!indices && n_q) return fail("rph_library_nearest_files", "null argument");
        return library_nearest("rph_library_nearest_files", lib, nullptr, indices, n_q, k, max_dist, out, counts_out);
    });
}

int rph_library_merge_tree(rph_library *lib, uint32_t top, uint32_t *into, uint8_t *level, uint64_t *edges_at)
{
    return rph_guarded("rph_library_merge_tree", [&]() -> int {
        if (!lib || !edges_at) return fail("rph_library_merge_tree", "null argument");
        if (top > RPH_MAX_SIMILARITY_256) return fail("rph_library_merge_tree", "Similarity distances above 63 require R=4 bit-flip checks, which are not implemented.");
        std::lock_guard<std::mutex> lock(lib->mu);
        if ((!into || !level) && lib->n) return fail("rph_library_merge_tree", "null argument");
        std::fill(edges_at, edges_at + top + 1, 0);
        if (lib->n == 0) return RPH_OK;
        RPH_HIP_CHECK(hipSetDevice(lib->ctx->device));
        if (lib->keeps_edges && top <= lib->top) return merge_tree_from_store(lib, top, into, level, edges_at);
        return merge_tree(lib, top, into, level, edges_at);
    });
}

// A store allocated or grown from now on starts at first_capacity_edges and doubles from there; 0 restores the default (exported for
// the tests, not in the header)
int rph_debug_library_edge_store(rph_library *lib, uint64_t first_capacity_edges)
{
    if (!lib) return fail("rph_debug_library_edge_store", "null argument");
    std::lock_guard<std::mutex> lock(lib->mu);
    lib->store_first_cap = first_capacity_edges;
    return RPH_OK;
}

// What the edge store has done (exported for the tests, not in the header; rph_internal.h says what the five numbers are)
int rph_debug_library_edge_stats(rph_library *lib, uint64_t *out)
{
    if (!lib || !out) return fail("rph_debug_library_edge_stats", "null argument");
    std::lock_guard<std::mutex> lock(lib->mu);
    for (int k = 0; k < 5; k++) out[k] = lib->edge_stats[k];
    return RPH_OK;
}

// What the last rph_library_merge_tree did (exported for the tests, not in the header): out[0..1] = edges its sweep found, the first
// edge capacity it tried
int rph_debug_library_merge_tree_stats(rph_library *lib, uint64_t *out)
{
    if (!lib || !out) return fail("rph_debug_library_merge_tree_stats", "null argument");
    std::lock_guard<std::mutex> lock(lib->mu);
    out[0] = lib->tree_stats[0], out[1] = lib->tree_stats[1];
    return RPH_OK;
}

// The stages of the last append in device time (exported for tools/library_rate.py, not in the header): on != 0 arms the events for the
// appends that follow; ms_out (nullable, 5 floats): upload and variants of the new files, cross sweep, triangular sweep, cursor read plus
// union and flatten kernels, labels back.
int rph_debug_library_stages(rph_library *lib, int on, float *ms_out)
{
    return rph_guarded("rph_debug_library_stages", [&]() -> int {
        if (!lib) return fail("rph_debug_library_stages", "null argument");
        std::lock_guard<std::mutex> lock(lib->mu);
        RPH_HIP_CHECK(hipSetDevice(lib->ctx->device));
        if (ms_out) {
            if (!lib->staged) return fail("rph_debug_library_stages", "no append has run with the events armed");
            for (int k = 0; k < 5; k++) RPH_HIP_CHECK(hipEventElapsedTime(&ms_out[k], lib->ev[k], lib->ev[k + 1]));
        }
        for (int k = 0; k < 6 && on && !lib->ev[k]; k++) RPH_HIP_CHECK(hipEventCreate(&lib->ev[k]));
        for (int k = 0; k < 7 && on && !lib->rm_ev[k]; k++) RPH_HIP_CHECK(hipEventCreate(&lib->rm_ev[k]));
        lib->profile = on != 0;
        lib->staged = lib->rm_staged = false;
        return RPH_OK;
    });
}

// What the last removal did (exported for the tests, not in the header; rph_internal.h says what the four numbers are)
int rph_debug_library_remove_stats(rph_library *lib, uint64_t *out)
{
    if (!lib || !out) return fail("rph_debug_library_remove_stats", "null argument");
    std::lock_guard<std::mutex> lock(lib->mu);
    for (int k = 0; k < 3; k++) out[k] = lib->rm_stats[k];
    out[3] = rph_stride_lanes_per_pass(lib->ctx);
    return RPH_OK;
}

// The stages of the last removal in device time, armed by rph_debug_library_stages (exported for tools/library_remove_rate.py)
int rph_debug_library_remove_stages(rph_library *lib, float *ms_out)
{
    return rph_guarded("rph_debug_library_remove_stages", [&]() -> int {
        if (!lib || !ms_out) return fail("rph_debug_library_remove_stages", "null argument");
        std::lock_guard<std::mutex> lock(lib->mu);
        if (!lib->rm_staged) return fail("rph_debug_library_remove_stages", "no removal has run with the events armed");
        RPH_HIP_CHECK(hipSetDevice(lib->ctx->device));
        for (int k = 0; k < 6; k++) RPH_HIP_CHECK(hipEventElapsedTime(&ms_out[k], lib->rm_ev[k], lib->rm_ev[k + 1]));
        return RPH_OK;
    });
}

}  // extern "C"
