// components.hip -- the union-find of group_files_generic (scanner.rs:1781-1817) on the device: connected components
// of an edge list as min-labels, and their export in the order rph_union_find_groups lists them.
//
// parent[] is a forest in which every pointer goes to a smaller index (parent[x] <= x, a root points at itself).  The two writes that
// exist keep that: a union hooks the LARGER of two roots under the smaller, and path halving replaces a pointer by an ancestor, which is
// smaller still.  So the root of a component is its smallest member, whatever the order of the edges and of the lanes, and the
// flattened array is the same on every run.
//
// Every access to parent[] inside the union and flatten kernels is a relaxed agent-scope atomic (loads that go past the CU's L1, vector
// atomics for the writes); nothing else is shared between workgroups, so no fence is needed: the only property the walk relies on is
// that a value read from parent[x], however old, is x itself or an ancestor of x -- once an ancestor, always an ancestor.
#include <hipcub/hipcub.hpp>

#include "rph_internal.h"
#include "uf_device.h"  // uf_parent, uf_find: shared with merge_tree.hip

namespace {
// One lane per edge.  bad edges and a forest that points upwards are refused by uf_check_kernel before this one runs.
__global__ void __launch_bounds__(256) uf_union_kernel(const rph_edge *__restrict__ edges, uint64_t n_edges, uint32_t i_base, uint32_t j_base, uint32_t *parent)
{
    for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n_edges; e += (uint64_t)gridDim.x * blockDim.x) {
        uint32_t a = edges[e].i + i_base, b = edges[e].j + j_base;
        // Lock-free: the loop is left when both ends have one root or when this lane's CAS hooked one root under the other.  It is
        // repeated only when the CAS found parent[hi] != hi, that is when ANOTHER lane's CAS on hi succeeded in between; every success
        // removes a root for good and there are fewer than n roots to remove, so all lanes together repeat fewer than n times.  The
        // next round starts from the value the failed CAS returned (an ancestor of hi, smaller than hi), so this lane moves down even
        // if a load were to show it an old value.  No lane waits for a flag, a lock or a value that another lane has yet to write, and
        // none depends on which blocks are resident or in which order they are scheduled; lanes of one wave that leave the loop early
        // are simply masked off.
        for (;;) {
            a = uf_find(parent, a);
            b = uf_find(parent, b);
            if (a == b) break;
            const uint32_t hi = a > b ? a : b, lo = a > b ? b : a;
            uint32_t seen = hi;
            if (__hip_atomic_compare_exchange_strong(parent + hi, &seen, lo, __ATOMIC_RELAXED, UF_RELAXED)) break;
            a = seen;
            b = lo;
        }
    }
}

__global__ void __launch_bounds__(256) uf_flatten_kernel(uint32_t *parent, uint64_t n)
{
    for (uint64_t x = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; x < n; x += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t r = uf_find(parent, (uint32_t)x);
        if (r != (uint32_t)x) __hip_atomic_fetch_min(parent + x, r, UF_RELAXED);  // other lanes still walk through x: an ancestor, never a rise
    }
}

// the pass before any write: *bad |= 1 when an edge names a file >= n or (with check_labels) a label points upwards: the walks would
// leave the array
__global__ void __launch_bounds__(256) uf_check_kernel(const rph_edge *__restrict__ edges, uint64_t n_edges, uint32_t i_base, uint32_t j_base,
                                                       const uint32_t *__restrict__ labels, uint64_t n, bool check_labels, uint32_t *bad)
{
    const uint64_t t0 = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, step = (uint64_t)gridDim.x * blockDim.x;
    bool wrong = false;
    for (uint64_t e = t0; e < n_edges; e += step) wrong |= (uint64_t)edges[e].i + i_base >= n || (uint64_t)edges[e].j + j_base >= n;
    for (uint64_t x = t0; x < n && check_labels; x += step) wrong |= labels[x] > x;
    if (wrong) __hip_atomic_fetch_or(bad, 1u, UF_RELAXED);
}

// ---- export ----
// count[label] of every file and the identity permutation the sort carries; a label that is not a flattened min-label (above its file,
// or not a root itself) is not counted: *bad |= 1
__global__ void __launch_bounds__(256) cc_count_kernel(const uint32_t *__restrict__ labels, uint64_t n, uint32_t *count, uint32_t *ids, uint32_t *bad)
{
    bool wrong = false;
    for (uint64_t x = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; x < n; x += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t l = labels[x];
        ids[x] = (uint32_t)x;
        if (l > x || labels[l] != l)
            wrong = true;
        else
            atomicAdd(&count[l], 1u);
    }
    if (wrong) __hip_atomic_fetch_or(bad, 1u, UF_RELAXED);
}

// member_flag[k]: the k-th file in (label, index) order is in a component of more than one; root_flag[x]: x is the root of one.  A label
// outside the set (cc_count_kernel has flagged it, the call will refuse) is not used as an index.
__global__ void __launch_bounds__(256) cc_flags_kernel(const uint32_t *__restrict__ sorted_labels, const uint32_t *__restrict__ count, uint64_t n,
                                                       uint8_t *member_flag, uint8_t *root_flag)
{
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t l = sorted_labels[k];
        member_flag[k] = l < n && count[l] > 1;
        root_flag[k] = count[k] > 1;
    }
}

int bad_argument(const char *who, const char *what)
{
    rph_set_error("%s: %s", who, what);
    return RPH_ERR_INVALID_ARG;
}
}  // namespace

// Several edge lists over one label array: ONE range check of all of them and of the entry forest (the call waits for it: nothing has
// been written when it refuses), then a union launch per list and one flatten, asynchronous on `s`.
int rph_union_find_labels(rph_ctx *ctx, const rph_union_edges *sets, uint32_t n_sets, uint32_t *d_labels, uint64_t n, hipStream_t s)
{
    uint32_t bad = 0;
    {
        std::lock_guard<std::mutex> lock(ctx->mu);
        ScratchUse use{ctx->sweep_scratch, s};
        RPH_TRY(use.acquire(4, 4096));
        uint32_t *d_bad = ctx->sweep_scratch.as<uint32_t>();
        RPH_HIP_CHECK(hipMemsetAsync(d_bad, 0, 4, s));
        for (uint32_t k = 0; k < n_sets || k == 0; k++) {  // (no list at all: the forest is still checked)
            const rph_union_edges none{}, &q = n_sets ? sets[k] : none;
            hipLaunchKernelGGL(uf_check_kernel, dim3(rph_stride_grid(ctx, std::max<uint64_t>(q.n_edges, k == 0 ? n : 0))), dim3(256), 0, s, q.edges, q.n_edges, q.i_base, q.j_base,
                               d_labels, n, k == 0, d_bad);
            RPH_HIP_CHECK(hipGetLastError());
        }
        RPH_HIP_CHECK(hipMemcpyAsync(&bad, d_bad, 4, hipMemcpyDeviceToHost, s));
        RPH_TRY(use.done());
        RPH_HIP_CHECK(hipStreamSynchronize(s));
    }
    if (bad) return bad_argument("union-find", "an edge names a file outside n, or a label lies above its file");
    for (uint32_t k = 0; k < n_sets; k++) {
        if (!sets[k].n_edges) continue;
        hipLaunchKernelGGL(uf_union_kernel, dim3(rph_stride_grid(ctx, sets[k].n_edges)), dim3(256), 0, s, sets[k].edges, sets[k].n_edges, sets[k].i_base, sets[k].j_base,
                           d_labels);
        RPH_HIP_CHECK(hipGetLastError());
    }
    hipLaunchKernelGGL(uf_flatten_kernel, dim3(rph_stride_grid(ctx, n)), dim3(256), 0, s, d_labels, n);
    RPH_HIP_CHECK(hipGetLastError());
    return RPH_OK;
}

// the flatten alone, for a forest another file's kernels built (merge_tree.hip)
int rph_launch_uf_flatten(rph_ctx *ctx, uint32_t *d_labels, uint64_t n, hipStream_t s)
{
    hipLaunchKernelGGL(uf_flatten_kernel, dim3(rph_stride_grid(ctx, n)), dim3(256), 0, s, d_labels, n);
    RPH_HIP_CHECK(hipGetLastError());
    return RPH_OK;
}

extern "C" int rph_union_find_labels_dev(rph_ctx *ctx, const void *d_edges, uint64_t n_edges, uint32_t i_base, uint32_t j_base, void *d_labels, uint64_t n,
                                         void *stream)
{
    return rph_guarded("rph_union_find_labels_dev", [&]() -> int {
        if (!ctx || (!d_edges && n_edges) || (!d_labels && n)) return bad_argument("rph_union_find_labels_dev", "null argument");
        if (n > 0x7FFFFFFFull) return bad_argument("rph_union_find_labels_dev", "at most 2^31 - 1 files");
        if (n == 0) return n_edges ? bad_argument("rph_union_find_labels_dev", "edges over an empty set") : RPH_OK;
        RPH_HIP_CHECK(hipSetDevice(ctx->device));
        const rph_union_edges one{(const rph_edge *)d_edges, n_edges, i_base, j_base};
        return rph_union_find_labels(ctx, &one, 1, (uint32_t *)d_labels, n, stream ? (hipStream_t)stream : ctx->stream);
    });
}

extern "C" int rph_groups_from_labels_dev(rph_ctx *ctx, const void *d_labels, uint64_t n, uint32_t *members, uint32_t *offsets, uint32_t *n_groups_out,
                                          void *stream)
{
    return rph_guarded("rph_groups_from_labels_dev", [&]() -> int {
        if (!ctx || (!d_labels && n) || !members || !offsets || !n_groups_out) return bad_argument("rph_groups_from_labels_dev", "null argument");
        if (n > 0x7FFFFFFFull) return bad_argument("rph_groups_from_labels_dev", "at most 2^31 - 1 files");  // hipCUB counts are int
        *n_groups_out = 0;
        offsets[0] = 0;
        if (n == 0) return RPH_OK;
        RPH_HIP_CHECK(hipSetDevice(ctx->device));
        hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
        const uint32_t *labels = (const uint32_t *)d_labels;
        if (n == 1) {  // no group; the one label there can be is 0
            uint32_t only = 0;
            RPH_HIP_CHECK(hipMemcpyAsync(&only, labels, 4, hipMemcpyDeviceToHost, s));
            RPH_HIP_CHECK(hipStreamSynchronize(s));
            return only ? bad_argument("rph_groups_from_labels_dev", "the labels are not flattened min-labels") : RPH_OK;
        }
        const int count_n = (int)n, scan_n = (int)(n / 2 + 1);
        int end_bit = 1;
        while (end_bit < 32 && ((n - 1) >> end_bit)) end_bit++;

        // temp sizes first (null pointers of the right types), then one piece of the context's scratch for everything
        size_t sort_bytes = 0, sel_m_bytes = 0, sel_r_bytes = 0, scan_bytes = 0;
        uint32_t *np32 = nullptr;
        uint8_t *np8 = nullptr;
        RPH_HIP_CHECK(hipcub::DeviceRadixSort::SortPairs(nullptr, sort_bytes, (const uint32_t *)np32, np32, (const uint32_t *)np32, np32, count_n, 0, end_bit, s));
        RPH_HIP_CHECK(hipcub::DeviceSelect::Flagged(nullptr, sel_m_bytes, np32, np8, np32, np32, count_n, s));
        RPH_HIP_CHECK(hipcub::DeviceSelect::Flagged(nullptr, sel_r_bytes, np32, np8, np32, np32, count_n, s));
        RPH_HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(nullptr, scan_bytes, np32, np32, scan_n, s));
        const size_t temp_bytes = std::max(std::max(sort_bytes, scan_bytes), std::max(sel_m_bytes, sel_r_bytes));
        Layout L;
        const size_t o_count = L.add(n * 4, 256), o_ids = L.add(n * 4, 256), o_keys = L.add(n * 4, 256), o_vals = L.add(n * 4, 256),
                     o_members = L.add(n * 4, 256), o_gcount = L.add(((size_t)scan_n + 1) * 4, 256), o_offsets = L.add(((size_t)scan_n + 1) * 4, 256),
                     o_mflag = L.add(n, 256), o_rflag = L.add(n, 256), o_nums = L.add(16, 256), o_temp = L.add(temp_bytes + 16, 256);

        // ctx->mu from the acquire to the last copy out of the scratch: the results stay in it until the host has them
        std::lock_guard<std::mutex> lock(ctx->mu);
        ScratchUse use{ctx->sweep_scratch, s};
        RPH_TRY(use.acquire(L.end(), L.end() + L.end() / 4));
        uint8_t *base = ctx->sweep_scratch.data();
        uint32_t *count = (uint32_t *)(base + o_count), *ids = (uint32_t *)(base + o_ids), *keys = (uint32_t *)(base + o_keys), *vals = (uint32_t *)(base + o_vals),
                 *d_members = (uint32_t *)(base + o_members), *gcount = (uint32_t *)(base + o_gcount), *d_offsets = (uint32_t *)(base + o_offsets),
                 *nums = (uint32_t *)(base + o_nums);  // nums: members selected, groups, bad labels
        uint8_t *mflag = base + o_mflag, *rflag = base + o_rflag;
        void *temp = base + o_temp;
        const unsigned grid = rph_stride_grid(ctx, n);
        RPH_HIP_CHECK(hipMemsetAsync(count, 0, n * 4, s));
        RPH_HIP_CHECK(hipMemsetAsync(gcount, 0, ((size_t)scan_n + 1) * 4, s));
        RPH_HIP_CHECK(hipMemsetAsync(nums, 0, 16, s));
        hipLaunchKernelGGL(cc_count_kernel, dim3(grid), dim3(256), 0, s, labels, n, count, ids, nums + 2);
        RPH_HIP_CHECK(hipGetLastError());
        // stable: indices ascend inside a label; labels ascend and a label is its component's first member: groups by first member
        size_t tb = sort_bytes;
        RPH_HIP_CHECK(hipcub::DeviceRadixSort::SortPairs(temp, tb, labels, keys, (const uint32_t *)ids, vals, count_n, 0, end_bit, s));
        hipLaunchKernelGGL(cc_flags_kernel, dim3(grid), dim3(256), 0, s, keys, count, n, mflag, rflag);
        RPH_HIP_CHECK(hipGetLastError());
        tb = sel_m_bytes;
        RPH_HIP_CHECK(hipcub::DeviceSelect::Flagged(temp, tb, vals, mflag, d_members, nums, count_n, s));
        tb = sel_r_bytes;
        RPH_HIP_CHECK(hipcub::DeviceSelect::Flagged(temp, tb, count, rflag, gcount, nums + 1, count_n, s));
        tb = scan_bytes;
        RPH_HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(temp, tb, gcount, d_offsets, scan_n, s));  // gcount is 0 behind the last group
        uint32_t host_nums[4] = {0, 0, 0, 0};
        RPH_HIP_CHECK(hipMemcpyAsync(host_nums, nums, 16, hipMemcpyDeviceToHost, s));
        RPH_HIP_CHECK(hipStreamSynchronize(s));
        int rc = RPH_OK;
        if (host_nums[2] || host_nums[1] > n / 2 || host_nums[0] > n) {
            rc = bad_argument("rph_groups_from_labels_dev", "the labels are not flattened min-labels (label[x] <= x and label[label[x]] == label[x])");
        } else if (host_nums[1]) {
            RPH_HIP_CHECK(hipMemcpyAsync(members, d_members, (size_t)host_nums[0] * 4, hipMemcpyDeviceToHost, s));
            RPH_HIP_CHECK(hipMemcpyAsync(offsets, d_offsets, ((size_t)host_nums[1] + 1) * 4, hipMemcpyDeviceToHost, s));
            RPH_HIP_CHECK(hipStreamSynchronize(s));
            *n_groups_out = host_nums[1];
        }
        RPH_TRY(use.done());
        return rc;
    });
}
