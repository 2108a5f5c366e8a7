// group_info.hip -- per-group max_dist of process_raw_groups (scanner.rs:1986-2022, :2214-2241) on the device: for every listed member
// the minimum Hamming distance to the rows of its group's pivot (its 8 dihedral hashes, or its hash alone), and per group the maximum.
//
// One lane per member slot, grid-stride (rph_stride_grid): most groups have 2 .. 5 members, a wave per group would idle nine lanes in
// ten.  The group of a slot is an upper bound in offsets[] (empty groups are equal neighbours there and are passed over), so the lanes
// of one group are neighbours in a wave.  Their values meet in a segmented scan over __shfl_up; the last lane of every run issues the one
// atomic of that run, and runs of one group in different waves, blocks and passes of the grid meet in that atomic: a group of m members
// costs about m / 64 atomics.  The default pivot (the first listed member that has features) is the same reduction with min over the slot.
//
// Every lane of a wave executes every shuffle: the loops below run over the wave's first slot, which is uniform, and lanes behind the
// last slot carry the operation's neutral value and a group number that is none.
#include "rph_internal.h"

namespace {
constexpr uint32_t NO_GROUP = 0xFFFFFFFFu, NO_SLOT = 0xFFFFFFFFu;

struct MaxInto {
    static constexpr uint32_t neutral = 0;  // what the output is initialised with
    static __device__ __forceinline__ uint32_t combine(uint32_t a, uint32_t b) { return a > b ? a : b; }
    static __device__ __forceinline__ void commit(uint32_t *out, uint32_t v) { atomicMax(out, v); }
};
struct MinInto {
    static constexpr uint32_t neutral = NO_SLOT;
    static __device__ __forceinline__ uint32_t combine(uint32_t a, uint32_t b) { return a < b ? a : b; }
    static __device__ __forceinline__ void commit(uint32_t *out, uint32_t v) { atomicMin(out, v); }
};

// out[g] = Op over the values of the lanes of this wave that carry group g, for every g in the wave.  g ascends with the lane, so a lane
// `step` below with the same group means that every lane in between has it too: the inclusive scan needs no head flags beyond that
// comparison.  After the six steps the last lane of a run holds the run's result; a result that is the neutral value changes nothing.
template <class Op>
__device__ __forceinline__ void reduce_runs(uint32_t g, uint32_t v, uint32_t *out)
{
    const uint32_t lane = threadIdx.x & 63;
    for (uint32_t step = 1; step < 64; step <<= 1) {
        const uint32_t below_v = __shfl_up(v, step, 64), below_g = __shfl_up(g, step, 64);
        if (lane >= step && below_g == g) v = Op::combine(v, below_v);
    }
    const uint32_t above_g = __shfl_down(g, 1, 64);
    if (g != NO_GROUP && (lane == 63 || above_g != g) && v != Op::neutral) Op::commit(out + g, v);
}

// the group of slot t < offsets[n_groups]: the last g with offsets[g] <= t, which is not empty (offsets[0] = 0, offsets ascend)
__device__ __forceinline__ uint32_t group_of_slot(const uint32_t *__restrict__ offsets, uint32_t n_groups, uint32_t t)
{
    uint32_t lo = 0, hi = n_groups;
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (offsets[mid] <= t)
            lo = mid;
        else
            hi = mid;
    }
    return lo;
}

__device__ __forceinline__ uint32_t distance256(const uint4 &a0, const uint4 &a1, const uint4 &b0, const uint4 &b1)
{
    return __popc(a0.x ^ b0.x) + __popc(a0.y ^ b0.y) + __popc(a0.z ^ b0.z) + __popc(a0.w ^ b0.w) + __popc(a1.x ^ b1.x) + __popc(a1.y ^ b1.y) +
           __popc(a1.z ^ b1.z) + __popc(a1.w ^ b1.w);
}

// The pass before anything is read through the arrays: *bad |= 1 for offsets that do not start at 0 or do not ascend, a member >= n, a
// pivot >= n that is not RPH_NO_PIVOT.  It reads offsets[0 .. n_groups], pivots[0 .. n_groups) and members[0 .. offsets[n_groups]), which
// is what the caller says the arrays hold, and nothing through them.  bad[1] = offsets[n_groups].
__global__ void __launch_bounds__(256) gi_check_kernel(const uint32_t *__restrict__ members, const uint32_t *__restrict__ offsets, uint32_t n_groups,
                                                       const uint32_t *__restrict__ pivots, uint64_t n, uint32_t *bad)
{
    const uint64_t t0 = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, step = (uint64_t)gridDim.x * blockDim.x;
    const uint32_t total = offsets[n_groups];
    bool wrong = offsets[0] != 0;
    for (uint64_t g = t0; g < n_groups; g += step) {
        wrong |= offsets[g] > offsets[g + 1];
        if (pivots) wrong |= pivots[g] != RPH_NO_PIVOT && pivots[g] >= n;
    }
    for (uint64_t t = t0; t < total; t += step) wrong |= members[t] >= n;
    if (wrong) atomicOr(bad, 1u);
    if (t0 == 0) bad[1] = total;
}

// first[g] = the smallest slot of group g whose member has features (first[] starts as NO_SLOT)
__global__ void __launch_bounds__(256) gi_first_featured_kernel(const uint32_t *__restrict__ members, const uint32_t *__restrict__ offsets, uint32_t n_groups,
                                                                uint32_t total, const uint8_t *__restrict__ has_features, uint32_t *first)
{
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t base = (uint64_t)blockIdx.x * blockDim.x + (threadIdx.x - lane); base < total; base += step) {
        const uint64_t t = base + lane;
        uint32_t g = NO_GROUP, v = MinInto::neutral;
        if (t < total) {
            g = group_of_slot(offsets, n_groups, (uint32_t)t);
            if (has_features[members[t]]) v = (uint32_t)t;
        }
        reduce_runs<MinInto>(g, v, first);
    }
}

// find_map (scanner.rs:2219-2232): the member at the slot found, else the first listed member, else none (an empty group)
__global__ void __launch_bounds__(256) gi_resolve_pivots_kernel(const uint32_t *__restrict__ members, const uint32_t *__restrict__ offsets, uint32_t n_groups,
                                                                const uint32_t *__restrict__ first, uint32_t *pivots)
{
    for (uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; g < n_groups; g += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t slot = first[g] != NO_SLOT ? first[g] : offsets[g];
        pivots[g] = offsets[g] < offsets[g + 1] ? members[slot] : RPH_NO_PIVOT;
    }
}

// member_dist[t] (nullable) and max_dist[g] (zeroed before).  The rows of a pivot: its hash alone when there are no rows or it has no
// features, else the 8 rows at its group (RPH_ROWS_PER_GROUP) or at its file (RPH_ROWS_PER_FILE).  The member's hash is two 16-byte loads;
// the lanes of a group read the same 256 bytes of rows.
__global__ void __launch_bounds__(256) gi_max_dist_kernel(const uint4 *__restrict__ hashes, const uint4 *__restrict__ rows, int row_mode,
                                                          const uint8_t *__restrict__ has_features, const uint32_t *__restrict__ members,
                                                          const uint32_t *__restrict__ offsets, uint32_t n_groups, uint32_t total,
                                                          const uint32_t *__restrict__ pivots, uint32_t *max_dist, uint32_t *member_dist)
{
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t base = (uint64_t)blockIdx.x * blockDim.x + (threadIdx.x - lane); base < total; base += step) {
        const uint64_t t = base + lane;
        uint32_t g = NO_GROUP, d = MaxInto::neutral;
        if (t < total) {
            g = group_of_slot(offsets, n_groups, (uint32_t)t);
            const uint32_t p = pivots[g];
            if (p != RPH_NO_PIVOT) {
                const uint64_t m = members[t];
                const uint4 h0 = hashes[m * 2], h1 = hashes[m * 2 + 1];
                const bool plain = row_mode == RPH_ROWS_NONE || (has_features && !has_features[p]);
                const uint4 *r = plain ? hashes + (uint64_t)p * 2 : rows + (uint64_t)(row_mode == RPH_ROWS_PER_GROUP ? g : p) * 16;
                const uint32_t n_rows = plain ? 1 : 8;
                d = 256;
                for (uint32_t k = 0; k < n_rows; k++) d = min(d, distance256(h0, h1, r[2 * k], r[2 * k + 1]));
            }
            if (member_dist) member_dist[t] = d;
        }
        reduce_runs<MaxInto>(g, d, max_dist);
    }
}

int bad_argument(const char *who, const char *what)
{
    rph_set_error("%s: %s", who, what);
    return RPH_ERR_INVALID_ARG;
}
}  // namespace

int rph_group_max_dist_run(rph_ctx *ctx, const rph_group_dist &q, uint64_t known_total, hipStream_t s)
{
    const uint32_t ng = q.n_groups;
    // scratch: the check's two words, then first[] and the resolved pivots when the caller gives none
    Layout L;
    const size_t o_bad = L.add(8, 256), o_first = L.add(q.pivots ? 0 : (size_t)ng * 4, 256), o_pivots = L.add(q.pivots ? 0 : (size_t)ng * 4, 256);
    std::lock_guard<std::mutex> lock(ctx->mu);
    ScratchUse use{ctx->sweep_scratch, s};
    RPH_TRY(use.acquire(L.end(), std::max<size_t>(L.end(), 4096)));
    uint8_t *w = ctx->sweep_scratch.data();
    uint32_t *d_bad = (uint32_t *)(w + o_bad), *d_first = (uint32_t *)(w + o_first), *d_own_pivots = (uint32_t *)(w + o_pivots);
    uint64_t total = known_total;
    if (total == RPH_GROUP_TOTAL_ON_DEVICE) {
        uint32_t host_bad[2] = {0, 0};
        RPH_HIP_CHECK(hipMemsetAsync(d_bad, 0, 8, s));
        hipLaunchKernelGGL(gi_check_kernel, dim3(rph_stride_grid(ctx, std::max<uint64_t>(q.n, (uint64_t)ng + 1))), dim3(256), 0, s, q.members, q.offsets, ng, q.pivots, q.n,
                           d_bad);
        RPH_HIP_CHECK(hipGetLastError());
        RPH_HIP_CHECK(hipMemcpyAsync(host_bad, d_bad, 8, hipMemcpyDeviceToHost, s));
        RPH_HIP_CHECK(hipStreamSynchronize(s));
        if (host_bad[0]) {
            RPH_TRY(use.done());
            return bad_argument("rph_group_max_dist_dev", "offsets do not start at 0 or do not ascend, or a member or a pivot names a file outside n");
        }
        total = host_bad[1];
    }
    const uint32_t *pivots = q.pivots;
    const uint8_t *has_features = q.row_mode == RPH_ROWS_NONE ? nullptr : q.has_features;  // the flags only count next to rows, as next to coefficients
    if (!pivots) {
        RPH_HIP_CHECK(hipMemsetAsync(d_first, 0xFF, (size_t)ng * 4, s));
        if (has_features && total) {
            hipLaunchKernelGGL(gi_first_featured_kernel, dim3(rph_stride_grid(ctx, total)), dim3(256), 0, s, q.members, q.offsets, ng, (uint32_t)total, has_features, d_first);
            RPH_HIP_CHECK(hipGetLastError());
        }
        hipLaunchKernelGGL(gi_resolve_pivots_kernel, dim3(rph_stride_grid(ctx, ng)), dim3(256), 0, s, q.members, q.offsets, ng, d_first, d_own_pivots);
        RPH_HIP_CHECK(hipGetLastError());
        pivots = d_own_pivots;
    }
    if (ctx->group_dist_ev[0]) RPH_HIP_CHECK(hipEventRecord(ctx->group_dist_ev[0], s));
    RPH_HIP_CHECK(hipMemsetAsync(q.max_dist, 0, (size_t)ng * 4, s));
    if (total) {
        hipLaunchKernelGGL(gi_max_dist_kernel, dim3(rph_stride_grid(ctx, total)), dim3(256), 0, s, (const uint4 *)q.hashes, (const uint4 *)q.rows, q.row_mode, has_features,
                           q.members, q.offsets, ng, (uint32_t)total, pivots, q.max_dist, q.member_dist);
        RPH_HIP_CHECK(hipGetLastError());
    }
    if (ctx->group_dist_ev[1]) RPH_HIP_CHECK(hipEventRecord(ctx->group_dist_ev[1], s));
    return use.done();
}

int rph_group_lists_dev::upload(const uint32_t *h_members, const uint32_t *h_offsets, uint32_t ng, const uint32_t *h_pivots, bool want_member_dist, hipStream_t s)
{
    n_groups = ng, total = h_offsets[ng];
    Layout in, out;
    const size_t o_members = in.add(total * 4, 256), o_offsets = in.add(((size_t)ng + 1) * 4, 256), o_pivots = in.add(h_pivots ? (size_t)ng * 4 : 0, 256);
    const size_t o_max = out.add((size_t)ng * 4, 256), o_member = out.add(want_member_dist ? total * 4 : 0, 256);
    RPH_TRY(d_groups.reserve(in.end(), s));
    RPH_TRY(d_out.reserve(out.end(), s));
    members = (uint32_t *)(d_groups.data() + o_members), offsets = (uint32_t *)(d_groups.data() + o_offsets);
    pivots = h_pivots ? (uint32_t *)(d_groups.data() + o_pivots) : nullptr;
    max_dist = (uint32_t *)(d_out.data() + o_max), member_dist = want_member_dist ? (uint32_t *)(d_out.data() + o_member) : nullptr;
    if (total) RPH_HIP_CHECK(hipMemcpyAsync(members, h_members, total * 4, hipMemcpyHostToDevice, s));
    RPH_HIP_CHECK(hipMemcpyAsync(offsets, h_offsets, ((size_t)ng + 1) * 4, hipMemcpyHostToDevice, s));
    if (h_pivots) RPH_HIP_CHECK(hipMemcpyAsync(pivots, h_pivots, (size_t)ng * 4, hipMemcpyHostToDevice, s));
    return RPH_OK;
}

int rph_group_lists_dev::download(uint32_t *max_dist_out, uint32_t *member_dist_out, hipStream_t s)
{
    RPH_HIP_CHECK(hipMemcpyAsync(max_dist_out, max_dist, (size_t)n_groups * 4, hipMemcpyDeviceToHost, s));
    if (member_dist_out && total) RPH_HIP_CHECK(hipMemcpyAsync(member_dist_out, member_dist, total * 4, hipMemcpyDeviceToHost, s));
    RPH_HIP_CHECK(hipStreamSynchronize(s));
    return RPH_OK;
}

extern "C" {

int rph_group_max_dist_dev(rph_ctx *ctx, const void *d_hashes32, uint64_t n, const void *d_rows, int row_mode, const void *d_has_features, const void *d_members,
                           const void *d_offsets, uint32_t n_groups, const void *d_pivots, void *d_max_dist, void *d_member_dist, void *stream)
{
    return rph_guarded("rph_group_max_dist_dev", [&]() -> int {
        const char *who = "rph_group_max_dist_dev";
        if (!ctx) return bad_argument(who, "null argument");
        if (row_mode != RPH_ROWS_NONE && row_mode != RPH_ROWS_PER_GROUP && row_mode != RPH_ROWS_PER_FILE) return bad_argument(who, "row_mode is none of RPH_ROWS_*");
        if (n_groups == 0) return RPH_OK;
        if (!d_hashes32 || !d_members || !d_offsets || !d_max_dist || (row_mode != RPH_ROWS_NONE && !d_rows)) return bad_argument(who, "null argument");
        if (n >= RPH_NO_PIVOT) return bad_argument(who, "at most 2^32 - 2 files");
        if (((uintptr_t)d_hashes32 | (row_mode != RPH_ROWS_NONE ? (uintptr_t)d_rows : 0)) & 15) return bad_argument(who, "hashes and rows are read 16 bytes at a time: align them to 16");
        RPH_HIP_CHECK(hipSetDevice(ctx->device));
        rph_group_dist q;
        q.hashes = (const uint8_t *)d_hashes32, q.n = n, q.rows = (const uint8_t *)d_rows, q.row_mode = row_mode, q.has_features = (const uint8_t *)d_has_features;
        q.members = (const uint32_t *)d_members, q.offsets = (const uint32_t *)d_offsets, q.n_groups = n_groups, q.pivots = (const uint32_t *)d_pivots;
        q.max_dist = (uint32_t *)d_max_dist, q.member_dist = (uint32_t *)d_member_dist;
        return rph_group_max_dist_run(ctx, q, RPH_GROUP_TOTAL_ON_DEVICE, stream ? (hipStream_t)stream : ctx->stream);
    });
}

int rph_group_max_dist(rph_ctx *ctx, const uint8_t *hashes32, const float *coeffs, const uint8_t *has_features, uint64_t n, const uint32_t *members,
                       const uint32_t *offsets, uint32_t n_groups, const uint32_t *pivots, uint32_t *max_dist_out, uint32_t *member_dist_out)
{
    return rph_guarded("rph_group_max_dist", [&]() -> int {
        if (!ctx) return bad_argument("rph_group_max_dist", "null argument");
        RPH_TRY(rph_host_group_lists_check("rph_group_max_dist", hashes32, n, members, offsets, n_groups, pivots, max_dist_out));
        if (n_groups == 0) return RPH_OK;
        // the pivots on the host in any case: their coefficient rows are the only ones that cross PCIe
        std::vector<uint32_t> own;
        if (!pivots) {
            own.resize(n_groups);
            for (uint32_t g = 0; g < n_groups; g++) own[g] = rph_host_default_pivot(members, offsets, g, coeffs, has_features);
            pivots = own.data();
        }
        RPH_HIP_CHECK(hipSetDevice(ctx->device));
        hipStream_t s = ctx->stream;
        DevBuf d_h, d_hf, d_rows, d_stage;
        rph_group_lists_dev call;
        StreamDrain drain{s};  // the buffers above go when the stream is through with them
        RPH_TRY(d_h.alloc(n * 32));
        RPH_HIP_CHECK(hipMemcpyAsync(d_h.data(), hashes32, n * 32, hipMemcpyHostToDevice, s));
        if (coeffs && has_features) {
            RPH_TRY(d_hf.alloc(n));
            RPH_HIP_CHECK(hipMemcpyAsync(d_hf.data(), has_features, n, hipMemcpyHostToDevice, s));
        }
        RPH_TRY(call.upload(members, offsets, n_groups, pivots, member_dist_out != nullptr, s));
        if (coeffs) {  // one row block per group, in pieces through a fixed staging buffer (a group whose pivot has no features: zeros, not read)
            const uint64_t step = 1u << 18;  // 256 MiB of coefficients per piece
            const uint64_t most = std::min<uint64_t>(step, n_groups);
            RPH_TRY(d_rows.alloc((size_t)n_groups * 256));
            RPH_TRY(d_stage.alloc(most * 1024));
            std::vector<float> piece(most * 256);
            for (uint64_t first = 0; first < n_groups; first += step) {
                const uint32_t m = (uint32_t)std::min<uint64_t>(step, n_groups - first);
                for (uint32_t k = 0; k < m; k++) {
                    const uint32_t p = pivots[first + k];
                    const bool featured = p != RPH_NO_PIVOT && (!has_features || has_features[p]);
                    if (featured)
                        std::copy(coeffs + (size_t)p * 256, coeffs + (size_t)p * 256 + 256, piece.begin() + (size_t)k * 256);
                    else
                        std::fill(piece.begin() + (size_t)k * 256, piece.begin() + (size_t)k * 256 + 256, 0.0f);
                }
                RPH_HIP_CHECK(hipMemcpyAsync(d_stage.data(), piece.data(), (size_t)m * 1024, hipMemcpyHostToDevice, s));
                RPH_TRY(rph_pdq_hashes_from_coeffs_dev(ctx, d_stage.data(), m, nullptr, d_rows.data() + first * 256, s));
                RPH_HIP_CHECK(hipStreamSynchronize(s));  // `piece` is filled again
            }
        }
        rph_group_dist q;
        q.hashes = d_h.data(), q.n = n, q.rows = d_rows.data(), q.row_mode = coeffs ? RPH_ROWS_PER_GROUP : RPH_ROWS_NONE, q.has_features = d_hf.data();
        call.fill(q);
        RPH_TRY(rph_group_max_dist_run(ctx, q, call.total, s));
        return call.download(max_dist_out, member_dist_out, s);
    });
}

}  // extern "C"

// Arms (or, with nulls, disarms) two events of the caller's around the zeroing and the distance kernel of the calls that follow on this
// context (exported for tools/group_max_dist_rate.py, not in the header)
extern "C" int rph_debug_group_max_dist_events(rph_ctx *ctx, void *start, void *stop)
{
    if (!ctx) return bad_argument("rph_debug_group_max_dist_events", "null argument");
    std::lock_guard<std::mutex> lock(ctx->mu);
    ctx->group_dist_ev[0] = (hipEvent_t)start, ctx->group_dist_ev[1] = (hipEvent_t)stop;
    return RPH_OK;
}
