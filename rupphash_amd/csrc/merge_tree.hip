// merge_tree.hip -- the merge tree of a swept edge list on the device (include/rupphash.h, "Merge tree"): the components of
// group_files_generic (scanner.rs:1640-1817) at EVERY similarity 0 .. top from the edges of one sweep at top.
//
// The components at s are those of the edges with d <= s (single linkage), so they are nested, and Kruskal by level finds them all:
// the union-find of components.hip run over the edges of level 0, then of level 1, ... never splits what it joined.  That union-find
// hooks the LARGER of two roots under the smaller, so a file stops being the root -- the smallest member -- of its component exactly
// once, when a CAS hooks it: that level is level[x].  into[x] is the root of x once ALL unions of that level are done (the root the
// CAS wrote may itself be hooked later in the level), so it is resolved by a second launch behind the level's unions.  Neither array
// depends on the order of the edges or of the lanes: they are defined by the components alone.
//
// One launch per step, no grid-wide barrier, no lane that waits for a value another lane has yet to write (uf_union_kernel's comment
// in components.hip says why that matters); the host synchronises once, for the range check and the per-level counts.
#include "rph_internal.h"
#include "uf_device.h"

namespace {
constexpr uint32_t LEVELS = 256;  // top <= 254 (255 is RPH_TREE_NEVER), and a block of these kernels has one lane per level

// the head of the call's piece of scratch
struct TreeHead {
    uint32_t bad;                      // the range check's flag
    uint32_t hooked;                   // cursor of the hooked list: roots absorbed so far
    uint32_t snap[LEVELS + 1];         // snap[k]: that cursor before the k-th non-empty level
    unsigned long long hist[LEVELS];   // edges_at
    unsigned long long fill[LEVELS];   // entries reserved so far in every level's bucket of `pairs`
};

// where every level's bucket begins in `pairs`: the exclusive prefix sum of the counts, made by the host behind its one synchronisation
// and passed to the scatter as a kernel argument (2 KB)
struct TreeOffsets {
    unsigned long long at[LEVELS];
};

// Range check and histogram in one pass.  An edge that names a file >= n or a distance above top sets the flag and is not counted; the
// host reads the flag and the counts before anything else runs.  Per-wave LDS bins (a wave whose lanes all carry one level serialises on
// one LDS word, not on one L2 line), then one global atomic per non-empty bin and block.
__global__ void __launch_bounds__(256) tree_check_kernel(const rph_edge *__restrict__ edges, uint64_t n_edges, uint32_t i_base, uint32_t j_base, uint64_t n, uint32_t top,
                                                         TreeHead *head)
{
    __shared__ uint32_t bins[4][LEVELS];
    for (uint32_t k = threadIdx.x; k < 4 * LEVELS; k += 256) (&bins[0][0])[k] = 0;
    __syncthreads();
    const uint32_t wave = threadIdx.x >> 6;
    bool wrong = false;
    for (uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x; e < n_edges; e += (uint64_t)gridDim.x * 256) {
        const rph_edge ed = edges[e];
        if ((uint64_t)ed.i + i_base < n && (uint64_t)ed.j + j_base < n && ed.d <= top)
            atomicAdd(&bins[wave][ed.d], 1u);
        else
            wrong = true;
    }
    __syncthreads();
    const uint32_t t = threadIdx.x, c = bins[0][t] + bins[1][t] + bins[2][t] + bins[3][t];
    if (c) atomicAdd(&head->hist[t], (unsigned long long)c);
    if (wrong) __hip_atomic_fetch_or(&head->bad, 1u, UF_RELAXED);
}

__global__ void __launch_bounds__(256) tree_init_kernel(uint32_t *parent, uint32_t *into, uint8_t *level, uint64_t n)
{
    for (uint64_t x = (uint64_t)blockIdx.x * 256 + threadIdx.x; x < n; x += (uint64_t)gridDim.x * 256) {
        parent[x] = (uint32_t)x;
        into[x] = (uint32_t)x;
        level[x] = RPH_TREE_NEVER;
    }
}

// The edges into level buckets as (i + i_base, j + j_base).  A block counts its edges per level, reserves its range of every non-empty
// bucket with one atomic, then reads its edges again and writes them; the order inside a bucket is whatever the lanes make it.  The
// counts come from the same edges as the histogram that sized the buckets, so every position lies inside its bucket.
__global__ void __launch_bounds__(256) tree_scatter_kernel(const rph_edge *__restrict__ edges, uint64_t n_edges, uint32_t i_base, uint32_t j_base, uint32_t top, TreeHead *head,
                                                           const TreeOffsets offsets, uint2 *pairs)
{
    __shared__ uint32_t cnt[LEVELS];
    __shared__ unsigned long long base[LEVELS];
    const uint32_t t = threadIdx.x;
    const uint64_t first = (uint64_t)blockIdx.x * 256 + threadIdx.x, step = (uint64_t)gridDim.x * 256;
    cnt[t] = 0;
    __syncthreads();
    for (uint64_t e = first; e < n_edges; e += step) {
        const uint32_t d = edges[e].d;
        if (d <= top) atomicAdd(&cnt[d], 1u);
    }
    __syncthreads();
    const uint32_t c = cnt[t];
    if (c) base[t] = offsets.at[t] + atomicAdd(&head->fill[t], (unsigned long long)c);
    __syncthreads();
    cnt[t] = 0;
    __syncthreads();
    for (uint64_t e = first; e < n_edges; e += step) {
        const rph_edge ed = edges[e];
        if (ed.d > top) continue;
        const unsigned long long at = base[ed.d] + atomicAdd(&cnt[ed.d], 1u);
        if (at < n_edges) pairs[at] = make_uint2(ed.i + i_base, ed.j + j_base);
    }
}

// uf_union_kernel's loop (components.hip) over one level's bucket.  The lane whose CAS hooks root `hi` is the only lane that ever does so
// for `hi` -- a root is hooked once and is never a root again -- so it alone writes level[hi] and appends hi to the hooked list, which
// therefore holds at most n - 1 entries over the whole call.
__global__ void __launch_bounds__(256) tree_union_kernel(const uint2 *__restrict__ pairs, uint64_t n_pairs, uint32_t *parent, uint8_t *level, uint32_t *hooked, uint64_t n,
                                                         TreeHead *head, uint32_t t)
{
    for (uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x; e < n_pairs; e += (uint64_t)gridDim.x * 256) {
        uint32_t a = pairs[e].x, b = pairs[e].y;
        for (;;) {
            a = uf_find(parent, a);
            b = uf_find(parent, b);
            if (a == b) break;
            const uint32_t hi = a > b ? a : b, lo = a > b ? b : a;
            uint32_t seen = hi;
            if (__hip_atomic_compare_exchange_strong(parent + hi, &seen, lo, __ATOMIC_RELAXED, UF_RELAXED)) {
                level[hi] = (uint8_t)t;
                const uint32_t at = atomicAdd(&head->hooked, 1u);
                if (at < n) hooked[at] = hi;
                break;
            }
            a = seen;
            b = lo;
        }
    }
}

// Behind the k-th non-empty level's unions: into[x] = the root of x now, for the roots that level hooked.  They are the entries of the
// hooked list from where the level before left the cursor (snap[k]) to where it stands; one lane leaves that for the next level.  Nothing
// changes a root during this launch (only path halving runs), so the answer does not depend on the lanes' order.
__global__ void __launch_bounds__(256) tree_resolve_kernel(uint32_t *parent, uint32_t *into, const uint32_t *__restrict__ hooked, uint64_t n, TreeHead *head, uint32_t k)
{
    const uint32_t first = head->snap[k], now = head->hooked, last = now < n ? now : (uint32_t)n;
    for (uint64_t at = (uint64_t)first + (uint64_t)blockIdx.x * 256 + threadIdx.x; at < last; at += (uint64_t)gridDim.x * 256) {
        const uint32_t x = hooked[at];
        into[x] = uf_find(parent, x);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) head->snap[k + 1] = last;
}

int bad_argument(const char *who, const char *what)
{
    rph_set_error("%s: %s", who, what);
    return RPH_ERR_INVALID_ARG;
}
}  // namespace

int rph_merge_tree_run(rph_ctx *ctx, const rph_edge *d_edges, uint64_t n_edges, uint32_t i_base, uint32_t j_base, uint64_t n, uint32_t top, uint32_t *d_into,
                       uint8_t *d_level, uint64_t *d_edges_at, uint32_t *d_labels, hipStream_t s)
{
    Layout L;
    const size_t o_head = L.add(sizeof(TreeHead), 256), o_pairs = L.add(n_edges * sizeof(uint2), 256), o_hooked = L.add(n * 4, 256),
                 o_parent = L.add(d_labels ? 0 : n * 4, 256);
    // ctx->mu for the whole call: the counts stay in the scratch between the check and the launches they size
    std::lock_guard<std::mutex> lock(ctx->mu);
    ScratchUse use{ctx->sweep_scratch, s};
    RPH_TRY(use.acquire(L.end(), L.end() + L.end() / 4));
    uint8_t *base = ctx->sweep_scratch.data();
    TreeHead *head = (TreeHead *)(base + o_head);
    uint2 *pairs = (uint2 *)(base + o_pairs);
    uint32_t *hooked = (uint32_t *)(base + o_hooked), *parent = d_labels ? d_labels : (uint32_t *)(base + o_parent);
    hipEvent_t *ev = ctx->merge_tree_ev;

    if (ev[0]) RPH_HIP_CHECK(hipEventRecord(ev[0], s));
    RPH_HIP_CHECK(hipMemsetAsync(head, 0, sizeof(TreeHead), s));
    if (n_edges) {
        hipLaunchKernelGGL(tree_check_kernel, dim3(rph_stride_grid(ctx, n_edges)), dim3(256), 0, s, d_edges, n_edges, i_base, j_base, n, top, head);
        RPH_HIP_CHECK(hipGetLastError());
    }
    if (ev[1]) RPH_HIP_CHECK(hipEventRecord(ev[1], s));
    struct {
        uint32_t bad;
        unsigned long long hist[LEVELS];
    } seen;
    {
        StreamDrain drain{s};  // the copies land in `seen` before it goes, whatever fails
        RPH_HIP_CHECK(hipMemcpyAsync(&seen.bad, &head->bad, 4, hipMemcpyDeviceToHost, s));
        RPH_HIP_CHECK(hipMemcpyAsync(seen.hist, head->hist, (size_t)(top + 1) * 8, hipMemcpyDeviceToHost, s));
        RPH_HIP_CHECK(hipStreamSynchronize(s));
    }
    if (seen.bad) {
        RPH_TRY(use.done());
        return bad_argument("merge tree", "an edge names a file outside n or a distance above top");
    }

    RPH_HIP_CHECK(hipMemcpyAsync(d_edges_at, head->hist, (size_t)(top + 1) * 8, hipMemcpyDeviceToDevice, s));
    hipLaunchKernelGGL(tree_init_kernel, dim3(rph_stride_grid(ctx, n)), dim3(256), 0, s, parent, d_into, d_level, n);
    RPH_HIP_CHECK(hipGetLastError());
    if (n_edges) {
        TreeOffsets offsets{};
        for (uint32_t t = 0; t < top; t++) offsets.at[t + 1] = offsets.at[t] + seen.hist[t];
        hipLaunchKernelGGL(tree_scatter_kernel, dim3(rph_stride_grid(ctx, n_edges)), dim3(256), 0, s, d_edges, n_edges, i_base, j_base, top, head, offsets, pairs);
        RPH_HIP_CHECK(hipGetLastError());
    }
    if (ev[2]) RPH_HIP_CHECK(hipEventRecord(ev[2], s));
    uint64_t offset = 0;
    uint32_t k = 0;
    for (uint32_t t = 0; t <= top; t++) {
        const uint64_t m = seen.hist[t];
        if (!m) continue;
        hipLaunchKernelGGL(tree_union_kernel, dim3(rph_stride_grid(ctx, m)), dim3(256), 0, s, pairs + offset, m, parent, d_level, hooked, n, head, t);
        RPH_HIP_CHECK(hipGetLastError());
        // at most one root per edge and fewer than n in all
        hipLaunchKernelGGL(tree_resolve_kernel, dim3(rph_stride_grid(ctx, std::min<uint64_t>(m, n))), dim3(256), 0, s, parent, d_into, hooked, n, head, k);
        RPH_HIP_CHECK(hipGetLastError());
        offset += m;
        k++;
    }
    if (d_labels) RPH_TRY(rph_launch_uf_flatten(ctx, d_labels, n, s));
    if (ev[3]) RPH_HIP_CHECK(hipEventRecord(ev[3], s));
    return use.done();
}

extern "C" int rph_merge_tree_dev(rph_ctx *ctx, const void *d_edges, uint64_t n_edges, uint32_t i_base, uint32_t j_base, uint64_t n, uint32_t top, void *d_into,
                                  void *d_level, void *d_edges_at, void *d_labels, void *stream)
{
    return rph_guarded("rph_merge_tree_dev", [&]() -> int {
        if (!ctx || (!d_edges && n_edges) || ((!d_into || !d_level) && n) || !d_edges_at) return bad_argument("rph_merge_tree_dev", "null argument");
        if (n > 0x7FFFFFFFull) return bad_argument("rph_merge_tree_dev", "at most 2^31 - 1 files");
        if (top >= RPH_TREE_NEVER) return bad_argument("rph_merge_tree_dev", "top at most 254: level 255 is RPH_TREE_NEVER");
        if (n == 0 && n_edges) return bad_argument("rph_merge_tree_dev", "edges over an empty set");
        RPH_HIP_CHECK(hipSetDevice(ctx->device));
        hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
        if (n == 0) {
            RPH_HIP_CHECK(hipMemsetAsync(d_edges_at, 0, (size_t)(top + 1) * 8, s));
            return RPH_OK;
        }
        return rph_merge_tree_run(ctx, (const rph_edge *)d_edges, n_edges, i_base, j_base, n, top, (uint32_t *)d_into, (uint8_t *)d_level, (uint64_t *)d_edges_at,
                                  (uint32_t *)d_labels, s);
    });
}

// Arms (or, with nulls, disarms) four events of the caller's in the calls that follow on this context: before the check, behind check and
// histogram, behind init and scatter, behind the level loop and the flatten (exported for tools/merge_tree_rate.py, not in the header)
extern "C" int rph_debug_merge_tree_events(rph_ctx *ctx, void *e0, void *e1, void *e2, void *e3)
{
    if (!ctx) return bad_argument("rph_debug_merge_tree_events", "null argument");
    std::lock_guard<std::mutex> lock(ctx->mu);
    ctx->merge_tree_ev[0] = (hipEvent_t)e0, ctx->merge_tree_ev[1] = (hipEvent_t)e1, ctx->merge_tree_ev[2] = (hipEvent_t)e2, ctx->merge_tree_ev[3] = (hipEvent_t)e3;
    return RPH_OK;
}
