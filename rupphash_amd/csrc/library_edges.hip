// library_edges.hip -- the device side of an edge-keeping library's store (library.cpp, rph_library_create_tree): the edges an append's
// two sweeps found at `top` go behind the store's end in the library's numbering, the ones within the library's similarity also into a
// compacted list for the union-find; a removal filters the store into a twin.
//
// Both kernels move whole 12-byte records, lane e record e on the reading side; on the writing side the lanes of a wave that keep a
// record take consecutive slots behind one cursor (ballot, one 64-bit atomic per wave), so the order of the records in a list is
// unspecified.  Every lane of a block walks the loop the same number of times: the ballot and the shuffle see whole waves.  Nothing is
// indexed by an edge's file numbers before they have been checked against the size; an edge that fails sets *bad and is written nowhere.
#include "rph_internal.h"

namespace {
// the slot of this lane's record behind *cursor, for the lanes with `take` (the others get nothing to use)
__device__ inline unsigned long long wave_slot(bool take, unsigned long long *cursor)
{
    const unsigned long long mask = __ballot(take);
    if (!mask) return 0;
    const uint32_t lane = threadIdx.x & 63u, leader = (uint32_t)__ffsll((long long)mask) - 1u;
    unsigned long long first = 0;
    if (lane == leader) first = atomicAdd(cursor, (unsigned long long)__popcll(mask));
    first = __shfl(first, (int)leader, 64);
    return first + (unsigned long long)__popcll(mask & ((1ull << lane) - 1ull));
}

// found[0 .. n_cross): (resident file, new-local file); found[n_cross .. n_found): (new-local, new-local), i < j.  nums[0]: cursor of
// `united`; nums[1]: != 0 when an edge lies outside its range or above `top`
__global__ void __launch_bounds__(256) lib_store_append_kernel(const rph_edge *__restrict__ found, uint64_t n_found, uint64_t n_cross, uint32_t n, uint32_t n_new,
                                                               uint32_t similarity, uint32_t top, rph_edge *__restrict__ store_end, rph_edge *__restrict__ united,
                                                               unsigned long long *nums)
{
    bool wrong = false;
    for (uint64_t first = (uint64_t)blockIdx.x * 256; first < n_found; first += (uint64_t)gridDim.x * 256) {
        const uint64_t e = first + threadIdx.x;
        bool unite = false;
        rph_edge r{};
        if (e < n_found) {
            r = found[e];
            const bool cross = e < n_cross;
            const bool ok = (cross ? r.i < n : r.i < r.j) && r.j < n_new && r.d <= top;
            wrong |= !ok;
            if (ok) {
                r.i += cross ? 0u : n;
                r.j += n;
                store_end[e] = r;
                unite = r.d <= similarity;
            }
        }
        const unsigned long long slot = wave_slot(unite, nums);
        if (unite) united[slot] = r;
    }
    if (wrong) atomicOr(nums + 1, 1ull);
}

// nums[0]: cursor of `twin`; nums[1]: dropped edges with d <= similarity; nums[2]: dropped edges; nums[3]: != 0 when an edge lies outside n
__global__ void __launch_bounds__(256) lib_store_filter_kernel(const rph_edge *__restrict__ store, uint64_t n_store, uint64_t n, const uint8_t *__restrict__ removed,
                                                               const uint32_t *__restrict__ new_index, uint32_t similarity, rph_edge *__restrict__ twin,
                                                               unsigned long long *nums)
{
    uint32_t gone_all = 0, gone_near = 0;
    bool wrong = false;
    for (uint64_t first = (uint64_t)blockIdx.x * 256; first < n_store; first += (uint64_t)gridDim.x * 256) {
        const uint64_t e = first + threadIdx.x;
        bool keep = false;
        rph_edge r{};
        if (e < n_store) {
            r = store[e];
            if (r.i < n && r.j < n) {
                keep = !(removed[r.i] | removed[r.j]);
                gone_all += !keep;
                gone_near += !keep && r.d <= similarity;
                if (keep) r.i = new_index[r.i], r.j = new_index[r.j];
            } else {
                wrong = true;
            }
        }
        const unsigned long long slot = wave_slot(keep, nums);
        if (keep) twin[slot] = r;
    }
    for (int step = 32; step > 0; step >>= 1) gone_all += __shfl_down(gone_all, step, 64), gone_near += __shfl_down(gone_near, step, 64);
    if ((threadIdx.x & 63) == 0 && gone_all) atomicAdd(nums + 2, (unsigned long long)gone_all);
    if ((threadIdx.x & 63) == 0 && gone_near) atomicAdd(nums + 1, (unsigned long long)gone_near);
    if (wrong) atomicOr(nums + 3, 1ull);
}
}  // namespace

int rph_library_launch_store_append(rph_ctx *ctx, const rph_edge *d_found, uint64_t n_found, uint64_t n_cross, uint32_t n, uint32_t n_new, uint32_t similarity,
                                    uint32_t top, rph_edge *d_store_end, rph_edge *d_united, unsigned long long *d_nums, hipStream_t s)
{
    RPH_HIP_CHECK(hipMemsetAsync(d_nums, 0, 16, s));
    if (n_found == 0) return RPH_OK;
    hipLaunchKernelGGL(lib_store_append_kernel, dim3(rph_stride_grid(ctx, n_found)), dim3(256), 0, s, d_found, n_found, n_cross, n, n_new, similarity, top, d_store_end,
                       d_united, d_nums);
    RPH_HIP_CHECK(hipGetLastError());
    return RPH_OK;
}

int rph_library_launch_store_filter(rph_ctx *ctx, const rph_edge *d_store, uint64_t n_store, uint64_t n, const uint8_t *d_removed, const uint32_t *d_new_index,
                                    uint32_t similarity, rph_edge *d_twin, unsigned long long *d_nums, hipStream_t s)
{
    RPH_HIP_CHECK(hipMemsetAsync(d_nums, 0, 32, s));
    if (n_store == 0) return RPH_OK;
    hipLaunchKernelGGL(lib_store_filter_kernel, dim3(rph_stride_grid(ctx, n_store)), dim3(256), 0, s, d_store, n_store, n, d_removed, d_new_index, similarity, d_twin,
                       d_nums);
    RPH_HIP_CHECK(hipGetLastError());
    return RPH_OK;
}
