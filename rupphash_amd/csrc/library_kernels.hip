// library_kernels.hip -- the device side of rph_library_remove (library.cpp): which files go and which components they touch, the two
// ascending index lists (survivors; members of the touched components), the row gather that both the compaction and the regroup's
// input are, the rewrite of the regroup's edges to the new numbering, and the survivors' labels.
//
// Nothing here writes an array the library answers from: every output is scratch or the twin of a resident array that library.cpp swaps
// in as its last step.  No kernel reads what another block of the same launch writes.
#include <hipcub/hipcub.hpp>

#include "rph_internal.h"

namespace {
// removed[x] = 1 for every listed file and touched[label[x]] = 1 for its component.  The list holds no file twice (checked by the host),
// so every removed[] byte has one writer; several lanes may store the same 1 into one touched[] byte.
__global__ void __launch_bounds__(256) lib_mark_kernel(const uint32_t *__restrict__ indices, uint64_t n_remove, const uint32_t *__restrict__ labels, uint8_t *removed,
                                                       uint8_t *touched)
{
    for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n_remove; t += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t x = indices[t];
        removed[x] = 1;
        touched[labels[x]] = 1;
    }
}

// the flags the two selections take: keep[x] = the file stays; regroup[x] = its component lost a member (removed files included)
__global__ void __launch_bounds__(256) lib_flags_kernel(const uint8_t *__restrict__ removed, const uint8_t *__restrict__ touched, const uint32_t *__restrict__ labels,
                                                        uint64_t n, uint8_t *keep, uint8_t *regroup)
{
    for (uint64_t x = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; x < n; x += (uint64_t)gridDim.x * blockDim.x) {
        keep[x] = !removed[x];
        regroup[x] = touched[labels[x]];
    }
}

// Rows of `src_*` named by an ascending list, to rows 0 .. count-1 of `dst_*`.  Sixteen lanes per file: each moves 16 bytes of the 256-byte
// variant row (a wave's access is four whole rows; rows that follow each other in the list, the common case, make it one 1 KiB run), the first
// two also move the hash, the next two a flag each.
__global__ void __launch_bounds__(256) lib_gather_kernel(const uint32_t *__restrict__ list, uint64_t count, const uint4 *__restrict__ src_h, const uint4 *__restrict__ src_var,
                                                         const uint8_t *__restrict__ src_lc, const uint8_t *__restrict__ src_hf, uint4 *__restrict__ dst_h,
                                                         uint4 *__restrict__ dst_var, uint8_t *__restrict__ dst_lc, uint8_t *__restrict__ dst_hf)
{
    const uint32_t part = threadIdx.x & 15;
    const uint64_t files_per_pass = (uint64_t)gridDim.x * (blockDim.x / 16);
    for (uint64_t k = (uint64_t)blockIdx.x * (blockDim.x / 16) + threadIdx.x / 16; k < count; k += files_per_pass) {
        const uint64_t x = list[k];
        dst_var[k * 16 + part] = src_var[x * 16 + part];
        if (part < 2)
            dst_h[k * 2 + part] = src_h[x * 2 + part];
        else if (part == 2)
            dst_lc[k] = src_lc[x];
        else if (part == 3)
            dst_hf[k] = src_hf[x];
    }
}

// The regroup's edges, local to the list `members`, in place.  One with a removed file at either end is counted and becomes (0, 0), which
// the union passes over (a self-edge; file 0 exists whenever a union runs); every other one gets the new numbers of its two files.  The
// count: per lane, summed over the wave, one atomic per wave that has any.
__global__ void __launch_bounds__(256) lib_split_edges_kernel(rph_edge *edges, uint64_t n_edges, const uint32_t *__restrict__ members, const uint8_t *__restrict__ removed,
                                                              const uint32_t *__restrict__ new_index, unsigned long long *dropped)
{
    uint32_t mine = 0;
    for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n_edges; e += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t i = members[edges[e].i], j = members[edges[e].j];
        const bool gone = removed[i] | removed[j];
        mine += gone;
        edges[e].i = gone ? 0u : new_index[i];
        edges[e].j = gone ? 0u : new_index[j];
    }
    for (int step = 32; step > 0; step >>= 1) mine += __shfl_down(mine, step, 64);
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd(dropped, (unsigned long long)mine);
}

// The label of every survivor in the new numbering, before the kept edges are united over it: a file of a touched component starts alone;
// every other file keeps its root, which stayed (its component lost nobody).  Order is kept, so the root is still the smallest member.
__global__ void __launch_bounds__(256) lib_labels_kernel(const uint32_t *__restrict__ labels, const uint8_t *__restrict__ removed, const uint8_t *__restrict__ touched,
                                                         const uint32_t *__restrict__ new_index, uint64_t n, uint32_t *new_labels)
{
    for (uint64_t x = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; x < n; x += (uint64_t)gridDim.x * blockDim.x) {
        if (removed[x]) continue;
        const uint32_t k = new_index[x], l = labels[x];
        new_labels[k] = touched[l] ? k : new_index[l];
    }
}

struct FlagToCount {
    __host__ __device__ uint32_t operator()(uint8_t f) const { return f; }
};
using FlagCounts = hipcub::TransformInputIterator<uint32_t, FlagToCount, const uint8_t *>;
using FileNumbers = hipcub::CountingInputIterator<uint32_t>;
}  // namespace

int rph_library_launch_mark(rph_ctx *ctx, const uint32_t *d_indices, uint64_t n_remove, const uint32_t *d_labels, uint64_t n, uint8_t *d_removed, uint8_t *d_touched,
                            uint8_t *d_keep, uint8_t *d_regroup, hipStream_t s)
{
    RPH_HIP_CHECK(hipMemsetAsync(d_removed, 0, n, s));
    RPH_HIP_CHECK(hipMemsetAsync(d_touched, 0, n, s));
    hipLaunchKernelGGL(lib_mark_kernel, dim3(rph_stride_grid(ctx, n_remove)), dim3(256), 0, s, d_indices, n_remove, d_labels, d_removed, d_touched);
    RPH_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(lib_flags_kernel, dim3(rph_stride_grid(ctx, n)), dim3(256), 0, s, d_removed, d_touched, d_labels, n, d_keep, d_regroup);
    RPH_HIP_CHECK(hipGetLastError());
    return RPH_OK;
}

int rph_library_select_temp_bytes(uint64_t n, size_t *bytes_out)
{
    size_t scan = 0, select = 0;
    uint32_t *np32 = nullptr;
    const uint8_t *np8 = nullptr;
    RPH_HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(nullptr, scan, FlagCounts(np8, FlagToCount()), np32, (int)n, nullptr));
    RPH_HIP_CHECK(hipcub::DeviceSelect::Flagged(nullptr, select, FileNumbers(0), np8, np32, np32, (int)n, nullptr));
    *bytes_out = std::max(scan, select);
    return RPH_OK;
}

// d_new_index[x] = kept files below x (the new number of a file that stays); d_survivors and d_members: the file numbers whose flag is
// set, ascending; d_counts[0], [1]: how many of each
int rph_library_launch_select(const uint8_t *d_keep, const uint8_t *d_regroup, uint64_t n, uint32_t *d_new_index, uint32_t *d_survivors, uint32_t *d_members,
                              uint32_t *d_counts, void *d_temp, size_t temp_bytes, hipStream_t s)
{
    size_t tb = temp_bytes;
    RPH_HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(d_temp, tb, FlagCounts(d_keep, FlagToCount()), d_new_index, (int)n, s));
    tb = temp_bytes;
    RPH_HIP_CHECK(hipcub::DeviceSelect::Flagged(d_temp, tb, FileNumbers(0), d_keep, d_survivors, d_counts, (int)n, s));
    tb = temp_bytes;
    RPH_HIP_CHECK(hipcub::DeviceSelect::Flagged(d_temp, tb, FileNumbers(0), d_regroup, d_members, d_counts + 1, (int)n, s));
    return RPH_OK;
}

int rph_library_launch_gather(rph_ctx *ctx, const uint32_t *d_list, uint64_t count, const rph_library_rows &src, const rph_library_rows &dst, hipStream_t s)
{
    if (count == 0) return RPH_OK;
    hipLaunchKernelGGL(lib_gather_kernel, dim3(rph_stride_grid(ctx, count * 16)), dim3(256), 0, s, d_list, count, (const uint4 *)src.hashes, (const uint4 *)src.variants, src.low_conf,
                       src.has_features, (uint4 *)dst.hashes, (uint4 *)dst.variants, dst.low_conf, dst.has_features);
    RPH_HIP_CHECK(hipGetLastError());
    return RPH_OK;
}

int rph_library_launch_split_edges(rph_ctx *ctx, rph_edge *d_edges, uint64_t n_edges, const uint32_t *d_members, const uint8_t *d_removed, const uint32_t *d_new_index,
                                   unsigned long long *d_dropped, hipStream_t s)
{
    RPH_HIP_CHECK(hipMemsetAsync(d_dropped, 0, 8, s));
    if (n_edges == 0) return RPH_OK;
    hipLaunchKernelGGL(lib_split_edges_kernel, dim3(rph_stride_grid(ctx, n_edges)), dim3(256), 0, s, d_edges, n_edges, d_members, d_removed, d_new_index, d_dropped);
    RPH_HIP_CHECK(hipGetLastError());
    return RPH_OK;
}

int rph_library_launch_labels(rph_ctx *ctx, const uint32_t *d_labels, const uint8_t *d_removed, const uint8_t *d_touched, const uint32_t *d_new_index, uint64_t n,
                              uint32_t *d_new_labels, hipStream_t s)
{
    hipLaunchKernelGGL(lib_labels_kernel, dim3(rph_stride_grid(ctx, n)), dim3(256), 0, s, d_labels, d_removed, d_touched, d_new_index, n, d_new_labels);
    RPH_HIP_CHECK(hipGetLastError());
    return RPH_OK;
}
