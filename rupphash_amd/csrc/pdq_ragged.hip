// pdq_ragged.hip -- PDQ hashes of images of any mix of geometries in one call (rph_pdq_hash_ragged, include/rupphash.h) for gfx950.
//
// The uniform path takes its geometry as launch constants, so a corpus of many sizes costs a launch sequence per size.  Here the geometry
// is data: the host plans the call into one descriptor per image and three work lists, uploads them in one copy, and three kernels whose
// grids cover the whole chunk read them with uniform (scalar) loads:
//   ragged_luma_kernel        to_luma601 of every colour image (and a copy of Luma8 images whose rows are not on dword boundaries) into
//                             Luma8 planes with 16-byte aligned rows: st_luma_kernel's arithmetic, a block finds its image in a prefix table.
//                             Images of rph_image_hash_ragged's other layouts (LumaA8, 16-bit samples) always get such a plane
//   resize_ragged_kernel      the pre-downsample of images with a side > 512 on the matrix pipe: resize_mfma_kernel's task (resize_mfma.hpp),
//                             (image, row tile, column tile) from a prefix table, the box windows from one blob of axis tables
//   pdq_stream_ragged_kernel  one wave per image or thumbnail: the stages of pdq_stream_kernel (pdq_stream_stages.hpp)
// No atomics, no dependence between workgroups; the kernels follow each other on one stream.  Images the kernels do not take (class F,
// below) go through rph_pdq_hash_batch_dev in runs of equal geometry; those of the other layouts as Luma8, from planes the first kernel
// wrote (the reference, too, does everything behind to_luma601 from the luma plane).  rph_image_hash_ragged(_dev) adds the pixel hash of
// every image from the same pixels (b3_pixels_ragged_kernel, blake3_kernels.hip).
#include <algorithm>
#include <cstring>
#include <map>
#include <utility>
#include <vector>

#include "pdq_stream_stages.hpp"
#include "resize_mfma.hpp"
#include "rph_internal.h"

namespace {

constexpr uint64_t RG_NONE = ~(uint64_t)0;

// One image of class S or R.  Offsets: src_off from the call's pixel base, the others from the start of the chunk's scratch.
struct RgDesc {
    uint64_t src_off;        // the image's first byte
    uint64_t row_stride;     // bytes between its rows
    uint32_t w, h, layout;   // RPH_LAYOUT_*: 1, 3, 4 = the channels of rph_pdq_hash_ragged
    uint32_t luma_pitch;     // Luma8 plane (rows of luma_pitch bytes, a multiple of 16) at luma_off; RG_NONE: the image is Luma8 and read where it is
    uint64_t luma_off;
    uint64_t thumb_off;      // class R: thumbnail of tw x th, rows of tpitch bytes (a multiple of 16); class S: tw = 0
    uint32_t tw, th, tpitch;
    uint32_t ax, ay;         // class R: the axes' tables in the axis blob, in dwords: start[out], size[out], c1[out]
    uint32_t prec_x, prec_y;
    uint32_t out;            // output slot
};
static_assert(sizeof(RgDesc) % 8 == 0, "descriptors follow each other in the blob");

// the task whose blocks include block b: first[i] <= b < first[i + 1] (first[n] = the grid).  Uniform: every load is scalar.
__device__ __forceinline__ uint32_t rg_find(const uint32_t *__restrict__ first, uint32_t n, uint32_t b)
{
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) / 2;
        if (first[mid] <= b)
            lo = mid;
        else
            hi = mid;
    }
    return lo;
}

__global__ void __launch_bounds__(256) ragged_luma_kernel(const uint8_t *__restrict__ src, uint8_t *__restrict__ scratch, const RgDesc *__restrict__ desc,
                                                          const uint32_t *__restrict__ first, const uint32_t *__restrict__ which, uint32_t n_tasks)
{
    const uint32_t task = rg_find(first, n_tasks, blockIdx.x);
    const RgDesc &d = desc[which[task]];
    const uint32_t w = d.w, h = d.h, quads = (w + 3) / 4;
    const uint32_t t = (blockIdx.x - first[task]) * 256 + threadIdx.x;
    if (t >= quads * h) return;
    const uint32_t y = t / quads, q = t - y * quads;
    const uint8_t *row = src + d.src_off + (size_t)y * d.row_stride;
    uint32_t o;
    switch (d.layout) {  // (uniform)
    case RPH_LAYOUT_LUMA8: o = st_luma_quad<1>(row + (size_t)q * 4, q, w); break;
    case RPH_LAYOUT_RGB8: o = st_luma_quad<3>(row + (size_t)q * 12, q, w); break;
    case RPH_LAYOUT_RGBA8: o = st_luma_quad<4>(row + (size_t)q * 16, q, w); break;
    case RPH_LAYOUT_LUMAA8: o = st_luma_quad_layout<RPH_LAYOUT_LUMAA8>(row + (size_t)q * 8, q, w); break;
    case RPH_LAYOUT_LUMA16: o = st_luma_quad_layout<RPH_LAYOUT_LUMA16>(row + (size_t)q * 8, q, w); break;
    case RPH_LAYOUT_LUMAA16: o = st_luma_quad_layout<RPH_LAYOUT_LUMAA16>(row + (size_t)q * 16, q, w); break;
    case RPH_LAYOUT_RGB16: o = st_luma_quad_layout<RPH_LAYOUT_RGB16>(row + (size_t)q * 24, q, w); break;
    default: o = st_luma_quad_layout<RPH_LAYOUT_RGBA16>(row + (size_t)q * 32, q, w); break;
    }
    reinterpret_cast<uint32_t *>(scratch + d.luma_off + (size_t)y * d.luma_pitch)[q] = o;
}

__global__ void __launch_bounds__(64) resize_ragged_kernel(const uint8_t *__restrict__ src, uint8_t *scratch, const RgDesc *__restrict__ desc,
                                                           const uint32_t *__restrict__ first, const uint32_t *__restrict__ which, uint32_t n_tasks,
                                                           const uint32_t *__restrict__ axes)
{
    const uint32_t task = rg_find(first, n_tasks, blockIdx.x);
    const RgDesc &d = desc[which[task]];
    const uint32_t tile = blockIdx.x - first[task], tiles_x = (d.tw + 63) / 64;
    const uint32_t ty = tile / tiles_x, tx = tile - ty * tiles_x;
    const uint32_t *tx_ = axes + d.ax, *ty_ = axes + d.ay;
    const DevAxis ax{tx_, tx_ + d.tw, nullptr, reinterpret_cast<const int32_t *>(tx_ + 2 * d.tw), 0, (int)d.prec_x};
    const DevAxis ay{ty_, ty_ + d.th, nullptr, reinterpret_cast<const int32_t *>(ty_ + 2 * d.th), 0, (int)d.prec_y};
    const bool plane = d.luma_off != RG_NONE;  // colour sources come as the Luma8 plane ragged_luma_kernel wrote
    const uint8_t *base = plane ? scratch + d.luma_off : src + d.src_off;
    const size_t rs = plane ? (size_t)d.luma_pitch : (size_t)d.row_stride;
    rz_mfma_tile(base, d.w, d.h, rs, d.tw, d.th, ax, ay, ty * 32, tx * 64, scratch + d.thumb_off, d.tpitch);
}

__global__ void __launch_bounds__(64, 2) pdq_stream_ragged_kernel(const uint8_t *__restrict__ src, const uint8_t *__restrict__ scratch, const RgDesc *__restrict__ desc,
                                                                  const uint32_t *__restrict__ list, uint8_t *hash, float *quality, float *coeffs, uint8_t *dihedral,
                                                                  uint8_t *valid)
{
    __shared__ __attribute__((aligned(16))) float lds[ST_LDS_FLOATS];
    const RgDesc &d = desc[list[blockIdx.x]];
    // what the wave hashes: the thumbnail (class R), the Luma8 plane, or the image itself (Luma8 with rows on dword boundaries)
    const uint8_t *px0 = src + d.src_off;
    uint32_t W = d.w, H = d.h;
    size_t rs = (size_t)d.row_stride;
    if (d.tw) {
        px0 = scratch + d.thumb_off;
        W = d.tw;
        H = d.th;
        rs = d.tpitch;
    } else if (d.luma_off != RG_NONE) {
        px0 = scratch + d.luma_off;
        rs = d.luma_pitch;
    }
    const uint32_t slot = d.out;
    const StGeo g = st_geo((int)W, (int)H);
    st_image(lds, px0, g, rs, hash, quality, coeffs, dihedral, slot);
    if (valid && threadIdx.x == 0) valid[slot] = 1;
}

// ---- host: the plan of a call

// pinned memory a chunk's blob is uploaded from: a ring, each slot guarded by the event of its last upload
struct RaggedState {
    static constexpr int kSlots = 4;
    PinnedBuf pin[kSlots];
    hipEvent_t done[kSlots] = {};
    int next = 0;
};

// The next slot of the context's ring with room for `bytes`, free to be written (ctx->mu held); staged() after the copy that reads it.
int stage(rph_ctx *ctx, size_t bytes, uint8_t **hb, int *slot_out)
{
    if (!ctx->ragged) ctx->ragged = new RaggedState();
    RaggedState &R = *static_cast<RaggedState *>(ctx->ragged);
    const int slot = R.next;
    R.next = (R.next + 1) % RaggedState::kSlots;
    if (R.done[slot])
        RPH_HIP_CHECK(hipEventSynchronize(R.done[slot]));  // the upload that last used this slot
    else
        RPH_HIP_CHECK(hipEventCreateWithFlags(&R.done[slot], hipEventDisableTiming));
    RPH_TRY(R.pin[slot].reserve(bytes, bytes + bytes / 2, synced));
    *hb = R.pin[slot].data();
    *slot_out = slot;
    return RPH_OK;
}

int staged(rph_ctx *ctx, int slot, hipStream_t stream)
{
    RPH_HIP_CHECK(hipEventRecord(static_cast<RaggedState *>(ctx->ragged)->done[slot], stream));
    return RPH_OK;
}

enum : uint8_t { CLS_F = 0, CLS_S = 1, CLS_R = 2 };

// the layouts rph_pdq_hash_batch_dev reads itself; the others reach every PDQ kernel as a Luma8 plane
inline bool hasher_layout(uint32_t layout) { return layout == RPH_LAYOUT_LUMA8 || layout == RPH_LAYOUT_RGB8 || layout == RPH_LAYOUT_RGBA8; }

struct AxisRef {
    bool uniform = false;
    uint32_t at = 0;  // in the axis blob, dwords
    int precision = 0;
};

constexpr size_t kLumaChunkBytes = (size_t)256 << 20;   // full-size luma planes per chunk (the uniform path's two-pass bound)
constexpr size_t kThumbChunkBytes = (size_t)1 << 30;    // thumbnails and <= 512 px luma planes per chunk (the uniform path's bound)
constexpr uint32_t kChunkImages = 1u << 20;

struct Planner {
    rph_ctx *ctx;
    const uint8_t *d_px;
    const uint64_t *offset;
    const uint32_t *w, *h, *layout;
    const size_t *row_stride;
    uint8_t *d_hash;
    float *d_quality, *d_coeffs;
    uint8_t *d_dihedral, *d_valid;
    hipStream_t stream;

    std::map<std::pair<uint32_t, uint32_t>, AxisRef> axes;  // (in, out) -> tables, built once per call
    std::vector<uint32_t> axis_blob;

    const AxisRef &axis(uint32_t in_size, uint32_t out_size)
    {
        auto it = axes.find({in_size, out_size});
        if (it != axes.end()) return it->second;
        std::vector<uint32_t> start, size;
        std::vector<int32_t> c1;
        AxisRef r;
        r.uniform = rph_resize_axis_tables(in_size, out_size, start, size, c1, &r.precision);
        if (r.uniform) {
            r.at = (uint32_t)axis_blob.size();
            axis_blob.insert(axis_blob.end(), start.begin(), start.end());
            axis_blob.insert(axis_blob.end(), size.begin(), size.end());
            for (int32_t c : c1) axis_blob.push_back((uint32_t)c);
        }
        return axes.emplace(std::make_pair(in_size, out_size), r).first->second;
    }

    // S: both sides 128..512.  R: a side > 512, thumbnail sides >= 128, uniform box axes, 32-bit offsets within the image and its luma plane.
    uint8_t classify(uint32_t i)
    {
        const uint32_t W = w[i], H = h[i];
        if (W < 128 || H < 128) return CLS_F;
        if (W <= RPH_PDQ_MAX_DIM && H <= RPH_PDQ_MAX_DIM) return CLS_S;
        uint32_t nw, nh;
        rph_pdq_target_dimensions(W, H, RPH_PDQ_MAX_DIM, &nw, &nh);
        if (nw < 128 || nh < 128) return CLS_F;
        if ((size_t)H * row_stride[i] >= ((size_t)1 << 31) || (size_t)H * align_up(W, 16) >= ((size_t)1 << 31)) return CLS_F;
        if (!axis(W, nw).uniform || !axis(H, nh).uniform) return CLS_F;
        return CLS_R;
    }

    int run_chunk(const std::vector<uint32_t> &imgs);
    int run_planes(const std::vector<uint32_t> &imgs);
};

// One chunk of class-S / class-R images: blob, luma planes and thumbnails in ctx->rz_scratch, one upload, at most three launches.
// Called with ctx->mu held.
int Planner::run_chunk(const std::vector<uint32_t> &imgs)
{
    const uint32_t m = (uint32_t)imgs.size();
    std::vector<RgDesc> desc(m);
    std::vector<uint32_t> lu_first, lu_which, rz_first, rz_which, list(m);
    uint32_t lu_blocks = 0, rz_tiles = 0;
    Layout planes;  // behind the blob
    for (uint32_t k = 0; k < m; k++) {
        const uint32_t i = imgs[k], W = w[i], H = h[i], ch = layout[i];
        const size_t rs = row_stride[i];
        RgDesc &d = desc[k];
        d = RgDesc{};
        d.src_off = offset[i];
        d.row_stride = rs;
        d.w = W;
        d.h = H;
        d.layout = ch;
        d.out = i;
        d.luma_off = RG_NONE;
        const bool large = W > RPH_PDQ_MAX_DIM || H > RPH_PDQ_MAX_DIM;
        // the streaming kernel reads whole dwords at 32-bit offsets; the resize takes Luma8 rows of any alignment
        const bool direct = ch == 1 && (large || (((uintptr_t)(d_px + offset[i]) | rs) % 4 == 0 && (size_t)H * rs < ((size_t)1 << 30)));
        if (!direct) {
            d.luma_pitch = (uint32_t)align_up(W, 16);
            d.luma_off = planes.add((size_t)d.luma_pitch * H, 16);
            lu_first.push_back(lu_blocks);
            lu_which.push_back(k);
            lu_blocks += ((W + 3) / 4 * H + 255) / 256;
        }
        if (large) {
            rph_pdq_target_dimensions(W, H, RPH_PDQ_MAX_DIM, &d.tw, &d.th);
            d.tpitch = (uint32_t)align_up(d.tw, 16);
            d.thumb_off = planes.add((size_t)d.tpitch * d.th, 16);
            const AxisRef &x = axis(W, d.tw), &y = axis(H, d.th);
            d.ax = x.at;
            d.ay = y.at;
            d.prec_x = (uint32_t)x.precision;
            d.prec_y = (uint32_t)y.precision;
            rz_first.push_back(rz_tiles);
            rz_which.push_back(k);
            rz_tiles += ((d.tw + 63) / 64) * ((d.th + 31) / 32);
        }
        list[k] = k;
    }
    lu_first.push_back(lu_blocks);
    rz_first.push_back(rz_tiles);

    // the blob: descriptors, work lists, axis tables
    Layout blob;
    const size_t o_desc = blob.add(desc.size() * sizeof(RgDesc), 16), o_luf = blob.add(lu_first.size() * 4, 4), o_luw = blob.add(lu_which.size() * 4, 4),
                 o_rzf = blob.add(rz_first.size() * 4, 4), o_rzw = blob.add(rz_which.size() * 4, 4), o_list = blob.add(list.size() * 4, 4),
                 o_axes = blob.add(axis_blob.size() * 4, 4);
    const size_t blob_bytes = align_up(blob.end(), 256);
    for (RgDesc &d : desc) {
        if (d.luma_off != RG_NONE) d.luma_off += blob_bytes;
        if (d.tw) d.thumb_off += blob_bytes;
    }
    uint8_t *hb = nullptr;
    int slot = 0;
    RPH_TRY(stage(ctx, blob_bytes, &hb, &slot));
    auto put = [&](size_t at, const void *p, size_t bytes) {
        if (bytes) std::memcpy(hb + at, p, bytes);
    };
    put(o_desc, desc.data(), desc.size() * sizeof(RgDesc));
    put(o_luf, lu_first.data(), lu_first.size() * 4);
    put(o_luw, lu_which.data(), lu_which.size() * 4);
    put(o_rzf, rz_first.data(), rz_first.size() * 4);
    put(o_rzw, rz_which.data(), rz_which.size() * 4);
    put(o_list, list.data(), list.size() * 4);
    put(o_axes, axis_blob.data(), axis_blob.size() * 4);

    RPH_TRY(ctx->rz_scratch.acquire(stream, blob_bytes + planes.end() + 16));
    uint8_t *sc = ctx->rz_scratch.data();
    ctx->rz_last.n = 0;  // (rph_debug_copy_thumbnails: the scratch no longer holds the last uniform call's thumbnails)
    RPH_HIP_CHECK(hipMemcpyAsync(sc, hb, blob.end(), hipMemcpyHostToDevice, stream));
    RPH_TRY(staged(ctx, slot, stream));
    const RgDesc *dd = reinterpret_cast<const RgDesc *>(sc + o_desc);
    auto u32 = [&](size_t at) { return reinterpret_cast<const uint32_t *>(sc + at); };
    if (lu_blocks)
        hipLaunchKernelGGL(ragged_luma_kernel, dim3(lu_blocks), dim3(256), 0, stream, d_px, sc, dd, u32(o_luf), u32(o_luw), (uint32_t)lu_which.size());
    if (rz_tiles)
        hipLaunchKernelGGL(resize_ragged_kernel, dim3(rz_tiles), dim3(64), 0, stream, d_px, sc, dd, u32(o_rzf), u32(o_rzw), (uint32_t)rz_which.size(), u32(o_axes));
    hipLaunchKernelGGL(pdq_stream_ragged_kernel, dim3(m), dim3(64), 0, stream, d_px, (const uint8_t *)sc, dd, u32(o_list), d_hash, d_quality, d_coeffs, d_dihedral,
                       d_valid);
    RPH_HIP_CHECK(hipGetLastError());
    return ctx->rz_scratch.publish(stream);
}

// Class-F images of the layouts rph_pdq_hash_batch_dev does not read (consecutive entries of imgs may be consecutive images): their Luma8
// planes into ctx->image_planes by ragged_luma_kernel, then runs of consecutive images of one size through the uniform path as Luma8.
int Planner::run_planes(const std::vector<uint32_t> &imgs)
{
    const uint32_t m = (uint32_t)imgs.size();
    std::vector<RgDesc> desc(m);
    std::vector<uint32_t> first(m + 1), which(m);
    uint32_t blocks = 0;
    Layout planes;
    for (uint32_t k = 0; k < m; k++) {
        const uint32_t i = imgs[k];
        RgDesc &d = desc[k];
        d = RgDesc{};
        d.src_off = offset[i];
        d.row_stride = row_stride[i];
        d.w = w[i];
        d.h = h[i];
        d.layout = layout[i];
        d.out = i;
        d.luma_pitch = (uint32_t)align_up(std::max(w[i], 1u), 16);
        d.luma_off = planes.add((size_t)d.luma_pitch * std::max(h[i], 1u), 16);  // (an empty image keeps its place in a run)
        first[k] = blocks;
        which[k] = k;
        const uint64_t quads = (uint64_t)((w[i] + 3) / 4) * h[i];
        if (quads + blocks * (uint64_t)256 >= ((uint64_t)1 << 32)) {
            rph_set_error("rph_image_hash_ragged: image %u (%ux%u) is too large for its luma plane", i, w[i], h[i]);
            return RPH_ERR_UNSUPPORTED;
        }
        blocks += (uint32_t)((quads + 255) / 256);
    }
    first[m] = blocks;
    Layout blob;
    const size_t o_desc = blob.add(desc.size() * sizeof(RgDesc), 16), o_first = blob.add(first.size() * 4, 4), o_which = blob.add(which.size() * 4, 4);
    const size_t blob_bytes = align_up(blob.end(), 256);
    for (RgDesc &d : desc) d.luma_off += blob_bytes;

    std::lock_guard<std::mutex> planes_lock(ctx->image_mu);  // until the last launch that reads the planes is on the stream
    uint8_t *sc = nullptr;
    {
        std::lock_guard<std::mutex> lock(ctx->mu);
        uint8_t *hb = nullptr;
        int slot = 0;
        RPH_TRY(stage(ctx, blob_bytes, &hb, &slot));
        std::memcpy(hb + o_desc, desc.data(), desc.size() * sizeof(RgDesc));
        std::memcpy(hb + o_first, first.data(), first.size() * 4);
        std::memcpy(hb + o_which, which.data(), which.size() * 4);
        RPH_TRY(ctx->image_planes.acquire(stream, blob_bytes + planes.end() + 16));
        sc = ctx->image_planes.data();
        RPH_HIP_CHECK(hipMemcpyAsync(sc, hb, blob.end(), hipMemcpyHostToDevice, stream));
        RPH_TRY(staged(ctx, slot, stream));
        if (blocks) {
            hipLaunchKernelGGL(ragged_luma_kernel, dim3(blocks), dim3(256), 0, stream, d_px, sc, reinterpret_cast<const RgDesc *>(sc + o_desc),
                               reinterpret_cast<const uint32_t *>(sc + o_first), reinterpret_cast<const uint32_t *>(sc + o_which), m);
            RPH_HIP_CHECK(hipGetLastError());
        }
    }
    for (uint32_t k = 0; k < m;) {
        const uint32_t i = imgs[k];
        uint32_t j = k + 1;
        while (j < m && imgs[j] == i + (j - k) && w[imgs[j]] == w[i] && h[imgs[j]] == h[i]) j++;
        const RgDesc &d = desc[k];
        RPH_TRY(rph_pdq_hash_batch_dev(ctx, sc + d.luma_off, j - k, w[i], h[i], 1, d.luma_pitch, (size_t)d.luma_pitch * std::max(h[i], 1u), d_hash + (size_t)i * 32,
                                       d_quality ? d_quality + i : nullptr, d_coeffs ? d_coeffs + (size_t)i * 256 : nullptr,
                                       d_dihedral ? d_dihedral + (size_t)i * 256 : nullptr, d_valid ? d_valid + i : nullptr, stream));
        k = j;
    }
    return ctx->image_planes.publish(stream);
}

}  // namespace

void rph_ragged_forget(rph_ctx *ctx)
{
    if (!ctx->ragged) return;
    RaggedState *R = static_cast<RaggedState *>(ctx->ragged);
    for (hipEvent_t e : R->done)
        if (e) {
            (void)hipEventSynchronize(e);
            (void)hipEventDestroy(e);
        }
    delete R;
    ctx->ragged = nullptr;
}

int rph_pdq_ragged_run(rph_ctx *ctx, const uint8_t *d_px, const uint64_t *offset, const uint32_t *w, const uint32_t *h, const uint32_t *layout,
                       const size_t *row_stride, uint32_t n, uint8_t *d_hash, float *d_quality, float *d_coeffs, uint8_t *d_dihedral, uint8_t *d_valid,
                       hipStream_t stream)
{
    if (n == 0) return RPH_OK;
    auto same = [&](uint32_t a, uint32_t b) { return w[a] == w[b] && h[a] == h[b] && layout[a] == layout[b] && row_stride[a] == row_stride[b]; };
    // images [first, first + count) through the uniform path if they are one geometry at one distance from each other, of a layout it reads
    auto uniform_run = [&](uint32_t first, uint32_t count, bool &took) -> int {
        took = false;
        if (!hasher_layout(layout[first])) return RPH_OK;
        const size_t one = (size_t)(h[first] ? h[first] - 1 : 0) * row_stride[first] + (size_t)w[first] * layout[first];
        size_t stride = one;
        if (count > 1) {
            if (offset[first + 1] <= offset[first]) return RPH_OK;
            stride = (size_t)(offset[first + 1] - offset[first]);
            if (stride < one) return RPH_OK;
            for (uint32_t i = first + 1; i < first + count; i++)
                if (!same(first, i) || offset[i] != offset[first] + (uint64_t)(i - first) * stride) return RPH_OK;
        }
        took = true;
        return rph_pdq_hash_batch_dev(ctx, d_px + offset[first], count, w[first], h[first], layout[first], row_stride[first], stride, d_hash + (size_t)first * 32,
                                      d_quality ? d_quality + first : nullptr, d_coeffs ? d_coeffs + (size_t)first * 256 : nullptr,
                                      d_dihedral ? d_dihedral + (size_t)first * 256 : nullptr, d_valid ? d_valid + first : nullptr, stream);
    };
    bool took = false;
    RPH_TRY(uniform_run(0, n, took));
    if (took) return RPH_OK;

    RPH_HIP_CHECK(hipSetDevice(ctx->device));
    Planner P{ctx, d_px, offset, w, h, layout, row_stride, d_hash, d_quality, d_coeffs, d_dihedral, d_valid, stream, {}, {}};
    // rph_pdq_set_kernel 0 and 5 ask for no single-pass kernel: every image is class F
    const bool single_pass = ctx->pdq_kernel != 0 && ctx->pdq_kernel != 5;
    std::vector<uint8_t> cls(n, CLS_F);
    if (single_pass)
        for (uint32_t i = 0; i < n; i++) cls[i] = P.classify(i);
    {
        std::lock_guard<std::mutex> lock(ctx->mu);
        std::vector<uint32_t> imgs;
        size_t luma = 0, thumbs = 0;
        for (uint32_t i = 0; i < n; i++) {
            if (cls[i] == CLS_F) continue;
            size_t l = 0, t = 0;
            if (cls[i] == CLS_S) {
                t = align_up(w[i], 16) * (size_t)h[i];
            } else {
                l = layout[i] == RPH_LAYOUT_LUMA8 ? 0 : align_up(w[i], 16) * (size_t)h[i];
                t = (size_t)512 * 512;
            }
            if (!imgs.empty() && (luma + l > kLumaChunkBytes || thumbs + t > kThumbChunkBytes || imgs.size() >= kChunkImages)) {
                RPH_TRY(P.run_chunk(imgs));
                imgs.clear();
                luma = thumbs = 0;
            }
            imgs.push_back(i);
            luma += l;
            thumbs += t;
        }
        if (!imgs.empty()) RPH_TRY(P.run_chunk(imgs));
    }
    // class F: runs of equal geometry through the uniform path, each into its images' own output slots; the images of the other layouts
    // as Luma8 planes, a chunk of them at a time
    std::vector<uint32_t> planes;
    size_t plane_bytes = 0;
    auto flush = [&]() -> int {
        if (planes.empty()) return RPH_OK;
        const int rc = P.run_planes(planes);
        planes.clear();
        plane_bytes = 0;
        return rc;
    };
    for (uint32_t i = 0; i < n;) {
        if (cls[i] != CLS_F) {
            i++;
            continue;
        }
        if (!hasher_layout(layout[i])) {
            const size_t bytes = align_up(std::max(w[i], 1u), 16) * (size_t)std::max(h[i], 1u);
            if (!planes.empty() && (plane_bytes + bytes > kLumaChunkBytes || planes.size() >= kChunkImages)) RPH_TRY(flush());
            planes.push_back(i);
            plane_bytes += bytes;
            i++;
            continue;
        }
        uint32_t j = i + 1;
        while (j < n && cls[j] == CLS_F && same(i, j)) j++;
        for (uint32_t count = j - i; count >= 1; count = 1) {  // the whole run if its images lie evenly, else its first image alone
            RPH_TRY(uniform_run(i, count, took));
            if (took) {
                i += count;
                break;
            }
        }
    }
    return flush();
}

int rph_image_ragged_run(rph_ctx *ctx, const uint8_t *d_px, const uint64_t *offset, const uint32_t *w, const uint32_t *h, const uint32_t *layout,
                         const size_t *row_stride, uint32_t n, uint8_t *d_hash, float *d_quality, float *d_coeffs, uint8_t *d_dihedral, uint8_t *d_valid,
                         uint8_t *d_pixel_hash, hipStream_t stream)
{
    if (n == 0) return RPH_OK;
    if (d_hash) RPH_TRY(rph_pdq_ragged_run(ctx, d_px, offset, w, h, layout, row_stride, n, d_hash, d_quality, d_coeffs, d_dihedral, d_valid, stream));
    if (!d_pixel_hash) return RPH_OK;
    // the pixel hashes: the plan and the group values in the context's BLAKE3 scratch, one upload, one or two launches
    std::vector<RphPixelImage> desc;
    std::vector<uint32_t> group_first;
    if (!rph_pixel_hash_ragged_plan(offset, w, h, layout, row_stride, n, desc, group_first)) {
        rph_set_error("rph_image_hash_ragged: call too large");
        return RPH_ERR_UNSUPPORTED;
    }
    const uint32_t groups = group_first[n];
    const bool multi_group = groups > n;  // every image has at least one group
    Layout blob;
    const size_t o_desc = blob.add(desc.size() * sizeof(RphPixelImage), 16), o_first = blob.add(group_first.size() * 4, 4);
    const size_t blob_bytes = align_up(blob.end(), 256), need = blob_bytes + (multi_group ? (size_t)groups * 32 : 0);
    RPH_HIP_CHECK(hipSetDevice(ctx->device));
    std::lock_guard<std::mutex> lock(ctx->mu);
    uint8_t *hb = nullptr;
    int slot = 0;
    RPH_TRY(stage(ctx, blob_bytes, &hb, &slot));
    std::memcpy(hb + o_desc, desc.data(), desc.size() * sizeof(RphPixelImage));
    std::memcpy(hb + o_first, group_first.data(), group_first.size() * 4);
    RPH_TRY(ctx->b3_scratch.acquire(stream, need, need + need / 4));
    uint8_t *sc = ctx->b3_scratch.data();
    RPH_HIP_CHECK(hipMemcpyAsync(sc, hb, blob.end(), hipMemcpyHostToDevice, stream));
    RPH_TRY(staged(ctx, slot, stream));
    RPH_TRY(rph_launch_pixel_hash_ragged(d_px, reinterpret_cast<const RphPixelImage *>(sc + o_desc), reinterpret_cast<const uint32_t *>(sc + o_first), n, groups,
                                         multi_group, reinterpret_cast<uint32_t *>(sc + blob_bytes), d_pixel_hash, stream));
    return ctx->b3_scratch.publish(stream);
}

extern "C" int rph_image_hash_ragged_dev(rph_ctx *ctx, const void *d_px, const uint64_t *offset, const uint32_t *w, const uint32_t *h, const uint32_t *layout,
                                         const size_t *row_stride, uint32_t n, void *d_hash32, void *d_quality, void *d_coeffs, void *d_dihedral, void *d_valid,
                                         void *d_pixel_hash32, void *stream)
{
    return rph_guarded("rph_image_hash_ragged_dev", [&]() -> int {
        if (ctx && n == 0) return RPH_OK;
        if (!ctx || (!d_hash32 && !d_pixel_hash32) || (!d_hash32 && (d_quality || d_coeffs || d_dihedral || d_valid))) {
            rph_set_error("rph_image_hash_ragged_dev: null argument (no output, or PDQ outputs without d_hash32)");
            return RPH_ERR_INVALID_ARG;
        }
        if (!d_px || !offset || !w || !h || !layout || !row_stride) {
            rph_set_error("rph_image_hash_ragged_dev: null argument");
            return RPH_ERR_INVALID_ARG;
        }
        for (uint32_t i = 0; i < n; i++) {
            const uint32_t bpp = rph_layout_bytes(layout[i]);
            const bool wide = layout[i] > 16;
            if (!bpp || row_stride[i] < (size_t)w[i] * bpp || (wide && ((((uintptr_t)d_px + offset[i]) | row_stride[i]) & 1)) ||
                (uint64_t)w[i] * h[i] > ((uint64_t)1 << 40)) {
                rph_set_error("rph_image_hash_ragged_dev: invalid argument (image %u: %ux%u layout %u row_stride=%zu offset=%llu)", i, w[i], h[i], layout[i],
                              row_stride[i], (unsigned long long)offset[i]);
                return RPH_ERR_INVALID_ARG;
            }
        }
        return rph_image_ragged_run(ctx, (const uint8_t *)d_px, offset, w, h, layout, row_stride, n, (uint8_t *)d_hash32, (float *)d_quality, (float *)d_coeffs,
                                    (uint8_t *)d_dihedral, (uint8_t *)d_valid, (uint8_t *)d_pixel_hash32, stream ? (hipStream_t)stream : ctx->stream);
    });
}

extern "C" int rph_pdq_hash_ragged_dev(rph_ctx *ctx, const void *d_px, const uint64_t *offset, const uint32_t *w, const uint32_t *h, const uint32_t *channels,
                                       const size_t *row_stride, uint32_t n, void *d_hash32, void *d_quality, void *d_coeffs, void *d_dihedral, void *d_valid,
                                       void *stream)
{
    return rph_guarded("rph_pdq_hash_ragged_dev", [&]() -> int {
        if (ctx && n == 0) return RPH_OK;
        if (!ctx || !d_hash32 || !d_px || !offset || !w || !h || !channels || !row_stride) {
            rph_set_error("rph_pdq_hash_ragged_dev: null argument");
            return RPH_ERR_INVALID_ARG;
        }
        for (uint32_t i = 0; i < n; i++)
            if ((channels[i] != 1 && channels[i] != 3 && channels[i] != 4) || row_stride[i] < (size_t)w[i] * channels[i]) {
                rph_set_error("rph_pdq_hash_ragged_dev: invalid argument (image %u: %ux%ux%u row_stride=%zu)", i, w[i], h[i], channels[i], row_stride[i]);
                return RPH_ERR_INVALID_ARG;
            }
        return rph_pdq_ragged_run(ctx, (const uint8_t *)d_px, offset, w, h, channels, row_stride, n, (uint8_t *)d_hash32, (float *)d_quality, (float *)d_coeffs,
                                  (uint8_t *)d_dihedral, (uint8_t *)d_valid, stream ? (hipStream_t)stream : ctx->stream);
    });
}
