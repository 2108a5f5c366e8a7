// resize_mfma.hpp -- the pre-downsample's two box passes on the matrix pipe as a device function of one wave's task, shared by
// resize_mfma_kernel (one geometry per launch, resize_kernels.hip) and resize_ragged_kernel (a geometry per image, pdq_ragged.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

struct DevAxis {
    const uint32_t *start, *size;
    const int16_t *coef;
    const int32_t *c1;
    int window, precision;
};

__device__ __forceinline__ uint8_t clip8(int32_t v, int precision)
{
    v >>= precision;
    return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// ---- both passes on the matrix pipe (Luma8 sources; the default).  A box convolution is a window SUM times one coefficient:
//   clip8((half + sum_i in[start + i] * k) >> p)  =  clip8((half + k * S) >> p),  S = the window sum (integer arithmetic: the same number),
// and window sums of many outputs are one product with a 0/1 band matrix.  One wave owns 32 output rows x 64 output columns:
//   pass 1  v_mfma_i32_32x32x32_i8, A = 32 source rows x 32 source bytes straight from memory (lane = row), B = the band matrix of 32 output
//           columns: the sums arrive with lane = output column and the 32 source rows spread over 16 registers x 2 lane halves -- rounded,
//           clipped and packed to bytes that is exactly the B operand layout of
//   pass 2  the same instruction with A = the band matrix of the 32 output rows over those 32 source rows: lane = output column, registers =
//           output rows; v_permlane32_swap gives every lane all 32 rows of one of the 64 columns, and a row is stored as 64 adjacent bytes.
// Nothing goes through LDS.  (Bytes are unsigned, the instruction is signed: operands ^ 0x80, and 128 x the window size comes back in the
// rounding constant.)  Rows of any alignment: aligned dwords + v_alignbyte, so the range check of the buffer resource never cuts a pixel.
typedef int rz_v4i __attribute__((ext_vector_type(4)));
typedef int rz_v16i __attribute__((ext_vector_type(16)));
typedef unsigned int rz_v4u __attribute__((ext_vector_type(4)));
constexpr int RZ_KG = 6;  // K steps per group of loads

// bits [lo, hi) of a 16-slot group as 16 bytes of 0 / 1
__device__ __forceinline__ rz_v4i band16(int lo, int hi)
{
    lo = lo < 0 ? 0 : (lo > 16 ? 16 : lo);
    hi = hi < 0 ? 0 : (hi > 16 ? 16 : hi);
    const uint32_t m = hi > lo ? ((1u << hi) - 1u) & ~((1u << lo) - 1u) : 0u;
    rz_v4i r;
#pragma unroll
    for (int q = 0; q < 4; q++) r[q] = (int)((((m >> (4 * q)) & 15u) * 0x00204081u) & 0x01010101u);
    return r;
}

// One wave: output rows r0 .. r0 + 31 x output columns o0 .. o0 + 63 of the nw x nh thumbnail `out_img` (rows dst_pitch bytes apart) of the
// w x h Luma8 image at `base` (any alignment, rows row_stride bytes apart, h * row_stride < 2^31); ax / ay: uniform box axes.
__device__ __forceinline__ void rz_mfma_tile(const uint8_t *__restrict__ base, const uint32_t w, const uint32_t h, const size_t row_stride, const uint32_t nw, const uint32_t nh,
                                             const DevAxis &ax, const DevAxis &ay, const uint32_t r0, const uint32_t o0, uint8_t *__restrict__ out_img, const uint32_t dst_pitch)
{
    const int lane = threadIdx.x, n = lane & 31, kh = lane >> 5;
    // the image as a buffer of whole dwords around its bytes
    const uint32_t mis = (uint32_t)(reinterpret_cast<uintptr_t>(base) & 3u);
    const uint32_t bytes = (uint32_t)((size_t)(h - 1) * row_stride + w);
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t *>(base - mis), 0, (int)((mis + bytes + 3u) & ~3u), 0x00027000);

    // source window of the task (uniform)
    const uint32_t o_last = min(o0 + 63u, nw - 1u), r_last = min(r0 + 31u, nh - 1u);
    const int x_lo = (int)ax.start[o0] & ~15, x_hi = (int)(ax.start[o_last] + ax.size[o_last]);
    const int y_lo = (int)ay.start[r0], y_hi = (int)(ay.start[r_last] + ay.size[r_last]);
    const int n_ks = (x_hi - x_lo + 31) / 32, n_yb = (y_hi - y_lo + 31) / 32;

    // per-lane tables of pass 1: the two column blocks' windows in slots of the lane's own half, coefficient and rounding constant
    int xs[2], xe[2], cx[2], c0[2], ks_lo[2], ks_hi[2];
#pragma unroll
    for (int cb = 0; cb < 2; cb++) {
        const uint32_t o = o0 + 32 * cb + n, oc = min(o, nw - 1u);
        const int st = (int)ax.start[oc], sz = o < nw ? (int)ax.size[oc] : 0;
        xs[cb] = st - x_lo - 16 * kh;
        xe[cb] = xs[cb] + sz;
        cx[cb] = ax.c1[oc];
        c0[cb] = (1 << (ax.precision - 1)) + 128 * sz * cx[cb];
        // K steps that meet this block's windows (uniform)
        const uint32_t ob0 = min(o0 + 32u * cb, nw - 1u), ob1 = min(o0 + 32u * cb + 31u, nw - 1u);
        ks_lo[cb] = ((int)ax.start[ob0] - x_lo) / 32;
        ks_hi[cb] = ((int)(ax.start[ob1] + ax.size[ob1]) - x_lo + 31) / 32;
        if (o0 + 32u * cb >= nw) ks_hi[cb] = ks_lo[cb] = 0;
    }
    // pass 2: this lane's output row as an A-operand row, its window relative to the first source row
    const uint32_t rr = min(r0 + (uint32_t)n, nh - 1u);
    const int ys = (int)ay.start[rr] - y_lo, ye = ys + (r0 + (uint32_t)n < nh ? (int)ay.size[rr] : 0);

    rz_v4i bx0[2][RZ_KG];  // band matrices of K steps 0 .. RZ_KG - 1
#pragma unroll
    for (int cb = 0; cb < 2; cb++)
#pragma unroll
        for (int u = 0; u < RZ_KG; u++) bx0[cb][u] = band16(xs[cb] - 32 * u, xe[cb] - 32 * u);
    const bool unaligned = (mis | (uint32_t)(row_stride & 3)) != 0;  // rows on dword boundaries: the 16 bytes of a step are four whole dwords
    // pass 2's per-row constants: lane n holds those of row r0 + n (read back with v_readlane: the row of a register is static)
    const int my_cy = ay.c1[rr], my_sz = (int)ay.size[rr];

    // One group of K steps: the group's loads go out together; every step multiplies into BOTH column blocks (a block whose windows the
    // step does not meet has an all-zero band matrix there: no branch, no copies of the accumulators).
    auto k_group = [&](int ks0, uint32_t row_off, bool row_ok, bool first, rz_v16i(&acc1)[2]) {
        rz_v4u d4[RZ_KG];
        uint32_t d5[RZ_KG], sh[RZ_KG];
#pragma unroll
        for (int u = 0; u < RZ_KG; u++) {
            const uint32_t a = row_off + 32u * (uint32_t)(ks0 + u), al = (row_ok && ks0 + u < n_ks) ? a & ~3u : 0x80000000u;
            sh[u] = a & 3u;
            d4[u] = __builtin_amdgcn_raw_buffer_load_b128(rs, al, 0, 0);
            d5[u] = 0;
            if (unaligned) d5[u] = __builtin_amdgcn_raw_buffer_load_b32(rs, al + 16u, 0, 0);
        }
#pragma unroll
        for (int u = 0; u < RZ_KG; u++) {
            rz_v4i av;
            av[0] = (int)(__builtin_amdgcn_alignbyte(d4[u][1], d4[u][0], sh[u]) ^ 0x80808080u);
            av[1] = (int)(__builtin_amdgcn_alignbyte(d4[u][2], d4[u][1], sh[u]) ^ 0x80808080u);
            av[2] = (int)(__builtin_amdgcn_alignbyte(d4[u][3], d4[u][2], sh[u]) ^ 0x80808080u);
            av[3] = (int)(__builtin_amdgcn_alignbyte(d5[u], d4[u][3], sh[u]) ^ 0x80808080u);
#pragma unroll
            for (int cb = 0; cb < 2; cb++)
                acc1[cb] = __builtin_amdgcn_mfma_i32_32x32x32_i8(av, first ? bx0[cb][u] : band16(xs[cb] - 32 * (ks0 + u), xe[cb] - 32 * (ks0 + u)), acc1[cb], 0, 0, 0);
        }
    };

    rz_v16i acc2[2];
#pragma unroll
    for (int cb = 0; cb < 2; cb++) acc2[cb] = rz_v16i{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};

#pragma unroll 1
    for (int b = 0; b < n_yb; b++) {
        const int yb = y_lo + 32 * b, y = yb + n;
        const bool row_ok = y < y_hi && y < (int)h;
        const uint32_t row_off = mis + (uint32_t)y * (uint32_t)row_stride + (uint32_t)x_lo + 16u * (uint32_t)kh;
        rz_v16i acc1[2];
#pragma unroll
        for (int cb = 0; cb < 2; cb++) acc1[cb] = rz_v16i{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        k_group(0, row_off, row_ok, true, acc1);
#pragma unroll 1
        for (int ks0 = RZ_KG; ks0 < n_ks; ks0 += RZ_KG) k_group(ks0, row_off, row_ok, false, acc1);  // (sources beyond ~2.9 x the thumbnail)
        // band matrix of the output rows over source rows yb + 8 q + 4 kh + i (slot (kh, 4 q + i))
        rz_v4i by;
        {
            const int lo = ys - 32 * b, hi = ye - 32 * b;
            const int l2 = lo < 0 ? 0 : (lo > 32 ? 32 : lo), h2 = hi < 0 ? 0 : (hi > 32 ? 32 : hi);
            const uint32_t m = h2 > l2 ? (uint32_t)((1ull << h2) - 1ull) & ~(uint32_t)((1ull << l2) - 1ull) : 0u;
#pragma unroll
            for (int q = 0; q < 4; q++) by[q] = (int)((((m >> (8 * q + 4 * kh)) & 15u) * 0x00204081u) & 0x01010101u);
        }
#pragma unroll
        for (int cb = 0; cb < 2; cb++) {
            rz_v4i hb;
#pragma unroll
            for (int q = 0; q < 4; q++) {
                uint32_t d = 0;
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    int v = (__mul24(acc1[cb][4 * q + i], cx[cb]) + c0[cb]) >> ax.precision;  // |sum| < 2^15, coefficient <= 2^15
                    asm volatile("" : "+v"(v));  // (opaque between shift and clamp: ROCm 7.2 fuses them into v_ashr_pk_u8_i32 and then ORs bytes into bits 16..31 of its result as if the instruction cleared them)
                    v = v < 0 ? 0 : (v > 255 ? 255 : v);
                    d |= (uint32_t)v << (8 * i);
                }
                hb[q] = (int)(d ^ 0x80808080u);
            }
            acc2[cb] = __builtin_amdgcn_mfma_i32_32x32x32_i8(by, hb, acc2[cb], 0, 0, 0);
        }
    }
    // lane l: column o0 + l; rows r0 + 8 q + i from P[4 q + i], r0 + 8 q + 4 + i from R[4 q + i]
    const uint32_t o = o0 + (uint32_t)lane;
    uint8_t *out = out_img + (size_t)r0 * dst_pitch + o;
    const int half_y = 1 << (ay.precision - 1);
    int res[32];
#pragma unroll
    for (int j = 0; j < 16; j++) {
        const auto sw = __builtin_amdgcn_permlane32_swap(acc2[0][j], acc2[1][j], false, false);
#pragma unroll
        for (int t = 0; t < 2; t++) {
            const int row = 8 * (j >> 2) + 4 * t + (j & 3);
            const int cy = __builtin_amdgcn_readlane(my_cy, row), sz = __builtin_amdgcn_readlane(my_sz, row);
            int v = (__mul24((int)sw[t] + 128 * sz, cy) + half_y) >> ay.precision;
            asm volatile("" : "+v"(v));
            res[row] = v < 0 ? 0 : (v > 255 ? 255 : v);
        }
    }
    if (o < nw) {
#pragma unroll
        for (int row = 0; row < 32; row++)
            if (r0 + (uint32_t)row < nh) out[(uint32_t)row * dst_pitch] = (uint8_t)res[row];  // (uniform)
    }
}

}  // namespace
