// pdq_stream.hip -- streaming single-pass PDQ hash of Luma8 images of any geometry 128..512 x 128..512 for gfx950:
// the hasher behind the pre-downsample (every photo's thumbnail), behind the JPEG decode, and for Luma8 inputs that are not 512x512.
//
// Replaces generate_pdq_from_luma (/root/reference/src/pdqhash.rs:238-262): u8 -> f32 (:244), jarosz_filter_float (2 x rows, cols;
// :341-426), decimate_float (:428-443), and feeds the shared tail (quality :445-460, DCT :306-336, median / hash :59-124; pdq_tail.hpp).
// The image is read once; nothing but the outputs is written (the multi-pass kernels of pdq_kernels.hip move 3.2 MB per 512x344 thumbnail).
//
// One wave owns one image and never synchronises with another wave.  It walks the image in bands of 56 rows x strips of 64 columns:
//   A  pass-1 rows.  The inputs are integers, so every window sum is exact in any order and out = fl(S / n): S comes from the matrix
//      pipe.  v_mfma_i32_32x32x32_i8 with 32 image rows x 64 bytes straight from memory as A (lane = row) and a 0/1 band matrix as B
//      yields S with lane = COLUMN and 16 rows per lane; v_permlane32_swap of two column blocks gives every lane all 32 rows of one
//      column -- the layout the column recurrence wants, with no transposition.  (Bytes are unsigned, the instruction is signed:
//      bytes ^ 0x80, and 128 n comes back through spare K slots: A = 64 there, B = 2 n.)
//   B  pass-1 columns, lane = column: the reference's recurrence step for step (sum += in[t]; sum -= in[t - win]; out = sum / cur),
//      the window's leaving element out of registers (rows of the block above: the first block of a band re-derives the 8 rows
//      above it, so only the running sums persist between bands: 2 KB of LDS).  Outputs go to a 56 x 64 f32 tile in LDS.
//   C  pass-2 rows, lane = row of the band: the tile row comes back as 16 ds_read_b128, the recurrence runs over registers, and only
//      the columns decimate_float keeps are divided and kept (a 32-entry register file, indexed through s_set_gpr_idx).
//   D  pass-2 columns on the kept columns, lane = kept column: the samples are transposed through the (then dead) tile; only the
//      rows decimate_float keeps are divided, and each goes straight into the streaming tail (DCT pass 1 + quality).
// Exactness: every f32 operation of the reference is executed with the same operands in the same order; positions outside the
// image enter the recurrences as +0.0 (x + 0 = x and x - 0 = x exactly; -0.0 cannot arise from sums of non-negative values), and
// sum / cur for cur = 1..8 is Markstein's 1 mul + 2 fma sequence, which IS the IEEE quotient for every normal |sum| < 4096
// (checked exhaustively on the CPU, tools/check_div_small.c).  No FMA contraction anywhere else (-ffp-contract=off).
#include "pdq_stream_stages.hpp"

namespace {

__global__ void __launch_bounds__(64, 2) pdq_stream_kernel(const uint8_t *__restrict__ px, uint32_t n, uint32_t w_, uint32_t h_, size_t row_stride, size_t image_stride,
                                                           uint8_t *hash, float *quality, float *coeffs, uint8_t *dihedral, uint8_t *valid)
{
    __shared__ __attribute__((aligned(16))) float lds[ST_LDS_FLOATS];
    const uint32_t img = blockIdx.x;
    StGeo g;
    g.W = (int)w_;
    g.H = (int)h_;
    g.win_r = (g.W + 63) / 64;
    g.win_c = (g.H + 63) / 64;
    const int half_r = (g.win_r + 2) / 2, half_c = (g.win_c + 2) / 2;
    g.lead_r = half_r - 1;
    g.a_r = g.win_r - half_r;
    g.lead_c = half_c - 1;
    g.ns_b = (g.W + 63) / 64;
    g.ns_c = ((127 * g.W) / 128 + g.lead_r) / 64 + 1;
    g.nb = (g.H + 2 * g.lead_c + ST_BAND - 1) / ST_BAND;
    const int rs32 = (int)row_stride;

    StWave w;
    w.lds = lds;
    w.lane = threadIdx.x;
    w.dsum = 0.0f;
#pragma unroll
    for (int j = 0; j < 8; j++) w.dprev[j] = 0.0f;
    w.smp = 0.0f;
    rph::tail_init(w.tail);
    w.want_quality = quality != nullptr;
#pragma unroll
    for (int i = 0; i < 8; i++) lds[ST_OFF_SUMS + 64 * i + w.lane] = 0.0f;

    // The range check works on whole dwords: the image ends with the aligned dword that holds its last pixel (rows start on dword
    // boundaries, so that dword never leaves the page of the last pixel; what follows the pixel in it is under no window).
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t *>(px + (size_t)img * image_stride), 0,
                                                                        (int)((size_t)(g.H - 1) * row_stride + (((size_t)g.W + 3) & ~(size_t)3)), 0x00027000);

    int ni = 0;  // next kept row (decimate_float's row index)
#pragma unroll 1
    for (int k = 0; k < g.nb; k++) {
        const int T0 = ST_BAND * k;
        w.csum = 0.0f;
#pragma unroll
        for (int j = 0; j < 8; j++) w.cprev[j] = 0.0f;
        int jn = 0, base = 0, cnt = 0;
        unsigned long long em = st_emit_mask(g, 0, jn);
        if (!(T0 >= g.win_c - 1 && T0 + ST_BAND - 1 <= g.H - 1) && w.lane < ST_BAND) {
            const int c = st_count(T0 + w.lane, g.H, g.win_c);
            lds[ST_OFF_DIV + 2 * w.lane] = c_div[c][0];
            lds[ST_OFF_DIV + 2 * w.lane + 1] = c_div[c][1];
        }
        st_fence();
#pragma unroll 1
        for (int s = 0; s < g.ns_c; s++) {
            const int c0 = 64 * s;
            if (s < g.ns_b) {
                switch (g.win_c) {
                case 2: st_ab_stage<2>(w, rs, g, rs32, T0, c0); break;
                case 3: st_ab_stage<3>(w, rs, g, rs32, T0, c0); break;
                case 4: st_ab_stage<4>(w, rs, g, rs32, T0, c0); break;
                case 5: st_ab_stage<5>(w, rs, g, rs32, T0, c0); break;
                case 6: st_ab_stage<6>(w, rs, g, rs32, T0, c0); break;
                case 7: st_ab_stage<7>(w, rs, g, rs32, T0, c0); break;
                default: st_ab_stage<8>(w, rs, g, rs32, T0, c0); break;
                }
            } else {  // past the last pixel: the recurrence only subtracts
#pragma unroll
                for (int r = 0; r < ST_BAND; r++) lds[r * ST_TP + w.lane] = 0.0f;
            }
            st_fence();
            switch (g.win_r) {
            case 2: st_c_stage<2>(w, g, c0, em, cnt); break;
            case 3: st_c_stage<3>(w, g, c0, em, cnt); break;
            case 4: st_c_stage<4>(w, g, c0, em, cnt); break;
            case 5: st_c_stage<5>(w, g, c0, em, cnt); break;
            case 6: st_c_stage<6>(w, g, c0, em, cnt); break;
            case 7: st_c_stage<7>(w, g, c0, em, cnt); break;
            default: st_c_stage<8>(w, g, c0, em, cnt); break;
            }
            st_fence();
            // the next strip's kept columns; the register file holds 32
            em = st_emit_mask(g, c0 + 64, jn);
            const bool last = s == g.ns_c - 1;
            if (cnt > 0 && (last || cnt + __builtin_popcountll(em) > 32)) {
                st_d_pass(w, g, T0, base, cnt, ni, 64);
                base += cnt;
                cnt = 0;
            }
        }
        // kept rows this band has produced: row ri leaves at pass-2 column step ri + lead_c = band row ri + 2 lead_c - T0
        while (ni < 64 && ((2 * ni + 1) * g.H) / 128 + 2 * g.lead_c < T0 + ST_BAND) ni++;
    }
    st_fence();
    rph::tail_finish(w.tail, lds, w.lane, hash + (size_t)img * 32, quality ? quality + img : nullptr, coeffs ? coeffs + (size_t)img * 256 : nullptr,
                     dihedral ? dihedral + (size_t)img * 256 : nullptr);
    if (valid && w.lane == 0) valid[img] = 1;
}

// to_luma601 (pdqhash.rs:268-284) of Rgb8 / Rgba8 pixels into a Luma8 plane with 16-byte aligned rows: four pixels per thread, whole dwords in
// and out.  The streaming kernel takes its A operand -- 16 luma bytes per lane -- straight from memory, so colour inputs pass through this
// plane (read 3 or 4 bytes, write 1, read 1 per pixel); so do Luma8 inputs whose rows do not start on dword boundaries (CH = 1: a copy).
// Source rows of any alignment: aligned dwords + v_alignbyte.
template <int CH>
__global__ void __launch_bounds__(256) st_luma_kernel(const uint8_t *__restrict__ px, uint32_t w, uint32_t h, size_t row_stride, size_t image_stride,
                                                      uint8_t *__restrict__ out, uint32_t out_pitch, size_t out_stride)
{
    const uint32_t quads = (w + 3) / 4;
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    if (t >= quads * h) return;
    const uint32_t y = t / quads, q = t - y * quads;
    const uint8_t *p = px + (size_t)blockIdx.y * image_stride + (size_t)y * row_stride + (size_t)q * 4 * CH;
    const uint32_t o = st_luma_quad<CH>(p, q, w);
    reinterpret_cast<uint32_t *>(out + (size_t)blockIdx.y * out_stride + (size_t)y * out_pitch)[q] = o;
}

}  // namespace

bool rph_pdq_stream_supported(const uint8_t *d_px, uint32_t w, uint32_t h, uint32_t channels, size_t row_stride, size_t image_stride)
{
    return channels == 1 && w >= 128 && w <= 512 && h >= 128 && h <= 512 && (row_stride % 4) == 0 && (image_stride % 4) == 0 && ((uintptr_t)d_px % 4) == 0 &&
           (size_t)h * row_stride < ((size_t)1 << 30);
}

// Rgb8 / Rgba8 images of the same geometries, and Luma8 images whose rows do not lie on dword boundaries: a Luma8 plane with aligned rows
// in the context's scratch, then the streaming kernel.  Called with ctx->mu held.
bool rph_pdq_stream_color_supported(const uint8_t *d_px, uint32_t w, uint32_t h, uint32_t channels, size_t row_stride, size_t image_stride)
{
    (void)d_px, (void)row_stride, (void)image_stride;  // any alignment
    return (channels == 1 || channels == 3 || channels == 4) && w >= 128 && w <= 512 && h >= 128 && h <= 512;
}

int rph_launch_pdq_stream_color(rph_ctx *ctx, const uint8_t *d_px, uint32_t n, uint32_t w, uint32_t h, uint32_t channels, size_t row_stride, size_t image_stride,
                                uint8_t *d_hash, float *d_quality, float *d_coeffs, uint8_t *d_dihedral, uint8_t *d_valid, hipStream_t stream)
{
    if (n == 0) return RPH_OK;
    const uint32_t pitch = (w + 15u) & ~15u;
    const size_t plane = (size_t)pitch * h;
    uint32_t chunk = (uint32_t)(((size_t)1 << 30) / plane);
    chunk = chunk > n ? n : (chunk > 65535u ? 65535u : chunk);
    const size_t need = plane * chunk;
    RPH_TRY(ctx->scratch.acquire(stream, need));
    uint8_t *luma = ctx->scratch.data();
    const uint32_t quads = (w + 3) / 4;
    for (uint32_t first = 0; first < n; first += chunk) {
        const uint32_t m = (n - first) < chunk ? (n - first) : chunk;
        const dim3 grid((quads * h + 255) / 256, m);
        const uint8_t *src = d_px + (size_t)first * image_stride;
        if (channels == 1)
            hipLaunchKernelGGL(st_luma_kernel<1>, grid, dim3(256), 0, stream, src, w, h, row_stride, image_stride, luma, pitch, plane);
        else if (channels == 3)
            hipLaunchKernelGGL(st_luma_kernel<3>, grid, dim3(256), 0, stream, src, w, h, row_stride, image_stride, luma, pitch, plane);
        else
            hipLaunchKernelGGL(st_luma_kernel<4>, grid, dim3(256), 0, stream, src, w, h, row_stride, image_stride, luma, pitch, plane);
        hipLaunchKernelGGL(pdq_stream_kernel, dim3(m), dim3(64), 0, stream, (const uint8_t *)luma, m, w, h, (size_t)pitch, plane, d_hash + (size_t)first * 32,
                           d_quality ? d_quality + first : nullptr, d_coeffs ? d_coeffs + (size_t)first * 256 : nullptr,
                           d_dihedral ? d_dihedral + (size_t)first * 256 : nullptr, d_valid ? d_valid + first : nullptr);
        RPH_HIP_CHECK(hipGetLastError());
    }
    return ctx->scratch.publish(stream);
}

int rph_launch_pdq_stream(rph_ctx *ctx, const uint8_t *d_px, uint32_t n, uint32_t w, uint32_t h, size_t row_stride, size_t image_stride, uint8_t *d_hash,
                          float *d_quality, float *d_coeffs, uint8_t *d_dihedral, uint8_t *d_valid, hipStream_t stream)
{
    (void)ctx;
    if (n == 0) return RPH_OK;
    hipLaunchKernelGGL(pdq_stream_kernel, dim3(n), dim3(64), 0, stream, d_px, n, w, h, row_stride, image_stride, d_hash, d_quality, d_coeffs, d_dihedral, d_valid);
    RPH_HIP_CHECK(hipGetLastError());
    return RPH_OK;
}
