// pdq_stream_stages.hpp -- the stages of the streaming single-pass PDQ hash (pdq_stream.hip has the description), shared by the two
// kernels that run them: pdq_stream_kernel (one geometry per launch, pdq_stream.hip) and pdq_stream_ragged_kernel (a geometry per
// image, from a descriptor; pdq_ragged.hip).  Device code only; every function is inlined into the kernel that calls it.
#pragma once
#include "pdq_tail.hpp"
#include "rph_internal.h"

namespace {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));
typedef unsigned int v4u __attribute__((ext_vector_type(4)));
typedef float f32x32 __attribute__((ext_vector_type(32)));

constexpr int ST_BAND = 56;                        // recurrence steps (rows) per band
constexpr int ST_TP = 68;                          // tile pitch in floats: 16-byte rows, conflict-free ds_read_b128 with lane = row
constexpr int ST_TILE_FLOATS = 64 * ST_TP;         // 17 408 B (rows 56..63 are never written)
constexpr int ST_XP = 65;                          // pitch of the sample transposition buffer [32 slots][8 rows above + 56]
constexpr int ST_OFF_SUMS = ST_TILE_FLOATS;        // pass-1 column sums, one per image column
constexpr int ST_OFF_EDGE = ST_OFF_SUMS + 512;     // kept rows of the last lane of a D pass, for the next pass's horizontal gradient
constexpr int ST_OFF_DIV = ST_OFF_EDGE + 32;       // (cur, 1 / cur) of the 56 steps of a band that touches the image's first or last rows
constexpr int ST_LDS_FLOATS = ST_OFF_DIV + 2 * ST_BAND;  // 20 032 B -> 8 waves per CU
static_assert(32 * ST_XP <= ST_TILE_FLOATS, "transposition buffer lives in the dead tile");
static_assert(rph::TAIL_LDS_FLOATS <= ST_TILE_FLOATS, "tail scratch lives in the dead tile");

// (cur, 1 / cur) for cur = 1..8
__constant__ float c_div[9][2] = {{1.0f, 1.0f},        {1.0f, 1.0f},        {2.0f, 0.5f},        {3.0f, 1.0f / 3.0f}, {4.0f, 0.25f},
                                  {5.0f, 1.0f / 5.0f}, {6.0f, 1.0f / 6.0f}, {7.0f, 1.0f / 7.0f}, {8.0f, 0.125f}};

struct StGeo {
    int W, H;
    int win_r, lead_r, a_r;  // window along rows, half - 1, win - half   (pdqhash.rs:246, :351-357)
    int win_c, lead_c;       // the same along columns
    int ns_b;                // strips that hold pixels
    int ns_c;                // strips the row recurrence walks (its last outputs come lead_r steps after the last pixel)
    int nb;                  // bands
};

__device__ __forceinline__ void st_fence() { asm volatile("" ::: "memory"); }  // one wave = one workgroup: the LDS keeps a wave's accesses in order

// IEEE N / d for d = 1..8 and every normal |N| < 4096 (Markstein: q0 = N * (1/d); r = N - q0 d; q = q0 + r * (1/d))
__device__ __forceinline__ float st_div(float N, float d, float dinv)
{
    const float q0 = N * dinv;
    const float r = __builtin_fmaf(-q0, d, N);
    return __builtin_fmaf(r, dinv, q0);
}

// number of samples under the window at recurrence step t of a line of `len` with window `win`
__device__ __forceinline__ int st_count(int t, int len, int win)
{
    const int hi = t < len - 1 ? t : len - 1, lo = t - win + 1 > 0 ? t - win + 1 : 0;
    const int c = hi - lo + 1;
    return c < 1 ? 1 : (c > 8 ? 8 : c);
}

struct StWave {
    float *lds;
    int lane;
    // pass-2 row recurrence (lane = row of the band), reset per band
    float csum, cprev[8];
    // pass-2 column recurrence (lane = kept column), carried over the whole image
    float dsum, dprev[8];
    f32x32 smp;  // pass-2 row outputs at the kept columns since the last D pass
    v4u carry[2];   // the strip's last 32 image bytes per row (two row blocks): they are the next strip's first 32
    v4u ahead[2][2];  // an even strip also fetches the odd strip's 64 new bytes per row: a row's 128 new bytes of a strip pair in one go
    rph::TailAcc tail;
    bool want_quality;
};

// ---- A + B: strip [c0, c0 + 64) of band [T0, T0 + 56) -> tile
template <int WIN_C>
__device__ __forceinline__ void st_ab_stage(StWave &w, const __amdgpu_buffer_rsrc_t rs, const StGeo &g, const int rs32, const int T0, const int c0)
{
    const int lane = w.lane, n = lane & 31, kh = lane >> 5;
    float *tile = w.lds;
    float *sums = w.lds + ST_OFF_SUMS;

    // image bytes: block m holds rows T0 - 8 + 32 m ..; lane (n, kh) fetches bytes [c0 - 16 + 32 c + 16 kh, + 16) of row n of the block.
    // Chunk 0 of a strip is chunk 2 of the strip before it ([c0 - 16, c0 + 16) = [(c0 - 64) + 48, (c0 - 64) + 80)): it stays in registers, and an
    // even strip fetches the 64 new bytes per row of the odd strip behind it as well: 128 new bytes per row and strip pair in one go, no byte of
    // a band requested twice, a 128-byte line touched by at most two fetches.
    v4u ch[2][3];
#pragma unroll
    for (int m = 0; m < 2; m++) {
        const int row = T0 - 8 + 32 * m + n;
        const int off0 = row * rs32 + c0 - 16 + 16 * kh;
        const bool odd_strip = (c0 & 64) != 0;  // (uniform)
#pragma unroll
        for (int c = 0; c < 5; c++) {  // chunks 3 and 4 are the next strip's chunks 1 and 2
            if (c == 0 && c0 != 0) {
                ch[m][0] = w.carry[m];
                continue;
            }
            if (odd_strip) {
                if (c == 1 || c == 2) ch[m][c] = w.ahead[m][c - 1];
                continue;
            }
            const int off = off0 + 32 * c;
            const uint32_t uoff = (row < 0 || row >= g.H || off < 0) ? 0x80000000u : (uint32_t)off;  // outside: the range check returns 0
            const v4u v = __builtin_amdgcn_raw_buffer_load_b128(rs, uoff, 0, 0);
            if (c < 3)
                ch[m][c] = v;
            else
                w.ahead[m][c - 3] = v;
        }
        w.carry[m] = ch[m][2];
    }
    // band matrices of the two 32-column blocks: slot 32 ks + 16 kh + j <-> source column c0 - 16 + 32 nb + 32 ks + 16 kh + j
    v4i bm[2][2];
#pragma unroll
    for (int nb = 0; nb < 2; nb++) {
        const int xo = c0 + 32 * nb + n;
        const bool ok = xo < g.W;
        const int lo = xo - g.a_r > 0 ? xo - g.a_r : 0, hi = xo + g.lead_r < g.W - 1 ? xo + g.lead_r : g.W - 1;
#pragma unroll
        for (int ks = 0; ks < 2; ks++) {
            const int s0 = c0 - 16 + 32 * nb + 32 * ks + 16 * kh;
            int jlo = lo - s0, jhi = hi - s0;
            jlo = jlo > 0 ? jlo : 0;
            jhi = jhi < 15 ? jhi : 15;
            const uint32_t m16 = (ok && jlo <= jhi) ? (((2u << jhi) - 1u) & ~((1u << jlo) - 1u)) : 0u;
            uint32_t bd[4];
#pragma unroll
            for (int q = 0; q < 4; q++) bd[q] = (((m16 >> (4 * q)) & 15u) * 0x00204081u) & 0x01010101u;
            if (ks == 1 && kh == 1) {  // slots 52..63 are never under a window: A = 64 there, B = 2 n in slot 52 -> + 128 n
                bd[1] = ok ? 2u * (uint32_t)(hi - lo + 1) : 0u;
                bd[2] = bd[3] = 0u;
            }
            bm[nb][ks] = v4i{(int)bd[0], (int)bd[1], (int)bd[2], (int)bd[3]};
        }
    }
    // divisor of this lane's column in the row pass
    float dA, dAinv;
    {
        const int x = c0 + lane;
        const int lo = x - g.a_r > 0 ? x - g.a_r : 0, hi = x + g.lead_r < g.W - 1 ? x + g.lead_r : g.W - 1;
        const int nr = x < g.W ? hi - lo + 1 : 1;
        dA = (float)nr;
        dAinv = 1.0f / dA;
    }
    const float sd = c_div[WIN_C][0], sdi = c_div[WIN_C][1];
    const bool steady = T0 >= WIN_C - 1 && T0 + ST_BAND - 1 <= g.H - 1;  // every step of the band divides by the full window
    const float2 *divtab = reinterpret_cast<const float2 *>(w.lds + ST_OFF_DIV);  // else: (cur, 1 / cur) per step, written once per band

    float sum = sums[c0 + lane];
    float keep[8];  // the last 8 row-pass values of block 0
#pragma unroll
    for (int m = 0; m < 2; m++) {
        v16i acc[2];
#pragma unroll
        for (int nb = 0; nb < 2; nb++) {
            acc[nb] = v16i{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
            for (int ks = 0; ks < 2; ks++) {
                const v4u raw = ch[m][nb + ks];
                v4i av = v4i{(int)(raw[0] ^ 0x80808080u), (int)(raw[1] ^ 0x80808080u), (int)(raw[2] ^ 0x80808080u), (int)(raw[3] ^ 0x80808080u)};
                if (ks == 1) {
                    av[1] = kh ? 0x40404040 : av[1];
                    av[2] = kh ? 0x40404040 : av[2];
                    av[3] = kh ? 0x40404040 : av[3];
                }
                acc[nb] = __builtin_amdgcn_mfma_i32_32x32x32_i8(av, bm[nb][ks], acc[nb], 0, 0, 0);
            }
        }
        // lane l < 32: column l of block 0, l >= 32: column l - 32 of block 1; rows 8 q + i in P[4 q + i], rows 8 q + 4 + i in R[4 q + i]
        float a[32];
#pragma unroll
        for (int i = 0; i < 16; i++) {
            const auto sw = __builtin_amdgcn_permlane32_swap(acc[0][i], acc[1][i], false, false);
            const int q = i >> 2, u = i & 3;
            a[8 * q + u] = st_div((float)(int)sw[0], dA, dAinv);
            a[8 * q + 4 + u] = st_div((float)(int)sw[1], dA, dAinv);
        }
#pragma unroll
        for (int r = (m == 0 ? 8 : 0); r < 32; r++) {
            const int tr = m == 0 ? r - 8 : 24 + r;  // step t = T0 + tr, tile row tr
            sum = sum + a[r];
            sum = sum - ((m == 0 || r >= WIN_C) ? a[r - WIN_C >= 0 ? r - WIN_C : 0] : keep[8 + r - WIN_C >= 0 && 8 + r - WIN_C < 8 ? 8 + r - WIN_C : 0]);
            float d = sd, di = sdi;
            if (!steady) {
                const float2 dd = divtab[tr];  // every lane reads the same address: one broadcast
                d = dd.x;
                di = dd.y;
            }
            tile[tr * ST_TP + lane] = st_div(sum, d, di);
        }
        if (m == 0) {
#pragma unroll
            for (int j = 0; j < 8; j++) keep[j] = a[24 + j];
        }
    }
    sums[c0 + lane] = sum;
}

// ---- C: the row recurrence over the tile's 64 columns; `em` marks the steps whose output decimate_float keeps
template <int WIN_R>
__device__ __forceinline__ void st_c_stage(StWave &w, const StGeo &g, const int c0, const unsigned long long em, int &cnt)
{
    const float4 *row = reinterpret_cast<const float4 *>(w.lds + w.lane * ST_TP);
    float v[64];
#pragma unroll
    for (int q = 0; q < 16; q++) {
        const float4 f = row[q];
        v[4 * q] = f.x;
        v[4 * q + 1] = f.y;
        v[4 * q + 2] = f.z;
        v[4 * q + 3] = f.w;
    }
    const float sd = c_div[WIN_R][0], sdi = c_div[WIN_R][1];
#pragma unroll
    for (int i = 0; i < 64; i++) {
        w.csum = w.csum + v[i];
        w.csum = w.csum - (i >= WIN_R ? v[i >= WIN_R ? i - WIN_R : 0] : w.cprev[i < WIN_R ? 8 + i - WIN_R : 0]);
        if ((em >> i) & 1ull) {
            const int t = c0 + i;
            float d = sd, di = sdi;
            if (t < WIN_R - 1 || t > g.W - 1) {
                const int c = __builtin_amdgcn_readfirstlane(st_count(t, g.W, WIN_R));
                d = c_div[c][0];
                di = c_div[c][1];
            }
            w.smp[__builtin_amdgcn_readfirstlane(cnt)] = st_div(w.csum, d, di);
            cnt++;
        }
    }
#pragma unroll
    for (int j = 0; j < 8; j++) w.cprev[j] = v[56 + j];
}

// steps of strip [c0, c0 + 64) whose output is a kept column: output column o leaves at step o + lead_r; jn = first slot not yet marked
__device__ __forceinline__ unsigned long long st_emit_mask(const StGeo &g, int c0, int &jn)
{
    unsigned long long em = 0;
    while (jn < 64) {
        const int te = ((2 * jn + 1) * g.W) / 128 + g.lead_r;
        if (te >= c0 + 64) break;
        em |= 1ull << (te - c0);
        jn++;
    }
    return em;
}

// ---- D: the column recurrence of kept columns [base, base + cnt) over the band's rows, feeding the tail.  ni / e_idx: next kept row and
// its index within the band, as they stood at the start of the band (every pass of a band walks the same rows).
__device__ __forceinline__ void st_d_pass(StWave &w, const StGeo &g, const int T0, const int base, const int cnt, int ni, const int want_rows)
{
    float *xp = w.lds;
    float *edge = w.lds + ST_OFF_EDGE;
    const int lane = w.lane;
    // samples to [slot][8 + row]; rows outside the image enter the recurrence as 0
    {
        const int o = T0 + lane - g.lead_c;
        const bool inside = o >= 0 && o < g.H;
        if (lane < ST_BAND) {
#pragma unroll
            for (int e = 0; e < 32; e++) xp[e * ST_XP + 8 + lane] = inside ? w.smp[e] : 0.0f;
        }
    }
    st_fence();
    const bool active = lane >= base && lane < base + cnt;
    if (active) {
        float *p = xp + (lane - base) * ST_XP;
#pragma unroll
        for (int j = 0; j < 8; j++) p[j] = w.dprev[j];
        const float *lv = p + 8 - g.win_c;
        int next_ri = ((2 * ni + 1) * g.H) / 128, e_idx = 0;
#pragma unroll 1
        for (int gidx = 0; gidx < ST_BAND / 8; gidx++) {
            float in[8], out[8];
#pragma unroll
            for (int u = 0; u < 8; u++) {
                in[u] = p[8 + 8 * gidx + u];
                out[u] = lv[8 * gidx + u];
            }
#pragma unroll
            for (int u = 0; u < 8; u++) {
                const int td = T0 + 8 * gidx + u - g.lead_c;  // step of this recurrence = row of the pass-2 row output
                w.dsum = w.dsum + in[u];
                w.dsum = w.dsum - out[u];
                if (ni < want_rows && td - g.lead_c == next_ri) {
                    const float val = w.dsum / (float)st_count(td, g.H, g.win_c);
                    float left = __shfl_up(val, 1);
                    if (lane == base && base > 0) left = edge[e_idx];
                    if (lane == base + cnt - 1) edge[e_idx] = val;
                    rph::tail_row_left(w.tail, val, left, lane > 0, ni, w.want_quality);
                    e_idx++;
                    ni++;
                    next_ri = ((2 * ni + 1) * g.H) / 128;
                }
            }
        }
#pragma unroll
        for (int j = 0; j < 8; j++) w.dprev[j] = p[8 + ST_BAND - 8 + j];
    }
    st_fence();
}

// the geometry of a W x H image (128..512 each)
__device__ __forceinline__ StGeo st_geo(int W, int H)
{
    StGeo g;
    g.W = W;
    g.H = H;
    g.win_r = (g.W + 63) / 64;
    g.win_c = (g.H + 63) / 64;
    const int half_r = (g.win_r + 2) / 2, half_c = (g.win_c + 2) / 2;
    g.lead_r = half_r - 1;
    g.a_r = g.win_r - half_r;
    g.lead_c = half_c - 1;
    g.ns_b = (g.W + 63) / 64;
    g.ns_c = ((127 * g.W) / 128 + g.lead_r) / 64 + 1;
    g.nb = (g.H + 2 * g.lead_c + ST_BAND - 1) / ST_BAND;
    return g;
}

// One wave hashes one Luma8 image: `px0` is its first pixel (on a dword boundary), rows `row_stride` bytes apart (a multiple of 4);
// lds: ST_LDS_FLOATS floats of the wave's own.  The results go to slot `slot` of the output arrays (quality, coeffs, dihedral: or nullptr).
__device__ __forceinline__ void st_image(float *lds, const uint8_t *px0, const StGeo &g, const size_t row_stride, uint8_t *hash, float *quality, float *coeffs,
                                         uint8_t *dihedral, const uint32_t slot)
{
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
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t *>(px0), 0,
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
    rph::tail_finish(w.tail, lds, w.lane, hash + (size_t)slot * 32, quality ? quality + slot : nullptr, coeffs ? coeffs + (size_t)slot * 256 : nullptr,
                     dihedral ? dihedral + (size_t)slot * 256 : nullptr);
}

// to_luma601 (pdqhash.rs:268-284) of pixels 4 q .. 4 q + 3 of a row of w Rgb8 / Rgba8 pixels, as one dword of Luma8 (CH = 1: a copy); p: the
// quad's first byte, of any alignment: aligned dwords + v_alignbyte.  The row's last, partial quad is read byte by byte: nothing is read
// behind the row.
template <int CH>
__device__ __forceinline__ uint32_t st_luma_quad(const uint8_t *p, uint32_t q, uint32_t w)
{
    uint32_t d[CH];
    if (q * 4 + 4 <= w) {
        const uint32_t sh = (uint32_t)(reinterpret_cast<uintptr_t>(p) & 3u);
        const uint32_t *p4 = reinterpret_cast<const uint32_t *>(p - sh);
        uint32_t raw[CH + 1];
#pragma unroll
        for (int i = 0; i < CH; i++) raw[i] = p4[i];
        raw[CH] = sh ? p4[CH] : 0u;  // (with sh != 0 that dword holds bytes of this quad: it is the image's own; with sh == 0 it is not touched)
#pragma unroll
        for (int i = 0; i < CH; i++) d[i] = __builtin_amdgcn_alignbyte(raw[i + 1], raw[i], sh);
    } else {
#pragma unroll
        for (int i = 0; i < CH; i++) d[i] = 0;
        for (uint32_t b = 0; b < (w - q * 4) * CH; b++) d[b >> 2] |= (uint32_t)p[b] << (8 * (b & 3));
    }
    uint32_t o = 0;
    if (CH == 1) {
        o = d[0];
    } else {
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int B = i * CH;
            const uint32_t r = (d[B >> 2] >> (8 * (B & 3))) & 0xFFu, g = (d[(B + 1) >> 2] >> (8 * ((B + 1) & 3))) & 0xFFu, b = (d[(B + 2) >> 2] >> (8 * ((B + 2) & 3))) & 0xFFu;
            o |= ((299u * r + 587u * g + 114u * b + 500u) / 1000u) << (8 * i);
        }
    }
    return o;
}

// The same dword of Luma8 for the layouts the hasher does not read directly (include/rupphash.h, rph_image_hash_ragged; the rules of
// pixel_rules.h): LumaA8 (L = 2) -- the L samples; Luma16 / LumaA16 (17, 18) -- (v + 128) / 257 of the L samples; Rgb16 / Rgba16 (19, 20) --
// each sample through (v + 128) / 257, then the 601 luma.  Alpha is not used.  The 8 .. 32 bytes of the quad come as aligned dwords +
// v_alignbyte; 16-bit rows start at even addresses.
template <int L>
__device__ __forceinline__ uint32_t st_luma_quad_layout(const uint8_t *p, uint32_t q, uint32_t w)
{
    constexpr int CH = L & 15, BPS = L > 16 ? 2 : 1, ND = CH * BPS;  // ND: dwords of four pixels
    uint32_t d[ND];
    if (q * 4 + 4 <= w) {
        const uint32_t sh = (uint32_t)(reinterpret_cast<uintptr_t>(p) & 3u);
        const uint32_t *p4 = reinterpret_cast<const uint32_t *>(p - sh);
        uint32_t raw[ND + 1];
#pragma unroll
        for (int i = 0; i < ND; i++) raw[i] = p4[i];
        raw[ND] = sh ? p4[ND] : 0u;  // (as in st_luma_quad: with sh != 0 that dword holds bytes of this quad)
#pragma unroll
        for (int i = 0; i < ND; i++) d[i] = __builtin_amdgcn_alignbyte(raw[i + 1], raw[i], sh);
    } else {
#pragma unroll
        for (int i = 0; i < ND; i++) d[i] = 0;
        for (uint32_t b = 0; b < (w - q * 4) * CH * BPS; b++) d[b >> 2] |= (uint32_t)p[b] << (8 * (b & 3));
    }
    auto sample8 = [&](int j) -> uint32_t {  // sample j of the quad as the hasher's u8
        if (BPS == 1) return (d[j >> 2] >> (8 * (j & 3))) & 0xFFu;
        return (((d[j >> 1] >> (16 * (j & 1))) & 0xFFFFu) + 128u) / 257u;
    };
    uint32_t o = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        uint32_t y;
        if (CH <= 2) {
            y = sample8(i * CH);
        } else {
            const uint32_t r = sample8(i * CH), g = sample8(i * CH + 1), b = sample8(i * CH + 2);
            y = (299u * r + 587u * g + 114u * b + 500u) / 1000u;
        }
        o |= y << (8 * i);
    }
    return o;
}

}  // namespace
