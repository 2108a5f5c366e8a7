// nearest_kernels.hip -- the nearest files of a query (include/rupphash.h): exact top-k Hamming search of n_q hashes in a
// library of n_lib files with 1 or 8 rows each.  No threshold, so no screen: the full 256-bit distance of every (row, query) pair comes
// from the matrix pipe and a selection follows it.
//
// Stage 1 (nearest_lists_kernel): one workgroup per (library segment, tile of 32 queries), looping over the items of the call.  The
// query tile is expanded once into LDS as +-1 e2m1 codes and is the B operand (column = lane & 31); 32 library rows are the A operand;
// four chained v_mfma_scale_f32_32x32x64_f8f6f4 at unit scales, one per 64-bit slice, give the exact dot, and d = (256 - dot) / 2.  The
// 32 x 32 result puts row (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5) of column lane & 31 into register `reg`, so a lane holds 16 rows of
// ONE query.  With 8 rows per file the A rows are ordered so that a file's variants fall into registers 0-7 or 8-15 of one lane half
// (a block is 4 files, two per half): the minimum over the variants and the smallest variant attaining it are in-lane compares.  With
// one row per file a block is 32 files.  Every lane keeps the k best keys of its query as an ascending list in LDS and tests a
// candidate against the list's worst key first; inserting is the rare path.  The 2 x waves lists of a query are merged when the segment
// is through and the k best go to the workspace.
//
// Stage 2 (nearest_merge_kernel): one wave per query.  Every lane merges the lists of its share of the segments into a list of its
// own, the 64 lists are merged by k rounds of a wave minimum, lane 0 writes the slots and the count.  The key (distance, file) is
// unique, so any correct selection gives the same bytes.
//
// Dead rows and columns are excluded by their INDEX: the tail of the library and of a segment, the tail of a query tile, rows 1-7 of a
// file without features.  A zeroed operand would give dot 0, distance 128, a perfectly good neighbour here.  skip, max_dist and the
// bounds are tested before a candidate can displace a list entry.
#include <atomic>

#include "rph_internal.h"

namespace {
typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v8i __attribute__((ext_vector_type(8)));
typedef float v16f __attribute__((ext_vector_type(16)));

constexpr uint32_t QT = 32;                       // queries per tile: the columns of one MFMA
constexpr uint32_t COL_PITCH = 8 * 16 + 16;       // bytes of a query's record in LDS: [slice][k-half][32 x fp4 = 16 B] + pad (conflict-free b128, lane = column)
constexpr uint32_t EMPTY = 0xFFFFFFFFu;           // a list slot without a file (as a key: distance 511)
constexpr uint64_t EMPTY64 = ~0ull;
constexpr uint32_t REL_BITS = 20;                 // a stage-1 key: distance << 23 | file relative to its segment << 3 | variant
constexpr uint64_t MAX_SEG_FILES = 1ull << REL_BITS;
constexpr uint64_t WORK_BYTES = (uint64_t)256 << 20;  // the partial lists never take more (the default of g_work_bytes)
constexpr uint64_t MIN_WORK_BYTES = QT * RPH_NEAREST_MAX_K * 4;  // one tile of the longest lists in one segment
constexpr uint64_t TARGET_ITEMS = 2048;           // (segment, tile) items a call is cut into at least when the library allows: 8 workgroups on each of 256 CUs
constexpr uint64_t MAX_CHUNK_QUERIES = 1u << 20;

std::atomic<uint32_t> g_forced_segment{0};  // rph_debug_nearest_set_segment
std::atomic<uint64_t> g_work_bytes{WORK_BYTES};  // rph_debug_nearest_set_workspace

struct NearestLayout {
    uint32_t files_per_block, seg_files, n_segs, chunk_queries;
};

uint64_t ceil_div(uint64_t a, uint64_t b) { return (a + b - 1) / b; }

// Segments: as many as fill the device for the query tiles there are (one query against a large library still spreads over all CUs),
// no shorter than 16 blocks, no longer than a key's 20 bits, and no more of them than let 32 queries' lists fit the workspace.
NearestLayout nearest_layout(uint64_t n_lib, uint32_t n_variants, uint64_t n_q, uint32_t k)
{
    NearestLayout L;
    const uint64_t fb = n_variants == 8 ? 4 : 32;
    const uint64_t n_tiles = std::max<uint64_t>(1, ceil_div(n_q, QT));
    const uint32_t forced = g_forced_segment.load();
    const uint64_t work_bytes = g_work_bytes.load();
    uint64_t seg;
    if (forced) {
        seg = ceil_div(forced, fb) * fb;
    } else {
        const uint64_t want = std::max<uint64_t>(1, ceil_div(TARGET_ITEMS, n_tiles));
        seg = std::max(ceil_div(ceil_div(std::max<uint64_t>(n_lib, 1), want), fb) * fb, 16 * fb);
    }
    const uint64_t most_segs = work_bytes / ((uint64_t)QT * k * 4);
    seg = std::max(seg, ceil_div(ceil_div(n_lib, most_segs), fb) * fb);
    seg = std::min(seg, MAX_SEG_FILES);
    L.files_per_block = (uint32_t)fb;
    L.seg_files = (uint32_t)seg;
    L.n_segs = (uint32_t)ceil_div(n_lib, seg);
    uint64_t chunk = MAX_CHUNK_QUERIES;
    if (L.n_segs) chunk = std::min(chunk, work_bytes / ((uint64_t)L.n_segs * k * 4) / QT * QT);
    L.chunk_queries = (uint32_t)std::max<uint64_t>(chunk, QT);
    return L;
}

struct NearestArgs {
    const uint4 *rows;
    const uint8_t *has_features;
    const uint32_t *hashes_q, *skip, *gather;
    uint32_t n_variants, k, max_dist;
    uint64_t n_lib;
    uint32_t q0, nq, n_tiles;  // this chunk: its first query, how many, their tiles
    uint32_t seg_files, n_segs;
    uint64_t n_items;          // n_segs * n_tiles
    uint32_t *part;            // [n_segs][nq][k] stage-1 keys, ascending, EMPTY behind the last
    rph_edge *out;
    uint32_t *counts;
};

__device__ __forceinline__ uint32_t fp4_pm1(uint32_t byte)  // 8 bits -> 8 e2m1 codes, 1 -> +1.0 (0x2), 0 -> -1.0 (0xA); FmtFp4 of hamming_kernels.hip
{
    uint32_t e = 0;
    for (int i = 0; i < 8; i++) e |= (((byte >> i) & 1u) ? 0x2u : 0xAu) << (4 * i);
    return e;
}

__device__ __forceinline__ v4i expand_dword(const uint32_t *lut, uint32_t dw)
{
    return v4i{(int)lut[dw & 0xFFu], (int)lut[(dw >> 8) & 0xFFu], (int)lut[(dw >> 16) & 0xFFu], (int)lut[dw >> 24]};
}

// One candidate of this lane's query: the tests by index and value first, then the list's worst key, then (rarely) the insertion.
// list: this lane's column of s_list, `pitch` words between entries.
__device__ __forceinline__ void offer(uint32_t *list, uint32_t pitch, uint32_t k, uint32_t &worst, bool eligible, uint32_t d, uint32_t rel, uint32_t variant)
{
    const uint32_t key = d << 23 | rel << 3 | variant;
    if (!eligible || key >= worst) return;
    uint32_t at = k - 1;
    while (at > 0) {
        const uint32_t above = list[(at - 1) * pitch];
        if (above < key) break;
        list[at * pitch] = above;
        at--;
    }
    list[at * pitch] = key;
    worst = list[(k - 1) * pitch];
}

__global__ void __launch_bounds__(256) nearest_lists_kernel(NearestArgs a)
{
    extern __shared__ uint32_t s_list[];  // [k][blockDim.x]: entry r of thread t's list at r * blockDim.x + t
    __shared__ __attribute__((aligned(16))) uint8_t s_q[QT * COL_PITCH];
    __shared__ uint32_t s_lut[256];
    const uint32_t tid = threadIdx.x, threads = blockDim.x, n_waves = threads >> 6;
    const uint32_t lane = tid & 63, wave = tid >> 6, c32 = lane & 31, hh = lane >> 5;
    const uint32_t nv = a.n_variants, k = a.k;
    const uint32_t fb = nv == 8 ? 4 : 32;
    for (uint32_t t = tid; t < 256; t += threads) s_lut[t] = fp4_pm1(t);
    uint32_t *list = s_list + tid;

    // the A row this lane loads in every block: MFMA row m = c32.  8 variants: row m of the result lands in lane half (m >> 2) & 1,
    // register (m & 3) + 4 (m >> 3); registers 0-7 / 8-15 of a half are one file, so file = 2 half + (register >> 3), variant = register & 7
    const uint32_t a_reg = (c32 & 3) + 4 * (c32 >> 3);
    const uint32_t a_file = nv == 8 ? 2 * ((c32 >> 2) & 1) + (a_reg >> 3) : c32;
    const uint32_t a_variant = nv == 8 ? (a_reg & 7) : 0;

    for (uint64_t item = blockIdx.x; item < a.n_items; item += gridDim.x) {
        const uint32_t seg = (uint32_t)(item / a.n_tiles), tile = (uint32_t)(item % a.n_tiles);
        const uint64_t seg_first = (uint64_t)seg * a.seg_files;
        const uint32_t seg_n = (uint32_t)std::min<uint64_t>(a.seg_files, a.n_lib - seg_first);
        __syncthreads();  // the LUT is there; the merge of the item before is through with the lists and nobody reads its queries
        for (uint32_t t = tid; t < QT * 8; t += threads) {
            const uint32_t col = t >> 3, kb = t & 7, ql = tile * QT + col;
            uint32_t dw = 0;  // (a column behind the last query: never offered, see q_live)
            if (ql < a.nq) {
                const uint64_t src = a.gather ? a.gather[a.q0 + ql] : (uint64_t)a.q0 + ql;
                dw = a.hashes_q[src * 8 + kb];
            }
            // dword kb is slice kb >> 1, k-half kb & 1: record (kb >> 1) * 2 + (kb & 1) = kb
            *reinterpret_cast<v4i *>(s_q + col * COL_PITCH + kb * 16) = expand_dword(s_lut, dw);
        }
        for (uint32_t r = 0; r < k; r++) list[r * threads] = EMPTY;
        __syncthreads();

        const uint32_t ql = tile * QT + c32;
        const bool q_live = ql < a.nq;
        uint32_t my_skip = RPH_NO_FILE;
        if (q_live) my_skip = a.gather ? a.gather[a.q0 + ql] : a.skip ? a.skip[a.q0 + ql] : RPH_NO_FILE;
        v4i B[4];
#pragma unroll
        for (int f = 0; f < 4; f++) B[f] = *reinterpret_cast<const v4i *>(s_q + c32 * COL_PITCH + (f * 2 + hh) * 16);

        uint32_t worst = EMPTY;
        const uint32_t n_blocks = (seg_n + fb - 1) / fb;
        // the row of the next block is fetched while this one is multiplied
        uint4 lo = make_uint4(0, 0, 0, 0), hi = lo;
        auto fetch = [&](uint32_t b) {
            const uint32_t rel = b * fb + a_file;
            lo = hi = make_uint4(0, 0, 0, 0);  // (a row behind the segment's end: never offered, see `inside`)
            if (b < n_blocks && rel < seg_n) {
                const uint4 *p = a.rows + ((seg_first + rel) * nv + a_variant) * 2;
                lo = p[0], hi = p[1];
            }
        };
        fetch(wave);
        for (uint32_t b = wave; b < n_blocks; b += n_waves) {
            const uint32_t d0 = hh ? lo.y : lo.x, d1 = hh ? lo.w : lo.z, d2 = hh ? hi.y : hi.x, d3 = hh ? hi.w : hi.z;  // dword 2 f + k-half of slice f
            // the flags of this lane's two files (8 variants): 0 keeps a file to its row 0
            bool plain[2] = {false, false};
            if (nv == 8 && a.has_features) {
#pragma unroll
                for (uint32_t s = 0; s < 2; s++) {
                    const uint32_t rel = b * 4 + 2 * hh + s;
                    plain[s] = rel < seg_n && a.has_features[seg_first + rel] == 0;
                }
            }
            fetch(b + n_waves);
            const v4i A0 = expand_dword(s_lut, d0), A1 = expand_dword(s_lut, d1), A2 = expand_dword(s_lut, d2), A3 = expand_dword(s_lut, d3);
            v16f acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
            // cbsz = blgp = 4: fp4 e2m1; E8M0 scale 127 = 2^0
            acc = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(v8i{A0[0], A0[1], A0[2], A0[3], 0, 0, 0, 0}, v8i{B[0][0], B[0][1], B[0][2], B[0][3], 0, 0, 0, 0}, acc, 4, 4, 0, 127, 0, 127);
            acc = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(v8i{A1[0], A1[1], A1[2], A1[3], 0, 0, 0, 0}, v8i{B[1][0], B[1][1], B[1][2], B[1][3], 0, 0, 0, 0}, acc, 4, 4, 0, 127, 0, 127);
            acc = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(v8i{A2[0], A2[1], A2[2], A2[3], 0, 0, 0, 0}, v8i{B[2][0], B[2][1], B[2][2], B[2][3], 0, 0, 0, 0}, acc, 4, 4, 0, 127, 0, 127);
            acc = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(v8i{A3[0], A3[1], A3[2], A3[3], 0, 0, 0, 0}, v8i{B[3][0], B[3][1], B[3][2], B[3][3], 0, 0, 0, 0}, acc, 4, 4, 0, 127, 0, 127);
            if (nv == 8) {
#pragma unroll
                for (uint32_t s = 0; s < 2; s++) {
                    const uint32_t rel = b * 4 + 2 * hh + s;
                    uint32_t d = (uint32_t)((256 - (int)acc[8 * s]) >> 1), variant = 0;
#pragma unroll
                    for (uint32_t v = 1; v < 8; v++) {
                        const uint32_t dv = (uint32_t)((256 - (int)acc[8 * s + v]) >> 1);
                        if (!plain[s] && dv < d) d = dv, variant = v;
                    }
                    const bool inside = rel < seg_n;
                    offer(list, threads, k, worst, q_live && inside && d <= a.max_dist && seg_first + rel != my_skip, d, rel, variant);
                }
            } else {
#pragma unroll
                for (uint32_t reg = 0; reg < 16; reg++) {
                    const uint32_t rel = b * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * hh;
                    const uint32_t d = (uint32_t)((256 - (int)acc[reg]) >> 1);
                    const bool inside = rel < seg_n;
                    offer(list, threads, k, worst, q_live && inside && d <= a.max_dist && seg_first + rel != my_skip, d, rel, 0);
                }
            }
        }
        __syncthreads();
        // the lists of lanes c and c + 32 of every wave serve query c: lane c of wave 0 merges them, one head per list
        if (tid < QT && q_live) {
            uint32_t *dst = a.part + ((uint64_t)seg * a.nq + ql) * k;
            const uint32_t n_lists = 2 * n_waves;
            uint64_t heads = 0;  // 8 bits per list
            for (uint32_t r = 0; r < k; r++) {
                uint32_t best = EMPTY, from = 0;
                for (uint32_t j = 0; j < n_lists; j++) {
                    const uint32_t at = (uint32_t)(heads >> (8 * j)) & 0xFFu;
                    const uint32_t key = at < k ? s_list[at * threads + j * 32 + tid] : EMPTY;
                    if (key < best) best = key, from = j;
                }
                dst[r] = best;
                if (best != EMPTY) heads += 1ull << (8 * from);
            }
        }
    }
}

__device__ __forceinline__ uint64_t wave_min64(uint64_t v)
{
#pragma unroll
    for (int step = 1; step < 64; step <<= 1) {
        const uint32_t lo = __shfl_xor((uint32_t)v, step, 64), hi = __shfl_xor((uint32_t)(v >> 32), step, 64);
        const uint64_t other = (uint64_t)hi << 32 | lo;
        v = other < v ? other : v;
    }
    return v;
}

// One wave per query of the chunk (the blocks stride over them).  Global keys: distance << 35 | file << 3 | variant.
__global__ void __launch_bounds__(64) nearest_merge_kernel(NearestArgs a)
{
    extern __shared__ uint64_t s_merge[];  // [k][64]
    const uint32_t lane = threadIdx.x, k = a.k;
    uint64_t *list = s_merge + lane;
    for (uint32_t ql = blockIdx.x; ql < a.nq; ql += gridDim.x) {
        for (uint32_t r = 0; r < k; r++) list[r * 64] = EMPTY64;
        uint64_t worst = EMPTY64;
        for (uint32_t seg = lane; seg < a.n_segs; seg += 64) {
            const uint32_t *src = a.part + ((uint64_t)seg * a.nq + ql) * k;
            const uint64_t first = (uint64_t)seg * a.seg_files;
            for (uint32_t r = 0; r < k; r++) {
                const uint32_t part = src[r];
                if (part == EMPTY) break;
                const uint64_t key = (uint64_t)(part >> 23) << 35 | (first + ((part >> 3) & (MAX_SEG_FILES - 1))) << 3 | (part & 7);
                if (key >= worst) break;  // the segment's list ascends: nothing behind this one gets in either
                uint32_t at = k - 1;
                while (at > 0) {
                    const uint64_t above = list[(at - 1) * 64];
                    if (above < key) break;
                    list[at * 64] = above;
                    at--;
                }
                list[at * 64] = key;
                worst = list[(k - 1) * 64];
            }
        }
        const uint64_t q = (uint64_t)a.q0 + ql;
        uint32_t head = 0, filled = 0;
        for (uint32_t r = 0; r < k; r++) {
            const uint64_t mine = head < k ? list[head * 64] : EMPTY64;
            const uint64_t least = wave_min64(mine);
            if (least != EMPTY64) {
                filled++;
                if (mine == least) head++;  // keys are unique: one lane
            }
            if (lane == 0) {
                rph_edge e;
                e.i = least != EMPTY64 ? (uint32_t)(least >> 3) : RPH_NO_FILE;
                e.j = (uint32_t)q;
                e.d = least != EMPTY64 ? (uint16_t)(least >> 35) : (uint16_t)0xFFFF;
                e.flags = least != EMPTY64 ? (uint16_t)((least & 7) << RPH_EDGE_VARIANT_SHIFT) : (uint16_t)0;
                a.out[q * k + r] = e;
            }
        }
        if (lane == 0 && a.counts) a.counts[q] = filled;
    }
}
}  // namespace

int rph_nearest_run(rph_ctx *ctx, const rph_nearest &q, hipStream_t s)
{
    if (q.n_q == 0) return RPH_OK;
    const NearestLayout L = nearest_layout(q.n_lib, q.n_variants, q.n_q, q.k);
    const uint64_t chunk = std::min<uint64_t>(L.chunk_queries, q.n_q);
    const size_t work = (size_t)L.n_segs * chunk * q.k * 4;  // <= the workspace limit by the layout
    std::lock_guard<std::mutex> lock(ctx->mu);
    ScratchUse use{ctx->sweep_scratch, s};
    RPH_TRY(use.acquire(std::max<size_t>(work, 256), std::max<size_t>(work, 4096)));
    NearestArgs a;
    a.rows = (const uint4 *)q.rows, a.has_features = q.has_features;
    a.hashes_q = (const uint32_t *)q.hashes_q, a.skip = q.skip, a.gather = q.gather;
    a.n_variants = q.n_variants, a.k = q.k, a.max_dist = q.max_dist, a.n_lib = q.n_lib;
    a.seg_files = L.seg_files, a.n_segs = L.n_segs;
    a.part = ctx->sweep_scratch.as<uint32_t>(), a.out = q.out, a.counts = q.counts;
    const uint64_t cus = ctx->compute_units > 1 ? ctx->compute_units : 1;
    // lists of up to 32 keys: four waves per workgroup; longer ones: two, which keeps the lists within 32 KB of LDS
    const unsigned threads = q.k > 32 ? 128 : 256;
    for (uint64_t q0 = 0; q0 < q.n_q; q0 += chunk) {
        a.q0 = (uint32_t)q0, a.nq = (uint32_t)std::min<uint64_t>(chunk, q.n_q - q0);
        a.n_tiles = (a.nq + QT - 1) / QT;
        a.n_items = (uint64_t)a.n_segs * a.n_tiles;
        if (a.n_items) {
            const unsigned grid = (unsigned)std::min<uint64_t>(a.n_items, cus * 8);
            hipLaunchKernelGGL(nearest_lists_kernel, dim3(grid), dim3(threads), (size_t)q.k * threads * 4, s, a);
            RPH_HIP_CHECK(hipGetLastError());
        }
        const unsigned grid2 = (unsigned)std::min<uint64_t>(a.nq, cus * 32);
        hipLaunchKernelGGL(nearest_merge_kernel, dim3(grid2), dim3(64), (size_t)q.k * 64 * 8, s, a);
        RPH_HIP_CHECK(hipGetLastError());
    }
    return use.done();
}

namespace {
int bad_argument(const char *who, const char *what)
{
    rph_set_error("%s: %s", who, what);
    return RPH_ERR_INVALID_ARG;
}
}  // namespace

extern "C" {

int rph_hamming_nearest_dev(rph_ctx *ctx, const void *d_rows, uint32_t n_variants, const void *d_has_features, uint64_t n_lib, const void *d_hashes_q,
                            const void *d_skip, uint64_t n_q, uint32_t k, uint32_t max_dist, void *d_out, void *d_counts, void *stream)
{
    return rph_guarded("rph_hamming_nearest_dev", [&]() -> int {
        const char *who = "rph_hamming_nearest_dev";
        if (!ctx) return bad_argument(who, "null argument");
        RPH_TRY(rph_nearest_check(who, d_rows, n_variants, n_lib, d_hashes_q, n_q, k, d_out));
        if (n_q == 0) return RPH_OK;
        if (((n_lib ? (uintptr_t)d_rows : 0) | (uintptr_t)d_hashes_q) & 15) return bad_argument(who, "rows and queries are read 16 bytes at a time: align them to 16");
        RPH_HIP_CHECK(hipSetDevice(ctx->device));
        rph_nearest q;
        q.rows = (const uint8_t *)d_rows, q.has_features = (const uint8_t *)d_has_features, q.hashes_q = (const uint8_t *)d_hashes_q;
        q.skip = (const uint32_t *)d_skip, q.n_variants = n_variants, q.k = k, q.max_dist = max_dist, q.n_lib = n_lib, q.n_q = n_q;
        q.out = (rph_edge *)d_out, q.counts = (uint32_t *)d_counts;
        return rph_nearest_run(ctx, q, stream ? (hipStream_t)stream : ctx->stream);
    });
}

int rph_hamming_nearest(rph_ctx *ctx, const uint8_t *rows, uint32_t n_variants, const uint8_t *has_features, uint64_t n_lib, const uint8_t *hashes32_q,
                        const uint32_t *skip, uint64_t n_q, uint32_t k, uint32_t max_dist, rph_edge *out, uint32_t *counts_out)
{
    return rph_guarded("rph_hamming_nearest", [&]() -> int {
        if (!ctx) return bad_argument("rph_hamming_nearest", "null argument");
        RPH_TRY(rph_nearest_check("rph_hamming_nearest", rows, n_variants, n_lib, hashes32_q, n_q, k, out));
        if (n_q == 0) return RPH_OK;
        RPH_HIP_CHECK(hipSetDevice(ctx->device));
        hipStream_t s = ctx->stream;
        DevBuf d_rows, d_hf, d_q, d_skip, d_out, d_counts;
        StreamDrain drain{s};  // the buffers above go when the stream is through with them
        const size_t row_bytes = (size_t)n_lib * n_variants * 32;
        RPH_TRY(d_rows.alloc(row_bytes));
        if (row_bytes) RPH_HIP_CHECK(hipMemcpyAsync(d_rows.data(), rows, row_bytes, hipMemcpyHostToDevice, s));
        if (has_features && n_lib) {
            RPH_TRY(d_hf.alloc(n_lib));
            RPH_HIP_CHECK(hipMemcpyAsync(d_hf.data(), has_features, n_lib, hipMemcpyHostToDevice, s));
        }
        RPH_TRY(d_q.alloc(n_q * 32));
        RPH_HIP_CHECK(hipMemcpyAsync(d_q.data(), hashes32_q, n_q * 32, hipMemcpyHostToDevice, s));
        if (skip) {
            RPH_TRY(d_skip.alloc(n_q * 4));
            RPH_HIP_CHECK(hipMemcpyAsync(d_skip.data(), skip, n_q * 4, hipMemcpyHostToDevice, s));
        }
        RPH_TRY(d_out.alloc(n_q * k * sizeof(rph_edge)));
        RPH_TRY(d_counts.alloc(n_q * 4));
        rph_nearest q;
        q.rows = d_rows.data(), q.has_features = d_hf.data(), q.hashes_q = d_q.data(), q.skip = d_skip.as<uint32_t>();
        q.n_variants = n_variants, q.k = k, q.max_dist = max_dist, q.n_lib = n_lib, q.n_q = n_q;
        q.out = d_out.as<rph_edge>(), q.counts = d_counts.as<uint32_t>();
        RPH_TRY(rph_nearest_run(ctx, q, s));
        RPH_HIP_CHECK(hipMemcpyAsync(out, d_out.data(), n_q * k * sizeof(rph_edge), hipMemcpyDeviceToHost, s));
        if (counts_out) RPH_HIP_CHECK(hipMemcpyAsync(counts_out, d_counts.data(), n_q * 4, hipMemcpyDeviceToHost, s));
        RPH_HIP_CHECK(hipStreamSynchronize(s));
        return RPH_OK;
    });
}

void rph_debug_nearest_layout(uint64_t n_lib, uint32_t n_variants, uint64_t n_q, uint32_t k, uint32_t *out)
{
    const NearestLayout L = nearest_layout(n_lib, n_variants == 8 ? 8 : 1, n_q, k < 1 ? 1 : k > RPH_NEAREST_MAX_K ? RPH_NEAREST_MAX_K : k);
    out[0] = L.files_per_block, out[1] = L.seg_files, out[2] = QT, out[3] = L.n_segs, out[4] = L.chunk_queries;
}

void rph_debug_nearest_set_segment(uint32_t files) { g_forced_segment.store(files); }

void rph_debug_nearest_set_workspace(uint64_t bytes) { g_work_bytes.store(bytes == 0 ? WORK_BYTES : std::max(bytes, MIN_WORK_BYTES)); }

}  // extern "C"
