// jpeg_pipeline.cpp -- host side of the JPEG path (row N3 of SURVEY 8f) and its C ABI: chunking, the two lanes of staging / device
// buffers, host entropy decoding or stream preparation for the device walk, reconstruction + hashing sub-batches, the one-file queue.
// The kernels are in jpeg_kernels.hip, the entropy decoder and the stream preparation in jpeg_host.cpp.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <type_traits>
#include <unordered_map>
#include <vector>

#include "jpeg_device.h"
#include "rph_internal.h"

namespace {

// growth of the pinned buffers: a quarter more, to whole 4 KiB pages
inline size_t pinned_slack(size_t bytes) { return align_up(bytes + bytes / 4, 4096); }

// A pinned host buffer with its device twin, grown together; `user` is the stream whose work uses them
struct Twin {
    PinnedBuf h;
    DevBuf d;
    int reserve(size_t bytes, hipStream_t user)
    {
        RPH_TRY(h.reserve(bytes, pinned_slack(bytes), user));
        return d.reserve(bytes, pinned_slack(bytes), user);
    }
};

constexpr size_t RES_BYTES = 32 + 4 + 1024 + 256 + 4;  // per image: hash, quality, coefficients, dihedral, valid + entropy status (padded)
struct ResView {  // the per-image result arrays inside one buffer laid out for `images` images
    uint8_t *hash, *quality, *coeffs, *dihedral, *valid, *status, *pixel;
    ResView(uint8_t *p, size_t images)
    {
        hash = p;
        quality = hash + images * 32;
        coeffs = quality + images * 4;
        dihedral = coeffs + images * 1024;
        valid = dihedral + images * 256;
        status = valid + images;
        pixel = p + images * RES_BYTES;  // pixel hashes (32 B per image) behind the rest, in slots reserved with room for them
    }
};

// ---------------------------------------------------------------------------------------------------------------------------
// The pipeline.  One JPEG batch call per context at a time (ctx->jpeg_mu); buffers are kept in the context across calls.
//   host entropy:   chunks of <= 192 MB of coefficients, two slots: the host threads decode chunk k + 1 while the device works on k
//   device entropy: chunks as large as the coefficient buffer allows (tens of thousands of images: one per lane), the host only
//                   prepares streams; reconstruction + hashing then runs over the chunk in sub-batches through small buffers
// ---------------------------------------------------------------------------------------------------------------------------
struct Slot {
    hipStream_t stream = nullptr;  // (release: synchronised before the buffers are freed)
    hipEvent_t done = nullptr;  // device entropy: the slot's chunk (work on another slot's stream) has delivered its results
    Twin coef;              // host entropy: pinned staging + device; device entropy: unused
    Twin stream_bytes;      // device entropy: de-stuffed entropy bytes
    Twin meta;              // descriptors (write_meta)
    PinnedBuf res;          // results
    size_t res_images = 0;
    bool res_pixel = false;  // the results buffer has room for the pixel hashes (ResView::pixel)
    DevBuf segwork;  // device entropy, segmented streams: states | records of round 0 | out positions | segment -> file map
    DevBuf pmask;    // device entropy, progressive files: which coefficients are nonzero, one word per block
    DevBuf pcorr;    // and the records of their AC refinement scans (PCorr, jpeg_device.h)
    DevBuf pdc;      // and the bits of their DC refinement scans, one byte per block
    void release()
    {
        if (stream) (void)hipStreamSynchronize(stream);
        if (stream) (void)hipStreamDestroy(stream);
        if (done) (void)hipEventDestroy(done);
        *this = Slot();
    }
    int ready()
    {
        if (!stream) RPH_HIP_CHECK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
        if (!done) RPH_HIP_CHECK(hipEventCreateWithFlags(&done, hipEventDisableTiming));
        return RPH_OK;
    }
    int reserve_res(size_t images, bool pixel)
    {
        if (res_images >= images && (res_pixel || !pixel)) return RPH_OK;
        images += images / 4;
        // pinned host memory the kernels write into directly (32 B .. 1.3 KB per image cross PCIe as they are produced): a copy back at the
        // end of a chunk queued behind the other lanes' kernels and held the lane up for tens of milliseconds
        const size_t bytes = images * (RES_BYTES + (pixel ? 32 : 0));
        RPH_TRY(res.reserve(bytes, pinned_slack(bytes), stream));
        res_images = images;
        res_pixel = pixel;
        return RPH_OK;
    }
};

struct Job {
    Job() {}  // user-provided on purpose: std::vector<Job>(n) then runs the member initialisers only instead of zeroing ~1 KB per job first
    const uint8_t *data = nullptr;
    size_t len = 0;
    rphj::Frame frame;
    int status = RPH_OK;
    uint64_t first_block = 0;  // within the chunk's coefficient buffer
    rphj::StreamPlan plan;     // device entropy
    const int16_t *pre = nullptr;  // coefficients already decoded by the caller into pinned memory (rph_jpeg_pdq_hash_one)
    std::vector<uint32_t> marks;   // device entropy: where the restart intervals of a one-scan file begin (empty: walk the file with one lane)
    size_t stream_off = 0, stream_used = 0;
};

using Jobs = std::vector<Job>;

constexpr int JPEG_LANES = 4;  // chunks in flight in the device-entropy pipeline (the host-entropy pipeline uses the first two)
struct JpegPipe {
    // (~JpegPipe synchronises the slots' streams, which use every buffer here, before the members are freed)
    DevBuf coef;  // device entropy: the chunk's coefficient buffer (one: chunks run back to back on one stream)
    // reconstruction buffers (sample planes, packed pixels) shared by the slots' sub-batches: used in stream order, one sub-batch at a
    // time per stream; each slot owns one pair
    DevBuf planes[JPEG_LANES], pixels[JPEG_LANES];
    size_t recon_coef_bytes[JPEG_LANES] = {};
    // pixel hashes: the group values of the images above 8192 px (allocated by the first call that asks for pixel hashes)
    DevBuf b3[JPEG_LANES];
    Slot slot[JPEG_LANES];
    // the per-file records of the last call, kept: a call of 100 000 files spent 15 ms constructing and first-touching 120 MB of them
    // before the first byte moved
    Jobs jobs_cache;
    ~JpegPipe()
    {
        for (Slot &S : slot) S.release();
    }
    // sample planes and packed pixels for sub-batches of up to `coef_need` bytes of coefficients
    int reserve_recon(int b, size_t coef_need, hipStream_t s)
    {
        if (recon_coef_bytes[b] >= coef_need) return RPH_OK;
        RPH_TRY(planes[b].reserve(coef_need / 2 + 256, s));  // 64 bytes of samples per 128 bytes of coefficients
        // packed pixels never exceed the coefficient bytes (4:2:0: both 3 w h; Luma8: w h against 2 w h), plus row / image padding
        RPH_TRY(pixels[b].reserve(coef_need + coef_need / 8 + 65536, s));
        recon_coef_bytes[b] = coef_need;
        return RPH_OK;
    }
};

constexpr size_t CHUNK_COEF_BYTES = (size_t)192 << 20;   // host entropy, per slot: ~250 images of 512x512 4:2:0
constexpr size_t SUB_COEF_BYTES = (size_t)4 << 30;        // device entropy: reconstruction sub-batch (~5400 such images)
constexpr size_t MAX_IMAGE_COEF_BYTES = (size_t)3 << 30;  // one image beyond this is refused (RPH_ERR_UNSUPPORTED)
// A frame header may announce any geometry: a file of a few hundred bytes that declares 20000 x 20000 would have gigabytes of pinned
// memory zeroed on its behalf.  Every coded block takes at least one bit of the file (sequential: a DC category code and an end-of-block
// code, two bits; a progressive file's first DC scan: one), so a header that announces more blocks than eight per file byte cannot be honest:
// refused before anything is allocated.
static inline bool frame_is_plausible(const rphj::Frame &f, size_t file_len) { return (size_t)f.total_blocks <= 8 * file_len + 64; }
constexpr uint32_t CHUNK_MAX_IMAGES = 4096;               // host entropy
constexpr size_t SUB_MAX_IMAGES = 16384;                  // images per reconstruction sub-batch (grid.y of the kernels: 3 planes each)
constexpr uint32_t DEVICE_ENTROPY_MIN_FILES = 512;        // automatic mode: below this many lanes (files, or restart intervals) the host decodes (latency)

// Huffman tables of a chunk, one per distinct content (most sequential files of a collection share the four Annex K tables; a
// progressive file brings a dozen of its own).  Sixteen threads ask at once: the index is cut into 64 shards by the tables' hash, each
// with a lock of its own, and the tables themselves lie in blocks that never move (an id is a slot, taken with an atomic add).
struct TableStore {
    static constexpr uint32_t SHARDS = 64, BLOCK = 1024, MAX_BLOCKS = 8192;
    struct Shard {
        std::mutex mu;
        std::unordered_multimap<uint64_t, uint32_t> by_hash;
    } shard[SHARDS];
    std::mutex grow_mu;
    std::atomic<rphj::DeviceLut *> lut_block[MAX_BLOCKS];
    std::atomic<rphj::TableSpec *> spec_block[MAX_BLOCKS];
    std::atomic<uint32_t> count{0};  // slots taken: never more than BLOCK * MAX_BLOCKS
    uint64_t serial = next_serial();  // tells a thread's cache of ids that it belongs to another store
    TableStore()
    {
        for (uint32_t b = 0; b < MAX_BLOCKS; b++) lut_block[b].store(nullptr, std::memory_order_relaxed), spec_block[b].store(nullptr, std::memory_order_relaxed);
    }
    ~TableStore()
    {
        for (uint32_t b = 0; b < MAX_BLOCKS; b++) {
            delete[] lut_block[b].load(std::memory_order_relaxed);
            delete[] spec_block[b].load(std::memory_order_relaxed);
        }
    }
    TableStore(const TableStore &) = delete;
    TableStore &operator=(const TableStore &) = delete;
    static uint64_t next_serial()
    {
        static std::atomic<uint64_t> n{1};
        return n.fetch_add(1);
    }
    static bool same(const rphj::TableSpec &a, const rphj::TableSpec &b)
    {
        return a.total == b.total && memcmp(a.counts + 1, b.counts + 1, 16) == 0 && memcmp(a.symbols, b.symbols, a.total) == 0;
    }
    const rphj::TableSpec &spec(uint32_t id) const { return spec_block[id / BLOCK].load(std::memory_order_acquire)[id % BLOCK]; }
    uint32_t size() const { return count.load(std::memory_order_acquire); }
    void copy_luts(rphj::DeviceLut *dst) const  // (when the threads are done)
    {
        const uint32_t n = size();
        for (uint32_t first = 0; first < n; first += BLOCK)
            memcpy(dst + first, lut_block[first / BLOCK].load(std::memory_order_acquire), (size_t)std::min(BLOCK, n - first) * sizeof(rphj::DeviceLut));
    }
    uint32_t find_locked(const Shard &sh, uint64_t h, const rphj::TableSpec &t) const
    {
        auto range = sh.by_hash.equal_range(h);
        for (auto it = range.first; it != range.second; ++it)
            if (same(spec(it->second), t)) return it->second;
        return UINT32_MAX;
    }
    uint32_t new_slot()  // UINT32_MAX: full (the file then goes to the host decoder); a full store does not count the refused slot
    {
        uint32_t id = count.load(std::memory_order_acquire);
        do {
            if (id >= BLOCK * MAX_BLOCKS) return UINT32_MAX;
        } while (!count.compare_exchange_weak(id, id + 1, std::memory_order_acq_rel, std::memory_order_acquire));
        const uint32_t b = id / BLOCK;
        if (!lut_block[b].load(std::memory_order_acquire) || !spec_block[b].load(std::memory_order_acquire)) {
            std::lock_guard<std::mutex> lock(grow_mu);
            if (!spec_block[b].load(std::memory_order_acquire)) spec_block[b].store(new rphj::TableSpec[BLOCK], std::memory_order_release);
            if (!lut_block[b].load(std::memory_order_acquire)) lut_block[b].store(new rphj::DeviceLut[BLOCK], std::memory_order_release);
        }
        return id;
    }
    // Every file of a call asks for its tables, from sixteen threads: each thread remembers the last few it was given (no lock at all
    // for them: the four tables a collection of sequential files shares); a table nobody has seen is built OUTSIDE the lock.
    static uint32_t intern(void *self, const rphj::TableSpec &t)
    {
        TableStore &T = *static_cast<TableStore *>(self);
        uint64_t h = 1469598103934665603ULL;
        for (int q = 1; q <= 16; q++) h = (h ^ t.counts[q]) * 1099511628211ULL;
        for (int q = 0; q < t.total; q++) h = (h ^ t.symbols[q]) * 1099511628211ULL;
        struct Recent {
            uint64_t serial = 0, hash[8];
            uint32_t id[8];
            rphj::TableSpec spec[8];
            int n = 0, next = 0;
        };
        static thread_local Recent recent;
        if (recent.serial != T.serial) {
            recent.serial = T.serial;
            recent.n = recent.next = 0;
        }
        for (int i = 0; i < recent.n; i++)
            if (recent.hash[i] == h && same(recent.spec[i], t)) return recent.id[i];
        Shard &sh = T.shard[(h >> 7) % SHARDS];
        uint32_t id;
        {
            std::lock_guard<std::mutex> lock(sh.mu);
            id = T.find_locked(sh, h, t);
        }
        if (id == UINT32_MAX) {
            rphj::DeviceLut L;
            if (rphj::build_device_lut(t, L) != RPH_OK) return UINT32_MAX;
            std::lock_guard<std::mutex> lock(sh.mu);
            id = T.find_locked(sh, h, t);  // (another thread may have been quicker)
            if (id == UINT32_MAX) {
                id = T.new_slot();
                if (id == UINT32_MAX) return UINT32_MAX;
                T.lut_block[id / BLOCK].load(std::memory_order_acquire)[id % BLOCK] = L;
                T.spec_block[id / BLOCK].load(std::memory_order_acquire)[id % BLOCK] = t;
                sh.by_hash.emplace(h, id);
            }
        }
        const int slot = recent.n < 8 ? recent.n++ : (recent.next = (recent.next + 1) & 7);
        recent.hash[slot] = h;
        recent.id[slot] = id;
        recent.spec[slot] = t;
        return id;
    }
};

// bytes of the chunk's stream buffer a file may need (prepare_stream: 32 zero bytes behind every scan)
inline size_t stream_cap(const Job &j) { return align_up(j.len + 160 + (j.frame.progressive ? 32 * (size_t)rphj::MAX_PROG_SCANS : 0), 16); }

// Channels of the pixels the device writes for a file: Rgb8 only where the caller reads RGB (rph_jpeg_decode, pixel hashes); a colour file that
// only the hasher reads is written as its Rec.601 luma (a third of the bytes, and the PDQ paths start from luma anyway: Luma8 input
// is borrowed as it is, pdqhash.rs:176; 512x512 Luma8 has its own form of the fused kernel)
inline uint32_t out_channels(const rphj::Frame &f, bool rgb_wanted) { return (f.ncomp == 1 || !rgb_wanted) ? 1u : 3u; }

size_t out_bytes_of(const rphj::Frame &f, uint32_t channels)
{
    const size_t stride = (size_t)channels * align_up(f.w, 8);
    return align_up(stride * f.h, 64);
}

inline double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
inline int trace_level()  // RPH_JPEG_TRACE=1: synchronise after every device phase and print its time; 2: host-side timestamps only (no extra synchronisation)
{
    static const int level = getenv("RPH_JPEG_TRACE") ? atoi(getenv("RPH_JPEG_TRACE")) : 0;
    return level;
}
inline bool trace_on() { return trace_level() == 1; }
#define RPH_JPEG_STAMP(...)                                   \
    do {                                                      \
        if (trace_level() == 2) {                             \
            fprintf(stderr, "[rph_jpeg %9.1f ms] ", now_ms() - g_trace_t0); \
            fprintf(stderr, __VA_ARGS__);                     \
            fprintf(stderr, "\n");                            \
        }                                                     \
    } while (0)
static double g_trace_t0 = 0;

struct Outputs {
    uint8_t *hash = nullptr, *dihedral = nullptr, *valid = nullptr;
    float *quality = nullptr, *coeffs = nullptr;
    int32_t *status = nullptr;
    uint8_t *pixels = nullptr;  // single-image decode: packed w * h * channels
    uint8_t *pixel_hash = nullptr;  // n x 32: BLAKE3 of to_rgba16() of every decoded image (rph_jpeg_pdq_pixel_hash_batch)
    bool want_hash = true;
    bool rgb_wanted() const { return pixels || pixel_hash; }  // colour files reconstructed as Rgb8 (no luma-only fused kernel)
};

// Reconstruction descriptors of the chunk idx[first..last): planes | images | quantisation tables at the start of the slot's meta buffer
// (host and device at the same offsets)
struct ChunkDesc {
    size_t bytes = 0;                  // of the three sections
    JPlane *planes = nullptr;          // host side
    JImage *images = nullptr;
    const JPlane *d_planes = nullptr;  // device side
    const JImage *d_images = nullptr;
    const uint16_t *d_tables = nullptr;
    std::vector<uint32_t> image_of, plane_of;  // per chunk position: index of its JImage / first JPlane (UINT32_MAX: not decodable)
    uint32_t n_planes = 0, n_images = 0;
    const PRef *d_refs = nullptr;   // device entropy, progressive files: the AC refinement scans of their planes and the records of
    const PCorr *d_corr = nullptr;  // their corrections (the IDCT kernel applies them)
    const uint8_t *d_dcbits = nullptr;
    std::vector<size_t> sub_starts;  // first chunk position of every sub-batch (build_descriptors)
};

// Sub-batch boundaries are where the offsets of planes and pixels restart from 0 (D.sub_starts).
int build_descriptors(Jobs &jobs, const std::vector<uint32_t> &idx, size_t first, size_t last, int flavour, bool rgb_wanted, size_t sub_coef_bytes, const Twin &meta,
                      ChunkDesc &D)
{
    const size_t m = last - first;
    Layout L;
    const size_t off_planes = L.add(m * 3 * sizeof(JPlane)), off_images = L.add(m * sizeof(JImage)), off_tables = L.add(m * 3 * 128);
    D.bytes = L.end();
    D.planes = reinterpret_cast<JPlane *>(meta.h.data() + off_planes);
    D.images = reinterpret_cast<JImage *>(meta.h.data() + off_images);
    uint16_t *hq = reinterpret_cast<uint16_t *>(meta.h.data() + off_tables);
    D.d_planes = reinterpret_cast<const JPlane *>(meta.d.data() + off_planes);
    D.d_images = reinterpret_cast<const JImage *>(meta.d.data() + off_images);
    D.d_tables = reinterpret_cast<const uint16_t *>(meta.d.data() + off_tables);
    D.image_of.assign(m, UINT32_MAX);
    D.plane_of.assign(m, UINT32_MAX);
    D.n_planes = D.n_images = 0;
    D.sub_starts.assign(1, 0);
    size_t plane_bytes = 0, out_bytes = 0, sub_blocks = 0, sub_images = 0;
    uint32_t sub_first_plane = 0;
    static const bool fuse = !getenv("RPH_JPEG_NO_FUSED");  // (A/B: the two-kernel reconstruction for every image)
    for (size_t r = 0; r < m; r++) {
        Job &j = jobs[idx[first + r]];
        if (j.status != RPH_OK) continue;
        const rphj::Frame &f = j.frame;
        // a sub-batch is full when its coefficients would not fit the reconstruction buffers, or at 16 384 images (the kernels take
        // the plane / image index from blockIdx.y, which ends at 65 535): offsets restart
        if (sub_blocks && ((sub_blocks + f.total_blocks) * 128 > sub_coef_bytes || sub_images == SUB_MAX_IMAGES)) {
            D.sub_starts.push_back(r);
            plane_bytes = out_bytes = sub_blocks = 0;
            sub_images = 0;
            sub_first_plane = D.n_planes;
        }
        sub_blocks += f.total_blocks;
        sub_images++;
        JImage im;
        memset(&im, 0, sizeof im);
        D.plane_of[r] = D.n_planes;
        // three components (luma sampled once or twice the chroma) and only the hasher reads the pixels: IDCT + upsampling + colour in one kernel
        const bool fused = fuse && f.ncomp == 3 && out_channels(f, rgb_wanted) == 1 && f.comp[0].H <= 2 && f.comp[0].V <= 2 && f.comp[1].H == 1 && f.comp[1].V == 1 &&
                           f.comp[2].H == 1 && f.comp[2].V == 1;
        im.fused = fused, im.first_plane = D.n_planes - sub_first_plane;
        im.tiles_x = (f.comp[0].blocks_w + 15) / 16, im.tiles_y = (f.comp[0].blocks_h + 7) / 8;
        for (int c = 0; c < f.ncomp; c++) {
            const rphj::Comp &kc = f.comp[c];
            const JPlane pl{j.first_block + kc.first_block, plane_bytes, kc.blocks_w, kc.blocks_h, D.n_planes, kc.blocks_w * 8, kc.real_bw, kc.real_bh, 0, 0, fused, 0};
            memcpy(hq + (size_t)D.n_planes * 64, f.qt[kc.tq], 128);
            im.plane_off[c] = plane_bytes;
            im.pitch[c] = pl.pitch;
            plane_bytes += (size_t)pl.pitch * kc.blocks_h * 8;
            D.planes[D.n_planes++] = pl;
        }
        im.w = f.w, im.h = f.h, im.ncomp = (uint32_t)f.ncomp;
        im.hs = im.vs = 1;
        if (f.ncomp == 3) {
            im.hs = f.comp[0].H / f.comp[1].H, im.vs = f.comp[0].V / f.comp[1].V;
            im.cw = flavour == RPH_JPEG_LIBJPEG ? f.comp[1].samp_w : f.comp[1].blocks_w * 8;
            im.ch = flavour == RPH_JPEG_LIBJPEG ? f.comp[1].samp_h : f.comp[1].blocks_h * 8;
        }
        const uint32_t och = out_channels(f, rgb_wanted);
        im.luma_out = f.ncomp == 3 && och == 1;
        im.out_stride = (uint32_t)((size_t)och * align_up(f.w, 8)), im.out_off = out_bytes;
        out_bytes += out_bytes_of(f, och);
        D.image_of[r] = D.n_images;
        D.images[D.n_images++] = im;
    }
    return RPH_OK;
}

// IDCT + upsampling / colour + hashing of chunk positions [r0, r1) (one sub-batch: its planes and pixels fit the slot's reconstruction buffers)
int reconstruct_and_hash(rph_ctx *ctx, JpegPipe &P, int b, Slot &S, Jobs &jobs, const std::vector<uint32_t> &idx, size_t first, const ChunkDesc &D, size_t r0,
                         size_t r1, const int16_t *d_coef, int flavour, const Outputs &out, hipStream_t s)
{
    // the planes and images of the sub-batch are contiguous in the descriptor arrays
    uint32_t p0 = UINT32_MAX, p1 = 0, i0 = UINT32_MAX, i1 = 0, max_blocks = 0, max_groups = 0;
    for (size_t r = r0; r < r1; r++) {
        if (D.image_of[r] == UINT32_MAX) continue;
        const rphj::Frame &f = jobs[idx[first + r]].frame;
        p0 = std::min(p0, D.plane_of[r]);
        p1 = std::max(p1, D.plane_of[r] + (uint32_t)f.ncomp);
        i0 = std::min(i0, D.image_of[r]);
        i1 = std::max(i1, D.image_of[r] + 1);
        for (int c = 0; c < f.ncomp; c++) max_blocks = std::max(max_blocks, f.comp[c].blocks_w * f.comp[c].blocks_h);
        max_groups = std::max<uint32_t>(max_groups, (uint32_t)(((f.w + 7) / 8) * (size_t)f.h));
    }
    if (i0 == UINT32_MAX) return RPH_OK;
    const JPlane *dp = D.d_planes + p0;
    const JImage *di = D.d_images + i0;
    uint32_t n_fused = 0, max_tiles = 0;
    for (uint32_t q = i0; q < i1; q++)
        if (D.images[q].fused) {
            n_fused++;
            max_tiles = std::max(max_tiles, D.images[q].tiles_x * D.images[q].tiles_y);
        }
    if (n_fused < i1 - i0) {  // (the plane kernels skip the images the fused kernel takes)
        RPH_TRY(rph_jpeg_launch_idct(flavour, max_blocks, p1 - p0, s, d_coef, D.d_tables, dp, P.planes[b].data(), D.d_refs, D.d_corr, D.d_dcbits));
        RPH_TRY(rph_jpeg_launch_color(flavour, max_groups, i1 - i0, s, P.planes[b].data(), di, P.pixels[b].data()));
    }
    if (n_fused) RPH_TRY(rph_jpeg_launch_fused(flavour, max_tiles, i1 - i0, s, d_coef, D.d_tables, dp, di, P.pixels[b].data(), D.d_refs, D.d_corr, D.d_dcbits));
    ResView R(S.res.data(), S.res_images);
    // pixel hashes (scanner.rs:1393-1404, before generate_pdq_features: images below 5 px have one too), runs of equal geometry
    for (size_t r = r0; out.pixel_hash && r < r1;) {
        if (D.image_of[r] == UINT32_MAX) {
            r++;
            continue;
        }
        const rphj::Frame &f = jobs[idx[first + r]].frame;
        const uint32_t och = out_channels(f, true);
        size_t e = r + 1;
        while (e < r1 && D.image_of[e] != UINT32_MAX && jobs[idx[first + e]].frame.w == f.w && jobs[idx[first + e]].frame.h == f.h && jobs[idx[first + e]].frame.ncomp == f.ncomp) e++;
        const size_t scratch = rph_pixel_hash_scratch_bytes((uint32_t)(e - r), f.w, f.h);
        if (scratch) RPH_TRY(P.b3[b].reserve(scratch, scratch + scratch / 4, s));  // (runs of one stream follow each other: one buffer serves them all)
        RPH_TRY(rph_launch_pixel_hash(P.pixels[b].data() + D.images[D.image_of[r]].out_off, (uint32_t)(e - r), f.w, f.h, och, (size_t)och * align_up(f.w, 8), out_bytes_of(f, och),
                                      R.pixel + r * 32, s, P.b3[b].data()));
        r = e;
    }
    if (!out.want_hash) return RPH_OK;
    // hash runs of equal geometry where the pixels lie (generate_pdq_features, scanner.rs:1410)
    for (size_t r = r0; r < r1;) {
        if (D.image_of[r] == UINT32_MAX) {
            r++;
            continue;
        }
        const rphj::Frame &f = jobs[idx[first + r]].frame;
        const uint32_t och = out_channels(f, out.rgb_wanted());
        size_t e = r + 1;
        while (e < r1 && D.image_of[e] != UINT32_MAX && jobs[idx[first + e]].frame.w == f.w && jobs[idx[first + e]].frame.h == f.h && jobs[idx[first + e]].frame.ncomp == f.ncomp) e++;
        RPH_TRY(rph_pdq_hash_batch_dev(ctx, P.pixels[b].data() + D.images[D.image_of[r]].out_off, (uint32_t)(e - r), f.w, f.h, och, (size_t)och * align_up(f.w, 8), out_bytes_of(f, och),
                                       R.hash + r * 32, out.quality ? R.quality + r * 4 : nullptr, out.coeffs ? R.coeffs + r * 1024 : nullptr,
                                       out.dihedral ? R.dihedral + r * 256 : nullptr, R.valid + r, s));
        r = e;
    }
    return RPH_OK;
}

// the first m entries of the slot's result arrays cleared by the host (the lane is idle: its previous chunk has delivered)
void zero_results(Slot &S, size_t m, const Outputs &out)
{
    ResView H(S.res.data(), S.res_images);
    memset(H.hash, 0, m * 32);
    memset(H.quality, 0, m * 4);
    if (out.coeffs) memset(H.coeffs, 0, m * 1024);
    if (out.dihedral) memset(H.dihedral, 0, m * 256);
    memset(H.valid, 0, m);
    memset(H.status, 0, m);
    if (out.pixel_hash) memset(H.pixel, 0, m * 32);
}

// results of a finished chunk -> the caller's arrays (scattered through idx); the kernels wrote them into the slot's pinned results buffer
// retry (device entropy): files the device walk flagged (a damaged stream, or a progressive wait that gave up: the status byte says which)
// are not written; they go to the host decoder, whose verdict is final (rupphash.h, rph_jpeg_set_entropy)
void scatter_results(const Slot &S, Jobs &jobs, const std::vector<uint32_t> &idx, size_t first, size_t last, const Outputs &out,
                     std::vector<uint32_t> *retry)
{
    ResView R(S.res.data(), S.res_images);
    for (size_t r = 0; r < last - first; r++) {
        const uint32_t g = idx[first + r];
        Job &j = jobs[g];
        if (retry && j.status == RPH_OK && R.status[r]) {
            retry->push_back(g);
            continue;
        }
        const bool ok = j.status == RPH_OK;
        if (out.hash) ok ? (void)memcpy(out.hash + (size_t)g * 32, R.hash + r * 32, 32) : (void)memset(out.hash + (size_t)g * 32, 0, 32);
        if (out.quality) ok ? (void)memcpy(out.quality + g, R.quality + r * 4, 4) : (void)memset(out.quality + g, 0, 4);
        if (out.coeffs) ok ? (void)memcpy(out.coeffs + (size_t)g * 256, R.coeffs + r * 1024, 1024) : (void)memset(out.coeffs + (size_t)g * 256, 0, 1024);
        if (out.dihedral) ok ? (void)memcpy(out.dihedral + (size_t)g * 256, R.dihedral + r * 256, 256) : (void)memset(out.dihedral + (size_t)g * 256, 0, 256);
        if (out.valid) out.valid[g] = ok ? R.valid[r] : 0;
        if (out.pixel_hash) ok ? (void)memcpy(out.pixel_hash + (size_t)g * 32, R.pixel + r * 32, 32) : (void)memset(out.pixel_hash + (size_t)g * 32, 0, 32);
    }
}

// The chunk lane b has in flight: positions idx[first, last) of the call's file list
struct InFlight {
    bool active = false;
    size_t first = 0, last = 0;
    // frees the lane: waits for the chunk, if any -- for the slot's event `done` (device entropy) or its stream (host entropy) -- and
    // scatters its results (retry: as scatter_results)
    int finish(int b, const Slot &S, bool on_event, Jobs &jobs, const std::vector<uint32_t> &idx, const Outputs &out, std::vector<uint32_t> *retry)
    {
        if (!active) return RPH_OK;
        RPH_JPEG_STAMP("lane %d: waiting for its chunk", b);
        RPH_HIP_CHECK(on_event ? hipEventSynchronize(S.done) : hipStreamSynchronize(S.stream));
        RPH_JPEG_STAMP("lane %d: chunk done", b);
        scatter_results(S, jobs, idx, first, last, out, retry);
        RPH_JPEG_STAMP("lane %d: results scattered", b);
        active = false;
        return RPH_OK;
    }
};

// ---- host entropy decoding: the files idx[...] in chunks over the two slots
int run_host_entropy(rph_ctx *ctx, JpegPipe &P, Jobs &jobs, const std::vector<uint32_t> &idx, int flavour, unsigned threads, const Outputs &out)
{
    InFlight lane[2];
    const size_t n = idx.size();
    int k = 0;
    RPH_JPEG_STAMP("buffers ready");
    for (size_t first = 0; first < n; k++) {
        size_t last = first, blocks = 0;
        while (last < n && last - first < CHUNK_MAX_IMAGES) {
            const Job &j = jobs[idx[last]];
            const size_t nb = j.status == RPH_OK ? (size_t)j.frame.total_blocks : 0;
            if (last > first && (blocks + nb) * 128 > CHUNK_COEF_BYTES) break;
            blocks += nb;
            last++;
        }
        const int b = k & 1;
        RPH_TRY(lane[b].finish(b, P.slot[b], false, jobs, idx, out, nullptr));
        Slot &S = P.slot[b];
        RPH_TRY(S.ready());
        const size_t m = last - first;
        const size_t coef_need = std::max(CHUNK_COEF_BYTES, blocks * 128);
        RPH_TRY(S.coef.reserve(coef_need, S.stream));
        RPH_TRY(P.reserve_recon(b, coef_need, S.stream));
        RPH_TRY(S.reserve_res(std::max<size_t>(m, std::min<size_t>(n, CHUNK_MAX_IMAGES)), out.pixel_hash != nullptr));
        const size_t meta_need = std::max<size_t>(m, std::min<size_t>(n, CHUNK_MAX_IMAGES)) * (3 * sizeof(JPlane) + sizeof(JImage) + 3 * 128);
        RPH_TRY(S.meta.reserve(meta_need, S.stream));
        uint64_t fb = 0;
        for (size_t i = first; i < last; i++) {
            Job &j = jobs[idx[i]];
            j.first_block = fb;
            if (j.status == RPH_OK) fb += j.frame.total_blocks;
        }
        int16_t *h_coef = reinterpret_cast<int16_t *>(S.coef.h.data());
        bool predecoded = false;
        for (size_t i = first; i < last; i++) predecoded |= jobs[idx[i]].pre != nullptr;
        if (!predecoded)
            parallel_for(first, last, threads, [&](size_t i) {
                Job &j = jobs[idx[i]];
                if (j.status == RPH_OK) j.status = rphj::decode_coefficients(j.data, j.len, j.frame, h_coef + j.first_block * 64);
            });
        RPH_JPEG_STAMP("lane %d: chunk %d buffers sized", b, k);
        ChunkDesc D;
        RPH_TRY(build_descriptors(jobs, idx, first, last, flavour, out.rgb_wanted(), SIZE_MAX / 256, S.meta, D));
        hipStream_t s = S.stream;
        zero_results(S, m, out);
        if (D.n_images) {
            if (predecoded) {  // every caller decoded into its own pinned buffer: the copy engine takes the coefficients from there
                for (size_t i = first; i < last; i++) {
                    const Job &j = jobs[idx[i]];
                    if (j.status == RPH_OK)
                        RPH_HIP_CHECK(hipMemcpyAsync(S.coef.d.data() + j.first_block * 128, j.pre, (size_t)j.frame.total_blocks * 128, hipMemcpyHostToDevice, s));
                }
            } else {
                RPH_HIP_CHECK(hipMemcpyAsync(S.coef.d.data(), S.coef.h.data(), blocks * 128, hipMemcpyHostToDevice, s));
            }
            RPH_HIP_CHECK(hipMemcpyAsync(S.meta.d.data(), S.meta.h.data(), D.bytes, hipMemcpyHostToDevice, s));
            RPH_TRY(reconstruct_and_hash(ctx, P, b, S, jobs, idx, first, D, 0, m, reinterpret_cast<const int16_t *>(S.coef.d.data()), flavour, out, s));
        }
        if (out.pixels && m == 1 && jobs[idx[first]].status == RPH_OK) {  // single-image decode: rows without their padding
            const rphj::Frame &f = jobs[idx[first]].frame;
            const size_t row = (size_t)f.ncomp * f.w, stride = (size_t)f.ncomp * align_up(f.w, 8);
            RPH_HIP_CHECK(hipMemcpy2DAsync(out.pixels, row, P.pixels[b].data(), stride, row, f.h, hipMemcpyDeviceToHost, s));
        }
        lane[b] = InFlight{true, first, last};
        first = last;
    }
    RPH_TRY(lane[k & 1].finish(k & 1, P.slot[k & 1], false, jobs, idx, out, nullptr));
    RPH_TRY(lane[(k + 1) & 1].finish((k + 1) & 1, P.slot[(k + 1) & 1], false, jobs, idx, out, nullptr));
    return RPH_OK;
}

// ---- device entropy decoding: the files idx[...]; files the device walk does not take come back in `leftover` for the host
// The walk of one lane takes ~0.65 us per entropy byte however few lanes there are (21 ms for 29 KB files, 236 ms for 366 KB photos)
constexpr double WALK_SECONDS_PER_BYTE = 0.65e-6;
// entropy bytes per second the segment passes (synchronisation + walk) move when the device is theirs: 2 GB in 14 + 18 ms
inline double seg_rate()
{
    static const double r = getenv("RPH_JPEG_SEG_RATE") ? atof(getenv("RPH_JPEG_SEG_RATE")) * 1e9 : 60e9;
    return r;
}
// Segments (three decoding passes over every byte, but a lane per KB) or one lane per file (one pass, as long as the longest file)?
// The walk of whole files takes ~0.65 us per byte of the longest one while there are fewer lanes than the device has (65 536); the
// segment passes move ~31 GB/s of entropy bytes (5 275 photos of 366 KB: 67 ms against 236; 25 000 files of 158 KB: 129 ms against
// 103).  Whole-file walks also leave most of the device to the other lane's chunk, so segments must win clearly.
// `files` files of `bytes` entropy bytes in all, the longest of them `longest` bytes.
inline bool segments_pay(size_t longest, double files, double bytes)
{
    const double t_whole = WALK_SECONDS_PER_BYTE * (double)longest * std::max(1.0, files / 65536.0), t_seg = bytes / seg_rate();
    return t_seg < 0.7 * t_whole;
}

// How a call's device-entropy files are cut into chunks: `lanes` chunks in flight, `region` bytes of the coefficient buffer per lane,
// chunks of at most `chunk_bytes` of coefficients (one larger image makes a chunk of its own)
struct DevicePlan { int lanes = 1; size_t region = 0, chunk_bytes = 0; };
// ---- call plan: sorts idx, sizes the coefficient buffer, readies the lanes' slots and reconstruction buffers
int plan_device_call(rph_ctx *ctx, JpegPipe &P, const Jobs &jobs, std::vector<uint32_t> &idx, DevicePlan &plan)
{
    // images of similar stream length share a wave: sort the whole list by file length first (chunks then are slices of it)
    {  // (keys side by side: sorting through the job records themselves took 22 ms per 100 000 files)
        std::vector<std::pair<uint64_t, uint32_t>> key(idx.size());
        for (size_t i = 0; i < idx.size(); i++) key[i] = {~(uint64_t)jobs[idx[i]].len, (uint32_t)i};  // longest first, equal lengths as they came
        std::sort(key.begin(), key.end());
        std::vector<uint32_t> sorted(idx.size());
        for (size_t i = 0; i < idx.size(); i++) sorted[i] = idx[key[i].second];
        idx.swap(sorted);
    }
    RPH_JPEG_STAMP("files sorted by length");
    // the chunk's coefficient buffer: as much of the free device memory as is reasonable, but no more than this call can use
    size_t need = 0;
    for (uint32_t g : idx) need += (size_t)jobs[g].frame.total_blocks * 128;
    size_t free_b = 0, total_b = 0;
    RPH_HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
    const size_t budget = std::max<size_t>((size_t)1 << 30, std::min<size_t>((free_b + P.coef.capacity()) / 2, (size_t)96 << 30));
    // Up to JPEG_LANES lanes of resources (stream, staging, a share of the coefficient buffer, reconstruction buffers), chunks take them in
    // turn: the host prepares chunk k + 1 and its bytes cross PCIe while chunk k is on the device, and the latency-bound walk of one
    // chunk runs beside the bandwidth-bound reconstruction of the other.  A call is cut into about four chunks when it is large
    // enough for each to still fill the device's lanes (16 GB of coefficients = 20 000 images of 512x512); a smaller call is one chunk.
    // The walk of a chunk takes as long as its longest file (WALK_SECONDS_PER_BYTE) however few files it has, and walks of different
    // chunks only overlap pairwise (two lanes): small files are cut into four chunks for the pipelining, files whose lanes have long
    // streams (photos without markers, segments switched off) into two so that the walks are not paid four times.
    size_t max_len = 0;  // longest stream one lane will walk: a file, or one restart interval of it (as the frame header announces them)
    size_t longest_plain = 0, plain_bytes = 0, plain_files = 0;  // files without restart intervals that are long enough for segments
    for (uint32_t g : idx) {
        const rphj::Frame &f = jobs[g].frame;
        const uint64_t mcus = (uint64_t)f.mcus_x * f.mcus_y, intervals = f.restart_interval ? (mcus + f.restart_interval - 1) / f.restart_interval : 1;
        const size_t lane_len = jobs[g].len / (size_t)std::max<uint64_t>(1, intervals);
        if (!f.restart_interval && !f.progressive && ctx->jpeg_seg_bytes && jobs[g].len >= ctx->jpeg_seg_min_bytes) {
            longest_plain = std::max(longest_plain, jobs[g].len), plain_bytes += jobs[g].len, plain_files++;
            continue;
        }
        max_len = std::max(max_len, lane_len);
    }
    bool by_segments = false;
    if (plain_files) {  // will a quarter of them be walked as segments (list_sequential decides the same way, per chunk)?
        by_segments = segments_pay(longest_plain, (double)plain_files / 4, (double)plain_bytes / 4);
        max_len = std::max(max_len, by_segments ? (size_t)ctx->jpeg_seg_bytes : longest_plain);
    }
    const bool long_lanes = WALK_SECONDS_PER_BYTE * (double)max_len > 0.08;
    size_t min_chunk = (size_t)16 << 30, parts = long_lanes ? 2 : 4;
    // A call whose long streams are cut into segments has no long lane: its walk scales with the bytes, and the call is bound by PCIe
    // (the entropy bytes of 20 000 photos cross it in 143 ms of the call's 240).  Many small chunks then keep the copy engine busy from
    // the first prepared chunk to the last and leave little device work behind the last upload (20 000 photos: 4 chunks 75 k files/s,
    // 8 chunks 81 k, 16 chunks 86 k, 32 chunks 71 k).
    if (by_segments && !long_lanes) min_chunk = (size_t)4 << 30, parts = 16;
    if (const char *e = getenv("RPH_JPEG_CHUNK_GB")) min_chunk = (size_t)atoi(e) << 30;  // experiments
    if (const char *e = getenv("RPH_JPEG_PARTS")) parts = (size_t)std::max(1, atoi(e));
    const size_t chunk_target = std::min(need, std::max(need / parts + 128, min_chunk));
    const bool single = need <= chunk_target && need <= budget;
    plan.lanes = single ? 1 : (int)std::min<size_t>(JPEG_LANES, (need + chunk_target - 1) / chunk_target);
    const size_t want = single ? need : std::min(budget, (size_t)plan.lanes * chunk_target);
    if (P.coef.capacity() < want) RPH_HIP_CHECK(hipDeviceSynchronize());  // every lane's stream may still use it
    RPH_TRY(P.coef.reserve(want, synced));
    plan.region = (P.coef.capacity() / (size_t)plan.lanes) / 128 * 128;
    plan.chunk_bytes = std::min(plan.region, chunk_target);
    for (int b = 0; b < plan.lanes; b++) RPH_TRY(P.slot[b].ready());
    size_t max_img = 0;  // a sub-batch holds at least one image
    for (uint32_t g : idx) max_img = std::max(max_img, (size_t)jobs[g].frame.total_blocks * 128);
    const size_t recon = std::max(std::min(SUB_COEF_BYTES, std::max(std::min(want, plan.chunk_bytes), (size_t)64 << 20)), max_img);
    for (int b = 0; b < plan.lanes; b++) RPH_TRY(P.reserve_recon(b, recon, P.slot[b].stream));
    return RPH_OK;
}

// One chunk: positions idx[first, last) of the call's sorted list, with `blocks` coefficient blocks and `file_bytes` of the slot's stream
// buffer (stream_cap); the call's k-th chunk, on lane b
struct Chunk {
    size_t first = 0, last = 0, blocks = 0, file_bytes = 0;
    int b = 0, k = 0;
    size_t m() const { return last - first; }
};

// the walk's record of a file that prepare_stream has accepted (`hi` zeroed before)
void fill_himage(const Job &j, HImage &hi)
{
    const rphj::Frame &f = j.frame;
    hi.first_block = j.first_block, hi.stream_base = j.stream_off;
    hi.mcus_x = f.mcus_x, hi.mcus_y = f.mcus_y;
    hi.n_scans = f.progressive ? 0u : (uint32_t)j.plan.n_scans, hi.ncomp = (uint32_t)f.ncomp;
    for (int c = 0; c < f.ncomp; c++) {
        const rphj::Comp &kc = f.comp[c];
        hi.comp[c] = HComp{kc.blocks_w, kc.real_bw, kc.real_bh, (uint32_t)kc.first_block, kc.H, kc.V};
    }
    for (int q = 0; q < (f.progressive ? 0 : j.plan.n_scans); q++) {
        const rphj::ScanPlan &sp = j.plan.scan[q];
        HScan &hs = hi.scan[q];
        hs.off = sp.stream_off, hs.len = sp.stream_len, hs.restart_interval = sp.restart_interval, hs.ns = sp.ns;
        for (int c = 0; c < sp.ns; c++) hs.ci[c] = sp.ci[c], hs.dc[c] = sp.dc[c], hs.ac[c] = sp.ac[c];
    }
}

// ---- chunk preparation (host threads: memchr + memcpy): the files' places in the stream and coefficient buffers, their de-stuffed
// streams in the slot's staging, their walk records (zero where prepare_stream refused the file) and the chunk's Huffman tables
void prepare_chunk(Jobs &jobs, const std::vector<uint32_t> &idx, const Chunk &C, unsigned threads, Slot &S, TableStore &store, std::vector<HImage> &himgs)
{
    size_t off = 0;
    uint64_t fb = 0;
    for (size_t i = C.first; i < C.last; i++) {
        Job &j = jobs[idx[i]];
        j.stream_off = off;
        off += stream_cap(j);
        j.first_block = fb;
        fb += j.frame.total_blocks;
    }
    himgs.resize(C.m());
    RPH_JPEG_STAMP("lane %d: chunk %d laid out", C.b, C.k);
    parallel_for(C.first, C.last, threads, [&](size_t i) {
        Job &j = jobs[idx[i]];
        HImage &hi = himgs[i - C.first];
        memset(&hi, 0, sizeof hi);
        j.status = rphj::prepare_stream(j.data, j.len, j.frame, j.plan, S.stream_bytes.h.data() + j.stream_off, stream_cap(j), &j.stream_used, &TableStore::intern, &store, &j.marks);
        if (j.status == RPH_OK) fill_himage(j, hi);
    });
}

// The walk items of a chunk's sequential files
struct SeqWork {
    std::vector<HItem> items;        // the host's: one per restart interval where a file has them, else one per file
    std::vector<uint32_t> order;     // the host's items, longest first (the lanes take them in this order)
    std::vector<SegFile> seg_files;  // long streams without markers, cut into segments
    uint32_t n_segs = 0, n_items = 0;  // n_items: the host's items, then one per segment (the device writes those)
    bool all_one_scan = true;        // every sequential file of the chunk has one scan: its MCUs cover all blocks of its components
};
// ---- sequential work.  Files that prepare_stream refused (more than four scans, damage it saw) go to `leftover` for the host decoder;
// they keep their place in the chunk as holes.  Progressive files are ProgPlan's.
SeqWork list_sequential(const rph_ctx *ctx, const Jobs &jobs, const std::vector<uint32_t> &idx, const Chunk &C, std::vector<uint32_t> &leftover)
{
    SeqWork W;
    bool use_segments = ctx->jpeg_seg_bytes != 0;
    if (use_segments && ctx->jpeg_seg_min_bytes > 0) use_segments = segments_pay(jobs[idx[C.first]].len, (double)C.m(), (double)C.file_bytes);
    std::vector<uint32_t> item_len;
    W.items.reserve(C.m());
    for (size_t i = C.first; i < C.last; i++) {
        const Job &j = jobs[idx[i]];
        if (j.status != RPH_OK) {  // whatever prepare_stream found, the host decoder judges the file
            leftover.push_back(idx[i]);
            continue;
        }
        if (j.frame.progressive) continue;
        const uint32_t r = (uint32_t)(i - C.first);
        const rphj::Frame &f = j.frame;
        const rphj::ScanPlan &sp = j.plan.scan[0];
        if (j.plan.n_scans != 1 || sp.ns != f.ncomp) W.all_one_scan = false;
        if (f.ncomp == 1 && (f.comp[0].blocks_w != f.comp[0].real_bw || f.comp[0].blocks_h != f.comp[0].real_bh))
            W.all_one_scan = false;  // (a one-component scan walks the real blocks only: a padded grid keeps its zeroing)
        if (j.marks.empty()) {
            if (use_segments && j.plan.n_scans == 1 && sp.restart_interval == 0 && sp.stream_len >= ctx->jpeg_seg_min_bytes && sp.stream_len < ((uint32_t)1 << 28)) {
                // a long stream without restart markers: cut into segments that synchronise on the device (jpeg_device.h); its items go
                // behind the host's (first_item, set below)
                const uint32_t n_segs = (sp.stream_len + ctx->jpeg_seg_bytes - 1) / ctx->jpeg_seg_bytes;
                const uint32_t total_mcus = sp.ns == 1 ? f.comp[sp.ci[0]].real_bw * f.comp[sp.ci[0]].real_bh : f.mcus_x * f.mcus_y;
                W.seg_files.push_back(SegFile{r, W.n_segs, n_segs, 0, total_mcus, sp.stream_len * 8});
                W.n_segs += n_segs;
                continue;
            }
            W.items.push_back(HItem{r, HITEM_ALL_SCANS, 0, 0, 0, 0, {0, 0, 0}, HITEM_NO_END});
            item_len.push_back((uint32_t)std::min<size_t>(j.len, 0xFFFFFFFFu));
            continue;
        }
        const uint64_t mcus = sp.ns == 1 ? (uint64_t)f.comp[sp.ci[0]].real_bw * f.comp[sp.ci[0]].real_bh : (uint64_t)f.mcus_x * f.mcus_y;
        const uint32_t n_int = (uint32_t)j.marks.size() + 1;
        for (uint32_t q = 0; q < n_int; q++) {
            const uint32_t off = q ? j.marks[q - 1] : 0, end = q + 1 < n_int ? j.marks[q] : sp.stream_len;
            const uint64_t m_first = (uint64_t)q * sp.restart_interval;
            W.items.push_back(HItem{r, 0, (uint32_t)m_first, (uint32_t)std::min<uint64_t>(sp.restart_interval, mcus - m_first), off, 0, {0, 0, 0}, end});
            item_len.push_back(end > off ? end - off : 0);
        }
    }
    W.order.resize(W.items.size());
    for (uint32_t t = 0; t < W.order.size(); t++) W.order[t] = t;
    std::stable_sort(W.order.begin(), W.order.end(), [&](uint32_t x, uint32_t y) { return item_len[x] > item_len[y]; });
    // the segments' items follow the host's: the device writes them, and the lanes take them as they lie (they are short, so they go last)
    W.n_items = (uint32_t)W.items.size();
    for (SegFile &sf : W.seg_files) sf.first_item = W.n_items, W.n_items += sf.n_segs;
    return W;
}

// ---- progressive plan: the scans of a chunk's progressive files (one lane per scan: jpeg_prog_kernel) and what they wait for
struct ProgPlan {
    std::vector<PScan> pscans;
    std::vector<uint32_t> pwaits;  // scans (indices into pscans) that must have ended before a scan begins (PScan::wait_first / wait_count)
    std::vector<PRef> prefs;       // their refinement scans, grouped by plane (file order within a plane)
    struct PlaneRefs { uint32_t r, first[3], count[3]; };  // a file's chunk position, and per component its range of prefs
    std::vector<PlaneRefs> plane_refs;
    std::vector<uint32_t> files;  // the progressive files (chunk positions)
    // their blocks (one mask word each), the records of their AC refinement scans, the bytes of their DC refinement scans
    uint64_t blocks = 0, corr = 0, dc_bytes = 0;
    size_t mask_bytes() const { return blocks * 8 + align_up(pscans.size() * 4, 16); }  // one mask word per block, then one progress word per scan

    // the scans of the file at chunk position r, the dependencies among them and their refinement records; hi: the file's walk record
    void add(uint32_t r, const Job &j, HImage &hi)
    {
        hi.mask_first = (uint32_t)blocks;
        blocks += j.frame.total_blocks;
        hi.pscan_first = (uint32_t)pscans.size();
        hi.pscan_count = (uint32_t)j.plan.prog.size();
        const size_t p0 = pscans.size();
        for (const rphj::ScanPlan &sp : j.plan.prog) {
            PScan ps;
            ps.off = sp.stream_off, ps.len = sp.stream_len, ps.ns = sp.ns, ps.ss = sp.ss, ps.se = sp.se, ps.ah = sp.ah, ps.al = sp.al;
            for (int c = 0; c < 3; c++) ps.ci[c] = sp.ci[c], ps.dc[c] = sp.dc[c], ps.dcb[c] = 0;
            ps.ac = sp.ac[0], ps.image = r, ps.corr_first = 0;
            for (int c = 0; sp.ss == 0 && sp.ah > 0 && c < sp.ns && c < 3; c++) {
                const rphj::Comp &kc = j.frame.comp[sp.ci[c]];
                ps.dcb[c] = (uint32_t)dc_bytes;
                dc_bytes += (uint64_t)kc.blocks_w * kc.blocks_h;
            }
            if (sp.ss > 0 && sp.ah > 0) {
                const rphj::Comp &kc = j.frame.comp[sp.ci[0]];
                ps.corr_first = (uint32_t)corr;
                corr += (uint64_t)kc.real_bw * kc.real_bh;
            }
            // The scans this one must come after: the earlier scans of the file that share a component and a coefficient with it.
            // An AC scan follows up to two of them (the longest) block by block (PScan::chase); the others must have ended.
            ps.chase[0] = ps.chase[1] = PSCAN_NONE, ps.wait_first = (uint32_t)pwaits.size();
            uint32_t my_comps = 0;
            for (uint32_t c = 0; c < ps.ns && c < 3; c++) my_comps |= 1u << ps.ci[c];
            uint32_t deps[rphj::MAX_PROG_SCANS], n_deps = 0;
            for (size_t q = p0; q < pscans.size(); q++) {
                const PScan &e = pscans[q];
                uint32_t its = 0;
                for (uint32_t c = 0; c < e.ns && c < 3; c++) its |= 1u << e.ci[c];
                if ((its & my_comps) && e.ss <= ps.se && ps.ss <= e.se) deps[n_deps++] = (uint32_t)q;
            }
            if (ps.ss > 0) {  // (AC scans of one component walk the same raster of blocks): the two longest are followed
                for (int t = 0; t < 2; t++) {
                    uint32_t best = PSCAN_NONE;
                    for (uint32_t d = 0; d < n_deps; d++)
                        if (deps[d] != PSCAN_NONE && (best == PSCAN_NONE || pscans[deps[d]].len > pscans[deps[best]].len)) best = d;
                    if (best == PSCAN_NONE) break;
                    ps.chase[t] = deps[best];
                    deps[best] = PSCAN_NONE;
                }
                for (uint32_t d = 0; d < n_deps; d++)
                    if (deps[d] != PSCAN_NONE) pwaits.push_back(deps[d]);
            } else if (ps.ah == 0) {
                pwaits.insert(pwaits.end(), deps, deps + n_deps);
            }  // (a DC refinement scan writes its bits beside the coefficients and reads nothing: it waits for nobody)
            ps.wait_count = (uint32_t)pwaits.size() - ps.wait_first;
            pscans.push_back(ps);
        }
        PlaneRefs pr{r, {}, {}};
        for (uint32_t c = 0; c < 3; c++) {
            pr.first[c] = (uint32_t)prefs.size();
            for (size_t q = p0; q < pscans.size(); q++) {
                const PScan &x = pscans[q];
                if (x.ss > 0 && x.ah > 0 && x.ci[0] == c) prefs.push_back(PRef{x.corr_first, x.al});
                if (x.ss == 0 && x.ah > 0)
                    for (uint32_t u = 0; u < x.ns && u < 3; u++)
                        if (x.ci[u] == c) prefs.push_back(PRef{x.dcb[u], x.al | PREF_DC});
            }
            pr.count[c] = (uint32_t)prefs.size() - pr.first[c];
        }
        plane_refs.push_back(pr);
        files.push_back(r);
    }
};

// ---- wave order: the lanes of the progressive launch, one scan (index into G.pscans) or PSCAN_NONE each.  64 files of one scan script
// make a batch, and wave k of a batch walks the k-th scan of each of them -- one kind of scan per wave, and a scan's producers in earlier
// workgroups of the same launch, which start first (jpeg_kernels.hip).
std::vector<uint32_t> order_waves(const ProgPlan &G, const std::vector<HImage> &himgs)
{
    auto signature = [&](uint32_t r) {
        uint64_t h = 1469598103934665603ull;
        for (uint32_t q = 0; q < himgs[r].pscan_count; q++) {
            const PScan &x = G.pscans[himgs[r].pscan_first + q];
            const uint32_t f[6] = {x.ns, x.ss, x.se, x.ah, x.al, x.ci[0] | (x.ci[1] << 8) | (x.ci[2] << 16)};
            for (uint32_t v : f) h = (h ^ v) * 1099511628211ull;
        }
        return h;
    };
    std::vector<std::pair<uint64_t, uint32_t>> sig(G.files.size());  // (script, file), files of a script in the chunk's order: longest first
    for (size_t t = 0; t < G.files.size(); t++) sig[t] = {signature(G.files[t]), G.files[t]};
    std::stable_sort(sig.begin(), sig.end(), [](const std::pair<uint64_t, uint32_t> &a, const std::pair<uint64_t, uint32_t> &b) { return a.first < b.first; });
    // A wave = (batch, k-th scan).  Waves go into the grid by how much work still hangs on them -- their own (bytes x the rate of their
    // kind of scan) plus the longest chain of scans behind them -- so the scans on a file's critical path (libjpeg's script: luma 6-63,
    // then its two refinements) start at once for every batch and the short scans fill the slots that are left; a producer always
    // ranks above its consumers, i.e. comes first in the grid.
    struct Wave {
        double rank;
        uint32_t batch, first, count, k;  // files sig[first .. first + count), their k-th scans
    };
    std::vector<Wave> waves;
    uint32_t n_batches = 0;
    for (size_t t0 = 0; t0 < sig.size();) {
        size_t t1 = t0;
        while (t1 < sig.size() && t1 - t0 < 64 && sig[t1].first == sig[t0].first) t1++;
        const HImage &h0 = himgs[sig[t0].second];  // (the batch's longest file stands for all of them)
        const uint32_t n_scans = h0.pscan_count;
        std::vector<double> rank(n_scans, 0.0);
        for (uint32_t q = n_scans; q-- > 0;) {
            const PScan &x = G.pscans[h0.pscan_first + q];
            double behind = 0.0;
            for (uint32_t c = q + 1; c < n_scans; c++) {  // scans that wait for q or follow it
                const PScan &y = G.pscans[h0.pscan_first + c];
                bool dep = y.chase[0] == h0.pscan_first + q || y.chase[1] == h0.pscan_first + q;
                for (uint32_t w = 0; w < y.wait_count && !dep; w++) dep = G.pwaits[y.wait_first + w] == h0.pscan_first + q;
                if (dep) behind = std::max(behind, rank[c]);
            }
            rank[q] = (double)x.len * (x.ss && x.ah ? 1.05 : 0.55) + 1.0 + behind;
        }
        for (uint32_t q = 0; q < n_scans; q++) waves.push_back(Wave{rank[q], n_batches, (uint32_t)t0, (uint32_t)(t1 - t0), q});
        n_batches++;
        t0 = t1;
    }
    std::stable_sort(waves.begin(), waves.end(), [](const Wave &a, const Wave &b) { return a.rank > b.rank; });
    std::vector<uint32_t> pitems;
    pitems.reserve(waves.size() * 64);
    for (const Wave &w : waves)
        for (uint32_t l = 0; l < 64; l++) pitems.push_back(l < w.count ? himgs[sig[w.first + l].second].pscan_first + w.k : PSCAN_NONE);
    return pitems;
}

// bytes of the segments' states at the start of the slot's segment work buffer (the kernels' work area follows)
inline size_t seg_states_bytes(uint32_t n_segs) { return align_up((size_t)n_segs * sizeof(SegState), 16); }

// A chunk's meta buffer as its launches read it (device side), behind the reconstruction descriptors
struct ChunkMeta {
    ChunkDesc D;
    size_t upload_bytes = 0;  // what the host fills: everything but the segments' items
    uint32_t n_luts = 0;
    const HImage *himgs = nullptr;
    const uint32_t *order = nullptr, *pitems = nullptr, *pwaits = nullptr;
    const rphj::DeviceLut *luts = nullptr;
    const SegFile *seg_files = nullptr;
    const PScan *pscans = nullptr;
    HItem *items = nullptr;
};
// ---- meta: lays out the slot's meta buffer for a chunk, sizes the walks' work buffers and fills the meta buffer's host side:
//   reconstruction descriptors | HImage | item order | tables | SegFile | PScan | progressive files | wave lanes | PRef | waits | items
// (host and device at the same offsets; the segments' items exist on the device only: room is left for them, the upload stops before)
int write_meta(JpegPipe &P, Jobs &jobs, const std::vector<uint32_t> &idx, const Chunk &C, int flavour, bool rgb_wanted, const TableStore &store,
               const std::vector<HImage> &himgs, const SeqWork &W, const ProgPlan &G, const std::vector<uint32_t> &pitems, ChunkMeta &M)
{
    Slot &S = P.slot[C.b];
    hipStream_t s = S.stream;
    const size_t m = C.m();
    M.n_luts = store.size();  // (the tables lie in the store's blocks)
    Layout L;
    L.add(m * (3 * sizeof(JPlane) + sizeof(JImage) + 3 * 128));  // (build_descriptors)
    const size_t off_himg = L.add(m * sizeof(HImage), 16), off_order = L.add(W.order.size() * 4), off_luts = L.add(M.n_luts * sizeof(rphj::DeviceLut), 16),
                 off_segf = L.add(W.seg_files.size() * sizeof(SegFile), 16), off_pscan = L.add(G.pscans.size() * sizeof(PScan), 16),
                 off_porder = L.add(G.files.size() * 4), off_pitems = L.add(pitems.size() * 4), off_prefs = L.add(G.prefs.size() * sizeof(PRef), 16),
                 off_pwaits = L.add(G.pwaits.size() * 4, 16), off_items = L.add(W.items.size() * sizeof(HItem), 16);
    M.upload_bytes = L.end();
    RPH_TRY(S.meta.reserve(off_items + (size_t)W.n_items * sizeof(HItem), s));
    // the walks' work buffers: segment states and work, the progressive files' masks, correction records and DC bits
    const size_t segwork = seg_states_bytes(W.n_segs) + rph_jpeg_segment_work_bytes(W.n_segs);
    if (W.n_segs) RPH_TRY(S.segwork.reserve(segwork, segwork + segwork / 4, s));
    if (G.blocks >= ((uint64_t)1 << 32)) return RPH_ERR_CAPACITY;  // (a chunk's coefficients are capped far below: 2^32 blocks are 512 GB)
    if (G.corr >= ((uint64_t)1 << 32) || G.dc_bytes >= ((uint64_t)1 << 32)) return RPH_ERR_CAPACITY;
    if (G.dc_bytes) RPH_TRY(S.pdc.reserve(G.dc_bytes, G.dc_bytes + G.dc_bytes / 4 + 64, s));
    if (G.corr) RPH_TRY(S.pcorr.reserve(G.corr * sizeof(PCorr), G.corr * sizeof(PCorr) + G.corr * 4, s));
    if (G.blocks) RPH_TRY(S.pmask.reserve(G.mask_bytes(), G.mask_bytes() + G.mask_bytes() / 4, s));
    RPH_TRY(build_descriptors(jobs, idx, C.first, C.last, flavour, rgb_wanted, P.recon_coef_bytes[C.b], S.meta, M.D));
    uint8_t *h = S.meta.h.data();
    const uint8_t *d = S.meta.d.data();
    memcpy(h + off_himg, himgs.data(), m * sizeof(HImage));
    memcpy(h + off_items, W.items.data(), W.items.size() * sizeof(HItem));
    memcpy(h + off_order, W.order.data(), W.order.size() * 4);
    if (M.n_luts) store.copy_luts(reinterpret_cast<rphj::DeviceLut *>(h + off_luts));
    if (W.n_segs) memcpy(h + off_segf, W.seg_files.data(), W.seg_files.size() * sizeof(SegFile));
    if (!G.files.empty()) {
        memcpy(h + off_pscan, G.pscans.data(), G.pscans.size() * sizeof(PScan));
        memcpy(h + off_porder, G.files.data(), G.files.size() * 4);
        memcpy(h + off_pitems, pitems.data(), pitems.size() * 4);
        if (!G.pwaits.empty()) memcpy(h + off_pwaits, G.pwaits.data(), G.pwaits.size() * 4);
        if (!G.prefs.empty()) {
            memcpy(h + off_prefs, G.prefs.data(), G.prefs.size() * sizeof(PRef));
            for (const ProgPlan::PlaneRefs &pr : G.plane_refs) {
                if (M.D.plane_of[pr.r] == UINT32_MAX) continue;
                JPlane *pl = M.D.planes + M.D.plane_of[pr.r];
                const int nc = jobs[idx[C.first + pr.r]].frame.ncomp;
                for (int c = 0; c < nc && c < 3; c++) pl[c].ref_first = pr.first[c], pl[c].ref_count = pr.count[c];
            }
            M.D.d_refs = reinterpret_cast<const PRef *>(d + off_prefs);
            M.D.d_corr = S.pcorr.as<PCorr>();
            M.D.d_dcbits = S.pdc.data();
        }
    }
    M.himgs = reinterpret_cast<const HImage *>(d + off_himg), M.luts = reinterpret_cast<const rphj::DeviceLut *>(d + off_luts);
    M.order = reinterpret_cast<const uint32_t *>(d + off_order), M.seg_files = reinterpret_cast<const SegFile *>(d + off_segf);
    M.pscans = reinterpret_cast<const PScan *>(d + off_pscan), M.pitems = reinterpret_cast<const uint32_t *>(d + off_pitems);
    M.pwaits = reinterpret_cast<const uint32_t *>(d + off_pwaits), M.items = reinterpret_cast<HItem *>(S.meta.d.data() + off_items);
    return RPH_OK;
}

constexpr int SEG_ROUNDS = 8;  // validation rounds of the segment synchroniser

// ---- rph_debug_jpeg_segment_log: behind the chunk's rph_jpeg_launch_segments, what it decided -- the segments' states, the `out` the
// prefix kernel read, round 0's n and out, what the validation rounds decoded, and the items written for the segmented files -- appended to the context's log (rph_internal.h)
int log_segments(rph_ctx *ctx, Slot &S, const Chunk &C, const std::vector<uint32_t> &idx, const SeqWork &W, const ChunkMeta &M)
{
    const uint32_t n = W.n_segs, first_item = W.seg_files[0].first_item;  // (the segments' items lie together behind the host's)
    std::vector<uint32_t> final_out(n), r0_n(n), r0_out(n), decodes(n), decoded_bits(n);
    std::vector<SegState> st(n);
    std::vector<HItem> items(n);
    RPH_TRY(rph_jpeg_debug_copy_segments(S.stream, S.segwork.data() + seg_states_bytes(n), n, SEG_ROUNDS, final_out.data(), r0_n.data(), r0_out.data(),
                                         decodes.data(), decoded_bits.data()));
    RPH_HIP_CHECK(hipMemcpy(st.data(), S.segwork.data(), (size_t)n * sizeof(SegState), hipMemcpyDeviceToHost));
    RPH_HIP_CHECK(hipMemcpy(items.data(), M.items + first_item, (size_t)n * sizeof(HItem), hipMemcpyDeviceToHost));
    std::vector<uint32_t> &lf = ctx->jpeg_seg_log_files, &ls = ctx->jpeg_seg_log_segs;
    for (const SegFile &F : W.seg_files) {
        const HItem *it = items.data() + (F.first_item - first_item);
        const uint32_t rec[RPH_SEG_LOG_FILE_WORDS] = {idx[C.first + F.image], F.n_segs, F.total_mcus, F.scan_bits, it[0].scan == HITEM_ALL_SCANS ? 0u : 1u,
                                                      (uint32_t)(ls.size() / RPH_SEG_LOG_SEG_WORDS), F.first_seg, M.n_luts};
        lf.insert(lf.end(), rec, rec + RPH_SEG_LOG_FILE_WORDS);
        for (uint32_t t = 0; t < F.n_segs; t++) {
            const SegState &x = st[F.first_seg + t];
            const uint32_t u = F.first_seg + t;
            const uint32_t seg[RPH_SEG_LOG_SEG_WORDS] = {x.entry, final_out[u], x.count, (uint32_t)x.dc[0], (uint32_t)x.dc[1], (uint32_t)x.dc[2], x.from, x.out_check, r0_n[u],
                                                         r0_out[u], it[t].mcu_first, it[t].mcu_count, it[t].stream_off, it[t].bit_skip, (uint32_t)it[t].dc[0],
                                                         (uint32_t)it[t].dc[1], (uint32_t)it[t].dc[2], decodes[u], decoded_bits[u]};
            ls.insert(ls.end(), seg, seg + RPH_SEG_LOG_SEG_WORDS);
        }
    }
    return RPH_OK;
}

// ---- launch: streams and descriptors up, segments, zeroed coefficients, the walks, then reconstruction + hashing sub-batch by sub-batch.
// RPH_JPEG_TRACE=1: synchronise after every phase and print where the time goes (stderr); t_host: start, prepared, descriptors written.
int launch_chunk(rph_ctx *ctx, JpegPipe &P, const Chunk &C, int16_t *d_coef, Jobs &jobs, const std::vector<uint32_t> &idx, int flavour, const Outputs &out,
                 const SeqWork &W, const ProgPlan &G, const std::vector<uint32_t> &pitems, const ChunkMeta &M, const double (&t_host)[3])
{
    Slot &S = P.slot[C.b];
    hipStream_t s = S.stream;
    const size_t m = C.m();
    const bool tr = trace_on();
    double t_up = 0, t_seg = 0, t_zero = 0, t_walk = 0, t_rec = 0;
    auto lap = [&](double &t) { if (tr) (void)hipStreamSynchronize(s), t = now_ms(); };
    ResView R(S.res.data(), S.res_images);
    zero_results(S, m, out);
    if (!W.n_items && G.files.empty()) return RPH_OK;
    RPH_HIP_CHECK(hipMemcpyAsync(S.stream_bytes.d.data(), S.stream_bytes.h.data(), C.file_bytes + 64, hipMemcpyHostToDevice, s));
    RPH_HIP_CHECK(hipMemcpyAsync(S.meta.d.data(), S.meta.h.data(), M.upload_bytes, hipMemcpyHostToDevice, s));
    lap(t_up);
    if (W.n_segs) {  // streams without markers: their segments find their entries and become walk items
        RPH_TRY(rph_jpeg_launch_segments(s, S.stream_bytes.d.data(), M.himgs, M.seg_files, (uint32_t)W.seg_files.size(), S.segwork.as<SegState>(), W.n_segs,
                                         ctx->jpeg_seg_bytes, S.segwork.data() + seg_states_bytes(W.n_segs), SEG_ROUNDS, M.luts, M.n_luts, M.items, ctx->jpeg_seg_log_on));
        if (ctx->jpeg_seg_log_on) RPH_TRY(log_segments(ctx, S, C, idx, W, M));
    }
    lap(t_seg);
    // The coefficients start from zero -- unless the walk writes whole blocks and covers every block of the chunk: sequential files of
    // one scan (interleaved, or one component), no progressive file.  (A file whose walk breaks off is reported as damaged; what its
    // remaining blocks hold is not looked at.)
    if (!(rph_jpeg_walk_writes_whole_blocks(W.n_items) && W.all_one_scan && G.files.empty())) RPH_HIP_CHECK(hipMemsetAsync(d_coef, 0, C.blocks * 128, s));
    lap(t_zero);
    if (W.n_items)
        RPH_TRY(rph_jpeg_launch_walk(s, S.stream_bytes.d.data(), M.himgs, M.items, M.order, (uint32_t)W.items.size(), W.n_items, M.luts, M.n_luts, d_coef, R.status));
    if (G.blocks) RPH_HIP_CHECK(hipMemsetAsync(S.pmask.data(), 0, G.mask_bytes(), s));
    RPH_TRY(rph_jpeg_launch_prog(s, S.stream_bytes.d.data(), M.himgs, M.pscans, (uint32_t)G.pscans.size(), M.pitems, (uint32_t)pitems.size(), M.pwaits, M.luts, M.n_luts,
                                 d_coef, S.pmask.as<unsigned long long>(), reinterpret_cast<uint32_t *>(S.pmask.as<unsigned long long>() + G.blocks), S.pcorr.as<PCorr>(),
                                 (size_t)G.corr, S.pdc.data(), (size_t)G.dc_bytes, R.status));
    lap(t_walk);
    const std::vector<size_t> &subs = M.D.sub_starts;
    for (size_t q = 0; q < subs.size(); q++)
        RPH_TRY(reconstruct_and_hash(ctx, P, C.b, S, jobs, idx, C.first, M.D, subs[q], q + 1 < subs.size() ? subs[q + 1] : m, d_coef, flavour, out, s));
    lap(t_rec);
    if (tr && W.n_segs) rph_jpeg_debug_segment_stats(s, S.segwork.data() + seg_states_bytes(W.n_segs), W.n_segs);  // (behind the timed phases)
    if (tr)
        fprintf(stderr, "[rph_jpeg] chunk of %zu files in %zu lanes (%.1f MB of entropy bytes, %.2f GB of coefficients, %zu tables, %zu sub-batches): prepare %.1f ms, "
                        "descriptors %.1f ms, upload %.1f ms, %u segments %.1f ms, zero %.1f ms, walk %.1f ms, reconstruct + hash %.1f ms\n",
                m, (size_t)W.n_items, C.file_bytes / 1e6, C.blocks * 128 / 1e9, (size_t)M.n_luts, subs.size(), t_host[1] - t_host[0], t_host[2] - t_host[1],
                t_up - t_host[2], W.n_segs, t_seg - t_up, t_zero - t_seg, t_walk - t_zero, t_rec - t_walk);
    return RPH_OK;
}

// The sequential and progressive files idx[...] with their Huffman streams walked on the device: the call plan, then chunk by chunk
// over the lanes.  Files the walk does not take, or flags, come back in `leftover` for the host decoder.
int run_device_entropy(rph_ctx *ctx, JpegPipe &P, Jobs &jobs, std::vector<uint32_t> idx, int flavour, unsigned threads, const Outputs &out,
                       std::vector<uint32_t> &leftover)
{
    DevicePlan plan;
    RPH_TRY(plan_device_call(ctx, P, jobs, idx, plan));
    InFlight lane[JPEG_LANES];
    const size_t n = idx.size();
    int k = 0;
    RPH_JPEG_STAMP("buffers ready");
    for (size_t first = 0; first < n; k++) {
        Chunk C;  // ---- pick the chunk: files while their coefficients fit plan.chunk_bytes, at least one
        for (C.first = C.last = first; C.last < n; C.last++) {
            const Job &j = jobs[idx[C.last]];
            if (C.last > first && (C.blocks + j.frame.total_blocks) * 128 > plan.chunk_bytes) break;
            C.blocks += j.frame.total_blocks, C.file_bytes += stream_cap(j);
        }
        first = C.last;
        if (C.blocks * 128 > plan.region) {  // one image larger than a whole region: the host path takes it
            leftover.push_back(idx[C.first]);
            k--;
            continue;
        }
        C.b = k % plan.lanes, C.k = k;
        // the lane is free again once its previous chunk (`lanes` chunks back) has delivered its results
        RPH_TRY(lane[C.b].finish(C.b, P.slot[C.b], true, jobs, idx, out, &leftover));
        Slot &S = P.slot[C.b];
        RPH_TRY(S.reserve_res(C.m(), out.pixel_hash != nullptr));
        RPH_TRY(S.stream_bytes.reserve(C.file_bytes + 64, S.stream));
        double t_host[3] = {now_ms(), 0, 0};
        TableStore store;
        std::vector<HImage> himgs;
        prepare_chunk(jobs, idx, C, threads, S, store, himgs);
        t_host[1] = now_ms();
        RPH_JPEG_STAMP("lane %d: chunk %d prepared (%zu files)", C.b, C.k, C.m());
        const SeqWork W = list_sequential(ctx, jobs, idx, C, leftover);
        ProgPlan G;
        for (size_t i = C.first; i < C.last; i++)
            if (jobs[idx[i]].status == RPH_OK && jobs[idx[i]].frame.progressive) G.add((uint32_t)(i - C.first), jobs[idx[i]], himgs[i - C.first]);
        RPH_JPEG_STAMP("lane %d: chunk %d items listed", C.b, C.k);
        const std::vector<uint32_t> pitems = order_waves(G, himgs);
        RPH_JPEG_STAMP("lane %d: chunk %d waves ordered", C.b, C.k);
        ChunkMeta M;
        RPH_TRY(write_meta(P, jobs, idx, C, flavour, out.rgb_wanted(), store, himgs, W, G, pitems, M));
        RPH_JPEG_STAMP("lane %d: chunk %d descriptors written", C.b, C.k);
        t_host[2] = now_ms();
        int16_t *d_coef = P.coef.as<int16_t>() + (size_t)C.b * (plan.region / 2);  // (int16 elements: region bytes per lane)
        RPH_TRY(launch_chunk(ctx, P, C, d_coef, jobs, idx, flavour, out, W, G, pitems, M, t_host));
        RPH_HIP_CHECK(hipEventRecord(S.done, S.stream));
        RPH_JPEG_STAMP("lane %d: chunk %d enqueued", C.b, C.k);
        lane[C.b] = InFlight{true, C.first, C.last};
    }
    for (int t = 0; t < plan.lanes; t++) {  // oldest first
        const int b = (k + t) % plan.lanes;
        RPH_TRY(lane[b].finish(b, P.slot[b], true, jobs, idx, out, &leftover));
    }
    // files handed to the host decoder start over there
    for (uint32_t g : leftover) jobs[g].status = RPH_OK;
    return RPH_OK;
}

int run_batch(rph_ctx *ctx, const uint8_t *const *data, const size_t *len, uint32_t n, int flavour, uint32_t n_threads, Outputs out, Jobs *prepared = nullptr)
{
    if (flavour != RPH_JPEG_ZUNE && flavour != RPH_JPEG_LIBJPEG) {
        rph_set_error("rph_jpeg: unknown flavour %d", flavour);
        return RPH_ERR_INVALID_ARG;
    }
    std::lock_guard<std::mutex> lock(ctx->jpeg_mu);
    RPH_HIP_CHECK(hipSetDevice(ctx->device));
    if (!ctx->jpeg) ctx->jpeg = new JpegPipe();
    JpegPipe &P = *static_cast<JpegPipe *>(ctx->jpeg);
    unsigned threads = n_threads ? n_threads : rph_host_threads();
    threads = std::min(threads, 256u);

    g_trace_t0 = now_ms();
    ctx->jpeg_seg_log_files.clear(), ctx->jpeg_seg_log_segs.clear();  // (rph_debug_jpeg_segment_log: the log holds one call)
    RPH_JPEG_STAMP("call: %u files", n);
    Jobs &jobs = prepared ? *prepared : P.jobs_cache;
    if (!prepared && jobs.size() < n) jobs.resize(n);  // (grown by this thread: first-touching the storage from the parsing threads is 5x slower, page faults under contention)
    if (!prepared)
        parallel_for(0, n, n >= 1024 ? threads : 1, [&](size_t i) {
            Job &j = jobs[i];
            j.data = data[i];
            j.len = len[i];
            j.pre = nullptr;
            j.status = (j.data && j.len) ? rphj::parse_frame(j.data, j.len, j.frame) : RPH_ERR_INVALID_ARG;
            if (j.status == RPH_OK && (j.frame.total_blocks * 128 > MAX_IMAGE_COEF_BYTES || !frame_is_plausible(j.frame, j.len))) j.status = RPH_ERR_UNSUPPORTED;
        });
    RPH_JPEG_STAMP("frames parsed");
    // Which files walk their Huffman streams on the device?  In automatic mode, those for which it is estimated to pay:
    //  * sequential files when the call has lanes to fill -- one per file, or one per restart interval where the frame header announces
    //    them (a few dozen photos with restart markers are thousands of short streams); a long stream without markers is cut into
    //    segments, whose passes cost ~10 ms of launches before they scale: counted as a lane per 8 KB, so that ~50 photos qualify (16 host
    //    threads decode 130 MB/s each);
    //  * progressive files, one lane each whatever their size, when the host threads (~41 MB/s each) would need longer for all of them
    //    than the device needs for the longest (~0.6 us per byte of the file: its scans follow one another block by block).
    std::vector<uint32_t> host_idx, dev_idx;
    const bool may_device = ctx->jpeg_entropy != 0 && out.want_hash && !prepared;
    uint64_t lanes = 0, prog_bytes = 0, prog_longest = 0;
    for (uint32_t i = 0; i < n; i++) {
        const Job &j = jobs[i];
        if (j.status != RPH_OK || !may_device) continue;
        const rphj::Frame &f = j.frame;
        if (f.progressive) {
            prog_bytes += j.len;
            prog_longest = std::max<uint64_t>(prog_longest, j.len);
        } else if (f.restart_interval) {
            lanes += ((uint64_t)f.mcus_x * f.mcus_y + f.restart_interval - 1) / f.restart_interval;
        } else if (ctx->jpeg_seg_bytes && j.len >= ctx->jpeg_seg_min_bytes) {
            lanes += std::max<uint64_t>(1, j.len / 8192);
        } else {
            lanes += 1;
        }
    }
    const bool seq_on_device = may_device && (ctx->jpeg_entropy == 1 || lanes >= DEVICE_ENTROPY_MIN_FILES);
    const bool prog_on_device = may_device && ctx->jpeg_progressive_on_device &&
                                (ctx->jpeg_entropy == 1 || (double)prog_bytes / ((double)threads * 41e6) > 0.6e-6 * (double)prog_longest);
    for (uint32_t i = 0; i < n; i++) {
        const Job &j = jobs[i];
        if (j.status == RPH_OK && (j.frame.progressive ? prog_on_device : seq_on_device))
            dev_idx.push_back(i);
        else
            host_idx.push_back(i);
    }
    if (!dev_idx.empty()) {
        std::vector<uint32_t> leftover;
        RPH_TRY(run_device_entropy(ctx, P, jobs, dev_idx, flavour, threads, out, leftover));
        host_idx.insert(host_idx.end(), leftover.begin(), leftover.end());
        std::sort(host_idx.begin(), host_idx.end());
    }
    if (!host_idx.empty()) RPH_TRY(run_host_entropy(ctx, P, jobs, host_idx, flavour, threads, out));
    RPH_JPEG_STAMP("all chunks done");
    int worst = RPH_OK;
    for (uint32_t i = 0; i < n; i++) {
        if (out.status) out.status[i] = jobs[i].status;
        if (jobs[i].status != RPH_OK) worst = jobs[i].status;
    }
    if (n == 1 && worst != RPH_OK) rph_set_error("rph_jpeg: not decodable (status %d)", worst);
    return n == 1 ? worst : RPH_OK;  // a batch reports per image (status / valid); one image reports itself
}

}  // namespace

void rph_jpeg_forget_threads(rph_ctx *ctx)  // rph_shutdown: no caller is inside the library any more
{
    for (void *p : ctx->jpeg_thread_buffers) (void)hipHostFree(p);
    ctx->jpeg_thread_buffers.clear();
}

void rph_jpeg_forget(rph_ctx *ctx)
{
    delete static_cast<JpegPipe *>(ctx->jpeg);
    ctx->jpeg = nullptr;
}

extern "C" {

int rph_jpeg_info(const uint8_t *data, size_t len, uint32_t *w, uint32_t *h, uint32_t *channels)
{
    return rph_guarded("rph_jpeg_info", [&]() -> int {
        if (!data || !w || !h || !channels) {
            rph_set_error("rph_jpeg_info: null argument");
            return RPH_ERR_INVALID_ARG;
        }
        rphj::Frame f;
        const int rc = rphj::parse_frame(data, len, f);
        if (rc != RPH_OK) {
            rph_set_error("rph_jpeg_info: %s", rc == RPH_ERR_UNSUPPORTED ? "unsupported kind of JPEG" : "not a JPEG stream");
            return rc;
        }
        *w = f.w;
        *h = f.h;
        *channels = (uint32_t)f.ncomp;
        return RPH_OK;
    });
}

int rph_jpeg_coefficients(const uint8_t *data, size_t len, uint32_t *geometry, uint16_t *qt, int16_t *coef, size_t cap_blocks, uint64_t *total_blocks)
{
    return rph_guarded("rph_jpeg_coefficients", [&]() -> int {
        if (!data || !geometry || !qt || !total_blocks) {
            rph_set_error("rph_jpeg_coefficients: null argument");
            return RPH_ERR_INVALID_ARG;
        }
        rphj::Frame f;
        int rc = rphj::parse_frame(data, len, f);
        if (rc != RPH_OK) return rc;
        *total_blocks = f.total_blocks;
        std::vector<int16_t> tmp;
        int16_t *dst = coef;
        if (!coef) {
            tmp.resize((size_t)f.total_blocks * 64);
            dst = tmp.data();
        } else if (cap_blocks < f.total_blocks) {
            rph_set_error("rph_jpeg_coefficients: %llu blocks, capacity %zu", (unsigned long long)f.total_blocks, cap_blocks);
            return RPH_ERR_CAPACITY;
        }
        rc = rphj::decode_coefficients(data, len, f, dst);
        if (rc != RPH_OK) {
            rph_set_error("rph_jpeg_coefficients: entropy decoding failed (status %d)", rc);
            return rc;
        }
        for (int c = 0; c < f.ncomp; c++) {
            const rphj::Comp &k = f.comp[c];
            uint32_t *g = geometry + 8 * c;
            g[0] = k.blocks_w, g[1] = k.blocks_h, g[2] = k.H, g[3] = k.V, g[4] = k.tq, g[5] = k.samp_w, g[6] = k.samp_h, g[7] = (uint32_t)k.first_block;
        }
        for (int t = 0; t < 4; t++) f.qt_present[t] ? (void)memcpy(qt + 64 * t, f.qt[t], 128) : (void)memset(qt + 64 * t, 0, 128);
        return RPH_OK;
    });
}

int rph_jpeg_set_segments(rph_ctx *ctx, uint32_t min_stream_bytes, uint32_t segment_bytes)
{
    if (!ctx || (segment_bytes && (segment_bytes < 64 || segment_bytes > 65536 || (segment_bytes & 3)))) {
        rph_set_error("rph_jpeg_set_segments: invalid argument");
        return RPH_ERR_INVALID_ARG;
    }
    std::lock_guard<std::mutex> lock(ctx->jpeg_mu);
    ctx->jpeg_seg_min_bytes = min_stream_bytes;
    ctx->jpeg_seg_bytes = segment_bytes;
    return RPH_OK;
}

int rph_debug_jpeg_segment_log(rph_ctx *ctx, int on)
{
    if (!ctx) return RPH_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lock(ctx->jpeg_mu);
    ctx->jpeg_seg_log_on = on != 0;
    return RPH_OK;
}

int rph_debug_jpeg_segments(rph_ctx *ctx, uint32_t *files_out, uint32_t file_cap, uint32_t *n_files_out, uint32_t *segs_out, uint32_t seg_cap, uint32_t *n_segs_out)
{
    if (!ctx) return RPH_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lock(ctx->jpeg_mu);
    const std::vector<uint32_t> &lf = ctx->jpeg_seg_log_files, &ls = ctx->jpeg_seg_log_segs;
    if (files_out) memcpy(files_out, lf.data(), std::min<size_t>((size_t)file_cap * RPH_SEG_LOG_FILE_WORDS, lf.size()) * 4);
    if (segs_out) memcpy(segs_out, ls.data(), std::min<size_t>((size_t)seg_cap * RPH_SEG_LOG_SEG_WORDS, ls.size()) * 4);
    if (n_files_out) *n_files_out = (uint32_t)(lf.size() / RPH_SEG_LOG_FILE_WORDS);
    if (n_segs_out) *n_segs_out = (uint32_t)(ls.size() / RPH_SEG_LOG_SEG_WORDS);
    return RPH_OK;
}

int rph_jpeg_release(rph_ctx *ctx)
{
    if (!ctx) {
        rph_set_error("rph_jpeg_release: null argument");
        return RPH_ERR_INVALID_ARG;
    }
    std::lock_guard<std::mutex> lock(ctx->jpeg_mu);
    RPH_HIP_CHECK(hipSetDevice(ctx->device));
    rph_jpeg_forget(ctx);
    return RPH_OK;
}

int rph_jpeg_set_entropy(rph_ctx *ctx, int where)
{
    if (!ctx || where < 0 || where > 3) {
        rph_set_error("rph_jpeg_set_entropy: invalid argument");
        return RPH_ERR_INVALID_ARG;
    }
    std::lock_guard<std::mutex> lock(ctx->jpeg_mu);
    ctx->jpeg_entropy = where == 3 ? 1 : where;
    ctx->jpeg_progressive_on_device = where == 3 ? 0 : 1;
    return RPH_OK;
}

int rph_jpeg_decode(rph_ctx *ctx, const uint8_t *data, size_t len, int flavour, uint8_t *pixels_out)
{
    return rph_guarded("rph_jpeg_decode", [&]() -> int {
        if (!ctx || !data || !pixels_out) {
            rph_set_error("rph_jpeg_decode: null argument");
            return RPH_ERR_INVALID_ARG;
        }
        Outputs o;
        o.pixels = pixels_out;
        o.want_hash = false;
        return run_batch(ctx, &data, &len, 1, flavour, 1, o);
    });
}

// One file per call from many threads (the reference's scan loop: load_image_fast + generate_pdq_features on every rayon worker,
// scanner.rs:1202, :1410).  Callers that arrive while a batch is on its way wait and leave together as the next batch, which one of
// them (the leader) runs through the reconstruction + hashing stages of rph_jpeg_pdq_hash_batch.  Every caller undoes the entropy
// coding of its own file first, on its own core, into a pinned buffer of its own that the copy engine reads directly.
namespace {
struct OneRequest {
    const uint8_t *data;
    size_t len;
    int flavour;
    rphj::Frame frame;
    const int16_t *coef;  // the caller's pinned buffer, decoded by the caller
    uint8_t hash[32];
    float quality, coeffs[256];
    uint8_t valid;
    int32_t status;
    bool want_coeffs, done;
};
// One pinned coefficient buffer per calling thread (a scan worker decodes thousands of files into it).  It belongs to the context:
// rph_shutdown frees it (a thread-local destructor would call into the HIP runtime at thread or process exit, possibly after the
// runtime is gone); `serial` tells a later context at the same address from the one that owned the buffer.
struct ThreadPinned {
    int16_t *p = nullptr;
    size_t cap = 0;
    rph_ctx *owner = nullptr;
    uint64_t serial = 0;
};
thread_local ThreadPinned tls_coef;
}  // namespace

int rph_jpeg_pdq_hash_one(rph_ctx *ctx, const uint8_t *data, size_t len, int flavour, uint8_t *hash32_out, float *quality_out, float *coeffs_out, uint8_t *valid_out)
{
    return rph_guarded("rph_jpeg_pdq_hash_one", [&]() -> int {
        if (!ctx || !data || !hash32_out || (flavour != RPH_JPEG_ZUNE && flavour != RPH_JPEG_LIBJPEG)) {
            rph_set_error("rph_jpeg_pdq_hash_one: invalid argument");
            return RPH_ERR_INVALID_ARG;
        }
        // ---- this thread: frame header and entropy decoding into its own pinned buffer (all callers do this side by side)
        OneRequest me;
        me.data = data, me.len = len, me.flavour = flavour, me.want_coeffs = coeffs_out != nullptr, me.done = false, me.valid = 0, me.quality = 0.f, me.coef = nullptr;
        me.status = rphj::parse_frame(data, len, me.frame);
        if (me.status == RPH_OK && (me.frame.total_blocks * 128 > MAX_IMAGE_COEF_BYTES || !frame_is_plausible(me.frame, len))) me.status = RPH_ERR_UNSUPPORTED;
        if (me.status == RPH_OK) {
            const size_t need = (size_t)me.frame.total_blocks * 128;
            if (tls_coef.owner != ctx || tls_coef.serial != ctx->serial) tls_coef = ThreadPinned();  // another (or an earlier) context's buffer is not ours to use
            if (tls_coef.cap < need) {
                RPH_HIP_CHECK(hipSetDevice(ctx->device));
                std::lock_guard<std::mutex> reg(ctx->jpeg_qmu);
                if (tls_coef.p) {
                    auto &v = ctx->jpeg_thread_buffers;
                    v.erase(std::remove(v.begin(), v.end(), (void *)tls_coef.p), v.end());
                    (void)hipHostFree(tls_coef.p);
                }
                tls_coef = ThreadPinned();
                const size_t cap = align_up(need + need / 2, 1 << 20);
                RPH_HIP_CHECK(hipHostMalloc((void **)&tls_coef.p, cap));
                tls_coef.cap = cap;
                tls_coef.owner = ctx;
                tls_coef.serial = ctx->serial;
                ctx->jpeg_thread_buffers.push_back(tls_coef.p);
            }
            me.status = rphj::decode_coefficients(data, len, me.frame, tls_coef.p);
            me.coef = tls_coef.p;
        }
        if (me.status != RPH_OK) {
            memset(hash32_out, 0, 32);
            if (quality_out) *quality_out = 0.f;
            if (coeffs_out) memset(coeffs_out, 0, 1024);
            if (valid_out) *valid_out = 0;
            rph_set_error("rph_jpeg_pdq_hash_one: not decodable here (status %d)", me.status);
            return me.status;
        }
        // ---- the device part: with everyone else who is waiting, as one batch, run by one of them
        std::unique_lock<std::mutex> lk(ctx->jpeg_qmu);
        ctx->jpeg_waiting.push_back(&me);
        while (!me.done) {
            if (ctx->jpeg_leader) {
                ctx->jpeg_qcv.wait(lk);
                continue;
            }
            ctx->jpeg_leader = true;
            std::vector<void *> batch;
            batch.swap(ctx->jpeg_waiting);
            lk.unlock();
            for (int fl = 0; fl < 2; fl++) {  // (callers may ask for different arithmetic flavours: one pass each)
                std::vector<OneRequest *> reqs;
                for (void *p : batch)
                    if (static_cast<OneRequest *>(p)->flavour == fl) reqs.push_back(static_cast<OneRequest *>(p));
                if (reqs.empty()) continue;
                const uint32_t n = (uint32_t)reqs.size();
                int rc = RPH_OK;
                std::vector<uint8_t> hashes((size_t)n * 32), valid(n);
                std::vector<float> quality(n), coeffs;
                std::vector<int32_t> status(n);
                try {
                    bool any_coeffs = false;
                    Jobs jobs(n);
                    for (uint32_t i = 0; i < n; i++) {
                        jobs[i].data = reqs[i]->data, jobs[i].len = reqs[i]->len, jobs[i].frame = reqs[i]->frame, jobs[i].pre = reqs[i]->coef;
                        any_coeffs |= reqs[i]->want_coeffs;
                    }
                    coeffs.resize(any_coeffs ? (size_t)n * 256 : 0);
                    Outputs o;
                    o.hash = hashes.data(), o.quality = quality.data(), o.coeffs = any_coeffs ? coeffs.data() : nullptr, o.valid = valid.data(), o.status = status.data();
                    rc = run_batch(ctx, nullptr, nullptr, n, fl, 1, o, &jobs);
                } catch (...) {
                    rc = RPH_ERR_OOM;
                }
                for (uint32_t i = 0; i < n; i++) {
                    OneRequest &r = *reqs[i];
                    r.status = (rc != RPH_OK && status[i] == RPH_OK) ? rc : status[i];  // a failure of the call itself fails all of its files
                    memcpy(r.hash, &hashes[(size_t)i * 32], 32);
                    r.quality = quality[i];
                    r.valid = r.status == RPH_OK ? valid[i] : 0;
                    if (r.want_coeffs && !coeffs.empty()) memcpy(r.coeffs, &coeffs[(size_t)i * 256], 1024);
                }
            }
            lk.lock();
            for (void *p : batch) static_cast<OneRequest *>(p)->done = true;
            ctx->jpeg_leader = false;
            ctx->jpeg_qcv.notify_all();
        }
        lk.unlock();
        memcpy(hash32_out, me.hash, 32);
        if (quality_out) *quality_out = me.quality;
        if (coeffs_out) memcpy(coeffs_out, me.coeffs, 1024);
        if (valid_out) *valid_out = me.valid;
        if (me.status != RPH_OK) rph_set_error("rph_jpeg_pdq_hash_one: failed (status %d)", me.status);
        return me.status;
    });
}

int rph_jpeg_pdq_hash_batch(rph_ctx *ctx, const uint8_t *const *data, const size_t *len, uint32_t n, int flavour, uint32_t n_threads, uint8_t *hash32_out,
                            float *quality_out, float *coeffs_out, uint8_t *dihedral_out, uint8_t *valid_out, int32_t *status_out)
{
    return rph_guarded("rph_jpeg_pdq_hash_batch", [&]() -> int {
        if (!ctx || (n && (!data || !len)) || !hash32_out) {
            rph_set_error("rph_jpeg_pdq_hash_batch: null argument");
            return RPH_ERR_INVALID_ARG;
        }
        if (n == 0) return RPH_OK;
        Outputs o;
        o.hash = hash32_out;
        o.quality = quality_out;
        o.coeffs = coeffs_out;
        o.dihedral = dihedral_out;
        o.valid = valid_out;
        o.status = status_out;
        return run_batch(ctx, data, len, n, flavour, n_threads, o);
    });
}

int rph_jpeg_pdq_pixel_hash_batch(rph_ctx *ctx, const uint8_t *const *data, const size_t *len, uint32_t n, int flavour, uint32_t n_threads,
                                  uint8_t *hash32_out, float *quality_out, float *coeffs_out, uint8_t *dihedral_out, uint8_t *valid_out,
                                  int32_t *status_out, uint8_t *pixel_hash32_out)
{
    return rph_guarded("rph_jpeg_pdq_pixel_hash_batch", [&]() -> int {
        if (!ctx || (n && (!data || !len)) || !hash32_out || !pixel_hash32_out) {
            rph_set_error("rph_jpeg_pdq_pixel_hash_batch: null argument");
            return RPH_ERR_INVALID_ARG;
        }
        if (n == 0) return RPH_OK;
        Outputs o;
        o.hash = hash32_out;
        o.quality = quality_out;
        o.coeffs = coeffs_out;
        o.dihedral = dihedral_out;
        o.valid = valid_out;
        o.status = status_out;
        o.pixel_hash = pixel_hash32_out;
        return run_batch(ctx, data, len, n, flavour, n_threads, o);
    });
}

}  // extern "C"
