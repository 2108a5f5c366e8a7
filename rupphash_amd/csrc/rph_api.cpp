// rph_api.cpp -- extern "C" surface of librupphash_hip.so (see include/rupphash.h).
// Host-pointer entry points stage through device memory and call the *_dev twins; there is no
// CPU implementation of any kernel behind this API.
#include <sched.h>

#include <algorithm>
#include <atomic>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

#include "pixel_rules.h"
#include "rph_internal.h"

static thread_local char g_err[512] = "";

void rph_set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
}

namespace {
hipStream_t pick(rph_ctx *ctx, void *stream) { return stream ? (hipStream_t)stream : ctx->stream; }
}  // namespace

// ---- what the Hamming and grouping entry points share (rph_sweep: rph_internal.h) ----
namespace {
// the two forms of a request over 256-bit hashes; where its edges go is set with `into`
rph_sweep square_sweep(const void *rows, uint32_t n_variants, const void *hashes, const void *low_conf, const void *has_features, uint64_t n,
                       uint32_t threshold, uint32_t part, uint32_t nparts)
{
    rph_sweep q;
    q.rows = rows, q.n_variants = n_variants, q.cols = hashes, q.n = n;
    q.low_conf = (const uint8_t *)low_conf, q.has_features = (const uint8_t *)has_features;
    q.threshold = threshold, q.part = part, q.nparts = nparts;
    return q;
}
rph_sweep cross_sweep(const void *rows, uint32_t n_variants, const void *low_conf, const void *has_features, uint64_t n, const void *hashes_b,
                      const void *low_conf_b, uint64_t n_b, uint32_t threshold, uint32_t part, uint32_t nparts)
{
    rph_sweep q = square_sweep(rows, n_variants, hashes_b, low_conf, has_features, n, threshold, part, nparts);
    q.cross = true, q.low_conf_cols = (const uint8_t *)low_conf_b, q.n_cols = n_b;
    return q;
}
rph_sweep into(rph_sweep q, void *edges, uint64_t cap, void *count = nullptr)
{
    q.edges = (rph_edge *)edges, q.cap = cap, q.count = (unsigned long long *)count;
    return q;
}

// a _dev entry point: the request as it is, on the caller's stream
int sweep_dev(const char *who, rph_ctx *ctx, const rph_sweep &q, void *stream)
{
    const uint64_t n_cols = q.cross ? q.n_cols : q.n;
    if (!ctx || (!q.rows && q.n) || (!q.cols && n_cols) || !q.count || (!q.edges && q.cap)) {
        rph_set_error("%s: null argument", who);
        return RPH_ERR_INVALID_ARG;
    }
    RPH_HIP_CHECK(hipSetDevice(ctx->device));
    return rph_launch_hamming_sweep(ctx, q, pick(ctx, stream), ctx->hamming_kernel);
}

// The edge list of a sweep on the device: the buffer and the 8-byte cursor that the kernels append through.  A sweep that finds more
// than `cap` edges writes the first `cap` and counts them all.
struct EdgeSink {
    DevBuf d_e, d_cnt;
    uint64_t cap = 0;
    // a buffer of `capacity` edges and the cursor zeroed on `s`; `q` reports there
    int open(uint64_t capacity, hipStream_t s, rph_sweep &q)
    {
        cap = capacity;
        RPH_TRY(d_e.alloc(cap * sizeof(rph_edge)));
        if (!d_cnt.data()) RPH_TRY(d_cnt.alloc(8));
        RPH_HIP_CHECK(hipMemsetAsync(d_cnt.data(), 0, 8, s));
        q = into(q, d_e.data(), cap, d_cnt.data());
        return RPH_OK;
    }
    // the cursor as it stands behind the work queued on `s` so far (asynchronous: *found is valid once `s` has been synchronised)
    int read(unsigned long long *found, hipStream_t s) const
    {
        RPH_HIP_CHECK(hipMemcpyAsync(found, d_cnt.data(), 8, hipMemcpyDeviceToHost, s));
        return RPH_OK;
    }
    // behind that synchronisation: the first min(found, cap) edges to `out`; more found than fit is RPH_ERR_CAPACITY, with the count
    int take(const char *who, unsigned long long found, rph_edge *out) const
    {
        const uint64_t n_take = std::min<uint64_t>(found, cap);
        if (n_take) RPH_HIP_CHECK(hipMemcpy(out, d_e.data(), n_take * sizeof(rph_edge), hipMemcpyDeviceToHost));
        if (found > cap) {
            rph_set_error("%s: %llu edges found, capacity %llu", who, found, (unsigned long long)cap);
            return RPH_ERR_CAPACITY;
        }
        return RPH_OK;
    }
};

// The arrays of a request given in host pointers, on the device.  Rows that the request names are an array of their own there, whatever
// they alias on the host; a square request without rows (rph_hamming_all_pairs, the 64-bit form, rph_find_groups*) sweeps its hashes
// against themselves, and only then rows and columns are one device array, as a caller of rph_hamming_all_pairs_dev passes them.
struct SweepOperands {
    DevBuf rows, cols, low_conf, has_features, low_conf_cols;
    int upload(const rph_sweep &host, hipStream_t s, rph_sweep &dev)
    {
        auto up = [s](DevBuf &b, const void *src, size_t bytes) -> int {
            RPH_TRY(b.alloc(bytes));
            RPH_HIP_CHECK(hipMemcpyAsync(b.data(), src, bytes, hipMemcpyHostToDevice, s));
            return RPH_OK;
        };
        const size_t width = host.bits64 ? 8 : 32;
        dev = host;
        RPH_TRY(up(cols, host.cols, (host.cross ? host.n_cols : host.n) * width));
        dev.rows = dev.cols = cols.data();
        if (host.rows) {
            RPH_TRY(up(rows, host.rows, host.n * width * host.n_variants));
            dev.rows = rows.data();
        }
        if (host.low_conf) {
            RPH_TRY(up(low_conf, host.low_conf, host.n));
            dev.low_conf = low_conf.data();
        }
        if (host.has_features) {
            RPH_TRY(up(has_features, host.has_features, host.n));
            dev.has_features = has_features.data();
        }
        if (host.low_conf_cols) {
            RPH_TRY(up(low_conf_cols, host.low_conf_cols, host.n_cols));
            dev.low_conf_cols = low_conf_cols.data();
        }
        return RPH_OK;
    }
};

// A host entry point: the request in host pointers (a square one may leave `rows` null: SweepOperands), `q.edges` the caller's array of
// `q.cap` edges.  The square forms answer a set of
// fewer than two files before they look at part / nparts / n_variants; the cross forms check those before they look at the sizes.
int sweep_host(const char *who, rph_ctx *ctx, const rph_sweep &q, uint64_t *n_edges_out)
{
    const uint64_t n_cols = q.cross ? q.n_cols : q.n;
    if (!ctx || (q.cross && !q.rows && q.n) || (!q.cols && n_cols) || !n_edges_out || (!q.edges && q.cap)) {
        rph_set_error("%s: null argument", who);
        return RPH_ERR_INVALID_ARG;
    }
    *n_edges_out = 0;
    if (!q.cross && q.n < 2) return RPH_OK;
    RPH_TRY(rph_hamming_sweep_check(q));
    if (q.n == 0 || n_cols == 0) return RPH_OK;
    RPH_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    SweepOperands ops;
    EdgeSink sink;
    rph_sweep d;
    RPH_TRY(ops.upload(q, s, d));
    RPH_TRY(sink.open(q.cap, s, d));
    RPH_TRY(rph_launch_hamming_sweep(ctx, d, s, ctx->hamming_kernel));
    unsigned long long found = 0;
    RPH_TRY(sink.read(&found, s));
    RPH_HIP_CHECK(hipStreamSynchronize(s));
    *n_edges_out = found;
    return sink.take(who, found, q.edges);
}

// A sweep whose edge count is not known in advance: into a buffer of `cap` edges, and while it finds more than fit, again into one
// that `growth` sizes from what it counted.  launch(sink, cap) opens the sink for its request and queues its sweeps on `s`, all of
// them appending through the one cursor.
template <class F>
int sweep_growing_dev(const char *who, uint64_t cap, const rph_edge_growth &growth, hipStream_t s, EdgeSink &sink, unsigned long long *found_out, F &&launch)
{
    unsigned long long found = 0;
    for (int attempt = 0; attempt < growth.attempts; attempt++) {
        RPH_TRY(launch(sink, cap));
        RPH_TRY(sink.read(&found, s));
        RPH_HIP_CHECK(hipStreamSynchronize(s));
        if (found <= cap) {
            *found_out = found;
            return RPH_OK;
        }
        cap = growth.next_cap(found);
    }
    rph_set_error("%s: edge list kept growing (%llu)", who, found);
    return RPH_ERR_CAPACITY;
}
// ... and the edges brought to the host; sweep_growing_dev leaves them in `sink` on the device (rph_group_files_pdq_tree)
template <class F>
int sweep_growing(const char *who, uint64_t cap, const rph_edge_growth &growth, hipStream_t s, std::vector<rph_edge> &edges, F &&launch)
{
    EdgeSink sink;
    unsigned long long found = 0;
    RPH_TRY(sweep_growing_dev(who, cap, growth, s, sink, &found, launch));
    edges.resize(found);
    return sink.take(who, found, edges.data());
}

// One set of files of the grouping calls on the device: hashes, the variants its files own as rows (8 per file from the coefficients,
// which cross PCIe in 256 MiB pieces through a fixed staging buffer: scanner.rs:1621-1623; else the hash itself), has_features and
// low-confidence flags.  Everything between the caller's arrays and the edge list stays on the device.
struct GroupSide {
    DevBuf d_h, d_var, d_lc, d_hf, d_stage;
    std::vector<uint8_t> low_conf_host;
    uint64_t n = 0;
    uint32_t n_variants = 1;
    bool use_hf = false;
    const uint8_t *rows() const { return n_variants == 8 ? d_var.data() : d_h.data(); }
    const uint8_t *has_features() const { return use_hf ? d_hf.data() : nullptr; }
    // this side's rows against its own hashes (pairs i < j), or against the hashes of `other` (every pair)
    rph_sweep sweep(uint32_t similarity, const GroupSide *other = nullptr) const
    {
        return other ? cross_sweep(rows(), n_variants, d_lc.data(), has_features(), n, other->d_h.data(), other->d_lc.data(), other->n, similarity, 0, 1)
                     : square_sweep(rows(), n_variants, d_h.data(), d_lc.data(), has_features(), n, similarity, 0, 1);
    }
    int upload(const uint8_t *hashes32, const float *coeffs, const uint8_t *hf, const int32_t *quality, uint64_t count, bool want_rows, hipStream_t s)
    {
        n = count;
        if (n == 0) return RPH_OK;
        RPH_TRY(d_h.alloc(n * 32));
        RPH_HIP_CHECK(hipMemcpyAsync(d_h.data(), hashes32, n * 32, hipMemcpyHostToDevice, s));
        if (quality) {
            low_conf_host.resize(n);
            for (uint64_t i = 0; i < n; i++) low_conf_host[i] = (uint8_t)rph_is_low_pdq_quality(quality[i]);
            RPH_TRY(d_lc.alloc(n));
            RPH_HIP_CHECK(hipMemcpyAsync(d_lc.data(), low_conf_host.data(), n, hipMemcpyHostToDevice, s));
        }
        if (!coeffs || !want_rows) return RPH_OK;
        n_variants = 8;
        use_hf = hf != nullptr;
        if (use_hf) {
            RPH_TRY(d_hf.alloc(n));
            RPH_HIP_CHECK(hipMemcpyAsync(d_hf.data(), hf, n, hipMemcpyHostToDevice, s));
        }
        RPH_TRY(d_var.alloc(n * 256));
        const uint64_t step = 1u << 18;  // 256 MiB of coefficients per piece
        RPH_TRY(d_stage.alloc(std::min<uint64_t>(step, n) * 1024));
        for (uint64_t first = 0; first < n; first += step) {
            const uint32_t m = (uint32_t)std::min<uint64_t>(step, n - first);
            RPH_HIP_CHECK(hipMemcpyAsync(d_stage.data(), coeffs + first * 256, (size_t)m * 1024, hipMemcpyHostToDevice, s));
            RPH_TRY(rph_launch_pdq_from_coeffs((const float *)d_stage.data(), m, nullptr, d_var.as<uint8_t>() + first * 256, s));
        }
        if (use_hf) RPH_TRY(rph_launch_featureless_variants(d_h.as<uint8_t>(), d_hf.as<uint8_t>(), n, d_var.as<uint8_t>(), s));
        return RPH_OK;
    }
};
}  // namespace

// 1/3/4 channels, rows do not overlap, images do not overlap (a single image needs no image_stride)
static bool pdq_geometry_ok(uint32_t n, uint32_t w, uint32_t h, uint32_t channels, size_t row_stride, size_t image_stride)
{
    if (channels != 1 && channels != 3 && channels != 4) return false;
    if (row_stride < (size_t)w * channels) return false;
    return n <= 1 || image_stride >= row_stride * (h ? h - 1 : 0) + (size_t)w * channels;
}

// ---- staging pipe of rph_pdq_hash_batch ----
namespace {
constexpr size_t kPipeChunkBytes = (size_t)64 << 20;
struct PipeSet {  // one staging set: pinned host + device buffers of one chunk and the stream they are used on
    hipStream_t stream = nullptr;
    PinnedBuf h_px, h_hash, h_q, h_c, h_d, h_v, h_ph;
    DevBuf d_px, d_hash, d_q, d_c, d_d, d_v, d_ph;  // (ph: pixel hashes, rph_image_hash_ragged only)
};
struct HostPipe {
    PipeSet set[2];
    ~HostPipe()  // the streams first: their work may still use the buffers
    {
        for (PipeSet &S : set)
            if (S.stream) {
                (void)hipStreamSynchronize(S.stream);
                (void)hipStreamDestroy(S.stream);
            }
    }
};

int pipe_of(rph_ctx *ctx, size_t px_bytes, uint32_t images, HostPipe **out, bool pixel_hashes = false)
{
    if (!ctx->pipe) ctx->pipe = new HostPipe();
    HostPipe &P = *static_cast<HostPipe *>(ctx->pipe);
    for (PipeSet &S : P.set) {
        if (!S.stream) RPH_HIP_CHECK(hipStreamCreateWithFlags(&S.stream, hipStreamNonBlocking));
        auto twin = [&](PinnedBuf &h, DevBuf &d, size_t bytes) -> int {
            RPH_TRY(h.reserve(bytes, S.stream));
            return d.reserve(bytes, S.stream);
        };
        RPH_TRY(twin(S.h_px, S.d_px, px_bytes));
        RPH_TRY(twin(S.h_hash, S.d_hash, (size_t)images * 32));
        RPH_TRY(twin(S.h_q, S.d_q, (size_t)images * 4));
        RPH_TRY(twin(S.h_c, S.d_c, (size_t)images * 1024));
        RPH_TRY(twin(S.h_d, S.d_d, (size_t)images * 256));
        RPH_TRY(twin(S.h_v, S.d_v, images));
        if (pixel_hashes) RPH_TRY(twin(S.h_ph, S.d_ph, (size_t)images * 32));
    }
    *out = &P;
    return RPH_OK;
}

// pageable -> pinned with a few threads (one core moves ~10 GB/s, PCIe takes ~55)
void parallel_copy(uint8_t *dst, const uint8_t *src, size_t bytes)
{
    const size_t parts = bytes / ((size_t)4 << 20) + 1;
    const unsigned nt = parts > 1 ? (unsigned)std::min<size_t>(std::min(8u, rph_host_threads()), parts) : 1;
    const size_t part = align_up(bytes / nt, 4096);
    parallel_for(0, nt, nt, [&](size_t t) {
        const size_t lo = std::min(bytes, part * t), hi = std::min(bytes, part * (t + 1));
        if (hi > lo) std::memcpy(dst + lo, src + lo, hi - lo);
    });
}
}  // namespace

unsigned rph_host_threads()
{
    unsigned n = std::max(1u, std::thread::hardware_concurrency());
    cpu_set_t set;
    if (sched_getaffinity(0, sizeof set, &set) == 0) n = std::min<unsigned>(n, (unsigned)std::max(1, CPU_COUNT(&set)));
    long long quota = -1, period = 100000;
    if (FILE *f = fopen("/sys/fs/cgroup/cpu.max", "r")) {  // cgroup v2: "max 100000" or "1600000 100000"
        char q[32] = "";
        if (fscanf(f, "%31s %lld", q, &period) == 2 && strcmp(q, "max") != 0) quota = atoll(q);
        fclose(f);
    } else if (FILE *g = fopen("/sys/fs/cgroup/cpu/cpu.cfs_quota_us", "r")) {  // cgroup v1
        if (fscanf(g, "%lld", &quota) != 1) quota = -1;
        fclose(g);
        if (FILE *h = fopen("/sys/fs/cgroup/cpu/cpu.cfs_period_us", "r")) {
            if (fscanf(h, "%lld", &period) != 1) period = 100000;
            fclose(h);
        }
    }
    if (quota > 0 && period > 0) n = std::min<unsigned>(n, (unsigned)std::max<long long>(1, (quota + period - 1) / period));
    return n;
}

void rph_pipe_forget(rph_ctx *ctx)
{
    delete static_cast<HostPipe *>(ctx->pipe);
    ctx->pipe = nullptr;
}

extern "C" {

int rph_abi_version(void) { return RPH_ABI_VERSION; }
const char *rph_last_error(void) { return g_err; }
const char *rph_status_string(int s)
{
    switch (s) {
        case RPH_OK: return "ok";
        case RPH_ERR_INVALID_ARG: return "invalid argument";
        case RPH_ERR_NO_DEVICE: return "no usable gfx950 device";
        case RPH_ERR_HIP: return "HIP runtime error";
        case RPH_ERR_OOM: return "out of device memory";
        case RPH_ERR_UNSUPPORTED: return "unsupported input";
        case RPH_ERR_CAPACITY: return "output capacity too small";
    }
    return "unknown status";
}

int rph_init(int device, rph_ctx **out)
{
    return rph_guarded("rph_init", [&]() -> int {
        if (!out) return RPH_ERR_INVALID_ARG;
        *out = nullptr;
        int count = 0;
        if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) {
            rph_set_error("rph_init: no HIP device visible (this library has no CPU fallback)");
            return RPH_ERR_NO_DEVICE;
        }
        if (device < 0 || device >= count) {
            rph_set_error("rph_init: device %d out of range (%d visible)", device, count);
            return RPH_ERR_NO_DEVICE;
        }
        hipDeviceProp_t prop;
        RPH_HIP_CHECK(hipGetDeviceProperties(&prop, device));
        if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
            rph_set_error("rph_init: device %d is %s; this build targets gfx950 (MI355X) only", device, prop.gcnArchName);
            return RPH_ERR_NO_DEVICE;
        }
        RPH_HIP_CHECK(hipSetDevice(device));
        rph_ctx *ctx = new rph_ctx();
        static std::atomic<uint64_t> next_serial{1};
        ctx->serial = next_serial.fetch_add(1);
        ctx->device = device;
        ctx->compute_units = prop.multiProcessorCount;
        if (const char *e = getenv("RPH_RAGGED_CHUNK_BYTES"))  // tests: several staging chunks from a few small images
            if (const long long v = atoll(e); v > 0) ctx->ragged_chunk_bytes = (size_t)v;
        // tests: several chunks (and WebP parse windows) from a hundred small files
        rph_file_limits &fl = ctx->file_limits;
        const struct {
            const char *name;
            uint64_t *value;
        } knobs[] = {{"RPH_FILE_CHUNK_FILES", &fl.files},
                     {"RPH_FILE_CHUNK_COMP_BYTES", &fl.comp},
                     {"RPH_FILE_CHUNK_RAW_BYTES", &fl.raw},
                     {"RPH_FILE_CHUNK_PIXELS", &fl.pixels},
                     {"RPH_WEBP_CHUNK_TABLE_BYTES", &fl.webp_chunk_tables},
                     {"RPH_WEBP_WINDOW_TABLE_BYTES", &fl.webp_window_tables},
                     {"RPH_BMP_CHUNK_SRC_BYTES", &fl.bmp_src},
                     {"RPH_BMP_CHUNK_OUT_BYTES", &fl.bmp_out}};
        for (const auto &k : knobs)
            if (const char *e = getenv(k.name))
                if (const long long v = atoll(e); v > 0) *k.value = (uint64_t)v;
        hipError_t e = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking);
        if (e != hipSuccess) {
            rph_set_error("hipStreamCreate failed: %s", hipGetErrorString(e));
            delete ctx;
            return RPH_ERR_HIP;
        }
        *out = ctx;
        return RPH_OK;
    });
}

int rph_shutdown(rph_ctx *ctx)
{
    if (!ctx) return RPH_ERR_INVALID_ARG;
    rph_batcher_forget(ctx);
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    rph_pipe_forget(ctx);
    rph_ragged_forget(ctx);
    rph_resize_forget(ctx);
    rph_jpeg_forget(ctx);
    rph_png_forget(ctx);
    rph_tiff_forget(ctx);
    rph_webp_forget(ctx);
    rph_gif_forget(ctx);
    rph_bmp_forget(ctx);
    rph_jpeg_forget_threads(ctx);
    if (ctx->sink) (void)hipFree(ctx->sink);
    (void)hipStreamDestroy(ctx->stream);
    delete ctx;  // the shared and per-stream scratch free themselves
    return RPH_OK;
}

int rph_debug_file_chunks(rph_ctx *ctx, int format, uint32_t *sizes_out, uint32_t cap, uint32_t *n_chunks_out, uint32_t *n_windows_out)
{
    if (!ctx || format < 0 || format >= RPH_FILE_FORMATS) return RPH_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lock(ctx->file[format].mu);
    const rph_file_chunk_log &log = ctx->file[format].log;
    if (sizes_out)
        for (size_t k = 0; k < std::min<size_t>(cap, log.sizes.size()); k++) sizes_out[k] = log.sizes[k];
    if (n_chunks_out) *n_chunks_out = (uint32_t)log.sizes.size();
    if (n_windows_out) *n_windows_out = log.n_windows;
    return RPH_OK;
}

int rph_device_info(rph_ctx *ctx, char *name64, int *cus, uint64_t *total_mem)
{
    if (!ctx) return RPH_ERR_INVALID_ARG;
    hipDeviceProp_t prop;
    RPH_HIP_CHECK(hipGetDeviceProperties(&prop, ctx->device));
    if (name64) snprintf(name64, 64, "%s (%s)", prop.name, prop.gcnArchName);
    if (cus) *cus = prop.multiProcessorCount;
    if (total_mem) *total_mem = prop.totalGlobalMem;
    return RPH_OK;
}

int rph_synchronize(rph_ctx *ctx)
{
    if (!ctx) return RPH_ERR_INVALID_ARG;
    RPH_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return RPH_OK;
}

void *rph_stream(rph_ctx *ctx) { return ctx ? (void *)ctx->stream : nullptr; }

int rph_hamming_set_kernel(rph_ctx *ctx, int which)
{
    if (!ctx || which < 0 || which > 4) return RPH_ERR_INVALID_ARG;
    ctx->hamming_kernel = which;
    return RPH_OK;
}

int rph_pdq_set_kernel(rph_ctx *ctx, int which)
{
    if (!ctx || which < 0 || which > 6) return RPH_ERR_INVALID_ARG;
    ctx->pdq_kernel = which;
    return RPH_OK;
}

// ------------------------------------------------------------------------------------------
// PDQ
// ------------------------------------------------------------------------------------------
int rph_pdq_hash_batch_dev(rph_ctx *ctx, const void *d_px, uint32_t n, uint32_t w, uint32_t h, uint32_t channels,
                           size_t row_stride, size_t image_stride, void *d_hash32, void *d_quality, void *d_coeffs,
                           void *d_dihedral, void *d_valid, void *stream)
{
    if (!ctx || (!d_px && n) || !d_hash32 || !pdq_geometry_ok(n, w, h, channels, row_stride, image_stride)) {
        rph_set_error("rph_pdq_hash_batch: invalid argument (n=%u %ux%ux%u row_stride=%zu image_stride=%zu)", n, w, h,
                      channels, row_stride, image_stride);
        return RPH_ERR_INVALID_ARG;
    }
    if (n == 0) return RPH_OK;
    hipStream_t s = pick(ctx, stream);
    std::lock_guard<std::mutex> lock(ctx->mu);
    RPH_HIP_CHECK(hipSetDevice(ctx->device));
    if (w < RPH_PDQ_MIN_DIM || h < RPH_PDQ_MIN_DIM) {
        // generate_pdq_features returns None (pdqhash.rs:167-169): valid = 0, outputs zeroed
        RPH_HIP_CHECK(hipMemsetAsync(d_hash32, 0, (size_t)n * 32, s));
        if (d_quality) RPH_HIP_CHECK(hipMemsetAsync(d_quality, 0, (size_t)n * 4, s));
        if (d_coeffs) RPH_HIP_CHECK(hipMemsetAsync(d_coeffs, 0, (size_t)n * 1024, s));
        if (d_dihedral) RPH_HIP_CHECK(hipMemsetAsync(d_dihedral, 0, (size_t)n * 256, s));
        if (d_valid) RPH_HIP_CHECK(hipMemsetAsync(d_valid, 0, n, s));
        return RPH_OK;
    }
    if (w > RPH_PDQ_MAX_DIM || h > RPH_PDQ_MAX_DIM)  // pre-downsample to the <= 512 px thumbnail first (pdqhash.rs:181-191)
        return rph_launch_pdq_resized(ctx, (const uint8_t *)d_px, n, w, h, channels, row_stride, image_stride, (uint8_t *)d_hash32,
                                      (float *)d_quality, (float *)d_coeffs, (uint8_t *)d_dihedral, (uint8_t *)d_valid, s);
    if (ctx->pdq_kernel >= 1 && ctx->pdq_kernel != 5 && w == 512 && h == 512 && (channels == 3 || channels == 1) && (row_stride % 4) == 0 && (image_stride % 4) == 0 &&
        ((uintptr_t)d_px % 4) == 0 && row_stride <= ((size_t)1 << 22)) {  // the fused kernel uses 32-bit in-image offsets
        int rc = rph_launch_pdq_fused512(ctx, (const uint8_t *)d_px, n, row_stride, image_stride, (uint8_t *)d_hash32,
                                         (float *)d_quality, (float *)d_coeffs, (uint8_t *)d_dihedral, (uint8_t *)d_valid, s, channels);
        if (rc != RPH_ERR_UNSUPPORTED) return rc;
    }
    // every other Luma8 geometry from 128 x 128: the streaming single-pass kernel (pdq_stream.hip) -- one wave per image, ~0.4 ms from an
    // image's first byte to its hash however few there are, so calls of a few images (the one-image-per-call queue) keep the multi-pass
    // kernels, which spread an image over the chip (~0.15 ms)
    const bool stream_ok = ctx->pdq_kernel >= 1 && ctx->pdq_kernel != 5 && (n >= RPH_STREAM_MIN_IMAGES || ctx->pdq_kernel == 6);
    if (stream_ok && rph_pdq_stream_supported((const uint8_t *)d_px, w, h, channels, row_stride, image_stride)) {
        return rph_launch_pdq_stream(ctx, (const uint8_t *)d_px, n, w, h, row_stride, image_stride, (uint8_t *)d_hash32, (float *)d_quality, (float *)d_coeffs,
                                     (uint8_t *)d_dihedral, (uint8_t *)d_valid, s);
    }
    if (stream_ok && rph_pdq_stream_color_supported((const uint8_t *)d_px, w, h, channels, row_stride, image_stride))
        return rph_launch_pdq_stream_color(ctx, (const uint8_t *)d_px, n, w, h, channels, row_stride, image_stride, (uint8_t *)d_hash32, (float *)d_quality,
                                           (float *)d_coeffs, (uint8_t *)d_dihedral, (uint8_t *)d_valid, s);
    return rph_launch_pdq_generic(ctx, (const uint8_t *)d_px, n, w, h, channels, row_stride, image_stride, (uint8_t *)d_hash32,
                                  (float *)d_quality, (float *)d_coeffs, (uint8_t *)d_dihedral, (uint8_t *)d_valid, s);
}

int rph_pdq_hash_batch(rph_ctx *ctx, const uint8_t *px, uint32_t n, uint32_t w, uint32_t h, uint32_t channels,
                       size_t row_stride, size_t image_stride, uint8_t *hash32_out, float *quality_out, float *coeffs_out,
                       uint8_t *dihedral_out, uint8_t *valid_out)
{
    return rph_pdq_hash_batch_keep(ctx, px, n, w, h, channels, row_stride, image_stride, hash32_out, quality_out, coeffs_out, dihedral_out, valid_out,
                                   nullptr, nullptr, nullptr);
}

}  // extern "C"

// rph_pdq_hash_batch, optionally leaving device-resident copies of the per-image results behind (rph_multi: the hash blocks
// go straight into the all-gather, multi.cpp).  d_*_keep: device arrays of n records on ctx's device, or nullptr.
int rph_pdq_hash_batch_keep(rph_ctx *ctx, const uint8_t *px, uint32_t n, uint32_t w, uint32_t h, uint32_t channels, size_t row_stride,
                            size_t image_stride, uint8_t *hash32_out, float *quality_out, float *coeffs_out, uint8_t *dihedral_out,
                            uint8_t *valid_out, void *d_hash_keep, void *d_quality_keep, void *d_dihedral_keep)
{
    return rph_guarded("rph_pdq_hash_batch", [&]() -> int {
        if (!ctx || (!px && n) || !hash32_out) {
            rph_set_error("rph_pdq_hash_batch: null argument");
            return RPH_ERR_INVALID_ARG;
        }
        if (n == 0) return RPH_OK;
        if (!pdq_geometry_ok(n, w, h, channels, row_stride, image_stride)) {
            rph_set_error("rph_pdq_hash_batch: invalid argument (n=%u %ux%ux%u row_stride=%zu image_stride=%zu)", n, w, h, channels,
                          row_stride, image_stride);
            return RPH_ERR_INVALID_ARG;
        }
        RPH_HIP_CHECK(hipSetDevice(ctx->device));
        // Chunks of <= 64 MiB of pixels alternate between two staging sets (pinned host + device) and two streams: while chunk k
        // crosses PCIe and is hashed, the host threads copy chunk k + 1 from the caller's (pageable) memory into the other pinned set.
        const size_t one_image = (size_t)(h ? h - 1 : 0) * row_stride + (size_t)w * channels;
        const size_t per = n > 1 ? image_stride : std::max<size_t>(one_image, 1);
        const uint32_t chunk = (uint32_t)std::min<size_t>(n, std::max<size_t>(1, kPipeChunkBytes / per));
        std::lock_guard<std::mutex> pipe_lock(ctx->pipe_mu);
        HostPipe *P = nullptr;
        RPH_TRY(pipe_of(ctx, per * (chunk - 1) + one_image, chunk, &P));
        struct Pending {
            uint32_t first = 0, m = 0;
            bool active = false;
        } pend[2];
        auto finish = [&](int b) -> int {  // results of the chunk that used set b -> the caller's arrays
            if (!pend[b].active) return RPH_OK;
            const PipeSet &S = P->set[b];
            RPH_HIP_CHECK(hipStreamSynchronize(S.stream));
            const uint32_t first = pend[b].first, m = pend[b].m;
            std::memcpy(hash32_out + (size_t)first * 32, S.h_hash.data(), (size_t)m * 32);
            if (quality_out) std::memcpy(quality_out + first, S.h_q.data(), (size_t)m * 4);
            if (coeffs_out) std::memcpy(coeffs_out + (size_t)first * 256, S.h_c.data(), (size_t)m * 1024);
            if (dihedral_out) std::memcpy(dihedral_out + (size_t)first * 256, S.h_d.data(), (size_t)m * 256);
            if (valid_out) std::memcpy(valid_out + first, S.h_v.data(), m);
            pend[b].active = false;
            return RPH_OK;
        };
        int k = 0;
        for (uint32_t first = 0; first < n; first += chunk, k++) {
            const int b = k & 1;
            RPH_TRY(finish(b));
            PipeSet &S = P->set[b];
            const uint32_t m = std::min(chunk, n - first);
            const size_t bytes = (size_t)(m - 1) * per + one_image;  // the last image may be shorter than image_stride in the caller's buffer
            parallel_copy(S.h_px.data(), px + (size_t)first * per, bytes);
            hipStream_t s = S.stream;
            RPH_HIP_CHECK(hipMemcpyAsync(S.d_px.data(), S.h_px.data(), bytes, hipMemcpyHostToDevice, s));
            const bool want_q = quality_out || d_quality_keep, want_d = dihedral_out || d_dihedral_keep;
            RPH_TRY(rph_pdq_hash_batch_dev(ctx, S.d_px.data(), m, w, h, channels, row_stride, per, S.d_hash.data(), want_q ? S.d_q.data() : nullptr,
                                           coeffs_out ? S.d_c.data() : nullptr, want_d ? S.d_d.data() : nullptr, valid_out ? S.d_v.data() : nullptr, s));
            if (d_hash_keep) RPH_HIP_CHECK(hipMemcpyAsync((uint8_t *)d_hash_keep + (size_t)first * 32, S.d_hash.data(), (size_t)m * 32, hipMemcpyDeviceToDevice, s));
            if (d_quality_keep) RPH_HIP_CHECK(hipMemcpyAsync((float *)d_quality_keep + first, S.d_q.data(), (size_t)m * 4, hipMemcpyDeviceToDevice, s));
            if (d_dihedral_keep)
                RPH_HIP_CHECK(hipMemcpyAsync((uint8_t *)d_dihedral_keep + (size_t)first * 256, S.d_d.data(), (size_t)m * 256, hipMemcpyDeviceToDevice, s));
            RPH_HIP_CHECK(hipMemcpyAsync(S.h_hash.data(), S.d_hash.data(), (size_t)m * 32, hipMemcpyDeviceToHost, s));
            if (quality_out) RPH_HIP_CHECK(hipMemcpyAsync(S.h_q.data(), S.d_q.data(), (size_t)m * 4, hipMemcpyDeviceToHost, s));
            if (coeffs_out) RPH_HIP_CHECK(hipMemcpyAsync(S.h_c.data(), S.d_c.data(), (size_t)m * 1024, hipMemcpyDeviceToHost, s));
            if (dihedral_out) RPH_HIP_CHECK(hipMemcpyAsync(S.h_d.data(), S.d_d.data(), (size_t)m * 256, hipMemcpyDeviceToHost, s));
            if (valid_out) RPH_HIP_CHECK(hipMemcpyAsync(S.h_v.data(), S.d_v.data(), m, hipMemcpyDeviceToHost, s));
            pend[b].first = first;
            pend[b].m = m;
            pend[b].active = true;
        }
        RPH_TRY(finish(k & 1));
        RPH_TRY(finish((k + 1) & 1));
        return RPH_OK;
    });
}

// Host form of the ragged calls: the images are packed into the pinned staging sets of rph_pdq_hash_batch -- each at a 16-byte aligned
// offset, rows at a pitch that is a multiple of 4 (the streaming kernel reads Luma8 images of 128..512 px straight from there; 16-bit
// images lie at even addresses with even pitches) -- in chunks of ctx->ragged_chunk_bytes; chunk k is hashed while the host threads pack
// chunk k + 1 into the other set.  layout: RPH_LAYOUT_* codes, checked by the caller; hash32_out or pixel_hash32_out may be null
// (rph_image_hash_ragged): both hashes of a chunk come from its one upload.
static int ragged_host(rph_ctx *ctx, const uint8_t *const *px, const uint32_t *w, const uint32_t *h, const uint32_t *layout, const size_t *row_stride, uint32_t n,
                       uint8_t *hash32_out, float *quality_out, float *coeffs_out, uint8_t *dihedral_out, uint8_t *valid_out, uint8_t *pixel_hash32_out)
{
    RPH_HIP_CHECK(hipSetDevice(ctx->device));
    // the packed form of every image, and the chunks
    constexpr uint32_t kMaxChunkImages = 16384;
    std::vector<size_t> pitch(n);
    std::vector<uint64_t> offset(n);
    std::vector<uint32_t> chunk_first;  // + the end
    size_t max_bytes = 0, bytes = 0;
    uint32_t max_images = 0;
    for (uint32_t i = 0; i < n; i++) {
        pitch[i] = align_up((size_t)w[i] * rph_layout_bytes(layout[i]), 4);
        const size_t size = pitch[i] * h[i];
        // (an image larger than a chunk gets one of its own)
        if (chunk_first.empty() || (i > chunk_first.back() && (align_up(bytes, 16) + size > ctx->ragged_chunk_bytes || i - chunk_first.back() >= kMaxChunkImages))) {
            chunk_first.push_back(i);
            bytes = 0;
        }
        offset[i] = align_up(bytes, 16);
        bytes = offset[i] + size;
        max_bytes = std::max(max_bytes, bytes);
        max_images = std::max(max_images, i - chunk_first.back() + 1);
    }
    chunk_first.push_back(n);
    std::lock_guard<std::mutex> pipe_lock(ctx->pipe_mu);
    HostPipe *P = nullptr;
    RPH_TRY(pipe_of(ctx, max_bytes + 16, max_images, &P, pixel_hash32_out != nullptr));
    struct Pending {
        uint32_t first = 0, m = 0;
        bool active = false;
    } pend[2];
    auto finish = [&](int b) -> int {  // results of the chunk that used set b -> the caller's arrays
        if (!pend[b].active) return RPH_OK;
        const PipeSet &S = P->set[b];
        RPH_HIP_CHECK(hipStreamSynchronize(S.stream));
        const uint32_t first = pend[b].first, m = pend[b].m;
        if (hash32_out) std::memcpy(hash32_out + (size_t)first * 32, S.h_hash.data(), (size_t)m * 32);
        if (quality_out) std::memcpy(quality_out + first, S.h_q.data(), (size_t)m * 4);
        if (coeffs_out) std::memcpy(coeffs_out + (size_t)first * 256, S.h_c.data(), (size_t)m * 1024);
        if (dihedral_out) std::memcpy(dihedral_out + (size_t)first * 256, S.h_d.data(), (size_t)m * 256);
        if (valid_out) std::memcpy(valid_out + first, S.h_v.data(), m);
        if (pixel_hash32_out) std::memcpy(pixel_hash32_out + (size_t)first * 32, S.h_ph.data(), (size_t)m * 32);
        pend[b].active = false;
        return RPH_OK;
    };
    const unsigned nt = std::min(8u, rph_host_threads());
    for (size_t k = 0; k + 1 < chunk_first.size(); k++) {
        const int b = (int)(k & 1);
        RPH_TRY(finish(b));
        PipeSet &S = P->set[b];
        const uint32_t first = chunk_first[k], m = chunk_first[k + 1] - first;
        parallel_for(first, first + m, nt, [&](size_t i) {
            uint8_t *to = S.h_px.data() + offset[i];
            const size_t row = (size_t)w[i] * rph_layout_bytes(layout[i]);
            if (row_stride[i] == pitch[i]) {
                if (h[i]) std::memcpy(to, px[i], pitch[i] * (h[i] - 1) + row);
            } else {
                for (uint32_t y = 0; y < h[i]; y++) std::memcpy(to + y * pitch[i], px[i] + (size_t)y * row_stride[i], row);
            }
        });
        const size_t used = (size_t)offset[first + m - 1] + pitch[first + m - 1] * h[first + m - 1];
        hipStream_t s = S.stream;
        if (used) RPH_HIP_CHECK(hipMemcpyAsync(S.d_px.data(), S.h_px.data(), used, hipMemcpyHostToDevice, s));
        RPH_TRY(rph_image_ragged_run(ctx, S.d_px.data(), offset.data() + first, w + first, h + first, layout + first, pitch.data() + first, m,
                                     hash32_out ? S.d_hash.data() : nullptr, quality_out ? S.d_q.as<float>() : nullptr, coeffs_out ? S.d_c.as<float>() : nullptr,
                                     dihedral_out ? S.d_d.data() : nullptr, valid_out ? S.d_v.data() : nullptr, pixel_hash32_out ? S.d_ph.data() : nullptr, s));
        if (hash32_out) RPH_HIP_CHECK(hipMemcpyAsync(S.h_hash.data(), S.d_hash.data(), (size_t)m * 32, hipMemcpyDeviceToHost, s));
        if (quality_out) RPH_HIP_CHECK(hipMemcpyAsync(S.h_q.data(), S.d_q.data(), (size_t)m * 4, hipMemcpyDeviceToHost, s));
        if (coeffs_out) RPH_HIP_CHECK(hipMemcpyAsync(S.h_c.data(), S.d_c.data(), (size_t)m * 1024, hipMemcpyDeviceToHost, s));
        if (dihedral_out) RPH_HIP_CHECK(hipMemcpyAsync(S.h_d.data(), S.d_d.data(), (size_t)m * 256, hipMemcpyDeviceToHost, s));
        if (valid_out) RPH_HIP_CHECK(hipMemcpyAsync(S.h_v.data(), S.d_v.data(), m, hipMemcpyDeviceToHost, s));
        if (pixel_hash32_out) RPH_HIP_CHECK(hipMemcpyAsync(S.h_ph.data(), S.d_ph.data(), (size_t)m * 32, hipMemcpyDeviceToHost, s));
        pend[b].first = first;
        pend[b].m = m;
        pend[b].active = true;
    }
    RPH_TRY(finish(0));
    RPH_TRY(finish(1));
    return RPH_OK;
}

extern "C" int rph_pdq_hash_ragged(rph_ctx *ctx, const uint8_t *const *px, const uint32_t *w, const uint32_t *h, const uint32_t *channels, const size_t *row_stride,
                                   uint32_t n, uint8_t *hash32_out, float *quality_out, float *coeffs_out, uint8_t *dihedral_out, uint8_t *valid_out)
{
    return rph_guarded("rph_pdq_hash_ragged", [&]() -> int {
        if (ctx && n == 0) return RPH_OK;
        if (!ctx || !hash32_out || !px || !w || !h || !channels || !row_stride) {
            rph_set_error("rph_pdq_hash_ragged: null argument");
            return RPH_ERR_INVALID_ARG;
        }
        for (uint32_t i = 0; i < n; i++)
            if (!px[i] || (channels[i] != 1 && channels[i] != 3 && channels[i] != 4) || row_stride[i] < (size_t)w[i] * channels[i]) {
                rph_set_error("rph_pdq_hash_ragged: invalid argument (image %u: %ux%ux%u row_stride=%zu)", i, w[i], h[i], channels[i], px[i] ? row_stride[i] : (size_t)0);
                return RPH_ERR_INVALID_ARG;
            }
        return ragged_host(ctx, px, w, h, channels, row_stride, n, hash32_out, quality_out, coeffs_out, dihedral_out, valid_out, nullptr);
    });
}

// what is wrong with one image of an rph_image_* call (px: null only where the caller allows it), or nullptr
static const char *image_fault(const void *px, uint32_t w, uint32_t h, uint32_t layout, size_t row_stride)
{
    const uint32_t bpp = rph_layout_bytes(layout);
    if (!bpp) return "unknown layout";
    if (row_stride < (size_t)w * bpp) return "row_stride below the row's bytes";
    if (layout > 16 && (((uintptr_t)px | row_stride) & 1)) return "16-bit image at an odd address or with an odd row_stride";
    if ((uint64_t)w * h > ((uint64_t)1 << 40)) return "more than 2^40 pixels";
    return nullptr;
}

extern "C" int rph_image_hash_ragged(rph_ctx *ctx, const void *const *px, const uint32_t *w, const uint32_t *h, const uint32_t *layout, const size_t *row_stride,
                                     uint32_t n, uint8_t *hash32_out, float *quality_out, float *coeffs_out, uint8_t *dihedral_out, uint8_t *valid_out,
                                     uint8_t *pixel_hash32_out)
{
    return rph_guarded("rph_image_hash_ragged", [&]() -> int {
        if (ctx && n == 0) return RPH_OK;
        if (!ctx || !px || !w || !h || !layout || !row_stride || (!hash32_out && !pixel_hash32_out) ||
            (!hash32_out && (quality_out || coeffs_out || dihedral_out || valid_out))) {
            rph_set_error("rph_image_hash_ragged: null argument (or no output, or PDQ outputs without hash32_out)");
            return RPH_ERR_INVALID_ARG;
        }
        for (uint32_t i = 0; i < n; i++)
            if (const char *why = px[i] ? image_fault(px[i], w[i], h[i], layout[i], row_stride[i]) : "null pixels") {
                rph_set_error("rph_image_hash_ragged: invalid argument (image %u: %ux%u layout %u: %s)", i, w[i], h[i], layout[i], why);
                return RPH_ERR_INVALID_ARG;
            }
        return ragged_host(ctx, reinterpret_cast<const uint8_t *const *>(px), w, h, layout, row_stride, n, hash32_out, quality_out, coeffs_out, dihedral_out, valid_out,
                           pixel_hash32_out);
    });
}

// the native samples of pixel x of a row (pixel_rules.h takes them as u32)
static inline void native_samples(const uint8_t *row, uint32_t x, uint32_t ch, bool wide, uint32_t v[4])
{
    for (uint32_t k = 0; k < ch; k++) {
        if (wide) {
            uint16_t s;
            std::memcpy(&s, row + ((size_t)x * ch + k) * 2, 2);
            v[k] = s;
        } else {
            v[k] = row[(size_t)x * ch + k];
        }
    }
}

extern "C" int rph_image_luma601_host(const void *px, uint32_t w, uint32_t h, uint32_t layout, size_t row_stride, uint8_t *luma_out)
{
    return rph_guarded("rph_image_luma601_host", [&]() -> int {
        const bool empty = (uint64_t)w * h == 0;
        if (const char *why = !px && !empty ? "null pixels" : image_fault(px, w, h, layout, row_stride); why || (!luma_out && !empty)) {
            rph_set_error("rph_image_luma601_host: invalid argument (%ux%u layout %u: %s)", w, h, layout, why ? why : "null output");
            return RPH_ERR_INVALID_ARG;
        }
        const uint32_t ch = layout & 15u, depth = layout > 16 ? 16 : 8;
        for (uint32_t y = 0; y < h; y++) {
            const uint8_t *row = (const uint8_t *)px + (size_t)y * row_stride;
            for (uint32_t x = 0; x < w; x++) {
                uint32_t v[4] = {0, 0, 0, 0};
                uint8_t o[4] = {0, 0, 0, 0};
                native_samples(row, x, ch, depth == 16, v);
                rphx::hasher_pixel(ch, depth, v, o);
                // to_luma601 (pdqhash.rs:268-284) of the hasher's pixel; Luma8 is borrowed
                luma_out[(size_t)y * w + x] = (ch == 1 && depth == 8) ? o[0] : (uint8_t)((299u * o[0] + 587u * o[1] + 114u * o[2] + 500u) / 1000u);
            }
        }
        return RPH_OK;
    });
}

extern "C" int rph_image_pixel_hash_host(const void *px, uint32_t w, uint32_t h, uint32_t layout, size_t row_stride, uint8_t *digest32_out)
{
    return rph_guarded("rph_image_pixel_hash_host", [&]() -> int {
        const bool empty = (uint64_t)w * h == 0;
        if (const char *why = !px && !empty ? "null pixels" : image_fault(px, w, h, layout, row_stride); why || !digest32_out) {
            rph_set_error("rph_image_pixel_hash_host: invalid argument (%ux%u layout %u: %s)", w, h, layout, why ? why : "null output");
            return RPH_ERR_INVALID_ARG;
        }
        const uint32_t ch = layout & 15u;
        const bool wide = layout > 16;
        std::vector<uint8_t> stream((size_t)w * h * 8);  // to_rgba16() as little-endian bytes
        size_t at = 0;
        for (uint32_t y = 0; y < h; y++) {
            const uint8_t *row = (const uint8_t *)px + (size_t)y * row_stride;
            for (uint32_t x = 0; x < w; x++) {
                uint32_t v[4] = {0, 0, 0, 0};
                uint16_t o[4];
                native_samples(row, x, ch, wide, v);
                if (!wide)
                    for (uint32_t k = 0; k < ch; k++) v[k] *= 257u;  // the crate's u8 -> u16
                rphx::rgba16_pixel(ch, v, o);
                for (int k = 0; k < 4; k++) stream[at++] = (uint8_t)(o[k] & 0xFF), stream[at++] = (uint8_t)(o[k] >> 8);
            }
        }
        rph_blake3_host(stream.data(), stream.size(), nullptr, digest32_out);
        return RPH_OK;
    });
}

extern "C" {

int rph_pdq_hashes_from_coeffs_dev(rph_ctx *ctx, const void *d_coeffs, uint32_t n, void *d_hash32, void *d_dihedral,
                                   void *stream)
{
    if (!ctx || (!d_coeffs && n) || (!d_hash32 && !d_dihedral)) {
        rph_set_error("rph_pdq_hashes_from_coeffs: null argument");
        return RPH_ERR_INVALID_ARG;
    }
    RPH_HIP_CHECK(hipSetDevice(ctx->device));
    return rph_launch_pdq_from_coeffs((const float *)d_coeffs, n, (uint8_t *)d_hash32, (uint8_t *)d_dihedral, pick(ctx, stream));
}

int rph_pdq_hashes_from_coeffs(rph_ctx *ctx, const float *coeffs, uint32_t n, uint8_t *hash32_out, uint8_t *dihedral_out)
{
    return rph_guarded("rph_pdq_hashes_from_coeffs", [&]() -> int {
        if (!ctx || (!coeffs && n) || (!hash32_out && !dihedral_out)) {
            rph_set_error("rph_pdq_hashes_from_coeffs: null argument");
            return RPH_ERR_INVALID_ARG;
        }
        if (n == 0) return RPH_OK;
        RPH_HIP_CHECK(hipSetDevice(ctx->device));
        DevBuf d_c, d_h, d_d;
        RPH_TRY(d_c.alloc((size_t)n * 1024));
        if (hash32_out) RPH_TRY(d_h.alloc((size_t)n * 32));
        if (dihedral_out) RPH_TRY(d_d.alloc((size_t)n * 256));
        RPH_HIP_CHECK(hipMemcpyAsync(d_c.data(), coeffs, (size_t)n * 1024, hipMemcpyHostToDevice, ctx->stream));
        RPH_TRY(rph_pdq_hashes_from_coeffs_dev(ctx, d_c.data(), n, d_h.data(), d_d.data(), ctx->stream));
        if (hash32_out) RPH_HIP_CHECK(hipMemcpyAsync(hash32_out, d_h.data(), (size_t)n * 32, hipMemcpyDeviceToHost, ctx->stream));
        if (dihedral_out) RPH_HIP_CHECK(hipMemcpyAsync(dihedral_out, d_d.data(), (size_t)n * 256, hipMemcpyDeviceToHost, ctx->stream));
        RPH_HIP_CHECK(hipStreamSynchronize(ctx->stream));
        return RPH_OK;
    });
}

// ------------------------------------------------------------------------------------------
// Hamming
// ------------------------------------------------------------------------------------------
int rph_hamming_all_pairs_dev(rph_ctx *ctx, const void *d_hashes32, uint64_t n, uint32_t threshold, uint32_t part,
                              uint32_t nparts, void *d_edges, uint64_t cap, void *d_count, void *stream)
{
    return sweep_dev("rph_hamming_all_pairs", ctx,
                     into(square_sweep(d_hashes32, 1, d_hashes32, nullptr, nullptr, n, threshold, part, nparts), d_edges, cap, d_count), stream);
}

int rph_hamming_variant_pairs_dev(rph_ctx *ctx, const void *d_variants, uint32_t n_variants, const void *d_hashes32,
                                  const void *d_low_conf, uint64_t n, uint32_t similarity, uint32_t part, uint32_t nparts,
                                  void *d_edges, uint64_t cap, void *d_count, void *stream)
{
    return sweep_dev("rph_hamming_variant_pairs", ctx,
                     into(square_sweep(d_variants, n_variants, d_hashes32, d_low_conf, nullptr, n, similarity, part, nparts), d_edges, cap, d_count),
                     stream);
}

int rph_hamming_all_pairs(rph_ctx *ctx, const uint8_t *hashes32, uint64_t n, uint32_t threshold, uint32_t part,
                          uint32_t nparts, rph_edge *edges, uint64_t cap, uint64_t *n_edges_out)
{
    return rph_guarded("rph_hamming_all_pairs", [&]() -> int {
        return sweep_host("rph_hamming_all_pairs", ctx, into(square_sweep(nullptr, 1, hashes32, nullptr, nullptr, n, threshold, part, nparts), edges, cap),
                          n_edges_out);
    });
}

int rph_hamming_variant_pairs(rph_ctx *ctx, const uint8_t *variants, uint32_t n_variants, const uint8_t *hashes32,
                              const uint8_t *low_conf, uint64_t n, uint32_t similarity, uint32_t part, uint32_t nparts,
                              rph_edge *edges, uint64_t cap, uint64_t *n_edges_out)
{
    return rph_guarded("rph_hamming_variant_pairs", [&]() -> int {
        if (!variants && n) {
            rph_set_error("rph_hamming_variant_pairs: variants is null");
            return RPH_ERR_INVALID_ARG;
        }
        return sweep_host("rph_hamming_variant_pairs", ctx,
                          into(square_sweep(variants, n_variants, hashes32, low_conf, nullptr, n, similarity, part, nparts), edges, cap), n_edges_out);
    });
}

// ---- cross sweeps: set A (variants, flags) against set B (hashes, flags), every pair ----
int rph_hamming_variant_cross_pairs_dev(rph_ctx *ctx, const void *d_variants_a, uint32_t n_variants, const void *d_low_conf_a, uint64_t n_a,
                                        const void *d_hashes_b, const void *d_low_conf_b, uint64_t n_b, uint32_t similarity, uint32_t part,
                                        uint32_t nparts, void *d_edges, uint64_t cap, void *d_count, void *stream)
{
    return sweep_dev("rph_hamming_variant_cross_pairs", ctx,
                     into(cross_sweep(d_variants_a, n_variants, d_low_conf_a, nullptr, n_a, d_hashes_b, d_low_conf_b, n_b, similarity, part, nparts), d_edges,
                          cap, d_count),
                     stream);
}

int rph_hamming_cross_pairs_dev(rph_ctx *ctx, const void *d_a32, uint64_t n_a, const void *d_b32, uint64_t n_b, uint32_t threshold, uint32_t part,
                                uint32_t nparts, void *d_edges, uint64_t cap, void *d_count, void *stream)
{
    return rph_hamming_variant_cross_pairs_dev(ctx, d_a32, 1, nullptr, n_a, d_b32, nullptr, n_b, threshold, part, nparts, d_edges, cap, d_count,
                                               stream);
}

int rph_hamming_variant_cross_pairs(rph_ctx *ctx, const uint8_t *variants_a, uint32_t n_variants, const uint8_t *low_conf_a, uint64_t n_a,
                                    const uint8_t *hashes_b, const uint8_t *low_conf_b, uint64_t n_b, uint32_t similarity, uint32_t part,
                                    uint32_t nparts, rph_edge *edges, uint64_t cap, uint64_t *n_edges_out)
{
    return rph_guarded("rph_hamming_variant_cross_pairs", [&]() -> int {
        return sweep_host("rph_hamming_variant_cross_pairs", ctx,
                          into(cross_sweep(variants_a, n_variants, low_conf_a, nullptr, n_a, hashes_b, low_conf_b, n_b, similarity, part, nparts), edges, cap),
                          n_edges_out);
    });
}

int rph_hamming_cross_pairs(rph_ctx *ctx, const uint8_t *a32, uint64_t n_a, const uint8_t *b32, uint64_t n_b, uint32_t threshold, uint32_t part,
                            uint32_t nparts, rph_edge *edges, uint64_t cap, uint64_t *n_edges_out)
{
    return rph_guarded("rph_hamming_cross_pairs", [&]() -> int {
        return sweep_host("rph_hamming_cross_pairs", ctx,
                          into(cross_sweep(a32, 1, nullptr, nullptr, n_a, b32, nullptr, n_b, threshold, part, nparts), edges, cap), n_edges_out);
    });
}

// ---- 64-bit hashes ----
static rph_sweep square_sweep64(const void *rows, const void *hashes64, uint64_t n, uint32_t threshold, uint32_t part, uint32_t nparts)
{
    rph_sweep q = square_sweep(rows, 1, hashes64, nullptr, nullptr, n, threshold, part, nparts);
    q.bits64 = true;
    return q;
}

int rph_hamming_all_pairs64_dev(rph_ctx *ctx, const void *d_hashes64, uint64_t n, uint32_t threshold, uint32_t part,
                                uint32_t nparts, void *d_edges, uint64_t cap, void *d_count, void *stream)
{
    return sweep_dev("rph_hamming_all_pairs64", ctx, into(square_sweep64(d_hashes64, d_hashes64, n, threshold, part, nparts), d_edges, cap, d_count), stream);
}

int rph_hamming_all_pairs64(rph_ctx *ctx, const uint64_t *hashes64, uint64_t n, uint32_t threshold, uint32_t part,
                            uint32_t nparts, rph_edge *edges, uint64_t cap, uint64_t *n_edges_out)
{
    return rph_guarded("rph_hamming_all_pairs64", [&]() -> int {
        return sweep_host("rph_hamming_all_pairs64", ctx, into(square_sweep64(nullptr, hashes64, n, threshold, part, nparts), edges, cap), n_edges_out);
    });
}

// rph_find_groups256 / rph_find_groups64: all pairs of one set, the operands uploaded once, then find_groups over the edges on the host
static int find_groups(const char *who, rph_ctx *ctx, const rph_sweep &q, uint32_t *members, uint32_t *offsets, uint32_t *n_groups_out)
{
    if (!ctx || (!q.cols && q.n) || !members || !offsets || !n_groups_out) {
        rph_set_error("%s: null argument", who);
        return RPH_ERR_INVALID_ARG;
    }
    *n_groups_out = 0;
    offsets[0] = 0;
    if (q.n < 2) return RPH_OK;
    RPH_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    SweepOperands ops;
    rph_sweep d;
    RPH_TRY(ops.upload(q, s, d));
    std::vector<rph_edge> edges;
    RPH_TRY(sweep_growing(who, std::max<uint64_t>(1u << 20, 4 * q.n), RPH_GROW_FIND_GROUPS, s, edges, [&](EdgeSink &sink, uint64_t cap) -> int {
        RPH_TRY(sink.open(cap, s, d));
        return rph_launch_hamming_sweep(ctx, d, s, ctx->hamming_kernel);
    }));
    return rph_host_find_groups(edges.data(), edges.size(), q.n, members, offsets, n_groups_out);
}

int rph_find_groups64(rph_ctx *ctx, const uint64_t *hashes64, uint64_t n, uint32_t max_dist, uint32_t *members,
                      uint32_t *offsets, uint32_t *n_groups_out)
{
    return rph_guarded("rph_find_groups64", [&]() -> int {
        return find_groups("rph_find_groups64", ctx, square_sweep64(nullptr, hashes64, n, max_dist, 0, 1), members, offsets, n_groups_out);
    });
}

int rph_find_groups_from_edges(const rph_edge *edges, uint64_t n_edges, uint64_t n, uint32_t *members, uint32_t *offsets,
                               uint32_t *n_groups_out)
{
    return rph_guarded("rph_find_groups_from_edges", [&]() -> int {
        if ((!edges && n_edges) || !members || !offsets || !n_groups_out) return RPH_ERR_INVALID_ARG;
        return rph_host_find_groups(edges, n_edges, n, members, offsets, n_groups_out);
    });
}

int rph_union_find_groups(const rph_edge *edges, uint64_t n_edges, uint64_t n, uint32_t *members, uint32_t *offsets,
                          uint32_t *n_groups_out)
{
    return rph_guarded("rph_union_find_groups", [&]() -> int {
        if ((!edges && n_edges) || !members || !offsets || !n_groups_out) return RPH_ERR_INVALID_ARG;
        return rph_host_union_find(edges, n_edges, n, members, offsets, n_groups_out);
    });
}

int rph_find_groups256(rph_ctx *ctx, const uint8_t *hashes32, uint64_t n, uint32_t max_dist, uint32_t *members,
                       uint32_t *offsets, uint32_t *n_groups_out)
{
    return rph_guarded("rph_find_groups256", [&]() -> int {
        return find_groups("rph_find_groups256", ctx, square_sweep(nullptr, 1, hashes32, nullptr, nullptr, n, max_dist, 0, 1), members, offsets,
                           n_groups_out);
    });
}

// scanner.rs:1650-1655 asserts this
static int check_similarity(uint32_t similarity)
{
    if (similarity <= RPH_MAX_SIMILARITY_256) return RPH_OK;
    rph_set_error("Similarity distances above %u require R=4 bit-flip checks, which are not implemented.", RPH_MAX_SIMILARITY_256);
    return RPH_ERR_INVALID_ARG;
}

int rph_group_files_pdq(rph_ctx *ctx, const uint8_t *hashes32, const float *coeffs, const uint8_t *has_features,
                        const int32_t *quality, uint64_t n, uint32_t similarity, uint32_t *members, uint32_t *offsets,
                        uint32_t *n_groups_out, uint64_t *comparison_count_out)
{
    return rph_guarded("rph_group_files_pdq", [&]() -> int {
        if (!ctx || (!hashes32 && n) || !members || !offsets || !n_groups_out) {
            rph_set_error("rph_group_files_pdq: null argument");
            return RPH_ERR_INVALID_ARG;
        }
        RPH_TRY(check_similarity(similarity));
        *n_groups_out = 0;
        offsets[0] = 0;
        if (comparison_count_out) *comparison_count_out = 0;
        if (n < 2) return RPH_OK;
        RPH_HIP_CHECK(hipSetDevice(ctx->device));
        hipStream_t s = ctx->stream;
        GroupSide set;
        RPH_TRY(set.upload(hashes32, coeffs, has_features, quality, n, true, s));
        // Edge capacity: 32 per file to begin with (device memory is plentiful, 12 B each)
        std::vector<rph_edge> edges;
        rph_sweep q = set.sweep(similarity);
        RPH_TRY(sweep_growing("rph_group_files_pdq", std::max<uint64_t>(1u << 20, 32 * n), RPH_GROW_GROUP_FILES, s, edges,
                              [&](EdgeSink &sink, uint64_t cap) -> int {
                                  RPH_TRY(sink.open(cap, s, q));
                                  return rph_launch_hamming_sweep(ctx, q, s, ctx->hamming_kernel);
                              }));
        if (comparison_count_out) *comparison_count_out = edges.size();
        return rph_host_union_find(edges.data(), edges.size(), n, members, offsets, n_groups_out);
    });
}

// One sweep at `top`, its edges left on the device, then the merge tree of them (merge_tree.hip)
int rph_group_files_pdq_tree(rph_ctx *ctx, const uint8_t *hashes32, const float *coeffs, const uint8_t *has_features, const int32_t *quality, uint64_t n,
                             uint32_t top, uint32_t *into, uint8_t *level, uint64_t *edges_at)
{
    return rph_guarded("rph_group_files_pdq_tree", [&]() -> int {
        if (!ctx || (!hashes32 && n) || ((!into || !level) && n) || !edges_at) {
            rph_set_error("rph_group_files_pdq_tree: null argument");
            return RPH_ERR_INVALID_ARG;
        }
        RPH_TRY(check_similarity(top));
        if (n > 0x7FFFFFFFull) {
            rph_set_error("rph_group_files_pdq_tree: at most 2^31 - 1 files");
            return RPH_ERR_INVALID_ARG;
        }
        std::fill(edges_at, edges_at + top + 1, 0);
        if (n == 0) return RPH_OK;
        RPH_HIP_CHECK(hipSetDevice(ctx->device));
        hipStream_t s = ctx->stream;
        GroupSide set;
        EdgeSink sink;
        unsigned long long found = 0;
        if (n > 1) {
            RPH_TRY(set.upload(hashes32, coeffs, has_features, quality, n, true, s));
            rph_sweep q = set.sweep(top);
            RPH_TRY(sweep_growing_dev("rph_group_files_pdq_tree", std::max<uint64_t>(1u << 20, 32 * n), RPH_GROW_GROUP_FILES, s, sink, &found,
                                      [&](EdgeSink &k, uint64_t cap) -> int {
                                          RPH_TRY(k.open(cap, s, q));
                                          return rph_launch_hamming_sweep(ctx, q, s, ctx->hamming_kernel);
                                      }));
        }
        Layout L;
        const size_t o_into = L.add(n * 4, 256), o_level = L.add(n, 256), o_at = L.add((size_t)(top + 1) * 8, 256);
        DevBuf d_tree;
        RPH_TRY(d_tree.alloc(L.end()));
        StreamDrain drain{s};  // the tree's buffer and the sink's are in use until the stream is through
        uint8_t *t = d_tree.data();
        RPH_TRY(rph_merge_tree_run(ctx, sink.d_e.as<rph_edge>(), found, 0, 0, n, top, (uint32_t *)(t + o_into), t + o_level, (uint64_t *)(t + o_at), nullptr, s));
        RPH_HIP_CHECK(hipMemcpyAsync(into, t + o_into, n * 4, hipMemcpyDeviceToHost, s));
        RPH_HIP_CHECK(hipMemcpyAsync(level, t + o_level, n, hipMemcpyDeviceToHost, s));
        RPH_HIP_CHECK(hipMemcpyAsync(edges_at, t + o_at, (size_t)(top + 1) * 8, hipMemcpyDeviceToHost, s));
        RPH_HIP_CHECK(hipStreamSynchronize(s));
        return RPH_OK;
    });
}

int rph_union_find_groups_append(const uint32_t *old_members, const uint32_t *old_offsets, uint32_t n_old_groups, const rph_edge *edges,
                                 uint64_t n_edges, uint64_t n_total, uint32_t *members, uint32_t *offsets, uint32_t *n_groups_out)
{
    return rph_guarded("rph_union_find_groups_append", [&]() -> int {
        if ((!edges && n_edges) || ((!old_members || !old_offsets) && n_old_groups) || !members || !offsets || !n_groups_out) {
            rph_set_error("rph_union_find_groups_append: null argument");
            return RPH_ERR_INVALID_ARG;
        }
        return rph_host_union_find_append(old_members, old_offsets, n_old_groups, edges, n_edges, n_total, members, offsets, n_groups_out);
    });
}

int rph_group_files_pdq_append(rph_ctx *ctx, const uint8_t *old_hashes32, const float *old_coeffs, const uint8_t *old_has_features,
                               const int32_t *old_quality, uint64_t n_old, const uint32_t *old_members, const uint32_t *old_offsets,
                               uint32_t n_old_groups, const uint8_t *new_hashes32, const float *new_coeffs, const uint8_t *new_has_features,
                               const int32_t *new_quality, uint64_t n_new, uint32_t similarity, uint32_t *members, uint32_t *offsets,
                               uint32_t *n_groups_out, uint64_t *new_comparisons_out)
{
    return rph_guarded("rph_group_files_pdq_append", [&]() -> int {
        if (!ctx || (!old_hashes32 && n_old) || (!new_hashes32 && n_new) || ((!old_members || !old_offsets) && n_old_groups) || !members ||
            !offsets || !n_groups_out) {
            rph_set_error("rph_group_files_pdq_append: null argument");
            return RPH_ERR_INVALID_ARG;
        }
        RPH_TRY(check_similarity(similarity));
        const uint64_t n_total = n_old + n_new;
        if (n_total > 0xFFFFFFFFull) {
            rph_set_error("rph_group_files_pdq_append: %llu files, at most 2^32 - 1", (unsigned long long)n_total);
            return RPH_ERR_INVALID_ARG;
        }
        *n_groups_out = 0;
        offsets[0] = 0;
        if (new_comparisons_out) *new_comparisons_out = 0;
        std::vector<rph_edge> edges;
        if (n_new) {
            RPH_HIP_CHECK(hipSetDevice(ctx->device));
            hipStream_t s = ctx->stream;
            // group_files_generic tests the variants of the lower-indexed file against the hash of the higher one (scanner.rs:1716), and
            // the library comes first: the pairs the new files add are (library variants x new hashes), all of them, and
            // (new variants x new hashes, i < j).  The library's variants are only needed as rows; the new files are rows and columns.
            GroupSide lib, add;
            RPH_TRY(lib.upload(old_hashes32, old_coeffs, old_has_features, old_quality, n_old, true, s));
            RPH_TRY(add.upload(new_hashes32, new_coeffs, new_has_features, new_quality, n_new, n_new > 1, s));
            rph_sweep cross = lib.sweep(similarity, &add), within = add.sweep(similarity);
            unsigned long long n_cross = 0;
            RPH_TRY(sweep_growing("rph_group_files_pdq_append", std::max<uint64_t>(1u << 20, 32 * n_new), RPH_GROW_GROUP_FILES, s, edges,
                                  [&](EdgeSink &sink, uint64_t cap) -> int {
                                      RPH_TRY(sink.open(cap, s, cross));
                                      if (n_old) RPH_TRY(rph_launch_hamming_sweep(ctx, cross, s, ctx->hamming_kernel));
                                      RPH_TRY(sink.read(&n_cross, s));
                                      // the triangular sweep of the new files appends behind the cross edges (one cursor); its indices
                                      // are local to the new set
                                      within = into(within, cross.edges, cross.cap, cross.count);
                                      return rph_launch_hamming_sweep(ctx, within, s, ctx->hamming_kernel);
                                  }));
            for (uint64_t e = 0; e < edges.size(); e++) {  // to the numbering of the concatenation
                if (e >= n_cross) edges[e].i += (uint32_t)n_old;
                edges[e].j += (uint32_t)n_old;
            }
        }
        if (new_comparisons_out) *new_comparisons_out = edges.size();
        return rph_host_union_find_append(old_members, old_offsets, n_old_groups, edges.data(), edges.size(), n_total, members, offsets,
                                          n_groups_out);
    });
}

int rph_mih_build256(rph_ctx *ctx, const uint8_t *hashes32, uint64_t n, uint32_t *offsets, uint32_t *values)
{
    return rph_guarded("rph_mih_build256", [&]() -> int {
        if (!ctx || (!hashes32 && n) || !offsets || (!values && n)) {
            rph_set_error("rph_mih_build256: null argument");
            return RPH_ERR_INVALID_ARG;
        }
        RPH_HIP_CHECK(hipSetDevice(ctx->device));
        const size_t n_off = (size_t)16 * 65536 + 1;
        DevBuf d_h, d_o, d_v;
        RPH_TRY(d_h.alloc(n * 32));
        RPH_TRY(d_o.alloc(n_off * 4));
        RPH_TRY(d_v.alloc(n * 16 * 4));
        RPH_HIP_CHECK(hipMemcpyAsync(d_h.data(), hashes32, n * 32, hipMemcpyHostToDevice, ctx->stream));
        {
            std::lock_guard<std::mutex> lock(ctx->mu);
            RPH_TRY(rph_launch_mih_build256(ctx, (const uint8_t *)d_h.data(), n, (uint32_t *)d_o.data(), (uint32_t *)d_v.data(), ctx->stream));
        }
        RPH_HIP_CHECK(hipMemcpyAsync(offsets, d_o.data(), n_off * 4, hipMemcpyDeviceToHost, ctx->stream));
        if (n) RPH_HIP_CHECK(hipMemcpyAsync(values, d_v.data(), n * 16 * 4, hipMemcpyDeviceToHost, ctx->stream));
        RPH_HIP_CHECK(hipStreamSynchronize(ctx->stream));
        return RPH_OK;
    });
}

int rph_mih_build64(rph_ctx *ctx, const uint64_t *hashes64, uint64_t n, uint32_t *offsets, uint32_t *values)
{
    return rph_guarded("rph_mih_build64", [&]() -> int {
        if (!ctx || (!hashes64 && n) || !offsets || (!values && n)) {
            rph_set_error("rph_mih_build64: null argument");
            return RPH_ERR_INVALID_ARG;
        }
        RPH_HIP_CHECK(hipSetDevice(ctx->device));
        const size_t n_off = (size_t)8 * 256 + 1;
        DevBuf d_h, d_o, d_v;
        RPH_TRY(d_h.alloc(n * 8));
        RPH_TRY(d_o.alloc(n_off * 4));
        RPH_TRY(d_v.alloc(n * 8 * 4));
        std::lock_guard<std::mutex> lock(ctx->mu);
        RPH_HIP_CHECK(hipMemcpyAsync(d_h.data(), hashes64, n * 8, hipMemcpyHostToDevice, ctx->stream));
        RPH_TRY(rph_launch_mih_build64(ctx, (const uint64_t *)d_h.data(), n, (uint32_t *)d_o.data(), (uint32_t *)d_v.data(), ctx->stream));
        RPH_HIP_CHECK(hipMemcpyAsync(offsets, d_o.data(), n_off * 4, hipMemcpyDeviceToHost, ctx->stream));
        if (n) RPH_HIP_CHECK(hipMemcpyAsync(values, d_v.data(), n * 8 * 4, hipMemcpyDeviceToHost, ctx->stream));
        RPH_HIP_CHECK(hipStreamSynchronize(ctx->stream));
        return RPH_OK;
    });
}

// ------------------------------------------------------------------------------------------
// synthetic workloads, device memory helpers, events
// ------------------------------------------------------------------------------------------
int rph_synth_images_dev(rph_ctx *ctx, void *d_out, uint64_t first_k, uint32_t n, uint32_t w, uint32_t h, uint32_t seed,
                         void *stream)
{
    if (!ctx || (!d_out && n)) return RPH_ERR_INVALID_ARG;
    RPH_HIP_CHECK(hipSetDevice(ctx->device));
    return rph_launch_synth_images((uint8_t *)d_out, first_k, n, w, h, seed, pick(ctx, stream));
}

int rph_synth_hashes_dev(rph_ctx *ctx, void *d_out, uint64_t first, uint64_t count, uint64_t n_total, uint64_t seed,
                         uint64_t n_clusters, void *stream)
{
    if (!ctx || (!d_out && count)) return RPH_ERR_INVALID_ARG;
    RPH_HIP_CHECK(hipSetDevice(ctx->device));
    return rph_launch_synth_hashes((uint8_t *)d_out, first, count, n_total, seed, n_clusters, pick(ctx, stream));
}

int rph_read_stream_dev(rph_ctx *ctx, const void *d_buf, size_t bytes, void *stream)
{
    if (!ctx || !d_buf || ((uintptr_t)d_buf % 16) != 0) return RPH_ERR_INVALID_ARG;
    RPH_HIP_CHECK(hipSetDevice(ctx->device));
    std::lock_guard<std::mutex> lock(ctx->mu);
    if (!ctx->sink) RPH_HIP_CHECK(hipMalloc((void **)&ctx->sink, 16));
    return rph_launch_read_stream(d_buf, bytes, ctx->sink, pick(ctx, stream));
}

int rph_dev_alloc(rph_ctx *ctx, size_t bytes, void **out)
{
    if (!ctx || !out) return RPH_ERR_INVALID_ARG;
    RPH_HIP_CHECK(hipSetDevice(ctx->device));
    RPH_HIP_CHECK(hipMalloc(out, bytes ? bytes : 1));
    return RPH_OK;
}
int rph_dev_free(rph_ctx *ctx, void *p)
{
    if (!ctx) return RPH_ERR_INVALID_ARG;
    RPH_HIP_CHECK(hipSetDevice(ctx->device));
    if (p) RPH_HIP_CHECK(hipFree(p));
    return RPH_OK;
}
int rph_dev_upload(rph_ctx *ctx, void *d_dst, const void *src, size_t bytes)
{
    if (!ctx || ((!d_dst || !src) && bytes)) return RPH_ERR_INVALID_ARG;
    RPH_HIP_CHECK(hipSetDevice(ctx->device));
    RPH_HIP_CHECK(hipMemcpyAsync(d_dst, src, bytes, hipMemcpyHostToDevice, ctx->stream));
    RPH_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return RPH_OK;
}
int rph_dev_download(rph_ctx *ctx, void *dst, const void *d_src, size_t bytes)
{
    if (!ctx || ((!dst || !d_src) && bytes)) return RPH_ERR_INVALID_ARG;
    RPH_HIP_CHECK(hipSetDevice(ctx->device));
    RPH_HIP_CHECK(hipMemcpyAsync(dst, d_src, bytes, hipMemcpyDeviceToHost, ctx->stream));
    RPH_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return RPH_OK;
}
int rph_dev_memset(rph_ctx *ctx, void *d_dst, int value, size_t bytes, void *stream)
{
    if (!ctx || (!d_dst && bytes)) return RPH_ERR_INVALID_ARG;
    RPH_HIP_CHECK(hipSetDevice(ctx->device));
    RPH_HIP_CHECK(hipMemsetAsync(d_dst, value, bytes, pick(ctx, stream)));
    return RPH_OK;
}

int rph_stream_create(rph_ctx *ctx, void **stream_out)
{
    if (!ctx || !stream_out) return RPH_ERR_INVALID_ARG;
    RPH_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t s = nullptr;
    RPH_HIP_CHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    *stream_out = s;
    return RPH_OK;
}

int rph_stream_synchronize(rph_ctx *ctx, void *stream)
{
    if (!ctx) return RPH_ERR_INVALID_ARG;
    RPH_HIP_CHECK(hipSetDevice(ctx->device));
    RPH_HIP_CHECK(hipStreamSynchronize(pick(ctx, stream)));
    return RPH_OK;
}

int rph_stream_destroy(rph_ctx *ctx, void *stream)
{
    if (!ctx || !stream) return RPH_ERR_INVALID_ARG;
    RPH_HIP_CHECK(hipSetDevice(ctx->device));
    std::lock_guard<std::mutex> lock(ctx->mu);
    RPH_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
    for (SharedScratch *sc : {&ctx->scratch, &ctx->rz_scratch, &ctx->sweep_scratch, &ctx->b3_scratch}) sc->forget_stream((hipStream_t)stream);
    ctx->ll_scratch.erase((hipStream_t)stream);
    RPH_HIP_CHECK(hipStreamDestroy((hipStream_t)stream));
    return RPH_OK;
}

int rph_event_create(rph_ctx *ctx, void **event_out)
{
    if (!ctx || !event_out) return RPH_ERR_INVALID_ARG;
    RPH_HIP_CHECK(hipSetDevice(ctx->device));
    hipEvent_t e;
    RPH_HIP_CHECK(hipEventCreate(&e));
    *event_out = e;
    return RPH_OK;
}
int rph_event_record(rph_ctx *ctx, void *event, void *stream)
{
    if (!ctx || !event) return RPH_ERR_INVALID_ARG;
    RPH_HIP_CHECK(hipEventRecord((hipEvent_t)event, pick(ctx, stream)));
    return RPH_OK;
}
int rph_event_elapsed_ms(rph_ctx *ctx, void *start, void *stop, float *ms)
{
    if (!ctx || !start || !stop || !ms) return RPH_ERR_INVALID_ARG;
    RPH_HIP_CHECK(hipEventSynchronize((hipEvent_t)stop));
    RPH_HIP_CHECK(hipEventElapsedTime(ms, (hipEvent_t)start, (hipEvent_t)stop));
    return RPH_OK;
}
int rph_event_destroy(rph_ctx *ctx, void *event)
{
    if (!ctx || !event) return RPH_ERR_INVALID_ARG;
    RPH_HIP_CHECK(hipEventDestroy((hipEvent_t)event));
    return RPH_OK;
}

}  // extern "C"
