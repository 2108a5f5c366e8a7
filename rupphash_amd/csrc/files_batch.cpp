// files_batch.cpp -- rph_files_pdq_hash_batch: a mixed list of files in one call (include/rupphash.h, the files section).
// Host code around the six per-format batch entry points: every file is routed by rph_file_format (file_format.cpp), the files of one
// format form a lane, every lane is one call of its format's own entry point -- one after another on the calling thread, or with
// RPH_FILES_CONCURRENT each on a host thread of its own -- and the lanes' outputs are scattered back into the caller's order.  Nothing
// here touches the device: concurrent lanes meet in the pipelines' own locks (each takes its slot's mutex, then ctx->mu or image_mu where
// it uses shared scratch, rph_buffers.h); this call holds no lock while they run.
#include <chrono>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "rph_internal.h"

namespace {

constexpr int N_FORMATS = RPH_FORMAT_BMP + 1;  // index 0 (RPH_FORMAT_NONE) is no lane
const char *const FORMAT_NAME[N_FORMATS] = {"none", "jpeg", "png", "tiff", "webp", "gif", "bmp"};

// the files of one format and what its entry point returned for them, in lane order
struct Lane {
    int format = 0;
    std::vector<uint32_t> file;  // indices into the call
    std::vector<const uint8_t *> data;
    std::vector<size_t> len;
    uint64_t bytes = 0;
    uint32_t threads = 1;
    std::vector<uint8_t> hash, dihedral, valid, pixel;
    std::vector<float> quality, coeffs;
    std::vector<int32_t> status;
    int rc = RPH_OK;
    std::string err;  // the lane thread's rph_last_error(), carried out of the thread
    double wall_ms = 0;
};

// what the last call on this thread did, per format (rph_debug_files_lanes)
struct LaneLog {
    double wall_ms[N_FORMATS] = {};
    uint32_t threads[N_FORMATS] = {};
    uint32_t files[N_FORMATS] = {};
};
thread_local LaneLog g_lane_log;

// threads joined on every way out (a thread that cannot be started throws while the earlier lanes run)
struct Joined {
    std::vector<std::thread> th;
    ~Joined()
    {
        for (auto &t : th)
            if (t.joinable()) t.join();
    }
};

// The thread budget of the concurrent lanes: every lane one thread, the rest in proportion to the lanes' compressed bytes weighted by what
// a byte of the format costs the host threads in the default modes (tools/files_rate.py, DESIGN.md 4.12: PNG inflate, VP8L and GIF LZW
// decoding about 5 thread-ms per MB, TIFF LZW about 2, a JPEG's parse and destuffing 1 while its Huffman walk is the device's; a BMP's
// pixel array crosses PCIe as it is).  What is left of the division goes to the largest remainders, ties to the earlier format.  The
// shares sum to max(total, lanes)
constexpr uint64_t HOST_COST[N_FORMATS] = {0, 1, 5, 2, 5, 5, 0};

void deal_threads(std::vector<Lane> &lanes, uint32_t total)
{
    for (Lane &l : lanes) l.threads = 1;
    if (total <= lanes.size()) return;
    const uint64_t spare = total - lanes.size();
    std::vector<unsigned __int128> weight(lanes.size());
    unsigned __int128 all = 0;
    for (size_t k = 0; k < lanes.size(); k++) all += weight[k] = (unsigned __int128)lanes[k].bytes * HOST_COST[lanes[k].format];
    if (all == 0)  // (no lane with a weight: by bytes)
        for (size_t k = 0; k < lanes.size(); k++) all += weight[k] = lanes[k].bytes;
    uint64_t dealt = 0;
    std::vector<unsigned __int128> rem(lanes.size());
    for (size_t k = 0; k < lanes.size(); k++) {
        const unsigned __int128 share = weight[k] * spare;  // (bytes < 2^64, cost < 2^3, spare < 2^32: no overflow in 128 bits)
        lanes[k].threads += (uint32_t)(share / all);
        rem[k] = share % all;
        dealt += (uint64_t)(share / all);
    }
    for (; dealt < spare; dealt++) {
        size_t best = 0;
        for (size_t k = 1; k < lanes.size(); k++)
            if (rem[k] > rem[best]) best = k;
        lanes[best].threads++;
        rem[best] = 0;
    }
}

void run_lane(rph_ctx *ctx, Lane &l, int jpeg_flavour, bool want_quality, bool want_coeffs, bool want_dihedral, bool want_pixel)
{
    const auto t0 = std::chrono::steady_clock::now();
    const uint32_t m = (uint32_t)l.file.size();
    l.hash.assign((size_t)m * 32, 0);
    l.valid.assign(m, 0);
    l.status.assign(m, RPH_OK);
    if (want_quality) l.quality.assign(m, 0.0f);
    if (want_coeffs) l.coeffs.assign((size_t)m * 256, 0.0f);
    if (want_dihedral) l.dihedral.assign((size_t)m * 256, 0);
    if (want_pixel) l.pixel.assign((size_t)m * 32, 0);
    float *q = want_quality ? l.quality.data() : nullptr, *c = want_coeffs ? l.coeffs.data() : nullptr;
    uint8_t *d = want_dihedral ? l.dihedral.data() : nullptr, *p = want_pixel ? l.pixel.data() : nullptr;
    const uint8_t *const *data = l.data.data();
    const size_t *len = l.len.data();
    switch (l.format) {
    case RPH_FORMAT_JPEG:
        l.rc = want_pixel ? rph_jpeg_pdq_pixel_hash_batch(ctx, data, len, m, jpeg_flavour, l.threads, l.hash.data(), q, c, d, l.valid.data(), l.status.data(), p)
                          : rph_jpeg_pdq_hash_batch(ctx, data, len, m, jpeg_flavour, l.threads, l.hash.data(), q, c, d, l.valid.data(), l.status.data());
        // (a JPEG call of one file returns that file's status: not a failure of the call)
        if (m == 1 && l.rc == l.status[0] && (l.rc == RPH_ERR_INVALID_ARG || l.rc == RPH_ERR_UNSUPPORTED)) l.rc = RPH_OK;
        break;
    case RPH_FORMAT_PNG: l.rc = rph_png_pdq_hash_batch(ctx, data, len, m, l.threads, l.hash.data(), q, c, d, l.valid.data(), l.status.data(), p); break;
    case RPH_FORMAT_TIFF: l.rc = rph_tiff_pdq_hash_batch(ctx, data, len, m, l.threads, l.hash.data(), q, c, d, l.valid.data(), l.status.data(), p); break;
    case RPH_FORMAT_WEBP: l.rc = rph_webp_pdq_hash_batch(ctx, data, len, m, l.threads, l.hash.data(), q, c, d, l.valid.data(), l.status.data(), p); break;
    case RPH_FORMAT_GIF: l.rc = rph_gif_pdq_hash_batch(ctx, data, len, m, l.threads, l.hash.data(), q, c, d, l.valid.data(), l.status.data(), p); break;
    case RPH_FORMAT_BMP: l.rc = rph_bmp_pdq_hash_batch(ctx, data, len, m, l.threads, l.hash.data(), q, c, d, l.valid.data(), l.status.data(), p); break;
    default: l.rc = RPH_ERR_INVALID_ARG; break;
    }
    if (l.rc != RPH_OK) l.err = rph_last_error();
    l.wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// width and height of a file its pipeline decoded: what the format's _info reports
void file_size(int format, const uint8_t *data, size_t len, uint32_t *wh)
{
    uint32_t w = 0, h = 0, ch = 0;
    int rc = RPH_ERR_INVALID_ARG;
    switch (format) {
    case RPH_FORMAT_JPEG: rc = rph_jpeg_info(data, len, &w, &h, &ch); break;
    case RPH_FORMAT_PNG:
        // (rph_png_info would run the CRC over every IDAT byte a second time: 0.4 thread-ms per 512 x 512 photo on top of the 2.9 the
        // lane spends on it.  The lane's own parse accepted this file, so the IHDR's fields are the size rph_png_info reports)
        if (len >= 24) {
            auto be32 = [](const uint8_t *p) { return (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | (uint32_t)p[3]; };
            w = be32(data + 16), h = be32(data + 20), rc = RPH_OK;
        }
        break;
    case RPH_FORMAT_TIFF: rc = rph_tiff_info(data, len, &w, &h, nullptr, nullptr); break;
    case RPH_FORMAT_WEBP: rc = rph_webp_info(data, len, &w, &h, nullptr, nullptr); break;
    case RPH_FORMAT_GIF: rc = rph_gif_info(data, len, &w, &h, nullptr, nullptr); break;
    case RPH_FORMAT_BMP: rc = rph_bmp_info(data, len, &w, &h, nullptr, nullptr); break;
    }
    wh[0] = rc == RPH_OK ? w : 0;
    wh[1] = rc == RPH_OK ? h : 0;
}

}  // namespace

extern "C" {

// what the last rph_files_pdq_hash_batch on the calling thread did, per RPH_FORMAT_* (7 entries each; index 0 unused): a lane's wall
// time, its share of the threads and its files (exported for tools/files_rate.py and the tests, not in the header; any output may be null)
void rph_debug_files_lanes(double *wall_ms_out, uint32_t *threads_out, uint32_t *files_out)
{
    for (int f = 0; f < N_FORMATS; f++) {
        if (wall_ms_out) wall_ms_out[f] = g_lane_log.wall_ms[f];
        if (threads_out) threads_out[f] = g_lane_log.threads[f];
        if (files_out) files_out[f] = g_lane_log.files[f];
    }
}

int rph_files_pdq_hash_batch(rph_ctx *ctx, const uint8_t *const *data, const size_t *len, const char *const *names, uint32_t n, int jpeg_flavour,
                             uint32_t n_threads, uint32_t flags, uint8_t *hash32_out, float *quality_out, float *coeffs_out, uint8_t *dihedral_out,
                             uint8_t *valid_out, int32_t *status_out, uint8_t *pixel_hash32_out, uint8_t *format_out, uint32_t *size_out)
{
    return rph_guarded("rph_files_pdq_hash_batch", [&]() -> int {
        if (!ctx || (n && (!data || !len || !hash32_out)) || (flags & ~(RPH_FILES_SEQUENTIAL | RPH_FILES_CONCURRENT)) ||
            flags == (RPH_FILES_SEQUENTIAL | RPH_FILES_CONCURRENT)) {
            rph_set_error("rph_files_pdq_hash_batch: null argument or unknown flag");
            return RPH_ERR_INVALID_ARG;
        }
        g_lane_log = LaneLog();
        if (n == 0) return RPH_OK;
        memset(hash32_out, 0, (size_t)n * 32);
        if (quality_out) memset(quality_out, 0, (size_t)n * 4);
        if (coeffs_out) memset(coeffs_out, 0, (size_t)n * 1024);
        if (dihedral_out) memset(dihedral_out, 0, (size_t)n * 256);
        if (valid_out) memset(valid_out, 0, n);
        if (pixel_hash32_out) memset(pixel_hash32_out, 0, (size_t)n * 32);
        if (format_out) memset(format_out, 0, n);
        if (size_out) memset(size_out, 0, (size_t)n * 8);
        // ---- route
        std::vector<uint8_t> format(n);
        for (uint32_t i = 0; i < n; i++) {
            const bool there = data[i] && len[i];
            format[i] = there ? (uint8_t)rph_file_format(data[i], len[i], names ? names[i] : nullptr) : (uint8_t)RPH_FORMAT_NONE;
            if (status_out) status_out[i] = !there ? RPH_ERR_INVALID_ARG : (format[i] == RPH_FORMAT_NONE ? RPH_ERR_UNSUPPORTED : RPH_OK);
        }
        uint32_t count[N_FORMATS] = {};
        for (uint32_t i = 0; i < n; i++) count[format[i]]++;
        std::vector<Lane> lanes;
        int lane_of[N_FORMATS];
        for (int f = RPH_FORMAT_JPEG; f < N_FORMATS; f++) {
            lane_of[f] = -1;
            if (!count[f]) continue;
            lane_of[f] = (int)lanes.size();
            lanes.emplace_back();
            Lane &l = lanes.back();
            l.format = f;
            l.file.reserve(count[f]), l.data.reserve(count[f]), l.len.reserve(count[f]);
        }
        std::vector<uint32_t> pos(n);  // a file's place in its lane
        for (uint32_t i = 0; i < n; i++) {
            if (format[i] == RPH_FORMAT_NONE) continue;
            Lane &l = lanes[lane_of[format[i]]];
            pos[i] = (uint32_t)l.file.size();
            l.file.push_back(i), l.data.push_back(data[i]), l.len.push_back(len[i]);
            l.bytes += len[i];
        }
        if (lanes.empty()) return RPH_OK;
        // ---- run: the lanes side by side, or one after another with every thread
        const uint32_t total = n_threads ? n_threads : rph_host_threads();
        const bool sequential = !(flags & RPH_FILES_CONCURRENT) || lanes.size() == 1;  // (the default: DESIGN.md 4.12 has the measurement)
        auto run = [&](Lane &l) { run_lane(ctx, l, jpeg_flavour, quality_out != nullptr, coeffs_out != nullptr, dihedral_out != nullptr, pixel_hash32_out != nullptr); };
        if (sequential) {
            for (Lane &l : lanes) {
                l.threads = total;
                run(l);
            }
        } else {
            deal_threads(lanes, total);
            Joined j;
            for (size_t k = 1; k < lanes.size(); k++) j.th.emplace_back([&, k] { run(lanes[k]); });
            run(lanes[0]);  // (the calling thread is the first lane's)
        }
        for (const Lane &l : lanes) {
            g_lane_log.wall_ms[l.format] = l.wall_ms;
            g_lane_log.threads[l.format] = l.threads;
            g_lane_log.files[l.format] = (uint32_t)l.file.size();
        }
        for (const Lane &l : lanes)
            if (l.rc != RPH_OK) {
                rph_set_error("rph_files_pdq_hash_batch (%s lane): %s", FORMAT_NAME[l.format], l.err.c_str());
                return l.rc;
            }
        // ---- scatter into the caller's order, and the sizes (the _info calls of a few thousand files are milliseconds on one thread)
        parallel_for(0, n, n >= 256 ? total : 1, [&](size_t i) {
            if (format[i] == RPH_FORMAT_NONE) return;
            const Lane &l = lanes[lane_of[format[i]]];
            const size_t k = pos[i];
            memcpy(hash32_out + i * 32, &l.hash[k * 32], 32);
            if (quality_out) quality_out[i] = l.quality[k];
            if (coeffs_out) memcpy(coeffs_out + i * 256, &l.coeffs[k * 256], 1024);
            if (dihedral_out) memcpy(dihedral_out + i * 256, &l.dihedral[k * 256], 256);
            if (valid_out) valid_out[i] = l.valid[k];
            if (status_out) status_out[i] = l.status[k];
            if (pixel_hash32_out) memcpy(pixel_hash32_out + i * 32, &l.pixel[k * 32], 32);
            if (format_out) format_out[i] = format[i];
            if (size_out && l.status[k] == RPH_OK) file_size(l.format, data[i], len[i], size_out + i * 2);
        });
        return RPH_OK;
    });
}

}  // extern "C"
