// webp_pipeline.cpp -- lossless WebP files -> PDQ hashes and pixel hashes (include/rupphash.h, WebP section).
//
// The host threads parse the container and read the serial front of every VP8L stream (webp_host.cpp): transforms with their sub-images,
// colour table, entropy image, the prefix codes of every group, built into lookup tables.  The built tables cross PCIe rather than the
// code lengths: the host has to build them anyway to apply the rule's checks to every code, so the kernel starts on the pixels at once
// and holds no table-building code.  Then either the VP8L chunk's bytes are copied into pinned staging (DEVICE: the compressed bytes
// cross; one wave per stream decodes the main ARGB image, webp_kernels.hip) or the host threads decode it themselves with the same
// vp8l.h (HOST: the ARGB residuals cross).  Everything after that runs on the device: the inverse transforms, last read first, one
// expand kernel, then the pixel hashes and PDQ over runs of equal geometry (decoded_hash.h, shared with the PNG and TIFF paths).
// A call is processed in chunks whose buffers are kept in the context between calls (rph_webp_release returns them).
#include <string.h>

#include <algorithm>
#include <atomic>
#include <vector>

#include "file_pipeline.h"
#include "rph_internal.h"
#include "webp_host.h"

int rph_webp_launch_entropy(const uint8_t *d_comp, const void *d_images, const void *d_codes, uint32_t n, uint32_t *d_argb, int32_t *d_status, hipStream_t s);
int rph_webp_launch_finish(const void *d_images, const uint32_t *d_list, uint32_t n, uint32_t levels, uint64_t max_pixels, const uint32_t *d_words, uint32_t *d_argb,
                           uint8_t *d_hp, uint8_t *d_nat, hipStream_t s);

namespace {

struct WebpPipe : FilePipeBase {
    DevBuf comp, argb, words, codes, meta, status;
    PinnedBuf h_comp, h_argb, h_words, h_codes, h_meta, h_status;
    HashStageBufs hash;
};

// AUTO: the device would decode a chunk whose ARGB bytes are at least this many times its compressed bytes (both unpadded), the host
// threads the rest.  The ratio is what the host knows before it decodes anything, in both modes; the share of pixels that come from
// backward references would say more but is known only after a HOST-mode decode.  Measured (profiles/webp_rate.txt):
// the device loses to 16 host threads at every ratio tried: photographs at 2:1 (1.23 vs 2.99 GB/s of pixels), palette images at 11:1
// (1.21 vs 1.55), screenshots at 2700:1 (14.9 vs 22.6).  So there is no threshold, and AUTO is HOST
constexpr uint64_t AUTO_DEVICE_MIN_RATIO = 0;  // 0: AUTO never chooses the device
// tables (and sub-images) a parsed file holds: bounded per window and per chunk (ctx->file_limits.webp_window_tables, webp_chunk_tables)
inline uint64_t table_bytes(const rphw::Parsed &p) { return p.codes.size() * 2 + p.words.size() * 4; }

// a stream's bytes in staging: zero bytes behind them for the dwords the bit reader loads past the end before the count of consumed
// bits stops it (at most 58 bits of one symbol group + 64 buffered + the dword loaded ahead)
inline uint64_t staged_bytes(const rphw::Parsed &p) { return align_up(p.chunk_len, 4) + 32; }
inline bool has_palette(const rphw::Image &im)
{
    for (uint32_t k = 0; k < im.n_tr; k++)
        if (im.tr[k].type == rphw::TR_COLOUR_INDEXING) return true;
    return false;
}

// one chunk: files[idx[k]] for k in [0, m), all parsed RPH_OK
int run_chunk(rph_ctx *ctx, WebpPipe &P, std::vector<rphw::Parsed> &parsed, const uint32_t *idx, size_t m, unsigned threads, const FileOutputs &out)
{
    hipStream_t s = P.s;
    auto reserve = [s](auto &buf, size_t bytes) { return reserve_slack(buf, bytes, s); };
    // placement: coded ARGB images first (the part a HOST-mode chunk uploads), the unbundled images of palette files behind them
    uint64_t a_words = 0, b_words = 0, comp_bytes = 0, n_words = 0, n_codes = 0, argb_bytes = 0, chunk_bytes = 0;
    uint32_t levels = 0;
    std::vector<uint64_t> word_base(m), code_base(m), comp_base(m);
    for (size_t k = 0; k < m; k++) {
        rphw::Parsed &pp = parsed[idx[k]];
        pp.im.a_off = a_words;
        a_words += align_up((uint64_t)pp.im.xw * pp.im.h, 16);
        word_base[k] = n_words;
        n_words += align_up(pp.words.size(), 4);
        code_base[k] = n_codes;
        n_codes += align_up(pp.codes.size(), 8);
        comp_base[k] = comp_bytes;
        comp_bytes += staged_bytes(pp);
        argb_bytes += (uint64_t)pp.im.xw * pp.im.h * 4;
        chunk_bytes += pp.chunk_len;
        levels = std::max<uint32_t>(levels, pp.im.n_tr);
    }
    for (size_t k = 0; k < m; k++) {
        rphw::Parsed &pp = parsed[idx[k]];
        if (!has_palette(pp.im)) continue;
        pp.im.b_off = a_words + b_words;
        b_words += align_up((uint64_t)pp.im.w * pp.im.h, 16);
    }
    int mode = ctx->file[RPH_FILE_WEBP].mode;
    if (mode == RPH_WEBP_ENTROPY_AUTO) mode = AUTO_DEVICE_MIN_RATIO && argb_bytes >= AUTO_DEVICE_MIN_RATIO * chunk_bytes ? RPH_WEBP_ENTROPY_DEVICE : RPH_WEBP_ENTROPY_HOST;
    const bool device = mode == RPH_WEBP_ENTROPY_DEVICE;
    Layout L;
    const size_t off_img = L.add(m * sizeof(rphw::Image)), off_list = L.add(m * 4, 256), off_b3 = L.add((m + 1) * 8, 256), meta_bytes = L.end();
    RPH_TRY(reserve(P.meta, meta_bytes));
    RPH_TRY(reserve(P.h_meta, meta_bytes));
    RPH_TRY(reserve(P.argb, (a_words + b_words) * 4));
    RPH_TRY(reserve(P.words, n_words * 4));
    RPH_TRY(reserve(P.h_words, n_words * 4));
    RPH_TRY(reserve(P.status, m * 4));
    RPH_TRY(reserve(P.h_status, m * 4));
    uint8_t *M = P.h_meta.data();
    rphw::Image *imgs = reinterpret_cast<rphw::Image *>(M + off_img);
    uint32_t *list = reinterpret_cast<uint32_t *>(M + off_list);
    int32_t *st = reinterpret_cast<int32_t *>(P.h_status.data());
    uint32_t *h_words = P.h_words.as<uint32_t>();
    for (size_t k = 0; k < m; k++) {
        const rphw::Parsed &pp = parsed[idx[k]];
        imgs[k] = pp.im;
        for (uint32_t q = 0; q < imgs[k].n_tr; q++) imgs[k].tr[q].off += (uint32_t)word_base[k];
        imgs[k].ent_off += code_base[k];
        imgs[k].tab_off += code_base[k];
        imgs[k].comp_off = comp_base[k];
        imgs[k].comp_len = pp.chunk_len;
        st[k] = RPH_OK;
        if (!pp.words.empty()) memcpy(h_words + word_base[k], pp.words.data(), pp.words.size() * 4);
    }
    RPH_HIP_CHECK(hipMemcpyAsync(P.meta.data(), M, meta_bytes, hipMemcpyHostToDevice, s));
    RPH_HIP_CHECK(hipMemcpyAsync(P.words.data(), h_words, n_words * 4, hipMemcpyHostToDevice, s));
    if (device) {
        RPH_TRY(reserve(P.comp, comp_bytes));
        RPH_TRY(reserve(P.h_comp, comp_bytes));
        RPH_TRY(reserve(P.codes, n_codes * 2));
        RPH_TRY(reserve(P.h_codes, n_codes * 2));
        uint16_t *h_codes = P.h_codes.as<uint16_t>();
        parallel_for(0, m, threads, [&](size_t k) {
            const rphw::Parsed &pp = parsed[idx[k]];
            uint8_t *d = P.h_comp.data() + comp_base[k];
            memcpy(d, pp.chunk, pp.chunk_len);
            memset(d + pp.chunk_len, 0, staged_bytes(pp) - pp.chunk_len);
            memcpy(h_codes + code_base[k], pp.codes.data(), pp.codes.size() * 2);
        });
        RPH_HIP_CHECK(hipMemcpyAsync(P.comp.data(), P.h_comp.data(), comp_bytes, hipMemcpyHostToDevice, s));
        RPH_HIP_CHECK(hipMemcpyAsync(P.codes.data(), h_codes, n_codes * 2, hipMemcpyHostToDevice, s));
        RPH_HIP_CHECK(hipMemcpyAsync(P.status.data(), st, m * 4, hipMemcpyHostToDevice, s));
        RPH_TRY(rph_webp_launch_entropy(P.comp.data(), P.meta.data() + off_img, P.codes.data(), (uint32_t)m, P.argb.as<uint32_t>(), P.status.as<int32_t>(), s));
        RPH_HIP_CHECK(hipMemcpyAsync(st, P.status.data(), m * 4, hipMemcpyDeviceToHost, s));
        RPH_HIP_CHECK(hipStreamSynchronize(s));
    } else {
        RPH_TRY(reserve(P.h_argb, a_words * 4));
        uint32_t *h_argb = P.h_argb.as<uint32_t>();
        parallel_for(0, m, threads, [&](size_t k) {
            if (!rphw::decode_main_host(parsed[idx[k]], h_argb + imgs[k].a_off)) st[k] = RPH_ERR_INVALID_ARG;
        });
        RPH_HIP_CHECK(hipMemcpyAsync(P.argb.data(), h_argb, a_words * 4, hipMemcpyHostToDevice, s));
    }
    return hash_decoded_images(ctx, s, P.hash, imgs, list, reinterpret_cast<uint64_t *>(M + off_b3), P.meta.data() + off_b3, st, idx, m, out,
                               [&](uint32_t g, uint64_t max_px, bool want_hp, uint64_t, uint64_t nat_bytes) -> int {
                                   RPH_HIP_CHECK(hipMemcpyAsync(P.meta.data(), M, meta_bytes, hipMemcpyHostToDevice, s));
                                   return rph_webp_launch_finish(P.meta.data() + off_img, (const uint32_t *)(P.meta.data() + off_list), g, levels, max_px,
                                                                 P.words.as<uint32_t>(), P.argb.as<uint32_t>(), want_hp ? P.hash.hp.data() : nullptr,
                                                                 nat_bytes ? P.hash.nat.data() : nullptr, s);
                               });
}

int run(rph_ctx *ctx, const uint8_t *const *data, const size_t *len, uint32_t n, unsigned threads, const FileOutputs &out)
{
    return with_file_pipe<WebpPipe>(ctx, RPH_FILE_WEBP, threads, [&](WebpPipe &P, rph_file_slot &slot, unsigned threads) -> int {
        // The fronts of a window of files at a time: their tables are the bulk of what a parsed file holds.  A window ends early at the
        // first file that finds the window's tables above their bound (files behind it that were parsed meanwhile are parsed again in the
        // next one)
        std::vector<rphw::Parsed> parsed(n);
        const rph_file_limits &lim = ctx->file_limits;
        rph_file_chunk_log &log = slot.log;
        log = rph_file_chunk_log();
        for (uint32_t a = 0; a < n;) {
            uint32_t b = (uint32_t)std::min<uint64_t>(n, (uint64_t)a + lim.files);
            std::atomic<uint64_t> held{0};
            std::atomic<uint32_t> deferred{b};
            log.n_windows++;
            parallel_for(a, b, threads, [&](size_t i) {
                if (i > a && (held.load() > lim.webp_window_tables || i > deferred.load())) {
                    uint32_t d = deferred.load();
                    while ((uint32_t)i < d && !deferred.compare_exchange_weak(d, (uint32_t)i)) {}
                    return;
                }
                out.status[i] = (data[i] && len[i]) ? rphw::front(data[i], len[i], parsed[i]) : RPH_ERR_INVALID_ARG;
                held += table_bytes(parsed[i]);
            });
            for (uint32_t i = deferred.load(); i < b; i++) parsed[i] = rphw::Parsed();
            b = deferred.load();
            const std::vector<uint32_t> ok = ok_files(out.status, a, b);
            for (size_t c = 0; c < ok.size();) {  // (no file bound: the window is one)
                const size_t e = chunk_end<3>(ok, c, UINT64_MAX, {lim.comp, lim.pixels / 2, lim.webp_chunk_tables}, [&](uint32_t i) -> std::array<uint64_t, 3> {
                    const rphw::Parsed &p = parsed[i];
                    return {p.chunk_len, (uint64_t)p.im.w * p.im.h, table_bytes(p)};
                });
                log.sizes.push_back((uint32_t)(e - c));
                RPH_TRY(run_chunk(ctx, P, parsed, ok.data() + c, e - c, threads, out));
                c = e;
            }
            for (uint32_t i = a; i < b; i++) parsed[i] = rphw::Parsed();
            a = b;
        }
        return RPH_OK;
    });
}

}  // namespace

void rph_webp_forget(rph_ctx *ctx) { forget_file_pipe<WebpPipe>(ctx, RPH_FILE_WEBP); }

extern "C" {

int rph_webp_info(const uint8_t *data, size_t len, uint32_t *w, uint32_t *h, uint32_t *channels, uint32_t *bit_depth)
{
    return rph_guarded("rph_webp_info", [&] { return file_info<rphw::Parsed>(data, len, w, h, channels, bit_depth, rphw::parse, image_out_depth); });
}

int rph_webp_decode_host(const uint8_t *data, size_t len, void *pixels_out, size_t cap_bytes)
{
    return rph_guarded("rph_webp_decode_host",
                       [&] { return file_decode_host<rphw::Parsed>("rph_webp_decode_host", data, len, pixels_out, cap_bytes, rphw::decode_host); });
}

int rph_webp_decode(rph_ctx *ctx, const uint8_t *data, size_t len, void *pixels_out, size_t cap_bytes)
{
    return rph_guarded("rph_webp_decode", [&] {
        return file_decode<rphw::Parsed>(
            "rph_webp_decode", ctx, data, len, pixels_out, cap_bytes, rphw::parse,
            [](const rphw::Image &im) { return (size_t)im.w * im.h * im.out_ch; }, [&](const FileOutputs &o) { return run(ctx, &data, &len, 1, 0, o); });
    });
}

int rph_webp_pdq_hash_batch(rph_ctx *ctx, const uint8_t *const *data, const size_t *len, uint32_t n, uint32_t n_threads, uint8_t *hash32_out,
                            float *quality_out, float *coeffs_out, uint8_t *dihedral_out, uint8_t *valid_out, int32_t *status_out,
                            uint8_t *pixel_hash32_out)
{
    return rph_guarded("rph_webp_pdq_hash_batch", [&] {
        return file_hash_batch("rph_webp_pdq_hash_batch", ctx, data, len, n, hash32_out, quality_out, coeffs_out, dihedral_out, valid_out, status_out, pixel_hash32_out,
                               [&](const FileOutputs &o) { return run(ctx, data, len, n, n_threads, o); });
    });
}

int rph_webp_set_entropy(rph_ctx *ctx, int where) { return file_set_mode(ctx, RPH_FILE_WEBP, where, RPH_WEBP_ENTROPY_HOST, RPH_WEBP_ENTROPY_AUTO); }

int rph_webp_release(rph_ctx *ctx) { return file_release(ctx, RPH_FILE_WEBP, rph_webp_forget); }

}  // extern "C"
