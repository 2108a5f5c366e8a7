// gif_pipeline.cpp -- GIF files -> PDQ hashes and pixel hashes (include/rupphash.h, GIF section).
//
// The host threads parse every file up to the end of its first frame's data (gif_host.cpp) and either join that frame's sub-blocks
// into one contiguous stream in pinned staging (DEVICE: the compressed bytes cross PCIe; one wave per file runs the LZW decoder,
// gif_kernels.hip) or decode the joined stream themselves with the same gif_lzw.h (HOST: the palette indices cross PCIe).  Everything
// after that runs on the device: one expand kernel (interlacing, palette, placement on the logical screen, alpha), then the pixel
// hashes and PDQ over runs of equal geometry (decoded_hash.h, shared with the PNG, TIFF and WebP paths).
// A call is processed in chunks whose buffers are kept in the context between calls (rph_gif_release returns them).
#include <string.h>

#include <algorithm>
#include <vector>

#include "file_pipeline.h"
#include "gif_host.h"
#include "rph_internal.h"

int rph_gif_launch_lzw(const uint8_t *d_comp, const void *d_images, uint32_t n, uint8_t *d_dec, int32_t *d_status, hipStream_t s);
int rph_gif_launch_expand(const uint8_t *d_dec, const void *d_images, const uint32_t *d_pals, const uint32_t *d_list, uint32_t n, uint32_t max_rows,
                          uint8_t *d_hp, uint8_t *d_nat, hipStream_t s);

namespace {

struct GifPipe : FilePipeBase {
    DevBuf comp, dec, meta, status;
    PinnedBuf h_comp, h_dec, h_meta, h_status;
    HashStageBufs hash;
};

// AUTO: the device would decode a chunk whose palette indices are at least this many times its joined streams' bytes, the host threads
// the rest.  The ratio is what the host knows before it decodes anything.  Measured (DESIGN.md 4.10,
// profiles/gif_rate.txt): the device beats 16 host threads on no corpus: dithered photographs at 1.2:1 (4.1 vs 13.6 GB/s of pixels),
// 512x512 screenshots at 94:1 (86.8 vs 85.1: a tie), 1920x1080 screenshots at 62:1 (15.6 vs 81.7; 96 files are 96 waves) and flat
// graphics at 164:1 (24.4 vs 100.6).  So there is no threshold, and AUTO is HOST
constexpr uint64_t AUTO_DEVICE_MIN_RATIO = 0;  // 0: AUTO never chooses the device

// one chunk: files[idx[k]] for k in [0, m), all parsed RPH_OK
int run_chunk(rph_ctx *ctx, GifPipe &P, const uint8_t *const *data, std::vector<rphg::Parsed> &parsed, const uint32_t *idx, size_t m, unsigned threads,
              const FileOutputs &out)
{
    hipStream_t s = P.s;
    auto reserve = [s](auto &buf, size_t bytes) { return reserve_slack(buf, bytes, s); };
    // placement of the streams in staging (4-byte aligned), of the frames' indices in the decoded buffer (slots of whole 16 bytes) and
    // of the palettes in the metadata
    uint64_t dec_bytes = 0, comp_bytes = 0, index_bytes = 0, stream_bytes = 0;
    uint32_t pal_words = 0, max_rows = 0;
    for (size_t k = 0; k < m; k++) {
        rphg::Parsed &pp = parsed[idx[k]];
        pp.im.dec_off = dec_bytes;
        dec_bytes += align_up((uint64_t)pp.im.fw * pp.im.fh, 16);
        pp.im.comp_off = comp_bytes;
        comp_bytes += align_up(pp.stream_len, 4);
        pp.im.pal_off = pal_words;
        pal_words += pp.im.pal_n;
        index_bytes += (uint64_t)pp.im.fw * pp.im.fh;
        stream_bytes += pp.stream_len;
        max_rows = std::max(max_rows, pp.im.h);
    }
    int mode = ctx->file[RPH_FILE_GIF].mode;
    if (mode == RPH_GIF_DECOMPRESS_AUTO)
        mode = AUTO_DEVICE_MIN_RATIO && index_bytes >= AUTO_DEVICE_MIN_RATIO * stream_bytes ? RPH_GIF_DECOMPRESS_DEVICE : RPH_GIF_DECOMPRESS_HOST;
    const bool device = mode == RPH_GIF_DECOMPRESS_DEVICE;
    Layout L;
    const size_t off_img = L.add(m * sizeof(rphg::Image)), off_pal = L.add((size_t)pal_words * 4, 256), off_list = L.add(m * 4, 256),
                 off_b3 = L.add((m + 1) * 8, 256), meta_bytes = L.end();
    RPH_TRY(reserve(P.meta, meta_bytes));
    RPH_TRY(reserve(P.h_meta, meta_bytes));
    RPH_TRY(reserve(P.dec, dec_bytes));
    RPH_TRY(reserve(P.status, m * 4));
    RPH_TRY(reserve(P.h_status, m * 4));
    uint8_t *M = P.h_meta.data();
    rphg::Image *imgs = reinterpret_cast<rphg::Image *>(M + off_img);
    uint32_t *pals = reinterpret_cast<uint32_t *>(M + off_pal), *list = reinterpret_cast<uint32_t *>(M + off_list);
    int32_t *st = reinterpret_cast<int32_t *>(P.h_status.data());
    for (size_t k = 0; k < m; k++) {
        const rphg::Parsed &pp = parsed[idx[k]];
        imgs[k] = pp.im;
        memcpy(pals + pp.im.pal_off, pp.pal, (size_t)pp.im.pal_n * 4);
        st[k] = RPH_OK;
    }
    if (device) {
        RPH_TRY(reserve(P.comp, comp_bytes + 64));
        RPH_TRY(reserve(P.h_comp, comp_bytes + 64));
        parallel_for(0, m, threads, [&](size_t k) { rphg::join(data[idx[k]], parsed[idx[k]], P.h_comp.data() + imgs[k].comp_off); });
        RPH_HIP_CHECK(hipMemcpyAsync(P.meta.data(), M, meta_bytes, hipMemcpyHostToDevice, s));
        RPH_HIP_CHECK(hipMemcpyAsync(P.comp.data(), P.h_comp.data(), comp_bytes, hipMemcpyHostToDevice, s));
        RPH_HIP_CHECK(hipMemcpyAsync(P.status.data(), st, m * 4, hipMemcpyHostToDevice, s));
        RPH_TRY(rph_gif_launch_lzw(P.comp.data(), P.meta.data() + off_img, (uint32_t)m, P.dec.data(), P.status.as<int32_t>(), s));
        RPH_HIP_CHECK(hipMemcpyAsync(st, P.status.data(), m * 4, hipMemcpyDeviceToHost, s));
        RPH_HIP_CHECK(hipStreamSynchronize(s));
    } else {
        RPH_TRY(reserve(P.h_dec, dec_bytes));
        parallel_for(0, m, threads, [&](size_t k) {
            const rphg::Parsed &pp = parsed[idx[k]];
            std::vector<uint8_t> stream(pp.stream_len);
            rphg::join(data[idx[k]], pp, stream.data());
            if (!rphg::decode_indices_host(stream.data(), stream.size(), imgs[k], P.h_dec.data() + imgs[k].dec_off)) st[k] = RPH_ERR_INVALID_ARG;
        });
        RPH_HIP_CHECK(hipMemcpyAsync(P.dec.data(), P.h_dec.data(), dec_bytes, hipMemcpyHostToDevice, s));
    }
    return hash_decoded_images(ctx, s, P.hash, imgs, list, reinterpret_cast<uint64_t *>(M + off_b3), P.meta.data() + off_b3, st, idx, m, out,
                               [&](uint32_t g, uint64_t, bool want_hp, uint64_t, uint64_t nat_bytes) -> int {
                                   RPH_HIP_CHECK(hipMemcpyAsync(P.meta.data(), M, meta_bytes, hipMemcpyHostToDevice, s));
                                   return rph_gif_launch_expand(P.dec.data(), P.meta.data() + off_img, (const uint32_t *)(P.meta.data() + off_pal),
                                                                (const uint32_t *)(P.meta.data() + off_list), g, max_rows, want_hp ? P.hash.hp.data() : nullptr,
                                                                nat_bytes ? P.hash.nat.data() : nullptr, s);
                               });
}

int run(rph_ctx *ctx, const uint8_t *const *data, const size_t *len, uint32_t n, unsigned threads, const FileOutputs &out)
{
    return with_file_pipe<GifPipe>(ctx, RPH_FILE_GIF, threads, [&](GifPipe &P, rph_file_slot &slot, unsigned threads) -> int {
        std::vector<rphg::Parsed> parsed(n);
        const std::vector<uint32_t> ok = parse_files(data, len, n, threads, out.status, slot.log, [&](size_t i) { return rphg::parse(data[i], len[i], parsed[i]); });
        const rph_file_limits &lim = ctx->file_limits;
        for (size_t a = 0; a < ok.size();) {
            const size_t b = chunk_end<3>(ok, a, lim.files, {lim.comp, lim.raw, lim.pixels / 2}, [&](uint32_t i) -> std::array<uint64_t, 3> {
                const rphg::Parsed &p = parsed[i];
                return {p.stream_len, (uint64_t)p.im.fw * p.im.fh, (uint64_t)p.im.w * p.im.h};  // (pixels / 2: 4 bytes per pixel)
            });
            slot.log.sizes.push_back((uint32_t)(b - a));
            RPH_TRY(run_chunk(ctx, P, data, parsed, ok.data() + a, b - a, threads, out));
            a = b;
        }
        return RPH_OK;
    });
}

}  // namespace

void rph_gif_forget(rph_ctx *ctx) { forget_file_pipe<GifPipe>(ctx, RPH_FILE_GIF); }

extern "C" {

int rph_gif_info(const uint8_t *data, size_t len, uint32_t *w, uint32_t *h, uint32_t *channels, uint32_t *bit_depth)
{
    return rph_guarded("rph_gif_info", [&] { return file_info<rphg::Parsed>(data, len, w, h, channels, bit_depth, rphg::parse, image_out_depth); });
}

int rph_gif_decode_host(const uint8_t *data, size_t len, void *pixels_out, size_t cap_bytes)
{
    return rph_guarded("rph_gif_decode_host",
                       [&] { return file_decode_host<rphg::Parsed>("rph_gif_decode_host", data, len, pixels_out, cap_bytes, rphg::decode_host); });
}

int rph_gif_decode(rph_ctx *ctx, const uint8_t *data, size_t len, void *pixels_out, size_t cap_bytes)
{
    return rph_guarded("rph_gif_decode", [&] {
        return file_decode<rphg::Parsed>(
            "rph_gif_decode", ctx, data, len, pixels_out, cap_bytes, rphg::parse,
            [](const rphg::Image &im) { return (size_t)im.w * im.h * 4; }, [&](const FileOutputs &o) { return run(ctx, &data, &len, 1, 0, o); });
    });
}

int rph_gif_pdq_hash_batch(rph_ctx *ctx, const uint8_t *const *data, const size_t *len, uint32_t n, uint32_t n_threads, uint8_t *hash32_out,
                           float *quality_out, float *coeffs_out, uint8_t *dihedral_out, uint8_t *valid_out, int32_t *status_out,
                           uint8_t *pixel_hash32_out)
{
    return rph_guarded("rph_gif_pdq_hash_batch", [&] {
        return file_hash_batch("rph_gif_pdq_hash_batch", ctx, data, len, n, hash32_out, quality_out, coeffs_out, dihedral_out, valid_out, status_out, pixel_hash32_out,
                               [&](const FileOutputs &o) { return run(ctx, data, len, n, n_threads, o); });
    });
}

int rph_gif_set_decompress(rph_ctx *ctx, int where) { return file_set_mode(ctx, RPH_FILE_GIF, where, RPH_GIF_DECOMPRESS_HOST, RPH_GIF_DECOMPRESS_AUTO); }

int rph_gif_release(rph_ctx *ctx) { return file_release(ctx, RPH_FILE_GIF, rph_gif_forget); }

}  // extern "C"
