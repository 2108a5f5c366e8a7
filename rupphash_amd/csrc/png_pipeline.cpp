// png_pipeline.cpp -- PNG files -> PDQ hashes and pixel hashes (include/rupphash.h, PNG section).
//
// The host threads parse the chunks (png_host.cpp) and either gather the IDAT payloads into pinned staging (DEVICE inflate: the
// compressed bytes cross PCIe, png_inflate_kernel decodes one stream per wave) or inflate them themselves with the same inflate.h
// (HOST: the filtered raw bytes cross PCIe).  Everything after that runs on the device: unfilter, expand to the hasher's pixels, the
// pixel hashes and PDQ over runs of equal geometry, as reconstruct_and_hash does for JPEG.  A call is processed in chunks whose device
// buffers are kept in the context between calls (rph_png_release returns them).
#include <string.h>

#include <algorithm>
#include <vector>

#include "file_pipeline.h"
#include "png_host.h"
#include "rph_internal.h"

int rph_png_launch_unfilter(uint8_t *d_raw, const void *d_jobs, uint32_t n_jobs, int32_t *d_status, hipStream_t s);
int rph_png_launch_expand(const uint8_t *d_raw, const void *d_images, const uint32_t *d_list, uint32_t n, uint64_t max_pixels, const uint8_t *d_pal,
                          uint8_t *d_hp, uint8_t *d_x16, uint8_t *d_nat, hipStream_t s);

namespace {

struct PngPipe : FilePipeBase {
    DevBuf comp, raw, meta, status;
    PinnedBuf h_comp, h_raw, h_meta, h_status;
    HashStageBufs hash;
};

// AUTO: the device inflates a chunk whose raw bytes are at least this many times its compressed bytes, the host threads inflate the rest.
// One wave walks a stream at a rate set by its symbols, so the device pays where a symbol yields many bytes (long copies: screenshots,
// 1920x1080 RGBA at ~400:1, 4.9 vs 3.8 GB/s of pixels for the host threads) and loses where nearly every byte is a literal (photographic
// RGB at ~1.5:1: 1.5 vs 3.2 GB/s; palette images at ~9:1: 1.5 vs 1.7 GB/s); DESIGN.md 4.7, profiles/png_rate.txt
constexpr uint64_t AUTO_DEVICE_MIN_RATIO = 32;

using Outputs = FileOutputs;

// one chunk: files[idx[k]] for k in [0, m), all parsed RPH_OK
int run_chunk(rph_ctx *ctx, PngPipe &P, const uint8_t *const *data, std::vector<rphp::Parsed> &parsed, const uint32_t *idx, size_t m, unsigned threads,
              const Outputs &out)
{
    hipStream_t s = P.s;
    auto reserve = [s](auto &buf, size_t bytes) { return reserve_slack(buf, bytes, s); };
    int mode = ctx->file[RPH_FILE_PNG].mode;
    // raw / compressed placement
    uint64_t raw_bytes = 0, comp_bytes = 0;
    std::vector<uint64_t> comp_off(m);
    for (size_t k = 0; k < m; k++) {
        rphp::Image &im = parsed[idx[k]].im;
        im.raw_off = raw_bytes;
        raw_bytes += align_up(im.raw_bytes, 16);
        comp_off[k] = comp_bytes;
        comp_bytes += parsed[idx[k]].idat_bytes;
    }
    if (mode == RPH_PNG_INFLATE_AUTO) mode = raw_bytes >= AUTO_DEVICE_MIN_RATIO * comp_bytes ? RPH_PNG_INFLATE_DEVICE : RPH_PNG_INFLATE_HOST;
    // metadata: images, palettes, streams, unfilter jobs, list, BLAKE3 offsets (each section 256-byte aligned)
    size_t n_jobs = 0;
    for (size_t k = 0; k < m; k++)
        for (int p = 0; p < 7; p++) n_jobs += parsed[idx[k]].im.pass_h[p] ? 1 : 0;
    Layout L;
    const size_t off_img = L.add(m * sizeof(rphp::Image)), off_pal = L.add(m * 1024, 256), off_str = L.add(m * sizeof(rphp::StreamDesc), 256),
                 off_job = L.add(n_jobs * sizeof(rphp::UnfilterJob), 256), off_list = L.add(m * 4, 256), off_b3 = L.add((m + 1) * 8, 256), meta_bytes = L.end();
    RPH_TRY(reserve(P.meta, meta_bytes));
    RPH_TRY(reserve(P.h_meta, meta_bytes));
    RPH_TRY(reserve(P.raw, raw_bytes));
    RPH_TRY(reserve(P.status, m * 4));
    RPH_TRY(reserve(P.h_status, m * 4));
    rphp::Image *imgs = reinterpret_cast<rphp::Image *>(P.h_meta.data() + off_img);
    rphp::StreamDesc *sd = reinterpret_cast<rphp::StreamDesc *>(P.h_meta.data() + off_str);
    rphp::UnfilterJob *jobs = reinterpret_cast<rphp::UnfilterJob *>(P.h_meta.data() + off_job);
    uint32_t *list = reinterpret_cast<uint32_t *>(P.h_meta.data() + off_list);
    int32_t *st = reinterpret_cast<int32_t *>(P.h_status.data());
    size_t j = 0;
    for (size_t k = 0; k < m; k++) {
        const rphp::Parsed &pp = parsed[idx[k]];
        imgs[k] = pp.im;
        imgs[k].pal = (uint32_t)k;
        memcpy(P.h_meta.data() + off_pal + k * 1024, pp.palette, 1024);
        sd[k] = rphp::StreamDesc{comp_off[k], pp.idat_bytes, pp.im.raw_off, pp.im.raw_bytes, (uint32_t)k, 0};
        for (int p = 0; p < 7; p++)
            if (pp.im.pass_h[p]) jobs[j++] = rphp::UnfilterJob{pp.im.raw_off + pp.im.pass_off[p], pp.im.pass_h[p], pp.im.pass_rb[p], pp.im.unit, (uint32_t)k};
        st[k] = RPH_OK;
    }
    RPH_HIP_CHECK(hipMemcpyAsync(P.meta.data(), P.h_meta.data(), meta_bytes, hipMemcpyHostToDevice, s));
    if (mode == RPH_PNG_INFLATE_DEVICE) {
        RPH_TRY(reserve(P.comp, comp_bytes));
        RPH_TRY(reserve(P.h_comp, comp_bytes));
        parallel_for(0, m, threads, [&](size_t k) { rphp::gather(data[idx[k]], parsed[idx[k]], P.h_comp.data() + comp_off[k]); });
        RPH_HIP_CHECK(hipMemcpyAsync(P.comp.data(), P.h_comp.data(), comp_bytes, hipMemcpyHostToDevice, s));
        RPH_HIP_CHECK(hipMemcpyAsync(P.status.data(), st, m * 4, hipMemcpyHostToDevice, s));
        RPH_TRY(rph_png_launch_inflate(P.comp.data(), P.meta.data() + off_str, (uint32_t)m, P.raw.data(), (int32_t *)P.status.data(), s));
    } else {
        RPH_TRY(reserve(P.h_raw, raw_bytes));
        parallel_for(0, m, threads, [&](size_t k) {
            const rphp::Parsed &pp = parsed[idx[k]];
            std::vector<uint8_t> z(pp.idat_bytes);
            rphp::gather(data[idx[k]], pp, z.data());
            if (rphz::inflate_host(z.data(), z.size(), P.h_raw.data() + pp.im.raw_off, pp.im.raw_bytes) != rphz::Z_OK) st[k] = RPH_ERR_INVALID_ARG;
        });
        RPH_HIP_CHECK(hipMemcpyAsync(P.raw.data(), P.h_raw.data(), raw_bytes, hipMemcpyHostToDevice, s));
        RPH_HIP_CHECK(hipMemcpyAsync(P.status.data(), st, m * 4, hipMemcpyHostToDevice, s));
    }
    RPH_TRY(rph_png_launch_unfilter(P.raw.data(), P.meta.data() + off_job, (uint32_t)n_jobs, (int32_t *)P.status.data(), s));
    RPH_HIP_CHECK(hipMemcpyAsync(st, P.status.data(), m * 4, hipMemcpyDeviceToHost, s));
    RPH_HIP_CHECK(hipStreamSynchronize(s));
    return hash_decoded_images(ctx, s, P.hash, imgs, list, reinterpret_cast<uint64_t *>(P.h_meta.data() + off_b3), P.meta.data() + off_b3, st, idx, m, out,
                               [&](uint32_t g, uint64_t max_px, bool want_hp, uint64_t x16_bytes, uint64_t nat_bytes) -> int {
                                   RPH_HIP_CHECK(hipMemcpyAsync(P.meta.data(), P.h_meta.data(), meta_bytes, hipMemcpyHostToDevice, s));
                                   return rph_png_launch_expand(P.raw.data(), P.meta.data() + off_img, (const uint32_t *)(P.meta.data() + off_list), g, max_px,
                                                                P.meta.data() + off_pal, want_hp ? P.hash.hp.data() : nullptr, x16_bytes ? P.hash.x16.data() : nullptr,
                                                                nat_bytes ? P.hash.nat.data() : nullptr, s);
                               });
}

int run(rph_ctx *ctx, const uint8_t *const *data, const size_t *len, uint32_t n, unsigned threads, const Outputs &out)
{
    return with_file_pipe<PngPipe>(ctx, RPH_FILE_PNG, threads, [&](PngPipe &P, rph_file_slot &slot, unsigned threads) -> int {
        std::vector<rphp::Parsed> parsed(n);
        const std::vector<uint32_t> ok = parse_files(data, len, n, threads, out.status, slot.log, [&](size_t i) { return rphp::parse(data[i], len[i], parsed[i]); });
        const rph_file_limits &lim = ctx->file_limits;
        for (size_t a = 0; a < ok.size();) {
            const size_t b = chunk_end<3>(ok, a, lim.files, {lim.comp, lim.raw, lim.pixels}, [&](uint32_t i) -> std::array<uint64_t, 3> {
                const rphp::Parsed &p = parsed[i];
                return {p.idat_bytes, p.im.raw_bytes, (uint64_t)p.im.w * p.im.h};
            });
            slot.log.sizes.push_back((uint32_t)(b - a));
            RPH_TRY(run_chunk(ctx, P, data, parsed, ok.data() + a, b - a, threads, out));
            a = b;
        }
        return RPH_OK;
    });
}

}  // namespace

void rph_png_forget(rph_ctx *ctx) { forget_file_pipe<PngPipe>(ctx, RPH_FILE_PNG); }

extern "C" {

int rph_png_info(const uint8_t *data, size_t len, uint32_t *w, uint32_t *h, uint32_t *channels, uint32_t *bit_depth)
{
    return rph_guarded("rph_png_info", [&] { return file_info<rphp::Parsed>(data, len, w, h, channels, bit_depth, rphp::parse, image_out_depth); });
}

int rph_png_decode_host(const uint8_t *data, size_t len, void *pixels_out, size_t cap_bytes)
{
    return rph_guarded("rph_png_decode_host",
                       [&] { return file_decode_host<rphp::Parsed>("rph_png_decode_host", data, len, pixels_out, cap_bytes, rphp::decode_host); });
}

int rph_png_decode(rph_ctx *ctx, const uint8_t *data, size_t len, void *pixels_out, size_t cap_bytes)
{
    return rph_guarded("rph_png_decode", [&] {
        return file_decode<rphp::Parsed>(
            "rph_png_decode", ctx, data, len, pixels_out, cap_bytes, rphp::parse,
            [](const rphp::Image &im) { return (size_t)im.w * im.h * im.out_ch * (im.out_depth / 8); }, [&](const Outputs &o) { return run(ctx, &data, &len, 1, 1, o); });
    });
}

int rph_png_pdq_hash_batch(rph_ctx *ctx, const uint8_t *const *data, const size_t *len, uint32_t n, uint32_t n_threads, uint8_t *hash32_out,
                           float *quality_out, float *coeffs_out, uint8_t *dihedral_out, uint8_t *valid_out, int32_t *status_out,
                           uint8_t *pixel_hash32_out)
{
    return rph_guarded("rph_png_pdq_hash_batch", [&] {
        return file_hash_batch("rph_png_pdq_hash_batch", ctx, data, len, n, hash32_out, quality_out, coeffs_out, dihedral_out, valid_out, status_out, pixel_hash32_out,
                               [&](const Outputs &o) { return run(ctx, data, len, n, n_threads, o); });
    });
}

int rph_png_set_inflate(rph_ctx *ctx, int where) { return file_set_mode(ctx, RPH_FILE_PNG, where, RPH_PNG_INFLATE_HOST, RPH_PNG_INFLATE_AUTO); }

int rph_png_release(rph_ctx *ctx) { return file_release(ctx, RPH_FILE_PNG, rph_png_forget); }

}  // extern "C"
