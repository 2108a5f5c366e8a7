// bmp_pipeline.cpp -- BMP files -> PDQ hashes and pixel hashes (include/rupphash.h, BMP section).
//
// The host threads parse every file (bmp_host.cpp) and copy its pixel array, as it lies in the file, into pinned staging at a 16-byte
// aligned offset; only RLE8 / RLE4 streams are decoded there, into 8-bit index planes (RLE files are rare, and a wave per stream has lost
// to the host threads in every format that tried it: DESIGN.md 4.10, 4.11).  Everything after that runs on the device: one
// descriptor-driven expand kernel for the whole chunk (bmp_kernels.hip: flip, byte order, bit fields, palettes), then
// rph_image_hash_ragged_dev over the chunk's native pixels where they lie -- Rgb8 or Rgba8 rows of align_up(w * channels, 4) bytes --
// so that the number of launches does not depend on the number of sizes.  One result read-back per chunk.
// A call is processed in chunks whose buffers are kept in the context between calls (rph_bmp_release returns them).
#include <string.h>

#include <algorithm>
#include <vector>

#include "bmp_host.h"
#include "file_pipeline.h"  // (of decoded_hash.h: FileOutputs, ResultSections and reserve_slack only: the hash stage here is the ragged one)
#include "rph_internal.h"

int rph_bmp_launch_expand(const uint8_t *d_src, const void *d_images, const uint32_t *d_pals, const void *d_work, uint32_t n_work, uint8_t *d_out, hipStream_t s);

namespace {

struct BmpPipe : FilePipeBase {
    DevBuf src, px, meta, res;
    PinnedBuf h_src, h_meta, h_res;
};

// one chunk: files[idx[k]] for k in [0, m), all parsed RPH_OK
int run_chunk(rph_ctx *ctx, BmpPipe &P, const uint8_t *const *data, std::vector<rphb::Parsed> &parsed, const uint32_t *idx, size_t m, unsigned threads,
              const FileOutputs &out)
{
    hipStream_t s = P.s;
    auto reserve = [s](auto &buf, size_t bytes) { return reserve_slack(buf, bytes, s); };
    uint64_t src_bytes = 0, out_bytes = 0, n_work = 0;
    uint32_t pal_words = 0;
    for (size_t k = 0; k < m; k++) {
        rphb::Image &im = parsed[idx[k]].im;
        im.src_off = src_bytes;
        src_bytes += align_up((uint64_t)im.src_stride * im.h, 16);
        im.out_off = out_bytes;
        out_bytes += align_up((uint64_t)im.out_stride * im.h, 256);
        im.pal_off = pal_words;
        pal_words += im.pal_n;
        n_work += (im.h + im.band - 1) / im.band;
    }
    Layout L;
    const size_t off_img = L.add(m * sizeof(rphb::Image)), off_pal = L.add((size_t)pal_words * 4, 256), off_work = L.add(n_work * sizeof(rphb::Work), 256),
                 meta_bytes = L.end();
    RPH_TRY(reserve(P.meta, meta_bytes));
    RPH_TRY(reserve(P.h_meta, meta_bytes));
    RPH_TRY(reserve(P.src, src_bytes + 16));
    RPH_TRY(reserve(P.h_src, src_bytes + 16));
    RPH_TRY(reserve(P.px, out_bytes + 256));  // (the hashers read whole dwords and quads of a row)
    uint8_t *M = P.h_meta.data();
    rphb::Image *imgs = reinterpret_cast<rphb::Image *>(M + off_img);
    uint32_t *pals = reinterpret_cast<uint32_t *>(M + off_pal);
    rphb::Work *work = reinterpret_cast<rphb::Work *>(M + off_work);
    size_t wi = 0;
    for (size_t k = 0; k < m; k++) {
        const rphb::Parsed &pp = parsed[idx[k]];
        imgs[k] = pp.im;
        memcpy(pals + pp.im.pal_off, pp.pal, (size_t)pp.im.pal_n * 4);
        for (uint32_t row = 0; row < pp.im.h; row += pp.im.band) work[wi++] = rphb::Work{(uint32_t)k, row};
    }
    parallel_for(0, m, threads, [&](size_t k) { rphb::stage(data[idx[k]], parsed[idx[k]], P.h_src.data() + imgs[k].src_off); });
    RPH_HIP_CHECK(hipMemcpyAsync(P.meta.data(), M, meta_bytes, hipMemcpyHostToDevice, s));
    RPH_HIP_CHECK(hipMemcpyAsync(P.src.data(), P.h_src.data(), src_bytes, hipMemcpyHostToDevice, s));
    RPH_TRY(rph_bmp_launch_expand(P.src.data(), P.meta.data() + off_img, (const uint32_t *)(P.meta.data() + off_pal), P.meta.data() + off_work, (uint32_t)n_work,
                                  P.px.data(), s));
    if (out.native) {  // (rph_bmp_decode: the call's one image, rows at the device's stride)
        RPH_HIP_CHECK(hipMemcpyAsync(out.native, P.px.data() + imgs[0].out_off, (size_t)imgs[0].out_stride * imgs[0].h, hipMemcpyDeviceToHost, s));
        RPH_HIP_CHECK(hipStreamSynchronize(s));
        return RPH_OK;
    }
    // the hash stage: the ragged kernels over the chunk's descriptors; result sections, each 256-byte aligned
    std::vector<uint64_t> offset(m);
    std::vector<uint32_t> w(m), h(m), layout(m);
    std::vector<size_t> row_stride(m);
    for (size_t k = 0; k < m; k++) {
        offset[k] = imgs[k].out_off;
        w[k] = imgs[k].w, h[k] = imgs[k].h;
        layout[k] = imgs[k].out_ch == 4 ? RPH_LAYOUT_RGBA8 : RPH_LAYOUT_RGB8;
        row_stride[k] = imgs[k].out_stride;
    }
    const ResultSections RS(m);
    RPH_TRY(reserve(P.res, RS.bytes()));
    RPH_TRY(reserve(P.h_res, RS.bytes()));
    const ResultSections::Slots r = RS.device(P.res.data(), 0, out);
    RPH_TRY(rph_image_hash_ragged_dev(ctx, P.px.data(), offset.data(), w.data(), h.data(), layout.data(), row_stride.data(), (uint32_t)m, r.hash, r.quality,
                                      r.coeffs, r.dihedral, r.valid, r.pixel, s));
    RPH_HIP_CHECK(hipMemcpyAsync(P.h_res.data(), P.res.data(), RS.bytes(), hipMemcpyDeviceToHost, s));
    RPH_HIP_CHECK(hipStreamSynchronize(s));
    for (size_t k = 0; k < m; k++) RS.scatter(P.h_res.data(), k, idx[k], out);
    return RPH_OK;
}

int run(rph_ctx *ctx, const uint8_t *const *data, const size_t *len, uint32_t n, unsigned threads, const FileOutputs &out)
{
    return with_file_pipe<BmpPipe>(ctx, RPH_FILE_BMP, threads, [&](BmpPipe &P, rph_file_slot &slot, unsigned threads) -> int {
        std::vector<rphb::Parsed> parsed(n);
        const std::vector<uint32_t> ok = parse_files(data, len, n, threads, out.status, slot.log, [&](size_t i) { return rphb::parse(data[i], len[i], parsed[i]); });
        const rph_file_limits &lim = ctx->file_limits;
        for (size_t a = 0; a < ok.size();) {
            const size_t b = chunk_end<2>(ok, a, lim.files, {lim.bmp_src, lim.bmp_out}, [&](uint32_t i) -> std::array<uint64_t, 2> {
                const rphb::Image &im = parsed[i].im;
                return {(uint64_t)im.src_stride * im.h, (uint64_t)im.out_stride * im.h};
            });
            slot.log.sizes.push_back((uint32_t)(b - a));
            RPH_TRY(run_chunk(ctx, P, data, parsed, ok.data() + a, b - a, threads, out));
            a = b;
        }
        return RPH_OK;
    });
}

}  // namespace

void rph_bmp_forget(rph_ctx *ctx)
{
    forget_file_pipe<BmpPipe>(ctx, RPH_FILE_BMP, [ctx](hipStream_t s) {
        // the ragged hashers ordered the context's shared scratch behind this stream (as rph_stream_destroy)
        std::lock_guard<std::mutex> lock(ctx->mu);
        for (SharedScratch *sc : {&ctx->scratch, &ctx->rz_scratch, &ctx->b3_scratch, &ctx->image_planes}) sc->forget_stream(s);
        ctx->ll_scratch.erase(s);
    });
}

extern "C" {

int rph_bmp_info(const uint8_t *data, size_t len, uint32_t *w, uint32_t *h, uint32_t *channels, uint32_t *bit_depth)
{
    return rph_guarded("rph_bmp_info",
                       [&] { return file_info<rphb::Parsed>(data, len, w, h, channels, bit_depth, rphb::parse, [](const rphb::Image &) { return 8u; }); });
}

// (the size follows from the header, so the capacity is checked before the decoder runs: not file_decode_host's order)
int rph_bmp_decode_host(const uint8_t *data, size_t len, void *pixels_out, size_t cap_bytes)
{
    return rph_guarded("rph_bmp_decode_host", [&]() -> int {
        if (!data || !pixels_out) return RPH_ERR_INVALID_ARG;
        rphb::Parsed p;
        const int rc = rphb::parse(data, len, p);
        if (rc) return rc;
        const size_t need = (size_t)p.im.w * p.im.h * p.im.out_ch;
        if (need > cap_bytes) {
            rph_set_error("rph_bmp_decode_host: %zu bytes needed", need);
            return RPH_ERR_CAPACITY;
        }
        std::vector<uint8_t> px;
        RPH_TRY(rphb::decode_host(data, len, p, px));
        memcpy(pixels_out, px.data(), px.size());
        return RPH_OK;
    });
}

int rph_bmp_decode(rph_ctx *ctx, const uint8_t *data, size_t len, void *pixels_out, size_t cap_bytes)
{
    return rph_guarded("rph_bmp_decode", [&] {
        const auto row = [](const rphb::Image &im) { return (size_t)im.w * im.out_ch; };
        return file_decode<rphb::Parsed>(
            "rph_bmp_decode", ctx, data, len, pixels_out, cap_bytes, rphb::parse, [&](const rphb::Image &im) { return row(im) * im.h; },
            [&](const FileOutputs &o) { return run(ctx, &data, &len, 1, 0, o); },
            [](const rphb::Image &im, size_t) { return (size_t)im.out_stride * im.h; },  // (run_chunk: rows at the device's stride)
            [&](const rphb::Image &im, const uint8_t *staging, size_t) {
                for (uint32_t y = 0; y < im.h; y++) memcpy((uint8_t *)pixels_out + y * row(im), staging + (size_t)y * im.out_stride, row(im));
            });
    });
}

int rph_bmp_pdq_hash_batch(rph_ctx *ctx, const uint8_t *const *data, const size_t *len, uint32_t n, uint32_t n_threads, uint8_t *hash32_out,
                           float *quality_out, float *coeffs_out, uint8_t *dihedral_out, uint8_t *valid_out, int32_t *status_out,
                           uint8_t *pixel_hash32_out)
{
    return rph_guarded("rph_bmp_pdq_hash_batch", [&] {
        return file_hash_batch("rph_bmp_pdq_hash_batch", ctx, data, len, n, hash32_out, quality_out, coeffs_out, dihedral_out, valid_out, status_out, pixel_hash32_out,
                               [&](const FileOutputs &o) { return run(ctx, data, len, n, n_threads, o); });
    });
}

int rph_bmp_release(rph_ctx *ctx) { return file_release(ctx, RPH_FILE_BMP, rph_bmp_forget); }

}  // extern "C"
