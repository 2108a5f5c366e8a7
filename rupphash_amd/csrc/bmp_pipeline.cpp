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
#include "decoded_hash.h"  // (FileOutputs and reserve_slack only: the hash stage here is the ragged one)
#include "rph_internal.h"

int rph_bmp_launch_expand(const uint8_t *d_src, const void *d_images, const uint32_t *d_pals, const void *d_work, uint32_t n_work, uint8_t *d_out, hipStream_t s);

namespace {

struct BmpPipe {
    hipStream_t s = nullptr;  // (rph_bmp_forget: synchronised before the buffers are freed)
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
    Layout RL;
    const size_t o_hash = RL.add(m * 32), o_q = RL.add(m * 4, 256), o_c = RL.add(m * 1024, 256), o_d = RL.add(m * 256, 256), o_v = RL.add(m, 256),
                 o_px = RL.add(m * 32, 256), res_bytes = RL.end();
    RPH_TRY(reserve(P.res, res_bytes));
    RPH_TRY(reserve(P.h_res, res_bytes));
    uint8_t *R = P.res.data();
    RPH_TRY(rph_image_hash_ragged_dev(ctx, P.px.data(), offset.data(), w.data(), h.data(), layout.data(), row_stride.data(), (uint32_t)m,
                                      out.want_pdq ? R + o_hash : nullptr, out.want_pdq && out.quality ? R + o_q : nullptr,
                                      out.want_pdq && out.coeffs ? R + o_c : nullptr, out.want_pdq && out.dihedral ? R + o_d : nullptr,
                                      out.want_pdq ? R + o_v : nullptr, out.pixel ? R + o_px : nullptr, s));
    RPH_HIP_CHECK(hipMemcpyAsync(P.h_res.data(), R, res_bytes, hipMemcpyDeviceToHost, s));
    RPH_HIP_CHECK(hipStreamSynchronize(s));
    const uint8_t *H = P.h_res.data();
    for (size_t k = 0; k < m; k++) {
        const uint32_t f = idx[k];
        if (out.want_pdq) {
            memcpy(out.hash + (size_t)f * 32, H + o_hash + k * 32, 32);
            if (out.quality) memcpy(out.quality + f, H + o_q + k * 4, 4);
            if (out.coeffs) memcpy(out.coeffs + (size_t)f * 256, H + o_c + k * 1024, 1024);
            if (out.dihedral) memcpy(out.dihedral + (size_t)f * 256, H + o_d + k * 256, 256);
            if (out.valid) out.valid[f] = H[o_v + k];
        }
        if (out.pixel) memcpy(out.pixel + (size_t)f * 32, H + o_px + k * 32, 32);
    }
    return RPH_OK;
}

int run(rph_ctx *ctx, const uint8_t *const *data, const size_t *len, uint32_t n, unsigned threads, const FileOutputs &out)
{
    std::lock_guard<std::mutex> lock(ctx->bmp_mu);
    RPH_HIP_CHECK(hipSetDevice(ctx->device));
    BmpPipe *P = static_cast<BmpPipe *>(ctx->bmp);
    if (!P) {
        P = new BmpPipe();
        hipError_t e = hipStreamCreateWithFlags(&P->s, hipStreamNonBlocking);
        if (e != hipSuccess) {
            delete P;
            rph_set_error("hipStreamCreate failed: %s", hipGetErrorString(e));
            return RPH_ERR_HIP;
        }
        ctx->bmp = P;
    }
    if (!threads) threads = rph_host_threads();
    std::vector<rphb::Parsed> parsed(n);
    parallel_for(0, n, threads, [&](size_t i) { out.status[i] = (data[i] && len[i]) ? rphb::parse(data[i], len[i], parsed[i]) : RPH_ERR_INVALID_ARG; });
    std::vector<uint32_t> ok;
    for (uint32_t i = 0; i < n; i++)
        if (out.status[i] == RPH_OK) ok.push_back(i);
    const rph_file_limits &lim = ctx->file_limits;
    rph_file_chunk_log &log = ctx->file_chunks[RPH_FILE_BMP];
    log = rph_file_chunk_log();
    for (size_t a = 0; a < ok.size();) {
        size_t b = a;
        uint64_t src = 0, px = 0;
        while (b < ok.size() && b - a < lim.files) {
            const rphb::Image &im = parsed[ok[b]].im;
            const uint64_t sb = (uint64_t)im.src_stride * im.h, ob = (uint64_t)im.out_stride * im.h;
            if (b > a && (src + sb > lim.bmp_src || px + ob > lim.bmp_out)) break;
            src += sb;
            px += ob;
            b++;
        }
        log.sizes.push_back((uint32_t)(b - a));
        RPH_TRY(run_chunk(ctx, *P, data, parsed, ok.data() + a, b - a, threads, out));
        a = b;
    }
    return RPH_OK;
}

}  // namespace

void rph_bmp_forget(rph_ctx *ctx)
{
    BmpPipe *P = static_cast<BmpPipe *>(ctx->bmp);
    if (!P) return;
    (void)hipStreamSynchronize(P->s);
    {  // the ragged hashers ordered the context's shared scratch behind this stream (as rph_stream_destroy)
        std::lock_guard<std::mutex> lock(ctx->mu);
        for (SharedScratch *sc : {&ctx->scratch, &ctx->rz_scratch, &ctx->b3_scratch, &ctx->image_planes}) sc->forget_stream(P->s);
        ctx->ll_scratch.erase(P->s);
    }
    (void)hipStreamDestroy(P->s);
    delete P;
    ctx->bmp = nullptr;
}

extern "C" {

int rph_bmp_info(const uint8_t *data, size_t len, uint32_t *w, uint32_t *h, uint32_t *channels, uint32_t *bit_depth)
{
    return rph_guarded("rph_bmp_info", [&]() -> int {
        if (!data) return RPH_ERR_INVALID_ARG;
        rphb::Parsed p;
        const int rc = rphb::parse(data, len, p);
        if (rc) return rc;
        if (w) *w = p.im.w;
        if (h) *h = p.im.h;
        if (channels) *channels = p.im.out_ch;
        if (bit_depth) *bit_depth = 8;
        return RPH_OK;
    });
}

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
    return rph_guarded("rph_bmp_decode", [&]() -> int {
        if (!ctx || !data || !pixels_out) return RPH_ERR_INVALID_ARG;
        rphb::Parsed p;
        int rc = rphb::parse(data, len, p);
        if (rc) return rc;
        const size_t row = (size_t)p.im.w * p.im.out_ch, need = row * p.im.h;
        if (need > cap_bytes) {
            rph_set_error("rph_bmp_decode: %zu bytes needed", need);
            return RPH_ERR_CAPACITY;
        }
        int32_t status = RPH_OK;
        FileOutputs o;
        o.want_pdq = false;
        o.status = &status;
        std::vector<uint8_t> staging((size_t)p.im.out_stride * p.im.h);
        o.native = staging.data();
        RPH_TRY(run(ctx, &data, &len, 1, 0, o));
        if (status != RPH_OK) return status;
        for (uint32_t y = 0; y < p.im.h; y++) memcpy((uint8_t *)pixels_out + y * row, staging.data() + (size_t)y * p.im.out_stride, row);
        return RPH_OK;
    });
}

int rph_bmp_pdq_hash_batch(rph_ctx *ctx, const uint8_t *const *data, const size_t *len, uint32_t n, uint32_t n_threads, uint8_t *hash32_out,
                           float *quality_out, float *coeffs_out, uint8_t *dihedral_out, uint8_t *valid_out, int32_t *status_out,
                           uint8_t *pixel_hash32_out)
{
    return rph_guarded("rph_bmp_pdq_hash_batch", [&]() -> int {
        if (!ctx || (n && (!data || !len || !hash32_out))) {
            rph_set_error("rph_bmp_pdq_hash_batch: null argument");
            return RPH_ERR_INVALID_ARG;
        }
        if (n == 0) return RPH_OK;
        std::vector<int32_t> st_local(status_out ? 0 : n);
        std::vector<uint8_t> v_local(valid_out ? 0 : n);
        FileOutputs o;
        o.hash = hash32_out;
        o.quality = quality_out;
        o.coeffs = coeffs_out;
        o.dihedral = dihedral_out;
        o.valid = valid_out ? valid_out : v_local.data();
        o.status = status_out ? status_out : st_local.data();
        o.pixel = pixel_hash32_out;
        memset(hash32_out, 0, (size_t)n * 32);
        if (quality_out) memset(quality_out, 0, (size_t)n * 4);
        if (coeffs_out) memset(coeffs_out, 0, (size_t)n * 1024);
        if (dihedral_out) memset(dihedral_out, 0, (size_t)n * 256);
        memset(o.valid, 0, n);
        if (pixel_hash32_out) memset(pixel_hash32_out, 0, (size_t)n * 32);
        return run(ctx, data, len, n, n_threads, o);
    });
}

int rph_bmp_release(rph_ctx *ctx)
{
    if (!ctx) return RPH_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lock(ctx->bmp_mu);
    (void)hipSetDevice(ctx->device);
    rph_bmp_forget(ctx);
    return RPH_OK;
}

}  // extern "C"
