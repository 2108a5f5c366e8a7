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

#include "decoded_hash.h"
#include "png_host.h"
#include "rph_internal.h"

int rph_png_launch_unfilter(uint8_t *d_raw, const void *d_jobs, uint32_t n_jobs, int32_t *d_status, hipStream_t s);
int rph_png_launch_expand(const uint8_t *d_raw, const void *d_images, const uint32_t *d_list, uint32_t n, uint64_t max_pixels, const uint8_t *d_pal,
                          uint8_t *d_hp, uint8_t *d_x16, uint8_t *d_nat, hipStream_t s);

namespace {

struct PngPipe {
    hipStream_t s = nullptr;  // (rph_png_forget: synchronised before the buffers are freed)
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
    int mode = ctx->png_inflate;
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
    std::lock_guard<std::mutex> lock(ctx->png_mu);
    RPH_HIP_CHECK(hipSetDevice(ctx->device));
    PngPipe *P = static_cast<PngPipe *>(ctx->png);
    if (!P) {
        P = new PngPipe();
        hipError_t e = hipStreamCreateWithFlags(&P->s, hipStreamNonBlocking);
        if (e != hipSuccess) {
            delete P;
            rph_set_error("hipStreamCreate failed: %s", hipGetErrorString(e));
            return RPH_ERR_HIP;
        }
        ctx->png = P;
    }
    if (!threads) threads = rph_host_threads();
    std::vector<rphp::Parsed> parsed(n);
    parallel_for(0, n, threads, [&](size_t i) { out.status[i] = (data[i] && len[i]) ? rphp::parse(data[i], len[i], parsed[i]) : RPH_ERR_INVALID_ARG; });
    std::vector<uint32_t> ok;
    for (uint32_t i = 0; i < n; i++)
        if (out.status[i] == RPH_OK) ok.push_back(i);
    const rph_file_limits &lim = ctx->file_limits;
    rph_file_chunk_log &log = ctx->file_chunks[RPH_FILE_PNG];
    log = rph_file_chunk_log();
    for (size_t a = 0; a < ok.size();) {
        size_t b = a;
        uint64_t comp = 0, raw = 0, px = 0;
        while (b < ok.size() && b - a < lim.files) {
            const rphp::Parsed &p = parsed[ok[b]];
            const uint64_t pix = (uint64_t)p.im.w * p.im.h;
            if (b > a && (comp + p.idat_bytes > lim.comp || raw + p.im.raw_bytes > lim.raw || px + pix > lim.pixels)) break;
            comp += p.idat_bytes;
            raw += p.im.raw_bytes;
            px += pix;
            b++;
        }
        log.sizes.push_back((uint32_t)(b - a));
        RPH_TRY(run_chunk(ctx, *P, data, parsed, ok.data() + a, b - a, threads, out));
        a = b;
    }
    return RPH_OK;
}

}  // namespace

void rph_png_forget(rph_ctx *ctx)
{
    PngPipe *P = static_cast<PngPipe *>(ctx->png);
    if (!P) return;
    (void)hipStreamSynchronize(P->s);
    (void)hipStreamDestroy(P->s);
    delete P;
    ctx->png = nullptr;
}

extern "C" {

int rph_png_info(const uint8_t *data, size_t len, uint32_t *w, uint32_t *h, uint32_t *channels, uint32_t *bit_depth)
{
    return rph_guarded("rph_png_info", [&]() -> int {
        if (!data) return RPH_ERR_INVALID_ARG;
        rphp::Parsed p;
        const int rc = rphp::parse(data, len, p);
        if (rc) return rc;
        if (w) *w = p.im.w;
        if (h) *h = p.im.h;
        if (channels) *channels = p.im.out_ch;
        if (bit_depth) *bit_depth = p.im.out_depth;
        return RPH_OK;
    });
}

int rph_png_decode_host(const uint8_t *data, size_t len, void *pixels_out, size_t cap_bytes)
{
    return rph_guarded("rph_png_decode_host", [&]() -> int {
        if (!data || !pixels_out) return RPH_ERR_INVALID_ARG;
        rphp::Parsed p;
        std::vector<uint8_t> px;
        const int rc = rphp::decode_host(data, len, p, px);
        if (rc) return rc;
        if (px.size() > cap_bytes) {
            rph_set_error("rph_png_decode_host: %zu bytes needed", px.size());
            return RPH_ERR_CAPACITY;
        }
        memcpy(pixels_out, px.data(), px.size());
        return RPH_OK;
    });
}

int rph_png_decode(rph_ctx *ctx, const uint8_t *data, size_t len, void *pixels_out, size_t cap_bytes)
{
    return rph_guarded("rph_png_decode", [&]() -> int {
        if (!ctx || !data || !pixels_out) return RPH_ERR_INVALID_ARG;
        rphp::Parsed p;
        int rc = rphp::parse(data, len, p);
        if (rc) return rc;
        const size_t need = (size_t)p.im.w * p.im.h * p.im.out_ch * (p.im.out_depth / 8);
        if (need > cap_bytes) {
            rph_set_error("rph_png_decode: %zu bytes needed", need);
            return RPH_ERR_CAPACITY;
        }
        int32_t status = RPH_OK;
        Outputs o;
        o.want_pdq = false;
        o.status = &status;
        // (the pinned result copy is skipped: the native pixels land in a device buffer and are copied to the caller's memory)
        std::vector<uint8_t> staging(align_up(need, 64) + 64);
        o.native = staging.data();
        RPH_TRY(run(ctx, &data, &len, 1, 1, o));
        if (status != RPH_OK) return status;
        memcpy(pixels_out, staging.data(), need);
        return RPH_OK;
    });
}

int rph_png_pdq_hash_batch(rph_ctx *ctx, const uint8_t *const *data, const size_t *len, uint32_t n, uint32_t n_threads, uint8_t *hash32_out,
                           float *quality_out, float *coeffs_out, uint8_t *dihedral_out, uint8_t *valid_out, int32_t *status_out,
                           uint8_t *pixel_hash32_out)
{
    return rph_guarded("rph_png_pdq_hash_batch", [&]() -> int {
        if (!ctx || (n && (!data || !len || !hash32_out))) {
            rph_set_error("rph_png_pdq_hash_batch: null argument");
            return RPH_ERR_INVALID_ARG;
        }
        if (n == 0) return RPH_OK;
        std::vector<int32_t> st_local(status_out ? 0 : n);
        std::vector<uint8_t> v_local(valid_out ? 0 : n);
        Outputs o;
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

int rph_png_set_inflate(rph_ctx *ctx, int where)
{
    if (!ctx || where < RPH_PNG_INFLATE_HOST || where > RPH_PNG_INFLATE_AUTO) return RPH_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lock(ctx->png_mu);
    ctx->png_inflate = where;
    return RPH_OK;
}

int rph_png_release(rph_ctx *ctx)
{
    if (!ctx) return RPH_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lock(ctx->png_mu);
    (void)hipSetDevice(ctx->device);
    rph_png_forget(ctx);
    return RPH_OK;
}

}  // extern "C"
