// decoded_hash.h -- the second half of a file pipeline (png_pipeline.cpp, tiff_pipeline.cpp): the decodable images of a chunk, sorted into
// runs of equal geometry, are expanded to the hasher's pixels by the format's own kernel and hashed where they lie (pixel hashes, PDQ);
// one result read-back per chunk.  The image type of a format names the fields used here alike: w, h, hc, out_ch, out_depth, hstride,
// hp_off, x16_off, nat_off.
#pragma once
#include <string.h>

#include <algorithm>
#include <vector>

#include "rph_internal.h"

// Per chunk of a call at most ctx->file_limits (rph_internal.h): files, compressed bytes, decompressed bytes, pixels (one image larger
// than a limit forms a chunk of its own)

// what a batch call hands out (any of them may be absent); native: the native pixels of the call's one image (rph_*_decode)
struct FileOutputs {
    uint8_t *hash = nullptr, *dihedral = nullptr, *valid = nullptr, *pixel = nullptr, *native = nullptr;
    float *quality = nullptr, *coeffs = nullptr;
    int32_t *status = nullptr;
    bool want_pdq = true;
};

// buffers of this stage, kept by the pipeline between calls
struct HashStageBufs {
    DevBuf hp, x16, nat, res, b3, dig;
    PinnedBuf h_res;
};

// a buffer that grows gets +25 % + 64 bytes, in whole pages
template <class Buf>
int reserve_slack(Buf &buf, size_t bytes, hipStream_t s)
{
    return buf.reserve(bytes, align_up(bytes + bytes / 4 + 64, 4096), s);
}

// imgs[0 .. m), list[0 .. m), b3off[0 .. m]: the chunk's images, work list and BLAKE3 offsets in the pinned copy of its metadata
// (d_b3off: the offsets' device twin); st[k]: status of image k after decoding; idx[k]: its file in the call.
// expand(g, max_px, want_hp, x16_bytes, nat_bytes) uploads the metadata again (the images now carry their output offsets) and launches
// the format's expand kernel over list[0 .. g).
template <class Image, class Expand>
int hash_decoded_images(rph_ctx *ctx, hipStream_t s, HashStageBufs &P, Image *imgs, uint32_t *list, uint64_t *b3off, const uint8_t *d_b3off, const int32_t *st,
                        const uint32_t *idx, size_t m, const FileOutputs &out, Expand &&expand)
{
    auto reserve = [s](auto &buf, size_t bytes) { return reserve_slack(buf, bytes, s); };
    // the decodable images in runs of equal geometry: (w, h, hasher channels, bit depth: 16-bit images take another pixel hash)
    std::vector<uint32_t> good;
    for (size_t k = 0; k < m; k++) {
        out.status[idx[k]] = st[k];
        if (st[k] == RPH_OK) good.push_back((uint32_t)k);
    }
    if (good.empty()) return RPH_OK;
    std::stable_sort(good.begin(), good.end(), [&](uint32_t a, uint32_t b) {
        const Image &x = imgs[a], &y = imgs[b];
        return x.w != y.w ? x.w < y.w : x.h != y.h ? x.h < y.h : x.hc != y.hc ? x.hc < y.hc : x.out_depth < y.out_depth;
    });
    const size_t g = good.size();
    const bool want_hp = out.want_pdq || out.pixel, want_x16 = out.pixel != nullptr;
    uint64_t hp_bytes = 0, x16_bytes = 0, nat_bytes = 0, max_px = 0;
    size_t n16 = 0;
    for (size_t q = 0; q < g; q++) {
        Image &im = imgs[good[q]];
        list[q] = good[q];
        max_px = std::max<uint64_t>(max_px, (uint64_t)im.w * im.h);
        if (want_hp) {
            im.hstride = (uint32_t)(im.hc * align_up(im.w, 8));
            im.hp_off = hp_bytes;
            hp_bytes += align_up((uint64_t)im.hstride * im.h, 64);
        }
        if (want_x16 && im.out_depth == 16) {
            im.x16_off = x16_bytes;
            b3off[n16++] = x16_bytes;
            x16_bytes += (uint64_t)im.w * im.h * 8;
        }
        if (out.native) {
            im.nat_off = nat_bytes;
            nat_bytes += align_up((uint64_t)im.w * im.h * im.out_ch * (im.out_depth / 8), 64);
        }
    }
    b3off[n16] = x16_bytes;
    // buffers of this stage
    const size_t res_bytes = g * (32 + 4 + 1024 + 256 + 1 + 32) + 4 * 256;
    RPH_TRY(reserve(P.hp, hp_bytes));
    if (x16_bytes) RPH_TRY(reserve(P.x16, x16_bytes));
    if (nat_bytes) RPH_TRY(reserve(P.nat, nat_bytes));
    RPH_TRY(reserve(P.res, res_bytes));
    RPH_TRY(reserve(P.h_res, res_bytes));
    size_t b3_scratch = 0;
    for (size_t q = 0; q < g;) {  // runs of equal geometry
        const Image &a = imgs[good[q]];
        size_t e = q + 1;
        while (e < g && imgs[good[e]].w == a.w && imgs[good[e]].h == a.h && imgs[good[e]].hc == a.hc && imgs[good[e]].out_depth == a.out_depth) e++;
        if (out.pixel && a.out_depth != 16) b3_scratch = std::max(b3_scratch, rph_pixel_hash_scratch_bytes((uint32_t)(e - q), a.w, a.h));
        q = e;
    }
    if (b3_scratch) RPH_TRY(reserve(P.b3, b3_scratch));
    if (n16) RPH_TRY(reserve(P.dig, n16 * 32));
    RPH_TRY(expand((uint32_t)g, max_px, want_hp, x16_bytes, nat_bytes));
    // result sections, each 256-byte aligned
    Layout RL;
    const size_t o_hash = RL.add(g * 32), o_q = RL.add(g * 4, 256), o_c = RL.add(g * 1024, 256), o_d = RL.add(g * 256, 256), o_v = RL.add(g, 256), o_px = RL.add(g * 32, 256);
    uint8_t *R = P.res.data(), *r_hash = R + o_hash, *r_q = R + o_q, *r_c = R + o_c, *r_d = R + o_d, *r_v = R + o_v, *r_px = R + o_px;
    for (size_t q = 0; q < g;) {
        const Image &a = imgs[good[q]];
        size_t e = q + 1;
        while (e < g && imgs[good[e]].w == a.w && imgs[good[e]].h == a.h && imgs[good[e]].hc == a.hc && imgs[good[e]].out_depth == a.out_depth) e++;
        const uint32_t cnt = (uint32_t)(e - q);
        const size_t istride = align_up((uint64_t)a.hstride * a.h, 64);
        // pixel hashes first: the reference hashes to_rgba16() before generate_pdq_features (scanner.rs:1393-1410).  (A run of 16-bit
        // images is consecutive in the RGBA16 buffer: hashed below, all 16-bit images of the chunk at once.)
        if (out.pixel && a.out_depth != 16)
            RPH_TRY(rph_launch_pixel_hash(P.hp.data() + a.hp_off, cnt, a.w, a.h, a.hc, a.hstride, istride, r_px + q * 32, s, b3_scratch ? P.b3.data() : nullptr));
        if (out.want_pdq)
            RPH_TRY(rph_pdq_hash_batch_dev(ctx, P.hp.data() + a.hp_off, cnt, a.w, a.h, a.hc, a.hstride, istride, r_hash + q * 32, out.quality ? r_q + q * 4 : nullptr,
                                           out.coeffs ? r_c + q * 1024 : nullptr, out.dihedral ? r_d + q * 256 : nullptr, r_v + q, s));
        q = e;
    }
    // 16-bit pixel hashes: BLAKE3 of the RGBA16 strings, digests into the result slots of those images (in the same order)
    std::vector<uint8_t> dig16(n16 * 32);
    if (n16) RPH_TRY(rph_blake3_batch_dev(ctx, P.x16.data(), d_b3off, (uint32_t)n16, nullptr, P.dig.data(), s));
    if (n16) RPH_HIP_CHECK(hipMemcpyAsync(dig16.data(), P.dig.data(), n16 * 32, hipMemcpyDeviceToHost, s));
    RPH_HIP_CHECK(hipMemcpyAsync(P.h_res.data(), R, res_bytes, hipMemcpyDeviceToHost, s));
    if (out.native) RPH_HIP_CHECK(hipMemcpyAsync(out.native, P.nat.data(), nat_bytes, hipMemcpyDeviceToHost, s));
    RPH_HIP_CHECK(hipStreamSynchronize(s));
    const uint8_t *H = P.h_res.data(), *h_hash = H + o_hash, *h_q = H + o_q, *h_c = H + o_c, *h_d = H + o_d, *h_v = H + o_v, *h_px = H + o_px;
    size_t i16 = 0;
    for (size_t q = 0; q < g; q++) {
        const uint32_t f = idx[good[q]];
        if (out.want_pdq) {
            memcpy(out.hash + (size_t)f * 32, h_hash + q * 32, 32);
            if (out.quality) memcpy(out.quality + f, h_q + q * 4, 4);
            if (out.coeffs) memcpy(out.coeffs + (size_t)f * 256, h_c + q * 1024, 1024);
            if (out.dihedral) memcpy(out.dihedral + (size_t)f * 256, h_d + q * 256, 256);
            if (out.valid) out.valid[f] = h_v[q];
        }
        if (out.pixel) {
            if (imgs[good[q]].out_depth == 16)
                memcpy(out.pixel + (size_t)f * 32, dig16.data() + 32 * i16++, 32);
            else
                memcpy(out.pixel + (size_t)f * 32, h_px + q * 32, 32);
        }
    }
    return RPH_OK;
}
