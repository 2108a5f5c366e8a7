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

// The result sections of a chunk of n images, each 256-byte aligned: where they lie in the device buffer and in its pinned copy
// (hash 32 B, quality 4 B, coefficients 1024 B, dihedral hashes 256 B, valid 1 B and pixel hash 32 B per image)
struct ResultSections {
    size_t hash, quality, coeffs, dihedral, valid, pixel, end;
    explicit ResultSections(size_t n)
    {
        Layout L;
        hash = L.add(n * 32), quality = L.add(n * 4, 256), coeffs = L.add(n * 1024, 256), dihedral = L.add(n * 256, 256), valid = L.add(n, 256);
        pixel = L.add(n * 32, 256), end = L.end();
    }
    size_t bytes() const { return end; }
    // slot k of every section in the device buffer R; nullptr for what `out` does not ask for
    struct Slots {
        uint8_t *hash, *quality, *coeffs, *dihedral, *valid, *pixel;
    };
    Slots device(uint8_t *R, size_t k, const FileOutputs &out) const
    {
        const bool pdq = out.want_pdq;
        return {pdq ? R + hash + k * 32 : nullptr,
                pdq && out.quality ? R + quality + k * 4 : nullptr,
                pdq && out.coeffs ? R + coeffs + k * 1024 : nullptr,
                pdq && out.dihedral ? R + dihedral + k * 256 : nullptr,
                pdq ? R + valid + k : nullptr,
                out.pixel ? R + pixel + k * 32 : nullptr};
    }
    // slot k of the pinned copy H -> file f of the caller's arrays
    void scatter(const uint8_t *H, size_t k, uint32_t f, const FileOutputs &out) const
    {
        if (out.want_pdq) {
            memcpy(out.hash + (size_t)f * 32, H + hash + k * 32, 32);
            if (out.quality) memcpy(out.quality + f, H + quality + k * 4, 4);
            if (out.coeffs) memcpy(out.coeffs + (size_t)f * 256, H + coeffs + k * 1024, 1024);
            if (out.dihedral) memcpy(out.dihedral + (size_t)f * 256, H + dihedral + k * 256, 256);
            if (out.valid) out.valid[f] = H[valid + k];
        }
        if (out.pixel) memcpy(out.pixel + (size_t)f * 32, H + pixel + k * 32, 32);
    }
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
    const ResultSections RS(g);
    RPH_TRY(reserve(P.hp, hp_bytes));
    if (x16_bytes) RPH_TRY(reserve(P.x16, x16_bytes));
    if (nat_bytes) RPH_TRY(reserve(P.nat, nat_bytes));
    RPH_TRY(reserve(P.res, RS.bytes()));
    RPH_TRY(reserve(P.h_res, RS.bytes()));
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
    uint8_t *R = P.res.data();
    for (size_t q = 0; q < g;) {
        const Image &a = imgs[good[q]];
        size_t e = q + 1;
        while (e < g && imgs[good[e]].w == a.w && imgs[good[e]].h == a.h && imgs[good[e]].hc == a.hc && imgs[good[e]].out_depth == a.out_depth) e++;
        const uint32_t cnt = (uint32_t)(e - q);
        const size_t istride = align_up((uint64_t)a.hstride * a.h, 64);
        const ResultSections::Slots r = RS.device(R, q, out);
        // pixel hashes first: the reference hashes to_rgba16() before generate_pdq_features (scanner.rs:1393-1410).  (A run of 16-bit
        // images is consecutive in the RGBA16 buffer: hashed below, all 16-bit images of the chunk at once.)
        if (out.pixel && a.out_depth != 16)
            RPH_TRY(rph_launch_pixel_hash(P.hp.data() + a.hp_off, cnt, a.w, a.h, a.hc, a.hstride, istride, r.pixel, s, b3_scratch ? P.b3.data() : nullptr));
        if (out.want_pdq)
            RPH_TRY(rph_pdq_hash_batch_dev(ctx, P.hp.data() + a.hp_off, cnt, a.w, a.h, a.hc, a.hstride, istride, r.hash, r.quality, r.coeffs, r.dihedral,
                                           r.valid, s));
        q = e;
    }
    // 16-bit pixel hashes: BLAKE3 of the RGBA16 strings, digests into the result slots of those images (in the same order)
    std::vector<uint8_t> dig16(n16 * 32);
    if (n16) RPH_TRY(rph_blake3_batch_dev(ctx, P.x16.data(), d_b3off, (uint32_t)n16, nullptr, P.dig.data(), s));
    if (n16) RPH_HIP_CHECK(hipMemcpyAsync(dig16.data(), P.dig.data(), n16 * 32, hipMemcpyDeviceToHost, s));
    RPH_HIP_CHECK(hipMemcpyAsync(P.h_res.data(), R, RS.bytes(), hipMemcpyDeviceToHost, s));
    if (out.native) RPH_HIP_CHECK(hipMemcpyAsync(out.native, P.nat.data(), nat_bytes, hipMemcpyDeviceToHost, s));
    RPH_HIP_CHECK(hipStreamSynchronize(s));
    size_t i16 = 0;
    for (size_t q = 0; q < g; q++) {
        const uint32_t f = idx[good[q]];
        RS.scatter(P.h_res.data(), q, f, out);
        if (out.pixel && imgs[good[q]].out_depth == 16) memcpy(out.pixel + (size_t)f * 32, dig16.data() + 32 * i16++, 32);  // (no kernel wrote its slot)
    }
    return RPH_OK;
}
