// tiff_pipeline.cpp -- TIFF files -> PDQ hashes and pixel hashes (include/rupphash.h, TIFF section).
//
// The host threads parse the first IFD of every file into a table of segments (strips or tiles, tiff_host.cpp) and either copy the
// segments' bytes back to back into pinned staging (DEVICE: the compressed bytes cross PCIe; one wave per segment decompresses, LZW and
// PackBits in tiff_kernels.hip, Deflate through the PNG path's inflate kernel; uncompressed segments are read where they landed) or
// decompress them themselves with the same decoders (HOST: the decoded bytes cross PCIe).  The work is dealt out by segment, so one
// large file keeps every thread and every CU busy.  Everything after that runs on the device: one expand kernel (byte order, predictor,
// inversion, tile placement), then the pixel hashes and PDQ over runs of equal geometry (decoded_hash.h, shared with the PNG path).
// A call is processed in chunks whose buffers are kept in the context between calls (rph_tiff_release returns them).
#include <string.h>

#include <algorithm>
#include <vector>

#include "file_pipeline.h"
#include "png_host.h"
#include "rph_internal.h"
#include "tiff_host.h"

int rph_tiff_launch_decompress(uint32_t comp, const uint8_t *d_comp, const void *d_segs, uint32_t n, uint8_t *d_dec, int32_t *d_status, hipStream_t s);
int rph_tiff_launch_expand(const uint8_t *d_comp, const uint8_t *d_dec, const void *d_images, const void *d_segs, const uint32_t *d_list, uint32_t n,
                           uint64_t max_pixels, uint8_t *d_hp, uint8_t *d_x16, uint8_t *d_nat, hipStream_t s);

namespace {

struct TiffPipe : FilePipeBase {
    DevBuf comp, dec, meta, status;
    PinnedBuf h_comp, h_dec, h_meta, h_status;
    HashStageBufs hash;
};

constexpr size_t SEGS_PER_TASK = 32;  // segments a host thread takes at a time

// AUTO: the device decompresses a chunk whose decoded bytes are at least this many times its compressed bytes, the host threads the
// rest.  As for PNG, one wave walks a segment at a rate set by its codes: it pays where a code yields many bytes (1920x1080 RGBA
// screenshots, LZW + predictor at 38:1: 40.8 vs 33.4 GB/s of pixels for 16 host threads, and 43 MB instead of 1.66 GB cross PCIe) and
// loses where a code yields one or two (photographic RGB at 1.2:1: LZW 2.3 vs 4.4-4.6 GB/s, Deflate 2.8 vs 4.0); uncompressed files run
// alike in both modes.  Nothing was measured between the two classes; DESIGN.md 4.8, profiles/tiff_rate.txt
constexpr uint64_t AUTO_DEVICE_MIN_RATIO = 16;
inline int kind_of(uint32_t comp) { return comp == 1 ? 0 : comp == 5 ? 1 : comp == 8 ? 2 : 3; }

// one chunk: files[idx[k]] for k in [0, m), all parsed RPH_OK
int run_chunk(rph_ctx *ctx, TiffPipe &P, const uint8_t *const *data, std::vector<rpht::Parsed> &parsed, const uint32_t *idx, size_t m, unsigned threads,
              const FileOutputs &out)
{
    hipStream_t s = P.s;
    auto reserve = [s](auto &buf, size_t bytes) { return reserve_slack(buf, bytes, s); };
    // placement of the images' segments in the staging and decoded buffers
    uint64_t dec_bytes = 0, comp_bytes = 0;
    size_t n_segs = 0, n_of[4] = {0, 0, 0, 0};
    std::vector<uint64_t> comp_base(m);
    for (size_t k = 0; k < m; k++) {
        rpht::Parsed &pp = parsed[idx[k]];
        pp.im.dec_off = dec_bytes;
        pp.im.first_seg = (uint32_t)n_segs;
        dec_bytes += pp.im.dec_bytes;
        comp_base[k] = comp_bytes;
        comp_bytes += pp.comp_bytes;
        n_segs += pp.segs.size();
        n_of[kind_of(pp.im.comp)] += pp.segs.size();
    }
    int mode = ctx->file[RPH_FILE_TIFF].mode;
    if (mode == RPH_TIFF_DECOMPRESS_AUTO) mode = dec_bytes >= AUTO_DEVICE_MIN_RATIO * comp_bytes ? RPH_TIFF_DECOMPRESS_DEVICE : RPH_TIFF_DECOMPRESS_HOST;
    const bool device = mode == RPH_TIFF_DECOMPRESS_DEVICE;
    // metadata: images, segments (in image order, for expand), the device's work lists per compression, list, BLAKE3 offsets
    Layout L;
    const size_t off_img = L.add(m * sizeof(rpht::Image)), off_seg = L.add(n_segs * sizeof(rpht::Segment), 256),
                 off_lzw = L.add(device ? n_of[1] * sizeof(rpht::Segment) : 0, 256), off_zip = L.add(device ? n_of[2] * sizeof(rphp::StreamDesc) : 0, 256),
                 off_pb = L.add(device ? n_of[3] * sizeof(rpht::Segment) : 0, 256), off_list = L.add(m * 4, 256), off_b3 = L.add((m + 1) * 8, 256),
                 meta_bytes = L.end();
    RPH_TRY(reserve(P.meta, meta_bytes));
    RPH_TRY(reserve(P.h_meta, meta_bytes));
    RPH_TRY(reserve(P.dec, dec_bytes));
    RPH_TRY(reserve(P.status, m * 4));
    RPH_TRY(reserve(P.h_status, m * 4));
    uint8_t *M = P.h_meta.data();
    rpht::Image *imgs = reinterpret_cast<rpht::Image *>(M + off_img);
    rpht::Segment *segs = reinterpret_cast<rpht::Segment *>(M + off_seg), *lzw = reinterpret_cast<rpht::Segment *>(M + off_lzw),
                  *pb = reinterpret_cast<rpht::Segment *>(M + off_pb);
    rphp::StreamDesc *zip = reinterpret_cast<rphp::StreamDesc *>(M + off_zip);
    uint32_t *list = reinterpret_cast<uint32_t *>(M + off_list);
    int32_t *st = reinterpret_cast<int32_t *>(P.h_status.data());
    size_t j = 0, n_lzw = 0, n_zip = 0, n_pb = 0;
    for (size_t k = 0; k < m; k++) {
        const rpht::Parsed &pp = parsed[idx[k]];
        imgs[k] = pp.im;
        imgs[k].staged = device && pp.im.comp == 1;
        st[k] = RPH_OK;
        for (const rpht::Segment &sg : pp.segs) {
            rpht::Segment &d = segs[j++];
            d = sg;
            d.comp_off += comp_base[k];
            d.dec_off += pp.im.dec_off;
            d.image = (uint32_t)k;
            if (!device) continue;
            if (pp.im.comp == 5) lzw[n_lzw++] = d;
            if (pp.im.comp == 32773) pb[n_pb++] = d;
            if (pp.im.comp == 8) zip[n_zip++] = rphp::StreamDesc{d.comp_off, d.src_len, d.dec_off, d.dec_bytes, d.image, 0};
        }
    }
    RPH_HIP_CHECK(hipMemcpyAsync(P.meta.data(), M, meta_bytes, hipMemcpyHostToDevice, s));
    const size_t n_tasks = (n_segs + SEGS_PER_TASK - 1) / SEGS_PER_TASK;
    if (device) {
        RPH_TRY(reserve(P.comp, comp_bytes + 64));
        RPH_TRY(reserve(P.h_comp, comp_bytes + 64));
        parallel_for(0, n_tasks, threads, [&](size_t t) {
            for (size_t q = t * SEGS_PER_TASK; q < std::min(n_segs, (t + 1) * SEGS_PER_TASK); q++)
                memcpy(P.h_comp.data() + segs[q].comp_off, data[idx[segs[q].image]] + segs[q].src_off, segs[q].src_len);
        });
        RPH_HIP_CHECK(hipMemcpyAsync(P.comp.data(), P.h_comp.data(), comp_bytes, hipMemcpyHostToDevice, s));
        RPH_HIP_CHECK(hipMemcpyAsync(P.status.data(), st, m * 4, hipMemcpyHostToDevice, s));
        int32_t *d_st = reinterpret_cast<int32_t *>(P.status.data());
        RPH_TRY(rph_tiff_launch_decompress(5, P.comp.data(), P.meta.data() + off_lzw, (uint32_t)n_lzw, P.dec.data(), d_st, s));
        RPH_TRY(rph_tiff_launch_decompress(32773, P.comp.data(), P.meta.data() + off_pb, (uint32_t)n_pb, P.dec.data(), d_st, s));
        RPH_TRY(rph_png_launch_inflate(P.comp.data(), P.meta.data() + off_zip, (uint32_t)n_zip, P.dec.data(), d_st, s));
        RPH_HIP_CHECK(hipMemcpyAsync(st, P.status.data(), m * 4, hipMemcpyDeviceToHost, s));
        RPH_HIP_CHECK(hipStreamSynchronize(s));
    } else {
        RPH_TRY(reserve(P.h_dec, dec_bytes));
        parallel_for(0, n_tasks, threads, [&](size_t t) {
            for (size_t q = t * SEGS_PER_TASK; q < std::min(n_segs, (t + 1) * SEGS_PER_TASK); q++) {
                const rpht::Segment &sg = segs[q];
                if (!rpht::decompress_host(imgs[sg.image].comp, data[idx[sg.image]] + sg.src_off, sg.src_len, P.h_dec.data() + sg.dec_off, sg.dec_bytes))
                    __atomic_store_n(&st[sg.image], (int32_t)RPH_ERR_INVALID_ARG, __ATOMIC_RELAXED);
            }
        });
        RPH_HIP_CHECK(hipMemcpyAsync(P.dec.data(), P.h_dec.data(), dec_bytes, hipMemcpyHostToDevice, s));
    }
    return hash_decoded_images(ctx, s, P.hash, imgs, list, reinterpret_cast<uint64_t *>(M + off_b3), P.meta.data() + off_b3, st, idx, m, out,
                               [&](uint32_t g, uint64_t max_px, bool want_hp, uint64_t x16_bytes, uint64_t nat_bytes) -> int {
                                   RPH_HIP_CHECK(hipMemcpyAsync(P.meta.data(), M, meta_bytes, hipMemcpyHostToDevice, s));
                                   return rph_tiff_launch_expand(device ? P.comp.data() : nullptr, P.dec.data(), P.meta.data() + off_img, P.meta.data() + off_seg,
                                                                 (const uint32_t *)(P.meta.data() + off_list), g, max_px, want_hp ? P.hash.hp.data() : nullptr,
                                                                 x16_bytes ? P.hash.x16.data() : nullptr, nat_bytes ? P.hash.nat.data() : nullptr, s);
                               });
}

int run(rph_ctx *ctx, const uint8_t *const *data, const size_t *len, uint32_t n, unsigned threads, const FileOutputs &out)
{
    return with_file_pipe<TiffPipe>(ctx, RPH_FILE_TIFF, threads, [&](TiffPipe &P, rph_file_slot &slot, unsigned threads) -> int {
        std::vector<rpht::Parsed> parsed(n);
        const std::vector<uint32_t> ok = parse_files(data, len, n, threads, out.status, slot.log, [&](size_t i) { return rpht::parse(data[i], len[i], parsed[i]); });
        const rph_file_limits &lim = ctx->file_limits;
        for (size_t a = 0; a < ok.size();) {
            const size_t b = chunk_end<3>(ok, a, lim.files, {lim.comp, lim.raw, lim.pixels}, [&](uint32_t i) -> std::array<uint64_t, 3> {
                const rpht::Parsed &p = parsed[i];
                return {p.comp_bytes, p.im.dec_bytes, (uint64_t)p.im.w * p.im.h};
            });
            slot.log.sizes.push_back((uint32_t)(b - a));
            RPH_TRY(run_chunk(ctx, P, data, parsed, ok.data() + a, b - a, threads, out));
            a = b;
        }
        return RPH_OK;
    });
}

}  // namespace

void rph_tiff_forget(rph_ctx *ctx) { forget_file_pipe<TiffPipe>(ctx, RPH_FILE_TIFF); }

extern "C" {

int rph_tiff_info(const uint8_t *data, size_t len, uint32_t *w, uint32_t *h, uint32_t *channels, uint32_t *bit_depth)
{
    return rph_guarded("rph_tiff_info", [&] { return file_info<rpht::Parsed>(data, len, w, h, channels, bit_depth, rpht::parse, image_out_depth); });
}

int rph_tiff_decode_host(const uint8_t *data, size_t len, void *pixels_out, size_t cap_bytes)
{
    return rph_guarded("rph_tiff_decode_host",
                       [&] { return file_decode_host<rpht::Parsed>("rph_tiff_decode_host", data, len, pixels_out, cap_bytes, rpht::decode_host); });
}

int rph_tiff_decode(rph_ctx *ctx, const uint8_t *data, size_t len, void *pixels_out, size_t cap_bytes)
{
    return rph_guarded("rph_tiff_decode", [&] {
        return file_decode<rpht::Parsed>(
            "rph_tiff_decode", ctx, data, len, pixels_out, cap_bytes, rpht::parse,
            [](const rpht::Image &im) { return (size_t)im.w * im.h * im.out_ch * (im.out_depth / 8); }, [&](const FileOutputs &o) { return run(ctx, &data, &len, 1, 0, o); });
    });
}

int rph_tiff_pdq_hash_batch(rph_ctx *ctx, const uint8_t *const *data, const size_t *len, uint32_t n, uint32_t n_threads, uint8_t *hash32_out,
                            float *quality_out, float *coeffs_out, uint8_t *dihedral_out, uint8_t *valid_out, int32_t *status_out,
                            uint8_t *pixel_hash32_out)
{
    return rph_guarded("rph_tiff_pdq_hash_batch", [&] {
        return file_hash_batch("rph_tiff_pdq_hash_batch", ctx, data, len, n, hash32_out, quality_out, coeffs_out, dihedral_out, valid_out, status_out, pixel_hash32_out,
                               [&](const FileOutputs &o) { return run(ctx, data, len, n, n_threads, o); });
    });
}

int rph_tiff_set_decompress(rph_ctx *ctx, int where) { return file_set_mode(ctx, RPH_FILE_TIFF, where, RPH_TIFF_DECOMPRESS_HOST, RPH_TIFF_DECOMPRESS_AUTO); }

int rph_tiff_release(rph_ctx *ctx) { return file_release(ctx, RPH_FILE_TIFF, rph_tiff_forget); }

}  // extern "C"
