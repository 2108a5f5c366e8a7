// file_pipeline.h -- the shell around run_chunk that the five file pipelines share (png_, tiff_, webp_, gif_, bmp_pipeline.cpp): a
// format's place in the context (rph_file_slot, rph_internal.h) with its pipe and stream, the parse of a call's files, the rule that
// cuts the parsed files into chunks, and the bodies of the entry points (info, decode_host, decode, pdq_hash_batch, set mode, release).
// A format hands in its own functions as callables; what only one format does stays in that format's file.
#pragma once
#include <string.h>

#include <array>
#include <vector>

#include "decoded_hash.h"
#include "rph_internal.h"

// what every format's pipe starts with; its buffers follow in the format's own struct
struct FilePipeBase {
    hipStream_t s = nullptr;  // (forget_file_pipe: synchronised before the buffers are freed)
};

// One call on a format's pipeline, one at a time per context: body(pipe, slot, threads) runs under the slot's mutex on the context's
// device, with the pipe and its stream made on first use and `threads` defaulted
template <class Pipe, class Body>
int with_file_pipe(rph_ctx *ctx, int format, unsigned threads, Body &&body)
{
    rph_file_slot &slot = ctx->file[format];
    std::lock_guard<std::mutex> lock(slot.mu);
    RPH_HIP_CHECK(hipSetDevice(ctx->device));
    Pipe *P = static_cast<Pipe *>(slot.pipe);
    if (!P) {
        P = new Pipe();
        hipError_t e = hipStreamCreateWithFlags(&P->s, hipStreamNonBlocking);
        if (e != hipSuccess) {
            delete P;
            rph_set_error("hipStreamCreate failed: %s", hipGetErrorString(e));
            return RPH_ERR_HIP;
        }
        slot.pipe = P;
    }
    if (!threads) threads = rph_host_threads();
    return body(*P, slot, threads);
}

// rph_*_forget (the caller holds the slot's mutex, or is rph_shutdown): the stream is drained, between(stream) runs, then the stream
// and the pipe's buffers go
template <class Pipe, class Between>
void forget_file_pipe(rph_ctx *ctx, int format, Between &&between)
{
    rph_file_slot &slot = ctx->file[format];
    Pipe *P = static_cast<Pipe *>(slot.pipe);
    if (!P) return;
    (void)hipStreamSynchronize(P->s);
    between(P->s);
    (void)hipStreamDestroy(P->s);
    delete P;
    slot.pipe = nullptr;
}
template <class Pipe>
void forget_file_pipe(rph_ctx *ctx, int format)
{
    forget_file_pipe<Pipe>(ctx, format, [](hipStream_t) {});
}

// rph_*_release: forget = the format's rph_*_forget
template <class Forget>
int file_release(rph_ctx *ctx, int format, Forget &&forget)
{
    if (!ctx) return RPH_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lock(ctx->file[format].mu);
    (void)hipSetDevice(ctx->device);
    forget(ctx);
    return RPH_OK;
}

// rph_*_set_*: where the format's streams are decoded, one of lo .. hi
inline int file_set_mode(rph_ctx *ctx, int format, int where, int lo, int hi)
{
    if (!ctx || where < lo || where > hi) return RPH_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lock(ctx->file[format].mu);
    ctx->file[format].mode = where;
    return RPH_OK;
}

// the files of [first, last) with status RPH_OK, in call order
inline std::vector<uint32_t> ok_files(const int32_t *status, uint32_t first, uint32_t last)
{
    std::vector<uint32_t> ok;
    for (uint32_t i = first; i < last; i++)
        if (status[i] == RPH_OK) ok.push_back(i);
    return ok;
}

// The start of a call: status[i] = parse(i) for every file that is there (RPH_ERR_INVALID_ARG for a null or empty one) on `threads`
// threads, and a fresh chunk log -> the files that parsed
template <class Parse>
std::vector<uint32_t> parse_files(const uint8_t *const *data, const size_t *len, uint32_t n, unsigned threads, int32_t *status, rph_file_chunk_log &log,
                                  Parse &&parse)
{
    parallel_for(0, n, threads, [&](size_t i) { status[i] = (data[i] && len[i]) ? parse(i) : RPH_ERR_INVALID_ARG; });
    log = rph_file_chunk_log();
    return ok_files(status, 0, n);
}

// The chunk cut: the chunk that starts at ok[a] ends before ok[b].  It takes files while it holds fewer than max_files and stops before
// the first file that would take any of the K running sums of cost(file) over its bound -- except that its first file always goes in
// (one image larger than a limit forms a chunk of its own).  tests/file_chunks.py restates this rule
template <size_t K, class Cost>
size_t chunk_end(const std::vector<uint32_t> &ok, size_t a, uint64_t max_files, const std::array<uint64_t, K> &bounds, Cost &&cost)
{
    std::array<uint64_t, K> sum{};
    size_t b = a;
    while (b < ok.size() && b - a < max_files) {
        const std::array<uint64_t, K> c = cost(ok[b]);
        bool over = false;
        for (size_t q = 0; q < K; q++) over |= sum[q] + c[q] > bounds[q];
        if (b > a && over) break;
        for (size_t q = 0; q < K; q++) sum[q] += c[q];
        b++;
    }
    return b;
}

// ---- the bodies of the entry points; each runs inside the entry point's rph_guarded, `name` is the entry point's ----

// the native bit depth of a format whose image type names it
constexpr auto image_out_depth = [](const auto &im) -> uint32_t { return im.out_depth; };

// rph_*_info
template <class Parsed, class Parse, class Depth>
int file_info(const uint8_t *data, size_t len, uint32_t *w, uint32_t *h, uint32_t *channels, uint32_t *bit_depth, Parse &&parse, Depth &&depth)
{
    if (!data) return RPH_ERR_INVALID_ARG;
    Parsed p;
    const int rc = parse(data, len, p);
    if (rc) return rc;
    if (w) *w = p.im.w;
    if (h) *h = p.im.h;
    if (channels) *channels = p.im.out_ch;
    if (bit_depth) *bit_depth = depth(p.im);
    return RPH_OK;
}

// rph_*_decode_host of the formats that decode first and know the size afterwards
template <class Parsed, class Decode>
int file_decode_host(const char *name, const uint8_t *data, size_t len, void *pixels_out, size_t cap_bytes, Decode &&decode)
{
    if (!data || !pixels_out) return RPH_ERR_INVALID_ARG;
    Parsed p;
    std::vector<uint8_t> px;
    const int rc = decode(data, len, p, px);
    if (rc) return rc;
    if (px.size() > cap_bytes) {
        rph_set_error("%s: %zu bytes needed", name, px.size());
        return RPH_ERR_CAPACITY;
    }
    memcpy(pixels_out, px.data(), px.size());
    return RPH_OK;
}

// rph_*_decode: need_of(image) = the bytes of its native pixels; run(outputs) = the format's run on this one file;
// staging_bytes(image, need) = the host buffer the chunk's native pixels are copied into, copy_out(image, staging, need) takes them
// from there to pixels_out
template <class Parsed, class Parse, class Need, class Run, class StagingBytes, class CopyOut>
int file_decode(const char *name, rph_ctx *ctx, const uint8_t *data, size_t len, void *pixels_out, size_t cap_bytes, Parse &&parse, Need &&need_of, Run &&run,
                StagingBytes &&staging_bytes, CopyOut &&copy_out)
{
    if (!ctx || !data || !pixels_out) return RPH_ERR_INVALID_ARG;
    Parsed p;
    int rc = parse(data, len, p);
    if (rc) return rc;
    const size_t need = need_of(p.im);
    if (need > cap_bytes) {
        rph_set_error("%s: %zu bytes needed", name, need);
        return RPH_ERR_CAPACITY;
    }
    int32_t status = RPH_OK;
    FileOutputs o;
    o.want_pdq = false;
    o.status = &status;
    // (the pinned result copy is skipped: the native pixels land in a device buffer and are copied to the caller's memory)
    std::vector<uint8_t> staging(staging_bytes(p.im, need));
    o.native = staging.data();
    RPH_TRY(run(o));
    if (status != RPH_OK) return status;
    copy_out(p.im, staging.data(), need);
    return RPH_OK;
}
// the formats whose native pixels arrive packed (decoded_hash.h places them in slots of whole 64 bytes)
template <class Parsed, class Parse, class Need, class Run>
int file_decode(const char *name, rph_ctx *ctx, const uint8_t *data, size_t len, void *pixels_out, size_t cap_bytes, Parse &&parse, Need &&need_of, Run &&run)
{
    return file_decode<Parsed>(
        name, ctx, data, len, pixels_out, cap_bytes, parse, need_of, run, [](const auto &, size_t need) { return align_up(need, 64) + 64; },
        [pixels_out](const auto &, const uint8_t *staging, size_t need) { memcpy(pixels_out, staging, need); });
}

// rph_*_pdq_hash_batch: run(outputs) = the format's run on the call's files
template <class Run>
int file_hash_batch(const char *name, rph_ctx *ctx, const uint8_t *const *data, const size_t *len, uint32_t n, uint8_t *hash32_out, float *quality_out,
                    float *coeffs_out, uint8_t *dihedral_out, uint8_t *valid_out, int32_t *status_out, uint8_t *pixel_hash32_out, Run &&run)
{
    if (!ctx || (n && (!data || !len || !hash32_out))) {
        rph_set_error("%s: null argument", name);
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
    return run(o);
}
