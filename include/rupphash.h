/*
 * rupphash.h -- C ABI of librupphash_hip.so: the MI355X (gfx950) engine for the
 * PDQ-hash + 256-bit Hamming-grouping hot path of Safari77/rupphash (phdupes).
 *
 * Each entry point names the reference interface it replaces (file:line in the
 * reference tree).  The library is a drop-in for that path only; the reference's
 * Rust modules keep their public signatures and call these functions through an
 * `extern "C"` block (INTEGRATION.md shows the binding).
 *
 * Conventions
 *   - every function returns 0 (RPH_OK) or a negative rph_status; nothing aborts
 *   - plain pointers and sizes only; the caller owns every buffer
 *   - one rph_ctx per GPU (one process per GPU with rupphash_amd/dist.py, or several
 *     contexts in one process under an rph_multi, below); a context is thread-safe:
 *     concurrent calls are safe, their GPU work is ordered on the stream each one uses
 *     (the context's own stream for the host-pointer entry points), and the library's
 *     shared scratch buffers are handed from one stream to the next with events
 *   - `*_dev` twins take DEVICE pointers and a hipStream_t (as void*) and enqueue
 *     asynchronously on it (work given to different streams may overlap; the library
 *     orders its own shared scratch between them).  They do not synchronise, except when
 *     a scratch buffer has to grow or a source geometry larger than 512 px is met for
 *     the first time (its resize tables are then uploaded once).  Host-pointer
 *     versions stage through device memory and return when the result is in the
 *     caller's buffer
 *   - there is no CPU fallback: if no gfx950 device is usable, rph_init fails
 */
#ifndef RUPPHASH_H
#define RUPPHASH_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RPH_ABI_VERSION 1

typedef enum rph_status {
    RPH_OK = 0,
    RPH_ERR_INVALID_ARG = -1,
    RPH_ERR_NO_DEVICE = -2,     /* no HIP device / not gfx950 */
    RPH_ERR_HIP = -3,           /* a HIP runtime call failed; rph_last_error() has the text */
    RPH_ERR_OOM = -4,
    RPH_ERR_UNSUPPORTED = -5,   /* an input this library does not take (e.g. a CMYK or arithmetic-coded JPEG): the caller keeps its own path for it */
    RPH_ERR_CAPACITY = -6       /* output capacity too small; the required count is still reported */
} rph_status;

typedef struct rph_ctx rph_ctx;

/* ---- constants of the reference ---- */
#define RPH_MAX_SIMILARITY_64 15u    /* hamminghash.rs:5  MAX_SIMILARITY_64  */
#define RPH_MAX_SIMILARITY_256 63u   /* hamminghash.rs:8  MAX_SIMILARITY_256 */
#define RPH_PDQ_MIN_QUALITY 50       /* scanner.rs:1588   PDQ_MIN_QUALITY    */
#define RPH_PDQ_MIN_DIM 5u           /* pdqhash.rs:17     MIN_HASHABLE_DIM   */
#define RPH_PDQ_MAX_DIM 512u         /* pdqhash.rs:19     DOWNSAMPLE_DIMS    */

/* ---- lifecycle ---- */
int rph_abi_version(void);
/* Bind to HIP device `device` (ordinal within HIP_VISIBLE_DEVICES).  Fails with
 * RPH_ERR_NO_DEVICE when the device is missing or is not gfx950. */
int rph_init(int device, rph_ctx **ctx_out);
int rph_shutdown(rph_ctx *ctx);
/* Text of the last error raised on this thread (never NULL). */
const char *rph_last_error(void);
const char *rph_status_string(int status);
/* name[64], compute-unit count, bytes of device memory */
int rph_device_info(rph_ctx *ctx, char *name64, int *compute_units, uint64_t *total_mem);
/* Block until all work queued on the context's own stream is done. */
int rph_synchronize(rph_ctx *ctx);

/* =====================================================================
 * PDQ hashing  (reference: src/pdqhash.rs)
 * ===================================================================== */

/*
 * Batch form of generate_pdq_features / generate_pdq (pdqhash.rs:166-201) +
 * PdqFeatures::to_hash (:59-61) + generate_dihedral_hashes (:71-87).
 *
 * px: n images of w x h pixels, `channels` interleaved u8 samples per pixel
 *     (1 = Luma8, borrowed as is pdqhash.rs:173; 3 = RGB8; 4 = RGBA8, alpha
 *     ignored :279), row_stride bytes between rows, image_stride bytes between
 *     images.  All images of a call share one geometry.
 * Outputs (each nullable except hash32_out):
 *   hash32_out   n x 32 bytes           to_hash() of the features
 *   quality_out  n floats in [0,1]      second member of the reference's tuple
 *   coeffs_out   n x 256 floats         PdqFeatures.coefficients, row-major i*16+j
 *   dihedral_out n x 8 x 32 bytes       generate_dihedral_hashes(), reference slot order
 *   valid_out    n bytes                1 = Some(..), 0 = None (w or h < 5, :167-169)
 * w or h > 512: the images are first converted to luma and pre-downsampled to the aspect-preserving <= 512 px
 * thumbnail exactly where the reference does it (:181-220, calculate_target_dimensions + resize_luma_fast).  The
 * resize is the third-party fast_image_resize 6.1.0 Convolution(Box)/U8, restated from its published algorithm:
 * parity with the Rust binary is unpinned for such inputs.
 */
int rph_pdq_hash_batch(rph_ctx *ctx, const uint8_t *px, uint32_t n, uint32_t w, uint32_t h,
                       uint32_t channels, size_t row_stride, size_t image_stride,
                       uint8_t *hash32_out, float *quality_out, float *coeffs_out,
                       uint8_t *dihedral_out, uint8_t *valid_out);
int rph_pdq_hash_batch_dev(rph_ctx *ctx, const void *d_px, uint32_t n, uint32_t w, uint32_t h,
                           uint32_t channels, size_t row_stride, size_t image_stride,
                           void *d_hash32, void *d_quality, void *d_coeffs, void *d_dihedral,
                           void *d_valid, void *stream);

/*
 * generate_pdq_features for n images of ANY mix of geometries and channel counts, one call.
 * px[i]: image i, w[i] x h[i] pixels, channels[i] in {1,3,4} interleaved u8, row_stride[i] bytes between rows.
 * Outputs as rph_pdq_hash_batch (index i = image i; all but hash32_out nullable).
 *  - Every input rph_pdq_hash_batch accepts with n = 1 is accepted per image, w[i] or h[i] < 5 (valid 0, outputs zeroed) and
 *    4000 x 5 among them.
 *  - The result for image i is bit for bit what rph_pdq_hash_batch returns for that image alone: hash, quality, coefficients
 *    and dihedral hashes.
 *  - channels[i] outside {1,3,4}, row_stride[i] < w[i] * channels[i] or a null required pointer (ctx, px, px[i], w, h, channels,
 *    row_stride, hash32_out) gives RPH_ERR_INVALID_ARG for the whole call, with nothing launched.  n = 0 is RPH_OK.
 *  - A call whose images all share one (w, h, channels, row_stride) goes to the uniform path of rph_pdq_hash_batch(_dev) (the
 *    device form: when the images also lie at one distance from each other, as that path's image_stride wants them).
 *  - Images with both sides 128..512, and larger ones whose <= 512 px thumbnail has both sides >= 128, are hashed by kernels that
 *    take each image's geometry from a descriptor: the number of launches does not depend on the number of geometries.  The
 *    rest (a side < 128, thumbnails thinner than 128, w or h < 5), and every image under rph_pdq_set_kernel modes 0 and 5, go
 *    through rph_pdq_hash_batch_dev in runs of equal geometry.
 */
int rph_pdq_hash_ragged(rph_ctx *ctx, const uint8_t *const *px, const uint32_t *w, const uint32_t *h, const uint32_t *channels,
                        const size_t *row_stride, uint32_t n, uint8_t *hash32_out, float *quality_out, float *coeffs_out,
                        uint8_t *dihedral_out, uint8_t *valid_out);
/* Pixels already on the device: image i starts at (uint8_t *)d_px + offset[i]; the descriptor arrays are HOST arrays
 * (the host plans the call).  Asynchronous on `stream` like rph_pdq_hash_batch_dev; the host arrays may be reused when the
 * call returns. */
int rph_pdq_hash_ragged_dev(rph_ctx *ctx, const void *d_px, const uint64_t *offset, const uint32_t *w, const uint32_t *h,
                            const uint32_t *channels, const size_t *row_stride, uint32_t n, void *d_hash32, void *d_quality,
                            void *d_coeffs, void *d_dihedral, void *d_valid, void *stream);

/*
 * What the scan computes for one decoded image (scanner.rs:1386-1410), for n images of ANY mix of geometries and LAYOUTS in
 * one call: the PDQ outputs and the pixel hash, both from one upload.  load_image_fast returns an image::DynamicImage of any
 * variant; scanner.rs:1393-1404 takes blake3 of its to_rgba16(), scanner.rs:1410 hands it to generate_pdq_features, whose
 * to_luma601 (pdqhash.rs:268-284) borrows Luma8, reads Rgb8 and Rgba8 directly and sends every other variant through to_rgb8().
 *
 * layout[i] = channels + (16-bit samples ? 16 : 0), one of the RPH_LAYOUT_* codes; 1, 3 and 4 mean what `channels` means in
 * rph_pdq_hash_ragged.  Samples are interleaved; 16-bit samples are native little-endian uint16, as in the crate's buffer.
 * Rgb32F / Rgba32F images are not taken.
 *  - hash32_out and pixel_hash32_out are each nullable; both null is RPH_ERR_INVALID_ARG.  With hash32_out null no PDQ kernel
 *    is launched and quality_out, coeffs_out, dihedral_out and valid_out must be null as well.  n = 0 is RPH_OK.
 *  - PDQ: image i's outputs are bit for bit what rph_pdq_hash_ragged returns for the 8-bit hasher pixels of that image ("What
 *    is hashed", PNG section): Luma8, Rgb8 and Rgba8 as they are; LumaA8: the L plane is the luma ((299 l + 587 l + 114 l + 500)
 *    / 1000 = l); Luma16 / LumaA16: luma = (v + 128) / 257; Rgb16 / Rgba16: each sample through (v + 128) / 257, then the 601
 *    luma.  Alpha is ignored.  w[i] or h[i] < 5: valid 0, outputs zeroed (pdqhash.rs:167-169).
 *  - Pixel hash: blake3::hash of to_rgba16() as little-endian bytes for EVERY image, those below 5 px too (the reference hashes
 *    before it looks at the size); w * h = 0 gives the hash of the empty string.  8-bit samples become v * 257, 16-bit samples
 *    stay, gray is replicated into R, G and B, a missing alpha is 65535.  The RGBA16 stream is never written to memory.
 *  - RPH_ERR_INVALID_ARG for the whole call, with nothing launched and no output touched: a layout outside the eight codes,
 *    row_stride[i] < w[i] * bytes per pixel, a 16-bit image whose address (device form: d_px + offset[i]) or row_stride is odd,
 *    w[i] * h[i] > 2^40, a null required pointer (ctx, px / d_px, px[i], offset, w, h, layout, row_stride).
 *  - Images with both sides 128..512, and larger ones whose <= 512 px thumbnail has both sides >= 128, are hashed by the
 *    descriptor-driven kernels of rph_pdq_hash_ragged; images of the five other layouts reach them as Luma8 planes a kernel
 *    writes into scratch.  The rest go through rph_pdq_hash_batch_dev in runs of equal geometry, the five other layouts as
 *    Luma8 read from their planes.  No pixel is converted on the host.
 */
#define RPH_LAYOUT_LUMA8 1
#define RPH_LAYOUT_LUMAA8 2
#define RPH_LAYOUT_RGB8 3
#define RPH_LAYOUT_RGBA8 4
#define RPH_LAYOUT_LUMA16 17
#define RPH_LAYOUT_LUMAA16 18
#define RPH_LAYOUT_RGB16 19
#define RPH_LAYOUT_RGBA16 20
int rph_image_hash_ragged(rph_ctx *ctx, const void *const *px, const uint32_t *w, const uint32_t *h, const uint32_t *layout,
                          const size_t *row_stride, uint32_t n, uint8_t *hash32_out, float *quality_out, float *coeffs_out,
                          uint8_t *dihedral_out, uint8_t *valid_out, uint8_t *pixel_hash32_out);
/* Pixels already on the device: image i starts at (uint8_t *)d_px + offset[i]; the descriptor arrays are HOST arrays,
 * reusable when the call returns.  Asynchronous on `stream`, exactly like rph_pdq_hash_ragged_dev. */
int rph_image_hash_ragged_dev(rph_ctx *ctx, const void *d_px, const uint64_t *offset, const uint32_t *w, const uint32_t *h,
                              const uint32_t *layout, const size_t *row_stride, uint32_t n, void *d_hash32, void *d_quality,
                              void *d_coeffs, void *d_dihedral, void *d_valid, void *d_pixel_hash32, void *stream);
/* Context-free host restatements of the two rules above, no GPU call (like rph_blake3_host, rph_png_decode_host): the Luma8
 * plane the hasher sees (luma_out: w * h bytes, rows packed) and the pixel hash of one image.  RPH_ERR_INVALID_ARG as above. */
int rph_image_luma601_host(const void *px, uint32_t w, uint32_t h, uint32_t layout, size_t row_stride, uint8_t *luma_out);
int rph_image_pixel_hash_host(const void *px, uint32_t w, uint32_t h, uint32_t layout, size_t row_stride, uint8_t *digest32_out);

/*
 * generate_pdq_features for ONE image, as scanner.rs:1410 calls it from many rayon workers at once: thread-safe and
 * blocking; concurrent callers are coalesced into GPU batches (images of any mix of sizes) whose transfers are pipelined
 * over three slots.  A batch goes as soon as nobody is still copying into it and a pipeline slot is free, so its size
 * follows the load; `max_batch` (default 256) bounds it, `max_wait_us` (default 0) optionally holds a non-full batch back
 * for more callers.  Same outputs as rph_pdq_hash_batch with n = 1.
 */
int rph_pdq_hash_one(rph_ctx *ctx, const uint8_t *px, uint32_t w, uint32_t h, uint32_t channels, size_t row_stride,
                     uint8_t *hash32_out, float *quality_out, float *coeffs_out, uint8_t *valid_out);
int rph_pdq_batcher_config(rph_ctx *ctx, uint32_t max_batch, uint32_t max_wait_us);
int rph_pdq_batcher_stats(rph_ctx *ctx, uint64_t *n_batches_out, uint64_t *n_images_out);

/* PdqFeatures::to_hash (pdqhash.rs:59-61) and generate_dihedral_hashes (:71-87)
 * for n stored coefficient vectors (n x 256 floats), e.g. features read back
 * from the cache (scanner.rs:1270-1272).  hash32_out / dihedral_out nullable. */
int rph_pdq_hashes_from_coeffs(rph_ctx *ctx, const float *coeffs, uint32_t n, uint8_t *hash32_out,
                               uint8_t *dihedral_out);
int rph_pdq_hashes_from_coeffs_dev(rph_ctx *ctx, const void *d_coeffs, uint32_t n, void *d_hash32,
                                   void *d_dihedral, void *stream);

/* PdqFeatures::to_hash (pdqhash.rs:59-61) and generate_dihedral_hashes (:71-87) for ONE coefficient vector, on the host:
 * compare + bit operations only, no GPU call, no context.  This is what the reference's per-file call sites bind
 * (scanner.rs:1412 `f.to_hash()`, :1622 and :2223 `features.generate_dihedral_hashes()`); same bits as the batch kernels. */
void rph_pdq_to_hash(const float *coeffs256, uint8_t *hash32_out);
void rph_pdq_dihedral_one(const float *coeffs256, uint8_t *out8x32);

/* Which PDQ kernels a context uses.  512x512 RGB8 / Luma8: 0 = generic multi-pass (any geometry), 1 = fused single-pass, one wave
 * per image, 64-px strips (8 waves per CU: the throughput kernel, ~0.3 ms per image however few there are), 2 = the same
 * with 128-px strips (cache-line aligned loads, 6 waves per CU), 3 = fused low-latency form (eight waves share an image:
 * ~60 us, one image per CU), 4 = automatic (default): 3 below 768 images per call, 1 from there.  Every other geometry of
 * 128..512 px (thumbnails behind the pre-downsample included): the streaming single-pass kernel (one wave per image) from 384
 * images per call, below that the multi-pass kernels (rows through LDS tiles); 6 = as 4 with the streaming kernel at every
 * batch size (tests); 5 = no single-pass kernel at all: the multi-pass kernels (0 = their plain one-thread-per-line form,
 * which also selects the two-pass pre-downsample).  All produce identical bits.  Debug/bench. */
int rph_pdq_set_kernel(rph_ctx *ctx, int which);

/* calculate_target_dimensions (pdqhash.rs:224-235): integer geometry, host. */
void rph_pdq_target_dimensions(uint32_t w, uint32_t h, uint32_t max_dim, uint32_t *new_w, uint32_t *new_h);

/* =====================================================================
 * Hamming distance, all-pairs sweep, grouping  (reference: src/hamminghash.rs,
 * src/scanner.rs:1588-1823)
 * ===================================================================== */

/* HammingHash::hamming_distance for [u8;32] (hamminghash.rs:56-58) and u64 (:34-36);
 * HammingHash::get_chunk (:29-31, :50-53).  Scalar integer helpers, host. */
uint32_t rph_hamming_distance256(const uint8_t *a32, const uint8_t *b32);
uint32_t rph_hamming_distance64(uint64_t a, uint64_t b);
uint16_t rph_get_chunk256(const uint8_t *h32, uint32_t chunk_idx);
uint16_t rph_get_chunk64(uint64_t h, uint32_t chunk_idx);

/* Which formulation the sweep's fast path uses: 2 = fp4 MFMA (default: bits as e2m1 +-1; plain all-pairs sweeps of >= 32768
 * hashes run on a popcount-sorted copy with bits as {0, 1}, which the power-limited chip clocks ~10 % higher), 3 = fp4 MFMA with
 * +-1 operands everywhere, 4 = the sorted {0, 1} form at every size (tests), 1 = int8 MFMA, 0 = VALU xor + popcount.  All feed the same exact completion and report the same edge
 * set.  Debug/bench.  Cross sweeps (rph_hamming_cross_pairs ...) have no sorted {0, 1} form -- it sorts one array and needs
 * rows == columns -- so settings 2, 3 and 4 all select the +-1 fp4 form there; 1 and 0 as above. */
int rph_hamming_set_kernel(rph_ctx *ctx, int which);
/* Width (in 32-bit words, 4..8) of the hash prefix the sweep's fast path examines for `threshold` under formulation `kernel`
 * (as in rph_hamming_set_kernel).  Informational (bench.py prices the fast path with it): results never depend on it. */
int rph_hamming_prefix_dwords(uint32_t threshold, int kernel);

/* One reported pair of the all-pairs sweep. */
typedef struct rph_edge {
    uint32_t i, j;  /* i < j (indices into the hash array; for variant sweeps i is the owning file); cross sweeps: i in A, j in B */
    uint16_t d;     /* Hamming distance, <= threshold */
    uint16_t flags; /* RPH_EDGE_* */
} rph_edge;
#define RPH_EDGE_MIH_R1 0x8000u      /* pair is reachable by find_groups' R<=1 probing (hamminghash.rs:206-238) */
#define RPH_EDGE_PROBE_MASK 0x01FFu  /* (first chunk k << 5) | probe slot: 0 = exact bucket, 1+b = flip of bit b */
#define RPH_EDGE_VARIANT_SHIFT 9     /* variant sweeps: bits 9..11 = dihedral slot that matched */
#define RPH_EDGE_VARIANT_MASK 0x0E00u

/*
 * All-pairs 256-bit sweep: every pair i<j of `hashes32` (n x 32 bytes) with
 * hamming_distance <= threshold (0..256), the exact counterpart of the
 * candidate generation of group_files_generic (scanner.rs:1704-1767, exact for
 * threshold <= 63) and, with RPH_EDGE_MIH_R1, of find_groups (hamminghash.rs:206-238).
 * Edges are written unordered; *n_edges_out always receives the total found; at
 * most `cap` are stored (RPH_ERR_CAPACITY if more were found).
 * part/nparts shard the upper-triangular tile pairs round-robin (multi-GPU:
 * rank r of N passes part=r, nparts=N; single GPU 0,1).
 */
int rph_hamming_all_pairs(rph_ctx *ctx, const uint8_t *hashes32, uint64_t n, uint32_t threshold,
                          uint32_t part, uint32_t nparts, rph_edge *edges, uint64_t cap,
                          uint64_t *n_edges_out);
/* d_count: device uint64 cursor, zeroed by the caller before the first shard. */
int rph_hamming_all_pairs_dev(rph_ctx *ctx, const void *d_hashes32, uint64_t n, uint32_t threshold,
                              uint32_t part, uint32_t nparts, void *d_edges, uint64_t cap,
                              void *d_count, void *stream);

/*
 * Variant sweep of group_files_generic + PdqStrategy (scanner.rs:1607-1637,
 * 1678-1776): rows are the 8 dihedral hashes of every file (n x 8 x 32 bytes,
 * or n x 1 x 32 when n_variants == 1), columns the plain hashes; an edge
 * (i, j, d, variant) is reported for every variant v of file i and every j > i
 * with hamming_distance(variant_v(i), hash(j)) <= limit(i, j), where
 * limit = 0 if low_conf[i] or low_conf[j] (scanner.rs:1699,1721) else `similarity`.
 * low_conf nullable (all 0).  The multiset of (i, j) equals the reference's edge
 * list (its comparison_count, scanner.rs:1778).
 */
int rph_hamming_variant_pairs(rph_ctx *ctx, const uint8_t *variants, uint32_t n_variants,
                              const uint8_t *hashes32, const uint8_t *low_conf, uint64_t n,
                              uint32_t similarity, uint32_t part, uint32_t nparts, rph_edge *edges,
                              uint64_t cap, uint64_t *n_edges_out);
int rph_hamming_variant_pairs_dev(rph_ctx *ctx, const void *d_variants, uint32_t n_variants,
                                  const void *d_hashes32, const void *d_low_conf, uint64_t n,
                                  uint32_t similarity, uint32_t part, uint32_t nparts, void *d_edges,
                                  uint64_t cap, void *d_count, void *stream);

/*
 * Cross sweeps: set A against a DIFFERENT set B (new files against a library, queries against a resident collection, two
 * collections against each other) without the pairs inside either set.  Every pair (a, b) with
 * hamming_distance(variant_v(a), hash(b)) <= limit(a, b) is reported, e.i indexing A and e.j indexing B; there is no i < j rule,
 * so a hash present in both sets at the same index is reported as (k, k).  limit = 0 if low_conf_a[a] or low_conf_b[b], else
 * the threshold; both flag arrays nullable.  flags as in the square sweeps (variant slot, RPH_EDGE_MIH_R1 and the probe key: all
 * symmetric in the pair).  Capacity protocol as above: the total is always reported, RPH_ERR_CAPACITY if it exceeds `cap`.
 * n_a == 0 or n_b == 0: RPH_OK, no edges; either count above 2^32 - 1: RPH_ERR_INVALID_ARG.  part/nparts shard the blocks of the
 * (row tile x column segment) rectangle round-robin: the parts are disjoint and their union is the whole edge set.
 */
int rph_hamming_cross_pairs(rph_ctx *ctx, const uint8_t *a32, uint64_t n_a, const uint8_t *b32, uint64_t n_b,
                            uint32_t threshold, uint32_t part, uint32_t nparts, rph_edge *edges, uint64_t cap,
                            uint64_t *n_edges_out);
int rph_hamming_cross_pairs_dev(rph_ctx *ctx, const void *d_a32, uint64_t n_a, const void *d_b32, uint64_t n_b,
                                uint32_t threshold, uint32_t part, uint32_t nparts, void *d_edges, uint64_t cap,
                                void *d_count, void *stream);
/* variants_a: n_a x n_variants x 32 bytes (n_variants 1 or 8), hashes_b: n_b x 32 bytes. */
int rph_hamming_variant_cross_pairs(rph_ctx *ctx, const uint8_t *variants_a, uint32_t n_variants,
                                    const uint8_t *low_conf_a, uint64_t n_a, const uint8_t *hashes_b,
                                    const uint8_t *low_conf_b, uint64_t n_b, uint32_t similarity, uint32_t part,
                                    uint32_t nparts, rph_edge *edges, uint64_t cap, uint64_t *n_edges_out);
int rph_hamming_variant_cross_pairs_dev(rph_ctx *ctx, const void *d_variants_a, uint32_t n_variants,
                                        const void *d_low_conf_a, uint64_t n_a, const void *d_hashes_b,
                                        const void *d_low_conf_b, uint64_t n_b, uint32_t similarity, uint32_t part,
                                        uint32_t nparts, void *d_edges, uint64_t cap, void *d_count, void *stream);

/*
 * find_groups::<[u8;32]> (hamminghash.rs:191-271), bit-exact including member
 * order: adjacency = pairs with d <= max_dist that R<=1 probing reaches, in
 * first-seen order, then the serial greedy star clustering.
 * members: capacity n; offsets: capacity n/2 + 2; group g = members[offsets[g] .. offsets[g+1]).
 */
int rph_find_groups256(rph_ctx *ctx, const uint8_t *hashes32, uint64_t n, uint32_t max_dist,
                       uint32_t *members, uint32_t *offsets, uint32_t *n_groups_out);
/* impl HammingHash for u64 (hamminghash.rs:23-41): all-pairs sweep over 64-bit hashes (pHash) and find_groups::<u64>
 * (8 chunks of 8 bits, chunk tolerance max_dist / 8), same edge / group conventions as the 256-bit forms. */
int rph_hamming_all_pairs64(rph_ctx *ctx, const uint64_t *hashes64, uint64_t n, uint32_t threshold, uint32_t part,
                            uint32_t nparts, rph_edge *edges, uint64_t cap, uint64_t *n_edges_out);
int rph_hamming_all_pairs64_dev(rph_ctx *ctx, const void *d_hashes64, uint64_t n, uint32_t threshold, uint32_t part,
                                uint32_t nparts, void *d_edges, uint64_t cap, void *d_count, void *stream);
int rph_find_groups64(rph_ctx *ctx, const uint64_t *hashes64, uint64_t n, uint32_t max_dist, uint32_t *members,
                      uint32_t *offsets, uint32_t *n_groups_out);
/* Same from a precomputed edge list (e.g. gathered from several GPUs). */
int rph_find_groups_from_edges(const rph_edge *edges, uint64_t n_edges, uint64_t n,
                               uint32_t *members, uint32_t *offsets, uint32_t *n_groups_out);

/*
 * group_files_generic with PdqStrategy (scanner.rs:1640-1823) up to and
 * including the union-find (merge_groups_by_stem / process_raw_groups are
 * file-name logic and stay in the caller; the one data-parallel step of
 * process_raw_groups, max_dist, is rph_group_max_dist below).
 *   hashes32 n x 32; coeffs n x 256 floats or NULL (then every file has the one
 *   variant out[0] = hash, scanner.rs:1624-1627); has_features n bytes or NULL
 *   (all 1 when coeffs != NULL); quality n x int32, <0 = None (scanner.rs:1592), or NULL.
 * similarity must be <= RPH_MAX_SIMILARITY_256 (scanner.rs:1650-1655) else RPH_ERR_INVALID_ARG.
 * Outputs: connected components with > 1 member: members ascending inside a
 * group (scanner.rs:1810-1814), groups ordered by first member (the reference's
 * HashMap order is unspecified); *comparison_count_out = number of edges
 * (scanner.rs:1778).  members capacity n, offsets capacity n/2 + 2.
 */
int rph_group_files_pdq(rph_ctx *ctx, const uint8_t *hashes32, const float *coeffs,
                        const uint8_t *has_features, const int32_t *quality, uint64_t n,
                        uint32_t similarity, uint32_t *members, uint32_t *offsets,
                        uint32_t *n_groups_out, uint64_t *comparison_count_out);
/* Union-find part alone (scanner.rs:1781-1817) over an edge list. */
int rph_union_find_groups(const rph_edge *edges, uint64_t n_edges, uint64_t n, uint32_t *members,
                          uint32_t *offsets, uint32_t *n_groups_out);

/*
 * Incremental rph_group_files_pdq: a library of n_old files that an earlier call grouped (old_members / old_offsets /
 * n_old_groups exactly as that call returned them) plus n_new new files.  Files are numbered as the concatenation: library
 * 0 .. n_old-1, new n_old .. n_old+n_new-1.  Only the pairs the new files add are swept -- (library variants x new hashes) by the
 * cross sweep, (new variants x new hashes, i < j) by the triangular one -- and the union-find starts from the old components.
 * members / offsets / *n_groups_out are identical to rph_group_files_pdq on the concatenated arrays;
 * *new_comparisons_out = that call's comparison count minus the library's own.
 * Per side, the nullable arguments are those of rph_group_files_pdq: coeffs NULL = that side has one variant per file;
 * has_features only counts next to coeffs; quality NULL = no low-confidence files on that side.
 * members capacity n_old + n_new, offsets capacity (n_old + n_new) / 2 + 2.  Malformed old groups: RPH_ERR_INVALID_ARG.
 */
int rph_group_files_pdq_append(rph_ctx *ctx, const uint8_t *old_hashes32, const float *old_coeffs,
                               const uint8_t *old_has_features, const int32_t *old_quality, uint64_t n_old,
                               const uint32_t *old_members, const uint32_t *old_offsets, uint32_t n_old_groups,
                               const uint8_t *new_hashes32, const float *new_coeffs, const uint8_t *new_has_features,
                               const int32_t *new_quality, uint64_t n_new, uint32_t similarity, uint32_t *members,
                               uint32_t *offsets, uint32_t *n_groups_out, uint64_t *new_comparisons_out);
/* Its host part alone: union-find over n_total files that starts from the groups of an earlier call and adds `edges`.  The old
 * groups are checked (a member >= n_total, a member listed twice, offsets that do not start at 0 or are not ascending:
 * RPH_ERR_INVALID_ARG); nothing is written outside members[0 .. n_total) and offsets[0 .. n_total / 2 + 2). */
int rph_union_find_groups_append(const uint32_t *old_members, const uint32_t *old_offsets, uint32_t n_old_groups,
                                 const rph_edge *edges, uint64_t n_edges, uint64_t n_total, uint32_t *members,
                                 uint32_t *offsets, uint32_t *n_groups_out);

/*
 * The union-find on the device (scanner.rs:1781-1817), over an edge list that a sweep left there.
 * d_labels: n uint32, in/out.  On entry a forest with d_labels[x] <= x (identity for a fresh set; the labels an earlier call left).
 * Every edge e of d_edges[0 .. n_edges) unites e.i + i_base and e.j + j_base.  On exit d_labels[x] is the SMALLEST index of x's
 * component, for every x (flattened); the result does not depend on the order of the edges.  An edge that names a file >= n, or a
 * label above its file: RPH_ERR_INVALID_ARG, labels untouched.  n at most 2^31 - 1.  The call waits for its range check (it
 * synchronises `stream` once); the unions and the flattening are asynchronous on `stream`.
 */
int rph_union_find_labels_dev(rph_ctx *ctx, const void *d_edges, uint64_t n_edges, uint32_t i_base, uint32_t j_base,
                              void *d_labels, uint64_t n, void *stream);
/* Flattened labels -> the groups of rph_union_find_groups: components with > 1 member, members ascending inside a group, groups
 * ordered by first member.  members / offsets are host arrays of capacity n and n / 2 + 2.  Labels that are not flattened
 * min-labels (label[x] > x, or label[label[x]] != label[x]) and n above 2^31 - 1: RPH_ERR_INVALID_ARG. */
int rph_groups_from_labels_dev(rph_ctx *ctx, const void *d_labels, uint64_t n, uint32_t *members, uint32_t *offsets,
                               uint32_t *n_groups_out, void *stream);

/*
 * A grouped library that stays on the device: hashes, the 8 variant rows of every file, flags and component labels live in HBM
 * between calls (294 bytes per file), so that an append moves and sweeps the new files only and a query moves the queries only.
 * The result is rph_group_files_pdq on the files it holds, in order.  One similarity per library; at most 2^31 - 1 files;
 * files leave through rph_library_remove, which renumbers the ones that stay.  One library serves one call at a time (calls
 * from several threads queue); several libraries on one context are independent.  Destroy every library before rph_shutdown
 * of its context.
 */
typedef struct rph_library rph_library;
int rph_library_create(rph_ctx *ctx, uint32_t similarity, rph_library **lib_out);   /* similarity > RPH_MAX_SIMILARITY_256: RPH_ERR_INVALID_ARG */
int rph_library_destroy(rph_library *lib);
int rph_library_reserve(rph_library *lib, uint64_t n_files);                        /* room for n_files without another growth */
int rph_library_size(rph_library *lib, uint64_t *n_files_out, uint64_t *comparisons_out);
/* The new files become n .. n + n_new - 1.  Arguments per file as rph_group_files_pdq: coeffs NULL = these files have no features
 * (has_features 0, one variant: scanner.rs:1624-1627); has_features only counts next to coeffs; quality NULL = none low-confidence.
 * labels_out (nullable, n_new): for each new file the smallest index of the component it is in now (its own index if it is alone).
 * All or nothing: an error (a null argument, the 2^31 - 1 limit, an edge list that kept growing, an allocation that failed) leaves
 * size, labels and comparison count as they were.  Excepted: a HIP call that fails once the unions have been launched (RPH_ERR_HIP, a
 * device lost to the context) leaves size and count, but resident labels may already be merged.  n_new == 0: RPH_OK, nothing changes. */
int rph_library_append(rph_library *lib, const uint8_t *hashes32, const float *coeffs, const uint8_t *has_features,
                       const int32_t *quality, uint64_t n_new, uint32_t *labels_out, uint64_t *new_comparisons_out);
/* Start from what an earlier run kept: files plus their groups as rph_group_files_pdq / _append / rph_library_groups returned them, for the
 * SAME similarity; no sweep.  Only on an empty library.  The groups are checked as rph_union_find_groups_append checks them. */
int rph_library_restore(rph_library *lib, const uint8_t *hashes32, const float *coeffs, const uint8_t *has_features,
                        const int32_t *quality, uint64_t n, const uint32_t *members, const uint32_t *offsets, uint32_t n_groups,
                        uint64_t comparisons);
/* Remove files (deleted duplicates, files gone at the next scan).  indices: n_remove current file numbers in any order.  The files that
 * stay keep their order and are renumbered densely: new number = old number - removed files below it; new_index_out (nullable, one entry
 * per file of the OLD size) gives the new number of every old file, 0xFFFFFFFF for a removed one -- the caller renumbers whatever it keeps
 * by file number through it.  Afterwards the library is what rph_group_files_pdq gives on the remaining files in order: groups, labels,
 * queries, every later append, and the comparison count, which goes down by the edges that had a removed file at either end
 * (*dropped_comparisons_out, nullable; a count restored too low stops at 0).  A union-find does not split, so the components that lost a
 * file are regrouped: their members are swept again among themselves and everything else keeps its labels.  The cost is one pass over the
 * resident arrays plus 8 * m^2 / 2 pairs for m members of such components -- a full regroup when one component holds the library.
 * Memory: the new state is built beside the old one, so for the length of the call a second copy of the library is allocated (294 bytes x
 * capacity, which does not shrink) plus 290 bytes per regrouped member and 16 per resident file of work space, which are kept.
 * All or nothing, with no exception: a null indices with n_remove > 0, an index >= size or an index listed twice (RPH_ERR_INVALID_ARG), an
 * allocation or a HIP call that fails -- each leaves groups, labels, size and count exactly as they were.  n_remove == 0: RPH_OK, nothing
 * changes.  Removing every file leaves an empty library that rph_library_restore accepts. */
int rph_library_remove(rph_library *lib, const uint32_t *indices, uint64_t n_remove, uint32_t *new_index_out,
                       uint64_t *dropped_comparisons_out);
/* members capacity size, offsets capacity size / 2 + 2: identical to rph_group_files_pdq on the files the library holds, in order. */
int rph_library_groups(rph_library *lib, uint32_t *members, uint32_t *offsets, uint32_t *n_groups_out);
/* first + count <= size */
int rph_library_labels(rph_library *lib, uint64_t first, uint64_t count, uint32_t *labels_out);
/* The library is not changed: every (library file i, variant v, query j) with d(variant_v(i), hash_q(j)) <= limit, the edge convention and
 * capacity protocol of rph_hamming_variant_cross_pairs (e.i library, e.j query); quality_q nullable. */
int rph_library_query(rph_library *lib, const uint8_t *hashes32_q, const int32_t *quality_q, uint64_t n_q, rph_edge *edges,
                      uint64_t cap, uint64_t *n_edges_out);
/* An edge-keeping library: beside everything above it holds, on the device, every edge the variant sweep at `top` reports among the
 * resident files -- one rph_edge per passing variant exactly as rph_hamming_variant_pairs emits them, in the library's current numbering
 * with i < j, in no particular order, 12 bytes each.  With that store rph_library_merge_tree(lib, t <= top) runs no sweep, so the
 * similarity can change, or the groups at every similarity be counted, for milliseconds after every append and removal.
 * similarity <= top <= RPH_MAX_SIMILARITY_256, else RPH_ERR_INVALID_ARG.  max_edges bounds the store; 0 means 2^28 edges (3 GiB).
 * In every call above such a library gives what rph_library_create(ctx, similarity) gives when fed the same calls: its groups are the
 * union-find of the stored edges with d <= similarity, its comparison count their number (the sweep at s reports exactly the edges with
 * d <= s of the sweep at top: see "Merge tree").  What differs:
 *  - an append sweeps at `top` (more edges than at `similarity`, and above 31 the slower sweep kernel).  One that would take the store
 *    past max_edges is RPH_ERR_CAPACITY and, as every refused append, leaves size, labels, count and store as they were.  The store
 *    grows geometrically; while it grows the old and the new allocation exist together.
 *  - a removal also filters the store into a second one, which then replaces it: for the length of the call a second store of the same
 *    capacity is allocated.  Still all or nothing.  The edges it drops within `similarity` must be the number the regroup counted; if
 *    they are not (a store restored from edges that are not the files' own), RPH_ERR_HIP with both numbers and nothing changed.
 *  - rph_library_restore is RPH_ERR_INVALID_ARG: groups alone cannot fill a store.  Use rph_library_restore_edges. */
#define RPH_NO_EDGE_STORE 0xFFFFFFFFu
int rph_library_create_tree(rph_ctx *ctx, uint32_t similarity, uint32_t top, uint64_t max_edges, rph_library **lib_out);
/* Any output may be NULL.  *top_out: the store's top, RPH_NO_EDGE_STORE for a library made by rph_library_create (the counts are 0
 * then); *n_edges_out: the edges the store holds; *capacity_out: the most it may hold (max_edges). */
int rph_library_edge_info(rph_library *lib, uint32_t *top_out, uint64_t *n_edges_out, uint64_t *capacity_out);
/* The store, downloaded.  *n_edges_out always receives the count; the records are written only if cap suffices, else RPH_ERR_CAPACITY
 * with nothing written.  A library without a store: RPH_ERR_INVALID_ARG. */
int rph_library_edges(rph_library *lib, rph_edge *edges_out, uint64_t cap, uint64_t *n_edges_out);
/* Start an empty edge-keeping library from files plus the edges an earlier run downloaded from a library of the same top: no sweep.
 * The labels are the union-find of the edges with d <= similarity (which may differ from the earlier run's), the comparison count
 * their number.  The edges are the caller's word: each is checked for i < j < n and d <= top before anything is stored -- a violation
 * is RPH_ERR_INVALID_ARG and the library stays empty -- and they are never trusted for indexing, but whether they are the files' edges
 * is not checked.  A library that is not empty or has no store: RPH_ERR_INVALID_ARG. */
int rph_library_restore_edges(rph_library *lib, const uint8_t *hashes32, const float *coeffs, const uint8_t *has_features,
                              const int32_t *quality, uint64_t n, const rph_edge *edges, uint64_t n_edges);

/*
 * max_dist of every group (process_raw_groups -> analyze_group_with_features, scanner.rs:1986-2022 and :2214-2241): the maximum, over the
 * group's members, of the minimum Hamming distance to the rows of the group's pivot file.  One rule for every form below.
 *   Group g is members[offsets[g] .. offsets[g + 1]) in the caller's order (the reference sorts a group by file name first: that stays
 *   with the caller), over n files.  pivots[g] is a file number or RPH_NO_PIVOT; a pivot need not be a member of its group, a file may be
 *   listed more than once, groups of one member and empty groups are legal.
 *   dist(m) = min over the pivot's rows of hamming256(row, hash[m]).  The rows of a pivot WITH features are its 8 dihedral hashes, exactly
 *   what rph_pdq_hashes_from_coeffs gives for its coefficients; the rows of a pivot without are its hash alone.  "With features":
 *   coeffs != NULL and has_features is NULL or 1 for that file.
 *   max_dist_out[g] (n_groups x uint32, required) = max of dist over the listed members; member_dist_out (nullable) gets dist for every
 *   member slot.  An empty group or RPH_NO_PIVOT gives max_dist 0 and member_dist 0 in that group's slots.
 *   pivots == NULL selects the reference's find_map pair (scanner.rs:2219-2232): the first listed member that has features, else the
 *   first listed member.
 * RPH_ERR_INVALID_ARG with NO output written: offsets[0] != 0, offsets that do not ascend, a member >= n, a pivot >= n that is not
 * RPH_NO_PIVOT, a null required argument.  n_groups == 0: RPH_OK.  n at most 2^32 - 2.
 */
#define RPH_NO_PIVOT 0xFFFFFFFFu
/* On the host, no context: the pivots' rows through rph_pdq_dihedral_one.  The rule's restatement for callers' own tests and the
 * fallback without a device, like rph_image_luma601_host. */
int rph_group_max_dist_host(const uint8_t *hashes32, const float *coeffs, const uint8_t *has_features, uint64_t n,
                            const uint32_t *members, const uint32_t *offsets, uint32_t n_groups, const uint32_t *pivots,
                            uint32_t *max_dist_out, uint32_t *member_dist_out);
/* Host arrays in, host arrays out: the hashes cross PCIe, and of the coefficients only the pivots' rows (in bounded pieces). */
int rph_group_max_dist(rph_ctx *ctx, const uint8_t *hashes32, const float *coeffs, const uint8_t *has_features, uint64_t n,
                       const uint32_t *members, const uint32_t *offsets, uint32_t n_groups, const uint32_t *pivots,
                       uint32_t *max_dist_out, uint32_t *member_dist_out);
/* The core, everything on the device.  d_hashes32: n x 32.  row_mode says what d_rows holds: RPH_ROWS_NONE nothing (plain distance to
 * hash[pivot], d_rows ignored), RPH_ROWS_PER_GROUP n_groups x 8 x 32 bytes (block g: the rows of pivot g), RPH_ROWS_PER_FILE n x 8 x 32
 * bytes (the library's layout).  d_has_features (n bytes, nullable; it only counts next to rows, as has_features next to coeffs): a pivot
 * with 0 there has its hash as its only row whatever d_rows holds.  d_hashes32 and d_rows are read 16 bytes at a time and must be aligned so.  d_members holds d_offsets[n_groups] entries,
 * d_offsets n_groups + 1.  d_pivots nullable: the default pair is then resolved on the device from d_has_features (if that is null too:
 * the first listed member).  The device arrays are range-checked by a pass of their own before anything is read through them -- the call
 * waits for that (it synchronises `stream` once) and a bad index is RPH_ERR_INVALID_ARG, never a read out of range; the rest is
 * asynchronous on `stream`.  d_member_dist nullable. */
#define RPH_ROWS_NONE 0
#define RPH_ROWS_PER_GROUP 1
#define RPH_ROWS_PER_FILE 2
int rph_group_max_dist_dev(rph_ctx *ctx, const void *d_hashes32, uint64_t n, const void *d_rows, int row_mode,
                           const void *d_has_features, const void *d_members, const void *d_offsets, uint32_t n_groups,
                           const void *d_pivots, void *d_max_dist, void *d_member_dist, void *stream);
/* Against the files a library holds (their hashes, variant rows and flags never leave the device): host group arrays in the library's
 * current numbering, e.g. what rph_library_groups returned, re-ordered by the caller as it likes; checked on the host against the
 * library's size.  The library is not changed. */
int rph_library_group_max_dist(rph_library *lib, const uint32_t *members, const uint32_t *offsets, uint32_t n_groups,
                               const uint32_t *pivots, uint32_t *max_dist_out, uint32_t *member_dist_out);

/*
 * The nearest files of a query: exact top-k Hamming search.  One rule for every form below; no threshold sweep, no capacity protocol --
 * the output is n_q x k slots whatever the data holds.
 *   Library side: n_lib files of n_variants (1 or 8) rows of 32 bytes, rows[n_lib][n_variants][32].  has_features (n_lib bytes,
 *   nullable): a file whose byte is 0 owns row 0 only, whatever its other rows hold (the convention of the variant sweeps).
 *   Query side: n_q hashes of 32 bytes.  skip (n_q x uint32, nullable): query q never reports library file skip[q]; RPH_NO_FILE skips
 *   nothing.
 *   dist(i, q) = min over the rows file i owns of hamming256(row, hash_q); variant(i, q) = the smallest row index that attains it.
 *   Quality and low confidence play no part: this is a distance query, not the grouping rule.
 *   Result of query q: the library files with i != skip[q] and dist(i, q) <= max_dist, ordered by the key (dist, i) ascending, the
 *   first k of them.  max_dist >= 256 means no cutoff.  Ties in distance go to the smaller file number, so the result is unique: it
 *   does not depend on launch geometry, on how the library is cut into segments or on the order in which anything was found.
 *   out: n_q x k rph_edge.  Slot (q, r) holds the r-th entry: e.i = library file, e.j = q, e.d = distance (0..256),
 *   e.flags = variant << RPH_EDGE_VARIANT_SHIFT.  Slots behind the end of the list are {RPH_NO_FILE, q, 0xFFFF, 0}.  counts_out
 *   (nullable, n_q x uint32): the number of filled slots.
 * k in 1 .. RPH_NEAREST_MAX_K, n_lib at most 2^32 - 2.  RPH_ERR_INVALID_ARG with NO output written: a k outside that range, an
 * n_variants other than 1 or 8, an n_lib above the limit, a null required pointer with a non-zero count.  n_q == 0: RPH_OK.
 * n_lib == 0: RPH_OK, every slot empty, counts 0.
 * rph_hamming_set_kernel selects nothing here: there is one kernel (the full 256-bit distance of every pair on the fp4 matrix pipe,
 * a running list of the k best per query and library segment, one merge per query).
 */
#define RPH_NO_FILE 0xFFFFFFFFu
#define RPH_NEAREST_MAX_K 64
/* On the host, no context and no device: the rule's restatement for callers' own tests and the fallback, like rph_group_max_dist_host
 * (the queries are spread over the host's threads). */
int rph_hamming_nearest_host(const uint8_t *rows, uint32_t n_variants, const uint8_t *has_features, uint64_t n_lib,
                             const uint8_t *hashes32_q, const uint32_t *skip, uint64_t n_q, uint32_t k, uint32_t max_dist,
                             rph_edge *out, uint32_t *counts_out);
/* Host arrays in, host arrays out: rows, flags and queries cross PCIe, the slots come back. */
int rph_hamming_nearest(rph_ctx *ctx, const uint8_t *rows, uint32_t n_variants, const uint8_t *has_features, uint64_t n_lib,
                        const uint8_t *hashes32_q, const uint32_t *skip, uint64_t n_q, uint32_t k, uint32_t max_dist, rph_edge *out,
                        uint32_t *counts_out);
/* The core, everything on the device and asynchronous on `stream`.  d_rows and d_hashes_q are read 16 bytes at a time and must be
 * aligned so.  The partial lists live in the context's kept scratch, at most 256 MiB of it: the queries are taken in chunks. */
int rph_hamming_nearest_dev(rph_ctx *ctx, const void *d_rows, uint32_t n_variants, const void *d_has_features, uint64_t n_lib,
                            const void *d_hashes_q, const void *d_skip, uint64_t n_q, uint32_t k, uint32_t max_dist, void *d_out,
                            void *d_counts, void *stream);
/* Against the files a library holds (8 rows each, with their flags, where they lie): only the queries go up and the slots come down.
 * The library is not changed; e.i is in its current numbering. */
int rph_library_nearest(rph_library *lib, const uint8_t *hashes32_q, uint64_t n_q, uint32_t k, uint32_t max_dist, rph_edge *out,
                        uint32_t *counts_out);
/* The queries are resident files, indices[q] in the library's current numbering: their hashes are gathered on the device, each with
 * skip = itself ("the neighbours of file 4711" without a hash ever being on the host).  An index >= size: RPH_ERR_INVALID_ARG with
 * nothing written. */
int rph_library_nearest_files(rph_library *lib, const uint32_t *indices, uint64_t n_q, uint32_t k, uint32_t max_dist, rph_edge *out,
                              uint32_t *counts_out);

/*
 * Merge tree: the groups at EVERY similarity 0 .. top from one sweep at top.  The grouping of group_files_generic (scanner.rs:1640-1817)
 * is connected components over the pairs within the limit -- single linkage -- so the groups at the similarities 0 .. top are nested, and
 * one record per file holds them all.  One rule for every form below.
 *   Files are 0 .. n-1; the arguments per file are those of rph_group_files_pdq (hashes32, nullable coeffs, has_features, quality).
 *   For i < j, with the rows file i owns as the reference has them (scanner.rs:1692-1701: its 8 dihedral hashes if it has features, else
 *   its hash): w(i, j) = min over those rows of hamming256(row, hash[j]).  lvl(i, j) = w(i, j) if neither file is low-confidence; if
 *   either is, lvl(i, j) = 0 when w == 0 and the pair has no edge otherwise (scanner.rs:1699, 1721).
 *   For 0 <= s <= top the components at s are the connected components of the pairs with lvl <= s, and label_s[x] is the smallest file
 *   number of x's component: what rph_group_files_pdq(similarity = s) yields.
 *   The tree is two arrays of n entries:
 *     level[x] (uint8)  = the smallest s <= top with label_s[x] != x, or RPH_TREE_NEVER if there is none;
 *     into[x]  (uint32) = label_{level[x]}[x], or x if level[x] is RPH_TREE_NEVER.
 *   So into[x] < x whenever level[x] is not RPH_TREE_NEVER; level[into[x]] > level[x], strictly, or RPH_TREE_NEVER, so a chain has at most
 *   top + 1 links (64 for the PDQ forms); label_s[x] is found by following `into` while level[current] <= s.  The tree is unique: it does
 *   not depend on the order of the edges, on launch geometry or on which of several equal-weight edges did a merge, and every form
 *   returns identical bytes.
 *   edges_at[t], t = 0 .. top (uint64): the number of edges with d == t that the variant sweep at similarity `top` reports, one per
 *   passing variant as in rph_hamming_variant_pairs.  The sweep at s reports exactly those with d <= s (a low-confidence pair only
 *   ever d = 0), so the sum of edges_at[0 .. s] is rph_group_files_pdq's comparison count at similarity s (scanner.rs:1778).
 */
#define RPH_TREE_NEVER 255u
/* The core, on any edge list a sweep left on the device (plain, variant, cross with bases, 64-bit): edge e joins e.i + i_base and
 * e.j + j_base at level e.d.  d_into n x uint32, d_level n bytes, d_edges_at (top + 1) x uint64, d_labels (nullable) n x uint32: the
 * flattened min-labels at `top`, as rph_union_find_labels_dev leaves them.  An edge that names a file >= n or has d > top:
 * RPH_ERR_INVALID_ARG with nothing written; the call waits for that check (it synchronises `stream` once) and everything else is
 * asynchronous on `stream`.  n at most 2^31 - 1; top at most 254, here and in the host form: a level of 255 could not be told from
 * RPH_TREE_NEVER, so 255 and above are RPH_ERR_INVALID_ARG.  n == 0 without edges: RPH_OK.  Workspace: the context's kept scratch, 8 bytes
 * per edge and 4 to 8 per file. */
int rph_merge_tree_dev(rph_ctx *ctx, const void *d_edges, uint64_t n_edges, uint32_t i_base, uint32_t j_base, uint64_t n,
                       uint32_t top, void *d_into, void *d_level, void *d_edges_at, void *d_labels, void *stream);
/* The same on the host, no context: for edge lists gathered from several GPUs and for callers' own tests. */
int rph_merge_tree_from_edges_host(const rph_edge *edges, uint64_t n_edges, uint64_t n, uint32_t top, uint32_t *into,
                                   uint8_t *level, uint64_t *edges_at);
/* Host arrays in, host arrays out: upload and variants as rph_group_files_pdq does them, ONE triangular variant sweep at `top` whose
 * edges stay on the device, then the core.  top > RPH_MAX_SIMILARITY_256: RPH_ERR_INVALID_ARG (scanner.rs:1650-1655). */
int rph_group_files_pdq_tree(rph_ctx *ctx, const uint8_t *hashes32, const float *coeffs, const uint8_t *has_features,
                             const int32_t *quality, uint64_t n, uint32_t top, uint32_t *into, uint8_t *level,
                             uint64_t *edges_at);
/* The rule without a device: brute force over the host's threads, the rows through rph_pdq_dihedral_one as rph_group_max_dist_host
 * derives them. */
int rph_merge_tree_host(const uint8_t *hashes32, const float *coeffs, const uint8_t *has_features, const int32_t *quality,
                        uint64_t n, uint32_t top, uint32_t *into, uint8_t *level, uint64_t *edges_at);
/* Of the files a library holds, at `top` whatever the library's own similarity is.  The library is not changed: its labels, size and
 * comparison count stay as they are.  One triangular sweep of everything resident -- except on a library made by
 * rph_library_create_tree with `top` at or below its store's: there no sweep runs, the core runs over the store and the result is cut
 * down to `top`.  The bytes are the same either way: those of rph_group_files_pdq_tree(top) on the resident files in order. */
int rph_library_merge_tree(rph_library *lib, uint32_t top, uint32_t *into, uint8_t *level, uint64_t *edges_at);
/* The tree for t <= top from the tree for top, on the host, no context: level_out[x] = level[x] and into_out[x] = into[x] where
 * level[x] <= t, RPH_TREE_NEVER and x elsewhere; edges_at_out = the first t + 1 entries of edges_at.  Exact, because level[x] does not
 * depend on top.  The outputs may be the inputs.  t > top or a malformed tree (as below): RPH_ERR_INVALID_ARG with nothing written. */
int rph_merge_tree_truncate(const uint32_t *into, const uint8_t *level, const uint64_t *edges_at, uint64_t n, uint32_t top,
                            uint32_t t, uint32_t *into_out, uint8_t *level_out, uint64_t *edges_at_out);
/* Cutting a tree, on the host: O(n).  A malformed tree -- into[x] > x, into[x] == x with a level other than RPH_TREE_NEVER (or the
 * reverse), a level that does not rise along a chain -- is RPH_ERR_INVALID_ARG with nothing written.
 * labels_out[x] = label_s[x]. */
int rph_merge_tree_labels(const uint32_t *into, const uint8_t *level, uint64_t n, uint32_t s, uint32_t *labels_out);
/* The groups at s in the order and with the capacities of rph_union_find_groups: components with > 1 member, members ascending, groups
 * by first member; members capacity n, offsets capacity n / 2 + 2. */
int rph_merge_tree_groups(const uint32_t *into, const uint8_t *level, uint64_t n, uint32_t s, uint32_t *members,
                          uint32_t *offsets, uint32_t *n_groups_out);
/* For every s in 0 .. top (top + 1 entries each, top at most 254): the number of components with more than one member, and the number of
 * files in them. */
int rph_merge_tree_profile(const uint32_t *into, const uint8_t *level, uint64_t n, uint32_t top, uint64_t *n_groups_out,
                           uint64_t *grouped_files_out);

/* is_low_pdq_quality (scanner.rs:1592-1594); quality < 0 encodes None. */
int rph_is_low_pdq_quality(int32_t quality);

/* MIHIndex::new (hamminghash.rs:89-130) for [u8;32]: CSR arrays built on the
 * device.  offsets: 16*65536+1 u32, values: 16*n u32 (ascending id per bucket). */
int rph_mih_build256(rph_ctx *ctx, const uint8_t *hashes32, uint64_t n, uint32_t *offsets, uint32_t *values);
/* MIHIndex::<u64>::new (hamminghash.rs:23-41, :89-130): 8 chunks of 8 bits.  offsets: 8*256+1 u32, values: 8*n u32. */
int rph_mih_build64(rph_ctx *ctx, const uint64_t *hashes64, uint64_t n, uint32_t *offsets, uint32_t *values);

/* =====================================================================
 * Several GPUs under ONE host process  
 *
 * phdupes is a single process (scanner.rs:1146: one call hashes every file, then groups them), so the multi-GPU form of the
 * path is offered inside the library: an rph_multi owns one rph_ctx per device and an RCCL communicator over them
 * (ncclCommInitAll; RCCL is loaded at run time).  Its entry points shard exactly as rupphash_amd/dist.py does across processes:
 * files are dealt to the devices in contiguous ranges (no communication), ONE ncclAllGather completes the per-file hash
 * blocks on every device (the only exchange step of the path), every device sweeps the blocks p == i (mod n_devices) of the
 * sweep's enumeration, the few edges go to the host for the serial union-find.  Results equal the single-context entry
 * points for every n_devices.  One multi-device call at a time per rph_multi.
 * ===================================================================== */
typedef struct rph_multi rph_multi;
/* devices: n_devices HIP ordinals, or NULL for 0 .. n_devices-1.  RPH_ERR_UNSUPPORTED when RCCL cannot be loaded. */
int rph_multi_init(const int *devices, int n_devices, rph_multi **multi_out);
int rph_multi_shutdown(rph_multi *multi);
int rph_multi_size(rph_multi *multi);
rph_ctx *rph_multi_ctx(rph_multi *multi, int index);  /* the context of device `index`: any single-device entry point works on it */
/* rph_hamming_all_pairs across the devices (BASELINE config 5): hashes from the host, edges (unordered) back. */
int rph_multi_hamming_all_pairs(rph_multi *multi, const uint8_t *hashes32, uint64_t n, uint32_t threshold, rph_edge *edges,
                                uint64_t cap, uint64_t *n_edges_out);
/*
 * The reference's scan-then-group call (scanner.rs:1146-1551 + group_files_generic with PdqStrategy, :1640-1823) across the
 * devices (BASELINE config 4): n images of one geometry in host memory -> PDQ hash, quality, coefficients (as
 * rph_pdq_hash_batch; coeffs_out / quality_out / valid_out nullable) -> all-gather of the 8 dihedral hashes and the
 * low-confidence flag of every file (quality = round(q * 100) < 50, scanner.rs:1416-1417, :1588-1594) -> variant sweep ->
 * connected components as rph_group_files_pdq reports them.
 */
int rph_multi_hash_and_group(rph_multi *multi, const uint8_t *px, uint32_t n, uint32_t w, uint32_t h, uint32_t channels,
                             size_t row_stride, size_t image_stride, uint32_t similarity, uint8_t *hash32_out, float *quality_out,
                             float *coeffs_out, uint8_t *valid_out, uint32_t *members, uint32_t *offsets, uint32_t *n_groups_out,
                             uint64_t *comparison_count_out);
/* The same from JPEG FILES in host memory (rows N3 + B6 in one call): device i decodes and hashes files [lo_i, hi_i) as
 * rph_jpeg_pdq_hash_batch does (n_threads host threads in all, 0 = what the process may use per device), then the files that
 * produced a hash are grouped as above; members are indices into the caller's file list.  quality_out / coeffs_out / valid_out /
 * status_out are nullable. */
int rph_multi_jpeg_hash_and_group(rph_multi *multi, const uint8_t *const *data, const size_t *len, uint32_t n, int flavour, uint32_t n_threads,
                                  uint32_t similarity, uint8_t *hash32_out, float *quality_out, float *coeffs_out, uint8_t *valid_out,
                                  int32_t *status_out, uint32_t *members, uint32_t *offsets, uint32_t *n_groups_out,
                                  uint64_t *comparison_count_out);
/* The same from files of any mix of the six formats: device i runs rph_files_pdq_hash_batch (the files section below) on files
 * [lo_i, hi_i) with their names, n_threads host threads in all; names, pixel_hash32_out and format_out as there (nullable).  The
 * sharding, the exchange and the grouping are those of rph_multi_jpeg_hash_and_group. */
int rph_multi_files_hash_and_group(rph_multi *multi, const uint8_t *const *data, const size_t *len, const char *const *names, uint32_t n,
                                   int jpeg_flavour, uint32_t n_threads, uint32_t similarity, uint8_t *hash32_out, float *quality_out,
                                   float *coeffs_out, uint8_t *valid_out, int32_t *status_out, uint8_t *pixel_hash32_out, uint8_t *format_out,
                                   uint32_t *members, uint32_t *offsets, uint32_t *n_groups_out, uint64_t *comparison_count_out);
/* rph_group_files_pdq across the devices: hashes / coefficients / quality from the cache (same arguments and results). */
int rph_multi_group_files_pdq(rph_multi *multi, const uint8_t *hashes32, const float *coeffs, const uint8_t *has_features,
                              const int32_t *quality, uint64_t n, uint32_t similarity, uint32_t *members, uint32_t *offsets,
                              uint32_t *n_groups_out, uint64_t *comparison_count_out);

/* =====================================================================
 * Cache record codecs (reference: src/db.rs), host scalar.  The layouts of the VALUES phdupes keeps per content hash,
 * for bulk import/export between an existing cache and the engine's flat arrays.  The XChaCha20-Poly1305 envelope
 * around them (db.rs:634-673) is the host application's business and is not touched here.
 * ===================================================================== */
#define RPH_PDQ_ALGO_VERSION 2u        /* db.rs:47 */
#define RPH_HASH_RECORD_BYTES 33u      /* hash_db value: [PDQ_ALGO_VERSION || 32-byte hash], db.rs:1200-1211 */
#define RPH_COEFF_RECORD_BYTES 1027u   /* coeff_db value of a 256-coefficient vector: [2 || 0x80 0x02 || 256 x f32 LE] */
void rph_hash_record_encode(const uint8_t *hash32, uint8_t *out33);
/* get_pdqhash's match (db.rs:683-696): 1 = Some(hash); 0 = None (another algorithm version or a length != 33: a miss, not an error) */
int rph_hash_record_decode(const uint8_t *rec, size_t len, uint8_t *hash32_out);
/* n records of 33 bytes each; decode returns the number of hits, present_out[i] (nullable) = 1/0, missing hashes zeroed */
void rph_hash_records_encode(const uint8_t *hashes32, size_t n, uint8_t *out33n);
size_t rph_hash_records_decode(const uint8_t *recs33n, size_t n, uint8_t *hashes32_out, uint8_t *present_out);
/* coeff_db value: [PDQ_ALGO_VERSION || postcard(CachedCoefficients { coefficients: Vec<f32> })] = [2 || varint(len) || len x f32 LE]
 * (db.rs:217-230, :1221-1231).  encode returns the record size (always; nothing is written if cap is smaller). */
size_t rph_coeff_record_size(size_t n_coeffs);
size_t rph_coeff_record_encode(const float *coeffs, size_t n_coeffs, uint8_t *out, size_t cap);
/* get_coefficients' match (db.rs:742-755): 1 = Some (n_out coefficients written; the caller keeps them only if n_out == 256,
 * scanner.rs:1265-1267); 0 = None (empty or another algorithm version); RPH_ERR_INVALID_ARG = the reference's
 * lmdb::Error::Corrupted (malformed postcard payload); RPH_ERR_CAPACITY = more than `cap` coefficients (n_out still set). */
int rph_coeff_record_decode(const uint8_t *rec, size_t len, float *coeffs_out, size_t cap, size_t *n_out);

/* =====================================================================
 * JPEG decode feeding the hasher.  Replaces the "jpg" | "jpeg" arm of load_image_fast
 * (reference: src/scanner.rs:461-508: zune-jpeg 0.5.15 -> Luma8 for one component, Rgb8 for three) followed by
 * generate_pdq_features (scanner.rs:1410).  The entropy coding is undone on the device too when a call brings enough
 * files (rph_jpeg_set_entropy; the host then only strips the byte stuffing), else by the host threads, one image each like
 * the reference's rayon workers (scanner.rs:1202); dequantisation, IDCT, chroma upsampling, colour conversion, luma and
 * the hash run on the device, a batch of files per launch, and only the hashes come back.
 * Supported: baseline / extended sequential / progressive Huffman JPEG, 8 bit, 1 or 3 components, luma sampling
 * 1x1, 2x1, 1x2, 2x2 with 1x1 chroma, restart intervals.  Anything else (CMYK, arithmetic coding, 12 bit, lossless)
 * returns RPH_ERR_UNSUPPORTED and a corrupt stream RPH_ERR_INVALID_ARG -- the caller falls through to its next
 * decoder exactly as the reference falls from tier 1 to tier 2 (scanner.rs:510-551).
 * `flavour`: the sample arithmetic behind the (decoder independent) coefficients.
 *   RPH_JPEG_ZUNE     what zune-jpeg does, as far as it can be restated without its source (absent from the reference
 *                     tree): PARITY UNPINNED against the Rust binary.
 *   RPH_JPEG_LIBJPEG  libjpeg-turbo's default arithmetic (islow IDCT, fancy upsampling): byte-identical to
 *                     libjpeg-turbo / Pillow, which is what the tests pin it with.
 * ===================================================================== */
#define RPH_JPEG_ZUNE 0
#define RPH_JPEG_LIBJPEG 1
/* Frame header only, host code: width, height and 1 or 3 channels (what zune's info() gives load_image_fast, scanner.rs:477-481). */
int rph_jpeg_info(const uint8_t *data, size_t len, uint32_t *w, uint32_t *h, uint32_t *channels);
/* The host half alone (tests, tools): quantised coefficients in natural order, component-major, raster over each component's
 * MCU-padded block grid.  geometry: 8 words per component {blocks_w, blocks_h, H, V, table, samples_w, samples_h, first_block};
 * qt: 4 x 64 quantisation tables in natural order; coef may be NULL to ask for *total_blocks only. */
int rph_jpeg_coefficients(const uint8_t *data, size_t len, uint32_t *geometry, uint16_t *qt, int16_t *coef, size_t cap_blocks,
                          uint64_t *total_blocks);
/* load_image_fast for one JPEG: pixels_out receives w * h * channels bytes, packed rows (Luma8 or Rgb8). */
int rph_jpeg_decode(rph_ctx *ctx, const uint8_t *data, size_t len, int flavour, uint8_t *pixels_out);
/* n files -> n hashes (optional quality / 256 coefficients / 8 dihedral hashes per file, as rph_pdq_hash_batch).
 * n_threads host threads undo the entropy coding (0 = as many as the process may use: affinity mask and cgroup CPU quota).  valid_out[i] = 0 and status_out[i] != RPH_OK
 * for a file that cannot be decoded (the call itself still returns RPH_OK); valid_out[i] = 0 with status RPH_OK for an
 * image below 5 px (generate_pdq_features' None, pdqhash.rs:167-169).  Files of any mix of sizes share a call. */
int rph_jpeg_pdq_hash_batch(rph_ctx *ctx, const uint8_t *const *data, const size_t *len, uint32_t n, int flavour, uint32_t n_threads,
                            uint8_t *hash32_out, float *quality_out, float *coeffs_out, uint8_t *dihedral_out, uint8_t *valid_out,
                            int32_t *status_out);

/* The same for ONE file per call, from any number of threads at once (the reference's scan loop as it stands: load_image_fast +
 * generate_pdq_features on every rayon worker, scanner.rs:1202, :1410): blocking.  The calling thread undoes the entropy coding of
 * its file itself (into a pinned buffer it keeps for its lifetime); callers that arrive while a batch is on the device leave
 * together as the next batch.  Returns the file's status (RPH_OK with *valid_out = 0: below 5 px); quality_out, coeffs_out
 * (256 floats) and valid_out may be NULL. */
int rph_jpeg_pdq_hash_one(rph_ctx *ctx, const uint8_t *data, size_t len, int flavour, uint8_t *hash32_out, float *quality_out, float *coeffs_out,
                          uint8_t *valid_out);

/* Where rph_jpeg_pdq_hash_batch decodes the Huffman streams:
 *   RPH_JPEG_ENTROPY_HOST (0)    n_threads host threads, one file each; the coefficients cross PCIe (0.8 MB per 512x512 file);
 *   RPH_JPEG_ENTROPY_DEVICE (1)  on the device, one file per lane: the host only copies the entropy bytes (stuffing undone) and the
 *                                compressed bytes cross PCIe; the walk of one file is serial (milliseconds), so this pays from
 *                                thousands of files per call;
 *   RPH_JPEG_ENTROPY_AUTO (2)    default: sequential files on the device from 512 lanes per call (a file is one lane, or one per
 *                                restart interval when it has restart markers, or one per 8 KB of a stream without them that is
 *                                long enough for segments), host below; progressive files on the device when the host threads
 *                                would need longer for all of them than the device for the longest (~0.6 us per byte);
 *   RPH_JPEG_ENTROPY_DEVICE_SEQUENTIAL (3)  as DEVICE, but progressive files stay with the host threads (tests, A/B timing).
 * Same results either way, for damaged files too: a file the device walk flags (or does not take) is decoded again by the host
 * decoder, and only the host decoder's verdict makes a file unreadable -- so a file's status and hash do not depend on the other
 * files of its call.  What a damaged stream gets, in the host decoder (jpeg_host.cpp), the device walks (jpeg_kernels.hip) and the
 * CPU oracle (oracle/jpeg_ref.c) alike:
 *   REFUSED (status RPH_ERR_INVALID_ARG)
 *     1. a Huffman code the table does not assign     (decode_symbol -1; jpeg_huff_kernel / BitR::symbol8 "l > 16"; huff_decode -1)
 *     2. a DC category above 15                        (block_seq / block_dc_first "s > 15"; the kernels "s > 15"; decode_block_* "s > 15")
 *     3. an AC value whose run passes coefficient 63, or Se in a progressive first AC scan
 *                                                      (block_seq "kk > 64", block_ac_first "kk > sc.se"; jpeg_huff_kernel "k > 64",
 *                                                       jpeg_prog_kernel "k > se"; decode_block_seq "kk > 63", decode_block_ac_first "kk > se")
 *     4. a ZRL that steps past the end of the block (past Se in a first AC scan); one that ends exactly there is sixteen zeros
 *                                                      (the same lines: "kk > 64", "kk > sc.se + 1"; "k > 64", "k > se + 1")
 *     5. a restart boundary whose next marker is not an RSTn (any n: a renumbered RSTn is accepted; bytes before the marker are
 *        skipped)                                      (Decoder::restart; decode_scan "RSTn"; the device takes restart intervals only
 *                                                       when the RSTn markers are exactly the boundaries, prepare_stream, and flags a
 *                                                       lane that reads past its interval, jpeg_huff_kernel "stream_end")
 *     6. an AC refinement symbol with a magnitude other than 1
 *                                                      (block_ac_refine "s != 1"; jpeg_prog_kernel "s != 1"; decode_block_ac_refine)
 *     7. the header checks (frame, tables, scan parameters, a second frame header behind a scan).
 *   DECODED ANYWAY, zeros fed for the missing bits
 *     8. data that ends early, or a marker inside a scan (an 0xFF followed by anything but 0x00, fill bytes included: Bits::refill,
 *        destuff, br_byte) -- unless a restart boundary follows (rule 5);
 *     9. an end-of-band run longer than the blocks left in the scan; a refinement run that ends beyond Se (the block ends there).
 * Parity with zune-jpeg on damaged streams is not pinned (nothing in the reference tree says what it does). */
#define RPH_JPEG_ENTROPY_HOST 0
#define RPH_JPEG_ENTROPY_DEVICE 1
#define RPH_JPEG_ENTROPY_AUTO 2
#define RPH_JPEG_ENTROPY_DEVICE_SEQUENTIAL 3
int rph_jpeg_set_entropy(rph_ctx *ctx, int where);
/* Tuning of the device walk for streams WITHOUT restart markers: from min_stream_bytes of entropy-coded data (default 8192) a
 * stream is cut into segments of segment_bytes (default 1024; a multiple of 4 in 64 .. 65536; 0 = never) that find their
 * entry points on the device (Huffman streams re-synchronise; the chain of entries is verified, a file that does not verify is
 * walked by one lane) and are then walked side by side -- unless, for a chunk of the call, one lane per file is estimated to be
 * quicker (many shorter files).  min_stream_bytes = 0 forces segments for every such file (tests).  Same results whatever the setting. */
int rph_jpeg_set_segments(rph_ctx *ctx, uint32_t min_stream_bytes, uint32_t segment_bytes);
/* The JPEG path keeps its staging and device buffers in the context between calls (for a large call up to half of the free device
 * memory for the coefficients of the files in flight); this returns them.  The next call allocates again. */
int rph_jpeg_release(rph_ctx *ctx);

/* rph_jpeg_pdq_hash_batch + the pixel hash (rph_pixel_hash_batch, below) of every decoded file: pixel_hash32_out receives n x 32
 * bytes.  The reference hashes the pixels before generate_pdq_features (scanner.rs:1393-1410), so an image below 5 px has its pixel
 * hash (valid_out 0, status RPH_OK); a file that cannot be decoded gets status != RPH_OK and 32 zero bytes.  Colour files are
 * reconstructed as Rgb8 (as rph_jpeg_decode does) instead of the luma-only fused kernel, and PDQ then hashes those pixels: the
 * other outputs are byte-identical to rph_jpeg_pdq_hash_batch's, in every entropy mode. */
int rph_jpeg_pdq_pixel_hash_batch(rph_ctx *ctx, const uint8_t *const *data, const size_t *len, uint32_t n, int flavour, uint32_t n_threads,
                                  uint8_t *hash32_out, float *quality_out, float *coeffs_out, uint8_t *dihedral_out, uint8_t *valid_out,
                                  int32_t *status_out, uint8_t *pixel_hash32_out);

/* =====================================================================
 * PNG decode feeding the hasher: the "png" arm of load_image_fast (image 0.25 + png 0.18 with Transformations::EXPAND, 16-bit samples
 * kept) followed by the pixel hash and generate_pdq_features (scanner.rs:1393-1410).  The host parses the chunks and uploads the
 * compressed bytes; the device inflates (one wave per stream), unfilters, expands to the hasher's pixels and hashes them where they lie;
 * only hashes come back.  Colour management chunks (gAMA, iCCP, sRGB, cHRM) are ignored, only the default image (IDAT) is decoded
 * (APNG frames are not), Adam7 is supported.
 * Native pixels (rph_png_decode, rph_png_decode_host): the DynamicImage the crates hand over, channels x bit_depth per sample:
 *   gray 1/2/4/8 -> Luma8 (a sub-8-bit sample v scaled by 255 / (2^d - 1));  gray + tRNS -> LumaA8 (alpha 0 where the unscaled sample
 *   equals the key, else 255);  RGB 8 -> Rgb8, with tRNS Rgba8 (alpha 0 where R, G and B all equal the key);  palette -> Rgb8, with tRNS
 *   Rgba8 (entries past a short tRNS opaque, an index past the palette opaque black);  gray+alpha 8 -> LumaA8;  RGBA 8 -> Rgba8;  any of
 *   these at 16 bit -> L16 / La16 / Rgb16 / Rgba16, samples as native uint16_t.
 * What is hashed:
 *   PDQ        to_luma601 (pdqhash.rs:268-284): Luma8 as it is, Rgb8 / Rgba8 through the 601 luma of R, G, B; LumaA8 as Rgba8 (l, l, l, a);
 *              16-bit images through to_rgb8, each sample v -> round(v / 257) = (v + 128) / 257 (no ties).  That last formula is
 *              UNPINNED against the crate (its source is not in the reference tree).
 *   pixel hash blake3 of to_rgba16() (scanner.rs:1393-1404): 8-bit samples v -> v * 257, 16-bit samples as they are, gray replicated into
 *              R, G, B, a missing alpha 65535.  An 8-bit PNG of a decoded JPEG therefore has the JPEG's pixel hash.
 * ONE RULE for damaged or hostile files, the same in the host parser (png_host.cpp), the shared inflate (inflate.h: host threads and
 * device kernel alike) and the unfilter (host and device): a file's status does not depend on the other files of its call or on where
 * it was inflated.  Parity with the png crate on damaged input is UNPINNED.
 *   REFUSED (RPH_ERR_INVALID_ARG)
 *     - a bad signature; an IHDR that is not the first chunk, comes twice or has invalid fields (size 0, depth / colour type pair,
 *       compression, filter or interlace method);
 *     - a chunk CRC mismatch before IEND; an unknown critical chunk; a second PLTE or one whose size is not 3 .. 768 in steps of 3;
 *       a missing PLTE for colour type 3;
 *     - zlib: CM != 8, CINFO > 7, FCHECK, FDICT; block type 3; stored LEN / NLEN mismatch; over-subscribed or incomplete Huffman codes
 *       (zlib's exception stands: a literal/length or distance code of a single length-1 code); HLIT > 286, HDIST > 30, a repeat with
 *       nothing before it or past the end, no end-of-block code; literal/length symbols 286-287, distance symbols 30-31, a bit pattern
 *       the code does not assign; a distance that reaches before the start of the output; an Adler-32 mismatch; a stream that ends
 *       (or whose input ends) before its final block and Adler-32 -- in particular one that ends before the image's last byte;
 *     - a filter type above 4.
 *   ACCEPTED
 *     - bytes after the image inside the zlib stream (decoded and checked, not stored); bytes after the Adler-32;
 *     - chunks after IEND (not read; IEND's own CRC is not checked); a missing IEND, or a last chunk cut short by the end of the file
 *       (the parse stops there), once the IDAT bytes before it hold a stream that has ended and verified;
 *     - a tRNS of the wrong size for its colour type, or in colour types 4 / 6: ignored; a palette tRNS longer than the palette: cut;
 *       a PLTE in a gray image or a truecolour image: not used.
 *   RPH_ERR_UNSUPPORTED, before anything is allocated: an IHDR whose raw size (filter bytes included) cannot come from the file's IDAT
 *     bytes (more than 1032 x their length: deflate expands at most 1032:1), or whose raw size exceeds 1 GiB or 2^28 pixels.
 *   VALID BUT SMALL: an image below 5 px gets valid = 0 with status RPH_OK, and still its pixel hash.
 * ===================================================================== */
#define RPH_PNG_INFLATE_HOST 0   /* n_threads host threads inflate (inflate.h); the raw filtered bytes cross PCIe */
#define RPH_PNG_INFLATE_DEVICE 1 /* one wave per stream on the device; the compressed bytes cross PCIe */
#define RPH_PNG_INFLATE_AUTO 2   /* default: the device for chunks that inflate 32:1 or more, else the host */
/* Header only, host code, no context: the native layout rph_png_decode will produce (channels 1-4, bit_depth 8 or 16); returns the
 * file's status by the rule above (the zlib stream itself is not inflated). */
int rph_png_info(const uint8_t *data, size_t len, uint32_t *w, uint32_t *h, uint32_t *channels, uint32_t *bit_depth);
/* The whole decoder on the CPU, no context (tests, tools): native pixels, packed rows, w * h * channels samples of bit_depth bits into
 * pixels_out (cap_bytes; RPH_ERR_CAPACITY if too small). */
int rph_png_decode_host(const uint8_t *data, size_t len, void *pixels_out, size_t cap_bytes);
/* load_image_fast for one PNG, decoded on the device: the same native pixels as rph_png_decode_host. */
int rph_png_decode(rph_ctx *ctx, const uint8_t *data, size_t len, void *pixels_out, size_t cap_bytes);
/* n PNG files -> n PDQ hashes (+ optional quality, 256 coefficients, 8 dihedral hashes, as rph_pdq_hash_batch) and optional pixel hashes
 * (32 bytes each).  Every output after hash32_out may be NULL.  n_threads host threads parse (and inflate in HOST mode; 0 = as many as
 * the process may use).  status_out[i] by the rule above (the call itself returns RPH_OK); a file that cannot be decoded has zero
 * outputs and valid 0.  Files of any mix of sizes and types share a call; it is processed in chunks of bounded device memory. */
int rph_png_pdq_hash_batch(rph_ctx *ctx, const uint8_t *const *data, const size_t *len, uint32_t n, uint32_t n_threads, uint8_t *hash32_out,
                           float *quality_out, float *coeffs_out, uint8_t *dihedral_out, uint8_t *valid_out, int32_t *status_out,
                           uint8_t *pixel_hash32_out);
/* Where rph_png_pdq_hash_batch inflates (RPH_PNG_INFLATE_*); the results are identical in every mode. */
int rph_png_set_inflate(rph_ctx *ctx, int where);
/* The PNG path keeps its staging and device buffers in the context between calls; this returns them. */
int rph_png_release(rph_ctx *ctx);

/* =====================================================================
 * TIFF decode feeding the hasher: the "tiff" arm of load_image_fast (scanner.rs:628-708: image 0.25's TiffDecoder over tiff 0.11 + weezl)
 * followed by the pixel hash and generate_pdq_features.  The host parses the first IFD into a table of segments (strips or tiles), which
 * are compressed independently: the device decompresses one segment per wave, then one expand kernel undoes the predictor, the byte
 * order and the tiling and writes the hasher's pixels, which are hashed where they lie; only hashes come back.
 * What is decoded (first IFD only; Orientation is ignored: the reference reads it apart from hashing, scanner.rs:130):
 *   container    classic TIFF, II and MM; further IFDs and unknown tags ignored.  BigTIFF (version 43): RPH_ERR_UNSUPPORTED.
 *   layout       strips (RowsPerStrip absent or above the height = one strip; a short last strip) and tiles (edge tiles decoded whole,
 *                cropped).  PlanarConfiguration 2 (with more than one sample) and FillOrder 2: RPH_ERR_UNSUPPORTED.
 *   Compression  1 none, 5 LZW (codes most significant bit first, "early change", Clear 256, EOI 257), 8 and 32946 zlib / Deflate,
 *                32773 PackBits.  Every other (JPEG 6 / 7, CCITT 2-4, old-style LSB-first LZW, ...): RPH_ERR_UNSUPPORTED.
 *   Photometric  0 WhiteIsZero (every sample inverted, an alpha sample included: UNPINNED), 1 BlackIsZero, 2 RGB; absent = 1 for one or
 *                two samples, 2 for more.  3 palette, 5 CMYK, 6 YCbCr, others: RPH_ERR_UNSUPPORTED.
 *   samples      gray at 1 / 2 / 4 / 8 / 16 bit; gray + alpha, RGB, RGBA at 8 / 16 bit; SampleFormat 1; the 4th (2nd for gray) sample is
 *                alpha whatever ExtraSamples says.  Unequal BitsPerSample, more samples, other SampleFormat: RPH_ERR_UNSUPPORTED.
 *   Predictor    1; 2 (horizontal differencing per sample, modulo 2^8 or 2^16, 16-bit words byte-swapped before accumulating) with
 *                Compression 5 / 8 / 32946.  3 (floating point), 2 on sub-8-bit samples, 2 with Compression 1 or 32773 (decoders
 *                disagree whether the tag applies there: libtiff implements the predictor only inside its LZW / Deflate codecs):
 *                RPH_ERR_UNSUPPORTED.
 * A file answered with RPH_ERR_UNSUPPORTED goes to the caller's own decoders, as a CMYK JPEG does (JPEG-in-TIFF, the reference's second
 * tier at scanner.rs:658-702, among them).
 * Native pixels (rph_tiff_decode, rph_tiff_decode_host) and what is hashed follow the PNG section word for word: Luma8 / LumaA8 / Rgb8 /
 * Rgba8 / L16 / La16 / Rgb16 / Rgba16, sub-8-bit gray scaled by 255 / (2^d - 1); PDQ through to_luma601 (LumaA8 as (l, l, l, a), 16-bit
 * through round(v / 257)); pixel hash = blake3 of to_rgba16() little-endian.  An 8-bit TIFF of the pixels of a PNG or of a decoded JPEG
 * therefore has that file's PDQ hash and pixel hash.  The reference's Rgb8 fast path (scanner.rs:639-647) and its from_decoder path
 * yield the same pixels: one path here.  Parity with the tiff / image crates is UNPINNED (their sources are not in the reference tree);
 * for a lossless format the pixels are fixed by the TIFF 6.0 text and pinned in the tests against libtiff (Pillow).
 * ONE RULE for damaged or hostile files, the same in the host parser and decompressors (tiff_host.cpp), the shared decoders (tiff_lzw.h,
 * inflate.h: host threads and device kernels alike): a file's status does not depend on the other files of its call or on where it was
 * decompressed.
 *   REFUSED (RPH_ERR_INVALID_ARG)
 *     - a bad byte-order mark or version; an IFD offset, entry count, or the value array of a tag that is read, reaching outside the
 *       file; a strip or tile whose offset + byte count reaches outside the file;
 *     - a required tag missing (ImageWidth, ImageLength, Strip / TileOffsets, TileWidth and TileLength for tiles; the byte counts
 *       unless Compression is 1, where they are computed); a tag that is read with a type other than SHORT / LONG or a wrong count
 *       (BitsPerSample count != SamplesPerPixel, a scalar with count != 1); zero width, height, RowsPerStrip, tile size or
 *       SamplesPerPixel; a strip or tile count that does not match the geometry;
 *     - LZW: the first code of a segment or after a Clear is 256 or above (a Clear as the very first code is the usual start); a code
 *       above the next free entry; a stream that runs out of bits, or sends EOI, before the segment's bytes are produced; a table that
 *       would grow past 4096 entries (a conforming writer sends Clear at 4094; libtiff refuses such a stream too, weezl is believed
 *       to go on: UNPINNED);
 *     - PackBits: a run or literal cut off by the end of the input before the segment's bytes are produced;
 *     - Deflate: everything the PNG section lists for zlib, and a stream that ends before the segment's last byte.
 *   ACCEPTED
 *     - LZW and PackBits stop when the segment is full: trailing bits, a missing EOI, further runs are not examined;
 *     - Deflate output past the segment's bytes is decoded and checked, not stored (the PNG rule); bytes after the Adler-32;
 *     - a tag that comes twice (the last one counts); tags out of order.
 *   RPH_ERR_UNSUPPORTED, before any pixel memory is allocated: the layouts named above; more than 2^28 pixels or 1 GiB of decoded bytes
 *     (the PNG bounds); a strip or tile whose decoded bytes exceed the most its compressed bytes can expand to: 1032:1 Deflate, 128:2
 *     PackBits, 1:1 uncompressed (a short uncompressed strip therefore lands here), 3839 bytes per 9 bits LZW (tiff_lzw.h).
 *   Where both apply, the order is: header, IFD and tag checks; width / height present and non-zero, SamplesPerPixel, BitsPerSample
 *   count; the UNSUPPORTED layouts; tile / strip tags; the size limits; segment counts; offsets inside the file; the expansion bounds.
 *   VALID BUT SMALL: an image below 5 px gets valid = 0 with status RPH_OK, and still its pixel hash.
 * ===================================================================== */
#define RPH_TIFF_DECOMPRESS_HOST 0   /* n_threads host threads decompress (tiff_lzw.h, inflate.h); the decoded bytes cross PCIe */
#define RPH_TIFF_DECOMPRESS_DEVICE 1 /* one wave per strip or tile on the device; the compressed bytes cross PCIe */
#define RPH_TIFF_DECOMPRESS_AUTO 2   /* default: the device for chunks that expand 16:1 or more, else the host */
/* Header only, host code, no context: the native layout rph_tiff_decode will produce (channels 1-4, bit_depth 8 or 16); returns the
 * file's status by the rule above (the strips and tiles themselves are not decompressed). */
int rph_tiff_info(const uint8_t *data, size_t len, uint32_t *w, uint32_t *h, uint32_t *channels, uint32_t *bit_depth);
/* The whole decoder on the CPU, no context (tests, tools): native pixels, packed rows, w * h * channels samples of bit_depth bits into
 * pixels_out (cap_bytes; RPH_ERR_CAPACITY if too small). */
int rph_tiff_decode_host(const uint8_t *data, size_t len, void *pixels_out, size_t cap_bytes);
/* load_image_fast for one TIFF, decoded on the device: the same native pixels as rph_tiff_decode_host. */
int rph_tiff_decode(rph_ctx *ctx, const uint8_t *data, size_t len, void *pixels_out, size_t cap_bytes);
/* n TIFF files -> n PDQ hashes (+ optional quality, 256 coefficients, 8 dihedral hashes, as rph_pdq_hash_batch) and optional pixel
 * hashes (32 bytes each); the arguments mean what they mean in rph_png_pdq_hash_batch.  status_out[i] by the rule above (the call itself
 * returns RPH_OK); a file that cannot be decoded has zero outputs and valid 0. */
int rph_tiff_pdq_hash_batch(rph_ctx *ctx, const uint8_t *const *data, const size_t *len, uint32_t n, uint32_t n_threads, uint8_t *hash32_out,
                            float *quality_out, float *coeffs_out, uint8_t *dihedral_out, uint8_t *valid_out, int32_t *status_out,
                            uint8_t *pixel_hash32_out);
/* Where rph_tiff_pdq_hash_batch decompresses (RPH_TIFF_DECOMPRESS_*); the results are identical in every mode. */
int rph_tiff_set_decompress(rph_ctx *ctx, int where);
/* The TIFF path keeps its staging and device buffers in the context between calls; this returns them. */
int rph_tiff_release(rph_ctx *ctx);

/* =====================================================================
 * Lossless WebP decode feeding the hasher: the last arm of load_image_fast, where the image crate guesses the format from the bytes
 * (scanner.rs:713-734; WebP is the first format it names), followed by the pixel hash and generate_pdq_features.  The host parses the
 * RIFF container and reads the small serial front of the VP8L stream (transforms with their sub-images, colour table, entropy image,
 * the prefix codes of every group); the main ARGB stream is decoded by one wave per file on the device (or by the host threads), the
 * inverse transforms and the expansion to pixels run on the device, the pixels are hashed where they lie; only hashes come back.
 * What is decoded:
 *   container    RIFF/WEBP whose image is one VP8L chunk (the simple form), or a VP8X extended container holding a VP8L chunk; ICCP,
 *                EXIF, XMP and unknown chunks are skipped.
 *   VP8L         all four transforms in any order the format allows (predictor modes 0-13, and 14 / 15 predicting as mode 0 as libwebp
 *                does; cross-colour; subtract-green; colour indexing with 1 / 2 / 4 / 8-bit bundling), a colour cache of 1-11 bits, the
 *                entropy image with any number of groups, simple and normal prefix codes, the 120 short distance codes.
 * What is not decoded, RPH_ERR_UNSUPPORTED before any pixel memory is allocated: a lossy `VP8 ` chunk (with or without ALPH; a different
 * codec whose chroma upsampling differs between decoders), animation (the VP8X animation flag, ANIM / ANMF), more than 2^28 pixels (the
 * PNG bound; 14-bit sizes cannot exceed it), and a stream whose used prefix-code groups need more than 64 MiB of lookup tables (checked
 * when the entropy image is known, before the codes are read).  Such a file goes to the caller's own decoders, as a CMYK JPEG does.
 * Native pixels (rph_webp_decode, rph_webp_decode_host): Rgb8 when the image has no alpha, Rgba8 when it has; bit_depth is always 8.
 * "Has alpha" is the VP8L header's alpha_is_used bit in both container forms: libwebp's VP8LGetInfo has the last word over the VP8X
 * alpha flag, and Pillow opens the file as RGBA or RGB by it (pinned in the tests on all four combinations).  An image whose bit is 0
 * loses whatever alpha its pixels carry.
 * What is hashed follows the PNG section word for word: PDQ through to_luma601 (alpha ignored), pixel hash = blake3 of to_rgba16()
 * (v -> v * 257, a missing alpha 65535).  A lossless WebP of the pixels of a PNG, a TIFF or a decoded JPEG therefore has that file's PDQ
 * hash and pixel hash.  Parity with the image-webp crate is UNPINNED (its source is not in the reference tree); for a lossless format
 * the pixels are fixed by the format text and pinned in the tests against libwebp (Pillow) in both directions.
 * ONE RULE for damaged or hostile files, the same in the host parser and front (webp_host.cpp) and the shared entropy decoder (vp8l.h:
 * host threads and device kernel alike): a file's status does not depend on the other files of its call or on the entropy mode.  The
 * choices below were checked against libwebp only: UNPINNED against the crate.
 *   REFUSED (RPH_ERR_INVALID_ARG)
 *     - a bad RIFF or WEBP tag; a RIFF size that reaches past the end of the file (libwebp waits for more data) or is below 4;
 *     - a chunk (header or payload) that reaches past the RIFF size before the image chunk is found; no image chunk; a VP8X chunk of
 *       fewer than 10 bytes; a VP8X canvas size that differs from the VP8L image size;
 *     - a VP8L chunk of fewer than 5 bytes, a signature byte other than 0x2f, a non-zero version;
 *     - a transform that comes twice; a colour-cache size of 0 or above 11 (in the main image or a sub-image);
 *     - a prefix code that is over-subscribed or incomplete, or has no symbol at all.  The exception: a code of a single symbol, of any
 *       length, is complete by definition and read with zero bits (libwebp's rule; zlib's differs).  A simple code's symbol at or past
 *       its alphabet (only the 40 distance symbols can be passed) does not count as a symbol;
 *     - a code-length repeat that runs past the alphabet; a max_symbol above the alphabet.  A repeat of the previous length with
 *       nothing before it is NOT refused: the format defines it (8 is repeated), and libwebp decodes it;
 *     - a bit pattern the code does not assign; a literal/length symbol at or past the alphabet (280 plus the cache size); a
 *       colour-cache symbol when no cache is declared (complete codes over the declared alphabet leave no way to write these three;
 *       the decoder checks them all the same);
 *     - a distance that reaches before the first pixel; a copy that runs past the last pixel (refused, not clamped: libwebp refuses);
 *     - a stream that consumes more bits than the chunk holds, anywhere (zero bits are read past the end and the count is checked
 *       after each element of the front and before each symbol of the pixels: libwebp's end-of-stream flag).  The chunk's own size
 *       bounds the bits.  libwebp bounds them by the bytes that follow in the file: behind a chunk of odd size it reads the pad byte
 *       (and whatever chunk comes next), so it decodes some streams that are refused here, never the other way round.
 *   ACCEPTED
 *     - bytes after the last pixel inside the chunk; chunks after the image; bytes after the RIFF size (not read: a RIFF size below the
 *       file length rules, as in libwebp, so a chunk must lie inside it);
 *     - a colour index past the palette (transparent black, as the format says); a missing pad byte after the image chunk;
 *     - prefix-code groups that no block of the entropy image uses (read and checked like the others, then dropped).
 *   Where both apply, the order is: container and chunk walk (a lossy or animated file is UNSUPPORTED as soon as its chunk is met), VP8L
 *   header, the size limit, then the stream in its own order.  Every refusal inside the stream has one status, so their order does not
 *   show.  rph_webp_info stops after the size limit.
 *   VALID BUT SMALL: an image below 5 px gets valid = 0 with status RPH_OK, and still its pixel hash.
 * ===================================================================== */
#define RPH_WEBP_ENTROPY_HOST 0   /* n_threads host threads decode the main ARGB stream (vp8l.h); the ARGB residuals cross PCIe */
#define RPH_WEBP_ENTROPY_DEVICE 1 /* one wave per stream on the device; the compressed bytes and the built tables cross PCIe */
#define RPH_WEBP_ENTROPY_AUTO 2   /* default: the host: the device won on no measured corpus, 2:1 to 2700:1 */
/* Container and VP8L header only, host code, no context: the native layout rph_webp_decode will produce (channels 3 or 4, bit_depth 8);
 * returns the file's status by the rule above as far as the header tells (the stream itself is not read). */
int rph_webp_info(const uint8_t *data, size_t len, uint32_t *w, uint32_t *h, uint32_t *channels, uint32_t *bit_depth);
/* The whole decoder on the CPU, no context (tests, tools): native pixels, packed rows, w * h * channels bytes into pixels_out (cap_bytes;
 * RPH_ERR_CAPACITY if too small). */
int rph_webp_decode_host(const uint8_t *data, size_t len, void *pixels_out, size_t cap_bytes);
/* load_image_fast for one lossless WebP, decoded on the device: the same native pixels as rph_webp_decode_host. */
int rph_webp_decode(rph_ctx *ctx, const uint8_t *data, size_t len, void *pixels_out, size_t cap_bytes);
/* n WebP files -> n PDQ hashes (+ optional quality, 256 coefficients, 8 dihedral hashes, as rph_pdq_hash_batch) and optional pixel
 * hashes (32 bytes each); the arguments mean what they mean in rph_png_pdq_hash_batch.  status_out[i] by the rule above (the call itself
 * returns RPH_OK); a file that cannot be decoded has zero outputs and valid 0. */
int rph_webp_pdq_hash_batch(rph_ctx *ctx, const uint8_t *const *data, const size_t *len, uint32_t n, uint32_t n_threads, uint8_t *hash32_out,
                            float *quality_out, float *coeffs_out, uint8_t *dihedral_out, uint8_t *valid_out, int32_t *status_out,
                            uint8_t *pixel_hash32_out);
/* Where rph_webp_pdq_hash_batch decodes the main ARGB stream (RPH_WEBP_ENTROPY_*); the results are identical in every mode. */
int rph_webp_set_entropy(rph_ctx *ctx, int where);
/* The WebP path keeps its staging and device buffers in the context between calls; this returns them. */
int rph_webp_release(rph_ctx *ctx);

/* =====================================================================
 * GIF decode feeding the hasher: GIF is in the reference's is_image_ext list (scanner.rs:2278) and goes through the image-crate arm of
 * load_image_fast (scanner.rs:713-734: image 0.25's GifDecoder over the gif crate), followed by the pixel hash and
 * generate_pdq_features.  The host parses the container up to the end of the first frame's data and joins that frame's sub-blocks into
 * one stream; one wave per file decodes its LZW codes into palette indices on the device (or the host threads do), one expand kernel
 * undoes the interlacing, looks up the palette, places the frame on the logical screen and sets alpha, and the pixels are hashed where
 * they lie; only hashes come back.
 * What is decoded:
 *   container    GIF87a and GIF89a: logical screen descriptor, global colour table, every extension before the first image descriptor
 *                skipped by its sub-blocks.  Of the Graphic Control Extensions (label 0xF9, one sub-block of 4 bytes) the last one before
 *                the first image descriptor counts: its transparency flag and index.  Disposal, delay, the background colour index, the
 *                pixel aspect ratio, comments, application blocks (NETSCAPE2.0 loops) and plain text are not used.
 *   first frame  position and size, local colour table (else the global one), interlace flag.  Nothing after the first frame's data is
 *                examined: an animated file yields its first frame, as GifDecoder does.
 *   LZW          codes least significant bit first, minimum code size m of 2 .. 8, Clear 1 << m, EOI Clear + 1, widths m + 1 .. 12
 *                growing when the next free entry reaches 1 << width; a table of 4096 entries is full: nothing is added and the width
 *                stays 12 until a Clear ("deferred clear"); a stream whose first code is not a Clear starts from the initial table.
 * Native pixels (rph_gif_decode, rph_gif_decode_host): always Rgba8 at the size of the logical screen, as image 0.25 reports a GIF:
 *   a pixel inside the frame has the palette's RGB and alpha 255; one whose index is the transparent index has the palette's RGB and
 *   alpha 0; an index past the palette's last entry gives (0, 0, 0, 0); a screen pixel outside the frame is (0, 0, 0, 0); the part of a
 *   frame that reaches past the screen is cut off.
 *   These rules follow the gif and image crates as recollected: their sources are not in the reference tree, so parity with them is
 *   UNPINNED (the RGB kept under alpha 0, the transparent black of an out-of-range index and of the screen around a small frame, the
 *   screen rather than the frame as the image's size).  Where the rules and Pillow (frame 0, convert("RGBA")) must agree -- LZW,
 *   interlacing, palettes, the transparent index, on files whose frame fills the screen and whose indices lie in the palette -- the
 *   arithmetic is pinned against Pillow in the tests.
 * What is hashed follows the PNG section word for word: PDQ through to_luma601 (alpha ignored), pixel hash = blake3 of to_rgba16()
 * little-endian (v -> v * 257); the pixels are hashed where they lie.  A GIF of the pixels of a palette PNG therefore has that PNG's PDQ
 * hash and pixel hash (a PNG without tRNS is Rgb8, whose to_rgba16() supplies the same alpha 65535).
 * ONE RULE for damaged or hostile files, the same in the host parser (gif_host.cpp) and the shared decoder (gif_lzw.h: host threads and
 * device kernel alike): a file's status does not depend on the other files of its call or on where it was decompressed.  Parity with
 * the gif crate on damaged input is UNPINNED.
 *   REFUSED (RPH_ERR_INVALID_ARG)
 *     - a signature other than GIF87a / GIF89a;
 *     - a screen descriptor, colour table, extension (label or sub-block), image descriptor, code size byte or data sub-block that
 *       reaches outside the file;
 *     - no image descriptor before the trailer or the end of the file; a block introducer other than 0x21 / 0x2C before it;
 *     - a zero screen width or height; a zero frame width or height;
 *     - no colour table at all for the first frame;
 *     - a code above the next free entry;
 *     - the first code of the stream or after a Clear being above Clear (a Clear after a Clear is accepted);
 *     - a stream that runs out of bits, or sends EOI, before the frame's w * h indices are produced.
 *   ACCEPTED
 *     - decoding stops when the frame is full: further codes, a missing EOI, and a missing block terminator (a file that ends on a
 *       sub-block boundary) are not examined;
 *     - a full table without a Clear;
 *     - anything after the first frame's data; a transparent index past the palette (it matches no pixel that has a colour).
 *   RPH_ERR_UNSUPPORTED, before any pixel memory is allocated
 *     - a minimum code size outside 2 .. 8;
 *     - a screen, or a frame, of more than 2^28 pixels (the PNG bound);
 *     - a frame whose w * h exceeds the most its joined stream of n bytes can expand to: (4095 - (1 << m)) indices from every m + 1 bits,
 *       (4095 - (1 << m)) * floor(8 n / (m + 1)) (gif_lzw.h); a frame without data bytes lands here.
 *   The checks run in file order and the first that fails decides: signature; screen descriptor inside the file, non-zero, its size
 *   limit; global table; blocks up to the image descriptor; the descriptor inside the file, non-zero frame; local table; a table at all;
 *   the code size byte present, its range; the sub-block chain; the frame's size limit; the expansion bound.  rph_gif_info stops there;
 *   every refusal inside the stream has one status.
 *   VALID BUT SMALL: a screen below 5 px gets valid = 0 with status RPH_OK, and still its pixel hash.
 * ===================================================================== */
#define RPH_GIF_DECOMPRESS_HOST 0   /* n_threads host threads decode the LZW streams (gif_lzw.h); the palette indices cross PCIe */
#define RPH_GIF_DECOMPRESS_DEVICE 1 /* one wave per file on the device; the joined compressed bytes cross PCIe */
#define RPH_GIF_DECOMPRESS_AUTO 2   /* default: the host: the device won on no measured corpus, 1.2:1 to 164:1 */
/* Container only, host code, no context: the native layout rph_gif_decode will produce (the logical screen's size, channels 4, bit_depth
 * 8); returns the file's status by the rule above (the codes themselves are not read). */
int rph_gif_info(const uint8_t *data, size_t len, uint32_t *w, uint32_t *h, uint32_t *channels, uint32_t *bit_depth);
/* The whole decoder on the CPU, no context (tests, tools): native pixels, packed rows, w * h * 4 bytes into pixels_out (cap_bytes;
 * RPH_ERR_CAPACITY if too small). */
int rph_gif_decode_host(const uint8_t *data, size_t len, void *pixels_out, size_t cap_bytes);
/* The first frame of one GIF on its screen, decoded on the device: the same native pixels as rph_gif_decode_host. */
int rph_gif_decode(rph_ctx *ctx, const uint8_t *data, size_t len, void *pixels_out, size_t cap_bytes);
/* n GIF files -> n PDQ hashes (+ optional quality, 256 coefficients, 8 dihedral hashes, as rph_pdq_hash_batch) and optional pixel
 * hashes (32 bytes each); the arguments mean what they mean in rph_png_pdq_hash_batch.  status_out[i] by the rule above (the call itself
 * returns RPH_OK); a file that cannot be decoded has zero outputs and valid 0. */
int rph_gif_pdq_hash_batch(rph_ctx *ctx, const uint8_t *const *data, const size_t *len, uint32_t n, uint32_t n_threads, uint8_t *hash32_out,
                           float *quality_out, float *coeffs_out, uint8_t *dihedral_out, uint8_t *valid_out, int32_t *status_out,
                           uint8_t *pixel_hash32_out);
/* Where rph_gif_pdq_hash_batch decodes the LZW streams (RPH_GIF_DECOMPRESS_*); the results are identical in every mode. */
int rph_gif_set_decompress(rph_ctx *ctx, int where);
/* The GIF path keeps its staging and device buffers in the context between calls; this returns them. */
int rph_gif_release(rph_ctx *ctx);

/* =====================================================================
 * BMP decode feeding the hasher: "bmp" is in the reference's is_image_ext list (scanner.rs:2271-2289) and goes through the image-crate arm
 * of load_image_fast (scanner.rs:713-734: image 0.25's BmpDecoder), followed by the pixel hash and generate_pdq_features.  Unless a file
 * is RLE-compressed its bytes already are the pixels: the host parses the headers and copies the pixel array into pinned staging as it
 * lies in the file, one descriptor-driven kernel turns the arrays of a whole chunk into native pixels (rows flipped, B G R reordered,
 * bit fields scaled, palettes looked up), and rph_image_hash_ragged_dev hashes them where they lie, whatever mix of sizes the call holds;
 * only hashes come back.  RLE8 / RLE4 streams are decoded by the host threads into 8-bit index planes, and there is no mode to choose.
 * What is decoded:
 *   headers      "BM" + the 14-byte file header; DIB headers of 12 (BITMAPCOREHEADER: 16-bit sizes, 3-byte palette entries), 40, 52,
 *                56, 108 and 124 bytes.  Width > 0; a negative height means top-down rows; planes = 1; a side of at most 65 535.
 *   depths       BI_RGB (0): 1, 2, 4, 8 with a palette, 16 as X1R5G5B5, 24, 32 (the fourth byte ignored); BI_RLE8 (1): 8; BI_RLE4 (2):
 *                4; BI_BITFIELDS (3) and BI_ALPHABITFIELDS (6): 16 or 32.
 *   masks        read under compressions 3 and 6 only.  Behind a 40-byte header: three dwords (3) or four (6); inside a 52-byte header:
 *                R G B; inside a 56-, 108- or 124-byte header: R G B A.  A mask is one contiguous run of bits (16-bit files: within the
 *                low 16).  A channel of len bits has max = 2^len - 1 and a sample v becomes (v * 255 + max / 2) / max, round to nearest
 *                (max is odd: no ties); a channel wider than 8 bits keeps its top 8; a zero colour mask gives 0.
 *   palette      biClrUsed entries, 1 << bits when that is 0, B G R x each; an index past the palette is black (0, 0, 0).
 *   rows         padded to 4 bytes, bottom-up unless the height is negative; depths below 8 most significant bits first.
 *   RLE          encoded runs, absolute runs (padded to 16 bits), end-of-line, end-of-bitmap, delta; always bottom-up.  Pixels the
 *                stream skips are (0, 0, 0), not palette entry 0.
 * Native pixels (rph_bmp_decode, rph_bmp_decode_host): top-down, rows packed, Rgba8 when the file declares a non-zero alpha mask
 *   (compression 3 or 6), else Rgb8: palette files, 24-bit files, BI_RGB at 16 and 32 bits and files whose alpha mask is zero or absent.
 *   These rules follow the image crate as recollected: its source is not in the reference tree, so parity with it is UNPINNED.  Where the
 *   rules and Pillow must agree -- BI_RGB at 1, 4, 8, 24, 32 bits, both row orders, 32-bit BITFIELDS without alpha, RLE streams that
 *   cover every pixel -- the arithmetic is pinned against Pillow in the tests byte for byte; Pillow floors where the rule rounds, so
 *   16-bit files agree within 1 per sample, and Pillow shows palette entry 0 for skipped RLE pixels.
 * What is hashed follows the PNG section word for word: PDQ through to_luma601 (alpha ignored), pixel hash = blake3 of to_rgba16()
 * little-endian (v -> v * 257, a missing alpha 65535).  A 24-bit BMP of the pixels of an Rgb8 PNG has that PNG's PDQ hash and pixel hash.
 * ONE RULE for damaged or hostile files, all of it in the host parser (bmp_host.cpp; the one RLE decoder lives there too and the device
 * never sees a stream): a file's status does not depend on the other files of its call, and a file rph_bmp_info accepts decodes.  Parity
 * with the image crate on damaged input is UNPINNED.
 *   REFUSED (RPH_ERR_INVALID_ARG)
 *     - fewer than 18 bytes, a signature other than "BM", a DIB header that reaches outside the file;
 *     - planes other than 1; a width <= 0; a height of 0;
 *     - a top-down RLE file;
 *     - a palette of more than 1 << bits entries, or one that reaches outside the file; masks that reach outside the file;
 *     - a mask whose bits are not one contiguous run, or (16-bit files) lie above bit 15;
 *     - a pixel-array offset that points into the headers (file header, DIB header, masks, palette) or at or past the end of the file;
 *     - a pixel array shorter than row_stride * |height| (the crate and Pillow fail on it too);
 *     - an RLE encoded or absolute run that passes the end of its row or lies above the top row, a delta that moves past the row's end
 *       (x > width) or above the row over the top (y > height), an end-of-line there; an absolute run cut off by the end of the file;
 *     - an RLE stream that ends without end-of-bitmap, whether or not every pixel has been set.
 *   ACCEPTED
 *     - anything behind end-of-bitmap, and behind the last row of an uncompressed array; a gap between the headers and the array;
 *     - biSizeImage, the resolution, biClrImportant, the colour space and profile fields of the long headers, bfSize: not read;
 *     - biClrUsed of a file deeper than 8 bits: not read (no palette is looked for);
 *     - masks in a long header under BI_RGB: not read; masks that overlap each other.
 *   RPH_ERR_UNSUPPORTED, before any pixel memory is allocated
 *     - a DIB header size other than 12, 40, 52, 56, 108, 124 (OS/2 2.x's 64 among them);
 *     - a side above 65 535 (the crate's bound); more than 2^28 pixels (the PNG bound);
 *     - BI_JPEG, BI_PNG and every other compression; a depth the table above does not list for its compression.
 *   The checks run in this order and the first that fails decides: length and signature; header size known; header inside the file;
 *   planes; width and height non-zero and positive width; the side and pixel limits; compression and depth; top-down RLE; palette count,
 *   palette inside the file (depth <= 8) or masks inside the file, their shape (depth 16, 32); the array's offset; its length; the RLE
 *   stream, start to end-of-bitmap.  rph_bmp_info runs all of them.
 *   VALID BUT SMALL: an image below 5 px gets valid = 0 with status RPH_OK, and still its pixel hash.
 * ===================================================================== */
/* Host code, no context: the native layout rph_bmp_decode will produce (channels 3 or 4, bit_depth 8); returns the file's status by the
 * rule above. */
int rph_bmp_info(const uint8_t *data, size_t len, uint32_t *w, uint32_t *h, uint32_t *channels, uint32_t *bit_depth);
/* The whole decoder on the CPU, no context (tests, tools): native pixels, packed rows, w * h * channels bytes into pixels_out
 * (cap_bytes; RPH_ERR_CAPACITY if too small). */
int rph_bmp_decode_host(const uint8_t *data, size_t len, void *pixels_out, size_t cap_bytes);
/* One BMP decoded on the device: the same native pixels as rph_bmp_decode_host. */
int rph_bmp_decode(rph_ctx *ctx, const uint8_t *data, size_t len, void *pixels_out, size_t cap_bytes);
/* n BMP files -> n PDQ hashes (+ optional quality, 256 coefficients, 8 dihedral hashes, as rph_pdq_hash_batch) and optional pixel
 * hashes (32 bytes each); the arguments mean what they mean in rph_png_pdq_hash_batch.  status_out[i] by the rule above (the call itself
 * returns RPH_OK); a file that cannot be decoded has zero outputs and valid 0.  Each file's outputs are bit for bit those of
 * rph_image_hash_ragged on its native pixels. */
int rph_bmp_pdq_hash_batch(rph_ctx *ctx, const uint8_t *const *data, const size_t *len, uint32_t n, uint32_t n_threads, uint8_t *hash32_out,
                           float *quality_out, float *coeffs_out, uint8_t *dihedral_out, uint8_t *valid_out, int32_t *status_out,
                           uint8_t *pixel_hash32_out);
/* The BMP path keeps its staging and device buffers in the context between calls; this returns them. */
int rph_bmp_release(rph_ctx *ctx);

/* =====================================================================
 * A mixed list of files in one call: the body of the scan loop's per-file closure (scanner.rs:1350-1417: decode, pixel hash, PDQ
 * features, hash, quality, resolution) for a chunk of files of any of the six formats above.  The content hash stays with the host
 * (INTEGRATION.md 7c).
 * THE ROUTING RULE (rph_file_format): which pipeline takes a file, from its name and its first bytes; load_image_fast's routing
 * (scanner.rs:461-735: extension first, then the bytes' magic, with a fall-through for a misnamed file) reduced to what it comes to.
 *   `name`: a path or file name, UTF-8, or NULL.  Its extension is Rust's Path::extension of the last component after the last '/': none
 *   when the component has no '.', or starts with its only '.'; else the part after the last '.' (which may be empty), compared ASCII
 *   case-insensitively.
 *   1. The extension is one of RAW_EXTS (scanner.rs:43-46: nef dng cr2 cr3 arw orf rw2 raf kdc dcr pef x3f srf 3fr), or jxl, or pdf:
 *      RPH_FORMAT_NONE, the bytes are not looked at.  load_image_fast refuses the RAW names itself (the caller hashes the JPEG thumbnail it
 *      extracts, and passes that with a .jpg name); the jxl and pdf arms return their decoder's error without falling through.
 *   2. Otherwise the magic decides:   PNG 89 50 4E 47 0D 0A 1A 0A;  JPEG FF D8 FF;  GIF "GIF87a" or "GIF89a";  WebP "RIFF" at 0 and "WEBP"
 *      at 8;  TIFF 4D 4D 00 2A or 49 49 2A 00;  BMP "BM".  Anything else, or a file too short for its magic: RPH_FORMAT_NONE.
 *      This is image 0.25's guess_format restated from the published crate, which is not in the reference tree: PARITY UNPINNED.
 *   3. The extension plays no further part: a .jpg or .tif whose bytes are another format fails the reference's dedicated arm and reaches
 *      with_guessed_format (so it goes by its magic), and a known extension over an unknown magic fails in the crate's decoder (NONE).
 *   A WebP goes to the WebP pipeline whatever its payload; that pipeline refuses a lossy one (RPH_ERR_UNSUPPORTED), as it does alone.
 * ===================================================================== */
#define RPH_FORMAT_NONE 0
#define RPH_FORMAT_JPEG 1
#define RPH_FORMAT_PNG 2
#define RPH_FORMAT_TIFF 3
#define RPH_FORMAT_WEBP 4
#define RPH_FORMAT_GIF 5
#define RPH_FORMAT_BMP 6
/* Host code, no context: RPH_FORMAT_* by the rule above.  data may be NULL when len is 0. */
int rph_file_format(const uint8_t *data, size_t len, const char *name);
/* n files of any mix of formats -> the outputs of the per-format calls, in the caller's order.  names (n entries, or NULL; any entry may
 * be NULL) feeds the rule; jpeg_flavour as rph_jpeg_pdq_hash_batch's flavour; every output behind hash32_out may be NULL.
 *  - File i goes to the pipeline rph_file_format names and gets, byte for byte, what that format's own batch call returns for it alone
 *    (JPEG: rph_jpeg_pdq_pixel_hash_batch when pixel_hash32_out is given, else rph_jpeg_pdq_hash_batch), the status of a refused or
 *    damaged file and valid 0 with RPH_OK below 5 px included.  RPH_FORMAT_NONE: status RPH_ERR_UNSUPPORTED, valid 0, zero outputs (the
 *    caller's own decoders take the file); a null or empty file: RPH_ERR_INVALID_ARG.  The call itself returns RPH_OK.
 *  - format_out[i]: the pipeline that took the file (RPH_FORMAT_*), set even when it refused the file; 0 for NONE, null and empty files.
 *    size_out[2 i], [2 i + 1]: width and height of the decoded image (the format's _info: the `resolution` of scanner.rs:1386-1390),
 *    0, 0 when status != RPH_OK.
 *  - The formats present run one after another on the calling thread, each with all n_threads host threads (0 = as many as the
 *    process may use): the default, and RPH_FILES_SEQUENTIAL says so explicitly.  RPH_FILES_CONCURRENT: every format present runs on a
 *    host thread of its own (a lane), so that one format's host decompression overlaps another's device work; the lanes are ordered by
 *    the pipelines' own locks where they share scratch, and the call holds none of them.  The n_threads are then dealt to the lanes in
 *    proportion to their compressed bytes weighted by the format's host cost, each lane at least one.  With 16 threads the lanes did
 *    not beat the sequential route on the measured folder of 512x512 files (they won about 5 % at 1920x1080), which is
 *    why they are not the default.
 *  - A file's results depend neither on the other files of the call nor on n_threads, flags or the pipelines' mode settings.
 *  - When a lane fails as a call (HIP error, allocation) every lane is still joined; the call returns the code of the first failing lane
 *    in RPH_FORMAT_* order, rph_last_error() its message. */
#define RPH_FILES_SEQUENTIAL 1u
#define RPH_FILES_CONCURRENT 2u
int rph_files_pdq_hash_batch(rph_ctx *ctx, const uint8_t *const *data, const size_t *len, const char *const *names, uint32_t n,
                             int jpeg_flavour, uint32_t n_threads, uint32_t flags, uint8_t *hash32_out, float *quality_out, float *coeffs_out,
                             uint8_t *dihedral_out, uint8_t *valid_out, int32_t *status_out, uint8_t *pixel_hash32_out, uint8_t *format_out,
                             uint32_t *size_out);

/* =====================================================================
 * BLAKE3 identity hashes (blake3 crate 1.x, 32-byte output): the two exact hashes the reference computes next to the PDQ hash.
 *   content hash  blake3::keyed_hash(content_key, file_bytes)                     scanner.rs:1343-1347 (the cache key)
 *                 -> rph_blake3_host per file in the scan loop, or rph_blake3_batch(_dev) for a batch of files
 *   pixel hash    blake3::hash of the decoded image's to_rgba16() as little-endian bytes (phdupes --pixel-hash, phdupes.rs:214,
 *                 :850; scanner.rs:1393-1404) -> rph_pixel_hash_batch(_dev) on decoded pixels, or rph_jpeg_pdq_pixel_hash_batch
 *                 for JPEG files (decode + PDQ + pixel hash in one call; the pixels never leave the device)
 * analyze_group then puts bit-identical and pixel-identical files first (scanner.rs:1843-1864; rupphash_amd.scanner.identical_duplicates).
 * Device layout: one lane per 1 KiB chunk, 64 chunks per wave folded across lanes into a 64 KiB subtree, a second kernel folds the
 * subtrees per input.  From host memory rph_blake3_batch is bounded by PCIe and does not beat the host crate: it is the
 * kernels' direct interface; the _dev form hashes bytes already on the device.
 * ===================================================================== */
/* BLAKE3 (hash, or keyed_hash when key32 != NULL: 32 key bytes) of n byte strings of any lengths (0 included) -> n x 32 bytes. */
int rph_blake3_batch(rph_ctx *ctx, const uint8_t *const *data, const size_t *len, uint32_t n, const uint8_t *key32, uint8_t *digest32_out);
/* The same on device memory: string i is d_data[d_offsets[i] .. d_offsets[i+1]) (n + 1 non-decreasing uint64 offsets, device memory).
 * Reads back d_offsets[0] and d_offsets[n] to size its scratch (one synchronisation of `stream`), then runs asynchronously. */
int rph_blake3_batch_dev(rph_ctx *ctx, const void *d_data, const void *d_offsets, uint32_t n, const uint8_t *key32, void *d_digest32,
                         void *stream);
/* One string on the host, no GPU call, no context (the same compression function as the kernels). */
void rph_blake3_host(const uint8_t *data, size_t len, const uint8_t *key32, uint8_t *digest32_out);
/* Pixel hash of scanner.rs:1393-1404: blake3::hash of to_rgba16() of n 8-bit images (channels 1 = Luma8, 3 = Rgb8, 4 = Rgba8;
 * row_stride / image_stride as rph_pdq_hash_batch), little-endian.  Each u8 sample v becomes the u16 v * 257 (255 -> 65535), Luma8
 * is copied into R, G and B, alpha is 65535 unless the input is Rgba8.  PARITY: that widening is the `image` crate's u8 -> u16
 * conversion as published; the crate's source is not in the reference tree, so agreement with the Rust binary rests on it.
 * The RGBA16 stream is built in registers, never in memory. */
int rph_pixel_hash_batch(rph_ctx *ctx, const uint8_t *px, uint32_t n, uint32_t w, uint32_t h, uint32_t channels, size_t row_stride,
                         size_t image_stride, uint8_t *hash32_out);
int rph_pixel_hash_batch_dev(rph_ctx *ctx, const void *d_px, uint32_t n, uint32_t w, uint32_t h, uint32_t channels, size_t row_stride,
                             size_t image_stride, void *d_hash32, void *stream);

/* =====================================================================
 * 64-bit pHash bit operations (reference: src/phash.rs:137-255), host scalar
 * ===================================================================== */
uint64_t rph_phash_rotate_90(uint64_t hash);            /* phash.rs:150 */
uint64_t rph_phash_rotate_180(uint64_t hash);           /* phash.rs:175 */
uint64_t rph_phash_rotate_270(uint64_t hash);           /* phash.rs:191 */
uint64_t rph_phash_flip_horizontal(uint64_t hash);      /* phash.rs:220 */
uint64_t rph_phash_rotation_invariant(uint64_t hash);   /* phash.rs:137 */
void rph_phash_dihedral(uint64_t hash, uint64_t out8[8]); /* phash.rs:242 */

/* =====================================================================
 * Synthetic workloads, generated on the device
 * ===================================================================== */
/* n RGB8 images w x h, global indices first_k.., packed (row stride 3*w). */
int rph_synth_images_dev(rph_ctx *ctx, void *d_out, uint64_t first_k, uint32_t n, uint32_t w, uint32_t h,
                         uint32_t seed, void *stream);
/* hashes [first, first+count) of a synthetic set of n_total (with n_clusters
 * injected 5-member clusters and one distance-32 "2 bits per chunk" pair). */
int rph_synth_hashes_dev(rph_ctx *ctx, void *d_out, uint64_t first, uint64_t count, uint64_t n_total,
                         uint64_t seed, uint64_t n_clusters, void *stream);

/* Measurement aid for bench.py: one pure read pass over a resident device buffer (16-byte aligned), on `stream`.
 * Timed with the event hooks below it gives the read bandwidth this GPU actually delivers to a streaming kernel --
 * the practical ceiling of the PDQ kernel, which reads every image byte exactly once and writes 32 bytes. */
int rph_read_stream_dev(rph_ctx *ctx, const void *d_buf, size_t bytes, void *stream);

/* Device memory helpers for callers without a HIP binding (tests, bench). */
int rph_dev_alloc(rph_ctx *ctx, size_t bytes, void **d_ptr_out);
int rph_dev_free(rph_ctx *ctx, void *d_ptr);
int rph_dev_upload(rph_ctx *ctx, void *d_dst, const void *src, size_t bytes);
int rph_dev_download(rph_ctx *ctx, void *dst, const void *d_src, size_t bytes);
int rph_dev_memset(rph_ctx *ctx, void *d_dst, int value, size_t bytes, void *stream);

/* Extra streams for callers without a HIP binding: the _dev entry points are asynchronous on the stream they are given, and
 * work given to different streams may overlap (the library orders its own shared scratch behind the previous user). */
int rph_stream_create(rph_ctx *ctx, void **stream_out);
int rph_stream_synchronize(rph_ctx *ctx, void *stream);
int rph_stream_destroy(rph_ctx *ctx, void *stream);

/* Timing hooks used by bench.py: HIP events recorded on `stream` (NULL = the
 * context's stream), so the measured interval is the kernels' own stream time. */
int rph_event_create(rph_ctx *ctx, void **event_out);
int rph_event_record(rph_ctx *ctx, void *event, void *stream);
int rph_event_elapsed_ms(rph_ctx *ctx, void *start, void *stop, float *ms_out); /* synchronises on stop */
int rph_event_destroy(rph_ctx *ctx, void *event);
/* The context's own stream (hipStream_t as void*). */
void *rph_stream(rph_ctx *ctx);

#ifdef __cplusplus
}
#endif
#endif /* RUPPHASH_H */
