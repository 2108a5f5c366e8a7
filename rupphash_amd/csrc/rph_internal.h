// rph_internal.h -- shared by the translation units of librupphash_hip.so (not installed).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <condition_variable>
#include <exception>
#include <map>
#include <mutex>
#include <new>
#include <vector>

#include "../../include/rupphash.h"
#include "rph_buffers.h"

// What one chunk of a file pipeline's call (PNG, TIFF, WebP, GIF, BMP) may hold at most; one image larger than a limit forms a chunk of
// its own.  files, comp, raw and pixels are shared by the five formats (GIF and WebP allow pixels / 2: their pixels take 4 bytes);
// webp_*_tables: tables and sub-images of the parsed files of one chunk, and of one parse window; bmp_*: staged source bytes and native
// pixel bytes.  The defaults are what the library runs with; the variables named behind them override them
// (tests only: read once, by rph_init; absent, zero or unparsable: the default)
struct rph_file_limits {
    uint64_t files = 8192;                                 // RPH_FILE_CHUNK_FILES
    uint64_t comp = (uint64_t)256 << 20;                   // RPH_FILE_CHUNK_COMP_BYTES
    uint64_t raw = (uint64_t)768 << 20;                    // RPH_FILE_CHUNK_RAW_BYTES
    uint64_t pixels = (uint64_t)192 << 20;                 // RPH_FILE_CHUNK_PIXELS
    uint64_t webp_chunk_tables = (uint64_t)256 << 20;      // RPH_WEBP_CHUNK_TABLE_BYTES
    uint64_t webp_window_tables = (uint64_t)1 << 30;       // RPH_WEBP_WINDOW_TABLE_BYTES
    uint64_t bmp_src = (uint64_t)256 << 20;                // RPH_BMP_CHUNK_SRC_BYTES
    uint64_t bmp_out = (uint64_t)384 << 20;                // RPH_BMP_CHUNK_OUT_BYTES
};

// the formats of rph_debug_file_chunks
enum { RPH_FILE_PNG = 0, RPH_FILE_TIFF = 1, RPH_FILE_WEBP = 2, RPH_FILE_GIF = 3, RPH_FILE_BMP = 4, RPH_FILE_FORMATS = 5 };

// what the last call of one file pipeline did (rph_debug_file_chunks): files per run_chunk call, in order; WebP's parse windows
struct rph_file_chunk_log {
    std::vector<uint32_t> sizes;
    uint32_t n_windows = 0;
};

// One file pipeline's place in the context (file_pipeline.h): its staging and device buffers and its stream, kept across calls behind
// `pipe`; one batch call at a time (mu); where the format's streams are decoded, 0 = host threads, 1 = device, 2 = automatic (the
// default: RPH_PNG_INFLATE_AUTO, RPH_TIFF_DECOMPRESS_AUTO, RPH_WEBP_ENTROPY_AUTO, RPH_GIF_DECOMPRESS_AUTO); what the last call did with
// the chunk limits, written under mu (rph_debug_file_chunks)
struct rph_file_slot {
    std::mutex mu;
    void *pipe = nullptr;
    int mode = 2;
    rph_file_chunk_log log;
};
static_assert(RPH_PNG_INFLATE_AUTO == 2 && RPH_TIFF_DECOMPRESS_AUTO == 2 && RPH_WEBP_ENTROPY_AUTO == 2 && RPH_GIF_DECOMPRESS_AUTO == 2, "rph_file_slot::mode");

struct rph_ctx {
    int device = 0;
    int compute_units = 0;
    hipStream_t stream = nullptr;
    std::mutex mu;
    uint32_t *sink = nullptr;  // 4-byte result slot of the read-stream probe
    // device scratch shared by every caller stream (rph_buffers.h): the generic (multi-pass) PDQ kernel's two f32 planes per in-flight
    // image; the pre-downsample's u8 planes for > 512 px inputs (full-resolution luma, horizontal pass, thumbnail); the popcount-sorted
    // sweep's sorted hashes, permutation, popcounts and radix-sort workspace, and the component export's counts, sorted labels and
    // hipCUB workspace (components.hip); BLAKE3's plan and group values
    SharedScratch scratch, rz_scratch, sweep_scratch, b3_scratch;
    // sample scratch of the low-latency PDQ kernel, one per caller stream (133 KB per image of a launch chunk): launches on different
    // streams -- the one-image queue's pipeline slots -- share nothing and need no ordering between them
    std::map<hipStream_t, DevBuf> ll_scratch;
    // rph_pdq_hash_batch (host pointers): two pinned staging sets + device twins, alternated over two streams so that the host
    // copy / H2D of one chunk overlaps the transfer and kernels of the other (rph_api.cpp); one host-batch call at a time
    std::mutex pipe_mu;
    void *pipe = nullptr;
    // rph_pdq_hash_ragged (pdq_ragged.hip): pinned descriptor buffers; the pixel bytes of one staging chunk of its host form
    // (RPH_RAGGED_CHUNK_BYTES, tests only: read once, by rph_init)
    void *ragged = nullptr;
    size_t ragged_chunk_bytes = (size_t)64 << 20;
    // rph_image_hash_ragged (pdq_ragged.hip): Luma8 planes of the images of the other layouts that go through rph_pdq_hash_batch_dev;
    // image_mu is held from the kernel that writes them to the last launch that reads them, and guards the scratch in place of mu
    std::mutex image_mu;
    SharedScratch image_planes;
    void *axis_cache = nullptr;  // per-geometry coefficient tables of the pre-downsample, kept across calls (resize_kernels.hip)
    // where the last pre-downsample call left its thumbnails in rz_scratch (rph_debug_copy_thumbnails; n = 0: the call took several chunks)
    struct {
        size_t offset = 0;
        uint32_t n = 0, nw = 0, nh = 0, pitch = 0;
    } rz_last;
    // 2 = fp4 MFMA formulation of the sweep's fast path, popcount-sorted {0,1} operands for plain all-pairs sweeps (default),
    // 3 = fp4 MFMA with +-1 operands everywhere, 4 = sorted {0,1} at every size, 1 = int8 MFMA, 0 = VALU xor + popcount
    // (cross sweeps: 2, 3 and 4 all mean fp4 MFMA with +-1 operands)
    int hamming_kernel = 2;
    // 512x512 RGB8: 0 = always generic; 1 / 2 = fused one-wave-per-image kernel (64- / 128-px strips); 3 = fused low-latency kernel (eight
    // waves per image); 4 = automatic: low-latency below 768 images per call, one-wave-per-image (64-px strips) from there
    int pdq_kernel = 4;
    // JPEG path (jpeg_pipeline.cpp): two chunk slots (pinned staging, device buffers, stream), kept across calls; one batch call at a time
    std::mutex jpeg_mu;
    void *jpeg = nullptr;
    // where the Huffman streams of sequential files are decoded: 0 = host threads, 1 = device (one image per lane), 2 = automatic
    // (device from 2048 sequential files per call: the walk of one image is serial, so it needs tens of thousands of images in flight)
    int jpeg_entropy = 2;
    int jpeg_progressive_on_device = 1;  // 0: progressive files stay with the host threads (rph_jpeg_set_entropy(ctx, 3))
    // device walk of streams without restart markers: from jpeg_seg_min_bytes of entropy data a stream is cut into segments of
    // jpeg_seg_bytes that synchronise on the device and are walked side by side (0 = never)
    uint32_t jpeg_seg_min_bytes = 8192, jpeg_seg_bytes = 1024;
    // rph_debug_jpeg_segment_log: what the segment synchroniser decided in every chunk of the last batch call, as flat records of
    // RPH_SEG_LOG_FILE_WORDS / RPH_SEG_LOG_SEG_WORDS words (under jpeg_mu; off: one branch per chunk)
    bool jpeg_seg_log_on = false;
    std::vector<uint32_t> jpeg_seg_log_files, jpeg_seg_log_segs;
    // rph_jpeg_pdq_hash_one: callers that arrive while a batch is on its way wait here and leave together as the next batch
    std::mutex jpeg_qmu;
    std::condition_variable jpeg_qcv;
    std::vector<void *> jpeg_waiting;
    bool jpeg_leader = false;
    std::vector<void *> jpeg_thread_buffers;  // the callers' pinned coefficient buffers (one per calling thread), freed with the context
    uint64_t serial = 0;                      // distinguishes this context from an earlier one at the same address
    // The five file pipelines, by RPH_FILE_*.  The mode says where the PNG path's zlib streams are inflated (RPH_PNG_INFLATE_*), the TIFF
    // path's strips and tiles decompressed (RPH_TIFF_DECOMPRESS_*), the WebP path's main ARGB streams entropy-decoded
    // (RPH_WEBP_ENTROPY_*) and the GIF path's LZW streams decoded (RPH_GIF_DECOMPRESS_*); the BMP path has no mode: the pixel arrays cross
    // PCIe as they are, RLE streams are the host's.  Their chunk limits (tests only: read once, by rph_init)
    rph_file_slot file[RPH_FILE_FORMATS];
    rph_file_limits file_limits;
    // rph_debug_group_max_dist_events: the caller's events around the distance kernel of group_info.hip (null: none), under mu
    hipEvent_t group_dist_ev[2] = {nullptr, nullptr};
    // rph_debug_merge_tree_events: the caller's events between the stages of merge_tree.hip (null: none), under mu
    hipEvent_t merge_tree_ev[4] = {nullptr, nullptr, nullptr, nullptr};
};

// ---- launchers implemented in the .hip files (all asynchronous on `stream`) ----
// pdq_kernels.hip
int rph_launch_pdq_generic(rph_ctx *ctx, const uint8_t *d_px, uint32_t n, uint32_t w, uint32_t h, uint32_t channels,
                           size_t row_stride, size_t image_stride, uint8_t *d_hash, float *d_quality, float *d_coeffs,
                           uint8_t *d_dihedral, uint8_t *d_valid, hipStream_t stream);
int rph_launch_pdq_fused512(rph_ctx *ctx, const uint8_t *d_px, uint32_t n, size_t row_stride, size_t image_stride,
                            uint8_t *d_hash, float *d_quality, float *d_coeffs, uint8_t *d_dihedral, uint8_t *d_valid,
                            hipStream_t stream, uint32_t channels = 3);  // channels: 3 (Rgb8) or 1 (Luma8)
// pdq_stream.hip: one streaming kernel for Luma8 images of 128..512 x 128..512 with dword-aligned rows; automatic mode takes it from
// RPH_STREAM_MIN_IMAGES images per call (below that a wave per image leaves the chip empty and the image waits ~0.4 ms for its one wave)
constexpr uint32_t RPH_STREAM_MIN_IMAGES = 384;
bool rph_pdq_stream_supported(const uint8_t *d_px, uint32_t w, uint32_t h, uint32_t channels, size_t row_stride, size_t image_stride);
int rph_launch_pdq_stream(rph_ctx *ctx, const uint8_t *d_px, uint32_t n, uint32_t w, uint32_t h, size_t row_stride, size_t image_stride, uint8_t *d_hash,
                          float *d_quality, float *d_coeffs, uint8_t *d_dihedral, uint8_t *d_valid, hipStream_t stream);
bool rph_pdq_stream_color_supported(const uint8_t *d_px, uint32_t w, uint32_t h, uint32_t channels, size_t row_stride, size_t image_stride);
int rph_launch_pdq_stream_color(rph_ctx *ctx, const uint8_t *d_px, uint32_t n, uint32_t w, uint32_t h, uint32_t channels, size_t row_stride, size_t image_stride,
                                uint8_t *d_hash, float *d_quality, float *d_coeffs, uint8_t *d_dihedral, uint8_t *d_valid, hipStream_t stream);
int rph_launch_pdq_resized(rph_ctx *ctx, const uint8_t *d_px, uint32_t n, uint32_t w, uint32_t h, uint32_t channels,
                           size_t row_stride, size_t image_stride, uint8_t *d_hash, float *d_quality, float *d_coeffs,
                           uint8_t *d_dihedral, uint8_t *d_valid, hipStream_t stream);
// resize_kernels.hip: the box windows of one axis of the pre-downsample as resize_mfma_kernel reads them (start, size and the one
// coefficient of every output); false: the taps of some output differ (the matrix-pipe form does not apply)
bool rph_resize_axis_tables(uint32_t in_size, uint32_t out_size, std::vector<uint32_t> &start, std::vector<uint32_t> &size, std::vector<int32_t> &c1, int *precision);
// pdq_ragged.hip: images of any mix of geometries, validated by the caller (rph_api.cpp); d_px + offset[i] = image i
// (channels: 1, 3, 4 for rph_pdq_hash_ragged; any RPH_LAYOUT_* code for rph_image_hash_ragged)
int rph_pdq_ragged_run(rph_ctx *ctx, const uint8_t *d_px, const uint64_t *offset, const uint32_t *w, const uint32_t *h, const uint32_t *channels,
                       const size_t *row_stride, uint32_t n, uint8_t *d_hash, float *d_quality, float *d_coeffs, uint8_t *d_dihedral, uint8_t *d_valid,
                       hipStream_t stream);
// rph_image_hash_ragged_dev without its checks: PDQ outputs when d_hash is given, pixel hashes when d_pixel_hash is
int rph_image_ragged_run(rph_ctx *ctx, const uint8_t *d_px, const uint64_t *offset, const uint32_t *w, const uint32_t *h, const uint32_t *layout,
                         const size_t *row_stride, uint32_t n, uint8_t *d_hash, float *d_quality, float *d_coeffs, uint8_t *d_dihedral, uint8_t *d_valid,
                         uint8_t *d_pixel_hash, hipStream_t stream);
// bytes per pixel of a layout code, 0 for a code that is none
static inline uint32_t rph_layout_bytes(uint32_t layout)
{
    const uint32_t ch = layout & 15u;
    return ((layout & ~16u) == ch && ch >= 1 && ch <= 4) ? ch * (layout > 16 ? 2u : 1u) : 0u;
}
void rph_ragged_forget(rph_ctx *ctx);
int rph_launch_pdq_from_coeffs(const float *d_coeffs, uint32_t n, uint8_t *d_hash, uint8_t *d_dihedral, hipStream_t stream);
int rph_launch_lowconf_from_quality(const float *d_quality, const uint8_t *d_valid, uint64_t n, uint8_t *d_low, hipStream_t stream);
int rph_launch_featureless_variants(const uint8_t *d_hashes, const uint8_t *d_has_features, uint64_t n, uint8_t *d_variants, hipStream_t stream);
// hamming_kernels.hip: one request of a Hamming sweep, in device pointers (rph_api.cpp also fills one with a host form's arrays before it
// uploads them; there a square request may leave `rows` null: its hashes are its rows).  Rows: n files of n_variants (1 or 8) 32-byte
// hashes each, [n][n_variants][32], with the files' flags (either may be null; has_features: files with 0 only own variant 0).  Columns:
// the hashes [n][32] of the SAME files -- the square form, which reports i < j; with one variant `cols` may be `rows` itself -- or, with
// `cross`, another set of n_cols hashes with flags of its own, every pair reported, e.i indexing the rows and e.j the columns.  bits64:
// rows == cols are n little-endian u64 hashes (square, no flags).  Edges are appended at edges[*count], the first `cap` of them written, all
// of them counted.
struct rph_sweep {
    const void *rows = nullptr;
    uint32_t n_variants = 1;
    const uint8_t *low_conf = nullptr, *has_features = nullptr;
    uint64_t n = 0;
    const void *cols = nullptr;
    bool cross = false, bits64 = false;
    const uint8_t *low_conf_cols = nullptr;
    uint64_t n_cols = 0;
    uint32_t threshold = 0, part = 0, nparts = 1;
    rph_edge *edges = nullptr;
    uint64_t cap = 0;
    unsigned long long *count = nullptr;
};
// RPH_ERR_INVALID_ARG for a part that is none, a number of variants other than 1 or 8, or a set of 2^32 files; the launcher's first step
int rph_hamming_sweep_check(const rph_sweep &q);
int rph_launch_hamming_sweep(rph_ctx *ctx, const rph_sweep &q, hipStream_t stream, int use_mfma);
// How an edge buffer that proved too small grows (rph_api.cpp: sweep_growing; multi.cpp: sweep_all): to what the sweep counted plus a
// margin, for a bounded number of attempts.  The find_groups calls and the grouping calls have always differed in both numbers.
struct rph_edge_growth {
    int attempts;
    uint64_t margin_div;
    uint64_t next_cap(uint64_t found) const { return found + found / margin_div + 1024; }
};
constexpr rph_edge_growth RPH_GROW_FIND_GROUPS{8, 8}, RPH_GROW_GROUP_FILES{3, 16};
// which set a cross sweep puts on the row side, its segment length and block count (exported for the tests, not in the header)
extern "C" void rph_debug_hamming_cross_layout(uint64_t n_a, uint32_t n_variants, uint64_t n_b, uint32_t nparts, int kernel, uint32_t *swap_out,
                                               uint32_t *seg_tiles_out, uint32_t *n_col_segs_out, uint64_t *n_blocks_out);
// how the last call of one file pipeline (RPH_FILE_*: a batch call or rph_*_decode) on this context was cut: the number of run_chunk
// calls, the files of each (the first `cap` of them into sizes_out) and, for WebP, the number of parse windows (exported for the tests,
// not in the header; any of the three outputs may be null)
extern "C" int rph_debug_file_chunks(rph_ctx *ctx, int format, uint32_t *sizes_out, uint32_t cap, uint32_t *n_chunks_out, uint32_t *n_windows_out);
// The JPEG segment synchroniser's decisions (jpeg_device.h), recorded chunk by chunk while the switch is on (off by default; every output
// is the same either way) and cleared at the start of every JPEG batch call.  Per segmented file RPH_SEG_LOG_FILE_WORDS words: its index
// in the caller's list, n_segs, total_mcus, scan_bits, verified (0: its first item is a whole-file walk), the index of its first segment
// record, its first lane in the chunk's launch, the chunk's number of Huffman tables.  Per segment RPH_SEG_LOG_SEG_WORDS words: SegState's
// entry, the final `out`, count, dc[3], from, out_check; round 0's n and out; its item's mcu_first, mcu_count, stream_off, bit_skip, dc[3];
// the decodes the validation rounds began in the segment and the bits they read (counted only while the switch is on).
// The reader copies the first file_cap / seg_cap records and reports how many there are (exported for the tests, not in the header; any
// output may be null).
constexpr uint32_t RPH_SEG_LOG_FILE_WORDS = 8, RPH_SEG_LOG_SEG_WORDS = 19;
extern "C" int rph_debug_jpeg_segment_log(rph_ctx *ctx, int on);
extern "C" int rph_debug_jpeg_segments(rph_ctx *ctx, uint32_t *files_out, uint32_t file_cap, uint32_t *n_files_out, uint32_t *segs_out, uint32_t seg_cap,
                                       uint32_t *n_segs_out);
// components.hip: one edge list of a union-find over a label array, e.i + i_base and e.j + j_base being the files an edge unites
struct rph_union_edges {
    const rph_edge *edges = nullptr;
    uint64_t n_edges = 0;
    uint32_t i_base = 0, j_base = 0;
};
// What rph_union_find_labels_dev does, for several lists at once: one range check of all of them and of the entry forest (it waits for
// that: RPH_ERR_INVALID_ARG with nothing written), then one union launch per list and ONE flatten, asynchronous on `stream`
int rph_union_find_labels(rph_ctx *ctx, const rph_union_edges *sets, uint32_t n_sets, uint32_t *d_labels, uint64_t n, hipStream_t stream);
// uf_flatten_kernel alone over a forest with d_labels[x] <= x (merge_tree.hip builds one with kernels of its own)
int rph_launch_uf_flatten(rph_ctx *ctx, uint32_t *d_labels, uint64_t n, hipStream_t stream);
// merge_tree.hip: rph_merge_tree_dev without its argument checks (n >= 1, top <= 255; d_labels nullable).  It takes ctx->mu and the
// sweep scratch (8 bytes per edge, 4 to 8 per file), waits once for the range check and the per-level counts -- RPH_ERR_INVALID_ARG with
// nothing written -- and queues the rest on `stream`
int rph_merge_tree_run(rph_ctx *ctx, const rph_edge *d_edges, uint64_t n_edges, uint32_t i_base, uint32_t j_base, uint64_t n, uint32_t top, uint32_t *d_into,
                       uint8_t *d_level, uint64_t *d_edges_at, uint32_t *d_labels, hipStream_t stream);
// host_merge_tree.cpp: the tree of a host edge list whose edges have been checked (i, j < n, d <= top); edges_at is not touched
void rph_host_merge_tree(const rph_edge *edges, uint64_t n_edges, uint64_t n, uint32_t top, uint32_t *into, uint8_t *level);
// the one definition of rph_merge_tree_truncate's cut, on a tree that has been checked or is the core's own: level <= t stays, the rest
// become roots; in place when the outputs are the inputs (library.cpp cuts the tree of its edge store with it)
void rph_host_merge_tree_cut(const uint32_t *into, const uint8_t *level, uint64_t n, uint32_t t, uint32_t *into_out, uint8_t *level_out);
// The grid of the grid-stride kernels of components.hip, merge_tree.hip and library_kernels.hip: blocks of 256 lanes, at most 8 per compute unit, the
// loops stride over the rest.  rph_stride_lanes_per_pass is what one pass of such a loop covers (rph_debug_library_remove_stats).
inline uint64_t rph_stride_lanes_per_pass(const rph_ctx *ctx) { return (uint64_t)(ctx->compute_units > 1 ? ctx->compute_units : 1) * 8 * 256; }
inline unsigned rph_stride_grid(const rph_ctx *ctx, uint64_t items)
{
    const uint64_t want = (items + 255) / 256, most = rph_stride_lanes_per_pass(ctx) / 256;
    return (unsigned)(want < 1 ? 1 : want < most ? want : most);
}
// library.cpp: the stages of a library's last append in device time (exported for tools/library_rate.py, not in the header)
struct rph_library;
extern "C" int rph_debug_library_stages(rph_library *lib, int on, float *ms_out);
// library.cpp: what the last rph_library_remove did (exported for the tests and tools/library_remove_rate.py, not in the header).
// out[0..3]: members of the components that lost a file (m), edges the regroup sweep found among them, the first edge capacity it tried,
// lanes of one pass of the removal kernels' grid-stride loops (the gather kernel moves a sixteenth as many files per pass).
extern "C" int rph_debug_library_remove_stats(rph_library *lib, uint64_t *out);
// its stages in device time, armed by rph_debug_library_stages(lib, 1, NULL) like the append's (6 floats): mark and select, gather of
// the members, regroup sweep, edge split, compaction and labels, union and flatten
extern "C" int rph_debug_library_remove_stages(rph_library *lib, float *ms_out);
// library.cpp: what the last rph_library_merge_tree did (exported for the tests, not in the header): out[0..1] = edges its sweep found,
// the first edge capacity it tried
extern "C" int rph_debug_library_merge_tree_stats(rph_library *lib, uint64_t *out);
// merge_tree.hip: the caller's events between the stages of the merge-tree calls that follow on this context (exported for
// tools/merge_tree_rate.py, not in the header; nulls disarm)
extern "C" int rph_debug_merge_tree_events(rph_ctx *ctx, void *e0, void *e1, void *e2, void *e3);
// library_kernels.hip: the steps of rph_library_remove, asynchronous on `stream`.  One file's rows in the four per-file arrays:
struct rph_library_rows {
    uint8_t *hashes = nullptr, *variants = nullptr, *low_conf = nullptr, *has_features = nullptr;  // [32], [8][32], [1], [1] per file; 16-byte aligned
};
// removed[x] and touched[label[x]] for the listed files (d_labels: flattened min-labels), then keep[x] = !removed[x] and
// regroup[x] = touched[label[x]]; n bytes each
int rph_library_launch_mark(rph_ctx *ctx, const uint32_t *d_indices, uint64_t n_remove, const uint32_t *d_labels, uint64_t n, uint8_t *d_removed, uint8_t *d_touched,
                            uint8_t *d_keep, uint8_t *d_regroup, hipStream_t stream);
int rph_library_select_temp_bytes(uint64_t n, size_t *bytes_out);
// d_new_index[x] = kept files below x; d_survivors / d_members: the files with keep / regroup set, ascending; d_counts[0], [1]: how many
int rph_library_launch_select(const uint8_t *d_keep, const uint8_t *d_regroup, uint64_t n, uint32_t *d_new_index, uint32_t *d_survivors, uint32_t *d_members,
                              uint32_t *d_counts, void *d_temp, size_t temp_bytes, hipStream_t stream);
// rows d_list[0 .. count) of src become rows 0 .. count-1 of dst
int rph_library_launch_gather(rph_ctx *ctx, const uint32_t *d_list, uint64_t count, const rph_library_rows &src, const rph_library_rows &dst, hipStream_t stream);
// edges local to d_members, in place: one that touches a removed file is counted in *d_dropped and becomes (0, 0), the others get new numbers
int rph_library_launch_split_edges(rph_ctx *ctx, rph_edge *d_edges, uint64_t n_edges, const uint32_t *d_members, const uint8_t *d_removed, const uint32_t *d_new_index,
                                   unsigned long long *d_dropped, hipStream_t stream);
// new_labels[new(x)] for every kept x: itself if its component lost a file, else the new number of its (kept) root
int rph_library_launch_labels(rph_ctx *ctx, const uint32_t *d_labels, const uint8_t *d_removed, const uint8_t *d_touched, const uint32_t *d_new_index, uint64_t n,
                              uint32_t *d_new_labels, hipStream_t stream);
// library_edges.hip: the edge store of a library made by rph_library_create_tree, asynchronous on `stream`.  Both range-check every edge
// before anything is indexed by it and write the lists in no particular order.
// What an append's sweeps left in d_found -- n_cross edges (resident file, new-local file), then (new-local, new-local) ones with i < j,
// over n resident and n_new new files -- rebased to the library's numbering: all n_found of them to d_store_end, the ones with
// d <= similarity also to d_united.  d_nums (2 x u64, zeroed here): how many went to d_united; != 0 if an edge was out of range or had
// d > top (it is written nowhere)
int rph_library_launch_store_append(rph_ctx *ctx, const rph_edge *d_found, uint64_t n_found, uint64_t n_cross, uint32_t n, uint32_t n_new, uint32_t similarity,
                                    uint32_t top, rph_edge *d_store_end, rph_edge *d_united, unsigned long long *d_nums, hipStream_t stream);
// The store of n files without the edges of removed files, renumbered through d_new_index, into d_twin.  d_nums (4 x u64, zeroed here):
// edges kept, edges dropped with d <= similarity, edges dropped, != 0 if an edge named a file >= n
int rph_library_launch_store_filter(rph_ctx *ctx, const rph_edge *d_store, uint64_t n_store, uint64_t n, const uint8_t *d_removed, const uint32_t *d_new_index,
                                    uint32_t similarity, rph_edge *d_twin, unsigned long long *d_nums, hipStream_t stream);
// library.cpp: the edge store's debug hooks (exported for the tests and tools/library_tree_rate.py, not in the header).
// rph_debug_library_edge_store: a store allocated or grown from now on starts at first_capacity_edges and doubles from there (0: the
// default).  rph_debug_library_edge_stats, out[0..4]: growths of the store so far; edges the last append's sweeps found at `top`; how
// many of them were united; edges the last removal dropped from the store; whether the last rph_library_merge_tree swept (0 or 1)
extern "C" int rph_debug_library_edge_store(rph_library *lib, uint64_t first_capacity_edges);
extern "C" int rph_debug_library_edge_stats(rph_library *lib, uint64_t *out);
// group_info.hip: one rph_group_max_dist_dev request in device pointers (include/rupphash.h says what each array is)
struct rph_group_dist {
    const uint8_t *hashes = nullptr, *rows = nullptr, *has_features = nullptr;
    uint64_t n = 0;
    int row_mode = RPH_ROWS_NONE;
    const uint32_t *members = nullptr, *offsets = nullptr, *pivots = nullptr;
    uint32_t n_groups = 0;
    uint32_t *max_dist = nullptr, *member_dist = nullptr;
};
// known_total: offsets[n_groups], from a caller that holds the group arrays on the host and has checked them there
// (rph_host_group_lists_check).  RPH_GROUP_TOTAL_ON_DEVICE: the arrays are only on the device; they are range-checked by a pass of their
// own before anything is read through them, and the call waits for that (RPH_ERR_INVALID_ARG with nothing written).  The rest is
// asynchronous on `stream`.
constexpr uint64_t RPH_GROUP_TOTAL_ON_DEVICE = ~0ull;
int rph_group_max_dist_run(rph_ctx *ctx, const rph_group_dist &q, uint64_t known_total, hipStream_t stream);
// the group arrays of a host caller on the device and room for its outputs, kept by whoever calls often (rph_library)
struct rph_group_lists_dev {
    DevBuf d_groups, d_out;
    uint32_t *members = nullptr, *offsets = nullptr, *pivots = nullptr, *max_dist = nullptr, *member_dist = nullptr;
    uint64_t total = 0;
    uint32_t n_groups = 0;
    int upload(const uint32_t *members, const uint32_t *offsets, uint32_t n_groups, const uint32_t *pivots, bool want_member_dist, hipStream_t stream);
    void fill(rph_group_dist &q) const { q.members = members, q.offsets = offsets, q.pivots = pivots, q.n_groups = n_groups, q.max_dist = max_dist, q.member_dist = member_dist; }
    int download(uint32_t *max_dist_out, uint32_t *member_dist_out, hipStream_t stream);  // waits for the stream
};
// host_grouping.cpp: what every form of rph_group_max_dist refuses, checked before anything is written: a null required argument,
// offsets that do not start at 0 or do not ascend, a member >= n, a pivot >= n that is not RPH_NO_PIVOT
int rph_host_group_lists_check(const char *who, const uint8_t *hashes32, uint64_t n, const uint32_t *members, const uint32_t *offsets, uint32_t n_groups,
                               const uint32_t *pivots, const uint32_t *max_dist_out);
// find_map (scanner.rs:2219-2232): the first listed member of group g that has features, else the first listed member, else RPH_NO_PIVOT
uint32_t rph_host_default_pivot(const uint32_t *members, const uint32_t *offsets, uint32_t g, const float *coeffs, const uint8_t *has_features);
// nearest_kernels.hip: one rph_hamming_nearest_dev request in device pointers (include/rupphash.h says what each array is).  gather
// (nullable, n_q x uint32): query q is the hash hashes_q[gather[q]] and skips that file (rph_library_nearest_files)
struct rph_nearest {
    const uint8_t *rows = nullptr, *has_features = nullptr, *hashes_q = nullptr;
    const uint32_t *skip = nullptr, *gather = nullptr;
    uint32_t n_variants = 1, k = 0, max_dist = 256;
    uint64_t n_lib = 0, n_q = 0;
    rph_edge *out = nullptr;
    uint32_t *counts = nullptr;
};
// what every form of rph_hamming_nearest refuses, checked before anything is written (host_grouping.cpp)
int rph_nearest_check(const char *who, const void *rows, uint32_t n_variants, uint64_t n_lib, const void *hashes_q, uint64_t n_q, uint32_t k, const void *out);
// takes ctx->mu and the sweep scratch for the partial lists; asynchronous on `stream`
int rph_nearest_run(rph_ctx *ctx, const rph_nearest &q, hipStream_t stream);
// how a call is cut (exported for the tests, not in the header): out[0..4] = files per MFMA block, files per segment, queries per
// tile, number of segments, queries per chunk
extern "C" void rph_debug_nearest_layout(uint64_t n_lib, uint32_t n_variants, uint64_t n_q, uint32_t k, uint32_t *out);
// forces the segment length of the calls that follow, in files (rounded up to whole MFMA blocks); 0 restores the default.  It lets a
// library of a few thousand files reach many segments (tests only)
extern "C" void rph_debug_nearest_set_segment(uint32_t files);
// bounds the partial lists of the calls that follow, in bytes; 0 restores 256 MiB, anything below one tile of 64-key lists in one
// segment (8192) is raised to that.  It lets a few dozen queries reach several chunks (tests only)
extern "C" void rph_debug_nearest_set_workspace(uint64_t bytes);
int rph_launch_mih_build256(rph_ctx *ctx, const uint8_t *d_hashes, uint64_t n, uint32_t *d_offsets, uint32_t *d_values,
                            hipStream_t stream);
int rph_launch_mih_build64(rph_ctx *ctx, const uint64_t *d_hashes, uint64_t n, uint32_t *d_offsets, uint32_t *d_values,
                           hipStream_t stream);
// synth_kernels.hip
int rph_launch_synth_images(uint8_t *d_out, uint64_t first_k, uint32_t n, uint32_t w, uint32_t h, uint32_t seed,
                            hipStream_t stream);
int rph_launch_synth_hashes(uint8_t *d_out, uint64_t first, uint64_t count, uint64_t n_total, uint64_t seed,
                            uint64_t n_clusters, hipStream_t stream);

// blake3_kernels.hip: pixel hashes (BLAKE3 of to_rgba16()) of n images of one checked geometry; d_scratch: rph_pixel_hash_scratch_bytes()
// of device memory used in stream order (nullptr when that is 0)
size_t rph_pixel_hash_scratch_bytes(uint32_t n, uint32_t w, uint32_t h);
int rph_launch_pixel_hash(const uint8_t *d_px, uint32_t n, uint32_t w, uint32_t h, uint32_t channels, size_t row_stride, size_t image_stride,
                          uint8_t *d_hash32, hipStream_t stream, void *d_scratch);
// the same for n images of any mix of geometries and layouts (RPH_LAYOUT_*), image i at d_px + src_off: the host plans the call into one
// descriptor per image and the prefix table of 64-chunk groups, the caller uploads both and gives 32 bytes of scratch per group
struct RphPixelImage {
    uint64_t src_off, row_stride;
    uint32_t w, h, layout, pad;
};
bool rph_pixel_hash_ragged_plan(const uint64_t *offset, const uint32_t *w, const uint32_t *h, const uint32_t *layout, const size_t *row_stride, uint32_t n,
                                std::vector<RphPixelImage> &desc, std::vector<uint32_t> &group_first);
int rph_launch_pixel_hash_ragged(const uint8_t *d_px, const RphPixelImage *d_desc, const uint32_t *d_group_first, uint32_t n, uint32_t groups, bool multi_group,
                                 uint32_t *d_cvs, uint8_t *d_hash32, hipStream_t stream);

// png_kernels.hip: one wave per zlib stream (rphp::StreamDesc: compressed bytes, destination, the image whose status a refused stream
// sets); the TIFF path runs its Deflate strips and tiles through it too
int rph_png_launch_inflate(const uint8_t *d_comp, const void *d_streams, uint32_t n, uint8_t *d_raw, int32_t *d_status, hipStream_t s);

int rph_launch_read_stream(const void *d_buf, size_t bytes, uint32_t *d_sink, hipStream_t stream);

// Runs an entry point's body; no C++ exception crosses the C ABI ("nothing aborts", include/rupphash.h)
template <class F>
static inline int rph_guarded(const char *where, F &&body) noexcept
{
    try {
        return body();
    } catch (const std::bad_alloc &) {
        rph_set_error("%s: out of host memory", where);
        return RPH_ERR_OOM;
    } catch (const std::exception &e) {
        rph_set_error("%s: %s", where, e.what());
        return RPH_ERR_HIP;
    } catch (...) {
        rph_set_error("%s: unknown exception", where);
        return RPH_ERR_HIP;
    }
}

// rph_api.cpp
void rph_pipe_forget(rph_ctx *ctx);
int rph_pdq_hash_batch_keep(rph_ctx *ctx, const uint8_t *px, uint32_t n, uint32_t w, uint32_t h, uint32_t channels, size_t row_stride,
                            size_t image_stride, uint8_t *hash32_out, float *quality_out, float *coeffs_out, uint8_t *dihedral_out,
                            uint8_t *valid_out, void *d_hash_keep, void *d_quality_keep, void *d_dihedral_keep);
// batcher.cpp
void rph_batcher_forget(rph_ctx *ctx);
// resize_kernels.hip
void rph_resize_forget(rph_ctx *ctx);
// jpeg_pipeline.cpp
void rph_jpeg_forget(rph_ctx *ctx);
// png_pipeline.cpp
void rph_png_forget(rph_ctx *ctx);
// tiff_pipeline.cpp
void rph_tiff_forget(rph_ctx *ctx);
// webp_pipeline.cpp
void rph_webp_forget(rph_ctx *ctx);
// gif_pipeline.cpp
void rph_gif_forget(rph_ctx *ctx);
// bmp_pipeline.cpp
void rph_bmp_forget(rph_ctx *ctx);
void rph_jpeg_forget_threads(rph_ctx *ctx);

// host_grouping.cpp
int rph_host_union_find(const rph_edge *edges, uint64_t n_edges, uint64_t n, uint32_t *members, uint32_t *offsets,
                        uint32_t *n_groups_out);
// the same union-find started from the components of an earlier call (old_members / old_offsets as it returned them, validated here)
int rph_host_union_find_append(const uint32_t *old_members, const uint32_t *old_offsets, uint32_t n_old_groups, const rph_edge *edges,
                               uint64_t n_edges, uint64_t n, uint32_t *members, uint32_t *offsets, uint32_t *n_groups_out);
int rph_host_find_groups(const rph_edge *edges, uint64_t n_edges, uint64_t n, uint32_t *members, uint32_t *offsets,
                         uint32_t *n_groups_out);
