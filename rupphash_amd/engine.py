"""Engine: one rph_ctx (one GPU) with numpy-friendly wrappers over the C ABI.

Everything here is argument marshalling; all arithmetic happens inside
librupphash_hip.so on the GPU (or, for the reference's serial host logic such
as union-find, in the library's C++).
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import RphEdge, check

EDGE_DTYPE = np.dtype([("i", np.uint32), ("j", np.uint32), ("d", np.uint16), ("flags", np.uint16)])


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _ragged_view(image):
    """(h, w), (h, w, 3) or (h, w, 4) uint8 -> (array, h, w, channels, row stride): the array as it is if its pixels are interleaved
    bytes and its rows lie at one non-negative distance >= w * channels (a slice of a larger array), else a contiguous copy."""
    a = np.asarray(image, np.uint8)
    if a.ndim not in (2, 3) or (a.ndim == 3 and a.shape[2] not in (3, 4)):
        raise ValueError(f"image of shape {a.shape}: (h, w), (h, w, 3) or (h, w, 4) wanted")
    h, w = a.shape[:2]
    ch = 1 if a.ndim == 2 else a.shape[2]
    inner = (1,) if a.ndim == 2 else (ch, 1)
    if h and w and (a.strides[1:] != inner or (h > 1 and a.strides[0] < w * ch)):
        a = np.ascontiguousarray(a)
    return a, h, w, ch, (a.strides[0] if h > 1 and w else w * ch)


def ragged_pack(images, align=16, pitch_align=4, fill=0):
    """The packed form of a list of images for Engine.pdq_hash_ragged_dev: one uint8 buffer with image i at offset[i] (a multiple of
    `align`), its rows row_stride[i] = w * channels rounded up to `pitch_align` bytes apart; gaps and row padding hold `fill`.
    Returns (buffer, offset uint64, w uint32, h uint32, channels uint32, row_stride uintp)."""
    views = [_ragged_view(im) for im in images]
    n = len(views)
    offset, ws, hs, chs, rs = np.zeros(n, np.uint64), np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uintp)
    end = 0
    for i, (a, h, w, ch, _) in enumerate(views):
        pitch = -(-(w * ch) // pitch_align) * pitch_align
        at = -(-end // align) * align
        offset[i], ws[i], hs[i], chs[i], rs[i] = at, w, h, ch, pitch
        end = at + pitch * h
    buf = np.full(max(end, 1), fill, np.uint8)
    for i, (a, h, w, ch, _) in enumerate(views):
        if h and w:
            rows = np.lib.stride_tricks.as_strided(buf[int(offset[i]):], (h, w * ch), (int(rs[i]), 1), writeable=True)
            rows[...] = a.reshape(h, w * ch) if a.flags.c_contiguous else np.ascontiguousarray(a).reshape(h, w * ch)
    return buf, offset, ws, hs, chs, rs


def _image_view(image):
    """(h, w), (h, w, 2), (h, w, 3) or (h, w, 4), uint8 or uint16 -> (array, h, w, layout, row stride in bytes): _ragged_view for every
    layout of rph_image_hash_ragged (layout = channels + 16 for uint16).  Other dtypes are taken as uint8, as np.asarray(image, np.uint8)."""
    a = np.asarray(image)
    if a.dtype.kind == "u" and a.dtype.itemsize == 2:
        a = a if a.dtype.isnative else a.astype(np.uint16)
    else:
        a = np.asarray(a, np.uint8)
    if a.ndim not in (2, 3) or (a.ndim == 3 and a.shape[2] not in (2, 3, 4)):
        raise ValueError(f"image of shape {a.shape}: (h, w), (h, w, 2), (h, w, 3) or (h, w, 4) wanted")
    h, w = a.shape[:2]
    ch, bps = (1 if a.ndim == 2 else a.shape[2]), a.dtype.itemsize
    inner = (bps,) if a.ndim == 2 else (ch * bps, bps)
    if h and w and (a.strides[1:] != inner or (h > 1 and a.strides[0] < w * ch * bps) or (a.ctypes.data | a.strides[0]) % bps):
        a = np.ascontiguousarray(a)
    return a, h, w, ch + (16 if bps == 2 else 0), (a.strides[0] if h > 1 and w else w * ch * bps)


def image_pack(images, align=16, pitch_align=4, fill=0):
    """ragged_pack for Engine.image_hash_ragged_dev: one uint8 buffer with image i (uint8 or uint16, 1 to 4 channels) at offset[i] (a
    multiple of `align`; rounded up to an even number for a 16-bit image), its rows row_stride[i] = the row's bytes rounded up to
    `pitch_align` (and to 2 for a 16-bit image) apart; 16-bit samples in native byte order; gaps and row padding hold `fill`.
    Returns (buffer, offset uint64, w uint32, h uint32, layout uint32, row_stride uintp)."""
    views = [_image_view(im) for im in images]
    n = len(views)
    offset, ws, hs, ls, rs = np.zeros(n, np.uint64), np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uintp)
    end = 0
    for i, (a, h, w, layout, _) in enumerate(views):
        row, even = w * (layout & 15) * a.dtype.itemsize, a.dtype.itemsize
        pitch = -(-(-(-row // pitch_align) * pitch_align) // even) * even
        at = -(-(-(-end // align) * align) // even) * even
        offset[i], ws[i], hs[i], ls[i], rs[i] = at, w, h, layout, pitch
        end = at + pitch * h
    buf = np.full(max(end, 1), fill, np.uint8)
    for i, (a, h, w, layout, _) in enumerate(views):
        if h and w:
            row = w * (layout & 15) * a.dtype.itemsize
            rows = np.lib.stride_tricks.as_strided(buf[int(offset[i]):], (h, row), (int(rs[i]), 1), writeable=True)
            rows[...] = np.ascontiguousarray(a).view(np.uint8).reshape(h, row)
    return buf, offset, ws, hs, ls, rs


class Engine:
    def __init__(self, device=0):
        self.L = _lib.load()
        h = C.c_void_p()
        check(self.L.rph_init(device, C.byref(h)), "rph_init")
        self.ctx = h
        self.device = device

    def close(self):
        if getattr(self, "ctx", None):
            self.L.rph_shutdown(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- info / sync ----
    def device_info(self):
        name = C.create_string_buffer(64)
        cus = C.c_int()
        mem = C.c_uint64()
        check(self.L.rph_device_info(self.ctx, name, C.byref(cus), C.byref(mem)), "rph_device_info")
        return name.value.decode(), cus.value, mem.value

    def synchronize(self):
        check(self.L.rph_synchronize(self.ctx), "rph_synchronize")

    @property
    def stream(self):
        return self.L.rph_stream(self.ctx)

    def set_pdq_kernel(self, which):
        check(self.L.rph_pdq_set_kernel(self.ctx, which), "rph_pdq_set_kernel")

    def set_hamming_kernel(self, which):
        check(self.L.rph_hamming_set_kernel(self.ctx, which), "rph_hamming_set_kernel")

    # ---- PDQ ----
    def pdq_hash_batch(self, images, want_quality=True, want_coeffs=False, want_dihedral=False):
        """images: uint8 (n,h,w,3|4) or (n,h,w) [Luma8].  Returns dict(hash, quality, coeffs, dihedral, valid)."""
        images = np.ascontiguousarray(images, np.uint8)
        if images.ndim == 3:
            n, h, w = images.shape
            ch = 1
        else:
            n, h, w, ch = images.shape
        out = {
            "hash": np.zeros((n, 32), np.uint8),
            "quality": np.zeros(n, np.float32) if want_quality else None,
            "coeffs": np.zeros((n, 256), np.float32) if want_coeffs else None,
            "dihedral": np.zeros((n, 8, 32), np.uint8) if want_dihedral else None,
            "valid": np.zeros(n, np.uint8),
        }
        check(self.L.rph_pdq_hash_batch(self.ctx, _ptr(images), n, w, h, ch, w * ch, w * h * ch, _ptr(out["hash"]),
                                        _ptr(out["quality"]), _ptr(out["coeffs"]), _ptr(out["dihedral"]), _ptr(out["valid"])),
              "rph_pdq_hash_batch")
        return out

    def pdq_hash_ragged(self, images, want_quality=True, want_coeffs=False, want_dihedral=False):
        """images: a list of uint8 arrays (h, w) [Luma8], (h, w, 3) or (h, w, 4) of ANY mix of sizes, rows possibly non-contiguous (slices
        of larger arrays are read where they are).  One call; returns dict(hash, quality, coeffs, dihedral, valid) like pdq_hash_batch,
        entry i for image i (valid 0 and zeros for an image with a side < 5)."""
        views = [_ragged_view(im) for im in images]
        n = len(views)
        px = (C.c_void_p * max(n, 1))(*[v[0].ctypes.data for v in views])
        h = np.array([v[1] for v in views], np.uint32)
        w = np.array([v[2] for v in views], np.uint32)
        ch = np.array([v[3] for v in views], np.uint32)
        rs = (C.c_size_t * max(n, 1))(*[v[4] for v in views])
        out = {
            "hash": np.zeros((n, 32), np.uint8),
            "quality": np.zeros(n, np.float32) if want_quality else None,
            "coeffs": np.zeros((n, 256), np.float32) if want_coeffs else None,
            "dihedral": np.zeros((n, 8, 32), np.uint8) if want_dihedral else None,
            "valid": np.zeros(n, np.uint8),
        }
        check(self.L.rph_pdq_hash_ragged(self.ctx, px, _ptr(w), _ptr(h), _ptr(ch), rs, n, _ptr(out["hash"]), _ptr(out["quality"]), _ptr(out["coeffs"]),
                                         _ptr(out["dihedral"]), _ptr(out["valid"])), "rph_pdq_hash_ragged")
        return out

    def pdq_hash_ragged_dev(self, d_px, offset, w, h, channels, row_stride, d_hash, d_quality=None, d_coeffs=None, d_dihedral=None, d_valid=None,
                            stream=None):
        """Images on the device: image i at d_px + offset[i]; the descriptor arrays are host arrays (ragged_pack() makes them).
        Asynchronous on `stream`; results in slot i of the device output arrays."""
        offset = np.ascontiguousarray(offset, np.uint64)
        w, h, channels = (np.ascontiguousarray(a, np.uint32) for a in (w, h, channels))
        row_stride = np.ascontiguousarray(row_stride, np.uintp)
        n = len(offset)
        if not (len(w) == len(h) == len(channels) == len(row_stride) == n):
            raise ValueError("descriptor arrays of different lengths")
        check(self.L.rph_pdq_hash_ragged_dev(self.ctx, d_px, _ptr(offset), _ptr(w), _ptr(h), _ptr(channels), row_stride.ctypes.data_as(C.POINTER(C.c_size_t)), n,
                                             d_hash, d_quality, d_coeffs, d_dihedral, d_valid, stream), "rph_pdq_hash_ragged_dev")

    def image_hash_ragged(self, images, want_pdq=True, want_pixel_hash=True, want_quality=True, want_coeffs=False, want_dihedral=False):
        """What the scan computes per decoded image (scanner.rs:1386-1410), one call for a list of images of ANY mix of sizes and layouts:
        uint8 or uint16 arrays (h, w), (h, w, 2) [gray + alpha], (h, w, 3) or (h, w, 4), slices of larger arrays read where they lie.
        Returns dict(hash, quality, coeffs, dihedral, valid, pixel_hash); the PDQ entries are None without want_pdq, pixel_hash (n x 32)
        without want_pixel_hash.  valid 0 and zeros for an image with a side < 5; its pixel hash is still there."""
        if not (want_pdq or want_pixel_hash):
            raise ValueError("image_hash_ragged: neither hash wanted")
        views = [_image_view(im) for im in images]
        n = len(views)
        px = (C.c_void_p * max(n, 1))(*[v[0].ctypes.data for v in views])
        h = np.array([v[1] for v in views], np.uint32)
        w = np.array([v[2] for v in views], np.uint32)
        layout = np.array([v[3] for v in views], np.uint32)
        rs = (C.c_size_t * max(n, 1))(*[v[4] for v in views])
        out = {
            "hash": np.zeros((n, 32), np.uint8) if want_pdq else None,
            "quality": np.zeros(n, np.float32) if want_pdq and want_quality else None,
            "coeffs": np.zeros((n, 256), np.float32) if want_pdq and want_coeffs else None,
            "dihedral": np.zeros((n, 8, 32), np.uint8) if want_pdq and want_dihedral else None,
            "valid": np.zeros(n, np.uint8) if want_pdq else None,
            "pixel_hash": np.zeros((n, 32), np.uint8) if want_pixel_hash else None,
        }
        check(self.L.rph_image_hash_ragged(self.ctx, px, _ptr(w), _ptr(h), _ptr(layout), rs, n, _ptr(out["hash"]), _ptr(out["quality"]), _ptr(out["coeffs"]),
                                           _ptr(out["dihedral"]), _ptr(out["valid"]), _ptr(out["pixel_hash"])), "rph_image_hash_ragged")
        return out

    def image_hash_ragged_dev(self, d_px, offset, w, h, layout, row_stride, d_hash=None, d_quality=None, d_coeffs=None, d_dihedral=None, d_valid=None,
                              d_pixel_hash=None, stream=None):
        """Images on the device: image i at d_px + offset[i]; the descriptor arrays are host arrays (image_pack() makes them).
        Asynchronous on `stream`; results in slot i of the device output arrays that are given (d_hash, d_pixel_hash or both)."""
        offset = np.ascontiguousarray(offset, np.uint64)
        w, h, layout = (np.ascontiguousarray(a, np.uint32) for a in (w, h, layout))
        row_stride = np.ascontiguousarray(row_stride, np.uintp)
        n = len(offset)
        if not (len(w) == len(h) == len(layout) == len(row_stride) == n):
            raise ValueError("descriptor arrays of different lengths")
        check(self.L.rph_image_hash_ragged_dev(self.ctx, d_px, _ptr(offset), _ptr(w), _ptr(h), _ptr(layout), row_stride.ctypes.data_as(C.POINTER(C.c_size_t)), n,
                                               d_hash, d_quality, d_coeffs, d_dihedral, d_valid, d_pixel_hash, stream), "rph_image_hash_ragged_dev")

    @staticmethod
    def image_luma601_host(image):
        """Host restatement (no GPU call): the Luma8 plane (h, w) the PDQ hasher sees for an image of any layout."""
        a, h, w, layout, rs = _image_view(image)
        out = np.zeros((h, w), np.uint8)
        check(_lib.load().rph_image_luma601_host(C.c_void_p(a.ctypes.data), w, h, layout, rs, _ptr(out)), "rph_image_luma601_host")
        return out

    @staticmethod
    def image_pixel_hash_host(image):
        """Host restatement (no GPU call): the pixel hash (32 bytes) of an image of any layout."""
        a, h, w, layout, rs = _image_view(image)
        out = np.zeros(32, np.uint8)
        check(_lib.load().rph_image_pixel_hash_host(C.c_void_p(a.ctypes.data), w, h, layout, rs, _ptr(out)), "rph_image_pixel_hash_host")
        return out.tobytes()

    def pdq_hash_one(self, image, want_coeffs=True):
        """One image through the batching queue (thread-safe; concurrent callers share a GPU batch).
        Returns (hash, quality, coeffs or None) or None when the image is too small (pdqhash.rs:167-169)."""
        image = np.ascontiguousarray(image, np.uint8)
        if image.ndim == 2:
            h, w = image.shape
            ch = 1
        else:
            h, w, ch = image.shape
        hash32 = np.zeros(32, np.uint8)
        q = C.c_float()
        coeffs = np.zeros(256, np.float32) if want_coeffs else None
        valid = C.c_uint8()
        check(self.L.rph_pdq_hash_one(self.ctx, _ptr(image), w, h, ch, w * ch, _ptr(hash32), C.cast(C.byref(q), C.c_void_p), _ptr(coeffs),
                                      C.cast(C.byref(valid), C.c_void_p)), "rph_pdq_hash_one")
        if not valid.value:
            return None
        return hash32, q.value, coeffs

    # ---- JPEG (scanner.rs:461-508) ----
    @staticmethod
    def jpeg_info(data):
        """(w, h, channels) from the frame header (host code), or raises RphError (RPH_ERR_UNSUPPORTED / RPH_ERR_INVALID_ARG)."""
        w, h, c = C.c_uint32(), C.c_uint32(), C.c_uint32()
        check(_lib.load().rph_jpeg_info(data, len(data), C.byref(w), C.byref(h), C.byref(c)), "rph_jpeg_info")
        return w.value, h.value, c.value

    @staticmethod
    def jpeg_coefficients(data):
        """The host half alone: (geometry[ncomp][8], qt[4][64], coef[total_blocks][64]) -- quantised coefficients in natural order."""
        L = _lib.load()
        _, _, c = Engine.jpeg_info(data)
        geo = np.zeros((3, 8), np.uint32)
        qt = np.zeros((4, 64), np.uint16)
        total = C.c_uint64()
        check(L.rph_jpeg_coefficients(data, len(data), _ptr(geo), _ptr(qt), None, 0, C.byref(total)), "rph_jpeg_coefficients")
        coef = np.zeros((total.value, 64), np.int16)
        check(L.rph_jpeg_coefficients(data, len(data), _ptr(geo), _ptr(qt), _ptr(coef), total.value, C.byref(total)), "rph_jpeg_coefficients")
        return geo[:c], qt, coef

    def jpeg_set_entropy(self, where):
        """0 = Huffman streams decoded by host threads, 1 = on the device, 2 = automatic (default), 3 = device for sequential files only"""
        check(self.L.rph_jpeg_set_entropy(self.ctx, int(where)), "rph_jpeg_set_entropy")

    def jpeg_pdq_hash_one(self, data, flavour=0, want_coeffs=True):
        """One JPEG file per call, thread-safe (concurrent callers share a batch): (hash, quality, coeffs or None), None when the image is
        below 5 px; raises RphError for a file the library does not decode."""
        hash32 = np.zeros(32, np.uint8)
        q = C.c_float()
        coeffs = np.zeros(256, np.float32) if want_coeffs else None
        valid = C.c_uint8()
        check(self.L.rph_jpeg_pdq_hash_one(self.ctx, data, len(data), int(flavour), _ptr(hash32), C.cast(C.byref(q), C.c_void_p), _ptr(coeffs),
                                           C.cast(C.byref(valid), C.c_void_p)), "rph_jpeg_pdq_hash_one")
        return (hash32, q.value, coeffs) if valid.value else None

    def jpeg_set_segments(self, min_stream_bytes=8192, segment_bytes=1024):
        """device walk of streams without restart markers: cut into segments from min_stream_bytes of entropy data (segment_bytes = 0: never)"""
        check(self.L.rph_jpeg_set_segments(self.ctx, int(min_stream_bytes), int(segment_bytes)), "rph_jpeg_set_segments")

    def debug_jpeg_segment_log(self, on):
        """Record what the segment synchroniser decides in every chunk of a JPEG batch call (off by default; the outputs are the same
        either way).  Debug / tests only."""
        check(self.L.rph_debug_jpeg_segment_log(self.ctx, int(bool(on))), "rph_debug_jpeg_segment_log")

    SEG_LOG_FILE_FIELDS = ("index", "n_segs", "total_mcus", "scan_bits", "verified", "first_record", "first_seg", "n_luts")
    SEG_LOG_SEG_FIELDS = ("entry", "out", "count", "dc0", "dc1", "dc2", "from", "out_check", "round0_n", "round0_out", "mcu_first", "mcu_count",
                          "stream_off", "bit_skip", "item_dc0", "item_dc1", "item_dc2", "decodes", "decoded_bits")

    def debug_jpeg_segments(self):
        """The log of the last JPEG batch call made with debug_jpeg_segment_log(True): (files, segments), two dicts of arrays with one
        entry per segmented file (SEG_LOG_FILE_FIELDS, uint32; a file's segments are records first_record .. first_record + n_segs - 1)
        and per segment (SEG_LOG_SEG_FIELDS; positions uint32 with 0xFFFFFFFF = none, the DC sums int32).  Debug / tests only."""
        nf, ns = C.c_uint32(), C.c_uint32()
        check(self.L.rph_debug_jpeg_segments(self.ctx, None, 0, C.byref(nf), None, 0, C.byref(ns)), "rph_debug_jpeg_segments")
        files = np.zeros((nf.value, len(self.SEG_LOG_FILE_FIELDS)), np.uint32)
        segs = np.zeros((ns.value, len(self.SEG_LOG_SEG_FIELDS)), np.uint32)
        check(self.L.rph_debug_jpeg_segments(self.ctx, _ptr(files), nf.value, C.byref(nf), _ptr(segs), ns.value, C.byref(ns)), "rph_debug_jpeg_segments")
        f = {name: files[:, k].copy() for k, name in enumerate(self.SEG_LOG_FILE_FIELDS)}
        s = {name: segs[:, k].copy().view(np.int32) if "dc" in name else segs[:, k].copy() for k, name in enumerate(self.SEG_LOG_SEG_FIELDS)}
        return f, s

    def jpeg_release(self):
        """give the JPEG path's cached staging / device buffers back"""
        check(self.L.rph_jpeg_release(self.ctx), "rph_jpeg_release")

    def jpeg_decode(self, data, flavour=0):
        """load_image_fast for one JPEG byte string: (h, w) uint8 [Luma8] or (h, w, 3) [Rgb8], decoded on the device."""
        w, h, c = self.jpeg_info(data)
        out = np.zeros((h, w, 3) if c == 3 else (h, w), np.uint8)
        check(self.L.rph_jpeg_decode(self.ctx, data, len(data), int(flavour), _ptr(out)), "rph_jpeg_decode")
        return out

    @staticmethod
    def jpeg_file_list(files):
        """The (pointer array, length array, n) a C caller would hold: build it once when the same files are hashed repeatedly"""
        n = len(files)
        return (C.c_char_p * n)(*files), (C.c_size_t * n)(*[len(f) for f in files]), n

    def jpeg_pdq_hash_batch(self, files, flavour=0, threads=0, want_quality=True, want_coeffs=False, want_dihedral=False, want_pixel_hash=False):
        """files: list of JPEG byte strings (any mix of sizes), or the tuple jpeg_file_list() made of one.  Returns dict(hash, quality,
        coeffs, dihedral, valid, status): valid[i] = 0 with status[i] != 0 for a file that cannot be decoded, valid[i] = 0 with status 0
        for an image below 5 px.  want_pixel_hash adds "pixel_hash" (n x 32: BLAKE3 of to_rgba16() of each decoded image, zero bytes
        where status != 0) through rph_jpeg_pdq_pixel_hash_batch."""
        arr, lens, n = files if isinstance(files, tuple) else self.jpeg_file_list(files)
        out = {
            "hash": np.zeros((n, 32), np.uint8),
            "quality": np.zeros(n, np.float32) if want_quality else None,
            "coeffs": np.zeros((n, 256), np.float32) if want_coeffs else None,
            "dihedral": np.zeros((n, 8, 32), np.uint8) if want_dihedral else None,
            "valid": np.zeros(n, np.uint8),
            "status": np.zeros(n, np.int32),
        }
        if want_pixel_hash:
            out["pixel_hash"] = np.zeros((n, 32), np.uint8)
            check(self.L.rph_jpeg_pdq_pixel_hash_batch(self.ctx, arr, lens, n, int(flavour), int(threads), _ptr(out["hash"]), _ptr(out["quality"]),
                                                       _ptr(out["coeffs"]), _ptr(out["dihedral"]), _ptr(out["valid"]), _ptr(out["status"]),
                                                       _ptr(out["pixel_hash"])),
                  "rph_jpeg_pdq_pixel_hash_batch")
            return out
        check(self.L.rph_jpeg_pdq_hash_batch(self.ctx, arr, lens, n, int(flavour), int(threads), _ptr(out["hash"]), _ptr(out["quality"]),
                                             _ptr(out["coeffs"]), _ptr(out["dihedral"]), _ptr(out["valid"]), _ptr(out["status"])),
              "rph_jpeg_pdq_hash_batch")
        return out

    # ---- the five file formats (include/rupphash.h, PNG / TIFF / WebP / GIF / BMP sections): one body behind every format's methods ----
    @staticmethod
    def _file_info(fmt, data):
        w, h, c, d = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint32()
        check(getattr(_lib.load(), f"rph_{fmt}_info")(data, len(data), C.byref(w), C.byref(h), C.byref(c), C.byref(d)), f"rph_{fmt}_info")
        return w.value, h.value, c.value, d.value

    @staticmethod
    def _file_array(fmt, data):
        """the zeroed array of a file's native pixels: PNG and TIFF give (h, w) for one channel and uint16 at 16 bits, the others
        always (h, w, channels) uint8 (GIF: always 4 channels)"""
        w, h, c, d = Engine._file_info(fmt, data)
        if fmt in ("png", "tiff"):
            return np.zeros((h, w) if c == 1 else (h, w, c), np.uint16 if d == 16 else np.uint8)
        return np.zeros((h, w, c), np.uint8)

    @staticmethod
    def _file_decode_host(fmt, data):
        out = Engine._file_array(fmt, data)
        check(getattr(_lib.load(), f"rph_{fmt}_decode_host")(data, len(data), _ptr(out), out.nbytes), f"rph_{fmt}_decode_host")
        return out

    def _file_decode(self, fmt, data):
        out = self._file_array(fmt, data)
        check(getattr(self.L, f"rph_{fmt}_decode")(self.ctx, data, len(data), _ptr(out), out.nbytes), f"rph_{fmt}_decode")
        return out

    def _file_release(self, fmt):
        check(getattr(self.L, f"rph_{fmt}_release")(self.ctx), f"rph_{fmt}_release")

    def _file_hash_batch(self, fmt, files, threads, want_quality, want_coeffs, want_dihedral, want_pixel_hash):
        arr, lens, n = files if isinstance(files, tuple) else self.jpeg_file_list(files)
        out = {
            "hash": np.zeros((n, 32), np.uint8),
            "quality": np.zeros(n, np.float32) if want_quality else None,
            "coeffs": np.zeros((n, 256), np.float32) if want_coeffs else None,
            "dihedral": np.zeros((n, 8, 32), np.uint8) if want_dihedral else None,
            "valid": np.zeros(n, np.uint8),
            "status": np.zeros(n, np.int32),
        }
        if want_pixel_hash:
            out["pixel_hash"] = np.zeros((n, 32), np.uint8)
        check(getattr(self.L, f"rph_{fmt}_pdq_hash_batch")(self.ctx, arr, lens, n, int(threads), _ptr(out["hash"]), _ptr(out["quality"]), _ptr(out["coeffs"]),
                                                           _ptr(out["dihedral"]), _ptr(out["valid"]), _ptr(out["status"]), _ptr(out.get("pixel_hash"))),
              f"rph_{fmt}_pdq_hash_batch")
        return out

    # ---- PNG (include/rupphash.h, PNG section) ----
    @staticmethod
    def png_info(data):
        """(w, h, channels, bit_depth) of the native pixels (host code), or raises RphError by the damaged-file rule."""
        return Engine._file_info("png", data)

    @staticmethod
    def png_decode_host(data):
        """The whole decoder on the CPU: (h, w) for Luma, else (h, w, channels); uint8, or uint16 for 16-bit files."""
        return Engine._file_decode_host("png", data)

    def png_decode(self, data):
        """load_image_fast for one PNG byte string, decoded on the device: the same array as png_decode_host."""
        return self._file_decode("png", data)

    def png_set_inflate(self, where):
        """0 = host threads inflate, 1 = the device (one wave per stream), 2 = automatic (default)"""
        check(self.L.rph_png_set_inflate(self.ctx, int(where)), "rph_png_set_inflate")

    def png_release(self):
        """give the PNG path's cached staging / device buffers back"""
        self._file_release("png")

    def png_pdq_hash_batch(self, files, threads=0, want_quality=True, want_coeffs=False, want_dihedral=False, want_pixel_hash=False):
        """files: list of PNG byte strings (any mix), or the tuple jpeg_file_list() made of one.  Returns dict(hash, quality, coeffs,
        dihedral, valid, status[, pixel_hash]) as jpeg_pdq_hash_batch: status[i] != 0 for a file the rule refuses (zero outputs),
        valid[i] = 0 with status 0 for an image below 5 px (which still has its pixel hash)."""
        return self._file_hash_batch("png", files, threads, want_quality, want_coeffs, want_dihedral, want_pixel_hash)

    # ---- TIFF (include/rupphash.h, TIFF section) ----
    @staticmethod
    def tiff_info(data):
        """(w, h, channels, bit_depth) of the native pixels (host code), or raises RphError by the damaged-file rule."""
        return Engine._file_info("tiff", data)

    @staticmethod
    def tiff_decode_host(data):
        """The whole decoder on the CPU: (h, w) for Luma, else (h, w, channels); uint8, or uint16 for 16-bit files."""
        return Engine._file_decode_host("tiff", data)

    def tiff_decode(self, data):
        """load_image_fast for one TIFF byte string, decoded on the device: the same array as tiff_decode_host."""
        return self._file_decode("tiff", data)

    def tiff_set_decompress(self, where):
        """0 = host threads decompress, 1 = the device (one wave per strip or tile), 2 = automatic (default)"""
        check(self.L.rph_tiff_set_decompress(self.ctx, int(where)), "rph_tiff_set_decompress")

    def tiff_release(self):
        """give the TIFF path's cached staging / device buffers back"""
        self._file_release("tiff")

    def tiff_pdq_hash_batch(self, files, threads=0, want_quality=True, want_coeffs=False, want_dihedral=False, want_pixel_hash=False):
        """files: list of TIFF byte strings (any mix), or the tuple jpeg_file_list() made of one.  Returns dict(hash, quality, coeffs,
        dihedral, valid, status[, pixel_hash]) as jpeg_pdq_hash_batch: status[i] != 0 for a file the rule refuses (zero outputs),
        valid[i] = 0 with status 0 for an image below 5 px (which still has its pixel hash)."""
        return self._file_hash_batch("tiff", files, threads, want_quality, want_coeffs, want_dihedral, want_pixel_hash)

    # ---- WebP (include/rupphash.h, WebP section) ----
    @staticmethod
    def webp_info(data):
        """(w, h, channels, bit_depth) of the native pixels (host code), or raises RphError by the damaged-file rule."""
        return Engine._file_info("webp", data)

    @staticmethod
    def webp_decode_host(data):
        """The whole decoder on the CPU: (h, w, 3) Rgb8 or (h, w, 4) Rgba8, uint8."""
        return Engine._file_decode_host("webp", data)

    def webp_decode(self, data):
        """load_image_fast for one WebP byte string, decoded on the device: the same array as webp_decode_host."""
        return self._file_decode("webp", data)

    def webp_set_entropy(self, where):
        """0 = host threads decode the main ARGB stream, 1 = the device (one wave per stream), 2 = automatic (default)"""
        check(self.L.rph_webp_set_entropy(self.ctx, int(where)), "rph_webp_set_entropy")

    def webp_release(self):
        """give the WebP path's cached staging / device buffers back"""
        self._file_release("webp")

    def webp_pdq_hash_batch(self, files, threads=0, want_quality=True, want_coeffs=False, want_dihedral=False, want_pixel_hash=False):
        """files: list of lossless WebP byte strings (any mix), or the tuple jpeg_file_list() made of one.  Returns dict(hash, quality, coeffs,
        dihedral, valid, status[, pixel_hash]) as jpeg_pdq_hash_batch: status[i] != 0 for a file the rule refuses (zero outputs),
        valid[i] = 0 with status 0 for an image below 5 px (which still has its pixel hash)."""
        return self._file_hash_batch("webp", files, threads, want_quality, want_coeffs, want_dihedral, want_pixel_hash)

    # ---- GIF (include/rupphash.h, GIF section) ----
    @staticmethod
    def gif_info(data):
        """(w, h, channels, bit_depth) of the native pixels (host code), or raises RphError by the damaged-file rule."""
        return Engine._file_info("gif", data)

    @staticmethod
    def gif_decode_host(data):
        """The whole decoder on the CPU: (h, w, 4) Rgba8 at the logical screen's size, uint8."""
        return Engine._file_decode_host("gif", data)

    def gif_decode(self, data):
        """The first frame of one GIF byte string on its screen, decoded on the device: the same array as gif_decode_host."""
        return self._file_decode("gif", data)

    def gif_set_decompress(self, where):
        """0 = host threads decode the LZW streams, 1 = the device (one wave per file), 2 = automatic (default)"""
        check(self.L.rph_gif_set_decompress(self.ctx, int(where)), "rph_gif_set_decompress")

    def gif_release(self):
        """give the GIF path's cached staging / device buffers back"""
        self._file_release("gif")

    def gif_pdq_hash_batch(self, files, threads=0, want_quality=True, want_coeffs=False, want_dihedral=False, want_pixel_hash=False):
        """files: list of GIF byte strings (any mix), or the tuple jpeg_file_list() made of one.  Returns dict(hash, quality, coeffs,
        dihedral, valid, status[, pixel_hash]) as jpeg_pdq_hash_batch: status[i] != 0 for a file the rule refuses (zero outputs),
        valid[i] = 0 with status 0 for an image below 5 px (which still has its pixel hash)."""
        return self._file_hash_batch("gif", files, threads, want_quality, want_coeffs, want_dihedral, want_pixel_hash)

    # ---- BMP (include/rupphash.h, BMP section) ----
    @staticmethod
    def bmp_info(data):
        """(w, h, channels, bit_depth) of the native pixels (host code), or raises RphError by the damaged-file rule."""
        return Engine._file_info("bmp", data)

    @staticmethod
    def bmp_decode_host(data):
        """The whole decoder on the CPU: (h, w, 3) Rgb8, or (h, w, 4) Rgba8 for a file with an alpha mask; uint8, top-down."""
        return Engine._file_decode_host("bmp", data)

    def bmp_decode(self, data):
        """One BMP byte string decoded on the device: the same array as bmp_decode_host."""
        return self._file_decode("bmp", data)

    def bmp_release(self):
        """give the BMP path's cached staging / device buffers back"""
        self._file_release("bmp")

    def bmp_pdq_hash_batch(self, files, threads=0, want_quality=True, want_coeffs=False, want_dihedral=False, want_pixel_hash=False):
        """files: list of BMP byte strings (any mix of sizes and depths), or the tuple jpeg_file_list() made of one.  Returns dict(hash,
        quality, coeffs, dihedral, valid, status[, pixel_hash]) as jpeg_pdq_hash_batch: status[i] != 0 for a file the rule refuses (zero
        outputs), valid[i] = 0 with status 0 for an image below 5 px (which still has its pixel hash)."""
        return self._file_hash_batch("bmp", files, threads, want_quality, want_coeffs, want_dihedral, want_pixel_hash)

    # ---- a mixed list of files (include/rupphash.h, the files section) ----
    @staticmethod
    def file_format(data, name=None):
        """The pipeline that takes a file (_lib.RPH_FORMAT_*: 0 none, 1 jpeg, 2 png, 3 tiff, 4 webp, 5 gif, 6 bmp) by the routing rule:
        the extension of `name` (str, bytes or None) rules out RAW, jxl and pdf names, else the bytes' magic decides.  Host code."""
        return _lib.load().rph_file_format(data, len(data) if data is not None else 0, Engine._name_bytes(name))

    @staticmethod
    def _name_bytes(name):
        return None if name is None else (bytes(name) if isinstance(name, (bytes, bytearray)) else str(name).encode("utf-8", "surrogateescape"))

    @staticmethod
    def files_list(files, names=None):
        """The (pointers, lengths, names, n) a C caller would hold; a file may be None (a null entry), names None or a list with None entries"""
        n = len(files)
        nm = None if names is None else (C.c_char_p * n)(*[Engine._name_bytes(x) for x in names])
        return (C.c_char_p * n)(*files), (C.c_size_t * n)(*[len(f) if f is not None else 0 for f in files]), nm, n

    def files_pdq_hash_batch(self, files, names=None, flavour=0, threads=0, sequential=False, want_quality=True, want_coeffs=False, want_dihedral=False,
                             want_pixel_hash=False, concurrent=False):
        """files: list of byte strings of any mix of the six formats (or the tuple files_list() made of one, names included).  Returns the
        per-format dict(hash, quality, coeffs, dihedral, valid, status[, pixel_hash]) in the caller's order plus "format" (n uint8:
        RPH_FORMAT_* of the pipeline that took the file, 0 for a file no pipeline takes -- status RPH_ERR_UNSUPPORTED) and "size"
        (n x (w, h) of the decoded images, 0 where status != 0).  The formats run one after another (the default; `sequential` says so
        explicitly) or, with `concurrent`, each on a host thread of its own."""
        arr, lens, nm, n = files if isinstance(files, tuple) else self.files_list(files, names)
        out = {
            "hash": np.zeros((n, 32), np.uint8),
            "quality": np.zeros(n, np.float32) if want_quality else None,
            "coeffs": np.zeros((n, 256), np.float32) if want_coeffs else None,
            "dihedral": np.zeros((n, 8, 32), np.uint8) if want_dihedral else None,
            "valid": np.zeros(n, np.uint8),
            "status": np.zeros(n, np.int32),
            "format": np.zeros(n, np.uint8),
            "size": np.zeros((n, 2), np.uint32),
        }
        if want_pixel_hash:
            out["pixel_hash"] = np.zeros((n, 32), np.uint8)
        check(self.L.rph_files_pdq_hash_batch(self.ctx, arr, lens, nm, n, int(flavour), int(threads),
                                              (_lib.RPH_FILES_SEQUENTIAL if sequential else 0) | (_lib.RPH_FILES_CONCURRENT if concurrent else 0),
                                              _ptr(out["hash"]), _ptr(out["quality"]), _ptr(out["coeffs"]), _ptr(out["dihedral"]), _ptr(out["valid"]),
                                              _ptr(out["status"]), _ptr(out.get("pixel_hash")), _ptr(out["format"]), _ptr(out["size"])),
              "rph_files_pdq_hash_batch")
        return out

    def debug_files_lanes(self):
        """What the last files_pdq_hash_batch of the calling thread did: {format name: (wall ms, threads, files)} of the lanes it ran.
        Debug / tools only."""
        ms, th, nf = (C.c_double * 7)(), (C.c_uint32 * 7)(), (C.c_uint32 * 7)()
        self.L.rph_debug_files_lanes(ms, th, nf)
        return {_lib.FORMAT_NAMES[f]: (ms[f], th[f], nf[f]) for f in range(1, 7) if nf[f]}

    # ---- BLAKE3 identity hashes ----
    @staticmethod
    def blake3_host(data, key=None):
        """BLAKE3 of one byte string on the host (keyed_hash with a 32-byte key): the content hash of scanner.rs:1345."""
        data = bytes(data)
        buf = np.frombuffer(data, np.uint8) if data else None
        k = None if key is None else np.frombuffer(bytes(key), np.uint8)
        if k is not None and len(k) != 32:
            raise ValueError("blake3 key: 32 bytes")
        out = np.zeros(32, np.uint8)
        _lib.load().rph_blake3_host(_ptr(buf), len(data), _ptr(k), _ptr(out))
        return out.tobytes()

    def blake3_batch(self, strings, key=None):
        """BLAKE3 (hash, or keyed_hash with a 32-byte key) of a list of byte strings on the device: (n, 32) uint8."""
        n = len(strings)
        k = None if key is None else np.frombuffer(bytes(key), np.uint8)
        if k is not None and len(k) != 32:
            raise ValueError("blake3 key: 32 bytes")
        out = np.zeros((n, 32), np.uint8)
        arr, lens, _ = self.jpeg_file_list([bytes(x) for x in strings])
        check(self.L.rph_blake3_batch(self.ctx, arr, lens, n, _ptr(k), _ptr(out)), "rph_blake3_batch")
        return out

    def blake3_batch_dev(self, d_data, d_offsets, n, d_digest, key=None, stream=None):
        k = None if key is None else np.frombuffer(bytes(key), np.uint8)
        check(self.L.rph_blake3_batch_dev(self.ctx, d_data, d_offsets, n, _ptr(k), d_digest, stream), "rph_blake3_batch_dev")

    def pixel_hash_batch(self, images):
        """Pixel hashes (scanner.rs:1393-1404: BLAKE3 of to_rgba16()) of uint8 images (n,h,w) [Luma8] or (n,h,w,3|4): (n, 32) uint8.
        Rows and images may be strided (a view into larger buffers) as long as each row's samples are contiguous."""
        a = np.asarray(images, np.uint8)
        ch = 1 if a.ndim == 3 else a.shape[3]
        if not (a.strides[2] == ch and (a.ndim == 3 or a.strides[3] == 1)) or min(a.strides[:2]) < 0:
            a = np.ascontiguousarray(a)
        n, h, w = a.shape[:3]
        out = np.zeros((n, 32), np.uint8)
        check(self.L.rph_pixel_hash_batch(self.ctx, C.c_void_p(a.ctypes.data), n, w, h, ch, a.strides[1], a.strides[0], _ptr(out)),
              "rph_pixel_hash_batch")
        return out

    def pixel_hash_batch_dev(self, d_px, n, w, h, channels, d_hash, row_stride=None, image_stride=None, stream=None):
        row_stride = w * channels if row_stride is None else row_stride
        image_stride = row_stride * h if image_stride is None else image_stride
        check(self.L.rph_pixel_hash_batch_dev(self.ctx, d_px, n, w, h, channels, row_stride, image_stride, d_hash, stream),
              "rph_pixel_hash_batch_dev")

    def pdq_batcher_config(self, max_batch=256, max_wait_us=0):
        check(self.L.rph_pdq_batcher_config(self.ctx, max_batch, max_wait_us), "rph_pdq_batcher_config")

    def pdq_batcher_stats(self):
        nb, ni = C.c_uint64(), C.c_uint64()
        check(self.L.rph_pdq_batcher_stats(self.ctx, C.byref(nb), C.byref(ni)), "rph_pdq_batcher_stats")
        return nb.value, ni.value

    def pdq_hash_batch_dev(self, d_px, n, w, h, channels, d_hash, d_quality=None, d_coeffs=None, d_dihedral=None,
                           d_valid=None, row_stride=None, image_stride=None, stream=None):
        row_stride = w * channels if row_stride is None else row_stride
        image_stride = row_stride * h if image_stride is None else image_stride
        check(self.L.rph_pdq_hash_batch_dev(self.ctx, d_px, n, w, h, channels, row_stride, image_stride, d_hash, d_quality,
                                            d_coeffs, d_dihedral, d_valid, stream), "rph_pdq_hash_batch_dev")

    def debug_thumbnails(self, n, nw, nh):
        """The thumbnails the last pre-downsample call (a side > 512 px) of this context left in its scratch: (n, nh, nw) uint8, the
        align16(nw) row pitch of the fused forms cut away, the two-pass form's planes in front of them skipped.  Debug / tests only: ONLY
        VALID after a call of at most one chunk (the library refuses the read-back after a call of several), with no other
        pre-downsample call on this context in between -- so after pdq_hash_batch_dev, or a pdq_hash_batch of at most 64 MiB of pixels."""
        out = np.zeros((n, nh, nw), np.uint8)
        check(self.L.rph_debug_copy_thumbnails(self.ctx, _ptr(out), n, nw, nh), "rph_debug_copy_thumbnails")
        return out

    FILE_FORMATS = ("png", "tiff", "webp", "gif", "bmp")

    def debug_file_chunks(self, fmt):
        """How the last call of one file pipeline ("png", "tiff", "webp", "gif", "bmp": a batch call or a *_decode) on this context was
        cut: (files of every run_chunk call in order, number of parse windows -- counted by WebP only, 0 elsewhere).  Debug / tests only."""
        which = self.FILE_FORMATS.index(fmt)
        n, nw = C.c_uint32(), C.c_uint32()
        check(self.L.rph_debug_file_chunks(self.ctx, which, None, 0, C.byref(n), C.byref(nw)), "rph_debug_file_chunks")
        sizes = (C.c_uint32 * max(1, n.value))()
        check(self.L.rph_debug_file_chunks(self.ctx, which, sizes, n.value, C.byref(n), C.byref(nw)), "rph_debug_file_chunks")
        return list(sizes[:n.value]), nw.value

    def pdq_hashes_from_coeffs(self, coeffs, want_hash=True, want_dihedral=True):
        coeffs = np.ascontiguousarray(coeffs, np.float32).reshape(-1, 256)
        n = len(coeffs)
        hashes = np.zeros((n, 32), np.uint8) if want_hash else None
        dih = np.zeros((n, 8, 32), np.uint8) if want_dihedral else None
        check(self.L.rph_pdq_hashes_from_coeffs(self.ctx, _ptr(coeffs), n, _ptr(hashes), _ptr(dih)), "rph_pdq_hashes_from_coeffs")
        return hashes, dih

    def pdq_hashes_from_coeffs_dev(self, d_coeffs, n, d_hash=None, d_dihedral=None, stream=None):
        check(self.L.rph_pdq_hashes_from_coeffs_dev(self.ctx, d_coeffs, n, d_hash, d_dihedral, stream),
              "rph_pdq_hashes_from_coeffs_dev")

    # ---- Hamming ----
    @staticmethod
    def _sweep_growing(call, cap, grow, where):
        """The edges of call(edges, cap, found) -> status, a host sweep into a buffer of `cap` edges.  While it answers RPH_ERR_CAPACITY and
        `grow` is set, again into a buffer with room for what it found."""
        while True:
            edges = np.zeros(cap, EDGE_DTYPE)
            found = C.c_uint64()
            rc = call(_ptr(edges), cap, C.byref(found))
            if rc == _lib.RPH_ERR_CAPACITY and grow:
                cap = int(found.value) + 1024
                continue
            check(rc, where)
            return edges[: found.value]

    def hamming_all_pairs(self, hashes, threshold, part=0, nparts=1, cap=None):
        hashes = np.ascontiguousarray(hashes, np.uint8).reshape(-1, 32)
        n = len(hashes)
        return self._sweep_growing(lambda e, c, f: self.L.rph_hamming_all_pairs(self.ctx, _ptr(hashes), n, threshold, part, nparts, e, c, f),
                                   max(1 << 16, 4 * n) if cap is None else cap, True, "rph_hamming_all_pairs")

    def hamming_all_pairs_dev(self, d_hashes, n, threshold, d_edges, cap, d_count, part=0, nparts=1, stream=None):
        check(self.L.rph_hamming_all_pairs_dev(self.ctx, d_hashes, n, threshold, part, nparts, d_edges, cap, d_count, stream),
              "rph_hamming_all_pairs_dev")

    def hamming_variant_pairs(self, variants, hashes, similarity, low_conf=None, part=0, nparts=1, cap=None):
        hashes = np.ascontiguousarray(hashes, np.uint8).reshape(-1, 32)
        n = len(hashes)
        variants = np.ascontiguousarray(variants, np.uint8).reshape(n, -1, 32)
        nv = variants.shape[1]
        lc = None if low_conf is None else np.ascontiguousarray(low_conf, np.uint8)
        return self._sweep_growing(lambda e, c, f: self.L.rph_hamming_variant_pairs(self.ctx, _ptr(variants), nv, _ptr(hashes), _ptr(lc), n, similarity,
                                                                                    part, nparts, e, c, f),
                                   max(1 << 16, 8 * n) if cap is None else cap, True, "rph_hamming_variant_pairs")

    def hamming_variant_pairs_dev(self, d_variants, n_variants, d_hashes, n, similarity, d_edges, cap, d_count, d_low_conf=None,
                                  part=0, nparts=1, stream=None):
        check(self.L.rph_hamming_variant_pairs_dev(self.ctx, d_variants, n_variants, d_hashes, d_low_conf, n, similarity, part,
                                                   nparts, d_edges, cap, d_count, stream), "rph_hamming_variant_pairs_dev")

    def hamming_cross_pairs(self, a, b, threshold, part=0, nparts=1, cap=None):
        """Every pair (i in a, j in b) within `threshold`: edges with i indexing `a` and j indexing `b`."""
        return self.hamming_variant_cross_pairs(np.ascontiguousarray(a, np.uint8).reshape(-1, 1, 32), b, threshold, part=part, nparts=nparts, cap=cap)

    def hamming_cross_pairs_dev(self, d_a, n_a, d_b, n_b, threshold, d_edges, cap, d_count, part=0, nparts=1, stream=None):
        check(self.L.rph_hamming_cross_pairs_dev(self.ctx, d_a, n_a, d_b, n_b, threshold, part, nparts, d_edges, cap, d_count, stream),
              "rph_hamming_cross_pairs_dev")

    def hamming_variant_cross_pairs(self, variants_a, hashes_b, similarity, low_conf_a=None, low_conf_b=None, part=0, nparts=1, cap=None):
        """variants_a: (n_a, 1 or 8, 32) rows of set A; hashes_b: (n_b, 32).  With cap given, RPH_ERR_CAPACITY raises (RphError)."""
        hashes_b = np.ascontiguousarray(hashes_b, np.uint8).reshape(-1, 32)
        variants_a = np.ascontiguousarray(variants_a, np.uint8)
        variants_a = variants_a.reshape(-1, 1, 32) if variants_a.ndim < 3 else variants_a
        n_a, nv, n_b = variants_a.shape[0], variants_a.shape[1], len(hashes_b)
        la = None if low_conf_a is None else np.ascontiguousarray(low_conf_a, np.uint8)
        lb = None if low_conf_b is None else np.ascontiguousarray(low_conf_b, np.uint8)
        start = max(1 << 16, 8 * (n_a + n_b)) if cap is None else cap
        if nv == 1 and la is None and lb is None:
            return self._sweep_growing(lambda e, c, f: self.L.rph_hamming_cross_pairs(self.ctx, _ptr(variants_a), n_a, _ptr(hashes_b), n_b, similarity, part,
                                                                                      nparts, e, c, f), start, cap is None, "rph_hamming_cross_pairs")
        return self._sweep_growing(lambda e, c, f: self.L.rph_hamming_variant_cross_pairs(self.ctx, _ptr(variants_a), nv, _ptr(la), n_a, _ptr(hashes_b),
                                                                                          _ptr(lb), n_b, similarity, part, nparts, e, c, f),
                                   start, cap is None, "rph_hamming_variant_cross_pairs")

    def hamming_variant_cross_pairs_dev(self, d_variants_a, n_variants, n_a, d_hashes_b, n_b, similarity, d_edges, cap, d_count, d_low_conf_a=None,
                                        d_low_conf_b=None, part=0, nparts=1, stream=None):
        check(self.L.rph_hamming_variant_cross_pairs_dev(self.ctx, d_variants_a, n_variants, d_low_conf_a, n_a, d_hashes_b, d_low_conf_b, n_b,
                                                         similarity, part, nparts, d_edges, cap, d_count, stream), "rph_hamming_variant_cross_pairs_dev")

    def hamming_cross_layout(self, n_a, n_b, n_variants=1, nparts=1, kernel=2):
        """(A rides on the column side?, column tiles per block, segments per row tile, blocks) of a cross sweep: the launcher's own rule."""
        swap, seg, segs, blocks = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint64()
        self.L.rph_debug_hamming_cross_layout(n_a, n_variants, n_b, nparts, kernel, C.byref(swap), C.byref(seg), C.byref(segs), C.byref(blocks))
        return bool(swap.value), seg.value, segs.value, blocks.value

    @staticmethod
    def _groups(members, offsets, ng):
        return [members[offsets[g]:offsets[g + 1]].tolist() for g in range(ng)]

    def find_groups256(self, hashes, max_dist):
        hashes = np.ascontiguousarray(hashes, np.uint8).reshape(-1, 32)
        n = len(hashes)
        members = np.zeros(max(n, 1), np.uint32)
        offsets = np.zeros(n // 2 + 2, np.uint32)
        ng = C.c_uint32()
        check(self.L.rph_find_groups256(self.ctx, _ptr(hashes), n, max_dist, _ptr(members), _ptr(offsets), C.byref(ng)),
              "rph_find_groups256")
        return self._groups(members, offsets, ng.value)

    def hamming_all_pairs64(self, hashes, threshold, part=0, nparts=1, cap=None):
        hashes = np.ascontiguousarray(hashes, np.uint64)
        n = len(hashes)
        return self._sweep_growing(lambda e, c, f: self.L.rph_hamming_all_pairs64(self.ctx, _ptr(hashes), n, threshold, part, nparts, e, c, f),
                                   max(1 << 16, 4 * n) if cap is None else cap, True, "rph_hamming_all_pairs64")

    def hamming_all_pairs64_dev(self, d_hashes, n, threshold, d_edges, cap, d_count, part=0, nparts=1, stream=None):
        check(self.L.rph_hamming_all_pairs64_dev(self.ctx, d_hashes, n, threshold, part, nparts, d_edges, cap, d_count, stream),
              "rph_hamming_all_pairs64_dev")

    def find_groups64(self, hashes, max_dist):
        hashes = np.ascontiguousarray(hashes, np.uint64)
        n = len(hashes)
        members = np.zeros(max(n, 1), np.uint32)
        offsets = np.zeros(n // 2 + 2, np.uint32)
        ng = C.c_uint32()
        check(self.L.rph_find_groups64(self.ctx, _ptr(hashes), n, max_dist, _ptr(members), _ptr(offsets), C.byref(ng)),
              "rph_find_groups64")
        return self._groups(members, offsets, ng.value)

    def find_groups_from_edges(self, edges, n):
        edges = np.ascontiguousarray(edges, EDGE_DTYPE)
        members = np.zeros(max(n, 1), np.uint32)
        offsets = np.zeros(n // 2 + 2, np.uint32)
        ng = C.c_uint32()
        check(self.L.rph_find_groups_from_edges(_ptr(edges), len(edges), n, _ptr(members), _ptr(offsets), C.byref(ng)),
              "rph_find_groups_from_edges")
        return self._groups(members, offsets, ng.value)

    def union_find_groups(self, edges, n):
        edges = np.ascontiguousarray(edges, EDGE_DTYPE)
        members = np.zeros(max(n, 1), np.uint32)
        offsets = np.zeros(n // 2 + 2, np.uint32)
        ng = C.c_uint32()
        check(self.L.rph_union_find_groups(_ptr(edges), len(edges), n, _ptr(members), _ptr(offsets), C.byref(ng)),
              "rph_union_find_groups")
        return self._groups(members, offsets, ng.value)

    def group_files_pdq(self, hashes, similarity, coeffs=None, has_features=None, quality=None):
        """group_files_generic + PdqStrategy up to the union-find: returns (groups, comparison_count)."""
        hashes = np.ascontiguousarray(hashes, np.uint8).reshape(-1, 32)
        n = len(hashes)
        c = None if coeffs is None else np.ascontiguousarray(coeffs, np.float32).reshape(n, 256)
        hf = None if has_features is None else np.ascontiguousarray(has_features, np.uint8)
        q = None if quality is None else np.ascontiguousarray(quality, np.int32)
        members = np.zeros(max(n, 1), np.uint32)
        offsets = np.zeros(n // 2 + 2, np.uint32)
        ng = C.c_uint32()
        cmp_count = C.c_uint64()
        check(self.L.rph_group_files_pdq(self.ctx, _ptr(hashes), _ptr(c), _ptr(hf), _ptr(q), n, similarity, _ptr(members),
                                         _ptr(offsets), C.byref(ng), C.byref(cmp_count)), "rph_group_files_pdq")
        return self._groups(members, offsets, ng.value), cmp_count.value

    @staticmethod
    def _flatten_groups(groups):
        members = np.array([m for g in groups for m in g], np.uint32)
        offsets = np.zeros(len(groups) + 1, np.uint32)
        if len(groups):
            offsets[1:] = np.cumsum([len(g) for g in groups])
        return members, offsets

    def union_find_groups_append(self, old_groups, edges, n_total):
        """Union-find over n_total files from the groups of an earlier call plus `edges`.  old_groups: a list of member lists, or the
        raw (members, offsets) arrays."""
        om, oo = old_groups if isinstance(old_groups, tuple) else self._flatten_groups(old_groups)
        om, oo = np.ascontiguousarray(om, np.uint32), np.ascontiguousarray(oo, np.uint32)
        edges = np.ascontiguousarray(edges, EDGE_DTYPE)
        members = np.zeros(max(n_total, 1), np.uint32)
        offsets = np.zeros(n_total // 2 + 2, np.uint32)
        ng = C.c_uint32()
        check(self.L.rph_union_find_groups_append(_ptr(om), _ptr(oo), max(len(oo) - 1, 0), _ptr(edges), len(edges), n_total, _ptr(members),
                                                  _ptr(offsets), C.byref(ng)), "rph_union_find_groups_append")
        return self._groups(members, offsets, ng.value)

    def group_files_pdq_append(self, old_hashes, old_groups, new_hashes, similarity, old_coeffs=None, old_has_features=None, old_quality=None,
                               new_coeffs=None, new_has_features=None, new_quality=None):
        """Incremental group_files_pdq: the library (grouped before: old_groups as group_files_pdq returned them) plus new files, numbered
        as the concatenation.  Returns (groups of the concatenation, comparisons the new files added)."""
        oh = np.ascontiguousarray(old_hashes, np.uint8).reshape(-1, 32)
        nh = np.ascontiguousarray(new_hashes, np.uint8).reshape(-1, 32)
        n_old, n_new = len(oh), len(nh)

        def side(coeffs, hf, q, n):
            return (None if coeffs is None else np.ascontiguousarray(coeffs, np.float32).reshape(n, 256),
                    None if hf is None else np.ascontiguousarray(hf, np.uint8), None if q is None else np.ascontiguousarray(q, np.int32))

        oc, ohf, oq = side(old_coeffs, old_has_features, old_quality, n_old)
        nc, nhf, nq = side(new_coeffs, new_has_features, new_quality, n_new)
        om, oo = self._flatten_groups(old_groups)
        n = n_old + n_new
        members = np.zeros(max(n, 1), np.uint32)
        offsets = np.zeros(n // 2 + 2, np.uint32)
        ng = C.c_uint32()
        cmp_count = C.c_uint64()
        check(self.L.rph_group_files_pdq_append(self.ctx, _ptr(oh), _ptr(oc), _ptr(ohf), _ptr(oq), n_old, _ptr(om), _ptr(oo), len(old_groups),
                                                _ptr(nh), _ptr(nc), _ptr(nhf), _ptr(nq), n_new, similarity, _ptr(members), _ptr(offsets),
                                                C.byref(ng), C.byref(cmp_count)), "rph_group_files_pdq_append")
        return self._groups(members, offsets, ng.value), cmp_count.value

    def union_find_labels_dev(self, d_edges, n_edges, d_labels, n, i_base=0, j_base=0, stream=None):
        """Union-find on the device: d_labels (n uint32, a forest with label[x] <= x) becomes the min-label of every file's component."""
        check(self.L.rph_union_find_labels_dev(self.ctx, d_edges, n_edges, i_base, j_base, d_labels, n, stream), "rph_union_find_labels_dev")

    def groups_from_labels_dev(self, d_labels, n, stream=None):
        """Flattened min-labels on the device -> the groups union_find_groups lists."""
        members = np.zeros(max(n, 1), np.uint32)
        offsets = np.zeros(n // 2 + 2, np.uint32)
        ng = C.c_uint32()
        check(self.L.rph_groups_from_labels_dev(self.ctx, d_labels, n, _ptr(members), _ptr(offsets), C.byref(ng), stream),
              "rph_groups_from_labels_dev")
        return self._groups(members, offsets, ng.value)

    def merge_tree_dev(self, d_edges, n_edges, n, top, d_into, d_level, d_edges_at, d_labels=None, i_base=0, j_base=0, stream=None):
        """rph_merge_tree_dev: the merge tree of an edge list on the device (d_into n x uint32, d_level n bytes, d_edges_at (top + 1) x
        uint64; d_labels, optional, the flattened min-labels at top)."""
        check(self.L.rph_merge_tree_dev(self.ctx, d_edges, n_edges, i_base, j_base, n, top, d_into, d_level, d_edges_at, d_labels, stream), "rph_merge_tree_dev")

    @staticmethod
    def _tree_call(call, where, n, top):
        into, level, edges_at = np.zeros(n, np.uint32), np.zeros(n, np.uint8), np.zeros(top + 1, np.uint64)
        check(call(_ptr(into), _ptr(level), _ptr(edges_at)), where)
        return MergeTree(into, level, edges_at)

    @staticmethod
    def merge_tree_from_edges_host(edges, n, top):
        """rph_merge_tree_from_edges_host: the merge tree of a host edge list (no device, no context)."""
        L = _lib.load()
        edges = np.ascontiguousarray(edges, EDGE_DTYPE)
        return Engine._tree_call(lambda i, l, e: L.rph_merge_tree_from_edges_host(_ptr(edges), len(edges), n, top, i, l, e), "rph_merge_tree_from_edges_host", n, top)

    def group_files_pdq_tree(self, hashes, top, coeffs=None, has_features=None, quality=None):
        """The groups of group_files_pdq at every similarity 0 .. top from one sweep at top: a MergeTree."""
        h, c, hf, q = Library._files(hashes, coeffs, has_features, quality)
        return self._tree_call(lambda i, l, e: self.L.rph_group_files_pdq_tree(self.ctx, _ptr(h), _ptr(c), _ptr(hf), _ptr(q), len(h), top, i, l, e),
                               "rph_group_files_pdq_tree", len(h), top)

    @staticmethod
    def merge_tree_host(hashes, top, coeffs=None, has_features=None, quality=None):
        """group_files_pdq_tree on the host (rph_merge_tree_host): brute force, no device, no context."""
        L = _lib.load()
        h, c, hf, q = Library._files(hashes, coeffs, has_features, quality)
        return Engine._tree_call(lambda i, l, e: L.rph_merge_tree_host(_ptr(h), _ptr(c), _ptr(hf), _ptr(q), len(h), top, i, l, e), "rph_merge_tree_host", len(h), top)

    @staticmethod
    def merge_tree_truncate(tree, t):
        """rph_merge_tree_truncate: the MergeTree for t <= tree.top from `tree` (host, no device, no context); `tree` is not changed."""
        L = _lib.load()
        if t < 0:
            raise ValueError(f"similarity {t} below 0")
        return Engine._tree_call(lambda i, l, e: L.rph_merge_tree_truncate(_ptr(tree.into), _ptr(tree.level), _ptr(tree.edges_at), len(tree), tree.top, t, i, l, e),
                                 "rph_merge_tree_truncate", len(tree), min(t, tree.top))

    @staticmethod
    def _group_lists(groups, pivots):
        """(members, offsets, n_groups, pivots or None) as the rph_group_max_dist forms take them.  groups: a list of index lists, or the
        raw (members, offsets) arrays; pivots: one file number or None (RPH_NO_PIVOT) per group, or None for the default pivots."""
        members, offsets = groups if isinstance(groups, tuple) else Engine._flatten_groups(groups)
        members, offsets = np.ascontiguousarray(members, np.uint32), np.ascontiguousarray(offsets, np.uint32)
        ng = max(len(offsets) - 1, 0)
        if pivots is not None:
            pivots = np.array([_lib.RPH_NO_PIVOT if p is None else int(p) for p in pivots], np.uint32)
            if len(pivots) != ng:
                raise ValueError(f"{len(pivots)} pivots for {ng} groups")
        return members, offsets, ng, pivots

    @staticmethod
    def _group_dist_result(max_dist, member_dist, offsets, ng):
        if member_dist is None:
            return max_dist.tolist()
        return max_dist.tolist(), [member_dist[offsets[g]:offsets[g + 1]].tolist() for g in range(ng)]

    @staticmethod
    def _group_max_dist_call(call, where, groups, pivots, want_member_dist):
        members, offsets, ng, piv = Engine._group_lists(groups, pivots)
        max_dist = np.zeros(ng, np.uint32)
        member_dist = np.zeros(len(members), np.uint32) if want_member_dist else None
        check(call(_ptr(members), _ptr(offsets), ng, _ptr(piv), _ptr(max_dist), _ptr(member_dist)), where)
        return Engine._group_dist_result(max_dist, member_dist, offsets, ng)

    def group_max_dist(self, groups, hashes, pivots=None, coeffs=None, has_features=None, want_member_dist=False):
        """max_dist of every group (process_raw_groups, scanner.rs:2214-2241) on the device: the maximum over a group's members of the
        minimum distance to its pivot's 8 dihedral hashes, or to its plain hash when the pivot has no features.  groups: index lists as
        group_files_pdq returns them, in the caller's order; pivots: a file number or None per group, or None for the reference's
        default (the first listed member with features, else the first).  Returns the list of max_dist, with want_member_dist
        (max_dist, per-group lists of the members' distances)."""
        h, c, hf, _ = Library._files(hashes, coeffs, has_features, None)
        return self._group_max_dist_call(lambda m, o, ng, p, out, md: self.L.rph_group_max_dist(self.ctx, _ptr(h), _ptr(c), _ptr(hf), len(h), m, o, ng, p, out, md),
                                         "rph_group_max_dist", groups, pivots, want_member_dist)

    @staticmethod
    def group_max_dist_host(groups, hashes, pivots=None, coeffs=None, has_features=None, want_member_dist=False):
        """group_max_dist on the host (rph_group_max_dist_host): no device, no context."""
        L = _lib.load()
        h, c, hf, _ = Library._files(hashes, coeffs, has_features, None)
        return Engine._group_max_dist_call(lambda m, o, ng, p, out, md: L.rph_group_max_dist_host(_ptr(h), _ptr(c), _ptr(hf), len(h), m, o, ng, p, out, md),
                                           "rph_group_max_dist_host", groups, pivots, want_member_dist)

    def group_max_dist_dev(self, d_hashes, n, d_members, d_offsets, n_groups, d_max_dist, d_rows=None, row_mode=_lib.RPH_ROWS_NONE, d_has_features=None,
                           d_pivots=None, d_member_dist=None, stream=None):
        """rph_group_max_dist_dev: everything on the device; row_mode says what d_rows holds (RPH_ROWS_*); d_pivots None: default pivots."""
        check(self.L.rph_group_max_dist_dev(self.ctx, d_hashes, n, d_rows, row_mode, d_has_features, d_members, d_offsets, n_groups, d_pivots, d_max_dist,
                                            d_member_dist, stream), "rph_group_max_dist_dev")

    @staticmethod
    def _nearest_inputs(rows, hashes_q, has_features, skip):
        """The arrays of a nearest call as the C forms take them.  rows: [n_lib, 32] or [n_lib, n_variants, 32] uint8."""
        rows = np.ascontiguousarray(rows, np.uint8)
        if rows.ndim == 2:
            rows = rows.reshape(len(rows), 1, 32)
        if rows.ndim != 3 or rows.shape[2] != 32:
            raise ValueError(f"rows of shape {rows.shape}: [n_lib, n_variants, 32] expected")
        hq = np.ascontiguousarray(hashes_q, np.uint8).reshape(-1, 32)
        hf = None if has_features is None else np.ascontiguousarray(has_features, np.uint8)
        if hf is not None and len(hf) != len(rows):
            raise ValueError(f"{len(hf)} has_features flags for {len(rows)} files")
        sk = None if skip is None else np.array([_lib.RPH_NO_FILE if x is None else int(x) for x in skip], np.uint32)
        if sk is not None and len(sk) != len(hq):
            raise ValueError(f"{len(sk)} skip entries for {len(hq)} queries")
        return rows, hq, hf, sk

    @staticmethod
    def _nearest_call(call, where, n_q, k):
        k = int(k)
        slots = max(k, 0) if 0 < k <= _lib.RPH_NEAREST_MAX_K else 0  # a refused k writes nothing
        edges, counts = np.zeros((n_q, slots), EDGE_DTYPE), np.zeros(n_q, np.uint32)
        check(call(k, _ptr(edges), _ptr(counts)), where)
        return edges, counts

    def hamming_nearest(self, rows, hashes_q, k, max_dist=256, has_features=None, skip=None):
        """The k nearest library files of every query (rph_hamming_nearest): rows [n_lib, 32] or [n_lib, 8, 32]; a file whose
        has_features byte is 0 owns row 0 only; skip[q] is a file query q never reports (None: none).  Returns (edges[n_q, k], counts[n_q]):
        slot (q, r) = (file, q, distance, variant << 9), ordered by (distance, file); slots behind counts[q] hold file RPH_NO_FILE and
        distance 0xFFFF.  max_dist >= 256: no cutoff."""
        r, hq, hf, sk = self._nearest_inputs(rows, hashes_q, has_features, skip)
        return self._nearest_call(lambda kk, out, cnt: self.L.rph_hamming_nearest(self.ctx, _ptr(r), r.shape[1], _ptr(hf), len(r), _ptr(hq), _ptr(sk), len(hq), kk,
                                                                                  max_dist, out, cnt), "rph_hamming_nearest", len(hq), k)

    @staticmethod
    def hamming_nearest_host(rows, hashes_q, k, max_dist=256, has_features=None, skip=None):
        """hamming_nearest on the host (rph_hamming_nearest_host): no device, no context."""
        L = _lib.load()
        r, hq, hf, sk = Engine._nearest_inputs(rows, hashes_q, has_features, skip)
        return Engine._nearest_call(lambda kk, out, cnt: L.rph_hamming_nearest_host(_ptr(r), r.shape[1], _ptr(hf), len(r), _ptr(hq), _ptr(sk), len(hq), kk, max_dist,
                                                                                    out, cnt), "rph_hamming_nearest_host", len(hq), k)

    def hamming_nearest_dev(self, d_rows, n_variants, n_lib, d_hashes_q, n_q, k, d_out, max_dist=256, d_has_features=None, d_skip=None, d_counts=None, stream=None):
        """rph_hamming_nearest_dev: everything on the device, asynchronous on `stream`; d_out: n_q x k edges, d_counts: n_q x uint32 or None."""
        check(self.L.rph_hamming_nearest_dev(self.ctx, d_rows, n_variants, d_has_features, n_lib, d_hashes_q, d_skip, n_q, k, max_dist, d_out, d_counts, stream),
              "rph_hamming_nearest_dev")

    @staticmethod
    def nearest_layout(n_lib, n_variants, n_q, k):
        """How a nearest call is cut (tests): files per MFMA block, files per segment, queries per tile, number of segments."""
        out = (C.c_uint32 * 5)()
        _lib.load().rph_debug_nearest_layout(n_lib, n_variants, n_q, k, out)
        return tuple(out)[:4]

    @staticmethod
    def nearest_chunk_queries(n_lib, n_variants, n_q, k):
        """How many queries a nearest call takes at a time (tests): the fifth word of rph_debug_nearest_layout."""
        out = (C.c_uint32 * 5)()
        _lib.load().rph_debug_nearest_layout(n_lib, n_variants, n_q, k, out)
        return out[4]

    @staticmethod
    def nearest_set_segment(files):
        """Forces the segment length of the nearest calls that follow (tests); 0 restores the default."""
        _lib.load().rph_debug_nearest_set_segment(files)

    @staticmethod
    def nearest_set_workspace(nbytes):
        """Bounds the partial lists of the nearest calls that follow, in bytes (tests); 0 restores 256 MiB, less than 8192 is 8192."""
        _lib.load().rph_debug_nearest_set_workspace(nbytes)

    def library(self, similarity, top=None, max_edges=0):
        """A grouped library that stays on this engine's device (rph_library): see Library.  With `top` it keeps its edges."""
        return Library(self, similarity, top, max_edges)

    def mih_build256(self, hashes):
        hashes = np.ascontiguousarray(hashes, np.uint8).reshape(-1, 32)
        n = len(hashes)
        offsets = np.zeros(16 * 65536 + 1, np.uint32)
        values = np.zeros(max(16 * n, 1), np.uint32)
        check(self.L.rph_mih_build256(self.ctx, _ptr(hashes), n, _ptr(offsets), _ptr(values)), "rph_mih_build256")
        return offsets, values[: 16 * n]

    def mih_build64(self, hashes):
        hashes = np.ascontiguousarray(hashes, np.uint64)
        n = len(hashes)
        offsets = np.zeros(8 * 256 + 1, np.uint32)
        values = np.zeros(max(8 * n, 1), np.uint32)
        check(self.L.rph_mih_build64(self.ctx, _ptr(hashes), n, _ptr(offsets), _ptr(values)), "rph_mih_build64")
        return offsets, values[: 8 * n]

    # ---- synthetic workloads ----
    def synth_images_dev(self, d_out, first_k, n, w=512, h=512, seed=0x5EED2026, stream=None):
        check(self.L.rph_synth_images_dev(self.ctx, d_out, first_k, n, w, h, seed, stream), "rph_synth_images_dev")

    def synth_hashes_dev(self, d_out, first, count, n_total, seed=0xC0FFEE, n_clusters=0, stream=None):
        check(self.L.rph_synth_hashes_dev(self.ctx, d_out, first, count, n_total, seed, n_clusters, stream), "rph_synth_hashes_dev")

    def synth_images(self, first_k, n, w=512, h=512, seed=0x5EED2026):
        d = self.dev_alloc(n * w * h * 3)
        try:
            self.synth_images_dev(d, first_k, n, w, h, seed)
            out = np.zeros((n, h, w, 3), np.uint8)
            self.dev_download(out, d)
        finally:
            self.dev_free(d)
        return out

    def synth_hashes(self, first, count, n_total, seed=0xC0FFEE, n_clusters=0):
        d = self.dev_alloc(count * 32)
        try:
            self.synth_hashes_dev(d, first, count, n_total, seed, n_clusters)
            out = np.zeros((count, 32), np.uint8)
            self.dev_download(out, d)
        finally:
            self.dev_free(d)
        return out

    # ---- device memory / events ----
    def read_stream_dev(self, d_buf, nbytes, stream=None):
        """one pure read pass over a device buffer (bench.py times it: the read bandwidth a streaming kernel can get)"""
        check(self.L.rph_read_stream_dev(self.ctx, d_buf, nbytes, stream), "rph_read_stream_dev")

    def stream_create(self):
        s = C.c_void_p()
        check(self.L.rph_stream_create(self.ctx, C.byref(s)), "rph_stream_create")
        return s

    def stream_synchronize(self, stream=None):
        check(self.L.rph_stream_synchronize(self.ctx, stream), "rph_stream_synchronize")

    def stream_destroy(self, stream):
        check(self.L.rph_stream_destroy(self.ctx, stream), "rph_stream_destroy")

    def dev_alloc(self, nbytes):
        p = C.c_void_p()
        check(self.L.rph_dev_alloc(self.ctx, nbytes, C.byref(p)), "rph_dev_alloc")
        return p.value

    def dev_free(self, p):
        check(self.L.rph_dev_free(self.ctx, p), "rph_dev_free")

    def dev_upload(self, d_dst, arr):
        arr = np.ascontiguousarray(arr)
        check(self.L.rph_dev_upload(self.ctx, d_dst, _ptr(arr), arr.nbytes), "rph_dev_upload")

    def dev_download(self, arr, d_src, nbytes=None):
        assert arr.flags["C_CONTIGUOUS"]
        check(self.L.rph_dev_download(self.ctx, _ptr(arr), d_src, arr.nbytes if nbytes is None else nbytes), "rph_dev_download")

    def dev_memset(self, d_dst, value, nbytes, stream=None):
        check(self.L.rph_dev_memset(self.ctx, d_dst, value, nbytes, stream), "rph_dev_memset")

    def event(self):
        e = C.c_void_p()
        check(self.L.rph_event_create(self.ctx, C.byref(e)), "rph_event_create")
        return e.value

    def event_record(self, e, stream=None):
        check(self.L.rph_event_record(self.ctx, e, stream), "rph_event_record")

    def event_elapsed_ms(self, start, stop):
        ms = C.c_float()
        check(self.L.rph_event_elapsed_ms(self.ctx, start, stop, C.byref(ms)), "rph_event_elapsed_ms")
        return ms.value

    def event_destroy(self, e):
        check(self.L.rph_event_destroy(self.ctx, e), "rph_event_destroy")


class MergeTree:
    """The groups at every similarity 0 .. top (include/rupphash.h, "Merge tree"): into (n x uint32), level (n x uint8) and edges_at
    (top + 1 x uint64) as the C calls return them.  Cutting is host work, O(n) per call; none of it needs an engine."""

    def __init__(self, into, level, edges_at):
        self.into = np.ascontiguousarray(into, np.uint32)
        self.level = np.ascontiguousarray(level, np.uint8)
        self.edges_at = np.ascontiguousarray(edges_at, np.uint64)
        self.top = len(self.edges_at) - 1

    def __len__(self):
        return len(self.into)

    def labels(self, s):
        """label_s: per file the smallest file number of its component at similarity s."""
        out = np.zeros(len(self), np.uint32)
        check(_lib.load().rph_merge_tree_labels(_ptr(self.into), _ptr(self.level), len(self), s, _ptr(out)), "rph_merge_tree_labels")
        return out

    def groups(self, s):
        """What group_files_pdq(similarity=s) lists: components with > 1 member, members ascending, groups by first member."""
        n = len(self)
        members = np.zeros(max(n, 1), np.uint32)
        offsets = np.zeros(n // 2 + 2, np.uint32)
        ng = C.c_uint32()
        check(_lib.load().rph_merge_tree_groups(_ptr(self.into), _ptr(self.level), n, s, _ptr(members), _ptr(offsets), C.byref(ng)), "rph_merge_tree_groups")
        return Engine._groups(members, offsets, ng.value)

    def comparisons(self, s):
        """group_files_pdq's comparison count at similarity s <= top."""
        if not 0 <= s <= self.top:
            raise ValueError(f"similarity {s} outside 0 .. {self.top}")
        return int(self.edges_at[:s + 1].sum())

    def profile(self):
        """(n_groups, grouped_files): for every s in 0 .. top the number of groups and the number of files in them."""
        n_groups, files = np.zeros(self.top + 1, np.uint64), np.zeros(self.top + 1, np.uint64)
        check(_lib.load().rph_merge_tree_profile(_ptr(self.into), _ptr(self.level), len(self), self.top, _ptr(n_groups), _ptr(files)), "rph_merge_tree_profile")
        return n_groups, files


class Library:
    """rph_library: files appended so far stay on the device with their variants, flags and component labels.  groups() equals
    Engine.group_files_pdq on the files it holds, in order.  One similarity, at most 2^31 - 1 files; remove() renumbers the files that
    stay.  Close it before its engine.

    With `top` (similarity <= top <= 63) the library keeps its edges (rph_library_create_tree): every edge of the sweep at `top` among the
    resident files stays on the device, at most max_edges of them (0: 2^28), so merge_tree(t) and groups_at(t) for t <= top run no sweep.
    Everything else behaves as without `top`; appends sweep at `top` and cost accordingly.  edges() and restore_edges() persist it."""

    def __init__(self, engine, similarity, top=None, max_edges=0):
        if top is not None and not isinstance(top, (int, np.integer)):  # (an engine passed where open_library(similarity, engine) used to take it)
            raise TypeError(f"top is a similarity (an int) or None, not {type(top).__name__}: pass the engine as engine=")
        if top is not None and not similarity <= top <= 63:
            raise ValueError(f"top {top} outside similarity .. 63 (similarity {similarity})")
        if max_edges < 0:
            raise ValueError("max_edges below 0")
        self.engine, self.L, self.similarity, self.top = engine, engine.L, similarity, top
        h = C.c_void_p()
        if top is None:
            check(self.L.rph_library_create(engine.ctx, similarity, C.byref(h)), "rph_library_create")
        else:
            check(self.L.rph_library_create_tree(engine.ctx, similarity, top, max_edges, C.byref(h)), "rph_library_create_tree")
        self.handle = h

    def close(self):
        if getattr(self, "handle", None):
            if getattr(self.engine, "ctx", None):  # the handle of a library that outlived its engine points into a context that is gone
                self.L.rph_library_destroy(self.handle)
            self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _size(self):
        n, c = C.c_uint64(), C.c_uint64()
        check(self.L.rph_library_size(self.handle, C.byref(n), C.byref(c)), "rph_library_size")
        return n.value, c.value

    def __len__(self):
        return self._size()[0]

    @property
    def comparisons(self):
        return self._size()[1]

    def reserve(self, n):
        check(self.L.rph_library_reserve(self.handle, n), "rph_library_reserve")

    @staticmethod
    def _files(hashes, coeffs, has_features, quality):
        hashes = np.ascontiguousarray(hashes, np.uint8).reshape(-1, 32)
        n = len(hashes)
        return (hashes, None if coeffs is None else np.ascontiguousarray(coeffs, np.float32).reshape(n, 256),
                None if has_features is None else np.ascontiguousarray(has_features, np.uint8),
                None if quality is None else np.ascontiguousarray(quality, np.int32))

    def append(self, hashes, coeffs=None, has_features=None, quality=None):
        """The files become len(self) .. len(self) + n - 1.  Returns (labels, new_comparisons): per new file the smallest index of the
        component it is in now, and the comparisons these files added."""
        h, c, hf, q = self._files(hashes, coeffs, has_features, quality)
        labels = np.zeros(len(h), np.uint32)
        cmp_count = C.c_uint64()
        check(self.L.rph_library_append(self.handle, _ptr(h), _ptr(c), _ptr(hf), _ptr(q), len(h), _ptr(labels), C.byref(cmp_count)),
              "rph_library_append")
        return labels, cmp_count.value

    def remove(self, indices):
        """Remove the files with these (current, distinct) numbers.  The others keep their order and are renumbered densely.  Returns
        (new_index, dropped): the new number of every old file (0xFFFFFFFF for a removed one) and the comparisons that went with the
        removed files.  Afterwards the library equals Engine.group_files_pdq on the remaining files; a refused call changes nothing."""
        idx = np.ascontiguousarray(indices, np.uint32).reshape(-1)
        new_index = np.zeros(len(self), np.uint32)
        dropped = C.c_uint64()
        check(self.L.rph_library_remove(self.handle, _ptr(idx), len(idx), _ptr(new_index), C.byref(dropped)), "rph_library_remove")
        return new_index, dropped.value

    def restore(self, hashes, groups, comparisons=0, coeffs=None, has_features=None, quality=None):
        """Start an empty library from files an earlier run grouped at the same similarity (`groups` as it returned them): no sweep."""
        h, c, hf, q = self._files(hashes, coeffs, has_features, quality)
        om, oo = groups if isinstance(groups, tuple) else Engine._flatten_groups(groups)
        om, oo = np.ascontiguousarray(om, np.uint32), np.ascontiguousarray(oo, np.uint32)
        check(self.L.rph_library_restore(self.handle, _ptr(h), _ptr(c), _ptr(hf), _ptr(q), len(h), _ptr(om), _ptr(oo), max(len(oo) - 1, 0),
                                         comparisons), "rph_library_restore")

    def groups(self):
        n = len(self)
        members = np.zeros(max(n, 1), np.uint32)
        offsets = np.zeros(n // 2 + 2, np.uint32)
        ng = C.c_uint32()
        check(self.L.rph_library_groups(self.handle, _ptr(members), _ptr(offsets), C.byref(ng)), "rph_library_groups")
        return Engine._groups(members, offsets, ng.value)

    def labels(self, first=0, count=None):
        count = len(self) - first if count is None else count
        out = np.zeros(max(count, 0), np.uint32)
        check(self.L.rph_library_labels(self.handle, first, count, _ptr(out)), "rph_library_labels")
        return out

    def group_max_dist(self, groups, pivots=None, want_member_dist=False):
        """Engine.group_max_dist against the resident files, in the library's current numbering: no hash or coefficient leaves the device.
        The library is not changed."""
        return self.engine._group_max_dist_call(lambda m, o, ng, p, out, md: self.L.rph_library_group_max_dist(self.handle, m, o, ng, p, out, md),
                                                "rph_library_group_max_dist", groups, pivots, want_member_dist)

    def merge_tree(self, top):
        """The MergeTree of the resident files at `top`, whatever the library's own similarity is; nothing resident changes.  One sweep
        -- none on a library that keeps its edges when `top` is at or below the library's."""
        return Engine._tree_call(lambda i, l, e: self.L.rph_library_merge_tree(self.handle, top, i, l, e), "rph_library_merge_tree", len(self), top)

    def groups_at(self, s):
        """What Engine.group_files_pdq(similarity=s) lists for the resident files: merge_tree(s) cut at s."""
        return self.merge_tree(s).groups(s)

    def edge_info(self):
        """(top, n_edges, max_edges) of the edge store; top is None for a library that keeps no edges."""
        top, n, cap = C.c_uint32(), C.c_uint64(), C.c_uint64()
        check(self.L.rph_library_edge_info(self.handle, C.byref(top), C.byref(n), C.byref(cap)), "rph_library_edge_info")
        return None if top.value == _lib.RPH_NO_EDGE_STORE else top.value, n.value, cap.value

    def edges(self):
        """The store as a structured array (EDGE_DTYPE: i < j in the current numbering, d, flags), in no particular order."""
        found = C.c_uint64()
        rc = self.L.rph_library_edges(self.handle, None, 0, C.byref(found))
        if rc != _lib.RPH_ERR_CAPACITY:
            check(rc, "rph_library_edges")
        out = np.zeros(found.value, EDGE_DTYPE)
        check(self.L.rph_library_edges(self.handle, _ptr(out), len(out), C.byref(found)), "rph_library_edges")
        return out

    def restore_edges(self, hashes, edges, coeffs=None, has_features=None, quality=None):
        """Start an empty edge-keeping library from files and the edges() of an earlier run with the same top: no sweep."""
        h, c, hf, q = self._files(hashes, coeffs, has_features, quality)
        e = np.ascontiguousarray(edges, EDGE_DTYPE).reshape(-1)
        check(self.L.rph_library_restore_edges(self.handle, _ptr(h), _ptr(c), _ptr(hf), _ptr(q), len(h), _ptr(e), len(e)), "rph_library_restore_edges")

    def query(self, hashes, quality=None, cap=None):
        """Edges (library file i, query j, d, variant in flags) of the queries against the resident files; the library is not changed.
        With cap given, RPH_ERR_CAPACITY raises (RphError)."""
        h, _, _, q = self._files(hashes, None, None, quality)
        return Engine._sweep_growing(lambda e, c, f: self.L.rph_library_query(self.handle, _ptr(h), _ptr(q), len(h), e, c, f),
                                     max(1 << 16, 8 * len(h)) if cap is None else cap, cap is None, "rph_library_query")


    def nearest(self, hashes, k, max_dist=256):
        """Engine.hamming_nearest of the queries against the resident files (their 8 rows and flags, where they lie): (edges[n_q, k],
        counts[n_q]), files in the library's current numbering.  The library is not changed."""
        hq = np.ascontiguousarray(hashes, np.uint8).reshape(-1, 32)
        return Engine._nearest_call(lambda kk, out, cnt: self.L.rph_library_nearest(self.handle, _ptr(hq), len(hq), kk, max_dist, out, cnt), "rph_library_nearest",
                                    len(hq), k)

    def nearest_files(self, indices, k, max_dist=256):
        """The neighbours of resident files (current numbering): nearest() of their hashes, gathered on the device, each skipping itself."""
        idx = np.ascontiguousarray(indices, np.uint32).reshape(-1)
        return Engine._nearest_call(lambda kk, out, cnt: self.L.rph_library_nearest_files(self.handle, _ptr(idx), len(idx), kk, max_dist, out, cnt),
                                    "rph_library_nearest_files", len(idx), k)


group_max_dist_host = Engine.group_max_dist_host  # needs no engine
hamming_nearest_host = Engine.hamming_nearest_host
merge_tree_host = Engine.merge_tree_host
merge_tree_from_edges_host = Engine.merge_tree_from_edges_host
merge_tree_truncate = Engine.merge_tree_truncate


_default = None


def default_engine():
    """Process-wide engine on HIP device LOCAL_RANK (or 0)."""
    global _default
    if _default is None:
        import os

        _default = Engine(int(os.environ.get("LOCAL_RANK", "0")))
    return _default


class MultiEngine:
    """Several GPUs under this one process: an rph_multi (one rph_ctx per device + an RCCL communicator inside the library).
    The sharded forms of the path (BASELINE configs 4 and 5) for a single-process host like the reference's scanner."""

    def __init__(self, devices=None, n_devices=None):
        self.L = _lib.load()
        if devices is None:
            devices = list(range(n_devices or 1))
        arr = (C.c_int * len(devices))(*devices)
        h = C.c_void_p()
        check(self.L.rph_multi_init(arr, len(devices), C.byref(h)), "rph_multi_init")
        self.m = h
        self.devices = list(devices)

    def close(self):
        if getattr(self, "m", None):
            self.L.rph_multi_shutdown(self.m)
            self.m = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def size(self):
        return self.L.rph_multi_size(self.m)

    def engine(self, index):
        """Engine view of device `index`'s context (owned by the multi: do not close it)"""
        e = Engine.__new__(Engine)
        e.L = self.L
        e.ctx = None
        ctx = self.L.rph_multi_ctx(self.m, index)
        assert ctx
        e.__dict__["ctx"] = C.c_void_p(ctx)
        e.device = self.devices[index]
        e.close = lambda: None
        return e

    def hamming_all_pairs(self, hashes, threshold, cap=None):
        hashes = np.ascontiguousarray(hashes, np.uint8).reshape(-1, 32)
        n = len(hashes)
        return Engine._sweep_growing(lambda e, c, f: self.L.rph_multi_hamming_all_pairs(self.m, _ptr(hashes), n, threshold, e, c, f),
                                     max(1 << 16, 4 * n) if cap is None else cap, True, "rph_multi_hamming_all_pairs")

    def hash_and_group(self, images, similarity, want_coeffs=False):
        """images: uint8 (n,h,w,3|4) or (n,h,w).  Returns dict(hash, quality, coeffs, valid, groups, comparison_count)."""
        images = np.ascontiguousarray(images, np.uint8)
        if images.ndim == 3:
            n, h, w = images.shape
            ch = 1
        else:
            n, h, w, ch = images.shape
        out = {"hash": np.zeros((n, 32), np.uint8), "quality": np.zeros(n, np.float32),
               "coeffs": np.zeros((n, 256), np.float32) if want_coeffs else None, "valid": np.zeros(n, np.uint8)}
        members = np.zeros(max(n, 1), np.uint32)
        offsets = np.zeros(n // 2 + 2, np.uint32)
        ng = C.c_uint32()
        cmp_count = C.c_uint64()
        check(self.L.rph_multi_hash_and_group(self.m, _ptr(images), n, w, h, ch, w * ch, w * h * ch, similarity, _ptr(out["hash"]), _ptr(out["quality"]),
                                              _ptr(out["coeffs"]), _ptr(out["valid"]), _ptr(members), _ptr(offsets), C.byref(ng), C.byref(cmp_count)),
              "rph_multi_hash_and_group")
        out["groups"] = Engine._groups(members, offsets, ng.value)
        out["comparison_count"] = cmp_count.value
        return out

    def jpeg_hash_and_group(self, files, similarity, flavour=0, threads=0):
        """files: list of JPEG byte strings.  Returns dict(hash, quality, coeffs, valid, status, groups, comparison_count); groups hold
        indices into `files` (only files that produced a hash are grouped)."""
        arr, lens, n = files if isinstance(files, tuple) else Engine.jpeg_file_list(files)
        out = {"hash": np.zeros((n, 32), np.uint8), "quality": np.zeros(n, np.float32), "coeffs": np.zeros((n, 256), np.float32),
               "valid": np.zeros(n, np.uint8), "status": np.zeros(n, np.int32)}
        members = np.zeros(max(n, 1), np.uint32)
        offsets = np.zeros(n // 2 + 2, np.uint32)
        ng = C.c_uint32()
        cmp_count = C.c_uint64()
        check(self.L.rph_multi_jpeg_hash_and_group(self.m, arr, lens, n, int(flavour), int(threads), similarity, _ptr(out["hash"]), _ptr(out["quality"]),
                                                   _ptr(out["coeffs"]), _ptr(out["valid"]), _ptr(out["status"]), _ptr(members), _ptr(offsets), C.byref(ng),
                                                   C.byref(cmp_count)), "rph_multi_jpeg_hash_and_group")
        out["groups"] = Engine._groups(members, offsets, ng.value)
        out["comparison_count"] = cmp_count.value
        return out

    def files_hash_and_group(self, files, similarity, names=None, flavour=0, threads=0, want_pixel_hash=False):
        """files: list of byte strings of any mix of the six formats (Engine.files_pdq_hash_batch), names: their names or None.  Returns
        dict(hash, quality, coeffs, valid, status, format[, pixel_hash], groups, comparison_count); groups hold indices into `files`."""
        arr, lens, nm, n = files if isinstance(files, tuple) else Engine.files_list(files, names)
        out = {"hash": np.zeros((n, 32), np.uint8), "quality": np.zeros(n, np.float32), "coeffs": np.zeros((n, 256), np.float32),
               "valid": np.zeros(n, np.uint8), "status": np.zeros(n, np.int32), "format": np.zeros(n, np.uint8)}
        if want_pixel_hash:
            out["pixel_hash"] = np.zeros((n, 32), np.uint8)
        members = np.zeros(max(n, 1), np.uint32)
        offsets = np.zeros(n // 2 + 2, np.uint32)
        ng = C.c_uint32()
        cmp_count = C.c_uint64()
        check(self.L.rph_multi_files_hash_and_group(self.m, arr, lens, nm, n, int(flavour), int(threads), similarity, _ptr(out["hash"]), _ptr(out["quality"]),
                                                    _ptr(out["coeffs"]), _ptr(out["valid"]), _ptr(out["status"]), _ptr(out.get("pixel_hash")),
                                                    _ptr(out["format"]), _ptr(members), _ptr(offsets), C.byref(ng), C.byref(cmp_count)),
              "rph_multi_files_hash_and_group")
        out["groups"] = Engine._groups(members, offsets, ng.value)
        out["comparison_count"] = cmp_count.value
        return out

    def group_files_pdq(self, hashes, similarity, coeffs=None, has_features=None, quality=None):
        hashes = np.ascontiguousarray(hashes, np.uint8).reshape(-1, 32)
        n = len(hashes)
        c = None if coeffs is None else np.ascontiguousarray(coeffs, np.float32).reshape(n, 256)
        hf = None if has_features is None else np.ascontiguousarray(has_features, np.uint8)
        q = None if quality is None else np.ascontiguousarray(quality, np.int32)
        members = np.zeros(max(n, 1), np.uint32)
        offsets = np.zeros(n // 2 + 2, np.uint32)
        ng = C.c_uint32()
        cmp_count = C.c_uint64()
        check(self.L.rph_multi_group_files_pdq(self.m, _ptr(hashes), _ptr(c), _ptr(hf), _ptr(q), n, similarity, _ptr(members), _ptr(offsets),
                                               C.byref(ng), C.byref(cmp_count)), "rph_multi_group_files_pdq")
        return Engine._groups(members, offsets, ng.value), cmp_count.value
