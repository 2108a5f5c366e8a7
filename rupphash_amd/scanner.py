"""Grouping half of /root/reference/src/scanner.rs (lines 1588-1832) on top of the C ABI.

    PDQ_MIN_QUALITY, is_low_pdq_quality            scanner.rs:1588-1594
    group_with_pdqhash / group_files_generic       scanner.rs:1640-1832 up to the union-find
    group_max_dist                                 scanner.rs:2214-2241 (the per-group max_dist of process_raw_groups)
    load_image_fast ("jpg" | "jpeg" arm)           scanner.rs:461-508
    load_png (the "png" arm, image + png crates)    scanner.rs:461-736 (load_image_fast's generic path for .png)
    load_tiff (the TiffDecoder arm)                scanner.rs:628-708
    load_gif (the image-crate arm for .gif)        scanner.rs:713-734
    load_bmp (the image-crate arm for .bmp)        scanner.rs:713-734
    pixel_hash (--pixel-hash)                      scanner.rs:1393-1404
    hash_images (both hashes of decoded images)    scanner.rs:1386-1410
    load_image_any (the routing over six formats)  scanner.rs:461-735
    hash_files (the per-file closure, mixed files) scanner.rs:1350-1417
    identical_duplicates                           scanner.rs:1843-1864 (analyze_group steps 1-3)
File-name logic after the union-find (merge_groups_by_stem, the sorting inside process_raw_groups) stays with the caller.
"""
import numpy as np

from . import _lib
from .engine import Library, default_engine

PDQ_MIN_QUALITY = 50


def load_image_fast(path, data, engine=None, flavour=_lib.RPH_JPEG_ZUNE):
    """The "jpg" | "jpeg" arm of load_image_fast (scanner.rs:461-508): decoded on the device, returned as (h, w) uint8 [Luma8] or
    (h, w, 3) [Rgb8] -- the DynamicImage the reference builds from zune-jpeg's buffer.  A stream the device path does not take
    (CMYK, arithmetic coding, corrupt) raises RphError: the caller goes on to its next decoder, as the reference goes from tier 1 to
    tier 2 (scanner.rs:510-551).  Every other extension is the host's business (ValueError)."""
    import os

    ext = os.path.splitext(str(path))[1].lstrip(".").lower()
    if ext not in ("jpg", "jpeg"):
        raise ValueError(f"load_image_fast: '{ext}' files are decoded by the host's decoders, not by this library")
    return (engine or default_engine()).jpeg_decode(data, flavour)


def load_png(path, data, engine=None):
    """The png arm of load_image_fast: decoded on the device and returned as the DynamicImage the image crate builds with
    Transformations::EXPAND -- (h, w) Luma8 / L16, (h, w, 2) LumaA, (h, w, 3) Rgb, (h, w, 4) Rgba; uint8, or uint16 for 16-bit files.
    A file the damaged-file rule refuses raises RphError (include/rupphash.h, PNG section); other extensions raise ValueError.
    load_image_fast itself stays JPEG-only: a scan loop routes .png files here."""
    import os

    ext = os.path.splitext(str(path))[1].lstrip(".").lower()
    if ext != "png":
        raise ValueError(f"load_png: '{ext}' is not a PNG file name")
    return (engine or default_engine()).png_decode(data)


def load_tiff(path, data, engine=None):
    """The tiff arm of load_image_fast (scanner.rs:628-708): decoded on the device and returned in the native layout of the header's TIFF
    section -- (h, w) Luma8 / L16, (h, w, 2) LumaA, (h, w, 3) Rgb, (h, w, 4) Rgba; uint8, or uint16 for 16-bit files.  A file the rule
    refuses raises RphError; status RPH_ERR_UNSUPPORTED (JPEG-in-TIFF, CCITT, palette, ...) means the caller's own decoders take the
    file.  Extensions other than tif / tiff raise ValueError."""
    import os

    ext = os.path.splitext(str(path))[1].lstrip(".").lower()
    if ext not in ("tif", "tiff"):
        raise ValueError(f"load_tiff: '{ext}' is not a TIFF file name")
    return (engine or default_engine()).tiff_decode(data)


def load_gif(path, data, engine=None):
    """The image-crate arm of load_image_fast for a .gif (scanner.rs:713-734): the first frame on its logical screen, decoded on the
    device and returned as (h, w, 4) uint8 Rgba8, the native layout of the header's GIF section.  A file the rule refuses raises
    RphError; extensions other than gif raise ValueError.  load_image_fast itself stays JPEG-only."""
    import os

    ext = os.path.splitext(str(path))[1].lstrip(".").lower()
    if ext != "gif":
        raise ValueError(f"load_gif: '{ext}' is not a GIF file name")
    return (engine or default_engine()).gif_decode(data)


def load_bmp(path, data, engine=None):
    """The image-crate arm of load_image_fast for a .bmp (scanner.rs:713-734): decoded on the device and returned as (h, w, 3) uint8
    Rgb8, or (h, w, 4) Rgba8 for a file with an alpha mask, the native layout of the header's BMP section.  A file the rule refuses raises
    RphError; extensions other than bmp raise ValueError.  load_image_fast itself stays JPEG-only."""
    import os

    ext = os.path.splitext(str(path))[1].lstrip(".").lower()
    if ext != "bmp":
        raise ValueError(f"load_bmp: '{ext}' is not a BMP file name")
    return (engine or default_engine()).bmp_decode(data)


def pixel_hash(image, engine=None):
    """The pixel hash of one decoded image (scanner.rs:1393-1404): blake3::hash of to_rgba16() as little-endian bytes, on the
    device.  image: (h, w) Luma8, (h, w, 3) Rgb8 or (h, w, 4) Rgba8 uint8; a uint16 array or (h, w, 2) gray + alpha (what load_png and
    load_tiff return for such files) goes through Engine.image_hash_ragged.  Returns 32 bytes."""
    a = np.asarray(image)
    if (a.dtype.kind == "u" and a.dtype.itemsize == 2) or (a.ndim == 3 and a.shape[2] == 2):
        return (engine or default_engine()).image_hash_ragged([a], want_pdq=False)["pixel_hash"][0].tobytes()
    a = np.asarray(image, np.uint8)
    return (engine or default_engine()).pixel_hash_batch(a[None])[0].tobytes()


def hash_images(images, pixel_hash=True, engine=None):
    """scanner.rs:1386-1410 for a list of decoded images of any mix of sizes and layouts (uint8 or uint16; (h, w), (h, w, 2), (h, w, 3),
    (h, w, 4)) in one GPU call: [(pdq hash, quality, PdqFeatures or None, pixel hash)] -- 32-byte hash and float quality, or
    (None, None, None, pixel hash) for an image below 5 px; pixel hash: 32 bytes, None without pixel_hash."""
    from .pdqhash import PdqFeatures

    out = (engine or default_engine()).image_hash_ragged(list(images), want_pixel_hash=pixel_hash, want_coeffs=True)
    res = []
    for i in range(len(out["valid"])):
        ph = out["pixel_hash"][i].tobytes() if pixel_hash else None
        if out["valid"][i]:
            res.append((out["hash"][i].tobytes(), float(out["quality"][i]), PdqFeatures(out["coeffs"][i]), ph))
        else:
            res.append((None, None, None, ph))
    return res


def load_image_any(path, data, engine=None, flavour=_lib.RPH_JPEG_ZUNE):
    """load_image_fast's routing (scanner.rs:461-735) over the six formats the library decodes: the file goes to the pipeline the routing
    rule names (Engine.file_format: RAW, jxl and pdf names to none, else by the bytes' magic, so a misnamed file falls through to its own
    format) and comes back as that format's device decode -- what load_image_fast, load_png, load_tiff, load_gif and load_bmp return, and
    Engine.webp_decode.  ValueError for a file no pipeline takes; RphError for one its pipeline refuses."""
    eng = engine or default_engine()
    fmt = eng.file_format(data, path)
    if fmt == _lib.RPH_FORMAT_NONE:
        raise ValueError(f"load_image_any: no pipeline of this library takes '{path}'")
    if fmt == _lib.RPH_FORMAT_JPEG:
        return eng.jpeg_decode(data, flavour)
    return getattr(eng, _lib.FORMAT_NAMES[fmt] + "_decode")(data)


def hash_files(names, datas=None, pixel_hash=True, engine=None):
    """The body of the scan loop's per-file closure (scanner.rs:1350-1417) for a list of files of any mix of formats in one call
    (Engine.files_pdq_hash_batch): [(pdq hash, quality, PdqFeatures or None, pixel hash, status, format, (w, h))] -- hash_images' tuples
    extended by the file's status (0, or why no pipeline of the library hashed it: the caller's CPU path takes the file), the pipeline
    that took it (_lib.RPH_FORMAT_*, 0: none) and the decoded image's resolution.  datas: the files' bytes; None reads the files."""
    from .pdqhash import PdqFeatures

    names = list(names)
    if datas is None:
        datas = []
        for name in names:
            with open(name, "rb") as f:
                datas.append(f.read())
    out = (engine or default_engine()).files_pdq_hash_batch(list(datas), names, want_coeffs=True, want_pixel_hash=pixel_hash)
    res = []
    for i in range(len(names)):
        rest = (int(out["status"][i]), int(out["format"][i]), (int(out["size"][i][0]), int(out["size"][i][1])))
        ph = out["pixel_hash"][i].tobytes() if pixel_hash and out["status"][i] == 0 else None
        if out["valid"][i]:
            res.append((out["hash"][i].tobytes(), float(out["quality"][i]), PdqFeatures(out["coeffs"][i]), ph) + rest)
        else:
            res.append((None, None, None, ph) + rest)
    return res


def identical_duplicates(content_hashes, pixel_hashes=None):
    """analyze_group steps 1-3 (scanner.rs:1843-1864): True for each file whose content hash is shared by another file of the group,
    or whose pixel hash is (a None entry, or pixel_hashes None, means no pixel hash).  Host code."""
    from collections import Counter

    ck = [bytes(c) for c in content_hashes]
    ph = [None if p is None else bytes(p) for p in pixel_hashes] if pixel_hashes is not None else [None] * len(ck)
    bit_counts = Counter(ck)
    pixel_counts = Counter(p for p in ph if p is not None)
    return [bit_counts[c] > 1 or (p is not None and pixel_counts[p] > 1) for c, p in zip(ck, ph)]


def is_low_pdq_quality(quality):
    return bool(_lib.load().rph_is_low_pdq_quality(-1 if quality is None else int(quality)))


def stored_quality(q):
    """scanner.rs:1416-1417: (q * 100).round().clamp(0, 100) as u16 (round half away from zero)."""
    v = np.float32(q) * np.float32(100.0)
    return int(min(100, max(0, np.floor(v + np.float32(0.5)))))


def group_with_pdqhash(hashes, similarity, coefficients=None, has_features=None, quality=None, engine=None):
    """Returns (groups, comparison_count): connected components (> 1 member, members ascending,
    groups by first member) of the edge set of group_files_generic::<[u8;32], PdqStrategy>."""
    q = None if quality is None else np.array([-1 if x is None else int(x) for x in quality], np.int32)
    return (engine or default_engine()).group_files_pdq(hashes, similarity, coefficients, has_features, q)


def merge_tree(hashes, top, coefficients=None, has_features=None, quality=None, engine=None):
    """group_with_pdqhash at every similarity 0 .. top from ONE sweep at top: a MergeTree whose groups(s) and comparisons(s) are what
    group_with_pdqhash(hashes, s, ...) returns, labels(s) the smallest file of every file's component, profile() the number of groups and
    of grouped files per s.  Where the similarity changes, cut the tree instead of grouping again."""
    return (engine or default_engine()).group_files_pdq_tree(hashes, top, coefficients, has_features, _quality32(quality))


def group_with_pdqhash_append(old_hashes, old_groups, new_hashes, similarity, old_coefficients=None, old_has_features=None, old_quality=None,
                              new_coefficients=None, new_has_features=None, new_quality=None, engine=None):
    """group_with_pdqhash for a library that was grouped before (`old_groups`: the groups that call returned) plus new files.
    Files are numbered as the concatenation library ++ new.  Returns (groups, new_comparisons): the groups group_with_pdqhash
    gives on the concatenation, and the comparisons the new files added to the library's own count."""
    def q32(quality):
        return None if quality is None else np.array([-1 if x is None else int(x) for x in quality], np.int32)

    return (engine or default_engine()).group_files_pdq_append(
        old_hashes, old_groups, new_hashes, similarity, old_coefficients, old_has_features, q32(old_quality), new_coefficients,
        new_has_features, q32(new_quality))


def _quality32(quality):
    return None if quality is None else np.array([-1 if x is None else int(x) for x in quality], np.int32)


class ScannerLibrary(Library):
    """Engine.library with the helpers' argument names and quality as a list of None / int, like group_with_pdqhash."""

    def append(self, hashes, coefficients=None, has_features=None, quality=None):
        return super().append(hashes, coefficients, has_features, _quality32(quality))

    def restore(self, hashes, groups, comparisons=0, coefficients=None, has_features=None, quality=None):
        return super().restore(hashes, groups, comparisons, coefficients, has_features, _quality32(quality))

    def query(self, hashes, quality=None, cap=None):
        return super().query(hashes, _quality32(quality), cap)

    def restore_edges(self, hashes, edges, coefficients=None, has_features=None, quality=None):
        return super().restore_edges(hashes, edges, coefficients, has_features, _quality32(quality))


def open_library(similarity, top=None, engine=None):
    """A grouped library that stays on the device between scans (ScannerLibrary): append(...) -> (labels, new_comparisons), restore(...),
    groups(), labels(), query(...).  groups() is group_with_pdqhash on the files the library holds, in order.
    remove(indices) -> (new_index, dropped) takes files out (deleted, or gone at the next scan) and renumbers the rest through new_index.
    nearest(hashes, k, max_dist=256) -> (edges[n_q, k], counts[n_q]) is the exact k-nearest search of query hashes among the resident
    files, ordered by (distance, file); nearest_files(indices, k, max_dist=256) asks it for resident files, each skipping itself.
    With `top` (similarity <= top <= 63) the library keeps its edges on the device: groups_at(s) and merge_tree(s) for any s <= top then run
    no sweep, and edges() / restore_edges(...) persist it in place of groups() / restore(...)."""
    if top is not None and not isinstance(top, (int, np.integer)):  # open_library(similarity, engine) of before this argument existed
        raise TypeError(f"top is a similarity (an int) or None, not {type(top).__name__}: pass the engine as engine=")
    return ScannerLibrary(engine or default_engine(), similarity, top)


def group_max_dist(groups, hashes, pivots, coefficients=None, has_features=None, engine=None):
    """Per-group `max_dist` of process_raw_groups (scanner.rs:2214-2241).

    `groups`: lists of file indices (in the caller's display order: the reference sorts by file name first, which stays with
    the caller); `pivots[g]`: index of the group's pivot file, i.e. the first file of the sorted group that has features, else
    the first that has a hash (the caller's find_map), or None.  With features the distance of a member is the minimum over
    the pivot's 8 dihedral hashes (one batched rph_pdq_hashes_from_coeffs for all pivots), otherwise the plain distance to the
    pivot's hash; the group's value is the maximum over its members that have a hash (here: all listed members)."""
    eng = engine or default_engine()
    hashes = np.ascontiguousarray(hashes, np.uint8).reshape(-1, 32)
    bits = np.unpackbits(hashes, axis=1)
    out = [0] * len(groups)
    with_feats = [g for g, p in enumerate(pivots)
                  if p is not None and coefficients is not None and (has_features is None or has_features[p])]
    variants = {}
    if with_feats:
        c = np.ascontiguousarray(np.asarray(coefficients, np.float32).reshape(-1, 256)[[pivots[g] for g in with_feats]])
        _, dih = eng.pdq_hashes_from_coeffs(c, want_hash=False, want_dihedral=True)
        variants = {g: np.unpackbits(dih[k], axis=1) for k, g in enumerate(with_feats)}
    for g, members in enumerate(groups):
        p = pivots[g]
        if p is None or not len(members):
            continue
        mb = bits[np.asarray(members, np.int64)]
        if g in variants:
            d = (mb[:, None, :] != variants[g][None, :, :]).sum(axis=2).min(axis=1)
        else:
            d = (mb != bits[p][None, :]).sum(axis=1)
        out[g] = int(d.max())
    return out


def groups_max_dist(groups, hashes, pivots=None, coefficients=None, has_features=None, want_member_dist=False, engine=None):
    """group_max_dist for all groups in one device call (Engine.group_max_dist): same rule and arguments, and pivots=None selects the
    reference's find_map pair per group (the first listed member that has features, else the first listed member).  A library that is
    resident answers without the hashes: ScannerLibrary.group_max_dist(groups, pivots)."""
    return (engine or default_engine()).group_max_dist(groups, hashes, pivots, coefficients, has_features, want_member_dist)
