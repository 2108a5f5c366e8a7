"""Mixed lists of files for the tests of rph_file_format and rph_files_pdq_hash_batch (test_files_cpu.py, test_files_gpu.py):

  - the routing rule's table: (bytes, name, expected format) for every magic, its near misses, the names that rule a file out and the
    names that do not, and a Python statement of Rust's Path::extension for the extractor;
  - the corpus per format: valid and refused files of file_chunks.py's pools for PNG, TIFF, WebP, GIF and BMP, small JPEGs from Pillow, per
    format one 600 x 400 image (a side above 512 px: the pre-downsample's shared scratch), for PNG and TIFF a 16-bit and a gray + alpha
    image (the shared planes of the ragged hasher);
  - the interleaved mix with its oddities, and what every file of a list gets from its own format's batch call."""
import functools

import numpy as np

import file_chunks as fc

NONE, JPEG, PNG, TIFF, WEBP, GIF, BMP = range(7)
FORMATS = ("jpeg",) + fc.FORMATS  # by RPH_FORMAT_* - 1
KEYS = ("hash", "quality", "coeffs", "dihedral", "valid", "status", "pixel_hash")
INVALID_ARG, UNSUPPORTED = -1, -5

MAGIC = {
    PNG: [b"\x89PNG\r\n\x1a\n"],
    JPEG: [b"\xff\xd8\xff"],
    GIF: [b"GIF87a", b"GIF89a"],
    WEBP: [b"RIFF\x10\x00\x00\x00WEBP"],
    TIFF: [b"MM\x00\x2a", b"II\x2a\x00"],
    BMP: [b"BM"],
}


def raw_exts():
    """the names recorded from the reference's RAW_EXTS"""
    import os

    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "raw_exts.txt")) as f:
        return f.read().split()


def mixed_case(s):
    return "".join(c.upper() if k % 2 else c for k, c in enumerate(s))


def path_extension(name):
    """Rust's Path::extension of the last component after the last '/' (str -> str or None): None without a '.', for a component that
    starts with its only '.', and for '..'; else the part after the last '.', which may be empty"""
    comp = name.rsplit("/", 1)[-1]
    if comp == ".." or "." not in comp:
        return None
    before, after = comp.rsplit(".", 1)
    return None if before == "" else after


EXTENSION_NAMES = ["a.jpg", "a.tar.gz", "a", "", ".png", ".a.png", "..", "...", "a.", "a..", "dir.jpg/a", "dir.jpg/a.PNG", "dir/.hidden", "dir/", "/", "a.jpg/",
                   "x/../y.nef", "..a", "a.b/.c", "ä.öü", "a.JpG", "./a", "a/.", "a/..", "nef", ".nef", "a.nef.", "a b.c d"]


def format_table():
    """[(bytes, name or None, expected RPH_FORMAT_*)]"""
    png = MAGIC[PNG][0] + b"\x00" * 24
    t = []
    for fmt, magics in MAGIC.items():
        for m in magics:
            t.append((m, None, fmt))  # the magic exactly
            t.append((m + b"\x00" * 40, "a.bin", fmt))
            t.append((m[:-1], None, NONE))  # one byte short
    t.append((b"RIFF\x10\x00\x00\x00WAVE", None, NONE))
    t.append((b"RIFF\x10\x00\x00\x00WEB", None, NONE))  # WEBP cut at 11 bytes
    t.append((b"RIFF", "a.webp", NONE))
    t.append((b"II+\x00\x08\x00\x00\x00", "a.tif", NONE))  # BigTIFF
    t.append((b"MM\x00+\x00\x08\x00\x00", "a.tif", NONE))
    for n in range(4):  # lengths 0 to 3 of bytes that are no magic, and of the start of every magic
        t.append((b"\x00\x01\x02"[:n], None, NONE))
        for fmt, magics in MAGIC.items():
            for m in magics:
                t.append((m[:n], "a.png", fmt if n >= len(m) else NONE))
    for ext in raw_exts() + ["jxl", "pdf"]:
        for e in (ext, ext.upper(), mixed_case(ext)):
            t.append((png, "a." + e, NONE))
            t.append((png, "dir/b.c." + e, NONE))
        t.append((png, ext, PNG))  # a name without a '.' has no extension
        t.append((png, "." + ext, PNG))
        t.append((png, "a." + ext + "x", PNG))
        t.append((png, "a." + ext + "/b", PNG))
    for name in ("a.jpg", "a.tif", "a.dat", "a", ".png", "dir.jpg/a", "a.", None):
        t.append((png, name, PNG))
    t.append((MAGIC[JPEG][0] + b"\xe0", "a.png", JPEG))  # the magic, not the name
    t.append((b"hello, world", "a.jpg", NONE))  # a known extension over an unknown magic
    return t


# ------------------------------------------------------------------ corpus
def _photo(w, h, seed, ch=3):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    base = np.stack([(np.sin(x / 9.0 + c) + np.cos(y / 6.0 - c)) * 60 + 128 for c in range(ch)], -1)
    return np.clip(base + rng.normal(0, 12, (h, w, ch)), 0, 255).astype(np.uint8)


def _jpegs():
    import jpeg_util as ju

    out = []
    for w, h in ((48, 40), (200, 136)):
        out.append((f"baseline420_{w}x{h}", ju.pillow_jpeg(ju.make_image(w, h, seed=w), quality=85, subsampling=2)))
        out.append((f"gray_{w}x{h}", ju.pillow_jpeg(ju.make_image(w, h, "L", seed=w + 1), quality=85)))
        out.append((f"progressive_{w}x{h}", ju.pillow_jpeg(ju.make_image(w, h, seed=w + 2), quality=85, subsampling=2, progressive=True)))
    out.append(("baseline420_600x400", ju.pillow_jpeg(ju.make_image(600, 400, seed=7), quality=80, subsampling=2)))
    out.append(("s444_130x90", ju.pillow_jpeg(ju.make_image(130, 90, seed=8), quality=90, subsampling=0)))
    out.append(("s422_131x77", ju.pillow_jpeg(ju.make_image(131, 77, seed=9), quality=75, subsampling=1)))
    out.append(("gray_progressive_90x70", ju.pillow_jpeg(ju.make_image(90, 70, "L", seed=10), quality=90, progressive=True)))
    out.append(("restart_160x120", ju.pillow_jpeg(ju.make_image(160, 120, seed=11), quality=85, subsampling=2, restart_marker_blocks=3)))
    out.append(("small_4x9", ju.pillow_jpeg(ju.make_image(4, 9, seed=12), quality=85)))  # below 5 px: valid 0, status 0, a pixel hash
    return out


def _large_and_deep(fmt):
    """the format's 600 x 400 image, and for PNG and TIFF a 16-bit and a gray + alpha image"""
    rng = np.random.default_rng(600)
    if fmt == "png":
        import png_util as pu

        return [("rgb8_600x400", pu.encode(_photo(600, 400, 1), 2, 8)), ("rgb16_70x50", pu.make_file(rng, 70, 50, 2, 16, False)),
                ("graya8_60x45", pu.make_file(rng, 60, 45, 4, 8, False))]
    if fmt == "tiff":
        import tiff_util as tu

        return [("rgb8_lzw_600x400", tu.encode(_photo(600, 400, 2).astype(np.int64), compression=5, rows_per_strip=32)),
                ("rgb16_70x50", tu.make_file(rng, 70, 50, 2, 3, 16, compression=5)), ("graya8_60x45", tu.make_file(rng, 60, 45, 1, 2, 8, compression=8))]
    if fmt == "webp":
        import webp_util as wu

        return [("photo_600x400", wu.encode(_photo(600, 400, 3), [("green",)]))]
    if fmt == "gif":
        import gif_streams as gs

        return [("frame_600x400", gs.image_gif(_photo(600, 400, 4, 1)[:, :, 0] // 8, gs.colour_palette(32, 5))[0])]
    import bmp_streams as bs

    return [("rgb24_600x400", bs.make("rgb24", 600, 400, seed=5)[0])]


PER_FORMAT = 12


@functools.lru_cache(maxsize=None)
def valid(fmt):
    """PER_FORMAT (name, bytes) of files the format's pipeline decodes"""
    if fmt == "jpeg":
        out = _jpegs()
    else:
        extra = _large_and_deep(fmt)
        ok = sorted(fc.of_kind(fmt, "ok"), key=lambda f: (-f.q["pixels"], f.name))
        pick = ok[::max(1, len(ok) // (PER_FORMAT - len(extra)))][:PER_FORMAT - len(extra)]
        out = extra + [(f.name, f.data) for f in pick]
    assert len(out) == PER_FORMAT and len({d for _, d in out}) == PER_FORMAT, fmt
    return tuple(out)


@functools.lru_cache(maxsize=None)
def refused(fmt):
    """one file the format's magic routes to its pipeline and the pipeline refuses"""
    if fmt == "jpeg":
        import jpeg_util as ju

        return ju.pillow_jpeg(ju.make_image(40, 30, seed=3).convert("CMYK"), quality=80)  # four components: RPH_ERR_UNSUPPORTED
    bad = [f for f in fc.of_kind(fmt, "decode", "parse") if file_format(f.data, None) == FORMATS.index(fmt) + 1]
    assert bad, fmt
    return bad[0].data


def file_format(data, name):
    from rupphash_amd import Engine

    return Engine.file_format(data, name)


def ext_of(fmt):
    return dict(jpeg="jpg", png="png", tiff="tif", webp="webp", gif="gif", bmp="bmp")[fmt]


@functools.lru_cache(maxsize=None)
def mix():
    """(files, names, index of the PNG named .jpg): PER_FORMAT files of each format in round-robin order, and sprinkled through them a
    refused file per format, a null entry, an empty one, a file of no format, a RAW-named TIFF and a PNG named .jpg"""
    import png_util as pu

    odd = [(refused(fmt), "refused." + ext_of(fmt)) for fmt in FORMATS]
    odd += [(None, "null.png"), (b"", "empty.jpg"), (b"no format's magic starts these bytes", "none.jpg"), (valid("tiff")[3][1], "raw_named.NEF"),
            (pu.encode(_photo(90, 60, 9), 2, 8), "misnamed.jpg")]  # (RGB, 8 bits: Pillow and blake3_util decode and hash it without the library)
    files, names, j = [], [], 0
    for k in range(PER_FORMAT):
        for fmt in FORMATS:
            name, data = valid(fmt)[k]
            files.append(data)
            # (names: mostly the format's own extension, some without a name, some with a directory)
            names.append(None if (k + len(fmt)) % 5 == 0 else f"dir.{k}/{name}.{ext_of(fmt)}")
            if len(files) % 7 == 3 and j < len(odd):
                files.append(odd[j][0])
                names.append(odd[j][1])
                j += 1
    assert j == len(odd)
    return tuple(files), tuple(names), names.index("misnamed.jpg")


def one_of_each():
    """(files, names): one valid file per format"""
    return [valid(fmt)[1][1] for fmt in FORMATS], [f"one.{ext_of(fmt)}" for fmt in FORMATS]


# ------------------------------------------------------------------ expectation
def info(fmt, data):
    """(w, h) by the format's _info"""
    from rupphash_amd import Engine

    return Engine.jpeg_info(data)[:2] if fmt == "jpeg" else Engine._file_info(fmt, data)[:2]


def format_batch(e, fmt, files, threads=0, flavour=0, **want):
    """the format's own batch call"""
    from rupphash_amd import RphError

    if fmt != "jpeg":
        return getattr(e, fmt + "_pdq_hash_batch")(files, threads=threads, **want)
    try:
        return e.jpeg_pdq_hash_batch(files, flavour=flavour, threads=threads, **want)
    except RphError as err:  # (a JPEG call of one file returns that file's status)
        assert len(files) == 1 and err.status in (INVALID_ARG, UNSUPPORTED)
        out = e.jpeg_pdq_hash_batch([valid("jpeg")[0][1]], flavour=flavour, threads=threads, **want)
        out = {k: (None if v is None else np.zeros_like(v)) for k, v in out.items()}
        out["status"][0] = err.status
        return out


def expected(e, files, names=None, threads=0, flavour=0, want_quality=True, want_coeffs=True, want_dihedral=True, want_pixel_hash=True):
    """what files_pdq_hash_batch must return for the list: every format's files in order through the format's own batch call on the same
    context, scattered back; format by the rule, size by the _info calls"""
    n = len(files)
    names = names if names is not None else [None] * n
    want = dict(want_quality=want_quality, want_coeffs=want_coeffs, want_dihedral=want_dihedral, want_pixel_hash=want_pixel_hash)
    out = {"hash": np.zeros((n, 32), np.uint8), "quality": np.zeros(n, np.float32) if want_quality else None,
           "coeffs": np.zeros((n, 256), np.float32) if want_coeffs else None, "dihedral": np.zeros((n, 8, 32), np.uint8) if want_dihedral else None,
           "valid": np.zeros(n, np.uint8), "status": np.zeros(n, np.int32), "format": np.zeros(n, np.uint8), "size": np.zeros((n, 2), np.uint32)}
    if want_pixel_hash:
        out["pixel_hash"] = np.zeros((n, 32), np.uint8)
    route = [file_format(f, nm) if f else NONE for f, nm in zip(files, names)]
    for i, f in enumerate(files):
        if route[i] == NONE:
            out["status"][i] = UNSUPPORTED if f else INVALID_ARG
    for fi, fmt in enumerate(FORMATS):
        idx = [i for i in range(n) if route[i] == fi + 1]
        if not idx:
            continue
        got = format_batch(e, fmt, [files[i] for i in idx], threads, flavour, **want)
        for key, arr in got.items():
            if arr is not None:
                out[key][idx] = arr
        out["format"][idx] = fi + 1
        for k, i in enumerate(idx):
            if got["status"][k] == 0:
                out["size"][i] = info(fmt, files[i])
    return out


def same(got, want, where=""):
    """every output of `want` bit for bit in `got` -> the number of arrays compared"""
    m = 0
    for key, w in want.items():
        g = got[key]
        assert (g is None) == (w is None), (where, key)
        if w is None:
            continue
        assert g.dtype == w.dtype and g.shape == w.shape, (where, key, g.dtype, g.shape)
        if g.tobytes() != w.tobytes():
            rows = [i for i in range(len(w)) if np.asarray(g[i]).tobytes() != np.asarray(w[i]).tobytes()]
            raise AssertionError((where, key, "files", rows[:10]))
        m += 1
    assert set(got) == set(want), (where, set(got) ^ set(want))
    return m
