"""How the PNG, TIFF, WebP, GIF and BMP batch calls cut a call into chunks (the split loop of every *_pipeline.cpp's run()), for the tests
of those cuts (test_file_chunks_cpu.py, test_file_chunks_gpu.py; numpy and the library's host-only calls, no device):

  - one pool of distinct small files per format from the formats' own helpers: valid files (geometries on both sides of 128 px, one side
    above 512, every depth class), files the parser refuses (they never enter a chunk) and, where the format has them, files that parse
    and fail while they are decoded (they get their status from inside a chunk);
  - the split rule in Python, over the quantities that follow from a file's structure without a decoder: file count, pixels, PNG raw
    bytes, TIFF decoded bytes, GIF index bytes, BMP source and native bytes.  Compressed bytes and WebP table bytes are not predicted;
  - the limits the tests lower (rph_internal.h, rph_file_limits), the small values chosen for them and the environment that sets them;
  - the calls: ordered lists over the pool with repeats;
  - the comparison of a call's outputs with what every file gets alone."""
import functools
import struct
from collections import namedtuple

import numpy as np

FORMATS = ("png", "tiff", "webp", "gif", "bmp")
KEYS = ("hash", "quality", "coeffs", "dihedral", "valid", "status", "pixel_hash")

# rph_file_limits: the defaults, and the variable rph_init reads each one from
DEFAULTS = dict(files=8192, comp=256 << 20, raw=768 << 20, pixels=192 << 20, webp_chunk_tables=256 << 20, webp_window_tables=1 << 30,
                bmp_src=256 << 20, bmp_out=384 << 20)
ENV = dict(files="RPH_FILE_CHUNK_FILES", comp="RPH_FILE_CHUNK_COMP_BYTES", raw="RPH_FILE_CHUNK_RAW_BYTES", pixels="RPH_FILE_CHUNK_PIXELS",
           webp_chunk_tables="RPH_WEBP_CHUNK_TABLE_BYTES", webp_window_tables="RPH_WEBP_WINDOW_TABLE_BYTES", bmp_src="RPH_BMP_CHUNK_SRC_BYTES",
           bmp_out="RPH_BMP_CHUNK_OUT_BYTES")
# the running sums of a format's split loop that this helper predicts (beside the file count), and the limits it does not
PREDICTED = dict(png=("raw", "pixels"), tiff=("raw", "pixels"), webp=("pixels",), gif=("raw", "pixels"), bmp=("bmp_src", "bmp_out"))
UNPREDICTED = dict(png=("comp",), tiff=("comp",), webp=("comp", "webp_chunk_tables"), gif=("comp",), bmp=())
HAS_DECODE_FAILURES = ("png", "tiff", "webp", "gif")  # (a BMP's RLE stream is decoded by the parser)

# kind: "ok" (decodes), "decode" (parses, then fails inside a chunk) or "parse" (refused before the chunks are formed); q: the file's
# share of every predicted sum (and, for TIFF, its compressed bytes as the AUTO mode counts them)
PoolFile = namedtuple("PoolFile", "name data kind q")


def _align(v, a):
    return -(-v // a) * a


def _status(fn, data):
    from rupphash_amd import RphError

    try:
        fn(data)
    except RphError as e:
        return e.status
    return 0


# ------------------------------------------------------------------ quantities
def gif_frame_size(data):
    """(fw, fh) of the first image descriptor of a file the parser takes"""
    o = 13 + ((3 << ((data[10] & 7) + 1)) if data[10] & 0x80 else 0)
    while data[o] != 0x2c:
        assert data[o] == 0x21
        o += 2
        while data[o]:
            o += 1 + data[o]
        o += 1
    return struct.unpack_from("<HH", data, o + 5)


def quantities(fmt, data):
    """the sums' shares of a file that parses"""
    from rupphash_amd import Engine

    w, h, ch, _ = getattr(Engine, fmt + "_info")(data)
    q = dict(pixels=w * h)
    if fmt == "png":  # scanlines with their filter bytes, the Adam7 passes summed
        import png_util as pu

        q["raw"] = pu.parse(data)[1]["raw_bytes"]
    elif fmt == "tiff":  # every strip or tile in a slot of whole 16 bytes; staged segments of whole 4 bytes
        import tiff_util as tu

        i = tu.parse(data)[1]
        q["raw"] = len(i["segs"]) * _align(i["sh"] * i["rb"], 16)
        q["comp"] = sum(_align(c, 4) for _, c, _, _ in i["segs"])
    elif fmt == "gif":
        fw, fh = gif_frame_size(data)
        q["raw"] = fw * fh
    elif fmt == "bmp":  # bmp_kernels.hip: source rows and native rows are multiples of 4 bytes; an RLE stream arrives as an 8-bit plane
        bits, comp = struct.unpack_from("<HI", data, 28)
        q["bmp_src"] = _align(w if comp in (1, 2) else (w * bits + 7) // 8, 4) * h
        q["bmp_out"] = _align(w * ch, 4) * h
    return q


# streams of webp_util.rule_corpus() that the front of the parser takes and the main ARGB stream's decoder refuses (the host-only calls do
# not tell the two apart: the chunk sizes the device reports do)
WEBP_MAIN_STREAM = ("distance_before_first_pixel", "copy_past_last_pixel", "out_of_bits")


def classify(fmt, name, data):
    from rupphash_amd import Engine

    if _status(getattr(Engine, fmt + "_info"), data):
        return PoolFile(name, data, "parse", None)
    if not _status(getattr(Engine, fmt + "_decode_host"), data):
        return PoolFile(name, data, "ok", quantities(fmt, data))
    if fmt == "bmp" or (fmt == "webp" and not name.startswith("main_stream_") and name not in WEBP_MAIN_STREAM):
        return PoolFile(name, data, "parse", None)  # (a WebP whose tables or transforms are damaged: refused by the front)
    return PoolFile(name, data, "decode", quantities(fmt, data))


# ------------------------------------------------------------------ pools
def _png_files():
    import png_util as pu

    rng = np.random.default_rng(41)
    out = []
    # (w, h, colour type, depth, tRNS, interlaced): both sides of 128 px, a side above 512 (the largest file), 8 and 16 bits, low depths
    for w, h, ct, d, t, il in [(200, 150, 2, 8, False, False), (130, 140, 6, 8, False, False), (127, 129, 0, 8, False, False), (128, 128, 3, 8, True, False),
                               (600, 100, 2, 8, False, False), (129, 64, 2, 8, True, False), (64, 48, 2, 16, False, False), (150, 130, 6, 16, False, False),
                               (33, 21, 0, 16, True, False), (40, 30, 4, 16, False, False), (131, 130, 2, 16, False, True), (90, 70, 2, 8, False, True),
                               (50, 40, 6, 16, False, True), (100, 80, 0, 1, False, False), (77, 33, 3, 4, False, True), (30, 20, 0, 2, False, False),
                               (140, 128, 4, 8, False, False), (131, 130, 2, 8, False, False), (131, 130, 2, 8, False, False), (4, 9, 2, 8, False, False),
                               (1, 1, 6, 8, False, False), (160, 120, 3, 8, False, False)]:
        out.append((f"ct{ct}_d{d}_t{int(t)}_i{int(il)}_{w}x{h}_{len(out)}", pu.make_file(rng, w, h, ct, d, t, interlace=il)))
    out += pu.valid_corpus()[3::9]
    # a larger file with one bit of its zlib stream flipped behind the CRC: it parses and fails while it is inflated
    b = bytearray(pu.make_file(rng, 130, 140, 2, 8, False))
    p, n = pu._idat_pos(b)
    b[p + 8 + n // 2] ^= 4
    pu._recrc(b, p)
    out.append(("bit_flip_in_stream_130x140", bytes(b)))
    return out + [(n, d) for n, d, s in pu.rule_corpus() if s][::2]


def _tiff_files():
    import tiff_util as tu

    rng = np.random.default_rng(42)
    out = []
    # (w, h, photometric, samples, bits, keywords)
    for w, h, photo, spp, bps, kw in [(200, 150, 2, 3, 8, dict(compression=5, predictor=2)), (130, 140, 2, 4, 8, dict(compression=8)),
                                      (127, 129, 1, 1, 8, dict(compression=32773)), (128, 128, 2, 3, 8, dict(compression=1, rows_per_strip=7)),
                                      (600, 100, 2, 3, 8, dict(compression=5, tile=(64, 64))), (129, 64, 0, 1, 8, dict(compression=1)),
                                      (64, 48, 2, 3, 16, dict(compression=5)), (150, 130, 2, 4, 16, dict(compression=8, predictor=2, bo=">")),
                                      (33, 21, 1, 1, 16, dict(compression=1)), (40, 30, 1, 2, 16, dict(compression=32773)),
                                      (131, 130, 2, 3, 16, dict(compression=5, predictor=2, tile=(32, 16))), (90, 70, 2, 3, 8, dict(compression=8, tile=(48, 64))),
                                      (100, 80, 1, 1, 1, dict(compression=5)), (77, 33, 0, 1, 4, dict(compression=1, bo=">")),
                                      (140, 128, 1, 2, 8, dict(compression=5, rows_per_strip=3)), (131, 130, 2, 3, 8, dict(compression=1)),
                                      (131, 130, 2, 3, 8, dict(compression=5)), (4, 9, 2, 3, 8, dict(compression=5)), (1, 1, 2, 4, 8, dict(compression=8)),
                                      (160, 120, 2, 3, 8, dict(compression=32773, rows_per_strip=16))]:
        out.append((f"p{photo}_s{spp}_b{bps}_c{kw['compression']}_{w}x{h}_{len(out)}", tu.make_file(rng, w, h, photo, spp, bps, **kw)))
    # flat content at more than 16 decoded bytes per compressed byte: alone, AUTO hands these to the device
    out.append(("flat_lzw_200x120", tu.encode(np.zeros((120, 200, 3), np.int64) + 9, compression=5, rows_per_strip=30)))
    out.append(("flat_deflate_180x150", tu.encode(np.zeros((150, 180, 3), np.int64) + 77, compression=8)))
    out.append(("flat_packbits_190x100", tu.encode(np.zeros((100, 190), np.int64) + 3, compression=32773)))
    out += tu.valid_corpus()[5::17]
    # a larger Deflate file with one bit of its strip flipped: it parses and fails while it is inflated (the Adler-32 at the latest)
    b = bytearray(tu.make_file(rng, 130, 140, compression=8))
    b[(8 + struct.unpack("<I", b[4:8])[0]) // 2] ^= 4
    out.append(("bit_flip_in_deflate_130x140", bytes(b)))
    return out + [(n, d) for n, d, s in tu.rule_corpus() if s][::5]


def _webp_files():
    import webp_util as wu

    rng = np.random.default_rng(43)
    base = [(n, d) for n, d in wu.valid_corpus() if not n.startswith(("distance_code", "predictor_mode", "size_1x16384"))]
    out = base[::2] + base[1::4]
    out.append(("photo_130x129", wu.encode(wu.photo(rng, 130, 129), [("predictor", 4, "mixed")], refs="lz", seed=1)))
    out.append(("photo_alpha_128x140", wu.encode(wu.photo(rng, 128, 140, alpha=True), [("green",)], cache_bits=5, refs="lz")))
    out.append(("palette_140x127", wu.encode(wu.flat(rng, 140, 127, 11), [("palette",)], refs="lz")))
    out.append(("palette_300x160", wu.encode(wu.flat(rng, 300, 160, 40), [("palette",), ("predictor", 5, "mixed")], refs="lz", seed=2)))
    # main streams that end in a copy past the last pixel: the front takes these files, the chunk's decoder refuses them
    lits = lambda n: [("lit", 0xff000000 + 977 * k) for k in range(n)]
    for w, h in ((19, 14), (70, 31), (129, 5)):
        out.append((f"main_stream_copy_past_last_pixel_{w}x{h}", wu.encode(np.zeros((h, w, 3), np.uint8), tokens=lits(w * h - 5) + [("ref", 6, 120 + 2)])))
    rule = wu.rule_corpus()
    out += [(n, d) for n, d, _ in rule if n in WEBP_MAIN_STREAM]
    return out + [(n, d) for n, d, s in rule if s and n not in WEBP_MAIN_STREAM and not n.startswith("tables_")][::3]


def _gif_files():
    import gif_streams as gs

    rng = np.random.default_rng(44)
    valid = [(n, d) for n, d, _ in gs.valid_files()]
    keep = ("frame_at_offset", "frame_past_the_screen", "transparent_index_interlaced_offset", "clear_every_300_large", "flat_image_large", "deferred_clear_2",
            "above_512_700x90", "width_129", "small_1x1", "small_4x9", "interlaced_h67", "interlaced_h5")
    out = [f for f in valid if f[0] in keep] + [f for f in valid if f[0] not in keep][::4]
    out += [f for f in gs.pillow_files() if f[0] in ("noise_300x200", "interlaced_67", "transparent", "colours_256", "size_64x48")]
    # both sides of 128 px, frames above 16 KiB of indices, an interlaced frame at an offset on a larger screen
    for w, h, kw in [(130, 140, dict()), (128, 128, dict(interlace=True)), (127, 129, dict(local=True)), (200, 150, dict(clear=300)),
                     (150, 120, dict(screen=(180, 131), pos=(9, 7), interlace=True, trans=3)), (131, 130, dict()), (131, 130, dict(clear="never"))]:
        out.append((f"frame_{w}x{h}_{len(out)}", gs.image_gif(rng.integers(0, 32, (h, w)) // (1 + len(out) % 3), gs.colour_palette(32, len(out)), **kw)[0]))
    # frames far larger than their screens: many index bytes for few pixels
    for w, h in ((200, 150), (190, 150), (150, 120)):
        out.append((f"frame_{w}x{h}_on_40x30", gs.image_gif(rng.integers(0, 16, (h, w)) // 3, gs.colour_palette(16, w), screen=(40, 30), pos=(3, 2))[0]))
    # a larger frame whose stream ends half way: it parses and fails while it is decoded
    idx, pal = rng.integers(0, 64, (140, 130)), gs.colour_palette(64, 50)
    stream = gs.pack_codes(gs.lzw_encode(idx.ravel(), 6), 6)
    out.append(("out_of_bits_130x140", gs.write_gif((130, 140), (0, 0), (130, 140), 6, stream[:len(stream) // 2], gct=pal)))
    return out + [(n, d) for n, d, _ in gs.damaged_files()][::3]


def _bmp_files():
    import bmp_streams as bs

    geo = [(128, 128), (131, 130), (200, 150), (129, 140), (4, 9), (64, 64), (127, 140), (33, 17), (130, 127)]
    out = []
    for k, v in enumerate(bs.VARIANTS):  # every depth class, twice: a larger and a smaller geometry, both row orders
        for w, h in (geo[k % len(geo)], geo[(k + 4) % len(geo)]):
            out.append((f"{v}_{w}x{h}", bs.make(v, w, h, bool(k & 1), seed=k)[0]))
    out.append(("rgb24_600x100", bs.make("rgb24", 600, 100, seed=70)[0]))  # a side above 512: the largest file
    out.append(("rgb24_131x130_again", bs.make("rgb24", 131, 130, seed=71)[0]))
    out.append(("rgb24_1x1", bs.make("rgb24", 1, 1)[0]))
    return out + [(n, d) for n, d, _ in bs.damaged_files()][::7]


@functools.lru_cache(maxsize=None)
def pool(fmt):
    """the format's distinct files, classified by the host-only calls"""
    files = dict(png=_png_files, tiff=_tiff_files, webp=_webp_files, gif=_gif_files, bmp=_bmp_files)[fmt]()
    seen, out = set(), []
    for name, data in files:
        if data not in seen:
            seen.add(data)
            out.append(classify(fmt, name, data))
    assert len({f.name for f in out}) == len(out)
    return tuple(out)


def of_kind(fmt, *kinds):
    return [f for f in pool(fmt) if f.kind in kinds]


# ------------------------------------------------------------------ the rule
def bound(fmt, key, limits):
    """what a sum is compared with: GIF and WebP pixels take 4 bytes, so their loops allow half the pixel limit"""
    return limits[key] // 2 if key == "pixels" and fmt in ("gif", "webp") else limits[key]


def _split(fmt, files, limits, max_files):
    """files: the ones that parsed, in call order.  A chunk takes files while every running sum stays at or below its limit; its first file
    is always taken; at most max_files files.  -> (sizes, causes): causes[c] = the limits that ended chunk c (empty: the files ran out)"""
    sizes, causes, a = [], [], 0
    while a < len(files):
        b, sums = a, dict.fromkeys(PREDICTED[fmt], 0)
        while b < len(files) and (max_files is None or b - a < max_files):
            if b > a and any(sums[k] + files[b].q[k] > bound(fmt, k, limits) for k in sums):
                break
            for k in sums:
                sums[k] += files[b].q[k]
            b += 1
        why = set()
        if b < len(files):
            if max_files is not None and b - a >= max_files:
                why.add("files")
            why.update(k for k in sums if sums[k] + files[b].q[k] > bound(fmt, k, limits))
        sizes.append(b - a)
        causes.append(why)
        a = b
    return sizes, causes


def predict(fmt, call, limits):
    """(sizes, causes) of the chunks of one call (a list of PoolFile) under `limits`, by the predicted sums alone.  WebP: the file limit
    bounds the parse windows, counted over every file of the call; the chunks of a window hold no file of the next one."""
    if fmt != "webp":
        return _split(fmt, [f for f in call if f.kind != "parse"], limits, limits["files"])
    sizes, causes = [], []
    for a in range(0, len(call), limits["files"]):
        s, c = _split(fmt, [f for f in call[a:a + limits["files"]] if f.kind != "parse"], limits, None)
        if s and a + limits["files"] < len(call):
            c[-1] = {"files"}
        sizes += s
        causes += c
    if causes:
        causes[-1] = set()
    return sizes, causes


# ------------------------------------------------------------------ limits
@functools.lru_cache(maxsize=None)
def _small(fmt):
    """the small value of every limit this format reads.  A predicted sum: the second largest share among the pool's files, so that the
    largest file alone exceeds it (a chunk of its own) and every other file fits.  The others: a few files' worth."""
    out = dict(files=8, comp=4096, webp_chunk_tables=40000, webp_window_tables=200000)
    for k in PREDICTED[fmt]:
        shares = sorted({f.q[k] for f in of_kind(fmt, "ok", "decode")})
        out[k] = shares[-2] * (2 if k == "pixels" and fmt in ("gif", "webp") else 1)
    return out


def limit_keys(fmt):
    """the limits the format's run() reads: predicted ones first"""
    return ("files",) + PREDICTED[fmt] + UNPREDICTED[fmt] + (("webp_window_tables",) if fmt == "webp" else ())


def lowered(fmt, *keys, **values):
    """the default limits with `keys` at their small values and `values` as given"""
    out = dict(DEFAULTS)
    out.update({k: _small(fmt)[k] for k in keys})
    out.update(values)
    return out


def environment(limits):
    """{variable: value} of the limits that differ from the defaults"""
    return {ENV[k]: str(v) for k, v in limits.items() if v != DEFAULTS[k]}


# ------------------------------------------------------------------ calls
def _sprinkle(files, extra, every, phase=0):
    """`extra` (files the parser refuses) put one by one behind every `every`-th file, what is left of them at the end"""
    out, j = [], 0
    for k, f in enumerate(files):
        out.append(f)
        if extra and (k + phase) % every == every - 1:
            out.append(extra[j % len(extra)])
            j += 1
    return out + list(extra[j:])


@functools.lru_cache(maxsize=None)
def calls(fmt):
    """{name: tuple of PoolFile}: every pool file three times over, ascending by size (every chunk larger than the one before: every kept
    buffer regrows mid-call), descending, shuffled, and -- `edges` -- an arrangement that, with 8 files per chunk, opens one chunk with a
    file that fails while it is decoded, ends the next one with such a file and fills the third with nothing else (BMP, which has no such
    files: the files its parser refuses first, last and eight in a row)"""
    enter, refused = of_kind(fmt, "ok", "decode"), of_kind(fmt, "parse")
    size = lambda f: (f.q["pixels"], f.name)
    asc = sorted(enter * 3, key=size)
    rng = np.random.default_rng(5)
    everything = list(enter) * 3 + list(refused) * 2
    out = dict(ascending=_sprinkle(asc, refused, 9), descending=_sprinkle(asc[::-1], refused, 7, 3),
               shuffled=[everything[i] for i in rng.permutation(len(everything))])
    rest = list(enter) * 2 + list(refused) * 2
    rest = [rest[i] for i in rng.permutation(len(rest))]
    if fmt in HAS_DECODE_FAILURES:
        bad, ok = of_kind(fmt, "decode"), sorted(of_kind(fmt, "ok"), key=size)
        out["edges"] = [bad[0]] + ok[:7] + ok[7:14] + [bad[1]] + [bad[k % len(bad)] for k in range(8)] + rest
    else:
        out["edges"] = refused[:1] + rest[:20] + [refused[k % len(refused)] for k in range(8)] + rest[20:] + refused[1:2]
    return {k: tuple(v) for k, v in out.items()}


def exact_fit(fmt, call, k):
    """limits at which the first k files of `call` that parse fill every predicted sum of the first chunk exactly: with them the k-th file
    stays in the chunk; with every one of them one lower (two for the halved pixel limit) it opens the next chunk"""
    first = [f for f in call if f.kind != "parse"][:k]
    at, below = {}, {}
    for key in PREDICTED[fmt]:
        total = sum(f.q[key] for f in first)
        halved = key == "pixels" and fmt in ("gif", "webp")
        at[key], below[key] = (2 * total, 2 * total - 2) if halved else (total, total - 1)
    return lowered(fmt, **at), lowered(fmt, **below)


def tiff_auto_call():
    """(call, limits): AUTO decides per chunk from decoded bytes >= 16 x compressed bytes.  Eight flat files (far above 16:1) in front of
    files that barely compress: below 16:1 as one chunk, and, with 8 files per chunk, one chunk at or above it -- the split changes which
    decoder the flat files get"""
    ok = of_kind("tiff", "ok")
    flat = [f for f in ok if f.name.startswith("flat_")]
    plain = [f for f in ok if f.q["raw"] < 4 * f.q["comp"]]
    call = [flat[k % len(flat)] for k in range(8)] + _sprinkle(plain * 2, of_kind("tiff", "decode", "parse"), 5)
    return tuple(call), lowered("tiff", "files")


# ------------------------------------------------------------------ comparison
def compare(out, call, alone):
    """every output of every file of the call against what the file got alone (alone[name]: the outputs of a one-file call), bit for bit;
    -> the number of files compared"""
    n = 0
    for k, f in enumerate(call):
        ref = alone[f.name]
        for key in KEYS:
            got, want = np.asarray(out[key][k]), np.asarray(ref[key][0])
            assert got.dtype == want.dtype and got.tobytes() == want.tobytes(), (k, f.name, key)
        n += 1
    return n
