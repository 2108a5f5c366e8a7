"""The grids of recon_grid.py, host half (no GPU).  The GPU tests compare the device with the plain Python decoders of png_util,
tiff_util and webp_util, so those are pinned first: every WebP file against libwebp (Pillow), modes 14 and 15 included, every PNG file
Pillow returns at full precision, every TIFF layout libtiff opens.  Then the host decoders against the references byte for byte on
every file.  (The ASan + UBSan host runs of test_png_cpu, test_tiff_cpu and test_webp_cpu take grid files as further inputs.)

WebP grid 1 is thinned by mode to keep the corpus build short: every mode 0 .. 15 keeps 2 x 66, 64 x 66, 65 x 66, 129 x 66,
65 x 65 and 65 x 129; each of 1 x 66, 3 x 66, 63 x 66, 127 x 66, 128 x 66, 65 x 1, 65 x 2 and 65 x 64 is written for four of the sixteen modes
(recon_grid.WEBP_THINNED).

GIF and BMP: the references are what gif_streams and bmp_streams state for the files they write, pinned against Pillow where Pillow
follows the same rule.  What the grids promise is asserted here, not assumed: the copies of the raw LZW streams from a trace of the rule
(gif_streams.lzw_events), the band walk of the BMP sizes from the kernel's formulas restated (recon_grid.bmp_walk), and that the LZW
files tell a wrong wave copy from a right one (a model of WaveSink::copy and four wrong variants of it).  The BMP grid is thinned by
variant: every variant and row order keeps 1 x 2049, 9 x 683, 1025 x 15 and 8193 x 3; each other size is written for four of the
sixteen variants (recon_grid.BMP_THINNED).  (The ASan + UBSan host runs of test_gif_cpu and test_bmp_cpu take the grid files too.)"""
import io
import os

import numpy as np
import pytest

import bmp_streams as bs
import gif_streams as gs
import recon_grid as rg

# PNG layouts Pillow hands back at the file's full precision (it narrows the other 16-bit layouts to 8 bits): layout -> Pillow mode
PNG_PILLOW = {"gray8": "L", "gray1": "L", "gray2": "L", "gray4": "L", "palette8": "RGB", "graya8": "LA", "rgb8": "RGB", "rgba8": "RGBA", "gray16": "I;16"}
# TIFF layouts (sample layout - byte order) not compared with libtiff: Pillow refuses to open them or hands them back at 8 bits
TIFF_NOT_COMPARED = ["graya16-II", "graya16-MM",  # Pillow cannot identify the file
                     "rgb16-II", "rgb16-MM", "rgba16-II", "rgba16-MM"]  # Pillow opens them as 8-bit RGB / RGBA


def _groups(fmt):
    return list(rg.GRIDS[fmt][0]())


def _open(data):
    Image = pytest.importorskip("PIL.Image")
    im = Image.open(io.BytesIO(data))
    im.load()
    return im


def test_grids_are_seeded_and_hold_the_cases():
    png, tiff, webp = rg.png_grid(), rg.tiff_grid(), rg.webp_grid()
    assert png is rg.png_grid() and tiff is rg.tiff_grid() and webp is rg.webp_grid()  # built once
    names = {n for g in (png, tiff, webp) for files in g.values() for n, _ in files}
    assert sum(len(f) for g in (png, tiff, webp) for f in g.values()) == len(names)
    for layout, _, _ in rg.PNG_LAYOUTS:
        for f in range(5):
            assert {f"{layout}-f{f}-{w}x{h}" for w in rg.PNG_WIDTHS for h in rg.PNG_ROWS} <= names
    assert len(png["pairs"]) == 2 * 2 * 25 and len(png["adam7"]) == 3 * 3 * 8 + 2
    for m in range(16):
        assert {f"mode{m}-{w}x{h}" for w, h in rg.WEBP_KEPT} <= names
    for w, h in rg.WEBP_THINNED:
        assert sum(f"mode{m}-{w}x{h}" in names for m in range(16)) == 4
    for w, h in ((65, 1), (65, 2), (65, 64), (65, 65), (65, 129), (1, 66), (2, 66), (3, 66), (63, 66), (64, 66), (65, 66), (127, 66), (128, 66), (129, 66)):
        assert (w, h) in rg.WEBP_KEPT + rg.WEBP_THINNED  # every size of grid 1 is written for some mode
    slots = rg.webp_slot_counts()  # (read from the kernel's sources: the four cache sizes give four slot counts, all below 7 groups)
    assert len(set(slots.values())) == 4 and slots[0] > slots[9] > slots[10] > slots[11] >= 2 and slots[0] < 7
    assert {n for n, _ in webp["slots"]} == {f"slots-groups{g}-cache{cb}" for g in (4, 7, 9) for cb in slots}
    for n_groups in (4, 7, 9):
        for n_slots in slots.values():
            ent = rg.slot_map(n_groups, n_slots, 90)
            assert set(ent) == set(range(n_groups))
            if n_groups > n_slots:  # groups of one slot follow each other, and come back after the slot has held another
                assert sum(a != b and a % n_slots == b % n_slots for a, b in zip(ent, ent[1:])) >= 3 * (n_groups - n_slots)


@pytest.mark.parametrize("group", _groups("webp"))
def test_webp_reference_equals_libwebp(group):
    for name, data, ref, _ in rg.references("webp", group, hashes=False):
        pil = np.asarray(_open(data))
        assert pil.shape == ref.shape and np.array_equal(pil, ref), name


@pytest.mark.parametrize("group", _groups("png"))
def test_png_reference_equals_pillow_where_pillow_keeps_the_precision(group):
    compared = 0
    for name, data, ref, _ in rg.references("png", group, hashes=False):
        mode = PNG_PILLOW.get(name.split("-")[0])
        if mode is None:
            continue
        im = _open(data)
        if im.mode != mode:
            assert im.mode in ("1", "P") or (mode == "I;16" and im.mode.startswith("I;16")), (name, im.mode)
            if not im.mode.startswith("I;16"):
                im = im.convert(mode)
        got = np.asarray(im)
        assert got.shape == ref.shape and np.array_equal(got.astype(np.int64), ref.astype(np.int64)), name
        compared += 1
    assert compared >= len(rg.png_grid()[group]) // 3


@pytest.mark.parametrize("group", _groups("tiff"))
def test_tiff_reference_equals_libtiff_for_every_layout_it_opens(group):
    for name, data, ref, _ in rg.references("tiff", group, hashes=False):
        if rg.tiff_layout(name) in TIFF_NOT_COMPARED:
            try:  # (the list holds only what Pillow cannot open or narrows)
                assert np.asarray(_open(data)).dtype.itemsize < ref.dtype.itemsize, name
            except OSError:
                pass
            continue
        im = _open(data)
        got = np.asarray(im.convert("L") if im.mode == "1" else im)
        assert got.dtype.itemsize == ref.dtype.itemsize, (name, im.mode)
        assert got.shape == ref.shape and np.array_equal(got.astype(np.int64), ref.astype(np.int64)), (name, im.mode)


def test_tiff_not_compared_list_is_short_and_named():
    layouts = {rg.tiff_layout(n) for files in rg.tiff_grid().values() for n, _ in files}
    assert set(TIFF_NOT_COMPARED) <= layouts
    for must in ("gray8", "rgb8", "rgba8", "gray16"):
        for bo in ("II", "MM"):
            assert f"{must}-{bo}" in layouts and f"{must}-{bo}" not in TIFF_NOT_COMPARED


# ------------------------------------------------------------------ GIF and BMP
def _gif_names():
    return {n for files in rg.gif_grid().values() for n, _ in files}


def test_gif_and_bmp_grids_are_seeded_and_hold_the_cases():
    gif, bmp = rg.gif_grid(), rg.bmp_grid()
    assert gif is rg.gif_grid() and bmp is rg.bmp_grid()  # built once
    for grid in (gif, bmp):
        assert sum(len(f) for f in grid.values()) == len({n for files in grid.values() for n, _ in files})
    assert set(gif) == {"expand_rows", "expand_cols", "lzw_switch", "lzw_copies"} and set(bmp) == {"bands"}
    names = _gif_names()
    # expand_rows: the second trip of a wave's row loop, the frame on the screen, one row down and 1020 rows down
    assert set(rg.GIF_TALL) == {1023, 1024, 1025, 1028, 2047, 2049} and max(rg.GIF_TALL) > 2 * rg.GIF_ROWS_PER_TRIP
    for k, h in enumerate(rg.GIF_TALL):
        w = 5 + k % 5
        for kind in ("plain", "interlaced"):
            assert {f"rows-{kind}-{w}x{h}", f"rows-{kind}-{w}x{h}-opaque"} & names
            assert {f"rows-{kind}-{w}x{h}-fy1", f"rows-{kind}-{w}x{h}-fy1020"} <= names
    for fh in range(1024, 1032):
        assert {f"rows-interlaced-frame5x{fh}-fy0", f"rows-interlaced-frame5x{fh}-fy3"} <= names
    assert gif["expand_rows"][0][0] == rg.GIF_SMALL
    # expand_cols: every left edge with every right edge behind it
    for w in (127, 128, 129, 130):
        for fx in (0, 1, 63, 64, 65):
            for right in (63, 64, 65, 128, 129, w + 3):
                assert (f"cols-{w}x6-fx{fx}-right{right}" in names) == (right > fx)
    # lzw_switch: frames on and beside the 16 KiB of LDS, every residue of the last 16-byte store, the smallest frames
    sizes = {}
    for name, _ in gif["lzw_switch"]:
        w, h = map(int, name.split("-")[1].split("x"))
        sizes.setdefault(w * h, set()).add((w, h) + tuple(name.split("-")[2:4]))
    for w, h in ((127, 129), (128, 128), (16384, 1), (1, 16384), (145, 113)):
        assert {(w, h, c, clear) for c in ("c4", "c256") for clear in ("never", "full")} <= sizes[w * h]
    assert 127 * 129 == rg.GIF_LDS_FRAME - 1 and 145 * 113 == rg.GIF_LDS_FRAME + 1
    assert set(range(16369, 16386)) | set(range(1, 34)) == set(sizes)
    assert {n % 16 for n in sizes if 16369 <= n <= 16384} == set(range(16))
    for key in ("c4", "c256", "never", "full"):
        assert sum(key in s[2:] for n in sizes if n < 16383 for s in sizes[n]) >= 10
    # BMP: the kept sizes for every variant and row order, every other size for four variants that between them are all sixteen
    names = {n for n, _ in bmp["bands"]}
    orders = lambda v: [False] if v.startswith("rle") else [False, True]
    for v in bs.VARIANTS:
        for w, h in rg.BMP_KEPT:
            assert {rg.bmp_name(v, td, w, h) for td in orders(v)} <= names
    assert set(rg.BMP_KEPT) == {(1, 2049), (9, 683), (1025, 15), (8193, 3)}
    assert set(rg.BMP_THINNED) == {(4, 2048), (5, 1025), (10, 1365), (17, 410), (25, 293), (1021, 9), (1024, 8), (8192, 3)}
    thinned = set()
    for w, h in rg.BMP_THINNED:
        has = [v for v in bs.VARIANTS if rg.bmp_name(v, False, w, h) in names]
        assert len(has) == 4 and all(rg.bmp_name(v, True, w, h) in names for v in has if not v.startswith("rle"))
        thinned |= set(has)
    assert thinned == set(bs.VARIANTS)


def test_gif_files_show_every_branch_of_the_pixel_rule():
    """every file but the opaque ones (what Pillow is asked about) has indices past the palette, the transparent index and indices on
    both sides of it inside the screen"""
    for group, files in rg.gif_grid().items():
        for name, data, ref, _ in rg.references("gif", group, hashes=False):
            px = ref.reshape(-1, 4)
            if name.endswith("-opaque"):
                assert (px[:, 3] == 255).all(), name
            elif len(px) >= 1000 and "fy1020" not in name:  # opaque, transparent with the palette's colour, past the palette
                assert (px[:, 3] == 255).any() and ((px[:, 3] == 0) & px[:, :3].any(axis=1)).any() and not px[px[:, 3] == 0].all(axis=0).any(), name
                assert (~px.any(axis=1)).any(), name


def _copy_files():
    """(name, m, frame bytes, joined stream, events, the rule's indices) of the lzw_copies group"""
    out = []
    for name, data in rg.gif_grid()["lzw_copies"]:
        m, (fw, fh), stream = gs.frame_stream(data)
        out.append((name, m, fw * fh, stream, gs.lzw_events(stream, m, fw * fh), gs.lzw_decode(stream, m, fw * fh)))
    return out


def test_lzw_events_trace_the_rule():
    """the trace and lzw_decode are two statements of one rule: replaying the trace's copies byte by byte gives lzw_decode's indices,
    on the grid's raw streams and on encoder-written streams with and without Clears; a refused stream is refused by both"""
    cases = [(m, n, stream, ref) for _, m, n, stream, _, ref in _copy_files()]
    rng = np.random.default_rng(5)
    for m, clear in ((2, "never"), (8, "full"), (4, 50)):
        idx = rng.integers(0, 1 << m, 9000)
        stream = gs.pack_codes(gs.lzw_encode(idx, m, clear), m)
        cases.append((m, 9000, stream, gs.lzw_decode(stream, m, 9000)))
        assert np.array_equal(cases[-1][3], idx)
    for m, n, stream, ref in cases:
        out = np.zeros(n, np.uint8)
        pos = 0
        for kind, at, src, length, written, distinct, clipped in gs.lzw_events(stream, m, n):
            assert at == pos and written == min(length, n - at) and clipped == (length > written)
            assert (kind == "literal") == (src is None) and (kind != "literal" or length == 1)
            if src is None:
                out[at] = ref[at]
            else:
                assert src + (length if kind == "copy" else length - 1) <= at
                for i in range(written):
                    out[at + i] = out[src + i]
            assert distinct == len(set(out[at:at + written].tolist()))
            pos += written
        assert pos == n and np.array_equal(out, ref)
    for codes, n in (([4, 0, 7, 0, 0, 0, 0, 0, 0], 8), ([4, 0, 1, 2, 5], 4), ([6, 0, 1, 2], 4), ([4, 0, 1], 8)):
        assert gs.lzw_events(gs.pack_codes(codes, 2), 2, n) is None and gs.lzw_decode(gs.pack_codes(codes, 2), 2, n) is None


def test_lzw_copies_hold_the_copies_they_promise():
    """from the trace: KwKwK and plain copies of 63, 64, 65, 127, 128 and 129 bytes with at least 8 different bytes each, in a frame the
    kernel builds in LDS and in one it builds in global memory; last strings clipped by the frame's end with 1, 63, 64 and 65 bytes
    left over, of both kinds and in both forms; joined streams of every length modulo 4 (the bit reader's byte-wise tail)"""
    seen, clipped, clips, tails = set(), set(), set(), set()
    for name, m, n, stream, events, _ in _copy_files():
        form = "lds" if n <= rg.GIF_LDS_FRAME else "global"
        assert form in name
        tails.add(len(stream) % 4)
        for kind, at, src, length, written, distinct, clip in events:
            if kind != "literal" and not clip and distinct >= 8:
                seen.add((kind, length, form))
            if clip:
                assert (kind, at + written) == (events[-1][0], n)
                clipped.add((kind, length - written, form))
                clips.add((kind, length, written, form))
    for form in ("lds", "global"):
        for kind in ("copy", "kwkwk"):
            assert {(kind, L, form) for L in rg.GIF_COPY_LENGTHS} <= seen, (kind, form)
            assert {(kind, o, form) for o in rg.GIF_OVERRUNS} <= clipped, (kind, form)
    assert tails == {0, 1, 2, 3}
    assert len([1 for name, *_ in _copy_files() if "-room" in name]) == len(clips)  # every clipped file clips, each differently


def _wave_sink(stream, m, n, ref, step=64, wrap="string", shift=0, stale=0):
    """gif_lzw.h's codes through a model of WaveSink::copy (wave_sink.h): 64 lanes, `step` bytes further per step, every step's reads
    before its writes, out[n + i] = out[from + (dist >= len ? i : i % dist)].  The memory behind the write position holds `stale`: what
    the last user of the LDS or of the slot left there.  wrap: "string" (the kernel's), None (no wrap: i), "step" (the lane's number
    modulo dist, not the byte's); shift: added to the source"""
    out = np.full(n + 512, stale, np.uint8)
    lanes = np.arange(64)
    for kind, at, src, length, written, _, _ in gs.lzw_events(stream, m, n):
        if src is None:
            out[at] = ref[at]
            continue
        dist = at - src
        for base in range(0, written, step):
            i = base + lanes
            i = i[i < written]
            # (the kernel clips the length before it compares it with the distance)
            off = i if dist >= written or wrap is None else (i % dist if wrap == "string" else (i - base) % dist)
            out[at + i] = out[src + shift + off]
    return out[:n]


MUTANTS = dict(no_wrap=dict(wrap=None), step_of_65=dict(step=65), wrap_per_step=dict(wrap="step"), source_shifted_by_one=dict(shift=1))


def test_lzw_copies_tell_a_wrong_copy_from_a_right_one():
    """The gap this group closes, on the CPU: the model of the wave's copy equals the rule on every file; a copy without the wrap, one
    that steps 65 bytes (and leaves one in 65 unwritten), one that wraps the lane's number where the byte's is meant and one that reads
    one byte further each differ on some file, whatever single byte the memory behind the frame holds.  On flat_kwkwk_chain, the only
    file the suite had with copies of these lengths, all four write the right bytes once that memory holds the file's one index (as it
    does after any earlier decode of the file in the same place): a wrong offset reads the same index.  (A step of 63 writes one byte
    of every step twice with the same value: not a wrong copy, nothing could show it.)"""
    files = _copy_files()
    for stale in (0, 1, 255):
        for name, m, n, stream, _, ref in files:
            assert np.array_equal(_wave_sink(stream, m, n, ref, stale=stale), ref), name
            assert np.array_equal(_wave_sink(stream, m, n, ref, step=63, stale=stale), ref), name
        for mutant, kw in MUTANTS.items():
            caught = [name for name, m, n, stream, _, ref in files if not np.array_equal(_wave_sink(stream, m, n, ref, stale=stale, **kw), ref)]
            assert caught, (mutant, stale)
            assert any("lds" in name for name in caught) and any("global" in name for name in caught), (mutant, stale)
    flat = [d for n, d, _ in gs.valid_files() if n == "flat_kwkwk_chain"][0]
    m, (fw, fh), stream = gs.frame_stream(flat)
    ref = gs.lzw_decode(stream, m, fw * fh)
    lengths = {(e[0], e[3]) for e in gs.lzw_events(stream, m, fw * fh)}
    assert {(kind, L) for kind in ("copy", "kwkwk") for L in rg.GIF_COPY_LENGTHS} <= lengths and set(ref.tolist()) == {1}
    assert np.array_equal(_wave_sink(stream, m, fw * fh, ref), ref)
    for mutant, kw in MUTANTS.items():
        assert np.array_equal(_wave_sink(stream, m, fw * fh, ref, stale=1, **kw), ref), mutant


def test_bmp_sizes_walk_the_bands_they_promise():
    """the kernel's own formulas (recon_grid.bmp_walk) at the sizes every variant is written at"""
    walk = {size: rg.bmp_walk(*size) for size in rg.BMP_KEPT + rg.BMP_THINNED}
    table = {(1, 2049): (1, 2048), (4, 2048): (1, 2048), (5, 1025): (2, 1024), (9, 683): (3, 682), (10, 1365): (3, 682), (17, 410): (5, 409), (25, 293): (7, 292),
             (1021, 9): (256, 8), (1024, 8): (256, 8), (1025, 15): (257, 7), (8192, 3): (2048, 1), (8193, 3): (2049, 1)}
    assert {s: (k["G"], k["band"]) for s, k in walk.items()} == table
    a, b, c, d = (walk[s] for s in rg.BMP_KEPT)
    assert a["items"] == [2048, 1] and a["trips"] >= 8 and a["dg"] == 0  # an item of one row behind a full band; eight trips
    assert b["items"] == [682, 1] and (b["dr"], b["dg"]) == (85, 1) and b["carries"] >= 100 and b["trips"] >= 8  # the carry
    assert (c["dr"], c["dg"]) == (0, 256) and c["items"] == [7, 7, 1] and c["carries"] >= 100  # more groups than threads
    assert d["clamped"] and d["band"] == 1 and d["items"] == [1, 1, 1] and not walk[(8192, 3)]["clamped"]  # the clamp
    assert walk[(10, 1365)]["items"] == [682, 682, 1] and walk[(5, 1025)]["dr"] == 128 and walk[(4, 2048)]["items"] == [2048]
    assert walk[(17, 410)]["dg"] == 1 and walk[(25, 293)]["dg"] == 4 and (walk[(1024, 8)]["dr"], walk[(1024, 8)]["dg"]) == (1, 0)
    # the constants restated are the sources'
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "rupphash_amd", "csrc")
    assert f"GROUPS_PER_ITEM = {rg.BMP_GROUPS_PER_ITEM};" in open(os.path.join(csrc, "bmp_host.h")).read()
    kernels = open(os.path.join(csrc, "bmp_kernels.hip")).read()
    assert f"THREADS = {rg.BMP_THREADS};" in kernels and "PX_PER_LANE = 4;" in kernels
    gif = open(os.path.join(csrc, "gif_kernels.hip")).read()
    assert f"LDS_FRAME = {rg.GIF_LDS_FRAME};" in gif and "blocks < 256 ?" in gif and "(max_rows + 3) / 4" in gif


@pytest.mark.parametrize("group", ["expand_rows", "lzw_switch"])
def test_gif_reference_equals_pillow_where_the_frame_is_the_screen_and_opaque(group):
    compared = 0
    for name, data, ref, _ in rg.references("gif", group, hashes=False):
        if name.endswith("-opaque"):
            im = _open(data)
            im.seek(0)
            got = np.asarray(im.convert("RGBA"))
            assert got.shape == ref.shape and np.array_equal(got, ref), name
            compared += 1
    assert compared >= 6


def test_bmp_reference_equals_pillow_for_the_variants_pillow_reads_by_the_rule():
    """the variants of bmp_streams.pillow_exact_files byte for byte (RLE4 apart: Pillow drops the last pixel of an odd absolute run),
    the 16-bit ones of pillow_16_bit_files within 1 (Pillow floors where the rule rounds)"""
    exact, close = ("pal1", "pal4", "pal8", "rgb24", "rgb32", "bf888x", "rle8"), ("rgb16", "bf565", "bf555")
    compared = 0
    for name, data, ref, _ in rg.references("bmp", "bands", hashes=False):
        variant = name.split("-")[0]
        if variant not in exact + close:
            continue
        im = _open(data)
        got = np.asarray(im if im.mode in ("RGB", "RGBA") else im.convert("RGB")).astype(np.int32)
        assert got.shape == ref.shape, name
        if variant in exact:
            assert np.array_equal(got, ref), name
        else:
            assert np.abs(ref - got).max() <= 1 and (ref >= got).all(), name
        compared += 1
    assert compared >= 10 * 2 * len(rg.BMP_KEPT) - len(rg.BMP_KEPT)


@pytest.mark.parametrize("fmt,group", [(fmt, g) for fmt in rg.GRIDS for g in _groups(fmt)])
def test_host_decoder_equals_reference(fmt, group):
    from rupphash_amd import Engine

    host = getattr(Engine, f"{fmt}_decode_host")
    for name, data, ref, _ in rg.references(fmt, group, hashes=False):
        got = host(data)
        assert got.dtype == ref.dtype and got.shape == ref.shape and np.array_equal(got, ref), name
