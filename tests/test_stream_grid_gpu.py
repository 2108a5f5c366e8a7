"""The streaming PDQ kernels at every width, every height and every flush, strip and band seam (-m gpu): pdq_stream_kernel
(csrc/pdq_stream.hip, one geometry per launch) and pdq_stream_ragged_kernel (csrc/pdq_ragged.hip, a geometry per image) over the sweep
lists of tests/stream_grid.py.  The two kernels carry textually parallel copies of the band loop; both walk every width and height here.

Every comparison is bit equality with the CPU oracle (oracle.pdq_features / to_hash / dihedral_hashes): all 256 coefficients and the
quality as uint32 views of the floats, the hash, the 8 dihedral hashes, `valid`.  Nothing here has a tolerance.  A reference is computed
once per (w, h, kind) and shared by the tests."""
import functools

import numpy as np
import pytest

import stream_grid as sg

pytestmark = pytest.mark.gpu

KEYS = ("hash", "quality", "coeffs", "dihedral", "valid")
SIZES = {"hash": 32, "quality": 4, "coeffs": 1024, "dihedral": 256, "valid": 1}


@pytest.fixture(scope="module")
def eng():
    from rupphash_amd import Engine

    e = Engine(0)
    yield e
    e.set_pdq_kernel(4)
    e.close()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


@functools.lru_cache(maxsize=None)
def reference(w, h, kind):
    """the oracle's (hash, quality, coeffs, dihedral) of sg.image(w, h, kind), or of sg.image_rgb(w, h) for kind "rgb"; read-only"""
    import oracle

    img = sg.image_rgb(w, h) if kind == "rgb" else sg.image(w, h, kind)
    rc, coeffs, q = oracle.pdq_features(img)
    assert rc == 0
    if kind == "b":  # the quality is clamped at 1: only below it does the comparison see the gradient sums (and with them edge[])
        assert 0.0 < q < 1.0, (w, h, q)
    out = (oracle.to_hash(coeffs), np.array([q], np.float32), coeffs, oracle.dihedral_hashes(coeffs))
    for a in out:
        a.setflags(write=False)
    return out


def hold(out, specs, what, skip=()):
    """entry i of the output dict against the oracle's results for specs[i] = (w, h, kind), bit for bit; names geometry and content"""
    assert len(out["hash"]) == len(specs)
    for i, (w, h, kind) in enumerate(specs):
        ref = dict(zip(KEYS, reference(w, h, kind)))
        tag = f"{what}: {w}x{h}, {sg.KIND_NAMES.get(kind, kind)} (image {i})"
        assert out["valid"][i] == 1, f"{tag}: valid = {out['valid'][i]}"
        for key in ("coeffs", "quality", "hash", "dihedral"):
            if key in skip:
                continue
            a, b = bits(out[key][i:i + 1]).reshape(-1), bits(ref[key]).reshape(-1)
            if not np.array_equal(a, b):
                bad = np.flatnonzero(a != b)
                pytest.fail(f"{tag}: {key} differs at {bad.size} of {a.size} places, first {bad[:6].tolist()}")


def same(a, b, specs, what, keys=KEYS):
    for key in keys:
        x, y = bits(a[key]).reshape(len(specs), -1), bits(b[key]).reshape(len(specs), -1)
        if not np.array_equal(x, y):
            bad = np.flatnonzero((x != y).any(axis=1))
            pytest.fail(f"{what}: {key} differs for {[specs[k] for k in bad[:8]]} ({bad.size} of {len(specs)})")


def blank(n):
    return {"hash": np.zeros((n, 32), np.uint8), "quality": np.zeros(n, np.float32), "coeffs": np.zeros((n, 256), np.float32),
            "dihedral": np.zeros((n, 8, 32), np.uint8), "valid": np.zeros(n, np.uint8)}


# ---- the uniform kernel -------------------------------------------------------------------------------------------------------------
_UNIFORM = {}


def uniform(eng, w, h):
    """pdq_stream_kernel on the three contents of (w, h) in one call (once per geometry): the C ABI with rows padded to whole dwords, the
    pad bytes 0xA5 (a packed row of odd width would leave the kernel for the aligned plane).  The caller has set mode 6."""
    from rupphash_amd._lib import check

    if (w, h) not in _UNIFORM:
        n, pitch = len(sg.KINDS), (w + 3) & ~3
        buf = np.full((n, h, pitch), 0xA5, np.uint8)
        for k, kind in enumerate(sg.KINDS):
            buf[k, :, :w] = sg.image(w, h, kind)
        out = blank(n)
        check(eng.L.rph_pdq_hash_batch(eng.ctx, buf.ctypes.data, n, w, h, 1, pitch, pitch * h, *[out[k].ctypes.data for k in KEYS]), "rph_pdq_hash_batch")
        _UNIFORM[(w, h)] = out
    return _UNIFORM[(w, h)]


def uniform_sweep(eng, geoms, what):
    eng.set_pdq_kernel(6)  # the streaming kernel at every batch size
    try:
        for w, h in geoms:
            hold(uniform(eng, w, h), [(w, h, kind) for kind in sg.KINDS], what)
    finally:
        eng.set_pdq_kernel(4)


@pytest.mark.parametrize("win", range(2, 9))
def test_uniform_kernel_every_width_of_a_window(eng, win):
    """PAIRING_A: every width of this window (at most 64), each with its own height, three contents per call"""
    geoms = [(w, h) for w, h in sg.PAIRING_A if sg.axis(w).win == win]
    assert 1 <= len(geoms) <= 64
    uniform_sweep(eng, geoms, f"uniform kernel, window {win}")


# ---- the ragged kernel --------------------------------------------------------------------------------------------------------------
def ragged_dev(eng, images, pitch_align, align=16, quality=True):
    """rph_pdq_hash_ragged_dev on ragged_pack(images): one upload, one call, every output (quality on request); gaps and row padding hold
    0xA5.  Returns (dict, offsets, row strides)."""
    from rupphash_amd.engine import ragged_pack

    n = len(images)
    buf, off, w, h, ch, rs = ragged_pack(images, align=align, pitch_align=pitch_align, fill=0xA5)
    want = {k: (quality or k != "quality") for k in KEYS}
    d_px = eng.dev_alloc(len(buf))
    d = {}
    try:
        for k in KEYS:
            d[k] = eng.dev_alloc(n * SIZES[k]) if want[k] else None
        eng.dev_upload(d_px, buf)
        eng.pdq_hash_ragged_dev(d_px, off, w, h, ch, rs, d["hash"], d["quality"], d["coeffs"], d["dihedral"], d["valid"])
        eng.synchronize()
        out = blank(n)
        for k in KEYS:
            if d[k] is None:
                out[k] = None
            else:
                eng.dev_download(out[k], d[k])
        return out, off, rs
    finally:
        eng.synchronize()
        for p in [d_px] + list(d.values()):
            if p is not None:
                eng.dev_free(p)


_RAGGED_B = {}


def ragged_b_direct(eng):
    """PAIRING_B, content a, read in place (once: three tests compare with it)"""
    if "out" not in _RAGGED_B:
        order = sg.ragged_order(sg.PAIRING_B)
        out, off, rs = ragged_dev(eng, [sg.image(w, h, "a") for w, h in order], pitch_align=4)
        assert all(int(o) % 16 == 0 for o in off) and all(int(r) % 4 == 0 for r in rs)  # what the kernel reads where it lies
        _RAGGED_B["out"] = out
    return _RAGGED_B["out"]


def test_ragged_kernel_pairing_a_in_place_and_the_uniform_kernel_says_the_same(eng):
    """PAIRING_A in one ragged call, every image read in place (rows on dword boundaries, the bytes of other rows and images or 0xA5 to
    the left and right of every row), neighbours of different window: st_image against the oracle, and against the inline band loop of
    pdq_stream_kernel byte for byte"""
    order = sg.ragged_order(sg.PAIRING_A)
    kinds = ("a", "b")  # (b: the content whose quality is below its clamp)
    specs = [(w, h, kind) for kind in kinds for w, h in order]
    out, off, rs = ragged_dev(eng, [sg.image(*s) for s in specs], pitch_align=4)
    assert all(int(o) % 16 == 0 for o in off) and all(int(r) % 4 == 0 for r in rs)
    hold(out, specs, "ragged kernel, PAIRING_A in place")
    eng.set_pdq_kernel(6)
    try:
        uni = [uniform(eng, w, h) for w, h in order]
    finally:
        eng.set_pdq_kernel(4)
    theirs = {key: np.stack([u[key][sg.KINDS.index(kind)] for kind in kinds for u in uni]) for key in KEYS}
    same(out, theirs, specs, "ragged kernel against uniform kernel, PAIRING_A")


def test_ragged_kernel_pairing_b_in_place(eng):
    order = sg.ragged_order(sg.PAIRING_B)
    hold(ragged_b_direct(eng), [(w, h, "a") for w, h in order], "ragged kernel, PAIRING_B in place")


def test_ragged_kernel_pairing_b_through_the_plane(eng):
    """the same images packed without any alignment: rows of odd width on odd addresses go through ragged_luma_kernel into planes with
    16-byte rows first; the results are those of the images read in place"""
    order = sg.ragged_order(sg.PAIRING_B)
    specs = [(w, h, "a") for w, h in order]
    out, off, rs = ragged_dev(eng, [sg.image(*s) for s in specs], pitch_align=1, align=1)
    unaligned = sum((int(o) | int(r)) % 4 != 0 for o, r in zip(off, rs))
    assert unaligned > 300 and any(int(o) % 2 for o in off), unaligned
    hold(out, specs, "ragged kernel, PAIRING_B through the plane")
    same(out, ragged_b_direct(eng), specs, "plane path against the images read in place")


def test_ragged_kernel_pairing_b_without_quality(eng):
    """d_quality absent: the tail's other branch (no gradient sums; edge[] is written and never read)"""
    order = sg.ragged_order(sg.PAIRING_B)
    specs = [(w, h, "a") for w, h in order]
    out, _, _ = ragged_dev(eng, [sg.image(*s) for s in specs], pitch_align=4, quality=False)
    assert out["quality"] is None
    hold(out, specs, "ragged kernel, PAIRING_B without quality", skip=("quality",))
    same(out, ragged_b_direct(eng), specs, "without quality against with it", keys=("hash", "coeffs", "dihedral", "valid"))


# ---- the rare widths against the rare heights ---------------------------------------------------------------------------------------
def test_cross_ragged_kernel(eng):
    """CROSS, the three contents of every geometry, in one ragged call"""
    specs = [(w, h, kind) for w, h in sg.CROSS for kind in sg.KINDS]
    out, _, _ = ragged_dev(eng, [sg.image(*s) for s in specs], pitch_align=4)
    hold(out, specs, "ragged kernel, CROSS")


def test_cross_uniform_kernel_where_a_strip_follows_the_pixels(eng):
    """W = 128, 256, 384, 512 (ns_c = ns_b + 1) against the rare heights, through the uniform kernel"""
    geoms = [(w, h) for w, h in sg.CROSS if sg.one_more_strip(w)]
    assert {w for w, _ in geoms} == {128, 256, 384, 512} and len(geoms) >= 8
    uniform_sweep(eng, geoms, "uniform kernel, CROSS")


def test_cross_colour(eng):
    """CROSS as Rgb8, content a per channel: st_luma_kernel<3> in front of the same geometries"""
    eng.set_pdq_kernel(6)
    try:
        for w, h in sg.CROSS:
            out = eng.pdq_hash_batch(sg.image_rgb(w, h)[None], want_quality=True, want_coeffs=True, want_dihedral=True)
            hold(out, [(w, h, "rgb")], "uniform kernel, Rgb8, CROSS")
    finally:
        eng.set_pdq_kernel(4)
