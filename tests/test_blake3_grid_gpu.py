"""The BLAKE3 kernels (csrc/blake3_kernels.hip: b3_plan_kernel, b3_bytes_kernel, b3_fold_kernel, b3_pixels_kernel<1|3|4>,
b3_pixels_ragged_kernel) at their wave, group, fold and grid seams: the case lists of tests/blake3_grid.py (test_blake3_grid_cpu.py holds them
to the seam classes they claim), every digest bit for bit against tests/blake3_util.py.  Device outputs are prefilled with 0xA5, so a digest
that no kernel wrote is seen and named."""
import functools

import numpy as np
import pytest

import blake3_grid as g
import blake3_util as b3
import png_util

pytestmark = pytest.mark.gpu
SENTINEL = 0xA5
KEYS = [None, g.KEY]
KEY_IDS = ["hash", "keyed"]
HELD = [0]  # digests compared with the reference in this module


@pytest.fixture(scope="module")
def eng():
    from rupphash_amd import Engine

    e = Engine(0)
    yield e
    e.close()
    print(f"\ntest_blake3_grid_gpu: {HELD[0]} device digests held to the reference")


def hold(got, want, labels, what):
    """every digest the reference's; names the first that differ and says which of them were never written"""
    got = np.asarray(got)
    assert got.shape == (len(want), 32), what
    HELD[0] += len(want)
    bad = [i for i, w in enumerate(want) if got[i].tobytes() != w]
    if bad:
        unwritten = [labels[i] for i in bad if (got[i] == SENTINEL).all()]
        pytest.fail(f"{what}: {len(bad)} of {len(want)} digests differ, first {[labels[i] for i in bad[:12]]}; never written: {unwritten[:12]}")


def labels_of(lengths):
    return [f"{i}:{x}" for i, x in enumerate(lengths)]


def sentinel_rows(n):
    return np.full((n, 32), SENTINEL, np.uint8)


# ---- byte strings ---------------------------------------------------------------------------------------------------------------------
def blake3_dev(eng, blob, off, key, null_data=False):
    """rph_blake3_batch_dev on the uploaded blob (256-aligned) and offsets; the digests were 0xA5 before the call"""
    n = len(off) - 1
    off = np.ascontiguousarray(off, np.uint64)
    d_data = None if null_data else eng.dev_alloc(max(blob.nbytes, 4))
    d_off, d_dig = eng.dev_alloc(off.nbytes), eng.dev_alloc(32 * n)
    try:
        if not null_data and blob.nbytes:
            eng.dev_upload(d_data, blob)
        eng.dev_upload(d_off, off)
        eng.dev_memset(d_dig, SENTINEL, 32 * n)
        eng.blake3_batch_dev(d_data, d_off, n, d_dig, key)
        eng.stream_synchronize()
        got = np.zeros((n, 32), np.uint8)
        eng.dev_download(got, d_dig)
        return got
    finally:
        eng.synchronize()
        for p in (d_data, d_off, d_dig):
            if p:
                eng.dev_free(p)


def blake3_host(eng, strings, key):
    """rph_blake3_batch into digests that were 0xA5 before the call"""
    from rupphash_amd._lib import check

    n = len(strings)
    out = sentinel_rows(n)
    k = None if key is None else np.frombuffer(bytes(key), np.uint8)
    arr, lens, _keep = eng.jpeg_file_list(strings)
    check(eng.L.rph_blake3_batch(eng.ctx, arr, lens, n, None if k is None else k.ctypes.data, out.ctypes.data), "rph_blake3_batch")
    return out


@functools.lru_cache(maxsize=None)
def in_wave_case():
    blob, off = g.blob_of(g.IN_WAVE_LENGTHS, 1, g.IN_WAVE_START)
    return blob, off, g.strings_of(blob, off)


@pytest.mark.parametrize("key", KEYS, ids=KEY_IDS)
def test_every_in_wave_count_as_root_and_not(eng, key):
    """strings of k chunks and of 64 + k chunks for every k in 1..64, ending on a full chunk, a full block, 63 bytes and 1 byte: the host form,
    and the _dev form from one blob whose first string starts at address 3"""
    blob, off, strings = in_wave_case()
    want = b3.blake3_many(strings, key)
    labels = labels_of(g.IN_WAVE_LENGTHS)
    hold(blake3_host(eng, strings, key), want, labels, "host form")
    hold(blake3_dev(eng, blob, off, key), want, labels, "_dev form")


@pytest.mark.parametrize("key", KEYS, ids=KEY_IDS)
def test_fold_rounds_and_carries(eng, key):
    """strings of 2 .. 257 groups: fold levels of one, two and three rounds of the 64 lanes, the odd node carried in each of them, in-place
    writes of nodes 64 and up"""
    blob, off = g.blob_of(g.FOLD_LENGTHS, 2)
    strings = g.strings_of(blob, off)
    want = b3.blake3_many(strings, key)
    labels = [f"{n} groups" for n in g.FOLD_GROUPS]
    hold(blake3_host(eng, strings, key), want, labels, "host form")
    # the _dev form on the three strings whose levels have two and three rounds, as neighbours of short ones
    pick = [g.FOLD_GROUPS.index(n) for n in (129, 3, 257, 2, 193)]
    lens = [g.FOLD_LENGTHS[i] for i in pick]
    parts = [strings[i] for i in pick]
    sub = np.frombuffer(b"\x5a" + b"".join(parts), np.uint8)
    hold(blake3_dev(eng, sub, np.concatenate([[1], 1 + np.cumsum(lens)]), key), [want[i] for i in pick], [labels[i] for i in pick], "_dev form")


@pytest.mark.parametrize("n", g.PLAN_SIZES)
def test_plan_kernel_thread_and_wave_edges(eng, n):
    """n strings of 0..3 bytes with two-group strings on the edges of the plan kernel's thread ranges and waves"""
    lens = g.plan_lengths(n)
    blob, off = g.blob_of(lens, 3 + n, start=1)
    strings = g.strings_of(blob, off)
    for key in KEYS:
        want = b3.blake3_many(strings, key)
        hold(blake3_dev(eng, blob, off, key), want, labels_of(lens), f"_dev form, n = {n}, {'keyed' if key else 'hash'}")
        hold(blake3_host(eng, strings, key), want, labels_of(lens), f"host form, n = {n}, {'keyed' if key else 'hash'}")


@pytest.mark.parametrize("key", KEYS, ids=KEY_IDS)
def test_second_pass_of_the_grid_stride_loop(eng, key):
    """compute units * 64 + 64 + 3 strings: more groups than the launch has waves, a three-group string across the pass"""
    cus = eng.device_info()[1]
    lens = g.grid_pass_lengths(cus)
    wit = g.byte_classes(lens, cus)
    assert wit.get("string straddling the grid pass") and wit.get("group in the second grid pass"), cus
    blob, off = g.blob_of(lens, 4)
    want = b3.blake3_many(g.strings_of(blob, off), key)
    hold(blake3_dev(eng, blob, off, key), want, labels_of(lens), f"_dev form, {cus} compute units")


@pytest.mark.parametrize("n", [1, 5, 1025])
def test_all_strings_empty_and_no_data_pointer(eng, n):
    off = np.full(n + 1, 12345, np.uint64)
    for key in KEYS:
        hold(blake3_dev(eng, np.zeros(0, np.uint8), off, key, null_data=True), [b3.blake3(b"", key)] * n, labels_of([0] * n), f"n = {n}")


# ---- uniform pixel hashes -------------------------------------------------------------------------------------------------------------
def uniform_both(eng, imgs, lead):
    """rph_pixel_hash_batch on the embedded images where they lie (padded rows, a gap between images) and rph_pixel_hash_batch_dev on the
    same bytes `lead` bytes into a device allocation"""
    from rupphash_amd._lib import check

    n, h, w = imgs.shape[:3]
    ch = 1 if imgs.ndim == 3 else imgs.shape[3]
    buf, rs, st = g.embed_uniform(imgs, lead)
    host = sentinel_rows(n)
    check(eng.L.rph_pixel_hash_batch(eng.ctx, buf[lead:].ctypes.data, n, w, h, ch, rs, st, host.ctypes.data), "rph_pixel_hash_batch")
    d_px, d_h = eng.dev_alloc(buf.nbytes), eng.dev_alloc(32 * n)
    try:
        eng.dev_upload(d_px, buf)
        eng.dev_memset(d_h, SENTINEL, 32 * n)
        eng.pixel_hash_batch_dev(d_px + lead, n, w, h, ch, d_h, row_stride=rs, image_stride=st)
        eng.stream_synchronize()
        dev = np.zeros((n, 32), np.uint8)
        eng.dev_download(dev, d_h)
    finally:
        eng.synchronize()
        eng.dev_free(d_px)
        eng.dev_free(d_h)
    return host, dev


def uniform_list(eng, ch, cases, what):
    """cases: (n, w, h); all references from one blake3_many"""
    sets = [g.uniform_images(w, h, ch, n) for n, w, h in cases]
    want = b3.blake3_many([b3.rgba16_bytes(im) for imgs in sets for im in imgs])
    at = 0
    for k, ((n, w, h), imgs) in enumerate(zip(cases, sets)):
        host, dev = uniform_both(eng, imgs, 1 + k % 4)
        labels = [f"{w}x{h}x{ch} image {i} of {n}" for i in range(n)]
        hold(host, want[at:at + n], labels, f"{what}, host form")
        hold(dev, want[at:at + n], labels, f"{what}, _dev form at d_px + {1 + k % 4}")
        at += n


@pytest.mark.parametrize("ch", g.UNIFORM_CHANNELS)
def test_uniform_block_classes(eng, ch):
    """fast blocks at every address & 3 and on the row end, blocks across one and several row ends, last blocks of 1..7 pixels, zero areas"""
    uniform_list(eng, ch, [(2, w, h) for w, h in g.BLOCK_GEOS], "block geometries")


@pytest.mark.parametrize("ch", g.UNIFORM_CHANNELS)
def test_uniform_in_wave_counts(eng, ch):
    """1..64 chunks in the image's only wave (ROOT on its last fold) and in the second of two"""
    uniform_list(eng, ch, [(2, w, h) for w, h in g.COUNT_GEOS], "in-wave counts")


@pytest.mark.parametrize("ch", g.UNIFORM_CHANNELS)
def test_uniform_group_edge_and_waves_that_leave_early(eng, ch):
    """8192 against 8193 pixels; n * G mod 4 = 0..3 with one and with three groups per image"""
    uniform_list(eng, ch, [(3, w, h) for w, h in g.EDGE_GEOS] + g.NG_CASES, "8192 / 8193 pixels and n * G mod 4")


@pytest.mark.parametrize("ch", g.UNIFORM_CHANNELS)
def test_uniform_129_and_257_groups_per_image(eng, ch):
    uniform_list(eng, ch, [(2, w, h) for w, h in g.BIG_GEOS], "129 and 257 groups")


# ---- ragged pixel hashes --------------------------------------------------------------------------------------------------------------
def ragged_dev(eng, buf, offs, specs, strides, d_px=None):
    n = len(specs)
    own = d_px is None
    if own:
        d_px = eng.dev_alloc(buf.nbytes)
    d_h = eng.dev_alloc(32 * n)
    try:
        if own:
            eng.dev_upload(d_px, buf)
        eng.dev_memset(d_h, SENTINEL, 32 * n)
        eng.image_hash_ragged_dev(d_px, offs, [s[1] for s in specs], [s[2] for s in specs], [s[0] for s in specs], strides, d_pixel_hash=d_h)
        eng.synchronize()
        got = np.zeros((n, 32), np.uint8)
        eng.dev_download(got, d_h)
        return got
    finally:
        eng.synchronize()
        if own:
            eng.dev_free(d_px)
        eng.dev_free(d_h)


def ragged_both(eng, specs, what):
    buf, views, offs, strides = g.embed_ragged(specs)
    want = b3.blake3_many([png_util.to_rgba16(v) for v in views])
    labels = [f"{i}: layout {lay} {w}x{h} at {o}" for i, ((lay, w, h, *_), o) in enumerate(zip(specs, offs))]
    assert all(o % 2 == 0 for (lay, *_), o in zip(specs, offs) if lay > 16)
    host = eng.image_hash_ragged(views, want_pdq=False)
    assert host["hash"] is None
    hold(host["pixel_hash"], want, labels, f"{what}, host form")
    hold(ragged_dev(eng, buf, offs, specs, strides), want, labels, f"{what}, _dev form")


def test_ragged_block_classes_all_layouts_in_one_call(eng):
    ragged_both(eng, g.ragged_block_specs(), "block geometries")


def test_ragged_in_wave_counts_all_layouts_in_one_call(eng):
    ragged_both(eng, g.ragged_count_specs(), "in-wave counts")


def test_ragged_one_two_and_more_than_128_groups_as_neighbours(eng):
    ragged_both(eng, g.RAGGED_BIG_SPECS, "1, 129, 2, 1, 257, 3 and 1 groups")


# ---- 4 GiB ----------------------------------------------------------------------------------------------------------------------------
FAR = 1 << 32


def test_addresses_at_and_beyond_4_gib(eng):
    """One allocation of 2^32 + 1 MiB, zeroed; only the bytes that are read are uploaded.  An address cut to 32 bits reads the zeros (or
    other bytes) at the front of the allocation and shows as a wrong digest."""
    nbytes = FAR + (1 << 20)
    base = eng.dev_alloc(nbytes)
    aux = None
    try:
        eng.dev_memset(base, 0, nbytes)
        eng.synchronize()
        # byte strings: the first straddles 2^32, the second and the third (two groups) start above it
        start, lens = FAR - 70_000, [80_000, 100, 70_000, 0, 5]
        off = np.concatenate([[start], start + np.cumsum(lens)]).astype(np.uint64)
        assert off[0] < FAR < off[1] and g.groups_of(lens[2]) == 2
        blob = np.random.default_rng(40).integers(0, 256, sum(lens), dtype=np.uint8)
        strings = g.strings_of(blob, off - np.uint64(start))
        n = len(lens)
        aux = eng.dev_alloc(4096)
        eng.dev_upload(base + start, blob)
        eng.dev_upload(aux, off)
        for key in KEYS:
            eng.dev_memset(aux + 1024, SENTINEL, 32 * n)
            eng.blake3_batch_dev(base, aux, n, aux + 1024, key)
            eng.stream_synchronize()
            got = np.zeros((n, 32), np.uint8)
            eng.dev_download(got, aux + 1024)
            hold(got, b3.blake3_many(strings, key), labels_of(lens), f"rph_blake3_batch_dev from offsets[0] = 2^32 - 70000, {'keyed' if key else 'hash'}")
        # two Rgb8 images of two groups, 2^32 + 12 bytes apart
        w, h, ch = 100, 90, 3
        imgs = g.uniform_images(w, h, ch, 2, seed=41)
        rs = w * ch + 1
        rows = np.full((2, h, rs), SENTINEL, np.uint8)
        rows[:, :, :w * ch] = imgs.reshape(2, h, w * ch)
        d_px, stride = base + 200_001, FAR + 12
        for i in range(2):
            eng.dev_upload(d_px + i * stride, rows[i])
        eng.dev_memset(aux, SENTINEL, 64)
        eng.pixel_hash_batch_dev(d_px, 2, w, h, ch, aux, row_stride=rs, image_stride=stride)
        eng.stream_synchronize()
        got = np.zeros((2, 32), np.uint8)
        eng.dev_download(got, aux)
        hold(got, [b3.pixel_hash(im) for im in imgs], ["image 0", "image at d_px + 2^32 + 12"], "rph_pixel_hash_batch_dev")
        # ragged: one image below 2^32, one across it, two above it (one of them 16-bit, one of two groups)
        specs = [(3, 43, 30), (4, 40, 30), (18, 9, 15), (1, 100, 90)]
        offs = [300_001, FAR - 1000, FAR + 300_002, FAR + 400_003]
        strides = [43 * 3 + 2, 40 * 4 + 1, 9 * 4 + 2, 101]
        want = []
        for (lay, w, h), o, st in zip(specs, offs, strides):
            im = g.ragged_image(lay, w, h, 42)
            _, bps, bpp = g.layout_bytes(lay)
            rows = np.full((h, st), SENTINEL, np.uint8)
            rows[:, :w * bpp] = np.ascontiguousarray(im).view(np.uint8).reshape(h, w * bpp)
            eng.dev_upload(base + o, rows)
            want.append(b3.blake3(png_util.to_rgba16(im)))
        assert offs[1] < FAR < offs[1] + strides[1] * 30
        hold(ragged_dev(eng, None, offs, specs, strides, d_px=base), want, [f"layout {s[0]} at {o}" for s, o in zip(specs, offs)], "rph_image_hash_ragged_dev")
    finally:
        eng.synchronize()
        eng.dev_free(base)
        if aux:
            eng.dev_free(aux)


# ---- two caller streams ---------------------------------------------------------------------------------------------------------------
def test_blake3_batch_dev_on_two_caller_streams():
    """The plan table and the group values of a call lie in one scratch per context, shared by every caller stream.  On a fresh context the
    second call needs more of it (more strings and more groups), so it grows while the other stream may still be using it."""
    from rupphash_amd import Engine

    eng = Engine(0)
    rng = np.random.default_rng(50)
    lens = [[5, 70_000, 1024, 0, 200_000], rng.integers(0, 5000, 600).tolist() + [3 * g.GROUP_BYTES + 5, 131 * g.GROUP_BYTES - 7, 0, 65_537]]
    keys = [None, g.KEY]
    blobs = [g.blob_of(x, 51 + k, start=k) for k, x in enumerate(lens)]
    want = [b3.blake3_many(g.strings_of(*blobs[k]), keys[k]) for k in range(2)]
    streams = [eng.stream_create(), eng.stream_create()]
    d_data = [eng.dev_alloc(b.nbytes) for b, _ in blobs]
    d_off = [eng.dev_alloc(o.nbytes) for _, o in blobs]
    d_dig = [eng.dev_alloc(32 * len(x)) for x in lens]
    try:
        for k in range(2):
            eng.dev_upload(d_data[k], blobs[k][0])
            eng.dev_upload(d_off[k], blobs[k][1])
            eng.dev_memset(d_dig[k], SENTINEL, 32 * len(lens[k]))
        eng.synchronize()
        for rep in range(20):  # no host synchronisation between the calls beyond the call's own read of its two end offsets
            for k in range(2):
                eng.blake3_batch_dev(d_data[k], d_off[k], len(lens[k]), d_dig[k], keys[k], stream=streams[k])
        for st in streams:
            eng.stream_synchronize(st)
        for k in range(2):
            got = np.zeros((len(lens[k]), 32), np.uint8)
            eng.dev_download(got, d_dig[k])
            hold(got, want[k], labels_of(lens[k]), f"stream {k}")
    finally:
        eng.synchronize()
        for p in d_data + d_off + d_dig:
            eng.dev_free(p)
        for st in streams:
            eng.stream_destroy(st)
        eng.close()
