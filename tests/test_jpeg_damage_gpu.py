"""Damaged JPEG streams through rph_jpeg_pdq_hash_batch in every entropy mode: the results (status, valid, hash, quality bit pattern,
coefficients, dihedral hashes, pixel hashes) are byte for byte those of the host decoder, which are those of "oracle decode, then oracle
hash" -- so a damaged file gets the same answer whichever files share its call (include/rupphash.h, rph_jpeg_set_entropy).  The corpus is
tests/jpeg_util.damaged_corpus: one file per rule and layout, and random damage."""
import numpy as np
import pytest

import jpeg_util as ju

pytestmark = pytest.mark.gpu
PIL = pytest.importorskip("PIL")

HOST, DEVICE, AUTO, DEVICE_SEQUENTIAL = 0, 1, 2, 3
KEYS = ("status", "valid", "hash", "quality", "coeffs", "dihedral", "pixel_hash")


@pytest.fixture(scope="module")
def eng():
    from rupphash_amd import Engine

    e = Engine(0)
    yield e
    e.jpeg_set_entropy(AUTO)
    e.jpeg_set_segments()
    e.close()


@pytest.fixture(scope="module")
def corpus():
    return [d for _, d, _ in ju.damaged_corpus()]


@pytest.fixture(scope="module")
def names():
    return [n for n, _, _ in ju.damaged_corpus()]


def _run(eng, files, mode, flavour, pixel_hash=False):
    eng.jpeg_set_entropy(mode)
    try:
        return eng.jpeg_pdq_hash_batch(files, flavour=flavour, threads=4, want_coeffs=True, want_dihedral=True, want_pixel_hash=pixel_hash)
    finally:
        eng.jpeg_set_entropy(AUTO)


def _view(out, key, i):
    v = out[key][i]
    return v.view(np.uint32) if v.dtype == np.float32 else v


def _same(a, b, names, rows_a=None, rows_b=None):
    """rows where outputs a and b differ: [(name, key)]"""
    rows_a = range(len(names)) if rows_a is None else rows_a
    rows_b = rows_a if rows_b is None else rows_b
    bad = []
    for name, i, j in zip(names, rows_a, rows_b):
        for key in KEYS:
            if a.get(key) is None:
                continue
            if not np.array_equal(_view(a, key, i), _view(b, key, j)):
                bad.append((name, key))
                break
    return bad


@pytest.mark.parametrize("flavour", [0, 1])
def test_host_mode_is_oracle_decode_then_oracle_hash(eng, oracle, corpus, names, flavour):
    out = _run(eng, corpus, HOST, flavour)
    bad = []
    for i, data in enumerate(corpus):
        try:
            px = oracle.jpeg_decode(data, flavour)
        except ValueError:
            if out["status"][i] == 0 or out["valid"][i] or out["hash"][i].any() or out["coeffs"][i].any() or out["dihedral"][i].any():
                bad.append((names[i], "oracle refuses"))
            continue
        if out["status"][i] != 0:
            bad.append((names[i], "host refuses"))
            continue
        rc, c, q = oracle.pdq_features(px)
        if bool(out["valid"][i]) != (rc == 0):
            bad.append((names[i], "valid"))
        elif rc == 0 and not (np.array_equal(out["hash"][i], oracle.to_hash(c)) and out["quality"][i].view(np.uint32) == np.float32(q).view(np.uint32)
                              and np.array_equal(out["coeffs"][i].view(np.uint32), np.asarray(c, np.float32).view(np.uint32))
                              and np.array_equal(out["dihedral"][i], oracle.dihedral_hashes(c))):
            bad.append((names[i], "hash"))
    assert not bad, bad


@pytest.mark.parametrize("flavour", [0, 1])
@pytest.mark.parametrize("mode", [DEVICE, DEVICE_SEQUENTIAL, AUTO])
def test_every_entropy_mode_gives_the_host_results(eng, corpus, names, mode, flavour):
    ref = _run(eng, corpus, HOST, flavour)
    got = _run(eng, corpus, mode, flavour)
    assert not _same(ref, got, names)


@pytest.mark.parametrize("seg_bytes", [64, 256, 1024])
def test_segments_give_the_host_results(eng, corpus, names, seg_bytes):
    ref = _run(eng, corpus, HOST, 0)
    eng.jpeg_set_segments(0, seg_bytes)
    try:
        got = _run(eng, corpus, DEVICE, 0)
    finally:
        eng.jpeg_set_segments()
    assert not _same(ref, got, names)


def test_pixel_hashes_of_damaged_files_match_the_host(eng, corpus, names):
    ref = _run(eng, corpus, HOST, 1, pixel_hash=True)
    got = _run(eng, corpus, DEVICE, 1, pixel_hash=True)
    assert not _same(ref, got, names)
    refused = ref["status"] != 0
    assert not ref["pixel_hash"][refused].any()


def _progressive(data):
    sos = data.find(b"\xff\xda")
    return sos > 0 and b"\xff\xc2" in data[:sos]


def test_large_auto_call_mixes_damaged_and_good_files(eng, corpus, names):
    """A call large enough for AUTO to take sequential and progressive files to the device (over several chunks and sub-batches): every
    damaged file keeps its host result, and every good file the result it has in a call of good files alone."""
    rng = np.random.default_rng(31)
    good = [d for _, d in ju._layouts(rng)] + [d for _, d in ju._pillow_layouts(rng, 150, 110)]
    n = 2000
    files, rows, kinds = [], [], []
    for k in range(n):
        if k % 5 == 2:
            files.append(corpus[(k // 5) % len(corpus)])
            kinds.append(("damaged", (k // 5) % len(corpus)))
        else:
            files.append(good[k % len(good)])
            kinds.append(("good", k % len(good)))
        rows.append(k)
    # AUTO's routing (jpeg_pipeline.cpp, run_batch), with the good files alone as the lower bound of what it counts: at least 512 lanes of
    # sequential files, and progressive files whose bytes would keep the 4 host threads (41 MB/s each) busy for longer than the device
    # needs for the longest of them (0.6 us per byte) -- by a margin
    g_files = [files[k] for k in rows if kinds[k][0] == "good"]
    assert sum(not _progressive(d) for d in g_files) >= 512
    prog_bytes = sum(len(d) for d in g_files if _progressive(d))
    assert prog_bytes / (4 * 41e6) > 1.5 * 0.6e-6 * max(len(d) for d in files if _progressive(d))
    clean = _run(eng, good, HOST, 0)
    ref = _run(eng, corpus, HOST, 0)
    got = _run(eng, files, AUTO, 0)
    g_rows = [k for k in rows if kinds[k][0] == "good"]
    d_rows = [k for k in rows if kinds[k][0] == "damaged"]
    assert not _same(clean, got, [f"good{kinds[k][1]}" for k in g_rows], [kinds[k][1] for k in g_rows], g_rows)
    assert not _same(ref, got, [names[kinds[k][1]] for k in d_rows], [kinds[k][1] for k in d_rows], d_rows)
    assert not clean["status"].any()
