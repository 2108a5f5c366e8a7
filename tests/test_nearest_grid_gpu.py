"""The nearest-files kernels past one query chunk, one pass of their grids and the small end of the key's file field (-m gpu): what
test_nearest_gpu.py cannot reach with a 256 MiB workspace and segments of 40 files.  rph_debug_nearest_set_workspace makes 33 queries a
second chunk (q0 > 0: the skip, gather and hash indices, the slots, e.j and the counts, the pitch of a short last chunk); 2^20 + 33
queries make one without a knob; 32 CUs + 33 queries in 10 segments loop both bounded grids; segments of 2^20 files put a winner on the
all-ones file field next to distance 256; k = 31 .. 33 and 63 cross the list-length switch; two rows other than row 0 tie; the device
form runs without a counts pointer; a k = 1 call reuses the workspace of a k = 64 call.

Every comparison is nearest_model.same: all n_q x k slots and the counts, exact, against the numpy model.  Queries are random, so
neighbouring tiles and chunks hold different answers.  Every premise is asserted from Engine.nearest_layout, nearest_chunk_queries and
device_info (test_nearest_cpu.py pins the same figures without a device); no test makes a kernel read out of range."""
import numpy as np
import pytest

import library_corpus as lc
import nearest_model as nm
from test_nearest_gpu import FORCED_SEGMENT, SENTINEL, dev_form, host_copy

pytestmark = pytest.mark.gpu

KIB, MIB = 1 << 10, 1 << 20
MAX_SEG = 1 << 20
NO = nm.NO_FILE


@pytest.fixture(scope="module")
def eng():
    from rupphash_amd import Engine

    e = Engine(0)
    yield e
    e.close()


@pytest.fixture
def knobs(request):
    """sets the workspace limit and the forced segment; both are back at their defaults when the test is through"""
    from rupphash_amd import Engine

    def restore():
        Engine.nearest_set_workspace(0)
        Engine.nearest_set_segment(0)

    def set_(workspace=0, segment=0):
        Engine.nearest_set_workspace(workspace)
        Engine.nearest_set_segment(segment)

    request.addfinalizer(restore)
    return set_


def cut(n_lib, nv, n_q, k):
    """(files per segment, segments, queries per chunk) under the knobs in force"""
    from rupphash_amd import Engine

    _, seg, qt, n_segs = Engine.nearest_layout(n_lib, nv, n_q, k)
    assert qt == 32
    return seg, n_segs, Engine.nearest_chunk_queries(n_lib, nv, n_q, k)


def head(want, n_q):
    """the model's answer for the first n_q queries: every query is answered on its own"""
    return want[0][:n_q], want[1][:n_q]


def j_is_the_query(e):
    assert np.array_equal(e["j"], np.broadcast_to(np.arange(len(e), dtype=np.uint32)[:, None], e.shape))  # empty slots included


def slots(e, q, n):
    """(file, distance, variant) of the first n slots of query q"""
    return [(int(x["i"]), int(x["d"]), int(x["flags"]) >> nm.VARIANT_SHIFT) for x in e[q, :n]]


# ---- a. chunk seams under a small workspace ----
# workspace, n_lib, nv, k, segments: test_nearest_cpu.py works these out; 66 and 105 segments give the merge kernel's lanes a second one
CHUNKED = [(64 * KIB, 300, 8, 7, 38), (64 * KIB, 1000, 1, 64, 8), (64 * KIB, 1000, 8, 64, 8), (MIB, 2100, 1, 64, 66), (MIB, 2100, 8, 64, 105)]


@pytest.mark.parametrize("workspace,n_lib,nv,k,n_segs", CHUNKED)
def test_chunk_seams(eng, knobs, workspace, n_lib, nv, k, n_segs):
    knobs(workspace, 8)
    chunk = cut(n_lib, nv, 1, k)[2]
    assert chunk == 32
    n_qs = [chunk - 1, chunk, chunk + 1, 2 * chunk + 5]
    for n_q in n_qs:
        assert cut(n_lib, nv, n_q, k)[1:] == (n_segs, chunk) and n_segs * min(chunk, n_q) * k * 4 <= workspace
    rows, rng = nm.random_library(n_lib, nv, 500 + n_lib + nv)
    hf = (rng.random(n_lib) < 0.7).astype(np.uint8) if nv == 8 else None
    hq = rng.integers(0, 256, (max(n_qs), 32), dtype=np.uint8)
    # every third query of the second and third chunk, and two of the first, is a file's own hash and skips that file: without the
    # skip, or with the skip entry of the same place in another chunk, that file is its best neighbour at distance 0
    skip = np.full(len(hq), NO, np.uint32)
    owners = [3, 20] + list(range(chunk, len(hq), 3))
    skip[owners] = rng.choice(n_lib, len(owners), replace=False)
    hq[owners] = rows[skip[owners], 0]
    unskipped = nm.nearest(rows, hq, k, has_features=hf)
    assert np.array_equal(unskipped[0]["i"][owners, 0], skip[owners]) and (unskipped[0]["d"][owners, 0] == 0).all()
    assert len(set(skip[owners].tolist())) == len(owners) and (skip[:chunk] != skip[chunk:2 * chunk]).any()
    want = nm.nearest(rows, hq, k, has_features=hf, skip=skip)
    assert not (want[0]["i"] == skip[:, None]).any()
    for n_q in n_qs:
        got = eng.hamming_nearest(rows, hq[:n_q], k, has_features=hf, skip=skip[:n_q])
        nm.same(got, head(want, n_q))
        j_is_the_query(got[0])
        status, e, c = dev_form(eng, rows, hq[:n_q], k, has_features=hf, skip=skip[:n_q])
        assert status == 0
        nm.same((e, c), head(want, n_q))
    # a cutoff that about half the slots pass: counts that differ from query to query, and empty slots in every chunk
    max_dist = int(np.median(unskipped[0]["d"][:, k // 2]))
    want = nm.nearest(rows, hq, k, max_dist=max_dist, has_features=hf, skip=skip)
    counts = want[1]
    assert (counts[:chunk] != counts[chunk:2 * chunk]).any() and (counts[:5] != counts[2 * chunk:]).any()  # a count in another chunk's place shows
    assert counts.min() < min(counts.max(), k)
    got = eng.hamming_nearest(rows, hq, k, max_dist=max_dist, has_features=hf, skip=skip)
    nm.same(got, want)
    j_is_the_query(got[0])
    status, e, c = dev_form(eng, rows, hq, k, max_dist=max_dist, has_features=hf, skip=skip)
    assert status == 0
    nm.same((e, c), want)


@pytest.mark.parametrize("n_files,k,n_segs", [(300, 7, 38), (1000, 64, 8)])
def test_chunk_seams_in_the_library_forms(eng, knobs, n_files, k, n_segs):
    f = lc.corpus()
    knobs(64 * KIB, 8)
    twice = np.concatenate([np.arange(n_files - 1), [7]])  # the last file is a true twin of file 7
    rows, hf, hashes = host_copy(f, twice)
    rng = np.random.default_rng(520 + k)
    n_q = 69
    assert cut(n_files, 8, n_q, k)[1:] == (n_segs, 32)
    hq = np.concatenate([f.hashes[rng.integers(0, lc.N_FILES, 40)], rng.integers(0, 256, (n_q - 40, 32), dtype=np.uint8)])[rng.permutation(n_q)]
    want = nm.nearest(rows, hq, k, has_features=hf)
    with eng.library(40) as lib:
        lib.append(f.hashes[twice], f.coeffs[twice], f.has_features[twice], f.quality[twice])
        for n in (31, 32, 33, n_q):
            got = lib.nearest(hq[:n], k)
            nm.same(got, head(want, n))
            j_is_the_query(got[0])
        # resident files as queries: indices in every chunk, file 7 in the second and the third, its twin in the third
        idx = rng.choice(n_files, n_q, replace=False).astype(np.uint32)
        idx[idx == 7] = 8
        idx[idx == n_files - 1] = 9
        idx[[40, 66, 68]] = 7, 7, n_files - 1
        want = nm.nearest(rows, hashes[idx], k, has_features=hf, skip=idx)
        unskipped = nm.nearest(rows, hashes[idx], k, has_features=hf)
        assert (unskipped[0]["d"][:, 0] == 0).all() and (unskipped[0]["i"][[40, 66, 68], 0] == 7).all()  # the skipped file would win
        for n in (33, n_q):
            got = lib.nearest_files(idx[:n], k)
            nm.same(got, head(want, n))
            j_is_the_query(got[0])
        e = got[0]
        assert slots(e, 40, 1) == slots(e, 66, 1) == [(n_files - 1, 0, 0)] and slots(e, 68, 1) == [(7, 0, 0)]
        assert not (e["i"] == idx[:, None]).any()


# ---- b. the chunk limit that needs no knob ----
def test_more_queries_than_one_chunk_takes(eng):
    n_q, k = (1 << 20) + 33, 2
    seg, n_segs, chunk = cut(5, 8, n_q, k)
    assert n_segs == 1 and chunk == 1 << 20 < n_q  # the last 33 queries are a second chunk
    rows, rng = nm.random_library(5, 8, 530)
    hf = np.array([1, 0, 1, 1, 0], np.uint8)
    hq = rng.integers(0, 256, (n_q, 32), dtype=np.uint8)
    skip = np.full(n_q, NO, np.uint32)
    owners = np.concatenate([np.arange(7, 1000, 11), np.arange(chunk - 3, n_q, 2)])  # around the seam and to the end
    skip[owners] = owners % 5
    hq[owners] = rows[skip[owners], 0]
    want = nm.nearest_vectorised(rows, hq, k, has_features=hf, skip=skip)
    assert (want[1] == k).all() and not (want[0]["i"] == skip[:, None]).any()
    spot = np.concatenate([np.arange(0, 40), np.arange(chunk - 40, n_q)])  # the vectorised model against the plain one where it matters most
    nm.same((want[0][spot], want[1][spot]), _rebased(nm.nearest(rows, hq[spot], k, has_features=hf, skip=skip[spot]), spot))
    got = eng.hamming_nearest(rows, hq, k, has_features=hf, skip=skip)
    nm.same(got, want)
    j_is_the_query(got[0])


def _rebased(result, queries):
    """the model's answer for a selection of queries, e.j as in the whole call"""
    e, c = result
    e["j"] = np.asarray(queries, np.uint32)[:, None]
    return e, c


# ---- c. past one pass of both grids in one call ----
@pytest.mark.parametrize("nv,n_lib", [(8, 73), (1, 9 * 32 + 1)])
def test_both_grids_loop(eng, knobs, nv, n_lib):
    knobs(0, 8)
    cus = eng.device_info()[1]
    n_q, k = 32 * cus + 33, 2
    seg, n_segs, chunk = cut(n_lib, nv, n_q, k)
    n_items = n_segs * -(-n_q // 32)
    assert n_segs == 10 and chunk >= n_q       # one chunk: one launch of each kernel
    assert n_items > 8 * cus and n_q > 32 * cus  # more items than the lists kernel has workgroups, more queries than the merge kernel has
    rows, rng = nm.random_library(n_lib, nv, 540 + nv)
    hf = (rng.random(n_lib) < 0.7).astype(np.uint8) if nv == 8 else None
    hq = rng.integers(0, 256, (n_q, 32), dtype=np.uint8)
    skip = np.full(n_q, NO, np.uint32)
    owners = np.arange(5, n_q, 7)
    skip[owners] = rng.integers(0, n_lib, len(owners))
    hq[owners] = rows[skip[owners], 0]
    want = nm.nearest_vectorised(rows, hq, k, has_features=hf, skip=skip)
    spot = np.concatenate([np.arange(0, 40), np.arange(n_q - 70, n_q)])
    nm.same((want[0][spot], want[1][spot]), _rebased(nm.nearest(rows, hq[spot], k, has_features=hf, skip=skip[spot]), spot))
    got = eng.hamming_nearest(rows, hq, k, has_features=hf, skip=skip)
    nm.same(got, want)
    j_is_the_query(got[0])
    # a cutoff that leaves many lists short or empty: an entry that outlives its item would fill them
    max_dist = int(np.median(want[0]["d"][:, 0]))
    want = nm.nearest_vectorised(rows, hq, k, max_dist=max_dist, has_features=hf, skip=skip)
    assert (want[1] == 0).sum() > n_q // 8 and (want[1] == k).sum() > n_q // 8
    nm.same(eng.hamming_nearest(rows, hq, k, max_dist=max_dist, has_features=hf, skip=skip), want)


# ---- d. the key's file field at its end ----
@pytest.mark.parametrize("nv,n_lib", [(1, 2 * MAX_SEG + 40), (8, MAX_SEG + 6)])
def test_file_field_of_the_key_at_its_end(eng, knobs, nv, n_lib):
    knobs(0, MAX_SEG)
    seg, n_segs, _ = cut(n_lib, nv, 3, 7)
    assert seg == MAX_SEG and n_segs == -(-n_lib // MAX_SEG) and n_lib % MAX_SEG != 0  # the last segment is ragged
    rng = np.random.default_rng(550 + nv)
    q = nm.base_hash(41)
    fill = nm.at_distance(q, 200, rng)
    rows = np.ascontiguousarray(np.broadcast_to(fill, (n_lib, nv, 32)))  # every row of every file: 200 from the query
    last = MAX_SEG - 1
    twin = nm.at_distance(q, 10, rng)
    for at, d in ((0, 50), (MAX_SEG // 2 - 1, 40), (MAX_SEG // 2, 30), (last - 1, 20)):
        rows[at, 0] = nm.at_distance(q, d, rng)
    rows[last, nv - 1] = twin  # 8 rows: through variant 7, so its key's low 23 bits are all ones
    rows[MAX_SEG, 0] = twin    # the first file of segment 1: the same distance
    hq = np.stack([q, fill, rng.integers(0, 256, 32, dtype=np.uint8)])
    want = nm.nearest(rows, hq, 7, distances=nm.distances_popcount)
    got = eng.hamming_nearest(rows, hq, 7, max_dist=256)
    v = nv - 1
    planted = [(last, 10, v), (MAX_SEG, 10, 0), (last - 1, 20, 0), (MAX_SEG // 2, 30, 0), (MAX_SEG // 2 - 1, 40, 0), (0, 50, 0)]
    assert slots(got[0], 0, 7) == planted + [(1, 200, 0)]                 # then the ties at 200, the smallest file number first
    # the fill itself: ties at 0 in file order; the planted file 0 is not among them, or is through the first row it has left
    assert slots(got[0], 1, 7) == ([(i, 0, 0) for i in range(1, 8)] if nv == 1 else [(0, 0, 1)] + [(i, 0, 0) for i in range(1, 7)])
    nm.same(got, want)
    # the complement of the fill: every unplanted file at 256, so keys with the top distance bit share the lists with the full file field
    far = nm.complement(fill)[None]
    want = nm.nearest(rows, far, 7, distances=nm.distances_popcount)
    got = eng.hamming_nearest(rows, far, 7, max_dist=256)
    d_last = int(nm.distances_popcount(rows[last][None], far)[0, v, 0])
    assert d_last < 256 and (last, d_last, v) in slots(got[0], 0, 6) and slots(got[0], 0, 7)[6] == (1, 256, 0)
    assert sorted(i for i, _, _ in slots(got[0], 0, 6)) == sorted(i for i, _, _ in planted)
    nm.same(got, want)


# ---- e. the list-length switch at k = 32 | 33 ----
@pytest.mark.parametrize("nv", [1, 8])
@pytest.mark.parametrize("k", [31, 32, 33, 63])
def test_k_either_side_of_the_wave_switch(eng, knobs, nv, k):
    knobs(0, FORCED_SEGMENT)
    from rupphash_amd import Engine

    fb, seg, _, _ = Engine.nearest_layout(10000, nv, 1, k)
    base = nm.base_hash()
    rng = np.random.default_rng(560 + nv + k)
    far = nm.complement(base)
    for hashes in (nm.ladder_descending(600, base), nm.ladder(600, base), nm.ladder_shuffled(600, 5, base)):
        assert cut(600, nv, 3, k)[1] == -(-600 // seg) >= 10
        lib = hashes.reshape(-1, 1, 32) if nv == 1 else nm.with_variants(hashes, far=far)
        hq = np.stack([base, hashes[77], nm.at_distance(base, 40, rng)])
        got = eng.hamming_nearest(lib, hq, k)
        nm.same(got, nm.nearest(lib, hq, k))
        # three files per distance (j, j + 257, j + 514 of the ascending ladder): every list fills, and every later nearer file displaces
        assert got[0]["d"][0].tolist() == [r // 3 for r in range(k)] and got[1][0] == k
    n = 2 * seg + fb + 1  # the seam library: a ragged block behind two whole segments
    rows, rng = nm.random_library(n, nv, 570 + nv + k)
    hf = (rng.random(n) < 0.7).astype(np.uint8) if nv == 8 else None
    hq = rng.integers(0, 256, (35, 32), dtype=np.uint8)
    nm.same(eng.hamming_nearest(rows, hq, k, has_features=hf), nm.nearest(rows, hq, k, has_features=hf))


# ---- f. two rows other than row 0 attain the minimum ----
def test_variant_tie_between_later_rows(eng, knobs):
    knobs(0, FORCED_SEGMENT)
    fb, (seg, _, _) = 4, cut(10000, 8, 1, 7)
    assert seg == FORCED_SEGMENT
    rng = np.random.default_rng(580)
    q = nm.base_hash(51)
    n = 2 * seg + 3  # a ragged last segment of three files
    hashes = np.stack([nm.at_distance(q, 60 + int(rng.integers(0, 90)), rng) for _ in range(n)])
    rows = nm.with_variants(hashes, far=nm.complement(q))
    # files 0 .. 3 of a block (both lane halves, both register groups of each) and the library's last file
    tied = [2 * fb, 2 * fb + 1, 2 * fb + 2, 2 * fb + 3, n - 1]
    for at in tied:
        rows[at, 0] = nm.at_distance(q, 9, rng)
        rows[at, 3] = nm.at_distance(q, 4, rng)
        rows[at, 5] = nm.at_distance(q, 4, rng)  # another hash at the same distance
        assert not np.array_equal(rows[at, 3], rows[at, 5])
    hq = np.stack([q, rng.integers(0, 256, 32, dtype=np.uint8)])
    got = eng.hamming_nearest(rows, hq, 7)
    assert slots(got[0], 0, 5) == [(at, 4, 3) for at in tied]
    nm.same(got, nm.nearest(rows, hq, 7))
    hf = np.ones(n, np.uint8)
    hf[tied] = 0  # ... and kept to their row 0
    got = eng.hamming_nearest(rows, hq, 7, has_features=hf)
    assert slots(got[0], 0, 5) == [(at, 9, 0) for at in tied]
    nm.same(got, nm.nearest(rows, hq, 7, has_features=hf))
    hf[tied[1]] = hf[tied[4]] = 1  # mixed within one block
    got = eng.hamming_nearest(rows, hq, 7, has_features=hf)
    assert slots(got[0], 0, 5) == [(tied[1], 4, 3), (tied[4], 4, 3), (tied[0], 9, 0), (tied[2], 9, 0), (tied[3], 9, 0)]
    nm.same(got, nm.nearest(rows, hq, 7, has_features=hf))


# ---- g. the device form without a counts pointer ----
@pytest.mark.parametrize("nv", [1, 8])
def test_device_form_without_counts(eng, knobs, nv):
    knobs(64 * KIB, 8)
    n_lib, k, n_q = 1000, 64, 69
    assert cut(n_lib, nv, n_q, k)[1:] == (8, 32)  # three chunks: the counts are passed over with q0 > 0 too
    rows, rng = nm.random_library(n_lib, nv, 590 + nv)
    hq = rng.integers(0, 256, (n_q, 32), dtype=np.uint8)
    max_dist = int(np.median(nm.nearest(rows, hq, k)[0]["d"][:, k // 2]))  # about half the slots stay empty
    want = nm.nearest(rows, hq, k, max_dist=max_dist)
    assert 0 < want[1].min() < want[1].max() <= k
    status, e, untouched = dev_form(eng, rows, hq, k, max_dist=max_dist, with_counts=False)
    assert status == 0 and e.tobytes() == want[0].tobytes()
    assert (untouched.view(np.uint8) == SENTINEL).all()  # the buffer allocated next to the slots
    status, e, c = dev_form(eng, rows, hq, k, max_dist=max_dist)
    nm.same((e, c), want)


# ---- h. a call after a longer-listed one on the same context ----
def test_workspace_is_reused_without_leaks(eng, knobs):
    rows, rng = nm.random_library(5000, 1, 600)
    hq = rng.integers(0, 256, (200, 32), dtype=np.uint8)
    few = cut(1000, 1, 33, 64)[1]
    nm.same(eng.hamming_nearest(rows[:1000], hq[:33], 64), nm.nearest(rows[:1000], hq[:33], 64))  # part[few][33][64], all of it keys
    knobs(0, 8)
    many = cut(5000, 1, 200, 1)[1]
    assert many >= 150 > 8 * few and many * 200 > few * 33 * 64  # the second call's lists lie over all of the first call's, and beyond
    uncut = nm.nearest(rows, hq, 1)
    nm.same(eng.hamming_nearest(rows, hq, 1), uncut)
    max_dist = int(np.median(uncut[0]["d"][:, 0])) - 1
    want = nm.nearest(rows, hq, 1, max_dist=max_dist)
    assert 50 < (want[1] == 0).sum() < 200  # empty slots, which a stale key would fill
    nm.same(eng.hamming_nearest(rows, hq, 1, max_dist=max_dist), want)
