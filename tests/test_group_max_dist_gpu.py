"""max_dist of every group on the GPU (-m gpu): the kernel of group_info.hip at its run, wave, block and grid seams, its distance
arithmetic, its pivot kinds and default pivots, and the four forms (host, context, device, library) against the numpy restatement of the
rule (group_max_dist_ref.py) and against each other.  Bad indices are only ever refused: no test makes a kernel read out of range."""
import numpy as np
import pytest

import group_max_dist_ref as ref
import library_corpus as lc

pytestmark = pytest.mark.gpu

WAVE, BLOCK = 64, 256
NONE, PER_GROUP, PER_FILE = 0, 1, 2


@pytest.fixture(scope="module")
def eng():
    from rupphash_amd import Engine

    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def files(oracle):
    return lc.corpus()


@pytest.fixture(scope="module")
def G(eng):
    """lanes of one pass of the grid-stride kernels (library_corpus.grid_sizes' convention)"""
    return 8 * eng.device_info()[1] * BLOCK


def dev_form(eng, groups, hashes, pivots=None, rows=None, row_mode=NONE, has_features=None, refuse=False):
    """rph_group_max_dist_dev on uploaded arrays, outputs prefilled with a sentinel: (max_dist, member_dist per group), or with
    refuse=True (status, raw max_dist, raw member_dist) of a call that must fail"""
    from rupphash_amd import Engine, RphError

    members, offsets, ng, piv = Engine._group_lists(groups, pivots)
    hashes = np.ascontiguousarray(hashes, np.uint8).reshape(-1, 32)
    out, md = np.full(max(ng, 1), ref.SENTINEL, np.uint32), np.full(max(len(members), 1), ref.SENTINEL, np.uint32)
    held = []

    def up(a):
        if a is None:
            return None
        a = np.ascontiguousarray(a)
        held.append(eng.dev_alloc(max(a.nbytes, 16)))
        if a.nbytes:
            eng.dev_upload(held[-1], a)
        return held[-1]

    status = 0
    try:
        d_out, d_md = up(out), up(md)
        try:
            eng.group_max_dist_dev(up(hashes), len(hashes), up(members), up(offsets), ng, d_out, d_rows=up(rows), row_mode=row_mode,
                                   d_has_features=up(None if has_features is None else np.asarray(has_features, np.uint8)), d_pivots=up(piv), d_member_dist=d_md)
        except RphError as e:
            status = e.status
        eng.synchronize()
        eng.dev_download(out, d_out)
        eng.dev_download(md, d_md)
    finally:
        for p in held:
            eng.dev_free(p)
    if refuse:
        return status, out, md
    assert status == 0
    return Engine._group_dist_result(out[:ng], md, offsets, ng)


def chain(rng, n):
    """file j = file 0 with j bits flipped: distance |i - j| between files i and j"""
    order = rng.permutation(256)
    base = rng.integers(0, 256, 32, dtype=np.uint8)
    return np.stack([ref.flip(base, order[:j]) for j in range(n)])


def test_run_boundaries_at_every_lane_and_empty_groups(eng):
    """groups of 1, 2, ..., 70 members one behind the other: a run ends at every lane position, runs cross wave and block edges; group
    g's maximum g + 1 sits at a slot that moves, every other member is below it, so a maximum that leaks into a neighbour shows"""
    rng = np.random.default_rng(70)
    hashes = chain(rng, 80)
    groups, want = [[], []], [0, 0]
    for size in range(1, 71):
        top = size + 1
        g = rng.integers(0, top, size).tolist()
        g[(5 * size // 3) % size] = top
        groups.append(g)
        want.append(top)
        if size == 35:
            groups += [[], []]
            want += [0, 0]
    groups.append([])
    want.append(0)
    pivots = [0] * len(groups)  # file 0: in some groups, outside most
    expect = (want, groups)  # file j is at distance j from file 0
    assert ref.restate(groups, hashes, pivots) == expect
    assert dev_form(eng, groups, hashes, pivots) == expect
    assert eng.group_max_dist(groups, hashes, pivots, want_member_dist=True) == expect
    rows = np.repeat(hashes[:, None, :], 8, axis=1)
    assert dev_form(eng, groups, hashes, pivots, rows=rows, row_mode=PER_FILE) == expect
    with eng.library(0) as lib:
        lib.append(hashes)
        assert lib.group_max_dist(groups, pivots, want_member_dist=True) == expect
        assert lib.group_max_dist(groups, want_member_dist=True) == ref.restate(groups, hashes)


def one_far_member(eng, hashes, size, slot, d, rng):
    members = rng.integers(0, len(hashes) - 1, size).astype(np.uint32)
    members[slot] = len(hashes) - 1
    got_max, got_members = dev_form(eng, (members, np.array([0, size], np.uint32)), hashes, [0])
    assert got_max == [d]
    want = np.zeros(size, np.uint32)
    want[slot] = d
    assert np.array_equal(np.array(got_members[0], np.uint32), want)


@pytest.fixture(scope="module")
def same_but_one():
    rng = np.random.default_rng(37)
    base = rng.integers(0, 256, 32, dtype=np.uint8)
    return np.concatenate([np.repeat(base[None, :], 999, axis=0), ref.flip(base, rng.choice(256, 37, replace=False))[None, :]])


@pytest.mark.parametrize("slot", (0, 63, 64, 255, 256, 299))
def test_where_the_maximum_sits_in_one_group(eng, same_but_one, slot):
    one_far_member(eng, same_but_one, 300, slot, 37, np.random.default_rng(slot))


@pytest.mark.parametrize("where", ("G-1", "G", "G+76"))
def test_where_the_maximum_sits_past_one_grid_pass(eng, G, same_but_one, where):
    """a group of G + 77 slots over 1 000 files: the second pass of the grid-stride loop and its ragged last wave"""
    one_far_member(eng, same_but_one, G + 77, {"G-1": G - 1, "G": G, "G+76": G + 76}[where], 37, np.random.default_rng(len(where)))


def test_distance_arithmetic_in_every_dword_and_row(eng):
    """distance 0, distance 256 (no 8-bit truncation), a difference confined to dword k of row v for every k and v"""
    rng = np.random.default_rng(256)
    p = rng.integers(0, 256, 32, dtype=np.uint8)
    rows_p = rng.integers(0, 256, (8, 32), dtype=np.uint8)
    rows_p[0] = p
    hashes, want = [p, p.copy(), ~p], [0, 0, 256]
    for k in range(8):
        hashes.append(ref.flip(p, 32 * k + rng.choice(32, 3 * (k + 1), replace=False)))
        want.append(3 * (k + 1))
    hashes = np.stack(hashes)
    groups = [[m] for m in range(len(hashes))] + [list(range(len(hashes)))]
    pivots = [0] * len(groups)
    expect = (want + [256], [[w] for w in want] + [want])
    assert ref.restate(groups, hashes, pivots) == expect
    assert dev_form(eng, groups, hashes, pivots) == expect
    assert eng.group_max_dist(groups, hashes, pivots, want_member_dist=True) == expect
    # against 8 unrelated rows: member (v, k) differs from row v in dword k alone
    members, want = [p], [0]
    for v in range(8):
        for k in range(8):
            members.append(ref.flip(rows_p[v], 32 * k + rng.choice(32, 1 + (v + k) % 9, replace=False)))
            want.append(1 + (v + k) % 9)
    hashes = np.stack(members)
    groups = [[m] for m in range(len(hashes))] + [list(range(len(hashes)))]
    pivots = [0] * len(groups)
    expect = (want + [9], [[w] for w in want] + [want])
    per_file = np.zeros((len(hashes), 8, 32), np.uint8)
    per_file[0] = rows_p
    assert dev_form(eng, groups, hashes, pivots, rows=per_file, row_mode=PER_FILE) == expect
    assert dev_form(eng, groups, hashes, pivots, rows=np.repeat(rows_p[None], len(groups), axis=0), row_mode=PER_GROUP) == expect


def test_every_dihedral_variant_in_every_row_mode(eng, oracle):
    coeffs, hashes, dih, groups, want = ref.variant_family(oracle)
    pivots = [0] * len(groups)
    expect = ref.restate(groups, hashes, pivots, dih)
    assert expect[0] == want
    assert eng.group_max_dist(groups, hashes, pivots, coeffs=coeffs, want_member_dist=True) == expect
    _, made = eng.pdq_hashes_from_coeffs(coeffs, want_hash=False, want_dihedral=True)
    assert np.array_equal(made, dih)
    assert dev_form(eng, groups, hashes, pivots, rows=made, row_mode=PER_FILE) == expect
    assert dev_form(eng, groups, hashes, pivots, rows=np.repeat(made[:1], len(groups), axis=0), row_mode=PER_GROUP) == expect
    plain = ref.restate(groups, hashes, pivots)
    assert dev_form(eng, groups, hashes, pivots) == plain and all(p > w + 60 for p, w in zip(plain[0][1:], want[1:]))
    with eng.library(0) as lib:
        lib.append(hashes, coeffs=coeffs)
        assert lib.group_max_dist(groups, pivots, want_member_dist=True) == expect


def test_pivot_kinds_in_one_call(eng, oracle):
    """a featured pivot; a featureless pivot whose ignored coefficients would give a smaller distance; no pivot; a pivot outside its group"""
    from rupphash_amd import engine

    rng = np.random.default_rng(4)
    n = 24
    coeffs = rng.normal(0, 30, (n, 256)).astype(np.float32)
    hashes = np.stack([oracle.to_hash(c) for c in coeffs])
    dih = np.stack([oracle.dihedral_hashes(c) for c in coeffs])
    hf = np.ones(n, np.uint8)
    hashes[1] = ref.flip(dih[0][5], [9, 200])          # featured pivot 0: 2 through row 5
    hf[2] = 0
    hashes[2] = rng.integers(0, 256, 32, dtype=np.uint8)  # featureless pivot 2: its hash is unrelated to its coefficients
    hashes[3] = ref.flip(dih[2][3], [17, 80])          # 2 from a row that must not be used
    hashes[7] = ref.flip(dih[6][4], [1])               # pivot 6 is outside its group
    groups = [[0, 1, 4], [2, 3, 5], [8, 9], [7, 10], [11, 12, 13]]
    pivots = [0, 2, None, 6, 12]
    expect = ref.restate(groups, hashes, pivots, dih, hf)
    assert expect[1][0][1] == 2 and expect[1][1][1] > 60 and expect[0][2] == 0 and expect[1][3][0] == 1
    assert ref.restate(groups, hashes, pivots, dih)[1][1][1] == 2  # what reading the ignored row would give
    assert engine.group_max_dist_host(groups, hashes, pivots, coeffs, hf, want_member_dist=True) == expect
    assert eng.group_max_dist(groups, hashes, pivots, coeffs, hf, want_member_dist=True) == expect
    assert dev_form(eng, groups, hashes, pivots, rows=dih, row_mode=PER_FILE, has_features=hf) == expect
    assert dev_form(eng, groups, hashes, pivots, rows=dih[[0, 2, 0, 6, 12]], row_mode=PER_GROUP, has_features=hf) == expect
    with eng.library(0) as lib:
        lib.append(hashes, coeffs=coeffs, has_features=hf)
        assert lib.group_max_dist(groups, pivots, want_member_dist=True) == expect


def test_default_pivots_at_wave_edges(eng, oracle):
    """groups of 130: the first member with features at slot 0, 1, 63, 64, 129, and nowhere; small groups in between move the runs"""
    from rupphash_amd import engine

    rng = np.random.default_rng(130)
    slots = (0, 1, 63, 64, 129, None)
    n = 130 * len(slots) + 10
    coeffs = rng.normal(0, 30, (n, 256)).astype(np.float32)
    hashes = np.stack([oracle.to_hash(c) for c in coeffs])
    dih = np.stack([oracle.dihedral_hashes(c) for c in coeffs])
    hf = np.zeros(n, np.uint8)
    groups = []
    for k, slot in enumerate(slots):
        g = (130 * k + rng.permutation(130)).tolist()
        if slot is not None:
            hf[g[slot]] = 1
            hf[g[min(slot + 7, 129)]] = 1
            hf[g[129]] = 1
            hashes[g[(slot + 1) % 130]] = ref.flip(dih[g[slot]][6], range(k + 1))  # k + 1 from the right pivot's row 6
        groups += [g, [n - 1 - k], []]
    expect = ref.restate(groups, hashes, None, dih, hf)
    assert [expect[1][3 * k][(s + 1) % 130] for k, s in enumerate(slots[:-1])] == [1, 2, 3, 4, 5]
    assert engine.group_max_dist_host(groups, hashes, None, coeffs, hf, want_member_dist=True) == expect
    assert eng.group_max_dist(groups, hashes, None, coeffs, hf, want_member_dist=True) == expect
    assert dev_form(eng, groups, hashes, None, rows=dih, row_mode=PER_FILE, has_features=hf) == expect
    with eng.library(0) as lib:
        lib.append(hashes, coeffs=coeffs, has_features=hf)
        assert lib.group_max_dist(groups, want_member_dist=True) == expect
    # no flags on the device: every file has features, the default is the first listed member
    first = ref.restate(groups, hashes, None, dih, None)
    assert first != expect
    assert dev_form(eng, groups, hashes, None, rows=dih, row_mode=PER_FILE) == first
    assert dev_form(eng, groups, hashes, None) == ref.restate(groups, hashes)
    assert dev_form(eng, groups, hashes, None, has_features=hf) == ref.restate(groups, hashes)  # flags without rows do not count


def fill_library(lib, f, split):
    for first, last in lc.batches(split):
        lib.append(f.hashes[first:last], coeffs=f.coeffs[first:last], has_features=f.has_features[first:last], quality=f.quality[first:last])


@pytest.mark.parametrize("split", (lc.SPLITS[2], lc.SPLITS[4]), ids=("1500-1-400", "1023-1-1-876"))
def test_library_form_on_the_corpus_before_and_after_a_removal(eng, files, split):
    f = files
    with eng.library(40) as lib:
        fill_library(lib, f, split)
        keep = np.arange(lc.N_FILES)
        for round_ in range(2):
            groups = lib.groups()
            assert len(groups) > 40
            before = (len(lib), lib.comparisons, lib.labels().tolist(), groups)
            hashes, dih, hf = f.hashes[keep], f.dih[keep], f.has_features[keep]
            assert lib.group_max_dist(groups, want_member_dist=True) == ref.restate(groups, hashes, None, dih, hf)
            pivots = ref.explicit_pivots(groups, len(keep), seed=round_)
            assert lib.group_max_dist(groups, pivots, want_member_dist=True) == ref.restate(groups, hashes, pivots, dih, hf)
            backwards = [g[::-1] for g in groups[::-1]]  # the caller's order, not the library's
            assert lib.group_max_dist(backwards) == ref.restate(backwards, hashes, None, dih, hf)[0]
            assert (len(lib), lib.comparisons, lib.labels().tolist(), lib.groups()) == before
            if round_ == 0:
                gone = np.random.default_rng(100).choice(lc.N_FILES, 100, replace=False)
                gone[:3] = groups[0][0], groups[1][-1], groups[2][0]
                gone = np.unique(gone)
                lib.remove(gone)
                keep = np.setdiff1d(keep, gone)
                assert len(lib) == len(keep)


def test_every_form_agrees_on_the_corpus(eng, files):
    from rupphash_amd import engine, scanner

    f = files
    groups = ref.corpus_groups()
    pivots = ref.explicit_pivots(groups, lc.N_FILES)
    want = ref.restate(groups, f.hashes, pivots, f.dih, f.has_features)
    assert scanner.group_max_dist(groups, f.hashes, pivots, coefficients=f.coeffs, has_features=f.has_features, engine=eng) == want[0]
    assert scanner.groups_max_dist(groups, f.hashes, pivots, coefficients=f.coeffs, has_features=f.has_features, engine=eng) == want[0]
    assert engine.group_max_dist_host(groups, f.hashes, pivots, f.coeffs, f.has_features, want_member_dist=True) == want
    assert eng.group_max_dist(groups, f.hashes, pivots, f.coeffs, f.has_features, want_member_dist=True) == want
    _, rows = eng.pdq_hashes_from_coeffs(f.coeffs, want_hash=False, want_dihedral=True)
    assert dev_form(eng, groups, f.hashes, pivots, rows=rows, row_mode=PER_FILE, has_features=f.has_features) == want
    with scanner.open_library(40, engine=eng) as lib:
        lib.append(f.hashes, coefficients=f.coeffs, has_features=f.has_features)
        assert lib.group_max_dist(groups, pivots, want_member_dist=True) == want
    # without coefficients every form is the plain distance
    plain = ref.restate(groups, f.hashes, pivots)
    assert scanner.group_max_dist(groups, f.hashes, pivots, engine=eng) == plain[0]
    assert eng.group_max_dist(groups, f.hashes, pivots, want_member_dist=True) == plain == dev_form(eng, groups, f.hashes, pivots)


def test_every_refusal_on_every_form_leaves_the_outputs_untouched(eng, files):
    import ctypes as C

    from rupphash_amd import _lib

    L = _lib.load()
    n = 50
    hashes = np.ascontiguousarray(files.hashes[:n])
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731
    ok_groups, ok_pivots = [[0, 1], [2, 3]], [0, None]
    want = ref.restate(ok_groups, hashes, ok_pivots)
    with eng.library(10) as lib:
        lib.append(hashes)
        state = (len(lib), lib.labels().tolist())
        cases = ref.error_cases(n) + [("null-max-dist", np.array([0, 1, 2, 3], np.uint32), np.array([0, 2, 4], np.uint32), None)]
        for name, members, offsets, pivots in cases:
            ng = len(offsets) - 1
            for form in ("ctx", "library"):
                out, md = np.full(ng, ref.SENTINEL, np.uint32), np.full(len(members), ref.SENTINEL, np.uint32)
                o = None if name == "null-max-dist" else p(out)
                if form == "ctx":
                    rc = L.rph_group_max_dist(eng.ctx, p(hashes), None, None, n, p(members), p(offsets), ng, p(pivots), o, p(md))
                else:
                    rc = L.rph_library_group_max_dist(lib.handle, p(members), p(offsets), ng, p(pivots), o, p(md))
                assert rc == ref.INVALID_ARG, (name, form)
                assert (out == ref.SENTINEL).all() and (md == ref.SENTINEL).all(), (name, form)
            if name != "null-max-dist":
                rc, out, md = dev_form(eng, (members, offsets), hashes, None if pivots is None else pivots.tolist(), refuse=True)
                assert rc == ref.INVALID_ARG, (name, "dev")
                assert (out == ref.SENTINEL).all() and (md == ref.SENTINEL).all(), (name, "dev")
            assert lib.group_max_dist(ok_groups, ok_pivots, want_member_dist=True) == want  # it still answers
        assert (len(lib), lib.labels().tolist()) == state
    # the device form's own arguments: a row mode that is none, rows missing, no output
    d = eng.dev_alloc(4096)
    try:
        for rows, mode, d_out in ((d, 3, d), (None, PER_FILE, d), (d, NONE, None)):
            assert L.rph_group_max_dist_dev(eng.ctx, d, 4, rows, mode, None, d, d, 1, None, d_out, None, None) == ref.INVALID_ARG
        assert L.rph_group_max_dist_dev(eng.ctx, d + 4, 4, None, NONE, None, d, d, 1, None, d, None, None) == ref.INVALID_ARG  # 16-byte alignment
        assert L.rph_group_max_dist_dev(eng.ctx, None, 0, None, NONE, None, None, None, 0, None, None, None, None) == 0
    finally:
        eng.dev_free(d)
