"""rph_group_max_dist_host (no device) against the numpy restatement of its rule (group_max_dist_ref.py), its refusals, and the C++
mirror's scanner::groups_max_dist_host."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import group_max_dist_ref as ref
import library_corpus as lc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def files(oracle):
    return lc.corpus()


def host(groups, hashes, pivots=None, coeffs=None, has_features=None):
    from rupphash_amd import engine

    return engine.group_max_dist_host(groups, hashes, pivots, coeffs, has_features, want_member_dist=True)


@pytest.mark.parametrize("with_coeffs", (True, False), ids=("coefficients", "no-coefficients"))
@pytest.mark.parametrize("explicit", (True, False), ids=("explicit-pivots", "default-pivots"))
def test_host_form_equals_the_restatement_on_the_corpus(oracle, files, explicit, with_coeffs):
    groups = ref.corpus_groups()
    assert len(groups) > 40 and max(map(len, groups)) > 3
    pivots = ref.explicit_pivots(groups, lc.N_FILES) if explicit else None
    kw = dict(coeffs=files.coeffs, has_features=files.has_features) if with_coeffs else {}
    want = ref.restate(groups, files.hashes, pivots, files.dih if with_coeffs else None, files.has_features if with_coeffs else None)
    assert host(groups, files.hashes, pivots, **kw) == want
    if with_coeffs and not explicit:  # has_features NULL: every file has features, the bridge files' unrelated coefficients included
        dih = files.dih.copy()
        for i in lc.BRIDGE.values():
            dih[i] = oracle.dihedral_hashes(files.coeffs[i])
        assert host(groups, files.hashes, None, coeffs=files.coeffs) == ref.restate(groups, files.hashes, None, dih, None)


def test_groups_in_the_callers_order_with_repeats_singles_and_empties(files):
    groups = [[7, 3, 7, 7], [5], [], [1900, 0, 200], []]
    for pivots in (None, [3, 9, 4, None, 1]):
        want = ref.restate(groups, files.hashes, pivots, files.dih, files.has_features)
        assert host(groups, files.hashes, pivots, coeffs=files.coeffs, has_features=files.has_features) == want
        assert want[0][2] == 0 and want[1][2] == [] and want[0][4] == 0


def test_every_dihedral_variant_is_found_and_the_plain_distance_is_larger(oracle):
    coeffs, hashes, dih, groups, want = ref.variant_family(oracle)
    pivots = [0] * len(groups)
    got, members = host(groups, hashes, pivots, coeffs=coeffs)
    assert got == want == ref.restate(groups, hashes, pivots, dih)[0]
    assert members[-1] == [0] + [v + 1 for v in range(8)]
    plain, plain_members = host(groups, hashes, pivots)
    assert (plain, plain_members) == ref.restate(groups, hashes, pivots)
    assert plain[0] == want[0] == 1  # variant 0 is the hash itself
    assert all(p > w + 60 for p, w in zip(plain[1:], want[1:]))
    # the same files, the pivot marked featureless: its coefficients are not looked at
    hf = np.ones(len(hashes), np.uint8)
    hf[0] = 0
    assert host(groups, hashes, pivots, coeffs=coeffs, has_features=hf)[0] == plain


def raw_host(L, hashes, members, offsets, pivots, coeffs=None, null=()):
    """the C entry point with outputs prefilled: (status, max_dist, member_dist)"""
    p = lambda a, name: None if a is None or name in null else a.ctypes.data_as(C.c_void_p)  # noqa: E731
    out = np.full(max(len(offsets) - 1, 1), ref.SENTINEL, np.uint32)
    md = np.full(max(len(members), 1), ref.SENTINEL, np.uint32)
    rc = L.rph_group_max_dist_host(p(hashes, "hashes"), p(coeffs, "coeffs"), None, len(hashes), p(members, "members"), p(offsets, "offsets"),
                                   len(offsets) - 1, p(pivots, "pivots"), p(out, "max_dist"), md.ctypes.data_as(C.c_void_p))
    return rc, out, md


def test_every_refusal_leaves_the_outputs_untouched(files):
    from rupphash_amd import _lib

    L = _lib.load()
    n = 50
    hashes = np.ascontiguousarray(files.hashes[:n])
    for name, members, offsets, pivots in ref.error_cases(n):
        rc, out, md = raw_host(L, hashes, members, offsets, pivots)
        assert rc == ref.INVALID_ARG, name
        assert (out == ref.SENTINEL).all() and (md == ref.SENTINEL).all(), name
        assert L.rph_last_error()
    ok = (np.array([0, 1, 2, 3], np.uint32), np.array([0, 2, 4], np.uint32), np.array([0, ref.NO_PIVOT], np.uint32))
    for null in ("hashes", "members", "offsets", "max_dist"):
        rc, out, md = raw_host(L, hashes, *ok, null=(null,))
        assert rc == ref.INVALID_ARG, null
        assert (out == ref.SENTINEL).all() and (md == ref.SENTINEL).all(), null
    rc, out, md = raw_host(L, hashes, *ok)
    assert rc == 0 and out.tolist() == ref.restate([[0, 1], [2, 3]], hashes, [0, None])[0] and md[2:].tolist() == [0, 0]
    # no groups: nothing to do, whatever else is passed
    assert L.rph_group_max_dist_host(None, None, None, 0, None, None, 0, None, None, None) == 0


def write_case(path, f, has_hash, groups, pivots):
    with open(path, "wb") as out:
        out.write(struct.pack("<III", len(has_hash), len(groups), pivots is not None))
        for i in range(len(has_hash)):
            out.write(struct.pack("<BB", has_hash[i], f.has_features[i]) + f.hashes[i].tobytes() + f.coeffs[i].astype("<f4").tobytes())
        for g in groups:
            out.write(struct.pack(f"<I{len(g)}I", len(g), *g))
        for p in pivots or ():
            out.write(struct.pack("<q", -1 if p is None else p))


def test_cpp_mirror_host_form(files, tmp_path):
    """scanner::groups_max_dist_host over ScannedFile: files without a hash are skipped, as members and as pivots"""
    exe = str(tmp_path / "group_max_dist_host")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "group_max_dist_host.cpp"),
                           "-o", exe, "-L", os.path.join(ROOT, "rupphash_amd"), "-lrupphash_hip", "-Wl,-rpath," + os.path.join(ROOT, "rupphash_amd"),
                           "-Wl,-rpath,/opt/rocm/lib", "-pthread"])
    n = lc.N_FILES
    groups = ref.corpus_groups() + [[5, 6, 7, 8], [], [9]]
    has_hash = np.ones(n, np.uint8)
    has_hash[[6, 9, groups[0][0], groups[1][-1]]] = 0
    kept = [[m for m in g if has_hash[m]] for g in groups]
    explicit = [p if p is None or has_hash[p] else None for p in ref.explicit_pivots(groups, n)]
    explicit[-3] = 6  # a pivot without a hash is no pivot
    for pivots, dense in ((None, None), (explicit, [p if p is None or has_hash[p] else None for p in explicit])):
        write_case(tmp_path / "case.bin", files, has_hash, groups, pivots)
        r = subprocess.run([exe, str(tmp_path / "case.bin")], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        want = ref.restate(kept, files.hashes, dense, files.dih, files.has_features)[0]
        assert [int(x) for x in r.stdout.split()] == want
