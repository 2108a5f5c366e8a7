"""The median of the 256 coefficients (select_rank127, rupphash_amd/csrc/pdq_tail.hpp) is an MSB-first radix select over total_cmp keys
that leaves its loop as soon as a single key still matches the prefix and fetches that key from its lane.  These coefficient vectors
are chosen for where the select stops: early, at the last bit, and never (ties at the median).  `rph_pdq_hashes_from_coeffs` must
return the oracle's hash and its eight dihedral hashes (three more medians over sign-flipped copies) for every one of them.

test_select_model_* run without a GPU: a numpy model of the select as the kernel performs it, checked against the sorted keys, says at
which bit each vector lets go -- so the corpus is known to hold the early, the last-bit and the never case."""
import numpy as np
import pytest

gpu = pytest.mark.gpu


def f32(bits):
    return np.asarray(bits, np.uint32).view(np.float32)


def total_keys(v):
    b = np.ascontiguousarray(v, np.float32).view(np.uint32)
    return b ^ np.where(b >> 31, np.uint32(0xFFFFFFFF), np.uint32(0x80000000))


def select_model(v):
    """(key of rank 127, bit after which a single candidate was left or None) -- the kernel's loop, key for key"""
    key = total_keys(v)
    prefix, mask, k, cand = 0, 0, 127, 256
    for bit in range(31, -1, -1):
        b = 1 << bit
        mask |= b
        cnt = int(np.count_nonzero((key & np.uint32(mask)) == np.uint32(prefix)))
        if k >= cnt:
            k -= cnt
            cand -= cnt
            prefix |= b
        else:
            cand = cnt
        assert 0 <= k < cand
        if cand == 1:
            hit = np.nonzero((key & np.uint32(mask)) == np.uint32(prefix))[0]
            assert len(hit) == 1 and k == 0
            return int(key[hit[0]]), bit
    return prefix, None


def _cases():
    """name -> 256 float32 values, positions shuffled (the dihedral patterns flip signs by position)"""
    rng = np.random.default_rng(20261020)
    out = {}

    def put(name, values):
        v = np.ascontiguousarray(values, np.float32).copy()
        assert v.shape == (256,), name
        out[name] = v[rng.permutation(256)]
        out[name + "/sorted"] = v  # and in the order given: equal values in neighbouring lanes and registers

    put("distinct", rng.standard_normal(256) * 37.0)
    put("distinct-wide", np.ldexp(rng.standard_normal(256), rng.integers(-60, 60, 256)))
    put("distinct-positive", np.abs(rng.standard_normal(256)) + 1.0)
    for c in (1.5, 0.0, -0.0, -7.25):
        put(f"all-equal {c!r}", np.full(256, c, np.float32))
    put("two-values 127/129", np.r_[np.full(127, -3.25), np.full(129, 7.5)])
    put("two-values 129/127", np.r_[np.full(129, -3.25), np.full(127, 7.5)])
    put("two-values 128/128", np.r_[np.full(128, -3.25), np.full(128, 7.5)])
    put("two-positive 127/129", np.r_[np.full(127, 3.25), np.full(129, 7.5)])
    # rank 127 is a -0 / a +0; the zeros are told apart only by the sign bit
    neg = -1.0 - np.arange(100)
    pos = 1.0 + np.arange(100)
    put("zeros: median -0", np.r_[neg, np.full(28, -0.0), np.full(28, 0.0), pos])
    put("zeros: median +0", np.r_[neg, np.full(27, -0.0), np.full(29, 0.0), pos])
    put("zeros: single -0 is the median", np.r_[-1.0 - np.arange(127), [-0.0], np.full(128, 0.0)])
    put("zeros: single +0 is the median", np.r_[np.full(127, -0.0), [0.0], 1.0 + np.arange(128)])
    put("zeros only 127/129", np.r_[np.full(127, -0.0), np.full(129, 0.0)])
    put("zeros only 128/128", np.r_[np.full(128, -0.0), np.full(128, 0.0)])
    # decided at bit 0
    base = np.float32(1.7).view(np.uint32) & np.uint32(0xFFFFFFFE)
    put("low-bit 127/129", f32(np.r_[np.full(127, base), np.full(129, base + 1)]))
    put("low-bit 128/128", f32(np.r_[np.full(128, base), np.full(128, base + 1)]))
    put("low-bit negative 128/128", f32(np.r_[np.full(128, base), np.full(128, base + 1)] | np.uint32(0x80000000)))
    put("low-byte distinct", f32((base & np.uint32(0xFFFFFF00)) + np.arange(256, dtype=np.uint32)))
    put("low-bit pair at the median", np.r_[np.full(127, 1.0), f32([base, base + 1]), np.full(127, 2.0)])
    # the median unique, everything else tied
    put("unique between two ties", np.r_[np.full(127, -2.0), [0.375], np.full(128, 5.0)])
    put("unique between two near ties", f32(np.r_[np.full(127, base - 1), [base], np.full(128, base + 1)]))
    put("unique, ties on one side", np.r_[-1.0 - np.arange(127), [0.375], np.full(128, 5.0)])
    # negative-heavy
    put("negative 200 distinct", np.r_[-np.abs(rng.standard_normal(200)) - 0.5, np.abs(rng.standard_normal(56))])
    put("negative all distinct", -np.abs(rng.standard_normal(256)) - 0.001)
    put("negative ties 127/129", np.r_[np.full(127, -9.0), np.full(129, -4.0)])
    # NaNs of both signs: -NaN sorts below -inf, +NaN above +inf (total_cmp)
    qnan, snan = np.uint32(0x7FC00000), np.uint32(0x7F800001)
    body = rng.standard_normal(256).astype(np.float32).view(np.uint32)
    v = body.copy()
    v[:20] = (qnan + np.arange(20, dtype=np.uint32)) | np.uint32(0x80000000)
    v[20:30] = snan + np.arange(10, dtype=np.uint32)
    put("nan: 20 negative, 10 positive", f32(v))
    v = body.copy()
    v[:130] = qnan + np.arange(130, dtype=np.uint32)
    put("nan: median is a positive NaN", f32(v))
    v = body.copy()
    v[:130] = (snan + np.arange(130, dtype=np.uint32)) | np.uint32(0x80000000)
    put("nan: median is a negative NaN", f32(v))
    put("nan: all the same", f32(np.full(256, qnan)))
    put("inf: 127 -inf, 129 +inf", np.r_[np.full(127, -np.inf), np.full(129, np.inf)])
    return out


@pytest.fixture(scope="module")
def corpus():
    cases = _cases()
    names = list(cases)
    coeffs = np.stack([cases[n] for n in names])
    coeffs.setflags(write=False)
    return names, coeffs


@pytest.fixture(scope="module")
def ref(oracle, corpus):
    """the oracle's hash and dihedral hashes of every vector of the corpus; computed once, read-only"""
    _, coeffs = corpus
    out = (np.stack([oracle.to_hash(c) for c in coeffs]), np.stack([oracle.dihedral_hashes(c) for c in coeffs]))
    for a in out:
        a.setflags(write=False)
    return out


def first_difference(names, got, want):
    bad = np.nonzero((got != want).reshape(len(got), -1).any(axis=1))[0]
    return f"{len(bad)} vectors differ, the first is {names[bad[0] % len(names)]!r}" if len(bad) else ""


# ---------------- without a GPU: the model of the select, and what the corpus covers ----------------
def test_select_model_returns_the_key_of_rank_127(corpus):
    names, coeffs = corpus
    for name, v in zip(names, coeffs):
        got, _ = select_model(v)
        assert got == int(np.sort(total_keys(v))[127]), name


def test_select_model_hash_is_the_oracles(oracle, corpus, ref):
    """v > median with the model's median, packed as the reference packs it (row 15 first, bit 15 of a row first)"""
    names, coeffs = corpus
    for name, v, want in zip(names, coeffs, ref[0]):
        key, _ = select_model(v)
        med = f32([key ^ 0x80000000 if key & 0x80000000 else key ^ 0xFFFFFFFF])[0]
        with np.errstate(invalid="ignore"):
            bit = (v > med).reshape(16, 16)
        rows = (bit * (1 << np.arange(16))).sum(axis=1)
        got = np.array([[rows[r] >> 8, rows[r] & 0xFF] for r in range(15, -1, -1)], np.uint8).reshape(32)
        assert np.array_equal(got, want), name


def test_corpus_stops_early_at_the_last_bit_and_never(corpus):
    names, coeffs = corpus
    stop = {name: select_model(v)[1] for name, v in zip(names, coeffs)}
    assert stop["all-equal 1.5"] is None and stop["two-values 127/129"] is None and stop["zeros: median -0"] is None
    assert stop["nan: all the same"] is None and stop["low-bit 128/128"] is None
    assert stop["low-byte distinct"] == 0 and stop["low-bit pair at the median"] == 0
    # a lone zero next to numbers of magnitude >= 1: the sign bit halves the set, the top exponent bits single the zero out
    assert stop["zeros: single -0 is the median"] >= 28 and stop["zeros: single +0 is the median"] >= 28
    assert stop["unique between two near ties"] in (0, 1)
    assert 8 <= stop["distinct"] <= 30 and 8 <= stop["negative all distinct"] <= 30
    assert stop["unique between two ties"] is not None and stop["unique between two ties"] > 20
    assert stop["nan: median is a positive NaN"] is not None and stop["nan: median is a negative NaN"] is not None
    assert len({s for s in stop.values() if s is not None}) >= 8


# ---------------- on the GPU ----------------
@pytest.fixture(scope="module")
def eng():
    from rupphash_amd import Engine

    e = Engine(0)
    yield e
    e.close()


@gpu
@pytest.mark.parametrize("outputs", ["hash", "dihedral", "both"])
def test_corpus_matches_the_oracle(eng, corpus, ref, outputs):
    names, coeffs = corpus
    hashes, dih = eng.pdq_hashes_from_coeffs(coeffs, want_hash=outputs != "dihedral", want_dihedral=outputs != "hash")
    if hashes is not None:
        assert np.array_equal(hashes, ref[0]), first_difference(names, hashes, ref[0])
    if dih is not None:
        assert np.array_equal(dih, ref[1]), first_difference(names, dih, ref[1])


@gpu
def test_one_vector_per_call(eng, corpus, ref):
    names, coeffs = corpus
    for k in range(len(names)):
        hashes, dih = eng.pdq_hashes_from_coeffs(coeffs[k:k + 1])
        assert np.array_equal(hashes[0], ref[0][k]) and np.array_equal(dih[0], ref[1][k]), names[k]


@gpu
def test_more_vectors_than_the_device_runs_at_once(eng, corpus, ref):
    """the corpus repeated, rolled by one vector per repetition, to a little more than 8 waves on each of 256 CUs (a 2 MB upload)"""
    names, coeffs = corpus
    m = len(names)
    reps = (8 * 256 + 3 * m) // m
    idx = np.concatenate([np.roll(np.arange(m), r) for r in range(reps)])
    assert len(idx) > 8 * 256
    hashes, dih = eng.pdq_hashes_from_coeffs(coeffs[idx])
    assert np.array_equal(hashes, ref[0][idx]), first_difference(names, hashes, ref[0][idx])
    assert np.array_equal(dih, ref[1][idx]), first_difference(names, dih, ref[1][idx])
