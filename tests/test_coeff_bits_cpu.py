"""Coefficient bits without a GPU: on every vector of coeff_bits.py the bit-level numpy restatement, the oracle's fast path, the oracle's
naive path and the host scalar PdqFeatures give the same hash and the same eight dihedral rows; and the corpus has the properties
test_coeff_bits_gpu.py relies on."""
import numpy as np
import pytest

import coeff_bits as cb
from rupphash_amd import pdqhash


@pytest.fixture(scope="module")
def hashed(oracle):
    """per vector (hash, dihedral rows) by the oracle's fast path"""
    _, bits = cb.corpus()
    f = bits.view(np.float32)
    return np.stack([oracle.to_hash(c) for c in f]), np.stack([oracle.dihedral_hashes(c) for c in f])


def test_four_host_forms_agree_on_every_vector(oracle, hashed):
    names, bits = cb.corpus()
    for name, b, want_hash, want_dih in zip(names, bits, *hashed):
        c = b.view(np.float32)
        assert np.array_equal(np.ascontiguousarray(c).view(np.uint32), b), name  # the bits reach the callee as they are
        assert np.array_equal(cb.to_hash(b), want_hash), name
        assert np.array_equal(cb.dihedral(b), want_dih), name
        assert np.array_equal(oracle.naive_dihedral(c), want_dih), name
        f = pdqhash.PdqFeatures(c)
        assert np.array_equal(f.to_hash(), want_hash), name
        assert np.array_equal(f.generate_dihedral_hashes(), want_dih), name
        assert np.array_equal(want_dih[0], want_hash), name


def test_keys_order_as_total_cmp_and_invert():
    order = ["-nan-all-ones", "-qnan", "-snan", "-inf", "-max-finite", "-min-normal", "-max-subnormal", "-min-subnormal", "-0", "+0", "+min-subnormal",
             "+max-subnormal", "+min-normal", "+max-finite", "+inf", "+snan", "+qnan", "+nan-all-ones"]
    assert sorted(order) == sorted(cb.SPECIALS)
    keys = [int(cb.key_of(cb.SPECIALS[name])) for name in order]
    assert keys == sorted(keys) and len(set(keys)) == len(keys)
    rng = np.random.default_rng(1)
    b = rng.integers(0, 2**32, 10000, dtype=np.uint64).astype(np.uint32)
    assert np.array_equal(cb.bits_of(cb.key_of(b)), b)
    finite = b[(b & 0x7F800000) != 0x7F800000].view(np.float32)
    finite = finite[finite != 0]
    assert np.array_equal(np.argsort(finite, kind="stable"), np.argsort(cb.key_of(finite.view(np.uint32)), kind="stable"))


def test_every_radix_bit_decides_a_median():
    names, bits = cb.corpus()
    at = {n: k for k, n in enumerate(names)}
    ordinary = 0
    for b in range(32):
        lo, hi = cb.RADIX_A & ~(1 << b), cb.RADIX_A | (1 << b)
        assert lo ^ hi == 1 << b
        even, odd = bits[at[f"radix-bit-{b}-128-128"]], bits[at[f"radix-bit-{b}-127-129"]]
        assert sorted(np.unique(cb.key_of(even)).tolist()) == sorted(np.unique(cb.key_of(odd)).tolist()) == [lo, hi]
        assert (int((cb.key_of(even) == lo).sum()), int((cb.key_of(odd) == lo).sum())) == (128, 127)
        assert int(cb.key_of(cb.median_bits(even))) == lo and int(cb.key_of(cb.median_bits(odd))) == hi  # they differ in bit b alone
        both = cb.bits_of(np.array([lo, hi], np.uint32))
        if ((both & 0x7F800000) != 0x7F800000).all() and ((both & 0x7F800000) != 0).all():
            ordinary += 1
            assert np.unpackbits(cb.to_hash(even)).sum() == 128 and not cb.to_hash(odd).any()
    assert ordinary == 32
    for n_lower, want in ((128, 0x80000000), (127, 0x00000000)):  # -0.0 < +0.0 under total_cmp
        v = bits[at[f"minus-zero-plus-zero-{n_lower}-{256 - n_lower}"]]
        assert int(cb.median_bits(v)) == want and not cb.dihedral(v).any()  # and equal under `>`: no bit is set


def test_rank_boundary_vectors_put_the_tie_where_they_say():
    names, bits = cb.corpus()
    tie_key = int(cb.key_of(np.float32(1.5).view(np.uint32)))
    seen = 0
    for name, b in zip(names, bits):
        if not name.startswith("rank-"):
            continue
        seen += 1
        below, tie = int(name.split("-")[1]), int(name.split("-")[-1])
        k = cb.key_of(b)
        assert (int((k < tie_key).sum()), int((k == tie_key).sum())) == (below, tie)
        assert len(np.unique(k)) == 256 - tie + 1
        in_tie = below <= 127 < below + tie
        assert (int(cb.key_of(cb.median_bits(b))) == tie_key) == in_tie, name
        # bits set: everything strictly above the median
        want = 256 - below - tie if in_tie else 128
        assert np.unpackbits(cb.to_hash(b)).sum() == want, name
    assert seen == 12


def test_adjacent_pairs_are_neighbours_in_the_order():
    names, bits = cb.corpus()
    at = {n: k for k, n in enumerate(names)}
    for name in cb.ADJACENT:
        for n_lower in (127, 128):
            v = bits[at[f"{name}-{n_lower}-{256 - n_lower}"]]
            k = np.unique(cb.key_of(v))
            assert len(k) == 2 and int((cb.key_of(v) == k[0]).sum()) == n_lower
            assert int(k[1]) - int(k[0]) == (0x400000 if "nan" in name else 1), name  # inf to the first quiet NaN: the signalling ones between
            assert int(cb.key_of(cb.median_bits(v))) == int(k[0] if n_lower == 128 else k[1])


def test_specials_nan_medians_and_distinct_dihedral_rows(hashed):
    names, bits = cb.corpus()
    assert len(names) == len(set(names)) == 64 + 18 * 4 + 12 + 66 + 10 + 12
    hashes, dih = hashed
    assert len(cb.SPECIALS) == 18 and all(f"all-{s}" in names for s in cb.SPECIALS)
    for s in cb.SPECIALS.values():
        assert (bits == s).any(axis=1).sum() >= 4
    nan_median = [k for k, b in enumerate(bits) if np.isnan(np.array(cb.median_bits(b), np.uint32).view(np.float32))]
    assert len(nan_median) >= 6
    assert not hashes[nan_median].any()  # `>` against a NaN is false everywhere
    specials_used = [int(n.split("-")[2]) for n in names if n.startswith("normal-with-")]
    assert len(specials_used) == 64 and min(specials_used) == 1 and max(specials_used) == 200
    subnormal = lambda b: ((b & 0x7F800000) == 0) & ((b & 0x007FFFFF) != 0)  # noqa: E731
    n_pos = 0
    for name, b, d in zip(names, bits, dih):
        if name.startswith("positive-distinct"):
            n_pos += 1
            assert not (b >> 31).any() and len(np.unique(b)) == 256
            assert subnormal(b).all() == ("subnormal" in name)
            medians = {int(cb.median_bits(cb.signed(b, nr, nc))) for nr in (False, True) for nc in (False, True)}
            assert len(medians) == 3, name  # the most positive magnitudes allow (coeff_bits.py says why)
            # a flipped pattern's hash is then the pattern itself, and the transposed row pattern is the column pattern: 5 distinct rows
            assert len({bytes(x) for x in d}) == 5 and len({bytes(d[k]) for k in (0, 2, 4, 5, 6)}) == 5, name
    assert n_pos == 12
    assert sum(len({bytes(x) for x in d}) == 8 for d in dih) >= 64  # the full dihedral group elsewhere
    assert len({bytes(h) for h in hashes}) > len(names) // 2
