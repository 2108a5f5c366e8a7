"""Coefficient bits on the GPU (-m gpu): from_coeffs_kernel on the corpus of coeff_bits.py -- NaNs, infinities, subnormals, signed zeros,
ties at rank 127, one vector pair per bit of the radix select -- bit for bit against the CPU oracle, through the host entry point, the
device entry point on a misaligned buffer, and the two grouping paths that hash stored coefficients on the device."""
import numpy as np
import pytest

import coeff_bits as cb

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from rupphash_amd import Engine

    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def ref(oracle):
    """(coefficients, hashes, dihedral rows) of the corpus by the oracle; computed once, read-only"""
    _, bits = cb.corpus()
    coeffs = bits.view(np.float32)
    out = (coeffs, np.stack([oracle.to_hash(c) for c in coeffs]), np.stack([oracle.dihedral_hashes(c) for c in coeffs]))
    for a in out[1:]:
        a.setflags(write=False)
    return out


def first_difference(names, got, want):
    bad = np.nonzero((got != want).reshape(len(got), -1).any(axis=1))[0]
    return f"{len(bad)} vectors differ, the first is {names[bad[0]]}" if len(bad) else ""


@pytest.mark.parametrize("outputs", ["hash", "dihedral", "both"])
@pytest.mark.parametrize("count", [1, 63, 64, 65, None], ids=lambda c: "all" if c is None else str(c))
def test_hashes_from_coeffs_match_the_oracle_bit_for_bit(eng, ref, count, outputs):
    names, _ = cb.corpus()
    coeffs, want_hash, want_dih = (a[:count] for a in ref)
    hashes, dih = eng.pdq_hashes_from_coeffs(coeffs, want_hash=outputs != "dihedral", want_dihedral=outputs != "hash")
    assert (hashes is None) == (outputs == "dihedral") and (dih is None) == (outputs == "hash")
    if hashes is not None:
        assert np.array_equal(hashes, want_hash), first_difference(names, hashes, want_hash)
    if dih is not None:
        assert np.array_equal(dih, want_dih), first_difference(names, dih, want_dih)


@pytest.mark.parametrize("own_stream", [False, True], ids=["context-stream", "caller-stream"])
def test_device_entry_point_on_a_buffer_that_starts_4_bytes_in(eng, ref, own_stream):
    names, _ = cb.corpus()
    coeffs, want_hash, want_dih = ref
    n = len(coeffs)
    st = eng.stream_create() if own_stream else None
    d_c, d_h, d_d = eng.dev_alloc(coeffs.nbytes + 16), eng.dev_alloc(n * 32), eng.dev_alloc(n * 256)
    try:
        eng.dev_upload(d_c + 4, coeffs)
        eng.pdq_hashes_from_coeffs_dev(d_c + 4, n, d_h, d_d, stream=st)
        eng.stream_synchronize(st)
        hashes, dih = np.zeros((n, 32), np.uint8), np.zeros((n, 8, 32), np.uint8)
        eng.dev_download(hashes, d_h)
        eng.dev_download(dih, d_d)
    finally:
        for p in (d_c, d_h, d_d):
            eng.dev_free(p)
        if own_stream:
            eng.stream_destroy(st)
    assert np.array_equal(hashes, want_hash), first_difference(names, hashes, want_hash)
    assert np.array_equal(dih, want_dih), first_difference(names, dih, want_dih)


@pytest.mark.parametrize("sim", [0, 40])
def test_grouping_the_doubled_corpus_matches_the_oracle(eng, oracle, ref, sim):
    coeffs, hashes, dih = (np.concatenate([a, a]) for a in ref)  # every vector twice: there are pairs at distance 0
    n = len(coeffs)
    rng = np.random.default_rng(33)
    quality = rng.integers(30, 101, n).astype(np.int32)
    quality[::7] = -1
    assert (quality < 0).any() and ((quality >= 0) & (quality < 50)).any() and (quality >= 50).any()
    hf = np.ones(n, np.uint8)
    edges, want_groups = oracle.group_pdq(hashes, sim, variants=dih, has_features=hf, quality=quality)
    assert len(want_groups) > 20
    assert eng.group_files_pdq(hashes, sim, coeffs, hf, quality) == (want_groups, len(edges))
    cut = n // 2 - 37  # the second batch holds the end of the first copy and all of the second
    with eng.library(sim) as lib:
        lib.append(hashes[:cut], coeffs[:cut], hf[:cut], quality[:cut])
        lib.append(hashes[cut:], coeffs[cut:], hf[cut:], quality[cut:])
        assert lib.groups() == want_groups and lib.comparisons == len(edges)
