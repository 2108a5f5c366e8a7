"""What the Hamming and grouping entry points answer before they touch a device (no GPU): a null context, and a null required pointer
behind a context, give RPH_ERR_INVALID_ARG.  Ten sweep entry points (all_pairs, variant_pairs, cross_pairs, variant_cross_pairs and
all_pairs64, each in host and _dev form) and the four grouping calls.  The context of the second half is a block of zeroed host memory:
every one of these calls checks its pointers before it reads the context, and a call that stopped doing so would show here."""
import ctypes as C

import numpy as np
import pytest

H = np.zeros((4, 32), np.uint8)        # hashes (also 4 x 1 variants)
H64 = np.zeros(4, np.uint64)
E = np.zeros(16 * 12, np.uint8)        # room for 16 edges
M = np.zeros(8, np.uint32)             # members / offsets
FAKE_CTX = np.zeros(1 << 16, np.uint8)  # stands in for a context that is never read


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _out64():
    return C.byref(C.c_uint64(7))


def _out32():
    return C.byref(C.c_uint32(7))


# name -> (arguments behind ctx of a call that is valid but for the context, [(index, value): the argument that is nulled])
def calls():
    h, h64, e, m, cnt = _p(H), _p(H64), _p(E), _p(M), _p(M)  # cnt: a "device" counter that is never written
    return {
        "rph_hamming_all_pairs": ([h, 4, 40, 0, 1, e, 16, _out64()], [0, 5, 7]),
        "rph_hamming_all_pairs_dev": ([h, 4, 40, 0, 1, e, 16, cnt, None], [0, 5, 7]),
        "rph_hamming_variant_pairs": ([h, 1, h, None, 4, 40, 0, 1, e, 16, _out64()], [0, 2, 8, 10]),
        "rph_hamming_variant_pairs_dev": ([h, 1, h, None, 4, 40, 0, 1, e, 16, cnt, None], [0, 2, 8, 10]),
        "rph_hamming_cross_pairs": ([h, 4, h, 4, 40, 0, 1, e, 16, _out64()], [0, 2, 7, 9]),
        "rph_hamming_cross_pairs_dev": ([h, 4, h, 4, 40, 0, 1, e, 16, cnt, None], [0, 2, 7, 9]),
        "rph_hamming_variant_cross_pairs": ([h, 1, None, 4, h, None, 4, 40, 0, 1, e, 16, _out64()], [0, 4, 10, 12]),
        "rph_hamming_variant_cross_pairs_dev": ([h, 1, None, 4, h, None, 4, 40, 0, 1, e, 16, cnt, None], [0, 4, 10, 12]),
        "rph_hamming_all_pairs64": ([h64, 4, 16, 0, 1, e, 16, _out64()], [0, 5, 7]),
        "rph_hamming_all_pairs64_dev": ([h64, 4, 16, 0, 1, e, 16, cnt, None], [0, 5, 7]),
        "rph_find_groups256": ([h, 4, 40, m, m, _out32()], [0, 3, 4, 5]),
        "rph_find_groups64": ([h64, 4, 16, m, m, _out32()], [0, 3, 4, 5]),
        "rph_group_files_pdq": ([h, None, None, None, 4, 40, m, m, _out32(), None], [0, 6, 7, 8]),
        "rph_group_files_pdq_append": ([h, None, None, None, 2, m, m, 1, h, None, None, None, 2, 40, m, m, _out32(), None], [0, 5, 6, 8, 14, 15, 16]),
    }


NAMES = sorted(calls())


def test_the_table_names_every_entry_point():
    sweeps = [f"rph_hamming_{form}{dev}" for form in ("all_pairs", "variant_pairs", "cross_pairs", "variant_cross_pairs", "all_pairs64") for dev in ("", "_dev")]
    assert sorted(sweeps + ["rph_find_groups256", "rph_find_groups64", "rph_group_files_pdq", "rph_group_files_pdq_append"]) == NAMES


@pytest.mark.parametrize("name", NAMES)
def test_null_context(name):
    from rupphash_amd import _lib

    args, _ = calls()[name]
    assert getattr(_lib.load(), name)(None, *args) == _lib.RPH_ERR_INVALID_ARG


@pytest.mark.parametrize("name", NAMES)
def test_null_required_pointer(name):
    from rupphash_amd import _lib

    args, required = calls()[name]
    fn = getattr(_lib.load(), name)
    for k in required:
        nulled = list(args)
        assert nulled[k] is not None
        nulled[k] = None
        assert fn(_p(FAKE_CTX), *nulled) == _lib.RPH_ERR_INVALID_ARG, (name, k)
    assert not FAKE_CTX.any() and not E.any() and not M.any()
