"""Inflate on the device (-m gpu) on the streams of deflate_util's own writer, through both carriers with decompression forced to the
device: decoded pixels against expand(tokens), batch statuses, pixel hashes against a BLAKE3 of the expected pixels (the bytes the
sink's flush stored, as opposed to the bytes its ring held), refused streams refused with zero outputs, the same arrays in the HOST,
DEVICE and AUTO modes, and every file alone as in one call of all of them."""
import functools

import numpy as np
import pytest

import blake3_util as b3
import deflate_util as du
import png_util as pu
import tiff_util as tu

pytestmark = pytest.mark.gpu

HOST, DEVICE, AUTO = 0, 1, 2
KEYS = ("hash", "quality", "valid", "status", "pixel_hash")
# the named streams by what they aim at (so that each test stays short), and the random ones
GROUPS = {
    "copies": ("copy_", "ring_", "dist32768_", "flush_start", "cap_"),
    "codes_and_blocks": ("lit_", "dist_lengths", "deep_", "all_length", "length_258", "single_", "no_distance", "literal_code", "two_code", "repeat_", "all_19", "hclen_",
                         "empty_", "final_empty", "only_empty", "stored_", "400_"),
    "flushes": ("final_flush_", "all_ff_"),
    "random": ("random",),
}


class Carrier:
    def __init__(self, kind):
        self.kind = kind
        self.invalid = pu.INVALID if kind == "png" else tu.INVALID

    def set_mode(self, eng, mode):
        (eng.png_set_inflate if self.kind == "png" else eng.tiff_set_decompress)(mode)

    def decode(self, eng, data):
        return (eng.png_decode if self.kind == "png" else eng.tiff_decode)(data)

    def batch(self, eng, files):
        return (eng.png_pdq_hash_batch if self.kind == "png" else eng.tiff_pdq_hash_batch)(files, want_pixel_hash=True)

    def pixels(self, want):
        """the expected bytes as the image the carrier holds: one row (PNG) or one column (TIFF) of gray"""
        a = np.frombuffer(want, np.uint8)
        return a.reshape(1, -1) if self.kind == "png" else a.reshape(-1, 1)


@pytest.fixture(scope="module")
def eng():
    from rupphash_amd import Engine

    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module", params=["png", "tiff"])
def carrier(request):
    return Carrier(request.param)


@functools.lru_cache(maxsize=None)
def group_files(kind, group):
    files = [f for f in du.carrier_files(kind) if f[2] is not None and f[0].startswith(GROUPS[group])]
    return files


@functools.lru_cache(maxsize=None)
def expected_pixel_hash(kind, name):
    want = {n: w for n, _, w in du.carrier_files(kind)}[name]
    return b3.blake3(pu.to_rgba16(Carrier(kind).pixels(want)))


def test_groups_leave_no_stream_out():
    for kind in ("png", "tiff"):
        valid = [f[0] for f in du.carrier_files(kind) if f[2] is not None]
        grouped = [f[0] for g in GROUPS for f in group_files(kind, g)]
        assert sorted(grouped) == sorted(valid) and len(valid) == len(du.valid_streams())


@pytest.mark.parametrize("group", list(GROUPS))
def test_device_decode_and_batch_equal_expected_bytes(eng, carrier, group):
    files = group_files(carrier.kind, group)
    assert len(files) >= 50
    carrier.set_mode(eng, DEVICE)
    try:
        for name, data, want in files:
            got = carrier.decode(eng, data)
            assert got.dtype == np.uint8 and got.shape == carrier.pixels(want).shape and got.tobytes() == want, name
        out = carrier.batch(eng, [d for _, d, _ in files])
    finally:
        carrier.set_mode(eng, AUTO)
    assert not out["status"].any(), [files[k][0] for k in np.nonzero(out["status"])[0]]
    for k, (name, data, want) in enumerate(files):
        assert out["pixel_hash"][k].tobytes() == expected_pixel_hash(carrier.kind, name), name
        assert out["valid"][k] == 0 and not out["hash"][k].any()  # (one pixel wide or high: below PDQ's 5 px)


def test_device_refuses_every_refused_stream_with_zero_outputs(eng, carrier):
    from rupphash_amd import RphError

    files = [f for f in du.carrier_files(carrier.kind) if f[2] is None]
    assert len(files) == len(du.refused_streams())
    carrier.set_mode(eng, DEVICE)
    try:
        out = carrier.batch(eng, [d for _, d, _ in files])
        for name, data, _ in files:
            with pytest.raises(RphError) as e:
                carrier.decode(eng, data)
            assert e.value.status == carrier.invalid, name
    finally:
        carrier.set_mode(eng, AUTO)
    for k, (name, _, _) in enumerate(files):
        assert out["status"][k] == carrier.invalid, name
        assert not out["hash"][k].any() and not out["pixel_hash"][k].any() and out["valid"][k] == 0, name


def test_modes_agree_on_valid_and_refused_streams(eng, carrier):
    corpus = du.carrier_files(carrier.kind)
    files = [d for _, d, _ in corpus]
    outs = []
    try:
        for mode in (HOST, DEVICE, AUTO):
            carrier.set_mode(eng, mode)
            outs.append(carrier.batch(eng, files))
    finally:
        carrier.set_mode(eng, AUTO)
    for k, (name, _, want) in enumerate(corpus):
        assert outs[0]["status"][k] == (0 if want is not None else carrier.invalid), name
        if want is None:
            assert not outs[0]["hash"][k].any() and not outs[0]["pixel_hash"][k].any()
    for o in outs[1:]:
        for key in KEYS:
            assert np.array_equal(o[key], outs[0][key]), key


def test_each_file_alone_as_in_one_call_of_all(eng, carrier):
    """valid and refused files interleaved in one call, then each alone: the ring, `flushed` and the Adler sums of one stream (or call)
    do not reach the next"""
    corpus = du.carrier_files(carrier.kind)
    order = np.random.default_rng(3).permutation(len(corpus))
    files = [corpus[int(i)][1] for i in order]
    carrier.set_mode(eng, DEVICE)
    try:
        big = carrier.batch(eng, files)
        assert (big["status"] != 0).sum() == len(du.refused_streams())
        for k, data in enumerate(files):
            one = carrier.batch(eng, [data])
            for key in KEYS:
                assert np.array_equal(big[key][k], one[key][0]), (corpus[int(order[k])][0], key)
    finally:
        carrier.set_mode(eng, AUTO)
