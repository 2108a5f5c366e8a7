"""The coefficient-level JPEG corpus (tests/jpeg_coef_corpus.py) through the device: the plane kernels (rph_jpeg_decode), every entropy
mode of rph_jpeg_pdq_pixel_hash_batch (the plane, colour and PDQ kernels, with pixel hashes) and of rph_jpeg_pdq_hash_batch (the fused
kernel for every three-component file), 64-byte segments, and a call large enough for AUTO to walk on the device -- each against "oracle
decode, then oracle features", in both flavours.  The reference is computed once per flavour and shared; a failure names the file (its
class is the part before "/"), the flavour and the mode."""
import numpy as np
import pytest

import blake3_util as b3
import jpeg_coef_corpus as cc

pytestmark = pytest.mark.gpu

HOST, DEVICE, AUTO, DEVICE_SEQUENTIAL = 0, 1, 2, 3
MODES = {"host": (HOST, None), "device": (DEVICE, None), "device_sequential": (DEVICE_SEQUENTIAL, None), "auto": (AUTO, None), "device_segments64": (DEVICE, 64)}
FLAVOURS = {0: "zune", 1: "libjpeg"}


@pytest.fixture(scope="module")
def eng():
    from rupphash_amd import Engine

    e = Engine(0)
    yield e
    e.jpeg_set_entropy(AUTO)
    e.jpeg_set_segments()
    e.close()


@pytest.fixture(scope="module")
def names():
    return list(cc.corpus())


@pytest.fixture(scope="module")
def files(names):
    return [cc.corpus()[n][0] for n in names]


@pytest.fixture(scope="module")
def want(oracle, files):
    """flavour -> per file None (the oracle refuses it) or dict(px, valid, hash, quality, coeffs, dihedral, pixel_hash); never modified"""
    out = {}
    for fl in FLAVOURS:
        rows = []
        for data in files:
            try:
                px = oracle.jpeg_decode(data, fl)
            except ValueError:
                rows.append(None)
                continue
            rc, c, q = oracle.pdq_features(px)
            row = {"px": px, "valid": rc == 0}
            if rc == 0:
                row.update(hash=oracle.to_hash(c), quality=np.float32(q).view(np.uint32), coeffs=np.asarray(c, np.float32).view(np.uint32),
                           dihedral=oracle.dihedral_hashes(c))
            rows.append(row)
        live = [r for r in rows if r is not None]
        for r, digest in zip(live, b3.blake3_many([b3.rgba16_bytes(r["px"]) for r in live])):
            r["pixel_hash"] = digest
        out[fl] = rows
    return out


def _run(eng, files, mode, flavour, pixel_hash):
    entropy, seg_bytes = MODES[mode]
    try:
        eng.jpeg_set_entropy(entropy)
        if seg_bytes is not None:
            eng.jpeg_set_segments(0, seg_bytes)
        return eng.jpeg_pdq_hash_batch(files, flavour=flavour, threads=4, want_quality=True, want_coeffs=True, want_dihedral=True, want_pixel_hash=pixel_hash)
    finally:
        eng.jpeg_set_entropy(AUTO)
        eng.jpeg_set_segments()


def _differences(out, rows, names, flavour, mode, index=None):
    """[(file, flavour, mode, what)] where the call's outputs are not the oracle's; index[k] = the corpus file of the call's row k"""
    n = len(out["status"])
    index = range(n) if index is None else index
    bad = []
    for k, i in zip(range(n), index):
        tag, w = (names[i], FLAVOURS[flavour], mode), rows[i]
        if w is None:
            zero = not (out["valid"][k] or out["hash"][k].any() or out["quality"][k].view(np.uint32) or out["coeffs"][k].any() or out["dihedral"][k].any()
                        or ("pixel_hash" in out and out["pixel_hash"][k].any()))
            if out["status"][k] == 0 or not zero:
                bad.append(tag + ("the oracle refuses it",))
            continue
        if out["status"][k] != 0:
            bad.append(tag + (f"status {int(out['status'][k])}",))
        elif bool(out["valid"][k]) != w["valid"]:
            bad.append(tag + ("valid",))
        elif "pixel_hash" in out and out["pixel_hash"][k].tobytes() != w["pixel_hash"]:
            bad.append(tag + ("pixel_hash",))
        elif w["valid"]:
            for key in ("coeffs", "hash", "quality", "dihedral"):
                got = out[key][k].view(np.uint32) if out[key].dtype == np.float32 else out[key][k]
                if not np.array_equal(got, w[key]):
                    bad.append(tag + (key,))
                    break
    return bad


@pytest.mark.parametrize("flavour", list(FLAVOURS), ids=list(FLAVOURS.values()))
def test_plane_kernels_give_the_oracles_pixels(eng, want, files, names, flavour):
    from rupphash_amd import RphError

    bad = []
    for name, data, w in zip(names, files, want[flavour]):
        if w is None:
            with pytest.raises(RphError):
                eng.jpeg_decode(data, flavour)
            continue
        got = eng.jpeg_decode(data, flavour)
        if not np.array_equal(got, w["px"]):
            bad.append((name, FLAVOURS[flavour], "decode", int((got != w["px"]).sum())))
    assert not bad, bad
    assert {cc.klass(n) for n, w in zip(names, want[flavour]) if w is not None} == set(cc.CLASSES)


@pytest.fixture(scope="module")
def refused_status():
    return {}


@pytest.mark.parametrize("flavour", list(FLAVOURS), ids=list(FLAVOURS.values()))
@pytest.mark.parametrize("mode", list(MODES))
def test_every_entropy_mode_with_pixel_hashes_gives_the_oracles_results(eng, want, files, names, refused_status, mode, flavour):
    """the plane kernels, the colour kernel, the PDQ kernels and BLAKE3 behind every way of walking the Huffman streams"""
    out = _run(eng, files, mode, flavour, pixel_hash=True)
    bad = _differences(out, want[flavour], names, flavour, mode)
    assert not bad, bad
    # a refused file has the same status in whichever mode ran first and in this one
    first = refused_status.setdefault(flavour, out["status"].copy())
    assert np.array_equal(out["status"], first), (FLAVOURS[flavour], mode, [names[i] for i in np.flatnonzero(out["status"] != first)])


@pytest.mark.parametrize("flavour", list(FLAVOURS), ids=list(FLAVOURS.values()))
@pytest.mark.parametrize("mode", list(MODES))
def test_fused_kernel_gives_the_oracles_results(eng, want, files, names, mode, flavour):
    """without pixel hashes every three-component file goes through the fused kernel (IDCT, upsampling, colour and luma in LDS tiles): its
    bytes are seen through the PDQ coefficients, bit for bit (tests/test_jpeg_coef_cpu.py: one luma level anywhere changes them)"""
    out = _run(eng, files, mode, flavour, pixel_hash=False)
    bad = _differences(out, want[flavour], names, flavour, mode)
    assert not bad, bad


def _progressive(data):
    sos = data.find(b"\xff\xda")
    return sos > 0 and b"\xff\xc2" in data[:sos]


@pytest.mark.parametrize("flavour", list(FLAVOURS), ids=list(FLAVOURS.values()))
def test_a_few_thousand_files_in_auto_mode_give_the_oracles_results(eng, want, files, names, flavour):
    """The corpus (without its one large file) repeated until AUTO takes sequential and progressive files to the device walks, over several
    chunks: every copy has the oracle's result wherever it fell in the call."""
    small = [i for i, n in enumerate(names) if n not in cc.LARGE]
    index = [small[k % len(small)] for k in range(14 * len(small))]
    call = [files[i] for i in index]
    # AUTO's routing (jpeg_pipeline.cpp, run_batch): at least 512 lanes of sequential files, and progressive files whose bytes would keep
    # the 4 host threads (41 MB/s each) busy for longer than the device needs for the longest of them (0.6 us per byte) -- by a margin
    assert 3000 <= len(call) <= 5000
    assert sum(not _progressive(d) for d in call) >= 512
    prog = [d for d in call if _progressive(d)]
    assert sum(map(len, prog)) / (4 * 41e6) > 1.5 * 0.6e-6 * max(map(len, prog))
    out = _run(eng, call, "auto", flavour, pixel_hash=False)
    bad = _differences(out, want[flavour], names, flavour, "auto, large call", index)
    assert not bad, bad[:40]
