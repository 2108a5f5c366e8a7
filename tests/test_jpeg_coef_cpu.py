"""The coefficient-level JPEG corpus (tests/jpeg_coef_corpus.py) on the CPU: the writers against the oracle's entropy decoder and the
library's host decoder, the oracle's two integer IDCTs against a numpy restatement that is not C, the Pillow pin on the files a 16-bit
decoder can agree on, and the PDQ coefficients as an observer of single luma bytes."""
import hashlib
import json
import os

import numpy as np
import pytest

import jpeg_coef_corpus as cc
import jpeg_util as ju

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def corpus():
    return cc.corpus()


@pytest.fixture(scope="module")
def decoded(oracle, corpus):
    """name -> (geometry, qt, coefficients) of the oracle, None where it refuses the file"""
    out = {}
    for name, (data, _, _) in corpus.items():
        try:
            out[name] = oracle.jpeg_coefficients(data)
        except ValueError:
            out[name] = None
    return out


def test_picture_encoders_write_the_bytes_they_wrote_before_the_split():
    """encode_baseline / encode_progressive are thin callers of the coefficient-level writers now: their output is pinned by the digests of
    what they wrote before (tests/golden/jpeg_encoder_sha256.json)"""
    a = np.array(ju.make_image(45, 37, seed=11))
    got = {
        "baseline_420_rst2": ju.encode_baseline(a, cc.S420, restart_interval=2),
        "baseline_440_noninterleaved_q16": ju.encode_baseline(a, cc.S440, quality_scale=0.3, sixteen_bit_tables=True, interleaved=False),
        "baseline_gray_rst3": ju.encode_baseline(a[..., 0], gray=True, restart_interval=3),
        "baseline_444_fault": ju.encode_baseline(a, cc.S444, fault=("dc_cat", 5, 13)),
        "progressive_deep_422": ju.encode_progressive(a, ju.SCRIPT_DEEP, cc.S422),
        "progressive_refine_first_420_long": ju.encode_progressive(a, ju.SCRIPT_REFINE_BEFORE_OTHER_BANDS, cc.S420, quality_scale=0.5, long_codes=True),
        "progressive_gray": ju.encode_progressive(a[..., 0], ju.SCRIPT_GRAY, gray=True),
        "progressive_libjpeg_fault": ju.encode_progressive(a, ju.SCRIPT_LIBJPEG, fault=("refine_bad_symbol", 9)),
    }
    with open(os.path.join(GOLDEN, "jpeg_encoder_sha256.json")) as f:
        want = json.load(f)
    assert {k: hashlib.sha256(v).hexdigest() for k, v in got.items()} == want


def test_corpus_is_the_same_on_every_call_and_names_every_class(corpus):
    again, rng = {}, np.random.default_rng(20260)  # (the first two classes that draw from the generator, drawn again)
    cc._overshoot(again, rng)
    cc._random_heavy(again, rng)
    assert len(again) > 70 and all(again[n][0] == corpus[n][0] for n in again)
    assert {cc.klass(n) for n in corpus} == set(cc.CLASSES)
    assert 200 <= len(corpus) <= 500
    assert all(len(d) < 40000 for d, _, _ in corpus.values())


def test_decoders_hold_the_coefficients_the_writer_expects(oracle, corpus, decoded):
    """the oracle against plain int16 arithmetic on the writer's arrays, then the host decoder (lookup tables, 64-bit refills, fast AC path)
    against the oracle, coefficient for coefficient"""
    from rupphash_amd.engine import Engine

    bad = []
    for name, (data, expected, _) in corpus.items():
        if decoded[name] is None:
            continue
        g, q, c = decoded[name]
        if expected is not None and not np.array_equal(c, expected):
            bad.append((name, "oracle != expected", int((c != expected).sum()) if c.shape == expected.shape else (c.shape, expected.shape)))
        assert Engine.jpeg_info(data) == oracle.jpeg_info(data), name
        g2, q2, c2 = Engine.jpeg_coefficients(data)
        if not (np.array_equal(g, g2) and np.array_equal(q, q2) and np.array_equal(c, c2)):
            bad.append((name, "host decoder != oracle", int((c != c2).sum()) if c.shape == c2.shape else (c.shape, c2.shape)))
    assert not bad, bad


def test_refusals_are_shared_and_rare(corpus, decoded):
    from rupphash_amd._lib import RphError
    from rupphash_amd.engine import Engine

    refused = [n for n in corpus if decoded[n] is None]  # (none at present: the loop below is for a corpus that gains one)
    for name in refused:
        with pytest.raises(RphError):
            Engine.jpeg_coefficients(corpus[name][0])
    assert len(refused) <= len(corpus) // 10, refused
    for k in cc.CLASSES:
        assert any(cc.klass(n) == k and decoded[n] is not None for n in corpus), k


# ---- the oracle's IDCTs restated in numpy: int64 arrays, reduced modulo 2^32 wherever the C code holds a 32-bit value ------------------

def _w(x):
    return ((x + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)


def _islow_1d(s, shift):
    """jidctint.c's butterfly along axis 0 of s (8, ...)"""
    z1 = _w(_w(s[2] + s[6]) * 4433)
    tmp2 = _w(z1 + _w(s[6] * -15137))
    tmp3 = _w(z1 + _w(s[2] * 6270))
    tmp0 = _w(_w(s[0] + s[4]) << 13)
    tmp1 = _w(_w(s[0] - s[4]) << 13)
    tmp10, tmp13, tmp11, tmp12 = _w(tmp0 + tmp3), _w(tmp0 - tmp3), _w(tmp1 + tmp2), _w(tmp1 - tmp2)
    tmp0, tmp1, tmp2, tmp3 = s[7], s[5], s[3], s[1]
    z1, z2, z3, z4 = _w(tmp0 + tmp3), _w(tmp1 + tmp2), _w(tmp0 + tmp2), _w(tmp1 + tmp3)
    z5 = _w(_w(z3 + z4) * 9633)
    tmp0, tmp1, tmp2, tmp3 = _w(tmp0 * 2446), _w(tmp1 * 16819), _w(tmp2 * 25172), _w(tmp3 * 12299)
    z1, z2 = _w(z1 * -7373), _w(z2 * -20995)
    z3, z4 = _w(_w(z3 * -16069) + z5), _w(_w(z4 * -3196) + z5)
    tmp0 = _w(tmp0 + _w(z1 + z3))
    tmp1 = _w(tmp1 + _w(z2 + z4))
    tmp2 = _w(tmp2 + _w(z2 + z3))
    tmp3 = _w(tmp3 + _w(z1 + z4))
    rnd = 1 << (shift - 1)
    pairs = [(tmp10, tmp3), (tmp11, tmp2), (tmp12, tmp1), (tmp13, tmp0)]
    lo = [_w(_w(a + b) + rnd) >> shift for a, b in pairs]
    hi = [_w(_w(a - b) + rnd) >> shift for a, b in pairs]
    return np.stack(lo + hi[::-1])


def _stb_1d(s, bias, shift):
    """stb_image's butterfly along axis 0 of s (8, ...)"""
    p1 = _w(_w(s[2] + s[6]) * 2217)
    t2 = _w(p1 + _w(s[6] * -7567))
    t3 = _w(p1 + _w(s[2] * 3135))
    t0 = _w(_w(s[0] + s[4]) << 12)
    t1 = _w(_w(s[0] - s[4]) << 12)
    x0, x3, x1, x2 = _w(t0 + t3), _w(t0 - t3), _w(t1 + t2), _w(t1 - t2)
    t0, t1, t2, t3 = s[7], s[5], s[3], s[1]
    p3, p4, p1, p2 = _w(t0 + t2), _w(t1 + t3), _w(t0 + t3), _w(t1 + t2)
    p5 = _w(_w(p3 + p4) * 4816)
    t0, t1, t2, t3 = _w(t0 * 1223), _w(t1 * 8410), _w(t2 * 12586), _w(t3 * 6149)
    p1 = _w(p5 + _w(p1 * -3685))
    p2 = _w(p5 + _w(p2 * -10497))
    p3, p4 = _w(p3 * -8034), _w(p4 * -1597)
    t3 = _w(t3 + _w(p1 + p4))
    t2 = _w(t2 + _w(p2 + p3))
    t1 = _w(t1 + _w(p2 + p4))
    t0 = _w(t0 + _w(p1 + p3))
    pairs = [(_w(x0 + bias), t3), (_w(x1 + bias), t2), (_w(x2 + bias), t1), (_w(x3 + bias), t0)]
    lo = [_w(a + b) >> shift for a, b in pairs]
    hi = [_w(a - b) >> shift for a, b in pairs]
    return np.stack(lo + hi[::-1])


def restated_blocks(coef, qt, flavour):
    """coef (n, 64) int16, qt (64,) -> (n, 8, 8) uint8 samples: dequantise, columns, rows, range limit"""
    c = _w(coef.astype(np.int64) * qt.astype(np.int64)).reshape(-1, 8, 8)  # [block, row, column]
    if flavour == 1:
        ws = _islow_1d(c.transpose(1, 0, 2), 11)                 # along rows' index = down the columns: [row, block, column]
        res = _islow_1d(ws.transpose(2, 1, 0), 18)               # along the column index = across a row: [column, block, row]
        v = ((_w(res + 512) & 1023) - 512) + 128                 # range_limit[v & RANGE_MASK], the table centred on 128
    else:
        ws = _stb_1d(c.transpose(1, 0, 2), 512, 10)
        v = _stb_1d(ws.transpose(2, 1, 0), 65536 + (128 << 17), 17)
    return np.clip(v, 0, 255).astype(np.uint8).transpose(1, 2, 0)


def restated_gray(geo, qt, coef, w, h, flavour):
    bw, bh, tq = int(geo[0][0]), int(geo[0][1]), int(geo[0][4])
    px = restated_blocks(coef[:bw * bh], qt[tq], flavour)
    return px.reshape(bh, bw, 8, 8).transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8)[:h, :w]


@pytest.mark.parametrize("flavour", [0, 1])
def test_oracle_idcts_equal_their_numpy_restatement_on_every_gray_file(oracle, corpus, decoded, flavour):
    """every product and sum of the two butterflies modulo 2^32, the range-limit mask of flavour 1 and the clamp of flavour 0 -- on
    impulses, the DC sweep (which also shows that a full butterfly gives what libjpeg's zero-AC shortcut gives: the oracle has no shortcut,
    Pillow has, and they agree on `overshoot`), heavy-tailed blocks and the wrapped coefficients of the progressive classes"""
    seen, bad = set(), []
    for name, (data, _, _) in corpus.items():
        if decoded[name] is None or len(decoded[name][0]) != 1:
            continue
        w, h, _ = oracle.jpeg_info(data)
        if not np.array_equal(restated_gray(*decoded[name], w, h, flavour), oracle.jpeg_decode(data, flavour)):
            bad.append(name)
        seen.add(cc.klass(name))
    assert not bad, (flavour, bad)
    assert {"impulse", "dc_sweep", "random_heavy", "overshoot", "dc_pred", "prog_extreme"} <= seen


OVERSHOOT_BOUND = 2


def test_both_flavours_stay_close_to_the_float_idct_on_overshoot(oracle, corpus, decoded):
    """On `overshoot` no intermediate leaves 16 bits, so both integer IDCTs approximate the real one: each sample is within OVERSHOOT_BOUND
    levels of clip(round(float64 IDCT) + 128).  The bound is a property of the fixed-point constants (13-bit with 2 guard bits in flavour 1,
    12-bit with a 10-bit intermediate shift in flavour 0), not of the code under test; measured here against the float64 IDCT on the
    class's five gray files: flavour 1 (islow) differs by at most 1, flavour 0 (stb) by at most 1.  The bound allows one level more than the
    measured maximum, for other seeds of the corpus.  Only the gray files are compared: a colour file's planes show in its pixels through
    upsampling and colour conversion alone (the class's colour files are held to Pillow byte for byte, below)."""
    k = np.arange(8)
    m = np.cos((2 * k[None, :] + 1) * k[:, None] * np.pi / 16) * 0.5
    m[0] *= 1 / np.sqrt(2)
    worst = {0: 0, 1: 0}
    n = 0
    for name, (data, _, in_range) in corpus.items():
        if cc.klass(name) != "overshoot" or len(decoded[name][0]) != 1:
            continue
        geo, qt, coef = decoded[name]
        w, h, _ = oracle.jpeg_info(data)
        bw, bh = int(geo[0][0]), int(geo[0][1])
        deq = (coef.astype(np.float64) * qt[int(geo[0][4])].astype(np.float64)).reshape(bh, bw, 8, 8)
        real = np.einsum("ux,abuv,vy->abxy", m, deq, m)
        ideal = np.clip(np.round(real) + 128, 0, 255).transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8)[:h, :w]
        for fl in (0, 1):
            worst[fl] = max(worst[fl], int(np.abs(oracle.jpeg_decode(data, fl).astype(np.int64) - ideal).max()))
        n += 1
    print("overshoot: max |integer IDCT - float IDCT| per flavour:", worst)
    assert n >= 5
    assert worst[0] <= OVERSHOOT_BOUND and worst[1] <= OVERSHOOT_BOUND, worst


def test_pillow_decodes_the_in_range_files_to_the_oracles_bytes(oracle, corpus):
    """The pin on libjpeg-turbo, on coefficients no forward DCT of an 8-bit picture gives -- but only where a 16-bit decoder can agree:
    libjpeg-turbo's SIMD IDCT keeps 16-bit intermediates where jidctint.c, which the oracle restates, keeps 32."""
    pytest.importorskip("PIL")
    bad = []
    n = 0
    for name, (data, _, in_range) in corpus.items():
        if not in_range:
            continue
        n += 1
        got, want = oracle.jpeg_decode(data, 1), ju.pillow_decode(data)
        if not np.array_equal(got, want):
            bad.append((name, int((got != want).sum())))
    assert n >= 25 and not bad, bad


def test_one_luma_level_anywhere_changes_the_pdq_coefficients(oracle, corpus):
    """The fused kernel's luma bytes are seen only through the 256 float32 PDQ coefficients.  On the corpus's image sizes they are a sharp
    enough observer: one luma byte moved by one level -- at 20 seeded positions, the last row and the last column among them -- changes
    their bits, on the oracle's own decode of five chroma_edges images."""
    rng = np.random.default_rng(5)
    names = [n for n in corpus if cc.klass(n) == "chroma_edges" and ("_136x72_" in n or "_129x65_" in n)][::7][:5]
    assert len(names) == 5
    for name in names:
        luma = oracle.luma601(oracle.jpeg_decode(corpus[name][0], 1))
        h, w = luma.shape
        rc, base, _ = oracle.pdq_from_luma(luma)
        assert rc == 0
        where = [(h - 1, int(rng.integers(w))), (int(rng.integers(h)), w - 1), (h - 1, w - 1), (0, 0)]
        where += [(int(rng.integers(h)), int(rng.integers(w))) for _ in range(16)]
        for y, x in where:
            moved = luma.copy()
            moved[y, x] = moved[y, x] + 1 if moved[y, x] < 255 else 254
            _, c, _ = oracle.pdq_from_luma(moved)
            assert not np.array_equal(c.view(np.uint32), base.view(np.uint32)), (name, y, x)
