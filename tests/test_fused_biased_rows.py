"""CPU model of three arithmetic facts the fused 512x512 PDQ kernel (rupphash_amd/csrc/pdq_fused512.hip) relies on since its luma
rows are carried biased (the f16 number 1024 + y, bits 0x6400 | y) and the frame bands divide with folded constants:

 (1) the window slide v = (v - hist_b) + l_b with both luma operands biased gives the integer v - h + l in f16;
 (2) the first window sum of a lane's eight rows removes the bias pairwise: x_b + (y_b - 2048) = x + y, and the tree
     (a + bb) + (cc + dd) over four such pairs is the integer sum of the eight rows;
 (3) q0 = hs * (8/d), r = fma(-q0, d/8, hs), q = fma(r, 8/d, q0) is the IEEE quotient (8 hs) / d for every integer hs the
     horizontal window sum can take (<= 8 * 2040 = 16 320) and d = 4..8: Markstein's sequence with the factor 8 folded into its
     constants.

numpy's float16 arithmetic rounds every single operation correctly, which is what v_pk_add_f16 does."""
import numpy as np

f16 = np.float16
f32 = np.float32
f64 = np.float64


def biased(y):
    b = (np.asarray(y, np.int64) + 1024).astype(f16)
    assert np.array_equal(b.view(np.uint16), (0x6400 | np.asarray(y, np.int64)).astype(np.uint16))  # 0x6400 | y IS 1024 + y
    return b


def test_slide_with_biased_operands_is_exact():
    """every v in [0, 2040] and h, l in [0, 255] with 0 <= v - h + l <= 2040 (the window sum stays a window sum)"""
    v = np.arange(0, 2041, dtype=np.int64)[:, None]
    l = np.arange(0, 256, dtype=np.int64)[None, :]
    vh, lb = v.astype(f16), biased(l)
    lo, hi = 0, 0
    for h in range(256):
        t = vh - biased(h)                       # first operation: v - hist_b, in [-1279, 1016]
        got = (t + lb).astype(np.int64)          # second: + L_b
        want = v - h + l
        ok = (want >= 0) & (want <= 2040)
        assert np.array_equal(got[ok], want[ok]), h
        ti = t.astype(np.int64)
        assert np.array_equal(ti, np.broadcast_to(v - h - 1024, ti.shape))  # the intermediate itself is exact
        lo, hi = min(lo, int(ti.min())), max(hi, int(ti.max()))
    assert (lo, hi) == (-1279, 1016)


def test_pair_sum_removes_two_biases_exactly():
    a = np.arange(256, dtype=np.int64)[:, None]
    b = np.arange(256, dtype=np.int64)[None, :]
    t = biased(b) - f16(2048)                    # in [-1024, -769]
    assert np.array_equal(t.astype(np.int64), b - 1024)
    s = biased(a) + t
    assert np.array_equal(s.astype(np.int64), a + b)


def first_v(rows):
    """rows: (..., 8) luma integers, the seven rows above and the lane's first row -> the kernel's first window sum"""
    r = biased(rows)
    two = f16(2048)
    a = r[..., 0] + (r[..., 1] - two)
    bb = r[..., 2] + (r[..., 3] - two)
    cc = r[..., 4] + (r[..., 5] - two)
    dd = r[..., 6] + (r[..., 7] - two)
    return (a + bb) + (cc + dd)


def test_first_window_sum_tree_is_the_integer_sum():
    extremes = np.array([[0] * 8, [255] * 8, [255, 0] * 4, [0, 255] * 4, [255] * 4 + [0] * 4, [0] * 4 + [255] * 4,
                         [255, 255, 0, 0] * 2, [0, 0, 255, 255] * 2, [255] * 7 + [254], [1] + [0] * 7], np.int64)
    corners = np.array([[255 * ((k >> i) & 1) for i in range(8)] for k in range(256)], np.int64)  # every 0 / 255 pattern
    rng = np.random.default_rng(8)
    sample = rng.integers(0, 256, (200_000, 8), dtype=np.int64)
    for rows in (extremes, corners, sample):
        got = first_v(rows)
        assert np.array_equal(got.astype(np.int64), rows.sum(axis=1))
    assert int(first_v(extremes[1:2])[0]) == 2040  # the f16 limit is reached


def fma32(a, b, c):
    """round_f32(a * b + c) for f32 arrays: the product is exact in f64 (24 x 24 bits); the f64 sum is rounded to odd whenever it
    is inexact (TwoSum), so that the final rounding to f32 is the single rounding of the exact value"""
    p = a.astype(f64) * b.astype(f64)
    c = np.broadcast_to(c.astype(f64), p.shape)
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)
    even = (s.view(np.int64) & 1) == 0
    fix = (e != 0) & even
    s = np.where(fix, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
    return s.astype(f32)


def test_folded_division_is_the_ieee_quotient():
    hs = np.arange(0, 16321, dtype=np.int64)
    hs32 = hs.astype(f32)
    assert np.array_equal(hs32.astype(np.int64), hs)
    for di in (4, 5, 6, 7, 8):
        d = f32(di)
        d8 = d * f32(0.125)                      # d / 8: exact
        assert f64(d8) * 8 == di
        dinv8 = (f32(1.0) / d) * f32(8.0)        # 8 fl(1 / d): exact scaling
        assert f64(dinv8) == f64(f32(1.0) / d) * 8
        q0 = hs32 * dinv8
        r = fma32(-q0, np.full_like(q0, d8), hs32)
        q = fma32(r, np.full_like(q0, dinv8), q0)
        want = (hs32 * f32(8.0)) / d             # the kernel's former form: (hs * 8) / d, one IEEE division of an exact product
        assert np.array_equal(q.view(np.uint32), want.view(np.uint32)), di
        # and column 511's window of 4: (16 hs) / d is twice that, power-of-two scaling commutes with the rounding
        want16 = (hs32 * f32(16.0)) / d
        assert np.array_equal((q * f32(2.0)).view(np.uint32), want16.view(np.uint32)), di
