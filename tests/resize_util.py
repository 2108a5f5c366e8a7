"""The > 512 px pre-downsample restated in plain Python / numpy (no GPU, no C), with the images and geometries its tests share.

The restatement follows the published algorithm as the comment block and build_axis of rupphash_amd/csrc/resize_kernels.hip state it
(fast_image_resize 6.1.0, Convolution(Box) on U8; the Pillow ImagingResample family), not the oracle's C code:

  per axis    scale = in / out, filter_scale = max(scale, 1), radius = filter_scale / 2, window = 2 ceil(radius) + 1
              output o: centre (o + 0.5) scale; candidates floor(centre - radius) .. ceil(centre + radius), clamped to the source;
              weight box((x - (centre - 0.5)) / filter_scale) over the half-open box (-1/2, 1/2], all in f64;
              leading zero weights are skipped and trailing ones cut (trimmed bounds), the rest normalised to sum 1;
              precision = the first p in 0 .. 15 with round(max weight * 2^(p + 1)) >= 2^15 (15 if none), coefficients round(w * 2^p) as i16
  pixel       clip8((2^(p - 1) + sum src * coef) >> p) in exact integers
  passes      horizontal into a u8 intermediate, then vertical
  (the clamp to 255 cannot bite: the coefficients of an output sum to 2^p + at most window / 2 of rounding, so the value stays below
  255 + 1/2 + 255 * window / 2^(p + 1), which needs a window of about 128 taps, a source beyond 64 x 512 px, to reach 256)

to_luma601 is (299 r + 587 g + 114 b + 500) // 1000 and the thumbnail's size is calculate_target_dimensions of pdqhash.rs:224-235.
PARITY with the crate itself stays UNPINNED: this pins the oracle and the kernels to the published arithmetic.
"""
import functools
import math
from collections import namedtuple

import numpy as np

MAX_DIM = 512

Axis = namedtuple("Axis", "start size coef window precision")  # start, size: int64[out]; coef: int16[out][window], zero behind size


# ---------------------------------------------------------------- the restatement
def target_dimensions(w, h, max_dim=MAX_DIM):
    if w == 0 or h == 0:
        return max(w, 1), max(h, 1)
    if w > h:
        return max_dim, max(h * max_dim // w, 1)
    return max(w * max_dim // h, 1), max_dim


def to_luma601(img):
    """(..., 3|4) uint8 -> (...) uint8; a Luma8 array is returned as it is"""
    img = np.asarray(img, np.uint8)
    if img.ndim < 3 or img.shape[-1] not in (3, 4):
        return img
    v = img.astype(np.uint32)
    return ((299 * v[..., 0] + 587 * v[..., 1] + 114 * v[..., 2] + 500) // 1000).astype(np.uint8)


def _round_half_away(x):
    """llround of non-negative f64 values, without the rounding of x + 0.5"""
    f = np.floor(x)
    return (f + (x - f >= 0.5)).astype(np.int64)


def build_axis_plain(in_size, out_size):
    """one output after the other, as the algorithm is written down"""
    scale = in_size / out_size
    filter_scale = max(scale, 1.0)
    radius = 0.5 * filter_scale
    window = int(math.ceil(radius)) * 2 + 1
    recip = 1.0 / filter_scale
    start, size, weights, max_w = [], [], [], 0.0
    for o in range(out_size):
        in_center = (o + 0.5) * scale
        x_min = int(max(0.0, math.floor(in_center - radius)))
        x_max = int(min(float(in_size), math.ceil(in_center + radius)))
        center = in_center - 0.5
        ws = []
        bound_start, bound_end = x_min, x_max
        for x in range(x_min, x_max):
            t = (x - center) * recip
            v = 1.0 if -0.5 < t <= 0.5 else 0.0
            if x == bound_start and v == 0.0 and not ws:
                bound_start += 1
            else:
                ws.append(v)
        for v in reversed(ws):
            if bound_end <= bound_start or v != 0.0:
                break
            bound_end -= 1
        total = 0.0
        for v in ws:
            total += v
        if total != 0.0:
            ws = [v / total for v in ws]
        max_w = max([max_w] + ws)
        start.append(bound_start)
        size.append(bound_end - bound_start)
        weights.append(ws)
    precision = 0
    for cur in range(16):
        precision = cur
        if int(_round_half_away(np.float64(max_w * float(1 << (cur + 1))))) >= 1 << 15:
            break
    coef = np.zeros((out_size, window), np.int16)
    for o, ws in enumerate(weights):
        assert len(ws) <= window
        coef[o, :len(ws)] = _round_half_away(np.array(ws, np.float64) * float(1 << precision)) if ws else 0
    return Axis(np.array(start, np.int64), np.array(size, np.int64), coef, window, precision)


@functools.lru_cache(maxsize=None)
def build_axis(in_size, out_size):
    """the same tables with all outputs of the axis at once (the f64 operations are the same ones, in the same order)"""
    scale = np.float64(in_size) / np.float64(out_size)
    filter_scale = max(scale, np.float64(1.0))
    radius = np.float64(0.5) * filter_scale
    window = int(math.ceil(radius)) * 2 + 1
    recip = np.float64(1.0) / filter_scale
    o = np.arange(out_size, dtype=np.float64)
    in_center = (o + 0.5) * scale
    x_min = np.maximum(0.0, np.floor(in_center - radius)).astype(np.int64)
    x_max = np.minimum(np.float64(in_size), np.ceil(in_center + radius)).astype(np.int64)
    center = in_center - 0.5
    span = x_max - x_min
    assert span.max() <= window
    j = np.arange(window, dtype=np.int64)
    t = ((x_min[:, None] + j[None, :]).astype(np.float64) - center[:, None]) * recip
    inside = j[None, :] < span[:, None]
    v = np.where(inside & (t > -0.5) & (t <= 0.5), 1.0, 0.0)
    nz = v != 0.0
    lead = np.where(nz.any(1), nz.argmax(1), span)                 # zero weights in front: skipped, the bound moves up
    cnt = span - lead
    last = np.where(nz.any(1), window - 1 - nz[:, ::-1].argmax(1), lead - 1)
    size = np.where(cnt > 0, last - lead + 1, 0)                   # zero weights behind the last real one: cut
    start = x_min + lead
    idx = np.minimum(lead[:, None] + j[None, :], window - 1)
    ws = np.where(j[None, :] < cnt[:, None], np.take_along_axis(v, idx, 1), 0.0)
    total = np.zeros(out_size, np.float64)
    for k in range(window):                                        # (the sum in tap order)
        total = total + ws[:, k]
    ws = np.where((total != 0.0)[:, None], ws / np.where(total != 0.0, total, 1.0)[:, None], ws)
    max_w = ws.max() if ws.size else 0.0
    precision = 0
    for cur in range(16):
        precision = cur
        if int(_round_half_away(np.float64(max_w * float(1 << (cur + 1))))) >= 1 << 15:
            break
    coef = _round_half_away(ws * float(1 << precision)).astype(np.int16)
    return Axis(start, size, coef, window, precision)


def axis_info(in_size, out_size):
    """(precision, window, smallest, largest sum of an output's coefficients): what oracle.resize_axis_info reports"""
    a = build_axis(in_size, out_size)
    sums = np.where(np.arange(a.window)[None, :] < a.size[:, None], a.coef.astype(np.int64), 0).sum(1)
    return a.precision, a.window, int(sums.min()), int(sums.max())


def _convolve_rows(src, a):
    """along the last axis: src (..., in) uint8 -> (..., out) uint8"""
    in_size = src.shape[-1]
    j = np.arange(a.window)
    used = j[None, :] < a.size[:, None]
    idx = np.where(used, np.minimum(a.start[:, None] + j[None, :], in_size - 1), 0)
    k = np.where(used, a.coef.astype(np.int64), 0)
    acc = np.full(src.shape[:-1] + (len(a.start),), 1 << (a.precision - 1), np.int64)
    for t in range(a.window):  # exact integers, tap by tap
        acc += src[..., idx[:, t]].astype(np.int64) * k[:, t]
    return np.clip(acc >> a.precision, 0, 255).astype(np.uint8)


def resize_box_u8(luma, nw, nh):
    """(h, w) or (n, h, w) uint8 -> (..., nh, nw): horizontal pass into a u8 intermediate, then vertical"""
    luma = np.asarray(luma, np.uint8)
    h, w = luma.shape[-2:]
    tmp = _convolve_rows(luma, build_axis(w, nw))
    out = _convolve_rows(np.swapaxes(tmp, -1, -2), build_axis(h, nh))
    return np.ascontiguousarray(np.swapaxes(out, -1, -2))


# ---------------------------------------------------------------- geometries and their seams
# Where the device forms cut an axis (resize_kernels.hip): the matrix-pipe kernel owns 64 output columns (two blocks of 32) x 32 output
# rows and walks its source columns from x_lo = start & ~15 in K steps of 32 bytes (16 per lane half), loaded in groups of 6 steps, and
# its source rows in blocks of 32; the LDS kernel owns 64 output columns x 16 output rows and stages 4 x 4 source rows at a time.
Geometry = namedtuple("Geometry", "w h nw nh seams_x seams_y src_x src_y note")


def _axis_seams(a, in_size, out_block, task, src_step, align):
    """(output boundaries b: outputs b - 1 | b, source boundaries s: source positions s - 1 | s) of one axis"""
    n_out = len(a.start)
    outs = set(range(out_block, n_out, out_block))
    srcs = set()
    for o0 in range(0, n_out, task):
        o_last = min(o0 + task, n_out) - 1
        lo = int(a.start[o0]) & ~(align - 1)
        hi = min(int(a.start[o_last] + a.size[o_last]), in_size)
        for s in range(lo, hi, src_step):
            if 0 < s < in_size:
                srcs.add(s)
                # the outputs whose windows meet the step: the first one that ends behind s, and its neighbours
                b = int(np.searchsorted(a.start + a.size, s, side="right"))
                outs.update(x for x in (b, b + 1) if 0 < x < n_out)
    return sorted(outs), sorted(srcs)


@functools.lru_cache(maxsize=None)
def geometry(w, h, note=""):
    nw, nh = target_dimensions(w, h)
    ax, ay = build_axis(w, nw), build_axis(h, nh)
    seams_x, src_x = _axis_seams(ax, w, 32, 64, 16, 16)
    seams_y, src_y = _axis_seams(ay, h, 16, 16, 16, 1)
    return Geometry(w, h, nw, nh, tuple(seams_x), tuple(seams_y), tuple(src_x), tuple(src_y), note)


_WIDE = [(513, 41, "scale just above 1"), (768, 60, "3:2, window 3"), (1024, 80, "2:1, window 3"), (1280, 100, "2.5, window 5"),
         (1537, 120, "3, window 5"), (3020, 236, "5.9, window 7"), (3328, 260, "6.5, the general window"),
         (6144, 480, "12: an Rgba8 staged row exceeds 8 x 256 bytes, the two-pass form takes it")]
GEOMETRIES = ([geometry(w, h, n) for w, h, n in _WIDE] + [geometry(h, w, n + ", transposed") for w, h, n in _WIDE] +
              [geometry(4000, 5, "thumbnail of one row"), geometry(5, 4000, "thumbnail of one column"),
               geometry(1285, 650, "thumbnail 512 x 258: no multiple of 64 / 32")])


def geometry_id(g):
    return f"{g.w}x{g.h}"


# ---------------------------------------------------------------- contents
def _lit_positions(a, in_size, seams, src):
    """source positions of an axis that get a lone pixel: first and last source position of the outputs on either side of every output
    seam, the two positions on either side of every source seam, and the axis's two ends"""
    pos = {0, in_size - 1}
    for b in seams:
        for o in (b - 1, b):
            if 0 <= o < len(a.start) and a.size[o] > 0:
                pos.update((int(a.start[o]), int(a.start[o] + a.size[o] - 1)))
    for s in src:
        pos.update((s - 1, s))
    return sorted(p for p in pos if 0 <= p < in_size)


def _spread(positions, gap):
    """positions split into as few lists as the order allows such that two of one list are at least `gap` apart"""
    groups = []
    for p in positions:
        for g in groups:
            if p - g[-1] >= gap:
                g.append(p)
                break
        else:
            groups.append([p])
    return groups


def contents(rng, h, w, seams_x=(), seams_y=(), src_x=(), src_y=()):
    """A stack (n, h, w) of Luma8 images at the limits of the kernels' arithmetic (the matrix-pipe kernel sums bytes ^ 0x80 as signed
    bytes, so flat 0 / 255 drive its biased sums to their ends and 127 | 128 sits on the sign boundary), with lone pixels where the
    kernels cut the axes.  A lone pixel is alone in every window that holds it: the seam positions are spread over several images so
    that two pixels of one image are at least two windows apart on either axis.  Returns (stack, names)."""
    nw, nh = target_dimensions(w, h)
    ax, ay = build_axis(w, nw), build_axis(h, nh)
    yy, xx = np.mgrid[0:h, 0:w]
    imgs, names = [], []

    def add(name, a):
        imgs.append(np.broadcast_to(np.asarray(a), (h, w)).astype(np.uint8))
        names.append(name)

    add("all 0", 0)
    add("all 255", 255)
    add("left 127 | right 128", np.where(xx < w // 2, 127, 128))
    add("top 127 | bottom 128", np.where(yy < h // 2, 127, 128))
    add("checkerboard", ((xx + yy) & 1) * 255)
    add("vertical stripes", (xx & 1) * 255)
    add("horizontal stripes", (yy & 1) * 255)
    add("vertical stripes of the window's period", ((xx // max(1, ax.window // 2)) & 1) * 255)
    add("horizontal stripes of the window's period", ((yy // max(1, ay.window // 2)) & 1) * 255)
    add("vertical stripes, period = window", (xx % ax.window == 0) * 255)
    add("horizontal stripes, period = window", (yy % ay.window == 0) * 255)
    frame = (xx < 2) | (xx >= w - 2) | (yy < 2) | (yy >= h - 2)
    add("frame of 255 on 0", frame * 255)
    add("frame of 0 on 255", ~frame * 255)
    corners = np.zeros((h, w), bool)
    corners[[0, 0, h - 1, h - 1], [0, w - 1, 0, w - 1]] = True
    add("corners 255 on 0", corners * 255)
    add("corners 0 on 255", ~corners * 255)
    gx = _spread(_lit_positions(ax, w, seams_x, src_x), 2 * ax.window)
    gy = _spread(_lit_positions(ay, h, seams_y, src_y), 2 * ay.window)
    for g in range(max(len(gx), len(gy))):
        xs, ys = gx[g % len(gx)], gy[g % len(gy)]
        k = np.arange(max(len(xs), len(ys)))
        dots = np.zeros((h, w), bool)
        dots[np.array(ys)[k % len(ys)], np.array(xs)[k % len(xs)]] = True
        add(f"seam pixels {g} 255 on 0", dots * 255)
        add(f"seam pixels {g} 0 on 255", ~dots * 255)
    add("noise from {0, 255}", rng.integers(0, 2, (h, w)) * 255)
    add("noise from {127, 128}", rng.integers(127, 129, (h, w)))
    add("uniform noise", rng.integers(0, 256, (h, w)))
    add("gradient", (xx * 200) // max(w - 1, 1) + (yy * 55) // max(h - 1, 1))
    return np.stack(imgs), names


def colour(imgs, ch, rng=None):
    """A Luma8 stack (n, h, w) spread into Rgb8 / Rgba8 whose channels differ: R = the image, G = the image reversed in x, B = the image
    reversed in y, A = noise.  The luma of the result mixes all three, so a kernel that copied one channel would be wrong."""
    if ch == 1:
        return imgs
    out = np.empty(imgs.shape + (ch,), np.uint8)
    out[..., 0] = imgs
    out[..., 1] = imgs[:, :, ::-1]
    out[..., 2] = imgs[:, ::-1, :]
    if ch == 4:
        out[..., 3] = (rng or np.random.default_rng(4)).integers(0, 256, imgs.shape, dtype=np.uint8)
    return out


@functools.lru_cache(maxsize=None)
def content_stack(g):
    """the content stack of a geometry (built once, shared, never written to) and its names"""
    imgs, names = contents(np.random.default_rng(g.w * 8191 + g.h), g.h, g.w, g.seams_x, g.seams_y, g.src_x, g.src_y)
    imgs.setflags(write=False)
    return imgs, names


def first_difference(got, want, names=None):
    """None, or a sentence naming the first differing byte of two (n, rows, cols) stacks"""
    if got.shape != want.shape:
        return f"shapes differ: {got.shape} and {want.shape}"
    bad = np.argwhere(got != want)
    if not len(bad):
        return None
    k, r, c = (int(v) for v in bad[0])
    what = f" ({names[k]})" if names else ""
    return f"image {k}{what} row {r} column {c}: got {got[k, r, c]}, want {want[k, r, c]} ({len(bad)} bytes differ in {len(set(bad[:, 0]))} images)"
