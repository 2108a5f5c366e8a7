#!/usr/bin/env python3
"""tools/ragged_rate.py -- images/s of rph_pdq_hash_ragged_dev (one call for images of any mix of geometries, csrc/pdq_ragged.hip) against
the same images as runs of equal geometry through rph_pdq_hash_batch_dev on one stream (what the one-image queue and the file pipelines
do with mixed sizes).  Pixels resident in HBM, generated there (rph_synth_images_dev, seeded); device events around each contender's
work, which includes the host's planning and launching (the stream idles while the host prepares the next launch); every shape warmed
up by an untimed pass of both contenders; the contenders alternate, three times; identical outputs asserted.

  corpus 1  4 096 Rgb8 images, every geometry distinct, sides uniform in 128..512 (image i: the top-left w x h of its own 512x512 field)
  corpus 2  4 096 Rgb8 photos over 64 geometries between 800x600 and 4000x3000, drawn unevenly (image i: the top-left w x h of one of
            256 fields of 4000x3000, sorted by geometry so that the runs of the per-geometry contender are as long as they can be)
  corpus 3  4 096 x 512x344 Luma8, one geometry: the uniform call against the ragged kernels, forced by one appended 500x344 image
  corpus 4  corpus 1 cut to its first n = 2, 4 .. 256 images: where the ragged call overtakes the per-geometry runs

usage: ragged_rate.py [corpus ...]   (default: 1 2 3 4)"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from rupphash_amd import Engine

eng = Engine(0)
which = [int(a) for a in sys.argv[1:]] or [1, 2, 3, 4]
ROUNDS = 3


class Corpus:
    """n images in one device buffer: image i at offset[i], w[i] x h[i] x ch[i], rows row_stride[i] apart"""

    def __init__(self, d_px, offset, w, h, ch, rs):
        self.d_px, self.n = d_px, len(offset)
        self.offset, self.w, self.h, self.ch = np.asarray(offset, np.uint64), np.asarray(w, np.uint32), np.asarray(h, np.uint32), np.asarray(ch, np.uint32)
        self.rs = np.asarray(rs, np.uintp)
        self.d_hash = [eng.dev_alloc(self.n * 32) for _ in range(2)]
        self.d_q = [eng.dev_alloc(self.n * 4) for _ in range(2)]

    def runs(self, n):
        """[first, count, image stride) of the runs of equal geometry at one distance among the first n images"""
        out, i = [], 0
        key = lambda k: (self.w[k], self.h[k], self.ch[k], self.rs[k])
        while i < n:
            j, stride = i + 1, 0
            if j < n and key(j) == key(i) and self.offset[j] > self.offset[i]:
                stride = int(self.offset[j] - self.offset[i])
                while j < n and key(j) == key(i) and int(self.offset[j]) == int(self.offset[i]) + (j - i) * stride:
                    j += 1
            out.append((i, j - i, stride))
            i = j
        return out

    def ragged(self, n):
        eng.pdq_hash_ragged_dev(self.d_px, self.offset[:n], self.w[:n], self.h[:n], self.ch[:n], self.rs[:n], self.d_hash[0], self.d_q[0])

    def per_geometry(self, n, runs):
        for first, count, stride in runs:
            eng.pdq_hash_batch_dev(self.d_px + int(self.offset[first]), count, int(self.w[first]), int(self.h[first]), int(self.ch[first]),
                                   self.d_hash[1] + first * 32, self.d_q[1] + first * 4, row_stride=int(self.rs[first]), image_stride=stride or None)

    def same_outputs(self, n):
        a, b = np.zeros((2, n, 32), np.uint8), np.zeros((2, n), np.float32)
        for k in range(2):
            eng.dev_download(a[k], self.d_hash[k], n * 32)
            eng.dev_download(b[k], self.d_q[k], n * 4)
        return np.array_equal(a[0], a[1]) and np.array_equal(b[0].view(np.uint32), b[1].view(np.uint32))

    def free(self):
        for p in self.d_hash + self.d_q:
            eng.dev_free(p)


def timed(work, reps):
    """ms per repetition of work() by device events on the context's stream"""
    e0, e1 = eng.event(), eng.event()
    eng.synchronize()
    eng.event_record(e0)
    for _ in range(reps):
        work()
    eng.event_record(e1)
    ms = eng.event_elapsed_ms(e0, e1) / reps
    eng.event_destroy(e0)
    eng.event_destroy(e1)
    return ms


def contest(name, c, n, reps=1, other=None):
    """the ragged call against the per-geometry runs (or `other`) on the first n images: warm-up, ROUNDS alternations"""
    runs = c.runs(n)
    a = lambda: c.ragged(n)
    b = other or (lambda: c.per_geometry(n, runs))
    a(), b()
    eng.synchronize()
    if other is None:
        assert c.same_outputs(n), f"{name}: the contenders' outputs differ"
    ta, tb = [], []
    for _ in range(ROUNDS):
        ta.append(timed(a, reps))
        tb.append(timed(b, reps))
    ratios = [y / x for x, y in zip(ta, tb)]
    calls = len(runs) if other is None else 1
    print(f"{name:34s} n={n:5d}  ragged {min(ta):9.3f}..{max(ta):9.3f} ms ({n / min(ta) * 1e3:10.0f} images/s)   "
          f"{'per-geometry' if other is None else 'uniform'} ({calls:4d} calls) {min(tb):9.3f}..{max(tb):9.3f} ms ({n / min(tb) * 1e3:10.0f} images/s)   "
          f"ragged faster by {min(ratios):6.2f}..{max(ratios):6.2f} x", flush=True)
    return ratios


FIELD = 512 * 512 * 3
N = 4096

if 1 in which or 3 in which or 4 in which:
    d_fields = eng.dev_alloc(N * FIELD + 16)
    eng.synth_images_dev(d_fields, 0, N, 512, 512, seed=0x5EED2026)
    eng.synchronize()

if 1 in which or 4 in which:
    rng = np.random.default_rng(1)
    geos = set()
    while len(geos) < N:
        geos.add((int(rng.integers(128, 513)), int(rng.integers(128, 513))))
    geos = [tuple(g) for g in rng.permutation(sorted(geos))]
    c1 = Corpus(d_fields, [i * FIELD for i in range(N)], [g[0] for g in geos], [g[1] for g in geos], [3] * N, [1536] * N)
    if 1 in which:
        contest("1: 4096 distinct 128..512 Rgb8", c1, N)
    if 4 in which:
        n = 2
        while n <= 256:
            contest("4: corpus 1, first n", c1, n, reps=max(1, 256 // n))
            n *= 2
    c1.free()

if 3 in which:
    w, h = 512, 344
    per = w * h
    off = [i * per for i in range(N)] + [N * per]
    c3 = Corpus(d_fields, off, [w] * N + [500], [h] * (N + 1), [1] * (N + 1), [w] * (N + 1))
    uniform = lambda: eng.pdq_hash_batch_dev(d_fields, N, w, h, 1, c3.d_hash[1], c3.d_q[1])
    contest("3: 4096 x 512x344 Luma8 (+ 1 odd)", c3, N + 1, other=uniform)
    assert c3.same_outputs(N)
    c3.free()

if 1 in which or 3 in which or 4 in which:
    eng.dev_free(d_fields)

if 2 in which:
    BW, BH, NB = 4000, 3000, 256
    big = BW * BH * 3
    d_big = eng.dev_alloc(NB * big + 16)
    for k in range(0, NB, 16):
        eng.synth_images_dev(d_big + k * big, k, 16, BW, BH, seed=0xF070)
    eng.synchronize()
    rng = np.random.default_rng(2)
    geos = set()
    while len(geos) < 64:
        if rng.random() < 0.7:  # landscape
            geos.add((int(rng.integers(800, 4001)), int(rng.integers(600, 3001))))
        else:  # portrait
            geos.add((int(rng.integers(600, 3001)), int(rng.integers(800, 3001))))
    geos = sorted(geos)
    weight = 1.0 / np.arange(1, 65) ** 1.1  # a few cameras take most of the photos, many sizes occur a few times
    pick = np.sort(rng.choice(64, N, p=weight / weight.sum()))
    c2 = Corpus(d_big, [(i % NB) * big for i in range(N)], [geos[k][0] for k in pick], [geos[k][1] for k in pick], [3] * N, [BW * 3] * N)
    from rupphash_amd.pdqhash import calculate_target_dimensions

    thin = sum(min(calculate_target_dimensions(*geos[k])) < 128 for k in pick)  # thumbnails the descriptor kernels leave to the uniform path
    print(f"2: {len(set(pick.tolist()))} geometries drawn, {np.mean([geos[k][0] * geos[k][1] for k in pick]) / 1e6:.1f} Mpx mean, {thin} images with a thumbnail side < 128",
          flush=True)
    contest("2: 4096 photos, 64 geometries Rgb8", c2, N)
    c2.free()
    eng.dev_free(d_big)

eng.close()
