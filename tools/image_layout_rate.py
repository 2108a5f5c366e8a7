#!/usr/bin/env python3
"""tools/image_layout_rate.py -- what rph_image_hash_ragged_dev (PDQ outputs + pixel hashes of decoded images of any mix of sizes and
layouts, one call) costs against the routes that existed before it.  Pixels resident in HBM (uploaded once); device events around each
contender's whole work, the host's planning and launching included; every contender warmed up by an untimed pass, repetitions chosen
so that a timed window is at least ~0.2 s; the contenders alternate, three times; identical outputs asserted (a 16-bit picture here
is its 8-bit picture times 257, so its hasher pixels, its RGBA16 stream and therefore both hashes are the 8-bit picture's).

  corpus 1  1 024 pictures, every geometry distinct, sides uniform in 128..512 (picture i: the top-left w x h of one of 64 fields of 512x512)
            a  the new call on the Rgb16 pictures, PDQ + pixel hash
            b  the new call on the Rgb8 pictures, PDQ + pixel hash
            c  the route before it on the Rgb8 pictures: rph_pdq_hash_ragged_dev + rph_pixel_hash_batch_dev once per geometry
  corpus 2  64 pictures of 2000x1500, one geometry: a, b, c as above (c: one call each)
  corpus 3  one geometry of Rgb8, pixel hashes only: b3_pixels_ragged_kernel (the new call without PDQ outputs) against
            rph_pixel_hash_batch_dev -- 1 024 x 512x512 and the 64 x 2000x1500 of corpus 2: the price of the descriptor
  corpus 4  corpus 1 cut to its first n = 1, 2, 4 .. 256 pictures, pixel hashes only, Rgb8: where the ragged pixel hash passes the
            per-geometry one

usage: image_layout_rate.py [corpus ...]   (default: 1 2 3 4)"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from rupphash_amd import Engine

eng = Engine(0)
which = [int(a) for a in sys.argv[1:]] or [1, 2, 3, 4]
ROUNDS = 3


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


class Pictures:
    """n pictures as Rgb8 and as Rgb16 (= Rgb8 x 257) in two device buffers: picture i is the top-left w[i] x h[i] of field i % fields"""

    def __init__(self, fields, fw, fh, w, h, seed, copies=1):
        rng = np.random.default_rng(seed)
        y, x = np.mgrid[0:fh, 0:fw]
        host8 = np.empty((fields, fh, fw, 3), np.uint8)
        for k in range(fields):  # a smooth picture + noise: quality well above 0
            a, b, c = rng.uniform(0.2, 1.0, 3)
            base = 128 + 60 * np.sin(x * a * 6.283 / fw * 3) + 50 * np.cos(y * b * 6.283 / fh * 2) + 20 * c
            host8[k] = np.clip(base[:, :, None] + rng.integers(-20, 21, (fh, fw, 3)), 0, 255).astype(np.uint8)
        host16 = host8.astype(np.uint16) * 257
        self.n, self.w, self.h = len(w), np.asarray(w, np.uint32), np.asarray(h, np.uint32)
        self.field8, self.field16 = fw * fh * 3, fw * fh * 6
        total = fields * copies
        self.d8, self.d16 = eng.dev_alloc(total * self.field8 + 16), eng.dev_alloc(total * self.field16 + 16)
        for c in range(copies):
            eng.dev_upload(self.d8 + c * fields * self.field8, host8)
            eng.dev_upload(self.d16 + c * fields * self.field16, host16)
        eng.synchronize()
        at = np.arange(self.n, dtype=np.uint64) % np.uint64(total)
        self.off8, self.off16 = at * np.uint64(self.field8), at * np.uint64(self.field16)
        self.rs8, self.rs16 = np.full(self.n, fw * 3, np.uintp), np.full(self.n, fw * 6, np.uintp)
        self.l8, self.l16 = np.full(self.n, 3, np.uint32), np.full(self.n, 19, np.uint32)
        # outputs of up to three contenders
        self.d_hash = [eng.dev_alloc(self.n * 32) for _ in range(3)]
        self.d_q = [eng.dev_alloc(self.n * 4) for _ in range(3)]
        self.d_ph = [eng.dev_alloc(self.n * 32) for _ in range(3)]

    def runs(self, n):
        """(first, count, image stride) of the runs of one geometry at one distance among the first n Rgb8 pictures"""
        out, i = [], 0
        key = lambda k: (self.w[k], self.h[k])
        while i < n:
            j, stride = i + 1, 0
            if j < n and key(j) == key(i) and self.off8[j] > self.off8[i]:
                stride = int(self.off8[j] - self.off8[i])
                while j < n and key(j) == key(i) and int(self.off8[j]) == int(self.off8[i]) + (j - i) * stride:
                    j += 1
            out.append((i, j - i, stride))
            i = j
        return out

    def new16(self, n, slot, pdq=True):
        eng.image_hash_ragged_dev(self.d16, self.off16[:n], self.w[:n], self.h[:n], self.l16[:n], self.rs16[:n], self.d_hash[slot] if pdq else None,
                                  self.d_q[slot] if pdq else None, d_pixel_hash=self.d_ph[slot])

    def new8(self, n, slot, pdq=True):
        eng.image_hash_ragged_dev(self.d8, self.off8[:n], self.w[:n], self.h[:n], self.l8[:n], self.rs8[:n], self.d_hash[slot] if pdq else None,
                                  self.d_q[slot] if pdq else None, d_pixel_hash=self.d_ph[slot])

    def before(self, n, slot, runs, pdq=True):
        if pdq:
            eng.pdq_hash_ragged_dev(self.d8, self.off8[:n], self.w[:n], self.h[:n], self.l8[:n], self.rs8[:n], self.d_hash[slot], self.d_q[slot])
        for first, count, stride in runs:
            eng.pixel_hash_batch_dev(self.d8 + int(self.off8[first]), count, int(self.w[first]), int(self.h[first]), 3, self.d_ph[slot] + first * 32,
                                     row_stride=int(self.rs8[first]), image_stride=stride or None)

    def outputs(self, n, slot, pdq=True):
        a, q, p = np.zeros((n, 32), np.uint8), np.zeros(n, np.float32), np.zeros((n, 32), np.uint8)
        if pdq:
            eng.dev_download(a, self.d_hash[slot], n * 32)
            eng.dev_download(q, self.d_q[slot], n * 4)
        eng.dev_download(p, self.d_ph[slot], n * 32)
        return a.tobytes() + q.tobytes() + p.tobytes()

    def free(self):
        for p in [self.d8, self.d16] + self.d_hash + self.d_q + self.d_ph:
            eng.dev_free(p)


def contest(name, n, contenders, same):
    """contenders: [(label, work)]; warm-up, the outputs compared by same(), then ROUNDS alternations"""
    for _, work in contenders:
        work()
    eng.synchronize()
    assert same(), f"{name}: the contenders' outputs differ"
    reps = max(1, int(200.0 / max(timed(contenders[-1][1], 1), 1e-3)))
    times = [[] for _ in contenders]
    for _ in range(ROUNDS):
        for t, (_, work) in zip(times, contenders):
            t.append(timed(work, reps))
    print(f"{name}  n={n}  ({reps} repetitions per window)", flush=True)
    for t, (label, _) in zip(times, contenders):
        print(f"    {label:58s} {min(t):9.3f}..{max(t):9.3f} ms  {n / min(t) * 1e3:11.0f} images/s", flush=True)
    last = times[-1]
    for t, (label, _) in zip(times[:-1], contenders[:-1]):
        r = [y / x for x, y in zip(t, last)]
        print(f"    {label.split(':')[0]} against {contenders[-1][0].split(':')[0]}: faster by {min(r):6.2f}..{max(r):6.2f} x", flush=True)


def three_way(name, P, n):
    runs = P.runs(n)
    contest(name, n, [("a: new call, Rgb16, PDQ + pixel hash", lambda: P.new16(n, 0)),
                      ("b: new call, Rgb8, PDQ + pixel hash", lambda: P.new8(n, 1)),
                      (f"c: pdq_hash_ragged_dev + {len(runs)} x pixel_hash_batch_dev, Rgb8", lambda: P.before(n, 2, runs))],
            lambda: P.outputs(n, 0) == P.outputs(n, 1) == P.outputs(n, 2))


def pixel_only(name, P, n):
    runs = P.runs(n)
    contest(name, n, [("b: new call, Rgb8, pixel hash only", lambda: P.new8(n, 1, pdq=False)),
                      (f"c: {len(runs)} x pixel_hash_batch_dev, Rgb8", lambda: P.before(n, 2, runs, pdq=False))],
            lambda: P.outputs(n, 1, pdq=False) == P.outputs(n, 2, pdq=False))


if 1 in which or 4 in which or 3 in which:
    N = 1024
    rng = np.random.default_rng(1)
    geos = set()
    while len(geos) < N:
        geos.add((int(rng.integers(128, 513)), int(rng.integers(128, 513))))
    geos = [tuple(g) for g in rng.permutation(sorted(geos))]
    P = Pictures(64, 512, 512, [g[0] for g in geos], [g[1] for g in geos], seed=11, copies=16)
    if 1 in which:
        three_way("1: 1024 distinct 128..512", P, N)
    if 4 in which:
        n = 1
        while n <= 256:
            pixel_only("4: corpus 1, first n, pixel hash only", P, n)
            n *= 2
    if 3 in which:
        P.w[:] = 512
        P.h[:] = 512
        pixel_only("3: 1024 x 512x512 Rgb8, one geometry, pixel hash only", P, N)
    P.free()

if 2 in which or 3 in which:
    N = 64
    P = Pictures(8, 2000, 1500, [2000] * N, [1500] * N, seed=12, copies=8)
    if 2 in which:
        three_way("2: 64 x 2000x1500", P, N)
    if 3 in which:
        pixel_only("3: 64 x 2000x1500 Rgb8, one geometry, pixel hash only", P, N)
    P.free()

eng.close()
