#!/usr/bin/env python3
"""tools/bmp_rate.py -- rph_bmp_pdq_hash_batch (PDQ + pixel hashes of BMP files) against the fastest route the library had for the same
files before it: Pillow decoding on --threads threads, then rph_image_hash_ragged from host memory.  Both are measured in the same run,
alternating, on corpora of distinct files written by Pillow's BMP encoder: 24-bit 512x512 photographs, 24-bit 1920x1080 screenshots,
24-bit files of distinct sizes 128 .. 512 px, and 8-bit palette files (512x512 screenshots).  The hashes of the two routes are compared.

    python tools/bmp_rate.py [--small N] [--large N] [--ragged N] [--threads 16] [--reps 3] [--out profiles/bmp_rate.txt]
"""
import argparse
import io
import os
import sys
import time
from multiprocessing import Pool

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _photo(rng, w, h):
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    ph = rng.uniform(0, 6.28, 3)
    img = np.stack([127 + 60 * np.sin(xx / (37 + 5 * c) + ph[c]) * np.cos(yy / (53 + 3 * c)) + 30 * np.sin((xx + yy) / 11.0 + ph[c]) for c in range(3)], -1)
    return np.clip(img + rng.normal(0, 6, img.shape), 0, 255).astype(np.uint8)


def _screen(rng, w, h):
    img = np.zeros((h, w), np.uint8)
    img[:] = rng.integers(0, 4)
    for _ in range(w * h // 50000):
        x0, y0 = rng.integers(0, w - 40), rng.integers(0, h - 40)
        img[y0:y0 + rng.integers(10, h // 4), x0:x0 + rng.integers(10, w // 4)] = rng.integers(0, 16)
    for _ in range(w * h // 7000):
        x0, y0 = rng.integers(0, w - 20), rng.integers(0, h - 10)
        img[y0:y0 + 9, x0:x0 + rng.integers(2, 20)] = rng.integers(0, 16)
    return img


def make(args):
    from PIL import Image

    kind, w, h, k = args
    rng = np.random.default_rng([k, w, h])
    if kind == "photo":
        im = Image.fromarray(_photo(rng, w, h))
    else:
        im = Image.frombytes("P", (w, h), _screen(rng, w, h).tobytes())
        im.putpalette(np.random.default_rng(k).integers(0, 256, 48, dtype=np.uint8).tobytes())
        if kind == "screen24":
            im = im.convert("RGB")
    buf = io.BytesIO()
    im.save(buf, format="BMP")
    return buf.getvalue()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--small", type=int, default=1500, help="files per 512x512 corpus")
    ap.add_argument("--large", type=int, default=96, help="files of the 1920x1080 corpus")
    ap.add_argument("--ragged", type=int, default=3000, help="files of the corpus of distinct sizes")
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from concurrent.futures import ThreadPoolExecutor

    from PIL import Image

    from rupphash_amd import Engine

    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    pool = Pool(a.threads)  # (the workers are started before the device is opened: they never hold it)
    eng = Engine(0)
    say(f"# {' '.join(['tools/bmp_rate.py'] + sys.argv[1:])} on {eng.device_info()[0]}")
    sizes = np.random.default_rng(3)
    ragged = [("photo", int(sizes.integers(128, 513)), int(sizes.integers(128, 513)), k) for k in range(a.ragged)]
    corpora = (("photo24_512x512", [("photo", 512, 512, k) for k in range(a.small)]),
               ("screen24_1920x1080", [("screen24", 1920, 1080, k) for k in range(a.large)]),
               ("photo24_distinct_sizes_128_512", ragged),
               ("palette8_512x512", [("screen8", 512, 512, k) for k in range(a.small)]))

    def pil(f):
        im = Image.open(io.BytesIO(f))
        return np.asarray(im if im.mode == "RGB" else im.convert("RGB"))

    for name, jobs in corpora:
        n = len(jobs)
        if not n:
            continue
        files = pool.map(make, jobs, chunksize=max(1, n // (4 * a.threads)))
        fl = eng.jpeg_file_list(files)
        px_bytes = sum(w * h * 3 for _, w, h, _ in jobs)
        say(f"{name}: {n} distinct files, {len(set((w, h) for _, w, h, _ in jobs))} sizes, {sum(map(len, files)) / 1e6:.1f} MB of files, {px_bytes / 1e9:.2f} GB of Rgb8 pixels")
        t_new, t_old = [], []
        with ThreadPoolExecutor(a.threads) as ex:
            for rep in range(a.reps + 1):  # (the first round warms both routes: buffers allocated)
                t0 = time.perf_counter()
                new = eng.bmp_pdq_hash_batch(fl, threads=a.threads, want_pixel_hash=True)
                t1 = time.perf_counter()
                old = eng.image_hash_ragged(list(ex.map(pil, files)))
                t2 = time.perf_counter()
                if rep:
                    t_new.append(t1 - t0)
                    t_old.append(t2 - t1)
        assert not new["status"].any() and new["valid"].all()
        assert np.array_equal(new["hash"], old["hash"]) and np.array_equal(new["pixel_hash"], old["pixel_hash"]), "the routes disagree"
        for label, ts in (("rph_bmp_pdq_hash_batch", t_new), (f"Pillow x{a.threads} + image_hash_ragged", t_old)):
            t = min(ts)
            say(f"  {label:34s} {n / t:9.1f} files/s  {px_bytes / t / 1e9:6.2f} GB/s of pixels  ({t * 1e3:.0f} ms, best of {a.reps}; median {sorted(ts)[len(ts) // 2] * 1e3:.0f} ms)")
        say(f"  ratio new / old: {min(t_old) / min(t_new):.2f}x")
        eng.bmp_release()
    eng.close()
    pool.close()
    pool.join()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
