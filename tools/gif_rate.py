#!/usr/bin/env python3
"""tools/gif_rate.py -- rph_gif_pdq_hash_batch rates on corpora of distinct files, each in DEVICE and HOST decompress mode (--threads host
threads), plus a --threads Pillow decode as the CPU baseline.  Corpora, each at 512x512 and 1920x1080, written by Pillow's GIF encoder:
photographs quantised to 256 colours with Floyd-Steinberg dithering; screenshots (flat panels, windows, rows of text-like marks, 16
colours); flat graphics (a few large shapes, 8 colours).  Every corpus is reported with its expansion ratio: palette indices per byte of
the frames' joined LZW streams, the figure AUTO decides by.

    python tools/gif_rate.py [--small N] [--large N] [--threads 16] [--reps 3]
"""
import argparse
import io
import os
import sys
import time
import zlib
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


def _flat(rng, w, h):
    img = np.zeros((h, w), np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    for _ in range(6):
        cx, cy, r = rng.integers(0, w), rng.integers(0, h), rng.integers(h // 8, h // 2)
        img[(xx - cx) ** 2 + (yy - cy) ** 2 < r * r] = rng.integers(0, 8)
    return img


def make(args):
    from PIL import Image

    kind, w, h, k = args
    rng = np.random.default_rng(zlib.crc32(f"{kind}{w}".encode()) % 100003 + 1000 * k)
    if kind == "photo":
        im = Image.fromarray(_photo(rng, w, h)).quantize(colors=256, dither=Image.Dither.FLOYDSTEINBERG)
    else:
        idx = (_screen if kind == "screen" else _flat)(rng, w, h)
        im = Image.frombytes("P", (w, h), idx.tobytes())
        im.putpalette(np.random.default_rng(k).integers(0, 256, 48, dtype=np.uint8).tobytes())
    buf = io.BytesIO()
    im.save(buf, format="GIF", optimize=False)
    return buf.getvalue()


def stream_bytes(d):
    """the bytes of the first frame's data sub-blocks (a file Pillow wrote: nothing is checked)"""
    pos = 13 + (3 * (2 << (d[10] & 7)) if d[10] & 0x80 else 0)
    while d[pos] == 0x21:
        pos += 2
        while d[pos]:
            pos += 1 + d[pos]
        pos += 1
    flags = d[pos + 9]
    pos += 11 + (3 * (2 << (flags & 7)) if flags & 0x80 else 0)
    n = 0
    while d[pos]:
        n += d[pos]
        pos += 1 + d[pos]
    return n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--small", type=int, default=1500, help="files per 512x512 corpus")
    ap.add_argument("--large", type=int, default=96, help="files per 1920x1080 corpus")
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    from concurrent.futures import ThreadPoolExecutor

    from PIL import Image

    from rupphash_amd import Engine

    pool = Pool(a.threads)  # (the workers are started before the device is opened: they never hold it)
    eng = Engine(0)
    for kind in ("photo", "screen", "flat"):
        for w, h, n in ((512, 512, a.small), (1920, 1080, a.large)):
            if not n:
                continue
            files = pool.map(make, [(kind, w, h, k) for k in range(n)], chunksize=max(1, n // (4 * a.threads)))
            fl = eng.jpeg_file_list(files)
            px_bytes = n * w * h * 4
            comp = sum(stream_bytes(f) for f in files)
            print(f"{kind}_{w}x{h}: {n} distinct files, {sum(map(len, files)) / 1e6:.1f} MB of files, {px_bytes / 1e9:.2f} GB decoded pixels, "
                  f"expansion {n * w * h / comp:.1f}:1 (indices per stream byte)", flush=True)
            ref = None
            for mode, name in ((1, "DEVICE"), (0, "HOST")):
                eng.gif_set_decompress(mode)
                eng.gif_pdq_hash_batch(fl, threads=a.threads)  # warm: buffers allocated
                ts = []
                for _ in range(a.reps):
                    t0 = time.perf_counter()
                    out = eng.gif_pdq_hash_batch(fl, threads=a.threads)
                    ts.append(time.perf_counter() - t0)
                assert not out["status"].any()
                if ref is None:
                    ref = out["hash"]
                assert np.array_equal(ref, out["hash"]), "modes disagree"
                t = min(ts)
                print(f"  {name:6s} {n / t:9.1f} files/s  {px_bytes / t / 1e9:6.2f} GB/s of pixels  ({t * 1e3:.0f} ms, best of {a.reps}; median {sorted(ts)[len(ts) // 2] * 1e3:.0f} ms)",
                      flush=True)

            def pil(f):
                im = Image.open(io.BytesIO(f))
                im.load()
                return im.size

            with ThreadPoolExecutor(a.threads) as ex:
                list(ex.map(pil, files[:16]))
                t0 = time.perf_counter()
                list(ex.map(pil, files))
                t = time.perf_counter() - t0
            print(f"  Pillow {n / t:9.1f} files/s  {px_bytes / t / 1e9:6.2f} GB/s of pixels  ({a.threads} threads)", flush=True)
            eng.gif_release()
    eng.gif_set_decompress(2)
    eng.close()
    pool.close()
    pool.join()


if __name__ == "__main__":
    main()
