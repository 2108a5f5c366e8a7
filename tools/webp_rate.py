#!/usr/bin/env python3
"""tools/webp_rate.py -- rph_webp_pdq_hash_batch rates on three corpora of distinct lossless files written by libwebp (Pillow, method 2):
photographic 512x512 RGB, screenshot-like 1920x1080 RGBA, and palette images of 200-600 px.  Each corpus in DEVICE and HOST entropy
mode (--threads host threads), plus a --threads Pillow decode as the CPU baseline.  Prints files/s and GB/s of decoded pixels; the PCIe
share is timed separately by uploading the bytes each mode moves (compressed for DEVICE, ARGB words for HOST).

    python tools/webp_rate.py [--photo N] [--screen N] [--palette N] [--threads 16] [--reps 3]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _webp(img, mode):
    from PIL import Image

    buf = io.BytesIO()
    Image.fromarray(img, mode).save(buf, format="WEBP", lossless=True, exact=True, method=2, quality=50)
    return buf.getvalue()


def make(args):
    kind, k = args
    rng = np.random.default_rng(1000003 * (kind == "screen") + 7 * (kind == "palette") + k)
    if kind == "photo":  # smooth gradients + texture + noise, distinct per file
        yy, xx = np.mgrid[0:512, 0:512].astype(np.float32)
        ph = rng.uniform(0, 6.28, 3)
        img = np.stack([127 + 60 * np.sin(xx / (37 + 5 * c) + ph[c]) * np.cos(yy / (53 + 3 * c)) + 30 * np.sin((xx + yy) / 11.0 + ph[c]) for c in range(3)], -1)
        img = np.clip(img + rng.normal(0, 6, img.shape), 0, 255).astype(np.uint8)
        return _webp(img, "RGB")
    if kind == "screen":  # flat panels, text-like strokes
        img = np.full((1080, 1920, 4), 255, np.uint8)
        img[:, :, :3] = rng.integers(200, 256, 3)
        for _ in range(40):
            x0, y0 = rng.integers(0, 1800), rng.integers(0, 1000)
            img[y0:y0 + rng.integers(10, 200), x0:x0 + rng.integers(10, 400), :3] = rng.integers(0, 256, 3)
        for _ in range(300):
            x0, y0 = rng.integers(0, 1900), rng.integers(0, 1070)
            img[y0:y0 + 9, x0:x0 + rng.integers(2, 20), :3] = rng.integers(0, 80)
        return _webp(img, "RGBA")
    w, h = int(rng.integers(200, 600)), int(rng.integers(200, 600))
    idx = ((np.add.outer(np.arange(h) // 8, np.arange(w) // 13) + rng.integers(0, 3, (h, w))) % 200).astype(np.uint8)
    return _webp(rng.integers(0, 256, (200, 3)).astype(np.uint8)[idx], "RGB")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--photo", type=int, default=4000)
    ap.add_argument("--screen", type=int, default=300)
    ap.add_argument("--palette", type=int, default=4000)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    from concurrent.futures import ThreadPoolExecutor

    from PIL import Image

    from rupphash_amd import Engine

    eng = Engine(0)
    with Pool(a.threads) as pool:
        corpora = [(kind, pool.map(make, [(kind, k) for k in range(n)], chunksize=16)) for kind, n in
                   (("photo", a.photo), ("screen", a.screen), ("palette", a.palette)) if n]
    for kind, files in corpora:
        fl = eng.jpeg_file_list(files)
        info = [Engine.webp_info(f) for f in files]
        px_bytes = sum(w * h * c for w, h, c, _ in info)
        comp = sum(len(f) for f in files)
        print(f"{kind}: {len(files)} distinct files, {comp / 1e6:.1f} MB compressed, {px_bytes / 1e9:.2f} GB decoded pixels", flush=True)
        ref = None
        for mode, name in ((1, "DEVICE"), (0, "HOST")):
            eng.webp_set_entropy(mode)
            eng.webp_pdq_hash_batch(fl, threads=a.threads)  # warm: buffers allocated
            ts = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                out = eng.webp_pdq_hash_batch(fl, threads=a.threads)
                ts.append(time.perf_counter() - t0)
            assert not out["status"].any()
            if ref is None:
                ref = out["hash"]
            assert np.array_equal(ref, out["hash"]), "modes disagree"
            t = min(ts)
            print(f"  {name:6s} {len(files) / t:9.0f} files/s  {px_bytes / t / 1e9:6.2f} GB/s of pixels  ({t * 1e3:.0f} ms)", flush=True)
        # PCIe: the bytes each mode moves, uploaded alone from pageable memory
        import ctypes as C

        L = eng.L
        for name, nbytes in (("compressed (DEVICE)", comp), ("ARGB words (HOST)", sum(h * w * 4 for w, h, c, _ in info))):
            d = C.c_void_p()
            L.rph_dev_alloc(eng.ctx, nbytes, C.byref(d))
            host = np.zeros(nbytes, np.uint8)
            t0 = time.perf_counter()
            L.rph_dev_upload(eng.ctx, d, host.ctypes.data_as(C.c_void_p), nbytes)
            t = time.perf_counter() - t0
            L.rph_dev_free(eng.ctx, d)
            print(f"  PCIe   {name}: {nbytes / 1e6:.0f} MB in {t * 1e3:.0f} ms (pageable upload)", flush=True)

        def pil(f):
            im = Image.open(io.BytesIO(f))
            im.load()
            return im.size

        with ThreadPoolExecutor(a.threads) as ex:
            list(ex.map(pil, files[:64]))
            t0 = time.perf_counter()
            list(ex.map(pil, files))
            t = time.perf_counter() - t0
        print(f"  Pillow {len(files) / t:9.0f} files/s  {px_bytes / t / 1e9:6.2f} GB/s of pixels  ({a.threads} threads)", flush=True)
    eng.webp_set_entropy(2)
    eng.close()


if __name__ == "__main__":
    main()
