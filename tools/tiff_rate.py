#!/usr/bin/env python3
"""tools/tiff_rate.py -- rph_tiff_pdq_hash_batch rates on corpora of distinct files, each in DEVICE and HOST decompress mode (--threads
host threads), plus a --threads Pillow (libtiff) decode as the CPU baseline and the pageable upload of the bytes each mode moves.
Corpora: photographic 512x512 RGB (LZW + predictor 2, 8 KB strips); 4000x3000 RGB scans as LZW + predictor and Deflate + predictor in
8 KB strips, and Deflate + predictor in 256x256 tiles; 1920x1080 RGBA screenshots (LZW + predictor); uncompressed 512x512 RGB.  Strip files
are written by libtiff through Pillow, tiled ones by tests/tiff_util.py with zlib (its LZW encoder is Python: no LZW tiles here).

    python tools/tiff_rate.py [--photo N] [--scan N] [--screen N] [--raw N] [--threads 16] [--reps 3]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _photo(rng, w, h):
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    ph = rng.uniform(0, 6.28, 3)
    img = np.stack([127 + 60 * np.sin(xx / (37 + 5 * c) + ph[c]) * np.cos(yy / (53 + 3 * c)) + 30 * np.sin((xx + yy) / 11.0 + ph[c]) for c in range(3)], -1)
    return np.clip(img + rng.normal(0, 6, img.shape), 0, 255).astype(np.uint8)


def _pil(img, compression, predictor):
    from PIL import Image, TiffImagePlugin

    TiffImagePlugin.STRIP_SIZE = 8192
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, format="TIFF", compression=compression, **({"tiffinfo": {317: 2}} if predictor else {}))
    return buf.getvalue()


def make(args):
    import tiff_util as tu

    kind, k = args
    rng = np.random.default_rng(zlib.crc32(kind.encode()) % 100003 + 1000 * k)
    if kind == "photo_lzw":
        return _pil(_photo(rng, 512, 512), "tiff_lzw", True)
    if kind == "raw":
        return _pil(_photo(rng, 512, 512), "raw", False)
    if kind == "screen_lzw":
        img = np.full((1080, 1920, 4), 255, np.uint8)
        img[:, :, :3] = rng.integers(200, 256, 3)
        for _ in range(40):
            x0, y0 = rng.integers(0, 1800), rng.integers(0, 1000)
            img[y0:y0 + rng.integers(10, 200), x0:x0 + rng.integers(10, 400), :3] = rng.integers(0, 256, 3)
        for _ in range(300):
            x0, y0 = rng.integers(0, 1900), rng.integers(0, 1070)
            img[y0:y0 + 9, x0:x0 + rng.integers(2, 20), :3] = rng.integers(0, 80)
        return _pil(img, "tiff_lzw", True)
    img = _photo(rng, 4000, 3000)
    if kind == "scan_lzw":
        return _pil(img, "tiff_lzw", True)
    if kind == "scan_deflate":
        return _pil(img, "tiff_adobe_deflate", True)
    tiles = [zlib.compress(raw, 6) for raw, _ in tu.segment_rows(img, 8, predictor=2, tile=(256, 256))]
    return tu.write(tu.base_tags(4000, 3000, 3, 8, 2, 8, 2, None, (256, 256)), tiles, tiled=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--photo", type=int, default=8000)
    ap.add_argument("--scan", type=int, default=24)
    ap.add_argument("--screen", type=int, default=400)
    ap.add_argument("--raw", type=int, default=4000)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    import ctypes as C
    from concurrent.futures import ThreadPoolExecutor

    from PIL import Image

    import tiff_util as tu
    from rupphash_amd import Engine

    eng = Engine(0)
    plan = [("photo_lzw", a.photo), ("scan_lzw", a.scan), ("scan_deflate", a.scan), ("scan_deflate_tiles", a.scan), ("screen_lzw", a.screen), ("raw", a.raw)]
    for kind, n in plan:
        if not n:
            continue
        with Pool(a.threads) as pool:
            files = pool.map(make, [(kind, k) for k in range(n)], chunksize=max(1, n // (4 * a.threads)))
        fl = eng.jpeg_file_list(files)
        info = [Engine.tiff_info(f) for f in files]
        px_bytes = sum(w * h * c for w, h, c, _ in info)
        st, i0 = tu.parse(files[0])
        comp = sum(len(f) for f in files)
        print(f"{kind}: {len(files)} distinct files, {len(i0['segs'])} segments in the first, {comp / 1e6:.1f} MB of files, {px_bytes / 1e9:.2f} GB decoded pixels", flush=True)
        ref = None
        for mode, name in ((1, "DEVICE"), (0, "HOST")):
            eng.tiff_set_decompress(mode)
            eng.tiff_pdq_hash_batch(fl, threads=a.threads)  # warm: buffers allocated
            ts = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                out = eng.tiff_pdq_hash_batch(fl, threads=a.threads)
                ts.append(time.perf_counter() - t0)
            assert not out["status"].any()
            if ref is None:
                ref = out["hash"]
            assert np.array_equal(ref, out["hash"]), "modes disagree"
            t = min(ts)
            print(f"  {name:6s} {len(files) / t:9.1f} files/s  {px_bytes / t / 1e9:6.2f} GB/s of pixels  ({t * 1e3:.0f} ms, best of {a.reps}; median {sorted(ts)[len(ts) // 2] * 1e3:.0f} ms)", flush=True)
        L = eng.L
        for name, nbytes in (("compressed (DEVICE)", comp), ("decoded (HOST)", px_bytes)):
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
            list(ex.map(pil, files[:16]))
            t0 = time.perf_counter()
            list(ex.map(pil, files))
            t = time.perf_counter() - t0
        print(f"  Pillow {len(files) / t:9.1f} files/s  {px_bytes / t / 1e9:6.2f} GB/s of pixels  ({a.threads} threads)", flush=True)
        eng.tiff_release()
    eng.tiff_set_decompress(2)
    eng.close()


if __name__ == "__main__":
    main()
