#!/usr/bin/env python3
"""tools/files_rate.py -- a folder of mixed files through the library, three routes timed against each other in one process:

    (a) rph_files_pdq_hash_batch with RPH_FILES_CONCURRENT, the formats side by side (one lane per format);
    (b) rph_files_pdq_hash_batch with RPH_FILES_SEQUENTIAL;
    (c) the six per-format batch calls one after the other, which is what a caller did before the one call existed.

The corpus is a fixed mix of distinct synthetic photographs written by Pillow: 3000 JPEG (4:2:0, quality 85), 1000 PNG, and 500 each of
TIFF-LZW, lossless WebP, GIF (256 colours, dithered) and BMP at 512x512, shuffled; then the same mix at 1920x1080 with a tenth of the
counts.  --threads host threads, default modes, pixel hashes on.  The routes alternate (a), (b), (c) --reps times after one warm-up of
each; every route is reported with the minimum and maximum of its runs, route (a) also with the wall time, threads and files of every
lane of its slowest and fastest run (rph_debug_files_lanes): the lane with the longest wall time bounds the call.

An older build of the library (RPH_LIB_PATH), which lacks the one call, is timed on route (c) alone: --routes c.

    python tools/files_rate.py [--scale 1.0] [--threads 16] [--reps 5] [--routes abc]
"""
import argparse
import ctypes as C
import io
import os
import sys
import time
import zlib
from multiprocessing import Pool

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FORMATS = ("jpeg", "png", "tiff", "webp", "gif", "bmp")
COUNTS = dict(jpeg=3000, png=1000, tiff=500, webp=500, gif=500, bmp=500)
EXT = dict(jpeg="jpg", png="png", tiff="tif", webp="webp", gif="gif", bmp="bmp")


def _photo(rng, w, h):
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    ph = rng.uniform(0, 6.28, 3)
    img = np.stack([127 + 60 * np.sin(xx / (37 + 5 * c) + ph[c]) * np.cos(yy / (53 + 3 * c)) + 30 * np.sin((xx + yy) / 11.0 + ph[c]) for c in range(3)], -1)
    return np.clip(img + rng.normal(0, 6, img.shape), 0, 255).astype(np.uint8)


def make(args):
    from PIL import Image

    fmt, w, h, k = args
    rng = np.random.default_rng(zlib.crc32(f"{fmt}{w}".encode()) % 100003 + 1000 * k)
    im = Image.fromarray(_photo(rng, w, h))
    buf = io.BytesIO()
    if fmt == "jpeg":
        im.save(buf, "JPEG", quality=85, subsampling=2)
    elif fmt == "png":
        im.save(buf, "PNG", compress_level=6)
    elif fmt == "tiff":
        im.save(buf, "TIFF", compression="tiff_lzw")
    elif fmt == "webp":
        im.save(buf, "WEBP", lossless=True, quality=50, method=2)
    elif fmt == "gif":
        im.quantize(colors=256, dither=Image.Dither.FLOYDSTEINBERG).save(buf, "GIF", optimize=False)
    else:
        im.save(buf, "BMP")
    return buf.getvalue()


def load_library():
    """the library, an older build included: entry points it does not export are taken out of the binding's tables first"""
    from rupphash_amd import _lib

    _lib._one_hip_runtime()
    probe = C.CDLL(_lib.LIB_PATH)
    missing = [name for table in (_lib.SIGNATURES, _lib.DEBUG_SIGNATURES) for name in table if not hasattr(probe, name)]
    for table in (_lib.SIGNATURES, _lib.DEBUG_SIGNATURES):
        for name in missing:
            table.pop(name, None)
    return missing


def span(ts):
    return f"{min(ts) * 1e3:8.0f} .. {max(ts) * 1e3:8.0f} ms"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0, help="multiplies every count of the corpus")
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--routes", default="abc")
    a = ap.parse_args()
    pool = Pool(a.threads)  # (the workers are started before the library is loaded and the device opened: they never hold it)
    missing = load_library()
    from rupphash_amd import Engine, _lib

    if "rph_files_pdq_hash_batch" in missing:
        assert a.routes == "c", "this build lacks rph_files_pdq_hash_batch: --routes c"
    print(f"library {_lib.LIB_PATH}, {a.threads} host threads, {a.reps} alternations of routes {a.routes}", flush=True)
    eng = Engine(0)
    for w, h, div in ((512, 512, 1), (1920, 1080, 10)):
        counts = {f: max(1, int(COUNTS[f] * a.scale) // div) for f in FORMATS}
        jobs = [(f, w, h, k) for f in FORMATS for k in range(counts[f])]
        made = pool.map(make, jobs, chunksize=max(1, len(jobs) // (8 * a.threads)))
        order = np.random.default_rng(w).permutation(len(jobs))  # the folder's order: shuffled, fixed
        files = [made[i] for i in order]
        fmt_of = [jobs[i][0] for i in order]
        names = [f"photo{k:05d}.{EXT[f]}" for k, f in enumerate(fmt_of)]
        n = len(files)
        by_fmt = {f: [i for i in range(n) if fmt_of[i] == f] for f in FORMATS}
        lists = {f: eng.jpeg_file_list([files[i] for i in by_fmt[f]]) for f in FORMATS}
        mixed = eng.files_list(files, names) if "rph_files_pdq_hash_batch" not in missing else None
        print(f"\n{w}x{h}: {n} files (" + ", ".join(f"{counts[f]} {f} {sum(len(files[i]) for i in by_fmt[f]) / 1e6:.0f} MB" for f in FORMATS) + ")", flush=True)

        def route_c():
            out = np.zeros((n, 32), np.uint8)
            for f in FORMATS:
                r = getattr(eng, f + "_pdq_hash_batch")(lists[f], threads=a.threads, want_pixel_hash=True)
                assert not r["status"].any(), f
                out[by_fmt[f]] = r["hash"]
            return out

        def route_ab(sequential):
            r = eng.files_pdq_hash_batch(mixed, threads=a.threads, sequential=sequential, concurrent=not sequential, want_pixel_hash=True)
            assert not r["status"].any() and np.array_equal(r["format"], [FORMATS.index(f) + 1 for f in fmt_of])
            return r["hash"]

        routes = {"a": lambda: route_ab(False), "b": lambda: route_ab(True), "c": route_c}
        ref = None
        for r in a.routes:  # warm: buffers allocated, and the routes agree
            got = routes[r]()
            ref = got if ref is None else ref
            assert np.array_equal(got, ref), "the routes disagree"
        ts = {r: [] for r in a.routes}
        lanes = []
        for rep in range(a.reps):
            for r in a.routes:
                t0 = time.perf_counter()
                routes[r]()
                ts[r].append(time.perf_counter() - t0)
                if r == "a":
                    lanes.append(eng.debug_files_lanes())
            print(f"  alternation {rep}: " + "  ".join(f"({r}) {ts[r][-1] * 1e3:8.0f} ms" for r in a.routes), flush=True)
        what = dict(a="(a) one call, lanes side by side", b="(b) one call, sequential      ", c="(c) six per-format calls      ")
        for r in a.routes:
            print(f"  {what[r]}  {span(ts[r])}   {n / min(ts[r]):9.0f} .. {n / max(ts[r]):9.0f} files/s", flush=True)
        if lanes:
            for label, k in (("fastest", int(np.argmin(ts["a"]))), ("slowest", int(np.argmax(ts["a"])))):
                print(f"  lanes of the {label} run of (a), {ts['a'][k] * 1e3:.0f} ms: " +
                      ", ".join(f"{f} {ms:.0f} ms ({th} threads, {nf} files)" for f, (ms, th, nf) in lanes[k].items()), flush=True)
        eng.jpeg_release()
        for f in FORMATS[1:]:
            getattr(eng, f + "_release")()
    eng.close()
    pool.close()
    pool.join()


if __name__ == "__main__":
    main()
