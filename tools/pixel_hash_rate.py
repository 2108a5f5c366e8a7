#!/usr/bin/env python3
"""tools/pixel_hash_rate.py -- rates of the BLAKE3 kernels (blake3_kernels.hip), device time by HIP events on resident buffers:
  * rph_blake3_batch_dev on device bytes: GB/s for strings of 1 KiB / 64 KiB / 8 MiB (256 MiB per call);
  * rph_pixel_hash_batch_dev on device Rgb8 at 512x512 and 1265x850: images/s and TB/s of hashed RGBA16 bytes (8 per pixel), against
    the VALU roof (256 CUs x 4 SIMDs x 32 lanes per clock at 2.4 GHz over the VALU instructions of one 64-byte block);
  * rph_jpeg_pdq_hash_batch with and without pixel hashes (wall time per call) on tools/jpeg_rate.py's 512x512 4:2:0 q85 files and on
    tools/jpeg_photo_rate.py's photo-sized crops of tests/golden/bench.jpg (baseline 4:2:0 q90)."""
import argparse
import io
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
VALU_PER_BLOCK = 690  # VALU instructions per 64-byte block compression (691 in the kernels: the ISA that tools/asmstat.sh leaves behind)
ROOF_LANE_OPS = 256 * 4 * 32 * 2.4e9


def dev_time(eng, fn, reps):
    fn()  # warm-up (the stream-ordered scratch pool)
    eng.stream_synchronize()
    e0, e1 = eng.event(), eng.event()
    eng.event_record(e0)
    for _ in range(reps):
        fn()
    eng.event_record(e1)
    ms = eng.event_elapsed_ms(e0, e1) / reps
    eng.event_destroy(e0)
    eng.event_destroy(e1)
    return ms * 1e-3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--jpeg-n", type=int, default=20000)
    ap.add_argument("--photo-n", type=int, default=4000)
    a = ap.parse_args()
    from PIL import Image

    from rupphash_amd import Engine

    eng = Engine(0)
    name, cus, _ = eng.device_info()
    print(f"device: {name} ({cus} CUs); VALU roof {ROOF_LANE_OPS / 1e12:.1f} T lane-ops/s -> {ROOF_LANE_OPS / VALU_PER_BLOCK * 64 / 1e12:.2f} TB/s "
          f"of hashed bytes at {VALU_PER_BLOCK} VALU per 64 B")

    # ---- byte strings on the device
    total = 256 << 20
    d_data = eng.dev_alloc(total)
    eng.synth_images_dev(d_data, 0, total // (512 * 512 * 3), 512, 512)  # any bytes will do
    for size in (1 << 10, 64 << 10, 8 << 20):
        n = total // size
        off = (np.arange(n + 1, dtype=np.uint64) * size)
        d_off, d_dig = eng.dev_alloc(off.nbytes), eng.dev_alloc(32 * n)
        eng.dev_upload(d_off, off)
        dt = dev_time(eng, lambda: eng.blake3_batch_dev(d_data, d_off, n, d_dig), a.reps)
        print(f"blake3 of device bytes, {n:7d} strings of {size:8d} B: {dt * 1e3:8.3f} ms per call  {total / dt / 1e9:8.1f} GB/s")
        eng.dev_free(d_off)
        eng.dev_free(d_dig)
    eng.dev_free(d_data)

    # ---- pixel hash of device Rgb8
    for (w, h, n) in ((512, 512, 2048), (1265, 850, 512)):
        d_px, d_h = eng.dev_alloc(n * w * h * 3), eng.dev_alloc(32 * n)
        if w == 512:
            eng.synth_images_dev(d_px, 0, n, w, h)
        dt = dev_time(eng, lambda: eng.pixel_hash_batch_dev(d_px, n, w, h, 3, d_h), a.reps)
        hashed = n * w * h * 8
        roof = ROOF_LANE_OPS / VALU_PER_BLOCK * 64
        print(f"pixel hash, device Rgb8 {w}x{h}, {n} per call: {dt * 1e3:8.3f} ms  {n / dt:9.0f} images/s  {hashed / dt / 1e12:6.2f} TB/s of RGBA16 "
              f"({hashed / dt / roof * 100:5.1f} % of the VALU roof)  {n * w * h * 3 / dt / 1e12:5.2f} TB/s of pixels read")
        eng.dev_free(d_px)
        eng.dev_free(d_h)

    # ---- the JPEG batch with and without pixel hashes
    imgs = eng.synth_images(0, 64, 512, 512)
    sets = []
    base = []
    for k in range(64):
        buf = io.BytesIO()
        Image.fromarray(imgs[k]).save(buf, "JPEG", quality=85, subsampling=2)
        base.append(buf.getvalue())
    sets.append(("512x512 baseline 4:2:0 q85", [base[k % 64] for k in range(a.jpeg_n)]))
    im = Image.open(os.path.join(ROOT, "tests", "golden", "bench.jpg"))
    im.load()
    photos = []
    for k in range(16):
        buf = io.BytesIO()
        im.crop((k, k // 2, 1280 - (15 - k), 854 - (7 - k // 2))).save(buf, "JPEG", quality=90, subsampling=2)
        photos.append(buf.getvalue())
    sets.append(("photo ~1265x850 baseline 4:2:0 q90", [photos[k % 16] for k in range(a.photo_n)]))
    for label, files in sets:
        lst = eng.jpeg_file_list(files)
        for mode, mname in ((2, "auto"), (0, "host")):
            eng.jpeg_set_entropy(mode)
            for ph in (False, True):
                eng.jpeg_pdq_hash_batch(lst, threads=16, want_pixel_hash=ph)  # warm-up: buffers
                best = 1e9
                for _ in range(3):
                    t = time.perf_counter()
                    out = eng.jpeg_pdq_hash_batch(lst, threads=16, want_pixel_hash=ph)
                    best = min(best, time.perf_counter() - t)
                assert (out["status"] == 0).all()
                print(f"jpeg batch {label}, {len(files)} files, entropy {mname}, pixel hash {'on ' if ph else 'off'}: {len(files) / best:9.0f} files/s  "
                      f"({best * 1e3:8.1f} ms per call)")
    eng.jpeg_set_entropy(2)
    eng.close()


if __name__ == "__main__":
    main()
