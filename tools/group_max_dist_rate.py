#!/usr/bin/env python3
"""tools/group_max_dist_rate.py -- what labelling every group of a resident library with its max_dist costs (rph_library_group_max_dist,
csrc/group_info.hip), beside the same from host arrays and beside the Python loop that was the only implementation.  One MI355X.

The files are the library of tools/library_rate.py: 1 M files with coefficients, 20 k near-duplicates among them, grouped at similarity 40
by one rph_library_append.  Groups are rph_library_groups' as they come; the pivot of a group is its first member (every file has
features: that is the reference's find_map pair).  Everything but (d) is timed by the host clock around calls that end in a synchronise,
from pageable host memory, in one process, ROUNDS alternations of the three forms, one untimed call of each first.

  (a) scanner.group_max_dist: the Python loop over groups, pivot rows by one rph_pdq_hashes_from_coeffs.  It is unchanged by the commit
      that adds the device forms, so it is the parent commit's path
  (b) rph_library_group_max_dist over all groups with member_dist, explicit pivots; and with default pivots (resolved on the device)
  (c) rph_group_max_dist from host arrays: the hashes of 1 M files and the pivots' coefficient rows cross PCIe
  (d) the zeroing and the distance kernel of (b) alone, by device events (rph_debug_group_max_dist_events), and its algorithmic bytes
      members x (4 + 32 + 4) + groups x (4 + 4 + 256) against the read stream of this device (rph_read_stream_dev over 1 GiB)
  (e) small calls: (b) for the first 4 groups, which is launch-bound
  (f) the kernel at a size that fills the device: 400 000 made-up groups of 2 .. 5 random files of the same resident library (what a
      looser similarity gives; any lists are legal), host clock and device events, compared with rph_group_max_dist_host

The results of (a), (b) and (c) are compared for equality first.  The bar: max of (b) < min of (a).

usage: group_max_dist_rate.py"""
import ctypes as C
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))

ROUNDS, TIMED = 3, 5
N, SIM = 1_000_000, 40


def spread(xs, fmt="%.3f"):
    return (fmt + ".." + fmt + "  median " + fmt) % (min(xs), max(xs), float(np.median(xs)))


def p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def make_files(eng):
    """the library files of tools/library_rate.py, restated: coefficients and hashes"""
    rng = np.random.default_rng(2026)
    coeffs = np.zeros((N, 256), np.float32)
    step = 100_000
    for first in range(0, N, step):
        coeffs[first:first + step] = rng.standard_normal((step, 256), dtype=np.float32) * 20
    dst = rng.choice(N, 20_000, replace=False)
    src = rng.integers(0, N, 20_000)
    coeffs[np.sort(dst)] = coeffs[src] + rng.standard_normal((len(src), 256), dtype=np.float32) * np.float32(0.8)
    hashes = np.zeros((N, 32), np.uint8)
    for first in range(0, N, step):
        hashes[first:first + step] = eng.pdq_hashes_from_coeffs(coeffs[first:first + step], want_dihedral=False)[0]
    return coeffs, hashes


def clocked(call):
    t = time.perf_counter()
    rc = call()
    ms = (time.perf_counter() - t) * 1e3
    assert rc == 0, rc
    return ms


def main():
    if sys.argv[1:]:
        raise SystemExit(__doc__)
    from rupphash_amd import Engine, scanner

    eng = Engine(0)
    L = eng.L
    coeffs, hashes = make_files(eng)
    lib = eng.library(SIM)
    lib.append(hashes, coeffs=coeffs)
    groups = lib.groups()
    members, offsets = eng._flatten_groups(groups)
    ng, total = len(groups), len(members)
    pivots = members[offsets[:-1]].copy()
    pivot_list = pivots.tolist()
    sizes = np.diff(offsets.astype(np.int64))
    print(f"library {N} files, {ng} groups of {sizes.min()}..{sizes.max()} members ({total} member slots), similarity {SIM}; pivot = first member; "
          f"{ROUNDS} alternations, 1 untimed + {TIMED} timed calls of (b) and (c) and 1 of (a) in each; host clock, ms", flush=True)

    out_b, md_b = np.zeros(ng, np.uint32), np.zeros(total, np.uint32)
    out_d, md_d = np.zeros(ng, np.uint32), np.zeros(total, np.uint32)
    out_c, md_c = np.zeros(ng, np.uint32), np.zeros(total, np.uint32)
    call_b = lambda: L.rph_library_group_max_dist(lib.handle, p(members), p(offsets), ng, p(pivots), p(out_b), p(md_b))  # noqa: E731
    call_d = lambda: L.rph_library_group_max_dist(lib.handle, p(members), p(offsets), ng, None, p(out_d), p(md_d))  # noqa: E731
    call_c = lambda: L.rph_group_max_dist(eng.ctx, p(hashes), p(coeffs), None, N, p(members), p(offsets), ng, p(pivots), p(out_c), p(md_c))  # noqa: E731
    call_small = lambda: L.rph_library_group_max_dist(lib.handle, p(members), p(offsets), 4, p(pivots), p(out_d), None)  # noqa: E731
    start, stop = eng.event(), eng.event()

    ms = {k: [] for k in "abcdeks"}
    result_a = None
    for r in range(ROUNDS):
        for key, call in (("b", call_b), ("d", call_d), ("c", call_c)):
            clocked(call)
            ms[key] += [clocked(call) for _ in range(TIMED)]
        assert L.rph_debug_group_max_dist_events(eng.ctx, start, stop) == 0
        for _ in range(TIMED):
            clocked(call_b)
            ms["k"].append(eng.event_elapsed_ms(start, stop))
        assert L.rph_debug_group_max_dist_events(eng.ctx, None, None) == 0
        clocked(call_small)
        ms["s"] += [clocked(call_small) for _ in range(TIMED)]
        t = time.perf_counter()
        got = scanner.group_max_dist(groups, hashes, pivot_list, coefficients=coeffs, engine=eng)
        ms["a"].append((time.perf_counter() - t) * 1e3)
        assert result_a is None or got == result_a
        result_a = got
        assert out_b.tolist() == result_a and np.array_equal(out_b, out_c) and np.array_equal(out_b, out_d), "the forms disagree on max_dist"
        assert np.array_equal(md_b, md_c) and np.array_equal(md_b, md_d), "the forms disagree on member_dist"
    wrapper = []
    for _ in range(TIMED):
        t = time.perf_counter()
        assert lib.group_max_dist(groups, pivot_list) == result_a
        wrapper.append((time.perf_counter() - t) * 1e3)
    eng.event_destroy(start)
    eng.event_destroy(stop)
    print(f"results: {ng} max_dist values equal in all three forms, {total} member_dist values equal in the device forms; max_dist {min(result_a)}..{max(result_a)}",
          flush=True)

    print(f"(a) scanner.group_max_dist, the Python loop (the parent's path)        {spread(ms['a'], '%.1f')}   all: " + " ".join("%.1f" % m for m in ms["a"]), flush=True)
    print(f"(b) rph_library_group_max_dist, all groups, explicit pivots            {spread(ms['b'])}", flush=True)
    print(f"(b) the same with default pivots (found on the device)                 {spread(ms['d'])}", flush=True)
    print(f"(b) Library.group_max_dist, the Python wrapper (lists in, lists out)   {spread(wrapper)}", flush=True)
    print(f"(c) rph_group_max_dist from host arrays (32 MB of hashes, {ng} pivots' coefficients)   {spread(ms['c'])}", flush=True)
    slowest_b = max(ms["b"] + ms["d"])
    print(f"bar: max (b) {slowest_b:.3f} < min (a) {min(ms['a']):.1f}: {'MET' if slowest_b < min(ms['a']) else 'NOT MET'}   "
          f"(median (a) / median (b) = {np.median(ms['a']) / np.median(ms['b']):.0f})", flush=True)

    # the read stream this device delivers, over 1 GiB
    nbytes = 1 << 30
    d_buf = eng.dev_alloc(nbytes)
    eng.dev_memset(d_buf, 1, nbytes)
    s0, s1 = eng.event(), eng.event()
    stream_ms = []
    for _ in range(1 + TIMED):
        eng.event_record(s0)
        eng.read_stream_dev(d_buf, nbytes)
        eng.event_record(s1)
        stream_ms.append(eng.event_elapsed_ms(s0, s1))
    eng.dev_free(d_buf)
    eng.event_destroy(s0)
    eng.event_destroy(s1)
    stream = nbytes / (min(stream_ms[1:]) * 1e-3) / 1e12
    algo = total * (4 + 32 + 4) + ng * (4 + 4 + 256)
    k = float(np.median(ms["k"]))
    print(f"(d) device time of the zeroing + distance kernel of (b)                    {spread(ms['k'], '%.4f')}", flush=True)
    print(f"(d) algorithmic bytes {algo} ({total} x 40 + {ng} x 264): {algo / (k * 1e-3) / 1e12:.3f} TB/s at the median; the read stream of this device: "
          f"{stream:.2f} TB/s, which would move them in {algo / (stream * 1e12) * 1e3:.4f} ms", flush=True)
    print(f"(e) rph_library_group_max_dist for 4 groups (launch-bound)                 {spread(ms['s'])}", flush=True)

    rng = np.random.default_rng(400)
    big_sizes = rng.integers(2, 6, 400_000)
    big_offsets = np.concatenate([[0], np.cumsum(big_sizes)]).astype(np.uint32)
    big_members = rng.integers(0, N, int(big_offsets[-1])).astype(np.uint32)
    big_ng, big_total = len(big_sizes), len(big_members)
    out_f, md_f, out_h, md_h = (np.zeros(k, np.uint32) for k in (big_ng, big_total, big_ng, big_total))
    call_f = lambda: L.rph_library_group_max_dist(lib.handle, p(big_members), p(big_offsets), big_ng, None, p(out_f), p(md_f))  # noqa: E731
    clocked(call_f)
    host_ms = clocked(lambda: L.rph_group_max_dist_host(p(hashes), p(coeffs), None, N, p(big_members), p(big_offsets), big_ng, None, p(out_h), p(md_h)))
    assert np.array_equal(out_f, out_h) and np.array_equal(md_f, md_h), "the library form and the host form disagree on the made-up groups"
    start, stop = eng.event(), eng.event()
    assert L.rph_debug_group_max_dist_events(eng.ctx, start, stop) == 0
    f_ms, f_dev = [], []
    for _ in range(ROUNDS * TIMED):
        f_ms.append(clocked(call_f))
        f_dev.append(eng.event_elapsed_ms(start, stop))
    assert L.rph_debug_group_max_dist_events(eng.ctx, None, None) == 0
    eng.event_destroy(start)
    eng.event_destroy(stop)
    algo_f = big_total * (4 + 32 + 4) + big_ng * (4 + 4 + 256)
    kf = float(np.median(f_dev))
    print(f"(f) {big_ng} made-up groups, {big_total} member slots, default pivots: host clock      {spread(f_ms)}   (rph_group_max_dist_host, one thread: {host_ms:.0f}, equal)",
          flush=True)
    print(f"(f) device time of its zeroing + distance kernel                               {spread(f_dev, '%.4f')}", flush=True)
    print(f"(f) algorithmic bytes {algo_f}: {algo_f / (kf * 1e-3) / 1e12:.3f} TB/s at the median (random files: every hash a 32-byte read of its own, every pivot 256); "
          f"the read stream would move them in {algo_f / (stream * 1e12) * 1e3:.4f} ms", flush=True)
    lib.close()
    eng.close()


if __name__ == "__main__":
    main()
