#!/usr/bin/env python3
"""tools/nearest_rate.py -- what the k nearest files of a query cost against a resident library (rph_library_nearest,
csrc/nearest_kernels.hip), beside the read stream of the device, beside the only route the parent commit has (a threshold query and a
host reduction), and beside the host form.  One MI355X.

The library: 1 M files of Engine.synth_hashes (20 000 clusters of 5 near-duplicates among unrelated hashes), appended without
coefficients at similarity 63, so every file's 8 resident rows repeat its hash and its has_features byte is 0: the kernel reads all
256 bytes of a file and keeps it to row 0.  (g) runs the device form on the same rows with every row owned, which adds the in-lane
minimum over the variants.  Queries are hashes of random library files.  Host clock around calls that end in a synchronise, from
pageable host memory, one untimed call first, CALLS timed calls, min..max and median in ms.

  (a) few queries: Library.nearest for n_q = 1 and 32, k = 10, no cutoff; rph_read_stream_dev over the same 256 MB by device events in
      the same run; the fraction of the stream's rate the call reaches (host clock) and the two kernels reach (device events around
      rph_hamming_nearest_dev on the same number of bytes)
  (b) many queries: n_q = 1 024 and 10 000, k = 10 and 64: row-pairs per second (8 rows x files x queries)
  (c) against the parent commit: max_dist = 63.  The parent's route is Library.query (unchanged by the commit that adds the nearest
      calls) and a host reduction: minimum per (file, query), sort by (d, i), cut at k.  n_q = 100 and 10 000, k = 10; the slots of both
      routes are compared for equality first.  The bar: max of the new call < min of the parent route
  (d) without a cutoff the parent has no device route: rph_hamming_nearest_host (the queries over the host's threads) on the same
      inputs, n_q = 100, and the ratio
  (g) rph_hamming_nearest_dev with has_features = NULL (every file owns its 8 rows), device events

usage: nearest_rate.py"""
import ctypes as C
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))

N, SIM, CLUSTERS, CALLS = 1_000_000, 63, 20_000, 15


def spread(xs, fmt="%.3f"):
    return (fmt + ".." + fmt + "  median " + fmt) % (min(xs), max(xs), float(np.median(xs)))


def timed(call, calls=CALLS):
    call()
    out = []
    for _ in range(calls):
        t = time.perf_counter()
        call()
        out.append((time.perf_counter() - t) * 1e3)
    return out


def by_events(eng, call, calls=CALLS):
    e0, e1 = eng.event(), eng.event()
    out = []
    for _ in range(1 + calls):
        eng.event_record(e0)
        call()
        eng.event_record(e1)
        out.append(eng.event_elapsed_ms(e0, e1))
    eng.event_destroy(e0)
    eng.event_destroy(e1)
    return out[1:]


def parent_route(lib, queries, k, max_dist):
    """Library.query and the reduction on the host: (edges[n_q, k], counts[n_q]) as the nearest calls return them"""
    from rupphash_amd import EDGE_DTYPE

    swept = lib.query(queries)
    swept = swept[swept["d"] <= max_dist]
    variant = (swept["flags"].astype(np.int64) & 0x0E00) >> 9
    order = np.lexsort((variant, swept["d"], swept["i"], swept["j"]))  # per (query, file): the smallest (d, variant) first
    s = swept[order]
    first = np.ones(len(s), bool)
    first[1:] = (s["j"][1:] != s["j"][:-1]) | (s["i"][1:] != s["i"][:-1])
    s, v = s[first], variant[order][first]
    order = np.lexsort((s["i"], s["d"], s["j"]))  # per query by (d, i)
    s, v = s[order], v[order]
    edges = np.zeros((len(queries), k), EDGE_DTYPE)
    edges["i"], edges["d"] = 0xFFFFFFFF, 0xFFFF
    edges["j"] = np.arange(len(queries), dtype=np.uint32)[:, None]
    counts = np.zeros(len(queries), np.uint32)
    start = np.searchsorted(s["j"], np.arange(len(queries) + 1))
    rank = np.arange(len(s)) - start[s["j"]]
    take = rank < k
    edges["i"][s["j"][take], rank[take]] = s["i"][take]
    edges["d"][s["j"][take], rank[take]] = s["d"][take]
    edges["flags"][s["j"][take], rank[take]] = v[take] << 9
    counts[:] = np.minimum(np.diff(start), k)
    return edges, counts


def main():
    if sys.argv[1:]:
        raise SystemExit(__doc__)
    from rupphash_amd import EDGE_DTYPE, Engine

    eng = Engine(0)
    hashes = eng.synth_hashes(0, N, N, n_clusters=CLUSTERS)
    lib = eng.library(SIM)
    t = time.perf_counter()
    lib.append(hashes)
    print(f"library {N} files ({CLUSTERS} clusters of 5), similarity {SIM}, no coefficients: 8 rows of 32 bytes per file, has_features 0; built by one append in "
          f"{(time.perf_counter() - t) * 1e3:.0f} ms, {lib.comparisons} comparisons; layout for 1 query, k = 10: {Engine.nearest_layout(N, 8, 1, 10)}, for 10 000: "
          f"{Engine.nearest_layout(N, 8, 10000, 10)}; {CALLS} timed calls each after 1 untimed; host clock, ms", flush=True)
    rng = np.random.default_rng(2027)
    queries = hashes[rng.integers(0, N, 10_000)].copy()
    row_bytes = N * 256

    # the read stream over the same number of bytes
    d_buf = eng.dev_alloc(row_bytes)
    eng.dev_memset(d_buf, 1, row_bytes)
    stream_ms = by_events(eng, lambda: eng.read_stream_dev(d_buf, row_bytes))
    stream = min(stream_ms)
    print(f"rph_read_stream_dev over {row_bytes} bytes, device events                      {spread(stream_ms, '%.4f')}   ({row_bytes / (stream * 1e-3) / 1e12:.2f} TB/s at the fastest)",
          flush=True)

    # the same rows in a buffer of the tool's, for the device form
    rows = np.repeat(hashes, 8, axis=0)
    eng.dev_upload(d_buf, rows)
    d_q, d_hf = eng.dev_alloc(len(queries) * 32), eng.dev_alloc(N)
    eng.dev_upload(d_q, queries)
    eng.dev_memset(d_hf, 0, N)
    d_out, d_cnt = eng.dev_alloc(len(queries) * 64 * EDGE_DTYPE.itemsize), eng.dev_alloc(len(queries) * 4)
    eng.synchronize()

    print("(a) few queries, k = 10, no cutoff", flush=True)
    for n_q in (1, 32):
        ms = timed(lambda: lib.nearest(queries[:n_q], 10))
        dev = by_events(eng, lambda: eng.hamming_nearest_dev(d_buf, 8, N, d_q, n_q, 10, d_out, d_has_features=d_hf, d_counts=d_cnt))
        print(f"    n_q = {n_q:<3} Library.nearest                                        {spread(ms)}   stream / call = {stream / max(ms):.2f}..{stream / min(ms):.2f}", flush=True)
        print(f"    n_q = {n_q:<3} the two kernels (rph_hamming_nearest_dev), device events   {spread(dev, '%.4f')}   stream / kernels = {stream / max(dev):.2f}..{stream / min(dev):.2f}",
              flush=True)

    print("(b) many queries, no cutoff: row-pairs = 8 x files x queries", flush=True)
    for n_q in (1024, 10_000):
        for k in (10, 64):
            ms = timed(lambda: lib.nearest(queries[:n_q], k))
            pairs = 8.0 * N * n_q
            print(f"    n_q = {n_q:<6} k = {k:<3} Library.nearest   {spread(ms)}   {pairs / (max(ms) * 1e-3) / 1e12:.2f}..{pairs / (min(ms) * 1e-3) / 1e12:.2f} T row-pairs/s", flush=True)

    print(f"(c) max_dist = {SIM}, k = 10: the parent's route (Library.query + host reduction) and Library.nearest", flush=True)
    for n_q in (100, 10_000):
        q = queries[:n_q]
        want = parent_route(lib, q, 10, SIM)
        got = lib.nearest(q, 10, max_dist=SIM)
        assert got[0].tobytes() == want[0].tobytes() and np.array_equal(got[1], want[1]), "the two routes disagree"
        old = timed(lambda: parent_route(lib, q, 10, SIM))
        sweep_only = timed(lambda: lib.query(q))
        new = timed(lambda: lib.nearest(q, 10, max_dist=SIM))
        print(f"    n_q = {n_q:<6} identical slots ({int(got[1].sum())} filled)", flush=True)
        print(f"    n_q = {n_q:<6} parent route           {spread(old)}   (its Library.query alone {spread(sweep_only)})", flush=True)
        print(f"    n_q = {n_q:<6} Library.nearest        {spread(new)}", flush=True)
        print(f"    n_q = {n_q:<6} bar: max new {max(new):.3f} < min parent {min(old):.3f}: {'MET' if max(new) < min(old) else 'NOT MET'}", flush=True)

    print("(d) no cutoff, n_q = 100, k = 10: the host form and the library", flush=True)
    hf = np.zeros(N, np.uint8)
    q = queries[:100]
    host = timed(lambda: Engine.hamming_nearest_host(rows.reshape(N, 8, 32), q, 10, has_features=hf), calls=3)
    new = timed(lambda: lib.nearest(q, 10))
    a, b = Engine.hamming_nearest_host(rows.reshape(N, 8, 32), q, 10, has_features=hf), lib.nearest(q, 10)
    assert a[0].tobytes() == b[0].tobytes() and np.array_equal(a[1], b[1]), "the host form and the library disagree"
    print(f"    rph_hamming_nearest_host, {os.cpu_count()} CPUs reported, threads as rph_host_threads allows (3 calls)   {spread(host, '%.1f')}", flush=True)
    print(f"    Library.nearest                                                           {spread(new)}   identical slots; median host / median library = "
          f"{np.median(host) / np.median(new):.0f}", flush=True)

    print("(g) rph_hamming_nearest_dev with every row owned (has_features NULL: the in-lane minimum over 8 variants), device events, k = 10", flush=True)
    for n_q in (1, 32, 1024):
        dev = by_events(eng, lambda: eng.hamming_nearest_dev(d_buf, 8, N, d_q, n_q, 10, d_out, d_counts=d_cnt))
        print(f"    n_q = {n_q:<5} {spread(dev, '%.4f')}", flush=True)
    for p in (d_buf, d_q, d_hf, d_out, d_cnt):
        eng.dev_free(p)
    lib.close()
    eng.close()


if __name__ == "__main__":
    main()
