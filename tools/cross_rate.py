#!/usr/bin/env python3
"""tools/cross_rate.py -- the three measurements behind the cross-set sweep (csrc/hamming_kernels.hip, CROSS instantiations) and
rph_group_files_pdq_append.  One MI355X.  Device events around windows of repeated calls on resident data unless a line says
"end to end"; every shape warmed up by an untimed call; ROUNDS windows per figure, min..max printed.

  cross    Tpairs/s of rph_hamming_cross_pairs_dev at thresholds 32 and 40 for (1 M x 1 M), (1 M x 10 k), (1 M x 100), (10 M x 1 k), with
           the bytes/s of the large side beside it, and the square sweep of 1 M in its +-1 fp4 form (kernel setting 3: the same loop)
           of the same run.  Uniform random hashes from two seeds: no edges, the figure is the fast path's.
  square   rph_hamming_all_pairs_dev of 1 M synthetic hashes (1000 clusters) at thresholds 32 and 63 and the 8-variant sweep of 100 k
           files, this build against --parent-tree (a checkout of the parent commit with its library built): child processes, one per build and round, alternating.
  append   library of 1 M files with coefficients + 10 k new files (half of them near-duplicates of library files), similarity 40:
           rph_group_files_pdq_append of this build against rph_group_files_pdq of --parent-tree on the concatenation, both end to end
           from host memory (host clock around the call), alternating child processes; then where the append's time goes, stage by
           stage through the device entry points.

usage: cross_rate.py [cross] [square] [append] [--parent-tree DIR]      (default: all three)"""
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# a child that measures the parent commit imports the package (and with it the library) of that checkout
sys.path.insert(0, os.environ.get("RPH_CROSS_RATE_TREE") or os.path.join(HERE, ".."))

ROUNDS = 5
SEED_A, SEED_B = 0xC0FFEE, 0xBEEF01


def timed(eng, work, reps):
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


def spread(xs, fmt="%.3f"):
    return (fmt + ".." + fmt) % (min(xs), max(xs))


def edge_count(eng, d_c):
    c = np.zeros(1, np.uint64)
    eng.dev_download(c, d_c)
    return int(c[0])


# ------------------------------------------------------------------------------------------ cross
def leg_cross(eng):
    cap = 1 << 16
    d_e, d_c = eng.dev_alloc(cap * 12), eng.dev_alloc(8)
    n_max = 10_000_000
    d_a, d_b = eng.dev_alloc(n_max * 32), eng.dev_alloc(1_000_000 * 32)
    eng.synth_hashes_dev(d_a, 0, n_max, n_max, seed=SEED_A)
    eng.synth_hashes_dev(d_b, 0, 1_000_000, 1_000_000, seed=SEED_B)
    eng.synchronize()
    for thr in (32, 40):
        for n_a, n_b, reps in ((1_000_000, 1_000_000, 8), (1_000_000, 10_000, 200), (1_000_000, 100, 400), (10_000_000, 1_000, 100)):
            def work():
                eng.dev_memset(d_c, 0, 8)
                eng.hamming_cross_pairs_dev(d_a, n_a, d_b, n_b, thr, d_e, cap, d_c)
            work()
            ms = [timed(eng, work, reps) for _ in range(ROUNDS)]
            pairs, big = n_a * n_b, max(n_a, n_b) * 32
            swap, seg, segs, blocks = eng.hamming_cross_layout(n_a, n_b)
            print(f"cross  thr {thr}  {n_a:>9d} x {n_b:>8d}  {spread(ms)} ms   {pairs / max(ms) / 1e9:7.2f}..{pairs / min(ms) / 1e9:7.2f} Tpairs/s   "
                  f"large side {big / max(ms) / 1e6:8.1f}..{big / min(ms) / 1e6:8.1f} GB/s   ({blocks} blocks of {seg} column tile(s), "
                  f"{'B' if swap else 'A'} on the rows, {edge_count(eng, d_c)} edges)", flush=True)
        n = 1_000_000
        for kernel, name in ((3, "+-1 fp4 (setting 3)"), (2, "default (setting 2, sorted {0,1})")):
            eng.set_hamming_kernel(kernel)

            def square():
                eng.dev_memset(d_c, 0, 8)
                eng.hamming_all_pairs_dev(d_a, n, thr, d_e, cap, d_c)
            square()
            ms = [timed(eng, square, 8) for _ in range(ROUNDS)]
            pairs = n * (n - 1) // 2
            print(f"square thr {thr}  {n:>9d} all pairs, {name:34s} {spread(ms)} ms   {pairs / max(ms) / 1e9:7.2f}..{pairs / min(ms) / 1e9:7.2f} Tpairs/s",
                  flush=True)
        eng.set_hamming_kernel(2)
    for p in (d_a, d_b, d_e, d_c):
        eng.dev_free(p)


# ------------------------------------------------------------------------------------------ square (child: one build)
def leg_square_child(eng):
    cap = 1 << 20
    n, nv_files = 1_000_000, 100_000
    d_h, d_v = eng.dev_alloc(n * 32), eng.dev_alloc(nv_files * 8 * 32)
    d_e, d_c = eng.dev_alloc(cap * 12), eng.dev_alloc(8)
    eng.synth_hashes_dev(d_h, 0, n, n, n_clusters=1000)
    eng.synth_hashes_dev(d_v, 0, nv_files * 8, nv_files * 8, seed=SEED_B)
    eng.synchronize()
    out = {}
    for name, reps, work in (
            ("all pairs 1 M thr 32", 8, lambda: eng.hamming_all_pairs_dev(d_h, n, 32, d_e, cap, d_c)),
            ("all pairs 1 M thr 63", 4, lambda: eng.hamming_all_pairs_dev(d_h, n, 63, d_e, cap, d_c)),
            ("variant sweep 100 k x 8, similarity 40", 8, lambda: eng.hamming_variant_pairs_dev(d_v, 8, d_h, nv_files, 40, d_e, cap, d_c))):
        def run():
            eng.dev_memset(d_c, 0, 8)
            work()
        run()
        out[name] = {"ms": [timed(eng, run, reps) for _ in range(3)], "edges": edge_count(eng, d_c)}
    print("RESULT " + json.dumps(out), flush=True)


def child(leg, tree, *args):
    env = dict(os.environ)
    env.pop("RPH_CROSS_RATE_TREE", None)
    if tree:
        env["RPH_CROSS_RATE_TREE"] = tree
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", leg, *args], env=env, capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        raise SystemExit(f"child {leg} ({tree or 'this build'}) failed with {r.returncode}:\n{r.stdout}\n{r.stderr}")
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])


def leg_square(parent_tree):
    runs = {"this": [], "parent": []}
    for _ in range(ROUNDS):
        runs["parent"].append(child("square", parent_tree))
        runs["this"].append(child("square", None))
    for name in runs["this"][0]:
        for who in ("parent", "this"):
            ms = [m for r in runs[who] for m in r[name]["ms"]]
            edges = {r[name]["edges"] for r in runs[who]}
            print(f"square {name:40s} {who:6s} build  {spread(ms)} ms  median {np.median(ms):.3f}  ({len(ms)} windows in {ROUNDS} processes, edges {sorted(edges)})   all: "
                  + " ".join("%.3f" % m for m in ms), flush=True)


# ------------------------------------------------------------------------------------------ append
N_OLD, N_NEW, SIM = 1_000_000, 10_000, 40


def make_files(eng, path):
    """coefficients (float32, n x 256), hashes and the library's groups, written once for the alternating children"""
    rng = np.random.default_rng(2026)
    n = N_OLD + N_NEW
    coeffs = np.lib.format.open_memmap(os.path.join(path, "coeffs.npy"), mode="w+", dtype=np.float32, shape=(n, 256))
    step = 100_000
    for first in range(0, n, step):
        coeffs[first:first + step] = rng.standard_normal((min(step, n - first), 256), dtype=np.float32) * 20
    near = lambda src: coeffs[src] + rng.standard_normal((len(src), 256), dtype=np.float32) * np.float32(0.8)
    dst = rng.choice(N_OLD, 20_000, replace=False)
    coeffs[np.sort(dst)] = near(rng.integers(0, N_OLD, 20_000))  # near-duplicates inside the library
    coeffs[N_OLD:N_OLD + N_NEW // 2] = near(rng.integers(0, N_OLD, N_NEW // 2))  # half of the new files join it
    hashes = np.zeros((n, 32), np.uint8)
    for first in range(0, n, step):
        hashes[first:first + step] = eng.pdq_hashes_from_coeffs(coeffs[first:first + step], want_dihedral=False)[0]
    np.save(os.path.join(path, "hashes.npy"), hashes)
    coeffs.flush()
    groups, cmp_old = eng.group_files_pdq(hashes[:N_OLD], SIM, coeffs=coeffs[:N_OLD])
    members, offsets = eng._flatten_groups(groups)
    np.save(os.path.join(path, "members.npy"), members)
    np.save(os.path.join(path, "offsets.npy"), offsets)
    return cmp_old, len(groups)


def load_files(path):
    return (np.load(os.path.join(path, "coeffs.npy")), np.load(os.path.join(path, "hashes.npy")), np.load(os.path.join(path, "members.npy")),
            np.load(os.path.join(path, "offsets.npy")))


def leg_regroup_child(eng, path):
    """rph_group_files_pdq on the concatenation (the loaded build: the parent's), end to end from host memory"""
    coeffs, hashes, _, _ = load_files(path)
    out = []
    for _ in range(3):
        t = time.perf_counter()
        groups, cmp_count = eng.group_files_pdq(hashes, SIM, coeffs=coeffs)
        out.append((time.perf_counter() - t) * 1e3)
    print("RESULT " + json.dumps({"ms": out, "groups": len(groups), "comparisons": cmp_count}), flush=True)


def leg_append_child(eng, path):
    coeffs, hashes, members, offsets = load_files(path)
    old_groups = [members[offsets[g]:offsets[g + 1]].tolist() for g in range(len(offsets) - 1)]
    out = []
    for _ in range(3):
        t = time.perf_counter()
        groups, new_cmp = eng.group_files_pdq_append(hashes[:N_OLD], old_groups, hashes[N_OLD:], SIM, old_coeffs=coeffs[:N_OLD], new_coeffs=coeffs[N_OLD:])
        out.append((time.perf_counter() - t) * 1e3)
    print("RESULT " + json.dumps({"ms": out, "groups": len(groups), "comparisons": new_cmp}), flush=True)


def append_stages(eng, path):
    """the append's work stage by stage through the device entry points (what rph_group_files_pdq_append does inside)"""
    from rupphash_amd import EDGE_DTYPE

    coeffs, hashes, members, offsets = load_files(path)
    cap = 1 << 22
    d_co, d_cn = eng.dev_alloc(N_OLD * 1024), eng.dev_alloc(N_NEW * 1024)
    d_vo, d_vn, d_hn = eng.dev_alloc(N_OLD * 256), eng.dev_alloc(N_NEW * 256), eng.dev_alloc(N_NEW * 32)
    d_e, d_c = eng.dev_alloc(cap * 12), eng.dev_alloc(8)
    rows = {"h2d library coefficients (1 GiB, pageable host memory)": [], "h2d new coefficients + hashes": [], "variants of the library (device)": [],
            "variants of the new files (device)": [], "cross sweep 1 M x 8 variants x 10 k": [], "triangular sweep 10 k x 8 variants": [],
            "edges to the host + union-find over old groups": []}
    for _ in range(3):
        def host_ms(f):
            eng.synchronize()
            t = time.perf_counter()
            f()
            eng.synchronize()
            return (time.perf_counter() - t) * 1e3
        rows["h2d library coefficients (1 GiB, pageable host memory)"].append(host_ms(lambda: eng.dev_upload(d_co, coeffs[:N_OLD])))
        rows["h2d new coefficients + hashes"].append(host_ms(lambda: (eng.dev_upload(d_cn, coeffs[N_OLD:]), eng.dev_upload(d_hn, hashes[N_OLD:]))))
        piece = 1 << 18
        rows["variants of the library (device)"].append(timed(eng, lambda: [eng.pdq_hashes_from_coeffs_dev(d_co + f * 1024, min(piece, N_OLD - f), None, d_vo + f * 256)
                                                                           for f in range(0, N_OLD, piece)], 1))
        rows["variants of the new files (device)"].append(timed(eng, lambda: eng.pdq_hashes_from_coeffs_dev(d_cn, N_NEW, None, d_vn), 1))
        eng.dev_memset(d_c, 0, 8)
        rows["cross sweep 1 M x 8 variants x 10 k"].append(timed(eng, lambda: eng.hamming_variant_cross_pairs_dev(d_vo, 8, N_OLD, d_hn, N_NEW, SIM, d_e, cap, d_c), 1))
        rows["triangular sweep 10 k x 8 variants"].append(timed(eng, lambda: eng.hamming_variant_pairs_dev(d_vn, 8, d_hn, N_NEW, SIM, d_e, cap, d_c), 1))

        def finish():
            edges = np.zeros(edge_count(eng, d_c), EDGE_DTYPE)
            eng.dev_download(edges, d_e)
            edges["j"] += N_OLD  # (the timing does not need the exact renumbering of the triangular edges)
            eng.union_find_groups_append((members, offsets), edges, N_OLD + N_NEW)
        rows["edges to the host + union-find over old groups"].append(host_ms(finish))
    for name, ms in rows.items():
        print(f"append stage  {name:60s} {spread(ms)} ms", flush=True)
    for p in (d_co, d_cn, d_vo, d_vn, d_hn, d_e, d_c):
        eng.dev_free(p)


def leg_append(eng, parent_tree):
    with tempfile.TemporaryDirectory(dir="/dev/shm" if os.path.isdir("/dev/shm") else None) as path:
        cmp_old, n_old_groups = make_files(eng, path)
        print(f"append: library {N_OLD} files ({n_old_groups} groups, {cmp_old} comparisons) + {N_NEW} new files, similarity {SIM}", flush=True)
        eng.close()  # the children open the device themselves
        runs = {"regroup": [], "append": []}
        for _ in range(3):
            runs["regroup"].append(child("regroup", parent_tree, path))
            runs["append"].append(child("append", None, path))
        re_, ap = runs["regroup"], runs["append"]
        assert len({r["groups"] for r in re_ + ap}) == 1 and all(r["comparisons"] == re_[0]["comparisons"] for r in re_)
        assert ap[0]["comparisons"] + cmp_old == re_[0]["comparisons"], "the comparison counts do not add up"
        for who, what in (("regroup", "rph_group_files_pdq on the concatenation, parent build"), ("append", "rph_group_files_pdq_append, this build")):
            ms = [m for r in runs[who] for m in r["ms"]]
            first = [r["ms"][0] for r in runs[who]]
            print(f"append end to end  {what:56s} {spread(ms, '%.1f')} ms  median {np.median(ms):.1f}  (first call of each process: {spread(first, '%.1f')})   all: "
                  + " ".join("%.1f" % m for m in ms), flush=True)
        print(f"append: {re_[0]['groups']} groups either way; comparisons {re_[0]['comparisons']} = {cmp_old} (library) + {ap[0]['comparisons']} (new)", flush=True)
        from rupphash_amd import Engine

        eng = Engine(0)
        append_stages(eng, path)
        eng.close()


def main():
    args = sys.argv[1:]
    from rupphash_amd import Engine

    if args[:1] == ["--leg"]:
        eng = Engine(0)
        {"square": leg_square_child, "regroup": leg_regroup_child, "append": leg_append_child}[args[1]](eng, *args[2:])
        eng.close()
        return
    parent_tree = None
    if "--parent-tree" in args:
        k = args.index("--parent-tree")
        parent_tree = os.path.abspath(args[k + 1])
        del args[k:k + 2]
    which = args or ["cross", "square", "append"]
    if ("square" in which or "append" in which) and not (parent_tree and os.path.exists(os.path.join(parent_tree, "rupphash_amd", "librupphash_hip.so"))):
        raise SystemExit("square and append compare with the parent commit: pass --parent-tree DIR, a checkout of it with its library built")
    if "cross" in which:
        eng = Engine(0)
        leg_cross(eng)
        eng.close()
    if "square" in which:
        leg_square(parent_tree)
    if "append" in which:
        leg_append(Engine(0), parent_tree)


if __name__ == "__main__":
    main()
