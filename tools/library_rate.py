#!/usr/bin/env python3
"""tools/library_rate.py -- what a device-resident library (rph_library, csrc/library.cpp + components.hip) saves an append.  One MI355X.

The files are those of tools/cross_rate.py's append leg: a library of 1 M files with coefficients (20 k near-duplicates inside it) plus
10 k new files, half of them near-duplicates of library files, similarity 40.  Everything is timed by the host clock around C calls that
end in a synchronise, from pageable host memory, in child processes that alternate between the two builds; each child makes one
untimed call first and then TIMED timed ones.

  (a) rph_group_files_pdq_append of --parent-tree (a checkout of the parent commit with its library built), the whole call
  (b) rph_library_append of the same 10 k files onto the resident 1 M; the library is restored before each timed call
  (c) the one-time costs: rph_library_restore of 1 M, and building the library by one rph_library_append of 1 M (once)
  (d) rph_library_groups of 1 M + 10 k
  (e) (b) stage by stage in device time (events inside the call: rph_debug_library_stages)

The groups of (a) and (b) are compared first (members and offsets, byte for byte).  The bar: max of (b) < min of (a).

usage: library_rate.py --parent-tree DIR"""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# a child that measures the parent commit imports the package (and with it the library) of that checkout
sys.path.insert(0, os.environ.get("RPH_LIBRARY_RATE_TREE") or os.path.join(HERE, ".."))

ROUNDS, TIMED = 3, 5
N_OLD, N_NEW, SIM = 1_000_000, 10_000, 40
STAGES = ("upload + variants of the new files", "cross sweep 1 M x 8 variants x 10 k", "triangular sweep 10 k x 8 variants",
          "cursor to the host, union + flatten kernels", "labels to the host")


def spread(xs, fmt="%.2f"):
    return (fmt + ".." + fmt) % (min(xs), max(xs))


def p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def make_files(eng, path):
    """tools/cross_rate.py's files, restated: coefficients, hashes and the library's groups, written once for the children"""
    rng = np.random.default_rng(2026)
    n = N_OLD + N_NEW
    coeffs = np.lib.format.open_memmap(os.path.join(path, "coeffs.npy"), mode="w+", dtype=np.float32, shape=(n, 256))
    step = 100_000
    for first in range(0, n, step):
        coeffs[first:first + step] = rng.standard_normal((min(step, n - first), 256), dtype=np.float32) * 20
    near = lambda src: coeffs[src] + rng.standard_normal((len(src), 256), dtype=np.float32) * np.float32(0.8)  # noqa: E731
    dst = rng.choice(N_OLD, 20_000, replace=False)
    coeffs[np.sort(dst)] = near(rng.integers(0, N_OLD, 20_000))
    coeffs[N_OLD:N_OLD + N_NEW // 2] = near(rng.integers(0, N_OLD, N_NEW // 2))
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


def clocked(call):
    t = time.perf_counter()
    rc = call()
    ms = (time.perf_counter() - t) * 1e3
    assert rc == 0, rc
    return ms


def digest(members, offsets, ng):
    return hashlib.sha256(members[: offsets[ng]].tobytes() + offsets[: ng + 1].tobytes()).hexdigest()


def child_parent_append(eng, path):
    """(a): the loaded build is the parent's"""
    coeffs, hashes, om, oo = load_files(path)
    n = N_OLD + N_NEW
    members, offsets = np.zeros(n, np.uint32), np.zeros(n // 2 + 2, np.uint32)
    ng, cmp_new = C.c_uint32(), C.c_uint64()
    oh, oc, nh, nc = hashes[:N_OLD], coeffs[:N_OLD], hashes[N_OLD:], coeffs[N_OLD:]
    call = lambda: eng.L.rph_group_files_pdq_append(eng.ctx, p(oh), p(oc), None, None, N_OLD, p(om), p(oo), len(oo) - 1, p(nh), p(nc), None, None, N_NEW,  # noqa: E731
                                                    SIM, p(members), p(offsets), C.byref(ng), C.byref(cmp_new))
    ms = [clocked(call) for _ in range(1 + TIMED)]
    print("RESULT " + json.dumps({"warm": ms[0], "ms": ms[1:], "groups": ng.value, "comparisons": cmp_new.value,
                                  "digest": digest(members, offsets, ng.value)}), flush=True)


def child_library(eng, path, build_once):
    """(b) to (e): this build"""
    coeffs, hashes, om, oo = load_files(path)
    n = N_OLD + N_NEW
    L = eng.L
    oh, oc, nh, nc = hashes[:N_OLD], coeffs[:N_OLD], hashes[N_OLD:], coeffs[N_OLD:]
    members, offsets, labels = np.zeros(n, np.uint32), np.zeros(n // 2 + 2, np.uint32), np.zeros(N_NEW, np.uint32)
    ng, cmp_new = C.c_uint32(), C.c_uint64()
    out = {"restore": [], "append": [], "groups_ms": [], "stages": []}
    for k in range(1 + TIMED):
        h = C.c_void_p()
        assert L.rph_library_create(eng.ctx, SIM, C.byref(h)) == 0
        assert L.rph_library_reserve(h, n) == 0
        out["restore"].append(clocked(lambda: L.rph_library_restore(h, p(oh), p(oc), None, None, N_OLD, p(om), p(oo), len(oo) - 1, 0)))
        assert L.rph_debug_library_stages(h, 1, None) == 0
        out["append"].append(clocked(lambda: L.rph_library_append(h, p(nh), p(nc), None, None, N_NEW, p(labels), C.byref(cmp_new))))
        stage_ms = (C.c_float * 5)()
        assert L.rph_debug_library_stages(h, 0, stage_ms) == 0
        out["stages"].append(list(stage_ms))
        out["groups_ms"].append(clocked(lambda: L.rph_library_groups(h, p(members), p(offsets), C.byref(ng))))
        assert L.rph_library_destroy(h) == 0
    res = {"warm": out["append"][0], "ms": out["append"][1:], "restore_ms": out["restore"][1:], "groups_ms": out["groups_ms"][1:], "stages": out["stages"][1:],
           "groups": ng.value, "comparisons": cmp_new.value, "digest": digest(members, offsets, ng.value)}
    if build_once == "1":  # the other way to get the library: one append of everything (the square sweep of 1 M x 8 variants)
        h = C.c_void_p()
        assert L.rph_library_create(eng.ctx, SIM, C.byref(h)) == 0
        res["build_ms"] = clocked(lambda: L.rph_library_append(h, p(oh), p(oc), None, None, N_OLD, None, C.byref(cmp_new)))
        res["build_comparisons"] = cmp_new.value
        assert L.rph_library_append(h, p(nh), p(nc), None, None, N_NEW, None, C.byref(cmp_new)) == 0
        assert L.rph_library_groups(h, p(members), p(offsets), C.byref(ng)) == 0
        res["build_digest"] = digest(members, offsets, ng.value)
        assert L.rph_library_destroy(h) == 0
    print("RESULT " + json.dumps(res), flush=True)


def child(leg, tree, *args):
    env = dict(os.environ)
    env.pop("RPH_LIBRARY_RATE_TREE", None)
    if tree:
        env["RPH_LIBRARY_RATE_TREE"] = tree
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", leg, *args], env=env, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise SystemExit(f"child {leg} ({tree or 'this build'}) failed with {r.returncode}:\n{r.stdout}\n{r.stderr}")
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])


def main():
    args = sys.argv[1:]
    from rupphash_amd import Engine

    if args[:1] == ["--leg"]:
        eng = Engine(0)
        {"parent-append": child_parent_append, "library": child_library}[args[1]](eng, *args[2:])
        eng.close()
        return
    if "--parent-tree" not in args:
        raise SystemExit(__doc__)
    parent_tree = os.path.abspath(args[args.index("--parent-tree") + 1])
    if not os.path.exists(os.path.join(parent_tree, "rupphash_amd", "librupphash_hip.so")):
        raise SystemExit("--parent-tree: a checkout of the parent commit with its library built")
    with tempfile.TemporaryDirectory(dir="/dev/shm" if os.path.isdir("/dev/shm") else None) as path:
        eng = Engine(0)
        cmp_old, n_old_groups = make_files(eng, path)
        eng.close()  # the children open the device themselves
        print(f"library {N_OLD} files ({n_old_groups} groups, {cmp_old} comparisons) + {N_NEW} new files, similarity {SIM}; {ROUNDS} processes per build, "
              f"alternating, 1 untimed + {TIMED} timed calls each; host clock, ms", flush=True)
        a, b = [], []
        for r in range(ROUNDS):
            a.append(child("parent-append", parent_tree, path))
            b.append(child("library", None, path, "1" if r == 0 else "0"))
        same = {x["digest"] for x in a + b} | {b[0]["build_digest"]}
        assert len(same) == 1 and len({(x["groups"], x["comparisons"]) for x in a + b}) == 1, "the two builds group differently"
        print(f"groups: {a[0]['groups']} either way, members and offsets identical (also when the library is built by appends alone); "
              f"{a[0]['comparisons']} new comparisons", flush=True)
        ms_a, ms_b = [m for x in a for m in x["ms"]], [m for x in b for m in x["ms"]]
        for tag, what, ms, runs in (("(a)", "rph_group_files_pdq_append, parent build", ms_a, a), ("(b)", "rph_library_append onto the resident 1 M, this build", ms_b, b)):
            print(f"{tag} {what:56s} {spread(ms)}  median {np.median(ms):.2f}  (untimed first calls {spread([x['warm'] for x in runs])})   all: "
                  + " ".join("%.2f" % m for m in ms), flush=True)
        print(f"bar: max (b) {max(ms_b):.2f} < min (a) {min(ms_a):.2f}: {'MET' if max(ms_b) < min(ms_a) else 'NOT MET'}   "
              f"(median (a) / median (b) = {np.median(ms_a) / np.median(ms_b):.1f})", flush=True)
        print(f"(c) rph_library_restore of 1 M (1 GiB of coefficients from pageable memory, variants, labels)   {spread([m for x in b for m in x['restore_ms']], '%.1f')}",
              flush=True)
        print(f"(c) building it by one rph_library_append of 1 M ({b[0]['build_comparisons']} comparisons; first call of its process)   {b[0]['build_ms']:.1f}", flush=True)
        print(f"(d) rph_library_groups of 1 M + 10 k   {spread([m for x in b for m in x['groups_ms']])}", flush=True)
        stages = np.array([s for x in b for s in x["stages"]])
        for k, name in enumerate(STAGES):
            print(f"(e) device time  {name:48s} {spread(stages[:, k], '%.3f')}  median {np.median(stages[:, k]):.3f}", flush=True)
        print(f"(e) device time  {'sum':48s} {spread(stages.sum(1), '%.3f')}  median {np.median(stages.sum(1)):.3f}", flush=True)
        slow = int(np.argmax(ms_b))
        print(f"(e) the slowest call of (b), {max(ms_b):.2f} ms on the host clock, by stage: " + " ".join("%.3f" % v for v in stages[slow]), flush=True)


if __name__ == "__main__":
    main()
