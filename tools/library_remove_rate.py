#!/usr/bin/env python3
"""tools/library_remove_rate.py -- what rph_library_remove (csrc/library.cpp + library_kernels.hip) saves a caller whose files disappear.
One MI355X.

The files are those of tools/library_rate.py: 1 M files with coefficients (20 k near-duplicates among them), similarity 40; the 10 k
further files of that corpus are not used.  Everything is timed by the host clock around C calls that end in a synchronise, from pageable
host memory, in child processes that alternate between the two builds; each child makes one untimed call first and then TIMED timed ones.

  (a) what the parent commit offers (--parent-tree, a checkout of it with its library built) when files are gone: rph_group_files_pdq of
      the survivors from host memory (the host's compaction of its arrays is not timed), and, to have a resident library again,
      rph_library_restore of the survivors with those groups
  (b) rph_library_remove of 10 000 random files from the resident 1 M, new_index and dropped asked for; the library is restored before
      each timed call
  (c) the same for 100 and for 100 000 files
  (d) (b) stage by stage in device time (events inside the call: rph_debug_library_remove_stages)

The groups (members and offsets, byte for byte) and the comparison counts of (a) and of (b), (c) are compared first.  The bar: max of (b)
< min of (a), over both calls of (a).

usage: library_remove_rate.py --parent-tree DIR"""
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.environ.get("RPH_LIBRARY_RATE_TREE") or os.path.join(HERE, ".."))
sys.path.insert(1, HERE)

from library_rate import N_NEW, N_OLD, SIM, clocked, digest, load_files, make_files, p, spread  # noqa: E402

ROUNDS, TIMED = 3, 5
COUNTS = (10_000, 100, 100_000)  # (b), then (c)
STAGES = ("indices up, mark, flags, scan + two selects", "gather of the regrouped members", "regroup sweep m x 8 variants",
          "edge split, dropped to the host", "compaction of the survivors, labels", "range check, union + flatten kernels")


def removal(count):
    return np.random.default_rng(count).choice(N_OLD, count, replace=False).astype(np.uint32)


def child_parent(eng, path):
    """(a): the loaded build is the parent's"""
    coeffs, hashes, _, _ = load_files(path)
    L = eng.L
    res = {}
    for count in COUNTS:
        keep = np.ones(N_OLD, bool)
        keep[removal(count)] = False
        h, c = np.ascontiguousarray(hashes[:N_OLD][keep]), np.ascontiguousarray(coeffs[:N_OLD][keep])
        n = len(h)
        members, offsets = np.zeros(n, np.uint32), np.zeros(n // 2 + 2, np.uint32)
        ng, cmp_count = C.c_uint32(), C.c_uint64()
        calls = 1 + TIMED if count == COUNTS[0] else 2
        ms = [clocked(lambda: L.rph_group_files_pdq(eng.ctx, p(h), p(c), None, None, n, SIM, p(members), p(offsets), C.byref(ng), C.byref(cmp_count)))
              for _ in range(calls)]
        res[str(count)] = {"regroup_ms": ms[1:], "groups": ng.value, "comparisons": cmp_count.value, "digest": digest(members, offsets, ng.value)}
        if count != COUNTS[0]:
            continue
        restore = []
        for _ in range(1 + TIMED):
            lib = C.c_void_p()
            assert L.rph_library_create(eng.ctx, SIM, C.byref(lib)) == 0
            assert L.rph_library_reserve(lib, n) == 0
            restore.append(clocked(lambda: L.rph_library_restore(lib, p(h), p(c), None, None, n, p(members), p(offsets), ng.value, cmp_count.value)))
            assert L.rph_library_destroy(lib) == 0
        res[str(count)]["restore_ms"] = restore[1:]
    print("RESULT " + json.dumps(res), flush=True)


def child_remove(eng, path):
    """(b) to (d): this build"""
    coeffs, hashes, om, oo = load_files(path)
    L = eng.L
    oh, oc = hashes[:N_OLD], coeffs[:N_OLD]
    cmp_old = int(np.load(os.path.join(path, "cmp_old.npy"))[0])
    res = {}
    for count in COUNTS:
        idx = removal(count)
        n = N_OLD - count
        members, offsets, new_index = np.zeros(n, np.uint32), np.zeros(n // 2 + 2, np.uint32), np.zeros(N_OLD, np.uint32)
        ng, dropped, size, cmp_count = C.c_uint32(), C.c_uint64(), C.c_uint64(), C.c_uint64()
        ms, stages, stats = [], [], (C.c_uint64 * 4)()
        for _ in range(1 + TIMED):
            lib = C.c_void_p()
            assert L.rph_library_create(eng.ctx, SIM, C.byref(lib)) == 0
            assert L.rph_library_restore(lib, p(oh), p(oc), None, None, N_OLD, p(om), p(oo), len(oo) - 1, cmp_old) == 0
            assert L.rph_debug_library_stages(lib, 1, None) == 0
            ms.append(clocked(lambda: L.rph_library_remove(lib, p(idx), count, p(new_index), C.byref(dropped))))
            stage_ms = (C.c_float * 6)()
            assert L.rph_debug_library_remove_stages(lib, stage_ms) == 0
            stages.append(list(stage_ms))
            assert L.rph_debug_library_remove_stats(lib, stats) == 0
            assert L.rph_library_groups(lib, p(members), p(offsets), C.byref(ng)) == 0
            assert L.rph_library_size(lib, C.byref(size), C.byref(cmp_count)) == 0 and size.value == n
            assert L.rph_library_destroy(lib) == 0
        keep = np.ones(N_OLD, bool)
        keep[idx] = False
        assert np.array_equal(new_index, np.where(keep, np.cumsum(keep) - 1, 0xFFFFFFFF).astype(np.uint32))
        res[str(count)] = {"warm": ms[0], "ms": ms[1:], "stages": stages[1:], "groups": ng.value, "comparisons": cmp_count.value, "dropped": dropped.value,
                           "digest": digest(members, offsets, ng.value), "m": stats[0], "edges": stats[1]}
    print("RESULT " + json.dumps(res), flush=True)


def child(leg, tree, *args):
    env = dict(os.environ)
    env.pop("RPH_LIBRARY_RATE_TREE", None)
    if tree:
        env["RPH_LIBRARY_RATE_TREE"] = tree
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", leg, *args], env=env, capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        raise SystemExit(f"child {leg} ({tree or 'this build'}) failed with {r.returncode}:\n{r.stdout}\n{r.stderr}")
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])


def main():
    args = sys.argv[1:]
    from rupphash_amd import Engine

    if args[:1] == ["--leg"]:
        eng = Engine(0)
        {"parent": child_parent, "remove": child_remove}[args[1]](eng, *args[2:])
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
        np.save(os.path.join(path, "cmp_old.npy"), np.array([cmp_old], np.uint64))
        print(f"library {N_OLD} files ({n_old_groups} groups, {cmp_old} comparisons; the corpus of tools/library_rate.py without its {N_NEW} new files), "
              f"similarity {SIM}; {ROUNDS} processes per build, alternating, 1 untimed + {TIMED} timed calls each; host clock, ms", flush=True)
        a, b = [], []
        for r in range(ROUNDS):
            a.append(child("parent", parent_tree, path))
            b.append(child("remove", None, path))
            print(f"processes {r + 1} of {ROUNDS} of each build done", file=sys.stderr, flush=True)
        for count in map(str, COUNTS):
            same = {(x[count]["digest"], x[count]["groups"], x[count]["comparisons"]) for x in a + b}
            assert len(same) == 1, f"the two builds group the survivors of {count} removals differently"
            one = b[0][count]
            print(f"remove {count:>6s}: {one['groups']} groups and {one['comparisons']} comparisons either way, members and offsets identical, new_index as numpy; "
                  f"{one['dropped']} comparisons dropped, {one['m']} members regrouped, {one['edges']} edges among them", flush=True)
        first = str(COUNTS[0])
        ms_regroup = [m for x in a for m in x[first]["regroup_ms"]]
        ms_restore = [m for x in a for m in x[first]["restore_ms"]]
        ms_b = [m for x in b for m in x[first]["ms"]]
        for tag, what, ms in (("(a)", "rph_group_files_pdq of the 990 000 survivors, parent build", ms_regroup),
                              ("(a)", "rph_library_restore of them with those groups, parent build", ms_restore),
                              ("(b)", "rph_library_remove of 10 000 from the resident 1 M, this build", ms_b)):
            print(f"{tag} {what:64s} {spread(ms)}  median {np.median(ms):.2f}   all: " + " ".join("%.2f" % m for m in ms), flush=True)
        print(f"    untimed first calls of (b): {spread([x[first]['warm'] for x in b])}", flush=True)
        fastest_a = min(ms_regroup + ms_restore)
        print(f"bar: max (b) {max(ms_b):.2f} < min (a) {fastest_a:.2f}: {'MET' if max(ms_b) < fastest_a else 'NOT MET'}   "
              f"(median regroup / median (b) = {np.median(ms_regroup) / np.median(ms_b):.1f}, median restore / median (b) = {np.median(ms_restore) / np.median(ms_b):.1f}, "
              f"median regroup + restore / median (b) = {(np.median(ms_regroup) + np.median(ms_restore)) / np.median(ms_b):.1f})", flush=True)
        for count in map(str, COUNTS[1:]):
            ms = [m for x in b for m in x[count]["ms"]]
            ref = [m for x in a for m in x[count]["regroup_ms"]]
            print(f"(c) rph_library_remove of {count:>6s}   {spread(ms)}  median {np.median(ms):.2f}   (rph_group_files_pdq of the survivors, parent build, one timed call "
                  f"per process: {spread(ref)})", flush=True)
        for count in map(str, COUNTS):
            stages = np.array([s for x in b for s in x[count]["stages"]])
            tag = "(d)" if count == first else "   "
            for k, name in enumerate(STAGES):
                print(f"{tag} device time, {count:>6s} removed  {name:48s} {spread(stages[:, k], '%.3f')}  median {np.median(stages[:, k]):.3f}", flush=True)
            print(f"{tag} device time, {count:>6s} removed  {'sum':48s} {spread(stages.sum(1), '%.3f')}  median {np.median(stages.sum(1)):.3f}", flush=True)
            # what the host adds: five allocations and frees of the resident twins, the sort of the indices, new_index, waits
            rest = np.array([m for x in b for m in x[count]["ms"]]) - stages.sum(1)
            print(f"{tag} host clock minus device time, {count:>6s} removed  {'':28s} {spread(rest, '%.3f')}  median {np.median(rest):.3f}", flush=True)
        # the compaction: 290 bytes read and written per survivor (its kernel also shares its stage with the label kernel)
        gather = np.array([s[4] for x in b for s in x[first]["stages"]])
        print(f"(d) compaction stage as a stream: 2 x 290 B x {N_OLD - COUNTS[0]} survivors + 2 x 4 B labels in {np.median(gather):.3f} ms = "
              f"{(2 * 290 + 8) * (N_OLD - COUNTS[0]) / np.median(gather) / 1e9:.2f} TB/s", flush=True)


if __name__ == "__main__":
    main()
