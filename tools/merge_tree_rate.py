#!/usr/bin/env python3
"""tools/merge_tree_rate.py -- what the merge tree (csrc/merge_tree.hip, host_merge_tree.cpp) saves a caller who moves the similarity.
One MI355X.

The files are the library of tools/library_rate.py: 1 M files with coefficients, 20 k near-duplicates inside it.  Everything is timed by
the host clock around C calls that end in a synchronise, from pageable host memory; each leg makes one untimed call first and then
TIMED timed ones, and min..max is reported.  The parent commit's routes run in a child process that loads the library of --parent-tree
(a checkout of the parent commit with its library built); this build's run in another.

  (a) rph_group_files_pdq_tree(top = 63)          against ONE rph_group_files_pdq at 63 and against the ten calls at SIMS
  (b) rph_library_merge_tree(top = 63) on a resident library (restored at 40)
                                                  against the parent's only route to another similarity: regroup (a call of (a)) and
                                                  rph_library_create + rph_library_restore with those groups
  (c) the core alone in device time (events inside the call: rph_debug_merge_tree_events): check + histogram, init + scatter, level loop;
      and as bytes moved against rph_read_stream_dev on the same box
  (d) rph_merge_tree_groups for one s on the host  against rph_group_files_pdq at that s

The groups of every cut at SIMS are compared with the parent's first (members and offsets, byte for byte).  No bar is fixed in advance; a
row where the new route loses is marked.

usage: merge_tree_rate.py --parent-tree DIR"""
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
sys.path.insert(0, os.environ.get("RPH_MERGE_TREE_RATE_TREE") or os.path.join(HERE, ".."))

TIMED = 15
N, SIM, TOP = 1_000_000, 40, 63
SIMS = (0, 1, 15, 16, 31, 32, 40, 47, 48, 63)


def spread(xs, fmt="%.2f"):
    return (fmt + ".." + fmt) % (min(xs), max(xs))


def p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def make_files(eng, path):
    """the library of tools/library_rate.py, restated: coefficients and hashes, written once for the children"""
    rng = np.random.default_rng(2026)
    coeffs = np.lib.format.open_memmap(os.path.join(path, "coeffs.npy"), mode="w+", dtype=np.float32, shape=(N, 256))
    step = 100_000
    for first in range(0, N, step):
        coeffs[first:first + step] = rng.standard_normal((min(step, N - first), 256), dtype=np.float32) * 20
    near = lambda src: coeffs[src] + rng.standard_normal((len(src), 256), dtype=np.float32) * np.float32(0.8)  # noqa: E731
    dst = rng.choice(N, 20_000, replace=False)
    coeffs[np.sort(dst)] = near(rng.integers(0, N, 20_000))
    hashes = np.zeros((N, 32), np.uint8)
    for first in range(0, N, step):
        hashes[first:first + step] = eng.pdq_hashes_from_coeffs(coeffs[first:first + step], want_dihedral=False)[0]
    np.save(os.path.join(path, "hashes.npy"), hashes)
    coeffs.flush()


def clocked(call):
    t = time.perf_counter()
    rc = call()
    ms = (time.perf_counter() - t) * 1e3
    assert rc == 0, rc
    return ms


def digest(members, offsets, ng):
    return hashlib.sha256(members[: offsets[ng]].tobytes() + offsets[: ng + 1].tobytes()).hexdigest()


def child_parent(eng, path):
    """the parent's routes: the loaded build is the parent's"""
    coeffs, hashes = np.load(os.path.join(path, "coeffs.npy")), np.load(os.path.join(path, "hashes.npy"))
    L = eng.L
    members, offsets = np.zeros(N, np.uint32), np.zeros(N // 2 + 2, np.uint32)
    ng, cmp_count = C.c_uint32(), C.c_uint64()
    group = lambda s: L.rph_group_files_pdq(eng.ctx, p(hashes), p(coeffs), None, None, N, s, p(members), p(offsets), C.byref(ng), C.byref(cmp_count))  # noqa: E731
    res = {"one63": [clocked(lambda: group(TOP)) for _ in range(1 + TIMED)][1:], "ten": [], "cuts": {}}
    for k in range(1 + TIMED):
        t = 0.0
        for s in SIMS:
            t += clocked(lambda: group(s))
            res["cuts"][str(s)] = (digest(members, offsets, ng.value), ng.value, cmp_count.value)
        res["ten"].append(t)
    res["ten"] = res["ten"][1:]
    res["one40"] = [clocked(lambda: group(SIM)) for _ in range(1 + TIMED)][1:]
    om, oo, n_groups = members[: offsets[ng.value]].copy(), offsets[: ng.value + 1].copy(), ng.value
    res["restore"] = []
    for k in range(1 + TIMED):  # the resident library at another similarity: a new one, restored from the regroup
        h = C.c_void_p()
        t = time.perf_counter()
        assert L.rph_library_create(eng.ctx, SIM, C.byref(h)) == 0
        assert L.rph_library_restore(h, p(hashes), p(coeffs), None, None, N, p(om), p(oo), n_groups, 0) == 0
        res["restore"].append((time.perf_counter() - t) * 1e3)
        assert L.rph_library_destroy(h) == 0
    res["restore"] = res["restore"][1:]
    print("RESULT " + json.dumps(res), flush=True)


def child_tree(eng, path):
    """this build's routes"""
    coeffs, hashes = np.load(os.path.join(path, "coeffs.npy")), np.load(os.path.join(path, "hashes.npy"))
    L = eng.L
    into, level, edges_at = np.zeros(N, np.uint32), np.zeros(N, np.uint8), np.zeros(TOP + 1, np.uint64)
    members, offsets = np.zeros(N, np.uint32), np.zeros(N // 2 + 2, np.uint32)
    ng = C.c_uint32()
    ev = [eng.event() for _ in range(4)]
    assert L.rph_debug_merge_tree_events(eng.ctx, *ev) == 0
    res = {"tree": [], "stages": [], "cuts": {}}
    for k in range(1 + TIMED):
        res["tree"].append(clocked(lambda: L.rph_group_files_pdq_tree(eng.ctx, p(hashes), p(coeffs), None, None, N, TOP, p(into), p(level), p(edges_at))))
        res["stages"].append([eng.event_elapsed_ms(ev[j], ev[j + 1]) for j in range(3)])
    assert L.rph_debug_merge_tree_events(eng.ctx, None, None, None, None) == 0
    res["tree"], res["stages"] = res["tree"][1:], res["stages"][1:]
    res["edges"] = int(edges_at.sum())
    res["levels"] = int((edges_at > 0).sum())
    res["merges"] = int((level != 255).sum())
    tree_bytes = into.tobytes() + level.tobytes() + edges_at.tobytes()
    for s in SIMS:
        assert L.rph_merge_tree_groups(p(into), p(level), N, s, p(members), p(offsets), C.byref(ng)) == 0
        res["cuts"][str(s)] = (digest(members, offsets, ng.value), ng.value, int(edges_at[: s + 1].sum()))
    res["cut40"] = [clocked(lambda: L.rph_merge_tree_groups(p(into), p(level), N, SIM, p(members), p(offsets), C.byref(ng))) for _ in range(1 + TIMED)][1:]
    groups, grouped = np.zeros(TOP + 1, np.uint64), np.zeros(TOP + 1, np.uint64)
    res["profile"] = [clocked(lambda: L.rph_merge_tree_profile(p(into), p(level), N, TOP, p(groups), p(grouped))) for _ in range(1 + TIMED)][1:]
    # the resident library, at similarity 40: its tree at 63
    assert L.rph_merge_tree_groups(p(into), p(level), N, SIM, p(members), p(offsets), C.byref(ng)) == 0
    h = C.c_void_p()
    assert L.rph_library_create(eng.ctx, SIM, C.byref(h)) == 0
    assert L.rph_library_restore(h, p(hashes), p(coeffs), None, None, N, p(members), p(offsets), ng.value, int(edges_at[: SIM + 1].sum())) == 0
    i2, l2, e2 = np.zeros(N, np.uint32), np.zeros(N, np.uint8), np.zeros(TOP + 1, np.uint64)
    res["library"] = [clocked(lambda: L.rph_library_merge_tree(h, TOP, p(i2), p(l2), p(e2))) for _ in range(1 + TIMED)][1:]
    res["library_same"] = i2.tobytes() + l2.tobytes() + e2.tobytes() == tree_bytes
    assert L.rph_library_destroy(h) == 0
    # the streaming rate of this box, for (c): 1 GiB read by rph_read_stream_dev
    nbytes = 1 << 30
    d = eng.dev_alloc(nbytes)
    eng.dev_memset(d, 1, nbytes)
    rates = []
    for k in range(6):
        eng.event_record(ev[0])
        eng.read_stream_dev(d, nbytes)
        eng.event_record(ev[1])
        eng.synchronize()
        rates.append(nbytes / eng.event_elapsed_ms(ev[0], ev[1]) / 1e6)
    eng.dev_free(d)
    res["read_gbs"] = rates[1:]
    for e in ev:
        eng.event_destroy(e)
    print("RESULT " + json.dumps(res), flush=True)


def child(leg, tree, path):
    env = dict(os.environ)
    env.pop("RPH_MERGE_TREE_RATE_TREE", None)
    if tree:
        env["RPH_MERGE_TREE_RATE_TREE"] = tree
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", leg, path], env=env, capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        raise SystemExit(f"child {leg} ({tree or 'this build'}) failed with {r.returncode}:\n{r.stdout}\n{r.stderr}")
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])


def row(tag, what, new, old):
    lost = min(new) >= min(old)
    line = f"{tag} {what:64s} {spread(new)}   against {spread(old)}   (min / min = {min(old) / min(new):.1f} x)"
    print(("**" + line + "  -- the new route loses**") if lost else line, flush=True)


def main():
    args = sys.argv[1:]
    from rupphash_amd import Engine

    if args[:1] == ["--leg"]:
        eng = Engine(0)
        {"parent": child_parent, "tree": child_tree}[args[1]](eng, args[2])
        eng.close()
        return
    if "--parent-tree" not in args:
        raise SystemExit(__doc__)
    parent_tree = os.path.abspath(args[args.index("--parent-tree") + 1])
    if not os.path.exists(os.path.join(parent_tree, "rupphash_amd", "librupphash_hip.so")):
        raise SystemExit("--parent-tree: a checkout of the parent commit with its library built")
    with tempfile.TemporaryDirectory(dir="/dev/shm" if os.path.isdir("/dev/shm") else None) as path:
        eng = Engine(0)
        make_files(eng, path)
        eng.close()  # the children open the device themselves
        print(f"{N} files with coefficients, 20 k near-duplicates; top {TOP}; one process per build, 1 untimed + {TIMED} timed calls per leg; host clock, ms, min..max", flush=True)
        a = child("parent", parent_tree, path)
        b = child("tree", None, path)
    assert a["cuts"] == b["cuts"], "a cut of the tree differs from rph_group_files_pdq of the parent build"
    assert b["library_same"], "rph_library_merge_tree and rph_group_files_pdq_tree differ"
    print(f"cuts at {SIMS}: groups (members, offsets) and comparison counts identical to the parent's rph_group_files_pdq, byte for byte; "
          f"{b['edges']} edges at 63 on {b['levels']} levels, {b['merges']} files absorbed; the library form returns the same bytes", flush=True)
    row("(a)", "rph_group_files_pdq_tree(63) against ONE rph_group_files_pdq(63)", b["tree"], a["one63"])
    row("(a)", "rph_group_files_pdq_tree(63) against the ten calls at SIMS", b["tree"], a["ten"])
    row("(b)", "rph_library_merge_tree(63), resident, against create + restore", b["library"], a["restore"])
    row("(b)", "  ... against regroup at 40 + create + restore", b["library"], [x + y for x, y in zip(a["one40"], a["restore"])])
    stages = np.array(b["stages"])
    for k, name in enumerate(("check + histogram", "init + scatter", "level loop (2 launches per non-empty level)")):
        print(f"(c) device time  {name:48s} {spread(stages[:, k], '%.3f')}  median {np.median(stages[:, k]):.3f}", flush=True)
    print(f"(c) device time  {'sum':48s} {spread(stages.sum(1), '%.3f')}  median {np.median(stages.sum(1)):.3f}", flush=True)
    e, gbs = b["edges"], float(np.median(b["read_gbs"]))
    moved = [12 * e, 2 * 12 * e + 8 * e + 9 * N, 8 * e + 9 * b["merges"]]
    print(f"(c) rph_read_stream_dev on this box: {spread(b['read_gbs'], '%.0f')} GB/s; the stages' compulsory bytes ({', '.join('%.1f MB' % (m / 1e6) for m in moved)}) "
          f"at that rate: {', '.join('%.3f' % (m / gbs / 1e6) for m in moved)} ms", flush=True)
    row("(d)", f"rph_merge_tree_groups(s = {SIM}) on the host against rph_group_files_pdq({SIM})", b["cut40"], a["one40"])
    print(f"(d) rph_merge_tree_profile, all {TOP + 1} levels   {spread(b['profile'])}", flush=True)


if __name__ == "__main__":
    main()
