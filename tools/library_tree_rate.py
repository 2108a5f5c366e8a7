#!/usr/bin/env python3
"""tools/library_tree_rate.py -- what a library that keeps its edges (rph_library_create_tree, csrc/library.cpp + library_edges.hip) saves
a caller who moves the similarity of a resident collection, and what it costs on every append and removal.  One MI355X.

The files are those of tools/library_rate.py: 1 M files with coefficients (20 k near-duplicates among them) plus 10 k new files, half of
them near-duplicates of library files; similarity 40, top 63.  Everything is timed by the host clock around C calls that end in a
synchronise, from pageable host memory; each leg makes one untimed call first and then TIMED timed ones, and min..max is reported.  The
parent commit's calls run in a child process that loads the library of --parent-tree (a checkout of the parent commit with its library
built); this build's run in another.

  (1) rph_library_merge_tree(63) and (40) on the resident 1 M: a library with its edges (top 63) against the parent's sweep path
  (2) rph_library_append of the 10 k files at similarity 40: with edges at top 63, with edges at top 40, and a plain library (this build
      and the parent's); the library is put back before each timed call (rph_library_restore_edges / rph_library_restore)
  (3) rph_library_remove of 10 000 random files: with edges (top 63) against plain (this build and the parent's)
      In (2) and (3) this build's process runs the plain leg and the top-63 leg a second time at its end: the order of the legs has shown
      in these figures, and a row measured once could not tell that from the kind of library
  (4) the store's size in edges and bytes
  (5) the first fill: one rph_library_append of the 1 M into an empty library with edges (top 63, top 40) and a plain one (this build and
      the parent's), the three kinds in turn in every round, the first round untimed; and rph_library_restore_edges / rph_library_edges
      of the 1 M

The tree bytes of (1) and the groups and counts after (2) and (3) are compared between the builds and the kinds of library first.  The
bar for (1): max of the new calls < min of the parent's.  (2), (3) and (5) are costs; they are printed as they are.

usage: library_tree_rate.py --parent-tree DIR"""
import ctypes as C
import hashlib
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

TIMED, TOP, N_REMOVE = 10, 63, 10_000
KINDS = (("edges, top 63", TOP), ("edges, top 40", SIM), ("plain", None))
EDGE = np.dtype([("i", np.uint32), ("j", np.uint32), ("d", np.uint16), ("flags", np.uint16)])


def removal():
    return np.random.default_rng(N_REMOVE).choice(N_OLD, N_REMOVE, replace=False).astype(np.uint32)


def tree_digest(into, level, edges_at):
    return hashlib.sha256(into.tobytes() + level.tobytes() + edges_at.tobytes()).hexdigest()


class Legs:
    """the legs both builds run on a plain library: trees by the sweep path, append, removal"""

    def __init__(self, eng, path):
        self.eng, self.L = eng, eng.L
        self.coeffs, self.hashes, self.om, self.oo = load_files(path)
        self.cmp_old = int(np.load(os.path.join(path, "cmp_old.npy"))[0])
        self.oh, self.oc, self.nh, self.nc = self.hashes[:N_OLD], self.coeffs[:N_OLD], self.hashes[N_OLD:], self.coeffs[N_OLD:]
        n = N_OLD + N_NEW
        self.members, self.offsets, self.labels, self.new_index = np.zeros(n, np.uint32), np.zeros(n // 2 + 2, np.uint32), np.zeros(N_NEW, np.uint32), np.zeros(N_OLD, np.uint32)
        self.into, self.level, self.edges_at = np.zeros(N_OLD, np.uint32), np.zeros(N_OLD, np.uint8), np.zeros(TOP + 1, np.uint64)

    def plain(self):
        lib = C.c_void_p()
        assert self.L.rph_library_create(self.eng.ctx, SIM, C.byref(lib)) == 0
        assert self.L.rph_library_restore(lib, p(self.oh), p(self.oc), None, None, N_OLD, p(self.om), p(self.oo), len(self.oo) - 1, self.cmp_old) == 0
        return lib

    def state(self, lib):
        ng, size, cmp_count = C.c_uint32(), C.c_uint64(), C.c_uint64()
        assert self.L.rph_library_groups(lib, p(self.members), p(self.offsets), C.byref(ng)) == 0
        assert self.L.rph_library_size(lib, C.byref(size), C.byref(cmp_count)) == 0
        return [digest(self.members, self.offsets, ng.value), ng.value, size.value, cmp_count.value]

    def trees(self, lib):
        out = {}
        for t in (TOP, SIM):
            e = self.edges_at[: t + 1]
            ms = [clocked(lambda: self.L.rph_library_merge_tree(lib, t, p(self.into), p(self.level), p(e))) for _ in range(1 + TIMED)]
            out[str(t)] = {"ms": ms[1:], "digest": tree_digest(self.into, self.level, e)}
        return out

    def fill(self, top):
        """one rph_library_append of the 1 M into an empty library with room for them (top None: a plain one): (ms, the library)"""
        lib, cmp_new = C.c_void_p(), C.c_uint64()
        create = self.L.rph_library_create(self.eng.ctx, SIM, C.byref(lib)) if top is None else self.L.rph_library_create_tree(self.eng.ctx, SIM, top, 0, C.byref(lib))
        assert create == 0 and self.L.rph_library_reserve(lib, N_OLD + N_NEW) == 0
        ms = clocked(lambda: self.L.rph_library_append(lib, p(self.oh), p(self.oc), None, None, N_OLD, None, C.byref(cmp_new)))
        assert cmp_new.value == self.cmp_old
        return ms, lib

    def appends(self, make):
        ms, cmp_new = [], C.c_uint64()
        for _ in range(1 + TIMED):
            lib = make()
            ms.append(clocked(lambda: self.L.rph_library_append(lib, p(self.nh), p(self.nc), None, None, N_NEW, p(self.labels), C.byref(cmp_new))))
            state = self.state(lib) + [cmp_new.value, hashlib.sha256(self.labels.tobytes()).hexdigest()]
            assert self.L.rph_library_destroy(lib) == 0
        return {"ms": ms[1:], "state": state}

    def removals(self, make):
        ms, dropped, idx = [], C.c_uint64(), removal()
        for _ in range(1 + TIMED):
            lib = make()
            ms.append(clocked(lambda: self.L.rph_library_remove(lib, p(idx), N_REMOVE, p(self.new_index), C.byref(dropped))))
            state = self.state(lib) + [dropped.value, hashlib.sha256(self.new_index.tobytes()).hexdigest()]
            assert self.L.rph_library_destroy(lib) == 0
        return {"ms": ms[1:], "state": state}


def child_parent(eng, path):
    """the loaded build is the parent's: its plain library"""
    legs = Legs(eng, path)
    lib = legs.plain()
    res = {"tree": legs.trees(lib)}
    assert eng.L.rph_library_destroy(lib) == 0
    res["append"] = legs.appends(legs.plain)
    res["remove"] = legs.removals(legs.plain)
    res["fill"] = []
    for _ in range(1 + TIMED):
        ms, lib = legs.fill(None)
        res["fill"].append(ms)
        assert eng.L.rph_library_destroy(lib) == 0
    res["fill"] = res["fill"][1:]
    print("RESULT " + json.dumps(res), flush=True)


def child_tree(eng, path):
    """this build: a plain library again, and the libraries with edges"""
    legs = Legs(eng, path)
    L = eng.L
    res = {"fill": {name: [] for name, _ in KINDS}, "store": {}}
    stores = {}
    # (5) and (4): the first fill, the kinds in turn in every round so that none is the cold one, the first round untimed; the libraries of
    # the last round give the stores and, at top 63, the trees of (1)
    for k in range(1 + TIMED):
        for name, top in KINDS:
            ms, lib = legs.fill(top)
            res["fill"][name].append(ms)
            if k == TIMED and top is not None:
                found = C.c_uint64()
                assert L.rph_library_edges(lib, None, 0, C.byref(found)) in (0, -6)
                e = np.zeros(found.value, EDGE)
                down = [clocked(lambda: L.rph_library_edges(lib, p(e), len(e), C.byref(found))) for _ in range(1 + TIMED)]
                stores[top] = e
                res["store"][name] = {"edges": len(e), "bytes": e.nbytes, "download_ms": down[1:]}
            if k == TIMED and top == TOP:
                res["tree"] = legs.trees(lib)
                stats = (C.c_uint64 * 5)()
                assert L.rph_debug_library_edge_stats(lib, stats) == 0
                res["swept"] = stats[4]
            assert L.rph_library_destroy(lib) == 0
    res["fill"] = {name: ms[1:] for name, ms in res["fill"].items()}

    def with_edges(top):
        def make():
            lib = C.c_void_p()
            assert L.rph_library_create_tree(eng.ctx, SIM, top, 0, C.byref(lib)) == 0
            assert L.rph_library_restore_edges(lib, p(legs.oh), p(legs.oc), None, None, N_OLD, p(stores[top]), len(stores[top])) == 0
            return lib
        return make

    res["restore_edges"] = []
    for _ in range(1 + TIMED):
        lib = C.c_void_p()
        assert L.rph_library_create_tree(eng.ctx, SIM, TOP, 0, C.byref(lib)) == 0
        res["restore_edges"].append(clocked(lambda: L.rph_library_restore_edges(lib, p(legs.oh), p(legs.oc), None, None, N_OLD, p(stores[TOP]), len(stores[TOP]))))
        state = legs.state(lib)
        assert L.rph_library_destroy(lib) == 0
    res["restore_edges"], res["restored_state"] = res["restore_edges"][1:], state
    lib = legs.plain()
    res["plain_state"] = legs.state(lib)
    res["plain_tree"] = legs.trees(lib)
    assert L.rph_library_destroy(lib) == 0
    # (both kinds once more at the end: the same calls, so what a pair differs by is the process's history, not the library)
    res["append"] = {"plain": legs.appends(legs.plain), "edges, top 63": legs.appends(with_edges(TOP)), "edges, top 40": legs.appends(with_edges(SIM)),
                     "plain, once more": legs.appends(legs.plain), "edges, top 63, once more": legs.appends(with_edges(TOP))}
    res["remove"] = {"plain": legs.removals(legs.plain), "edges, top 63": legs.removals(with_edges(TOP)), "plain, once more": legs.removals(legs.plain),
                     "edges, top 63, once more": legs.removals(with_edges(TOP))}
    print("RESULT " + json.dumps(res), flush=True)


def child(leg, tree, path):
    env = dict(os.environ)
    env.pop("RPH_LIBRARY_RATE_TREE", None)
    if tree:
        env["RPH_LIBRARY_RATE_TREE"] = tree
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", leg, path], env=env, capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        raise SystemExit(f"child {leg} ({tree or 'this build'}) failed with {r.returncode}:\n{r.stdout}\n{r.stderr}")
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])


def line(tag, what, ms):
    print(f"{tag} {what:72s} {spread(ms)}  median {np.median(ms):.2f}", flush=True)


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
        cmp_old, n_old_groups = make_files(eng, path)
        eng.close()  # the children open the device themselves
        np.save(os.path.join(path, "cmp_old.npy"), np.array([cmp_old], np.uint64))
        print(f"library {N_OLD} files with coefficients ({n_old_groups} groups, {cmp_old} comparisons at {SIM}), {N_NEW} new files; similarity {SIM}, top {TOP}; "
              f"one process per build, 1 untimed + {TIMED} timed calls per leg; host clock, ms, min..max", flush=True)
        a = child("parent", parent_tree, path)
        b = child("tree", None, path)
    for t in (str(TOP), str(SIM)):
        assert a["tree"][t]["digest"] == b["tree"][t]["digest"] == b["plain_tree"][t]["digest"], f"the trees at {t} differ"
    assert b["swept"] == 0, "the library with edges swept"
    assert b["restored_state"] == b["plain_state"], "a library restored from its edges differs from the plain one"
    for kind, x in b["append"].items():
        assert x["state"] == a["append"]["state"], f"after the append the library ({kind}) differs from the parent's"
    for kind, x in b["remove"].items():
        assert x["state"] == a["remove"]["state"], f"after the removal the library ({kind}) differs from the parent's"
    print(f"trees at {TOP} and {SIM}: into, level and edges_at identical to the parent's sweep path, byte for byte, and no sweep ran; groups, labels_out / new_index, sizes and "
          f"counts after the append and after the removal identical for every kind of library and the parent's", flush=True)
    for t in (str(TOP), str(SIM)):
        new, old = b["tree"][t]["ms"], a["tree"][t]["ms"]
        line("(1)", f"rph_library_merge_tree({t}), library with edges (top {TOP}), this build", new)
        line("(1)", f"rph_library_merge_tree({t}), sweep path, parent build", old)
        line("(1)", f"rph_library_merge_tree({t}), sweep path on a plain library, this build", b["plain_tree"][t]["ms"])
        print(f"    bar: max new {max(new):.2f} < min parent {min(old):.2f}: {'MET' if max(new) < min(old) else 'NOT MET'}   (min / min = {min(old) / min(new):.1f} x)", flush=True)
    for kind, x in b["append"].items():
        line("(2)", f"rph_library_append of {N_NEW} onto the resident 1 M, {kind}, this build", x["ms"])
    line("(2)", f"rph_library_append of {N_NEW} onto the resident 1 M, plain, parent build", a["append"]["ms"])
    for kind, x in b["remove"].items():
        line("(3)", f"rph_library_remove of {N_REMOVE} from the resident 1 M, {kind}, this build", x["ms"])
    line("(3)", f"rph_library_remove of {N_REMOVE} from the resident 1 M, plain, parent build", a["remove"]["ms"])
    for kind, s in b["store"].items():
        print(f"(4) the store of the 1 M, {kind}: {s['edges']} edges, {s['bytes']} bytes; rph_library_edges of it {spread(s['download_ms'])}", flush=True)
    for kind, ms in b["fill"].items():
        line("(5)", f"first fill, rph_library_append of the 1 M into an empty library, {kind}, this build", ms)
    line("(5)", "first fill, rph_library_append of the 1 M into an empty library, plain, parent build", a["fill"])
    line("(5)", "rph_library_restore_edges of the 1 M and their edges at 63 (no sweep)", b["restore_edges"])


if __name__ == "__main__":
    main()
