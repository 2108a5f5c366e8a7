"""The rule of rph_group_max_dist (include/rupphash.h) restated in numpy, independent of the code under test: pivot rows from the CPU
oracle's dihedral hashes, distances by unpackbits, default pivots by a plain find_map.  Plus the inputs the CPU and the GPU tests share."""
import functools

import numpy as np

import library_corpus as lc

NO_PIVOT = 0xFFFFFFFF
INVALID_ARG = -1
SENTINEL = 0xA5A5A5A5


def default_pivot(members, dih, has_features):
    """find_map (scanner.rs:2219-2232): the first listed member that has features, else the first listed member, else none"""
    if not len(members):
        return None
    if dih is not None:
        for m in members:
            if has_features is None or has_features[m]:
                return m
    return members[0]


def restate(groups, hashes, pivots=None, dih=None, has_features=None):
    """(max_dist per group, member_dist per group as lists).  dih: (n, 8, 32) from oracle.dihedral_hashes of every file's coefficients, or
    None for a call without coefficients; pivots: a file number or None per group, or None for the default pivots."""
    hashes = np.asarray(hashes, np.uint8).reshape(-1, 32)
    bits = np.unpackbits(hashes, axis=1).astype(np.int16)
    max_dist, member_dist = [], []
    for g, members in enumerate(groups):
        members = [int(m) for m in members]
        p = pivots[g] if pivots is not None else default_pivot(members, dih, has_features)
        if p is None or not members:
            max_dist.append(0)
            member_dist.append([0] * len(members))
            continue
        featured = dih is not None and (has_features is None or has_features[p])
        rows = np.unpackbits(np.asarray(dih[p], np.uint8), axis=1).astype(np.int16) if featured else bits[p][None, :]
        d = np.abs(bits[members][:, None, :] - rows[None, :, :]).sum(axis=2).min(axis=1)
        max_dist.append(int(d.max()))
        member_dist.append([int(x) for x in d])
    return max_dist, member_dist


def plain_distances(hashes):
    """(n, n) Hamming distances"""
    b = np.unpackbits(np.asarray(hashes, np.uint8).reshape(-1, 32), axis=1).astype(np.float32)
    return (b @ (1 - b).T + (1 - b) @ b.T).astype(np.int32)


@functools.lru_cache(maxsize=None)
def corpus_groups(sim=40):
    """the groups library_corpus' Python union-find yields on the corpus' plain distances <= sim, as index lists"""
    f = lc.corpus()
    i, j = np.nonzero(np.triu(plain_distances(f.hashes) <= sim, 1))
    return lc.groups_of(lc.min_labels(lc.N_FILES, np.stack([i, j], axis=1)))


def explicit_pivots(groups, n, seed=5):
    """one pivot per group: mostly a member (not the first where there is another), every fifth a file outside the group, every
    eleventh (and an empty group) none"""
    rng = np.random.default_rng(seed)
    out = []
    for g, members in enumerate(groups):
        if g % 11 == 10 or not len(members):
            out.append(None)
        elif g % 5 == 4:
            out.append(int(rng.choice(np.setdiff1d(np.arange(n), members))))
        else:
            out.append(int(members[-1]))
    return out


def flip(h, bit_list):
    v = np.array(h, np.uint8).copy()
    for b in bit_list:
        v[b // 8] ^= 1 << (b % 8)
    return v


def variant_family(oracle, seed=8):
    """File 0 with coefficients; files 1 .. 8: dihedral variant v = 0 .. 7 of file 0 with k = v + 1 bits flipped; files 9 .. 11 unrelated.
    Returns (coeffs, hashes, dih, groups, want): group v = [0, 1 + v] must give k, the last group (all nine) 8."""
    rng = np.random.default_rng(seed)
    n = 12
    coeffs = rng.normal(0, 30, (n, 256)).astype(np.float32)
    hashes = np.stack([oracle.to_hash(c) for c in coeffs])
    dih = np.stack([oracle.dihedral_hashes(c) for c in coeffs])
    for v in range(8):
        hashes[1 + v] = flip(dih[0][v], rng.choice(256, v + 1, replace=False))
    groups = [[0, 1 + v] for v in range(8)] + [list(range(9))]
    return coeffs, hashes, dih, groups, [v + 1 for v in range(8)] + [8]


def error_cases(n):
    """(name, members, offsets, pivots) of every refusal of the rule over n files; each keeps len(members) == offsets[-1]"""
    u = lambda *x: np.array(x, np.uint32)  # noqa: E731
    return [
        ("offsets-start-at-1", u(0, 1, 2, 3), u(1, 2, 4), u(0, 2)),
        ("offsets-descend", u(0, 1, 2, 3), u(0, 3, 2, 4), u(0, 1, 2)),
        ("member-is-n", u(0, n, 2, 3), u(0, 2, 4), u(0, 2)),
        ("member-is-no-pivot", u(0, 1, 2, NO_PIVOT), u(0, 2, 4), None),
        ("pivot-is-n", u(0, 1, 2, 3), u(0, 2, 4), u(0, n)),
        ("pivot-far-outside", u(0, 1, 2, 3), u(0, 2, 4), u(0xFFFFFFFE, 2)),
    ]
