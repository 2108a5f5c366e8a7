"""What rph_library_remove is tested on (test_library_remove_cpu.py pins the expectations without a GPU; test_library_remove_gpu.py runs
them): a numpy model of removal on an edge list, the closed forms of the dense and the blocks-of-four libraries, and a mirror of a
library's files on the host.  Everything is seeded and needs numpy only."""
import numpy as np

import library_corpus as lc

GONE = 0xFFFFFFFF


def new_index(n, removed):
    """old file number -> new file number (GONE for a removed file): the survivors keep their order and are numbered densely"""
    keep = np.ones(n, bool)
    keep[np.asarray(removed, np.int64)] = False
    return np.where(keep, np.cumsum(keep) - 1, GONE).astype(np.uint32)


def remove_from_edges(n, edges, removed):
    """The model: drop the edges that touch a removed file, renumber the rest, min-label union-find over the survivors.
    edges: (m, 2) with i < j, as often as the sweep reports them.  Returns (new_index, kept edges, dropped, labels, groups)."""
    edges = np.asarray(edges, np.uint32).reshape(-1, 2)
    new = new_index(n, removed)
    gone = (new[edges] == GONE).any(axis=1)
    kept = new[edges[~gone]]
    assert (kept[:, 0] < kept[:, 1]).all()  # order survives the renumbering
    labels = lc.min_labels(n - len(removed), kept)
    return new, kept, int(gone.sum()), labels, lc.groups_of(labels)


# ---------------------------------------------------------------- dense sets
def dense_minus_one(c, rows=1):
    """c identical files, one removed: (comparisons dropped, comparisons kept)"""
    return rows * (c - 1), rows * (c - 1) * (c - 2) // 2


# ---------------------------------------------------------------- blocks of four
BLOCK_SIM = 10
_MEMBER_BITS = ((), (0, 1), (2, 3), (4, 5))  # member k of a block differs from its base in these bits: 2 or 4 bits between members


def block_hashes(n, seed):
    """n files in blocks of four (the last one ragged): a random base hash per block, members a few bits away.  Two bases are about 128
    bits apart, so at BLOCK_SIM the edges are exactly the pairs inside a block."""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, ((n + 3) // 4, 32), dtype=np.uint8)
    hashes = np.repeat(base, 4, axis=0)[:n].copy()
    member = np.arange(n) % 4
    for k, bits in enumerate(_MEMBER_BITS):
        for b in bits:
            hashes[member == k, b // 8] ^= np.uint8(1 << (b % 8))
    return hashes


def block_state(alive):
    """Closed form of a blocks-of-four library of which the files with alive[x] are left (numbered densely): every pair inside a block is an
    edge, so a block stays one component whatever it loses.  (labels, (members, offsets), comparisons), the groups as restore takes them."""
    alive = np.asarray(alive, bool)
    block = np.nonzero(alive)[0] // 4
    n = len(block)
    ids = np.arange(n, dtype=np.uint32)
    first = np.ones(n, bool)
    first[1:] = block[1:] != block[:-1]
    labels = np.maximum.accumulate(np.where(first, ids, 0)).astype(np.uint32)
    size = np.diff(np.append(np.nonzero(first)[0], n))
    in_group = np.repeat(size > 1, size)
    offsets = np.concatenate([[0], np.cumsum(size[size > 1])]).astype(np.uint32)
    return labels, (ids[in_group], offsets), int((size * (size - 1) // 2).sum())


def groups_as_lists(groups):
    members, offsets = groups
    return [members[a:b].tolist() for a, b in zip(offsets[:-1], offsets[1:])]


def grid_removals(n):
    """every file with x % 1000 == 1, the first and the last"""
    return np.unique(np.concatenate([np.arange(1, n, 1000), [0, n - 1]])).astype(np.uint32)


# ---------------------------------------------------------------- a library's files on the host
class Mirror:
    """Which corpus files a library holds, in order, and with which has_features (0 for files appended without coefficients)"""

    def __init__(self, files):
        self.f = files
        self.ids = np.zeros(0, np.int64)
        self.hf = np.zeros(0, np.uint8)

    def __len__(self):
        return len(self.ids)

    def appended(self, ids, with_coeffs=True):
        """the arguments of Library.append for these corpus files; they are recorded as appended"""
        ids = np.asarray(ids, np.int64)
        self.ids = np.concatenate([self.ids, ids])
        self.hf = np.concatenate([self.hf, self.f.has_features[ids] if with_coeffs else np.zeros(len(ids), np.uint8)])
        kw = dict(quality=self.f.quality[ids])
        if with_coeffs:
            kw.update(coeffs=self.f.coeffs[ids], has_features=self.f.has_features[ids])
        return self.f.hashes[ids], kw

    def removed(self, indices):
        keep = new_index(len(self), indices) != GONE
        self.ids, self.hf = self.ids[keep], self.hf[keep]

    @property
    def hashes(self):
        return self.f.hashes[self.ids]

    @property
    def coeffs(self):
        return self.f.coeffs[self.ids]

    @property
    def quality(self):
        return self.f.quality[self.ids]

    @property
    def rows(self):
        """the eight rows of every file as the library holds them"""
        return np.where(self.hf[:, None, None] != 0, self.f.dih[self.ids], self.f.hashes[self.ids][:, None, :])
