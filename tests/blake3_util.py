"""BLAKE3 (32-byte output, `hash` and `keyed_hash` modes) restated from the published specification, vectorised with numpy
across chunks, as the reference the tests compare the library with.  Not a test module.

Two tree builders over the same chunk chaining values:
  blake3(...)        the pairwise fold: parents of neighbouring nodes level by level, an odd last node carried up a level
  blake3_stack(...)  the specification's incremental chaining-value stack (merge while the chunk count has trailing zero bits)
They must agree at every length: that is what makes the fold a statement of BLAKE3's left-full tree.
  blake3_many(...)   the pairwise fold over a list of messages at once, keyed or not (test_blake3_cpu.py holds it to blake3 at every length)

rgba16_bytes(image): the byte stream of the pixel hash (the `image` crate's to_rgba16() as little-endian bytes: u8 v -> u16 v * 257,
Luma8 copied into R, G and B, alpha 65535 unless the input has four channels).
"""
import numpy as np

IV = np.array([0x6A09E667, 0xBB67AE85, 0x3C6EF372, 0xA54FF53A, 0x510E527F, 0x9B05688C, 0x1F83D9AB, 0x5BE0CD19], np.uint32)
PERM = [2, 6, 3, 10, 7, 0, 4, 13, 1, 11, 12, 5, 9, 14, 15, 8]
CHUNK_START, CHUNK_END, PARENT, ROOT, KEYED_HASH = 1, 2, 4, 8, 16
CHUNK_LEN, BLOCK_LEN = 1024, 64


def _rotr(x, n):
    return (x >> np.uint32(n)) | (x << np.uint32(32 - n))


def _g(v, a, b, c, d, mx, my):
    v[a] = v[a] + v[b] + mx
    v[d] = _rotr(v[d] ^ v[a], 16)
    v[c] = v[c] + v[d]
    v[b] = _rotr(v[b] ^ v[c], 12)
    v[a] = v[a] + v[b] + my
    v[d] = _rotr(v[d] ^ v[a], 8)
    v[c] = v[c] + v[d]
    v[b] = _rotr(v[b] ^ v[c], 7)


def compress(cv, m, counter, block_len, flags):
    """cv: (8, N) uint32, m: (16, N) uint32, counter: (N,) uint64, block_len / flags: (N,) -> (8, N) chaining values."""
    n = cv.shape[1]
    with np.errstate(over="ignore"):
        counter = np.asarray(counter, np.uint64)
        v = [cv[i].copy() for i in range(8)] + [np.full(n, IV[i], np.uint32) for i in range(4)]
        v += [(counter & np.uint64(0xFFFFFFFF)).astype(np.uint32), (counter >> np.uint64(32)).astype(np.uint32),
              np.broadcast_to(np.asarray(block_len, np.uint32), (n,)).copy(), np.broadcast_to(np.asarray(flags, np.uint32), (n,)).copy()]
        m = [m[i] for i in range(16)]
        for r in range(7):
            _g(v, 0, 4, 8, 12, m[0], m[1])
            _g(v, 1, 5, 9, 13, m[2], m[3])
            _g(v, 2, 6, 10, 14, m[4], m[5])
            _g(v, 3, 7, 11, 15, m[6], m[7])
            _g(v, 0, 5, 10, 15, m[8], m[9])
            _g(v, 1, 6, 11, 12, m[10], m[11])
            _g(v, 2, 7, 8, 13, m[12], m[13])
            _g(v, 3, 4, 9, 14, m[14], m[15])
            if r < 6:
                m = [m[PERM[i]] for i in range(16)]
        return np.stack([v[i] ^ v[i + 8] for i in range(8)])


def _key_words(key):
    if key is None:
        return IV.copy(), 0
    key = bytes(key)
    assert len(key) == 32
    return np.frombuffer(key, "<u4").astype(np.uint32), KEYED_HASH


def chunk_cvs(data, key=None):
    """Chaining values of every chunk, (8, n_chunks); the ROOT flag is set on the last block when there is one chunk only."""
    data = np.frombuffer(bytes(data), np.uint8)
    kw, base = _key_words(key)
    n = len(data)
    nch = max(1, -(-n // CHUNK_LEN))
    buf = np.zeros(nch * CHUNK_LEN, np.uint8)
    buf[:n] = data
    words = buf.view("<u4").astype(np.uint32).reshape(nch, 16, 16)  # chunk, block, word
    clen = np.clip(n - np.arange(nch, dtype=np.int64) * CHUNK_LEN, 0, CHUNK_LEN)
    nblocks = np.maximum(1, -(-clen // BLOCK_LEN))
    cv = np.repeat(kw[:, None], nch, axis=1)
    counter = np.arange(nch, dtype=np.uint64)
    for b in range(16):
        act = b < nblocks
        if not act.any():
            break
        blen = np.clip(clen - b * BLOCK_LEN, 0, BLOCK_LEN)
        last = b + 1 == nblocks
        flags = base | np.where(b == 0, CHUNK_START, 0) | np.where(last, CHUNK_END, 0) | np.where(last & (nch == 1), ROOT, 0)
        new = compress(cv, words[:, b, :].T, counter, blen, flags)
        cv = np.where(act[None, :], new, cv)
    return cv, kw, base


def _digest(cv):
    return np.ascontiguousarray(cv.reshape(8)).astype("<u4").tobytes()


def blake3(data, key=None):
    """Pairwise fold of the chunk values, an odd last node carried up a level."""
    cv, kw, base = chunk_cvs(data, key)
    while cv.shape[1] > 1:
        cnt = cv.shape[1]
        npair = cnt // 2
        left, right = cv[:, 0:2 * npair:2], cv[:, 1:2 * npair:2]
        root = npair == 1 and cnt == 2
        m = np.concatenate([left, right], axis=0)
        par = compress(np.repeat(kw[:, None], npair, axis=1), m, np.zeros(npair, np.uint64), BLOCK_LEN, base | PARENT | (ROOT if root else 0))
        cv = np.concatenate([par, cv[:, 2 * npair:]], axis=1) if cnt % 2 else par
    return _digest(cv)


def blake3_many(datas, key=None):
    """[blake3(d, key) for d in datas] with the chunks and the tree levels of all messages in the same array operations: many
    short messages cost what one long message costs"""
    datas = [bytes(d) for d in datas]
    if not datas:
        return []
    kw, base = _key_words(key)
    nchs = np.array([max(1, -(-len(d) // CHUNK_LEN)) for d in datas], np.int64)
    offs = np.concatenate([[0], np.cumsum(nchs)])
    total = int(offs[-1])
    buf = np.zeros(total * CHUNK_LEN, np.uint8)
    for d, o in zip(datas, offs):
        buf[o * CHUNK_LEN:o * CHUNK_LEN + len(d)] = np.frombuffer(d, np.uint8)
    words = buf.view("<u4").astype(np.uint32).reshape(total, 16, 16)
    which = np.repeat(np.arange(len(datas)), nchs)
    counter = np.arange(total, dtype=np.int64) - offs[which]  # a chunk's number within its message
    clen = np.clip(np.array([len(d) for d in datas], np.int64)[which] - counter * CHUNK_LEN, 0, CHUNK_LEN)
    nblocks = np.maximum(1, -(-clen // BLOCK_LEN))
    single = nchs[which] == 1
    cv = np.repeat(kw[:, None], total, axis=1)
    for b in range(16):
        act = b < nblocks
        if not act.any():
            break
        last = b + 1 == nblocks
        flags = base | np.where(b == 0, CHUNK_START, 0) | np.where(last, CHUNK_END, 0) | np.where(last & single, ROOT, 0)
        new = compress(cv, words[:, b, :].T, counter.astype(np.uint64), np.clip(clen - b * BLOCK_LEN, 0, BLOCK_LEN), flags)
        cv = np.where(act[None, :], new, cv)
    nodes = [cv[:, offs[k]:offs[k + 1]] for k in range(len(datas))]
    while True:
        busy = [k for k, c in enumerate(nodes) if c.shape[1] > 1]
        if not busy:
            break
        pairs = [nodes[k].shape[1] // 2 for k in busy]
        left = np.concatenate([nodes[k][:, 0:2 * n:2] for k, n in zip(busy, pairs)], axis=1)
        right = np.concatenate([nodes[k][:, 1:2 * n:2] for k, n in zip(busy, pairs)], axis=1)
        flags = np.concatenate([np.full(n, base | PARENT | (ROOT if nodes[k].shape[1] == 2 else 0)) for k, n in zip(busy, pairs)])
        par = compress(np.repeat(kw[:, None], left.shape[1], axis=1), np.concatenate([left, right], axis=0), np.zeros(left.shape[1], np.uint64), BLOCK_LEN, flags)
        o = 0
        for k, n in zip(busy, pairs):
            nodes[k] = np.concatenate([par[:, o:o + n], nodes[k][:, 2 * n:]], axis=1)  # (an odd last node is carried up a level)
            o += n
    return [_digest(c) for c in nodes]


def blake3_stack(data, key=None):
    """The specification's incremental tree: a stack of subtree values, merged as the chunk count's trailing zero bits say."""
    cv, kw, base = chunk_cvs(data, key)
    nch = cv.shape[1]
    if nch == 1:
        return _digest(cv)

    def parent(l, r, flags):
        return compress(kw[:, None], np.concatenate([l, r])[:, None], np.zeros(1, np.uint64), BLOCK_LEN, base | PARENT | flags)[:, 0]

    stack = []
    for i in range(nch - 1):  # every chunk but the last: push, merging completed subtrees
        node = cv[:, i]
        total = i + 1
        while total & 1 == 0:
            node = parent(stack.pop(), node, 0)
            total >>= 1
        stack.append(node)
    node = cv[:, nch - 1]
    while stack:
        node = parent(stack.pop(), node, ROOT if not stack else 0)
    return _digest(node)


def test_input(n):
    """The published test vectors' input: byte i = i mod 251."""
    return (np.arange(n, dtype=np.int64) % 251).astype(np.uint8).tobytes()


def rgba16_bytes(image):
    """to_rgba16() of an (h, w) Luma8, (h, w, 3) Rgb8 or (h, w, 4) Rgba8 uint8 image as little-endian bytes."""
    a = np.asarray(image, np.uint8)
    if a.ndim == 2:
        a = a[:, :, None]
    h, w, c = a.shape
    out = np.full((h, w, 4), 65535, np.uint16)
    v = a.astype(np.uint16) * np.uint16(257)
    if c == 1:
        out[:, :, 0:3] = v
    elif c == 3:
        out[:, :, 0:3] = v
    else:
        out[:, :, :] = v
    return out.astype("<u2").tobytes()


def pixel_hash(image):
    return blake3(rgba16_bytes(image))
