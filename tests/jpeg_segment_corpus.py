"""The corpus of the segment synchroniser's tests: small one-scan baseline files without restart markers, every one at most 160 px a side
(so every block carries weight in the 256 PDQ coefficients), built with jpeg_util's coefficient encoder -- which controls the length of
every symbol -- and a few with Pillow.  The files were found by search with the model (jpeg_segments.py): candidates of the generators
below over their seeds and sizes, kept where the model reports a wanted property.  What is kept is the list of generator arguments; the
properties are recomputed from the files here (classes_of) and pinned by test_jpeg_segments_cpu.py."""
import functools

import numpy as np

import jpeg_segments as js
import jpeg_util as ju

SEG_SIZES = (64, 68, 256, 1024)  # the minimum; a multiple of 4 that is no power of two; 256; 1024 (on a subset)

GRAY = ((1, 1),)
S444 = ((1, 1), (1, 1), (1, 1))
S422 = ((2, 1), (1, 1), (1, 1))
S440 = ((1, 2), (1, 1), (1, 1))
S420 = ((2, 2), (1, 1), (1, 1))
S222 = ((2, 1), (2, 1), (2, 1))  # chroma at luma's sampling.  (2x2 / 2x1 / 2x1, 8 blocks per MCU, is a frame the library refuses as
# unsupported: its chroma is either 1x1 or sampled like luma.  Refused files are not this corpus's.)
LAYOUTS = {"gray": GRAY, "444": S444, "422": S422, "440": S440, "420": S420, "2x1_2x1_2x1": S222}

ONES = np.ones(64, np.int64)
ANNEX_K_TABLES = {(tuple(t[0]), tuple(t[1])) for t in (ju.DC_L, ju.DC_C, ju.AC_L, ju.AC_C, ju.DC_L_WIDE)}


def _grid_blocks(w, h, sampling):
    _, _, mx, my = ju.grid(w, h, sampling)
    return [np.zeros((my * V, mx * H, 64), np.int64) for H, V in sampling]


def _encode(blocks, w, h, sampling, tables):
    gray = len(sampling) == 1
    return ju.encode_baseline_coefficients(blocks, [ONES, ONES], w, h, sampling=sampling, gray=gray, tables=tables, mcu_positions=True)


def mixed(seed, w, h, layout, tables, p_flat=0.3, p_dense=0.3, cats=(1, 2, 3, 4), dc_step=40):
    """blocks of three kinds by chance: flat (the DC of the block before, no AC: an MCU of a few bits), sparse (a few values behind runs of
    zeros) and dense (every coefficient, values of the categories `cats`); DC values walk in steps of up to dc_step"""
    rng = np.random.default_rng(seed)
    sampling = LAYOUTS[layout]
    blocks = _grid_blocks(w, h, sampling)
    for b in blocks:
        flat = b.reshape(-1, 64)
        dc = 0
        for k in range(len(flat)):
            u = rng.random()
            if u >= p_flat:
                dc += int(rng.integers(-dc_step, dc_step + 1))
                n = 63 if u < p_flat + p_dense else int(rng.integers(1, 8))
                where = 1 + rng.choice(63, n, replace=False)
                cat = rng.choice(cats, n)
                mag = [int(rng.integers(1 << (c - 1), 1 << c)) for c in cat]
                flat[k, where] = [m if rng.random() < 0.5 else -m for m in mag]
            flat[k, 0] = dc
    return _encode(blocks, w, h, sampling, tables)


def flat(w, h, layout, tables="annex_k", value=5):
    """every block the same DC and nothing else: after the first, an MCU is its shortest (gray, Annex K: 6 bits)"""
    sampling = LAYOUTS[layout]
    blocks = _grid_blocks(w, h, sampling)
    for b in blocks:
        b[..., 0] = value
    return _encode(blocks, w, h, sampling, tables)


def long_mcu(n_values, w=160, h=16, where=1, bits=15, seed=0, layout="420", tables="used"):
    """one MCU (number `where`) of dense blocks -- n_values coefficients of `bits` bits, spread over its blocks from the first on -- among
    MCUs of a few sparse values: the long MCU covers whole segments in which no MCU begins"""
    rng = np.random.default_rng(seed)
    sampling = LAYOUTS[layout]
    hmax, vmax, mx, my = ju.grid(w, h, sampling)
    blocks = _grid_blocks(w, h, sampling)
    for ci, b in enumerate(blocks):
        flat_ = b.reshape(-1, 64)
        for k in range(len(flat_)):
            n = int(rng.integers(1, 6))
            flat_[k, 1 + rng.choice(63, n, replace=False)] = rng.integers(-7, 8, n)
            flat_[k, 0] = int(rng.integers(-30, 31))
    left = n_values
    my_, mx_ = divmod(where, mx)
    for ci, (H, V) in enumerate(sampling):
        for v in range(V):
            for hh in range(H):
                n = min(left, 63)
                left -= n
                blk = blocks[ci][my_ * V + v, mx_ * H + hh]
                blk[1:] = 0
                mag = rng.integers(1 << (bits - 1), 1 << bits, n)
                blk[ju.ZIGZAG[1:1 + n]] = np.where(rng.random(n) < 0.5, mag, -mag)
    assert left == 0, "more values than the MCU has coefficients"
    return _encode(blocks, w, h, sampling, tables)


def big_dc(seed, w, h, layout="444", n_ac=3):
    """DC values of both signs far apart (differences of up to 15 bits, sums that leave int16 both ways), a few AC values"""
    rng = np.random.default_rng(seed)
    sampling = LAYOUTS[layout]
    blocks = _grid_blocks(w, h, sampling)
    for b in blocks:
        flat_ = b.reshape(-1, 64)
        for k in range(len(flat_)):
            flat_[k, 0] = int(rng.integers(-70000, 70001))
            flat_[k, 1 + rng.choice(63, n_ac, replace=False)] = rng.integers(-100, 101, n_ac)
    return _encode(blocks, w, h, sampling, tables="used")


def ones(seed, w, h, layout, tables, wide_dc=False):
    """values whose bits are all ones (2^s - 1) at every category the tables can code, dense: runs of one bits for a decode that starts at
    a boundary to break off in.  wide_dc: the file's Annex K luma DC table is replaced by one that also codes the categories 12..16 (the
    codes of 0..11 stay what they were), so that thirteen one bits and a zero where a DC code is expected read as category 16"""
    rng = np.random.default_rng(seed)
    sampling = LAYOUTS[layout]
    top = 10 if tables == "annex_k" else 15
    blocks = _grid_blocks(w, h, sampling)
    for b in blocks:
        flat_ = b.reshape(-1, 64)
        dc = 0
        for k in range(len(flat_)):
            dc += int(rng.integers(-3, 4))
            flat_[k, 0] = dc
            n = int(rng.integers(8, 40))
            s = rng.integers(top - 3, top + 1, n)
            flat_[k, ju.ZIGZAG[1:1 + n]] = (1 << s) - 1
    data, expected, positions = _encode(blocks, w, h, sampling, tables)
    if wide_dc:
        old = bytes([0x00]) + bytes(ju.DC_L[0]) + bytes(ju.DC_L[1])
        new = bytes([0x00]) + bytes(ju.DC_L_WIDE[0]) + bytes(ju.DC_L_WIDE[1])
        at = data.index(b"\xff\xc4" + (len(old) + 2).to_bytes(2, "big") + old)
        data = data[:at] + b"\xff\xc4" + (len(new) + 2).to_bytes(2, "big") + new + data[at + 4 + len(old):]
    return data, expected, positions


def pillow(seed, w, h, mode, quality, subsampling=0):
    kw = dict(quality=quality)
    if mode == "RGB":
        kw["subsampling"] = subsampling
    return ju.pillow_jpeg(ju.make_image(w, h, mode, seed=seed), **kw), None, None


def units(seed, w, h, p_unit=0.7, max_n=63):
    """gray, tables "used" with the DC categories {0, 2} and the AC symbols {EOB, 0/4}: every code has 2 bits, and a coefficient of -15
    (code 01, bits 0000) reads, where a decode expects an MCU, as a whole MCU of 6 bits (DC category 2: code 01, bits 00; EOB: 00).  A
    decode that starts inside a block of such values records an MCU start every 6 bits and never falls into step before the block ends"""
    rng = np.random.default_rng(seed)
    blocks = _grid_blocks(w, h, GRAY)
    flat_ = blocks[0].reshape(-1, 64)
    dc = 0
    for k in range(len(flat_)):
        dc += int(rng.choice([0, 0, 2, 3, -2, -3]))
        flat_[k, 0] = dc
        n = int(rng.integers(0, max_n + 1))
        v = np.where(rng.random(n) < p_unit, -15, rng.integers(8, 16, n) * rng.choice([-1, 1], n))
        flat_[k, ju.ZIGZAG[1:1 + n]] = v
    flat_[0, 0], flat_[1, 0] = 2, 2  # (both DC categories occur)
    flat_[0, 1] = -15
    return _encode(blocks, w, h, GRAY, "used")


GENERATORS = {"units": units, "mixed": mixed, "flat": flat, "long_mcu": long_mcu, "big_dc": big_dc, "ones": ones, "pillow": pillow}


# ---- what a file is a witness of, at one segment size (from the model alone) ----------------------------------------------------------

def classes_of(F, seg_bytes, result=None):
    """the set of class names the file belongs to at this segment size; `result` = js.protocol(F, seg_bytes)"""
    R = result or js.protocol(F, seg_bytes)
    chain, settles = js.true_chain(F, seg_bytes)
    starts, sums, dc_ranges = js.mcu_starts(F)
    seg_bits = seg_bytes * 8
    n = len(chain)
    out = {"verifies" if R["verified"] else "falls_back"}
    if not settles:
        out.add("last_mcu_shorter_than_a_byte")  # (the exit rule cuts it off: the counts cannot reach total_mcus)
    inner = [p for p in starts[1:-1]]
    if any(p % seg_bits == 0 for p in inner):
        out.add("start_at_boundary")
    if any(p % seg_bits == seg_bits - 1 and p // seg_bits < n - 1 for p in inner):
        out.add("start_at_hi_minus_1")
    if any(p % seg_bits == 1 for p in inner):
        out.add("start_at_hi_plus_1")
    for t, ev in enumerate(R["events"] if R["verified"] else []):  # (what the rounds did at true entries, where the device's log can confirm it)
        for e in ev:
            if e == "pass_on":
                continue
            if isinstance(e, tuple):
                kind, k = e
                if kind == "recorded":
                    out.add("entry_is_the_boundary" if k == 0 else "entry_is_the_16th_start" if k == 15 else "entry_is_a_recorded_start")
                else:
                    out.add("step_in")
                    if k == 1:
                        out.add("step_in_at_the_2nd")
                    if k == 15:
                        out.add("step_in_at_the_16th")
            else:
                out.add({"to_the_end": "decode_to_the_end", "behind_the_16th": "entry_behind_the_16th"}[e])
    if any(s["round0_n"] == js.SEG_MARKS for s in R["segs"]):
        out.add("table_full")
    run = 0
    for t, c in enumerate(chain):  # segments in which no MCU begins, behind one that begins before them
        passes = c["entry"] >= (t + 1) * seg_bits
        run = run + 1 if passes else 0
        if run == 1:
            out.add("pass_on")
        if run == 2:
            out.add("pass_on_several")
    annex_k = F.distinct_tables <= ANNEX_K_TABLES
    for why, name in (("code", "round0_no_code_annex_k" if annex_k else "round0_no_code_other_tables"), ("size", "round0_size_above_15")):
        if why in R["round0"] and R["verified"]:
            out.add(name)
    pad = F.end_bits - starts[-1]
    if pad in (0, 1, 7):
        out.add(f"padding_{pad}")
    if len(F.stream) % seg_bytes == 0:
        out.add("length_multiple_of_segment")
    if len(F.stream) % seg_bytes == 4:
        out.add("last_segment_4_bytes")
    if n == 1:
        out.add("one_segment")
    if n > 1 and chain[-1]["count"] == 0:
        out.add("last_segment_without_mcu")
    if n > 1 and pad and chain[-1]["entry"] == starts[-1] and starts[-2] < (n - 1) * seg_bits:
        out.add("last_mcu_straddles_padding")
        if js.protocol(F, seg_bytes, fixed=False)["verified"] != R["verified"]:
            out.add("padding_decoded_before_the_fix")
    if F.ns == 3 and min(min(s) for s in sums) < 0 and max(max(s) for s in sums) > 32767:
        out.add("dc_sums_beyond_int16")
        if any(a < t * seg_bits < b for a, b in dc_ranges for t in range(a // seg_bits, b // seg_bits + 1)):
            out.add("boundary_in_dc_bits")
    if F.ns == 1 and F.w % 8:
        out.add("gray_odd_width")
    if R["stable_after"] is not None:
        out.add(f"stable_after_{R['stable_after']}")
    return out


def longest_span(F, seg_bytes):
    """segments the file's longest MCU touches"""
    starts = js.mcu_starts(F)[0]
    seg_bits = seg_bytes * 8
    return max((b - 1) // seg_bits - a // seg_bits + 1 for a, b in zip(starts, starts[1:]))


def layout_of(F):
    return {s: name for name, s in LAYOUTS.items()}[tuple((c[1], c[2]) for c in F.comps)]


# ---- the files: generator and arguments, as the search left them (the ladder first: one MCU that touches 3, 4, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10
# segments of 64 bytes, beginning in segment 0) -------------------------------------------------------------------------------------------
CORPUS = [
    ("long_mcu", {"n_values": 20, "bits": 10, "tables": "annex_k"}),
    ("long_mcu", {"n_values": 40, "bits": 10, "tables": "annex_k"}),
    ("long_mcu", {"n_values": 89, "bits": 10, "tables": "annex_k"}),
    ("long_mcu", {"n_values": 92, "bits": 10, "tables": "annex_k"}),
    ("long_mcu", {"n_values": 107, "bits": 10, "tables": "annex_k"}),
    ("long_mcu", {"n_values": 110, "bits": 10, "tables": "annex_k"}),
    ("long_mcu", {"n_values": 131, "bits": 10, "tables": "annex_k"}),
    ("long_mcu", {"n_values": 134, "bits": 10, "tables": "annex_k"}),
    ("long_mcu", {"n_values": 143, "bits": 10, "tables": "annex_k"}),
    ("long_mcu", {"n_values": 146, "bits": 10, "tables": "annex_k"}),
    ("long_mcu", {"n_values": 161, "bits": 10, "tables": "annex_k"}),
    ("long_mcu", {"n_values": 164, "bits": 10, "tables": "annex_k"}),
    ("mixed", {"seed": 501, "w": 160, "h": 160, "layout": "420", "tables": "annex_k", "p_flat": 0.2, "p_dense": 0.5}),
    ("mixed", {"seed": 503, "w": 152, "h": 160, "layout": "gray", "tables": "annex_k", "p_flat": 0.2, "p_dense": 0.5}),
    ("pillow", {"seed": 300, "w": 120, "h": 80, "mode": "RGB", "quality": 90, "subsampling": 2}),
    ("pillow", {"seed": 301, "w": 97, "h": 61, "mode": "L", "quality": 75, "subsampling": 0}),
    ("pillow", {"seed": 302, "w": 160, "h": 120, "mode": "RGB", "quality": 75, "subsampling": 0}),
    ("pillow", {"seed": 303, "w": 33, "h": 160, "mode": "RGB", "quality": 50, "subsampling": 1}),
    ("pillow", {"seed": 304, "w": 16, "h": 16, "mode": "RGB", "quality": 85, "subsampling": 2}),
    ("pillow", {"seed": 305, "w": 8, "h": 8, "mode": "L", "quality": 90, "subsampling": 0}),
    ("pillow", {"seed": 312, "w": 160, "h": 152, "mode": "L", "quality": 95}),
    ("mixed", {"seed": 108, "w": 14, "h": 92, "layout": "gray", "tables": "annex_k"}),
    ("mixed", {"seed": 24, "w": 26, "h": 80, "layout": "gray", "tables": "annex_k"}),
    ("mixed", {"seed": 84, "w": 146, "h": 20, "layout": "gray", "tables": "annex_k"}),
    ("flat", {"w": 160, "h": 160, "layout": "gray"}),
    ("units", {"seed": 122, "w": 53, "h": 32, "p_unit": 1.0}),
    ("mixed", {"seed": 38, "w": 124, "h": 22, "layout": "444", "tables": "annex_k"}),
    ("units", {"seed": 110, "w": 29, "h": 16, "p_unit": 1.0}),
    ("units", {"seed": 121, "w": 45, "h": 24, "p_unit": 1.0}),
    ("units", {"seed": 106, "w": 69, "h": 24, "p_unit": 1.0}),
    ("flat", {"w": 13, "h": 9, "layout": "gray"}),
    ("units", {"seed": 14, "w": 64, "h": 48}),
    ("mixed", {"seed": 68, "w": 34, "h": 52, "layout": "420", "tables": "annex_k"}),
    ("big_dc", {"seed": 0, "w": 24, "h": 16, "layout": "444"}),
    ("units", {"seed": 2, "w": 40, "h": 32}),
    ("mixed", {"seed": 112, "w": 42, "h": 24, "layout": "422", "tables": "annex_k"}),
    ("big_dc", {"seed": 1, "w": 32, "h": 24, "layout": "420"}),
    ("big_dc", {"seed": 5, "w": 64, "h": 24, "layout": "422"}),
    ("ones", {"seed": 24, "w": 16, "h": 16, "layout": "gray", "tables": "annex_k", "wide_dc": True}),
    ("ones", {"seed": 27, "w": 40, "h": 16, "layout": "gray", "tables": "annex_k", "wide_dc": True}),
    ("ones", {"seed": 21, "w": 40, "h": 16, "layout": "gray", "tables": "annex_k", "wide_dc": True}),
    ("mixed", {"seed": 22, "w": 12, "h": 54, "layout": "2x1_2x1_2x1", "tables": "annex_k"}),
    ("mixed", {"seed": 47, "w": 37, "h": 19, "layout": "2x1_2x1_2x1", "tables": "used"}),
    ("mixed", {"seed": 10, "w": 78, "h": 18, "layout": "2x1_2x1_2x1", "tables": "annex_k"}),
    ("mixed", {"seed": 66, "w": 20, "h": 26, "layout": "440", "tables": "annex_k"}),
    ("mixed", {"seed": 67, "w": 27, "h": 39, "layout": "440", "tables": "used"}),
    ("mixed", {"seed": 102, "w": 122, "h": 14, "layout": "440", "tables": "annex_k"}),
    ("units", {"seed": 1102, "w": 47, "h": 32, "p_unit": 1.0}),
    ("units", {"seed": 1239, "w": 24, "h": 40, "p_unit": 1.0}),
    ("units", {"seed": 1359, "w": 32, "h": 40, "p_unit": 1.0}),
]


def name_of(k):
    gen, kw = CORPUS[k]
    return gen + "(" + ", ".join(f"{a}={v}" for a, v in kw.items()) + ")"


@functools.lru_cache(maxsize=None)
def files():
    """per corpus file dict(name, data, expected: the coefficients its encoder aimed at (None: Pillow's), positions: where the encoder
    wrote its MCUs (None: Pillow's), F: the parsed file)"""
    out = []
    for k, (gen, kw) in enumerate(CORPUS):
        data, expected, positions = GENERATORS[gen](**kw)
        out.append(dict(name=name_of(k), data=data, expected=expected, positions=positions and positions[0], F=js.parse(data)))
    return out


@functools.lru_cache(maxsize=None)
def model(seg_bytes):
    """per corpus file (layer A's chain, whether its counts reach total_mcus, layer B's result) at one segment size, computed once"""
    return [js.true_chain(f["F"], seg_bytes) + (js.protocol(f["F"], seg_bytes),) for f in files()]


@functools.lru_cache(maxsize=None)
def classes(seg_bytes):
    return [classes_of(f["F"], seg_bytes, m[2]) | {"layout_" + layout_of(f["F"])} for f, m in zip(files(), model(seg_bytes))]


def annex_k_only():
    """indices of the files whose Huffman tables are T.81 K.3's (and the widened luma DC table): a call of these has at most 8 tables"""
    return [k for k, f in enumerate(files()) if f["F"].distinct_tables <= ANNEX_K_TABLES]


LARGE = 1024  # the subset that runs at 1024-byte segments: streams longer than one such segment


def subset_1024():
    return [k for k, f in enumerate(files()) if len(f["F"].stream) > LARGE]
