"""A model of the JPEG segment synchroniser (rupphash_amd/csrc/jpeg_device.h, jpeg_sync_kernel and jpeg_seg_items_kernel), in plain Python
and numpy, for one-scan baseline files without restart markers.  Two layers that share only the Huffman symbol reader:

(A) the TRUE CHAIN.  A sequential parse from bit 0 gives every MCU start and the DC differences; from those alone the chain a verified
    file must end with follows: entry[0] = 0; a segment [lo, hi) whose entry lies at or behind hi, or less than 8 bits before the end of
    the scan (the padding), passes it on with count 0; otherwise its `out` is the first MCU boundary behind the entry with pos >= hi or
    pos + 8 > end_bits, and entry[t + 1] = out[t].  The walk items follow from the chain.

(B) the PROTOCOL.  Round 0 from every boundary with the kernel's break-off rules, the record of up to 16 MCU starts, 8 double-buffered
    validation rounds with their three outcomes, the count pass and the prefix check -- a restatement of what the kernels do, buffer by
    buffer.  Its verdict (does the file's chain verify?) is what the device must agree with; it also says what happened on the way.

Everything works on the file's own headers and de-stuffed entropy bytes, never on an encoder's internals.  Behind the scan the device reads
zeros (prepare_stream leaves 32 zero bytes and the lanes' loads are clamped inside them): so does the model."""
import numpy as np

NONE = 0xFFFFFFFF
SEG_MARKS = 16
ROUNDS = 8

_lut_cache = {}


def _lut(counts, symbols):
    """65536 entries, (length << 8) | symbol of the code that begins a 16-bit window, 0 where none does"""
    key = (tuple(counts), tuple(symbols))
    if key not in _lut_cache:
        lut = np.zeros(65536, np.uint32)
        code, k = 0, 0
        for length in range(1, 17):
            for _ in range(counts[length - 1]):
                lut[code << (16 - length):(code + 1) << (16 - length)] = (length << 8) | symbols[k]
                code += 1
                k += 1
            code <<= 1
        _lut_cache[key] = lut.tolist()
    return _lut_cache[key]


class Scan:
    """a parsed file: frame, tables, de-stuffed entropy bytes"""


def parse(data):
    """headers and tables of a one-scan baseline file, its entropy bytes with the stuffing undone"""
    F = Scan()
    dht = {}
    pos = 2
    assert data[:2] == b"\xff\xd8"
    while True:
        assert data[pos] == 0xFF
        m = data[pos + 1]
        n = int.from_bytes(data[pos + 2:pos + 4], "big")
        p = data[pos + 4:pos + 2 + n]
        pos += 2 + n
        if m == 0xC0 or m == 0xC1:
            F.h, F.w = int.from_bytes(p[1:3], "big"), int.from_bytes(p[3:5], "big")
            F.comps = [(p[6 + 3 * i], p[7 + 3 * i] >> 4, p[7 + 3 * i] & 15) for i in range(p[5])]
        elif m == 0xC4:
            while p:
                counts = list(p[1:17])
                total = sum(counts)
                dht[p[0] >> 4, p[0] & 15] = (counts, list(p[17:17 + total]))
                p = p[17 + total:]
        elif m == 0xDD:
            assert int.from_bytes(p[:2], "big") == 0, "restart intervals are not this model's"
        elif m == 0xDA:
            ns = p[0]
            sel = [(p[1 + 2 * i], p[2 + 2 * i] >> 4, p[2 + 2 * i] & 15) for i in range(ns)]
            break
    assert ns == len(F.comps), "one scan with every component"
    end = data.index(b"\xff\xd9", pos)
    body = data[pos:end]
    assert not any(body[i] == 0xFF and body[i + 1] != 0 for i in range(len(body) - 1)), "no markers inside the scan"
    F.stream = body.replace(b"\xff\x00", b"\xff")
    F.end_bits = 8 * len(F.stream)
    F.ns = ns
    ids = [c[0] for c in F.comps]
    F.ci = [ids.index(s[0]) for s in sel]
    hmax, vmax = max(c[1] for c in F.comps), max(c[2] for c in F.comps)
    if ns == 1:  # a scan of one component walks its real blocks, one per MCU
        F.nblk = [1]
        F.total_mcus = -(-F.w // 8) * -(-F.h // 8)
    else:
        F.nblk = [F.comps[c][1] * F.comps[c][2] for c in F.ci]
        F.total_mcus = -(-F.w // (8 * hmax)) * -(-F.h // (8 * vmax))
    F.tables = [(dht[0, s[1]], dht[1, s[2]]) for s in sel]
    F.dc = [_lut(*dht[0, s[1]]) for s in sel]
    F.ac = [_lut(*dht[1, s[2]]) for s in sel]
    F.distinct_tables = {(tuple(t[0]), tuple(t[1])) for pair in F.tables for t in pair}
    # win[p]: the 32 bits from bit p on, zeros behind the scan
    b = np.frombuffer(F.stream + bytes(8), np.uint8).astype(np.uint64)
    w40 = (b[:-4] << 32) | (b[1:-3] << 24) | (b[2:-2] << 16) | (b[3:-1] << 8) | b[4:]
    p = np.arange(F.end_bits + 8, dtype=np.uint64)
    F.win = ((w40[(p >> 3).astype(np.int64)] >> (8 - (p & 7))) & 0xFFFFFFFF).tolist()
    return F


def _extend(raw, s):
    return raw - ((1 << s) - 1) if raw < (1 << (s - 1)) else raw


def decode(F, start, hi, mode, lo=0, marks=None, seg_bits=None, strict=False, limit_mcus=None, trace=None):
    """jpeg_sync_kernel's loop: MCU after MCU from bit `start` until one begins at or behind `hi` or less than 8 bits before the end.
    mode 0 records the MCU starts (offsets from lo) with the DC sums at each; mode 1 stops at the first of `marks` an MCU begins at;
    mode 2 breaks off at a run past coefficient 63.  Returns dict(out, count, dc, why, hit, pos: the bit it stopped at[, starts, sum: mode 0's
    record]); out = NONE when it broke off (why: "code" no code of <= 16 bits, "size" a DC category above 15, "run" mode 2's, "iterations" the bound).
    strict / limit_mcus / trace serve layer A: a sequential parse that must not break off, of a known number of MCUs."""
    win, nwin, end_bits, ns = F.win, len(F.win), F.end_bits, F.ns
    pos, i, b, k, is_dc = start, 0, 0, 0, True
    count, out, why, hit = 0, NONE, None, None
    dc = [0, 0, 0]
    rec_pos, rec_sum = ([0], [[0, 0, 0]]) if mode == 0 else (None, None)
    max_it = None if seg_bits is None else seg_bits + 70000  # (the kernel's bound: every symbol takes a bit, an MCU has at most 10 blocks)
    it = 0
    while True:
        if max_it is not None and it >= max_it:
            why = "iterations"
            break
        it += 1
        w = win[pos] if pos < nwin else 0
        e = (F.dc[i] if is_dc else F.ac[i])[w >> 16]
        if e == 0:
            why = "code"
            break
        length, sym = e >> 8, e & 255
        s, r = (sym, 0) if is_dc else (sym & 15, sym >> 4)
        if s > 15:
            why = "size"
            break
        val = _extend((w >> (32 - length - s)) & ((1 << s) - 1), s) if s else 0
        if is_dc:
            if trace is not None and s:
                trace.append((pos + length, pos + length + s))
            dc[i] += val
            k, is_dc = 1, False
        elif s == 0:
            k = k + 16 if r == 15 else 64
        else:
            k += r + 1
        pos += length + s
        if (mode == 2 or strict) and k > 64:
            why = "run"
            break
        if k >= 64:
            is_dc, k = True, 0
            b += 1
            if b == F.nblk[i]:
                b = 0
                i += 1
                if i == ns:
                    i = 0
                    count += 1
                    if limit_mcus is not None:
                        rec_pos.append(pos)
                        rec_sum.append(list(dc))
                        if count == limit_mcus:
                            out = pos
                            break
                        continue
                    if pos >= hi or pos + 8 > end_bits:
                        out = pos
                        break
                    if mode == 0:
                        if len(rec_pos) < SEG_MARKS:
                            rec_pos.append(pos - lo)
                            rec_sum.append(list(dc))
                    elif mode == 1 and pos in marks:
                        hit = marks.index(pos)
                        break
    res = dict(out=out, count=count, dc=dc, why=why, hit=hit, pos=pos)
    if rec_pos is not None:
        res["starts"], res["sum"] = rec_pos, rec_sum
    return res


def _i32(v):
    return ((int(v) + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)


# ---- layer A ---------------------------------------------------------------------------------------------------------------------------

def mcu_starts(F):
    """the sequential parse: (bit position of every MCU and behind the last, DC sums per scan component before each, the bit ranges of
    the DC magnitudes)"""
    if not hasattr(F, "_starts"):
        ranges = []
        r = decode(F, 0, 0, 0, strict=True, limit_mcus=F.total_mcus, trace=ranges)
        assert r["why"] is None and r["count"] == F.total_mcus, "the file does not parse"
        assert 0 <= F.end_bits - r["out"] < 8, "padding of less than a byte behind the last MCU"
        F._starts = (r["starts"], r["sum"], ranges)
    return F._starts


def true_chain(F, seg_bytes):
    """per segment dict(entry, out, count, dc, mcu_first, stream_off, bit_skip, item_dc), and whether the counts reach total_mcus (they do
    not when the exit rule cuts a last MCU of less than a byte off: such a file cannot verify).  The item of a segment begins at its entry
    (stream_off = entry >> 3, bit_skip = entry & 7) -- but for an entry at the very end of the scan (no padding), whose empty item is kept
    off the byte behind the scan: 0 and 0"""
    starts, sums, _ = mcu_starts(F)
    seg_bits = seg_bytes * 8
    n_segs = -(-len(F.stream) // seg_bytes)
    index = {p: j for j, p in enumerate(starts)}
    segs, entry, running = [], 0, 0
    for t in range(n_segs):
        hi = (t + 1) * seg_bits
        j = index[entry]
        if entry >= hi or entry + 8 > F.end_bits:
            out, j2 = entry, j
        else:
            j2 = j + 1
            while not (starts[j2] >= hi or starts[j2] + 8 > F.end_bits):
                j2 += 1
            out = starts[j2]
        count = min(j2 - j, F.total_mcus - running)
        behind = entry >= F.end_bits  # (no padding: the last MCU ends with the scan's last byte, and no item starts behind that byte)
        segs.append(dict(entry=entry, out=out, count=count, dc=[_i32(sums[j2][c] - sums[j][c]) for c in range(3)], mcu_first=running,
                         stream_off=0 if behind else entry >> 3, bit_skip=0 if behind else entry & 7, item_dc=[_i32(v) for v in sums[j]]))
        running += count
        entry = out
    return segs, running == F.total_mcus


# ---- layer B ---------------------------------------------------------------------------------------------------------------------------

def protocol(F, seg_bytes, fixed=True):
    """The kernels' rounds on one file.  fixed=False: the validation rounds and the count pass hand an entry on only at or behind the end
    of the scan (`e >= end_bits`), as they did before less than a byte of padding counted as the end.
    Returns dict(verified, segs: per segment the final SegState fields with `out`, round 0's n and out, the decodes its validation rounds
    began and the bits they read; events: what the validation
    rounds did at each segment's TRUE entry; round0: why round 0 broke off per segment or None; stable_after: the first round after which
    every entry is the true one, None if none is)."""
    seg_bits, end_bits = seg_bytes * 8, F.end_bits
    n = -(-len(F.stream) // seg_bytes)
    true_entry = [s["entry"] for s in true_chain(F, seg_bytes)[0]]
    at_end = (lambda e: e + 8 > end_bits) if fixed else (lambda e: e >= end_bits)
    st = [dict(entry=NONE, count=NONE, dc=[-1, -1, -1], frm=NONE, out_check=NONE, decodes=0, decoded_bits=0) for _ in range(n)]
    outs = [[NONE, NONE] for _ in range(n)]
    tabs, round0 = [], []
    for t in range(n):  # round 0
        lo = t * seg_bits
        r = decode(F, lo, lo + seg_bits, 0, lo=lo, seg_bits=seg_bits)
        st[t].update(entry=0 if t == 0 else NONE, frm=lo, count=0 if r["out"] == NONE else r["count"], dc=r["dc"], out_check=r["out"])
        outs[t][0] = r["out"]
        tabs.append(dict(n=len(r["starts"]), count=r["count"], dc=r["dc"], out=r["out"], pos=r["starts"], sum=r["sum"]))
        round0.append(r["why"])
    events = [set() for _ in range(n)]
    stable_after = None
    for rnd in range(1, ROUNDS + 1):
        rd, wr = (rnd + 1) & 1, rnd & 1
        prev = [o[rd] for o in outs]  # (double-buffered: every lane reads the last round's)
        for t in range(n):
            lo, hi = t * seg_bits, (t + 1) * seg_bits
            s, tab = st[t], tabs[t]
            e = 0 if t == 0 else prev[t - 1]
            outs[t][wr] = prev[t]
            if e == NONE:
                continue
            s["entry"] = e
            ev = events[t] if e == true_entry[t] else set()
            if e >= hi or at_end(e):
                s.update(frm=e, count=0, dc=[0, 0, 0], out_check=e)
                outs[t][wr] = e
                ev.add("pass_on")
                continue
            if e == s["frm"]:
                continue
            marks = [lo + p for p in tab["pos"]] if tab["out"] != NONE else []
            if e in marks:
                k = marks.index(e)
                s.update(frm=e, count=tab["count"] - k, dc=[_i32(tab["dc"][c] - tab["sum"][k][c]) for c in range(3)], out_check=tab["out"])
                outs[t][wr] = tab["out"]
                ev.add(("recorded", k))
                continue
            r = decode(F, e, hi, 1, marks=marks, seg_bits=seg_bits)
            s["decodes"] += 1
            s["decoded_bits"] += r["pos"] - e
            if r["hit"] is not None:
                k = r["hit"]
                r["count"] += tab["count"] - k
                r["dc"] = [_i32(r["dc"][c] + tab["dc"][c] - tab["sum"][k][c]) for c in range(3)]
                r["out"] = tab["out"]
                ev.add(("step_in", k))
            elif r["out"] != NONE:
                ev.add("to_the_end")
                if len(marks) == SEG_MARKS and e > marks[-1]:
                    ev.add("behind_the_16th")
            s.update(frm=e, count=0 if r["out"] == NONE else r["count"], dc=r["dc"], out_check=r["out"])
            outs[t][wr] = r["out"]
        if stable_after is None and [s["entry"] for s in st] == true_entry:
            stable_after = rnd
    for t in range(n):  # the count pass
        s = st[t]
        e = s["entry"]
        if e == NONE or e >= (t + 1) * seg_bits or at_end(e):
            s.update(count=0, dc=[0, 0, 0], out_check=e)
        elif s["frm"] != e:
            r = decode(F, e, (t + 1) * seg_bits, 2, seg_bits=seg_bits)
            s.update(frm=e, count=0 if r["out"] == NONE else r["count"], dc=r["dc"], out_check=r["out"])
    final = ROUNDS & 1
    ok, running, prev_out = True, 0, 0
    for t in range(n):  # the prefix check
        s, out = st[t], outs[t][final]
        if s["entry"] != (0 if t == 0 else prev_out) or s["entry"] == NONE or out == NONE or s["out_check"] != out:
            ok = False
        if s["entry"] != NONE and s["entry"] >= end_bits and s["count"] != 0:
            ok = False
        if ok:
            running += min(s["count"], F.total_mcus - running)
        prev_out = out
        s["out"], s["round0_n"], s["round0_out"] = out, tabs[t]["n"], tabs[t]["out"]
    return dict(verified=ok and running == F.total_mcus, segs=st, events=events, round0=round0, stable_after=stable_after)
