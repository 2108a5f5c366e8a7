"""The segment synchroniser on the device (jpeg_sync_kernel, jpeg_seg_items_kernel) against its model: the corpus of
jpeg_segment_corpus.py, every file forced into segments, with the log of what the synchroniser decided (Engine.debug_jpeg_segment_log).
A file whose chain does not verify is walked whole and gives the same coefficients, so hashes cannot tell whether the fast path was taken:
the log can.  For every file the device's verdict must be the model's; for a verified file every segment's entry, exit, count and DC sums and
every walk item must be what the sequential parse of the file says (layer A), field for field; round 0's record and the final states must
be the protocol restatement's (layer B) for every file; and the hashes, qualities and coefficients must be the host decoder's bit for bit."""
import numpy as np
import pytest

import jpeg_segment_corpus as jc

pytestmark = pytest.mark.gpu
PIL = pytest.importorskip("PIL")

SEG_FIELDS = ("entry", "out", "count", "dc0", "dc1", "dc2", "from", "out_check", "round0_n", "round0_out", "mcu_first", "mcu_count", "stream_off", "bit_skip",
              "item_dc0", "item_dc1", "item_dc2", "decodes", "decoded_bits")


@pytest.fixture(scope="module")
def eng():
    from rupphash_amd import Engine

    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def host(eng):
    """the host decoder's results for the whole corpus, computed once"""
    eng.jpeg_set_entropy(0)
    try:
        return eng.jpeg_pdq_hash_batch([f["data"] for f in jc.files()], threads=8, want_coeffs=True)
    finally:
        eng.jpeg_set_entropy(2)


def run(eng, which, seg_bytes, log=True):
    """the corpus files `which` in one call, every one cut into segments of seg_bytes: (outputs, log of files, log of segments)"""
    eng.jpeg_set_entropy(1)
    eng.jpeg_set_segments(0, seg_bytes)
    eng.debug_jpeg_segment_log(log)
    try:
        out = eng.jpeg_pdq_hash_batch([jc.files()[k]["data"] for k in which], threads=4, want_coeffs=True)
        files, segs = eng.debug_jpeg_segments()
    finally:
        eng.debug_jpeg_segment_log(False)
        eng.jpeg_set_segments()
        eng.jpeg_set_entropy(2)
    return out, files, segs


def same_results(out, host, which):
    assert out["valid"].all() and not out["status"].any()
    assert np.array_equal(out["hash"], host["hash"][which])
    assert np.array_equal(out["quality"].view(np.uint32), host["quality"][which].view(np.uint32))
    assert np.array_equal(out["coeffs"].view(np.uint32), host["coeffs"][which].view(np.uint32))


def records(files, segs, j):
    """the segment records of the log's j-th file, one tuple of SEG_FIELDS per segment"""
    a, n = int(files["first_record"][j]), int(files["n_segs"][j])
    return [tuple(int(segs[name][a + t]) for name in SEG_FIELDS) for t in range(n)]


def check_against_model(which, seg_bytes, files, segs):
    """every file of the call against the model: returns (files verified, files fallen back)"""
    assert sorted(files["index"].tolist()) == list(range(len(which)))  # every file was cut into segments, each logged once
    verified = 0
    for j, pos in enumerate(files["index"].tolist()):
        k = which[pos]
        f = jc.files()[k]
        F = f["F"]
        chain, _, R = jc.model(seg_bytes)[k]
        got = records(files, segs, j)
        print(f"{seg_bytes:5d} {f['name']}: {len(got)} segments, device {'verified' if files['verified'][j] else 'fell back'}, model "
              f"{'verifies' if R['verified'] else 'falls back'}")
        assert (int(files["n_segs"][j]), int(files["total_mcus"][j]), int(files["scan_bits"][j])) == (len(chain), F.total_mcus, F.end_bits), f["name"]
        assert bool(files["verified"][j]) == R["verified"], f["name"]
        for t, (g, c, s) in enumerate(zip(got, chain, R["segs"])):
            d = dict(zip(SEG_FIELDS, g))
            where = (f["name"], seg_bytes, t)
            # layer B, every file: round 0's record, and where the rounds and the count pass left the segment
            assert (d["round0_n"], d["round0_out"]) == (s["round0_n"], s["round0_out"]), where
            assert (d["decodes"], d["decoded_bits"]) == (s["decodes"], s["decoded_bits"]), where  # what the validation rounds cost: no decode where the record answers
            assert (d["entry"], d["out"], d["from"], d["out_check"], d["count"]) == (s["entry"], s["out"], s["frm"], s["out_check"], s["count"]), where
            if R["verified"]:  # layer A: the chain and the items that the file's own MCU positions dictate
                assert (d["entry"], d["out"], d["out_check"], d["count"]) == (c["entry"], c["out"], c["out"], c["count"]), where
                assert [d["dc0"], d["dc1"], d["dc2"]] == c["dc"], where
                assert (d["mcu_first"], d["mcu_count"], d["stream_off"], d["bit_skip"]) == (c["mcu_first"], c["count"], c["stream_off"], c["bit_skip"]), where
                assert [d["item_dc0"], d["item_dc1"], d["item_dc2"]] == c["item_dc"], where
                assert not (d["entry"] + 8 > F.end_bits and d["count"]), where  # padding is never decoded as MCUs
            else:  # one whole-file item in the file's first place, nothing in the others
                assert d["mcu_count"] == 0, where
                if t == 0:
                    assert (d["mcu_first"], d["stream_off"], d["bit_skip"], d["item_dc0"], d["item_dc1"], d["item_dc2"]) == (0, 0, 0, 0, 0, 0), where
        verified += R["verified"]
    return verified, len(which) - verified


@pytest.mark.parametrize("call", ["annex_k", "all"])
@pytest.mark.parametrize("seg_bytes", jc.SEG_SIZES)
def test_the_log_is_the_models_and_the_results_the_host_decoders(eng, host, seg_bytes, call):
    """the corpus at every segment size (1024: the files longer than that), once as a call of at most 8 distinct Huffman tables -- the kernels
    that keep the tables in LDS -- and once with every file: more than 8, the kernels that read them from memory"""
    which = jc.annex_k_only() if call == "annex_k" else list(range(len(jc.files())))
    if seg_bytes == 1024:
        which = [k for k in which if k in jc.subset_1024()]
    out, files, segs = run(eng, which, seg_bytes)
    same_results(out, host, which)
    n_tables = len(set().union(*[jc.files()[k]["F"].distinct_tables for k in which]))
    assert (n_tables <= 8) == (call == "annex_k")
    assert (files["n_luts"] == n_tables).all()  # one chunk, its tables interned: <= 8 take jpeg_sync_kernel<HUFF_LDS_TABLES, .>, more <0, .>
    verified, fell_back = check_against_model(which, seg_bytes, files, segs)
    print(f"{seg_bytes} bytes, {call}: {verified} files verified, {fell_back} fell back, {int(files['n_segs'].sum())} segments")
    assert verified + fell_back == len(which) and verified > 0


def test_the_launch_geometry_the_corpus_was_chosen_for(eng, host):
    """64-byte segments, every file: more than 256 segments, no multiple of 256; one chunk whose files lie segment behind segment; at
    least 3 files share a workgroup of 256 lanes; a file begins at lane 0 of a workgroup"""
    which = list(range(len(jc.files())))
    _, files, _ = run(eng, which, 64)
    first, n = files["first_seg"].astype(np.int64), files["n_segs"].astype(np.int64)
    order = np.argsort(first)
    assert np.array_equal(first[order], np.concatenate([[0], np.cumsum(n[order])[:-1]]))
    total = int(n.sum())
    assert total == sum(len(m[0]) for m in jc.model(64)) and total > 256 and total % 256
    per_group = np.zeros(total // 256 + 1, np.int64)
    for a, b in zip(first, first + n - 1):
        per_group[a // 256:b // 256 + 1] += 1
    assert per_group.max() >= 3 and (first % 256 == 0).any()


def test_the_same_call_twice_leaves_the_same_log(eng, host):
    """every buffer is reused: the states, the two `out` slots, round 0's records and the items of the call before are still there"""
    which = list(range(len(jc.files())))
    a = run(eng, which, 68)
    run(eng, which[::2], 64)  # (another call in between: other files at the same places)
    b = run(eng, which, 68)
    same_results(b[0], host, which)
    for x, y in ((a[1], b[1]), (a[2], b[2])):
        assert x.keys() == y.keys() and all(np.array_equal(x[name], y[name]) for name in x)


def test_the_outputs_do_not_depend_on_the_log_switch(eng, host):
    which = list(range(len(jc.files())))
    for seg_bytes in (64, 256):
        on, files, _ = run(eng, which, seg_bytes, log=True)
        off, no_files, no_segs = run(eng, which, seg_bytes, log=False)
        assert len(files["index"]) == len(which) and len(no_files["index"]) == 0 and len(no_segs["entry"]) == 0
        for name in ("hash", "quality", "coeffs", "valid", "status"):
            assert np.array_equal(on[name].view(np.uint8), off[name].view(np.uint8)), name
        same_results(off, host, which)


def test_a_files_verdict_does_not_depend_on_its_neighbour(eng, host):
    """files whose last MCU straddles the last boundary and leaves padding -- all those that the earlier rule sent to the whole-file
    walk, and six more -- and the upper rungs of the ladder: alone in a call (nothing behind them in the chunk's stream buffer), and with
    another file before and behind them, one whose values are runs of one bits.  The log of the file is the same in all three calls, and
    its verdict the model's"""
    partner = next(k for k, (gen, kw) in enumerate(jc.CORPUS) if gen == "ones")
    for seg_bytes in (64, 68):
        cl = jc.classes(seg_bytes)
        decoded = [k for k in range(len(jc.files())) if "padding_decoded_before_the_fix" in cl[k]]
        others = [k for k in range(len(jc.files())) if "last_mcu_straddles_padding" in cl[k] and k not in decoded and k != partner]
        assert len(decoded) >= 2 and len(others) >= 6
        witnesses = decoded + others[:6] + [8, 9, 10, 11]
        for k in witnesses:
            seen = []
            for which in ([k], [k, partner], [partner, k]):
                out, files, segs = run(eng, which, seg_bytes)
                same_results(out, host, which)
                j = files["index"].tolist().index(which.index(k))
                seen.append((bool(files["verified"][j]), records(files, segs, j)))
                if len(which) == 2:
                    seen.append(bool(files["verified"][1 - j]))
            assert seen[0] == seen[1] == seen[3] and seen[2] == seen[4], jc.name_of(k)
            assert seen[0][0] == jc.model(seg_bytes)[k][2]["verified"], jc.name_of(k)


def test_the_encoders_expectations_hold_through_the_oracle(eng, oracle, host):
    """a sample of the corpus: the coefficients the encoder aimed at are what the oracle's decoder holds, and the device's hash of the
    segmented file is the hash of the oracle's decode"""
    sample = [2, 10, 27, 36, 40, 47]
    out, _, _ = run(eng, sample, 64)
    for pos, k in enumerate(sample):
        f = jc.files()[k]
        assert np.array_equal(oracle.jpeg_coefficients(f["data"])[2], f["expected"]), f["name"]
        rc, coeffs, _ = oracle.pdq_features(oracle.jpeg_decode(f["data"], 0))
        assert rc == 0 and np.array_equal(out["hash"][pos], oracle.to_hash(coeffs)), f["name"]
