"""The segment synchroniser's model (jpeg_segments.py) against the corpus (jpeg_segment_corpus.py), without a device: layer A's parse is
held to the positions the encoder wrote, layers A and B -- which share only the symbol reader -- to each other, and what the corpus is a
witness of is pinned, so that a change to a generator, to the model or to the protocol's restatement shows here first."""
import time

import pytest

import jpeg_segment_corpus as jc
import jpeg_segments as js

SIZES = (64, 68, 256)

# files of the corpus (out of 50) that belong to each class at 64, 68 or 256-byte segments; every class has at least two
CLASS_FILES = {
    # boundary positions
    "start_at_boundary": 9, "start_at_hi_minus_1": 3, "start_at_hi_plus_1": 5,
    "entry_is_the_boundary": 3, "entry_is_a_recorded_start": 28, "entry_is_the_16th_start": 3,
    "step_in": 31, "step_in_at_the_2nd": 20, "step_in_at_the_16th": 3, "decode_to_the_end": 44,
    # many MCU starts in one segment
    "table_full": 14, "entry_behind_the_16th": 7,
    # long MCUs
    "pass_on": 26, "pass_on_several": 16,
    # break-offs in round 0 of files that verify
    "round0_no_code_annex_k": 25, "round0_no_code_other_tables": 7, "round0_size_above_15": 3,
    # the end of the scan
    "padding_0": 7, "padding_1": 7, "padding_7": 6, "length_multiple_of_segment": 3, "last_segment_4_bytes": 3, "one_segment": 7,
    "last_segment_without_mcu": 40, "last_mcu_straddles_padding": 36, "padding_decoded_before_the_fix": 8, "last_mcu_shorter_than_a_byte": 3,
    # DC sums
    "dc_sums_beyond_int16": 3, "boundary_in_dc_bits": 3,
    # scan layouts
    "layout_gray": 21, "layout_444": 3, "layout_422": 3, "layout_440": 3, "layout_420": 17, "layout_2x1_2x1_2x1": 3, "gray_odd_width": 10,
    "verifies": 47, "falls_back": 22,
}
# the files whose chain does not verify, per segment size (1024: of the subset that runs there)
FALLS_BACK = {
    64: [10, 11, 12, 13, 14, 20, 21, 22, 23, 32, 39, 40, 41, 42, 43, 45, 46],
    68: [4, 5, 7, 8, 9, 12, 13, 14, 20, 21, 22, 23, 32, 42, 43, 45, 46],
    256: [21, 22, 23],
    1024: [],
}
# files 21..23 (gray, Annex K) end in an MCU of 6 bits with at most one bit of padding: the exit rule `pos + 8 > end_bits` cuts it off, the
# counts never reach total_mcus, and the file is walked whole at every segment size
CUT_OFF = [21, 22, 23]
LADDER = range(2, 12)  # one MCU that touches 6, 6, 7, 7, 8, 8, 9, 9, 10, 10 segments of 64 bytes and begins in segment 0


def test_the_corpus_is_what_the_issue_asks_for():
    files = jc.files()
    assert len(files) == 50
    for f in files:
        F = f["F"]
        assert 8 <= F.w <= 160 and 8 <= F.h <= 160
    lengths = sorted(len(f["F"].stream) for f in files)
    assert lengths[0] < 64 and 15000 < lengths[-1] < 17000
    assert sum(f["positions"] is None for f in files) == 7  # Pillow's
    assert len(jc.annex_k_only()) == 36 and len(jc.subset_1024()) == 15
    assert len(set().union(*[files[k]["F"].distinct_tables for k in jc.annex_k_only()])) == 5  # at most 8: the kernels with tables in LDS
    assert len(set().union(*[f["F"].distinct_tables for f in files])) == 26                    # more than 8: tables in memory


def test_layer_a_finds_the_mcus_where_the_encoder_wrote_them():
    """two statements of one fact, neither derived from the kernel: the bit position of every MCU as the encoder counted the bits it
    put, and as the sequential parse of the file's own tables and bytes finds them"""
    checked = 0
    for f in jc.files():
        starts, sums, _ = js.mcu_starts(f["F"])
        assert len(starts) == f["F"].total_mcus + 1 and len(sums) == len(starts)
        if f["positions"] is not None:
            assert starts == f["positions"], f["name"]
            checked += 1
    assert checked == 43


@pytest.mark.parametrize("seg_bytes", SIZES + (1024,))
def test_the_chain_covers_every_mcu_and_both_layers_agree(seg_bytes):
    """layer A's chain is linked (entry = the predecessor's out, from 0) and its counts sum to total_mcus, but for the files whose last MCU
    the exit rule cuts off; where layer B's rounds verify a file they end at layer A's chain, field by field, and a file that layer B's
    rounds reach the true entries of (stable_after) verifies; no entry from which less than a byte is left is decoded from"""
    for k, (f, (chain, settles, R)) in enumerate(zip(jc.files(), jc.model(seg_bytes))):
        F = f["F"]
        assert len(chain) == -(-len(F.stream) // seg_bytes)
        assert chain[0]["entry"] == 0 and all(a["out"] == b["entry"] for a, b in zip(chain, chain[1:]))
        assert settles == (k not in CUT_OFF), f["name"]
        assert sum(c["count"] for c in chain) == (F.total_mcus if settles else F.total_mcus - 1)
        assert R["verified"] == (R["stable_after"] is not None and settles), f["name"]
        for c, s in zip(chain, R["segs"]):
            if c["entry"] + 8 > F.end_bits:
                assert c["count"] == 0 and c["out"] == c["entry"]
            if R["verified"]:
                assert (s["entry"], s["out"], s["out_check"], s["count"]) == (c["entry"], c["out"], c["out"], c["count"]), f["name"]
                assert [js._i32(v) for v in s["dc"]] == c["dc"], f["name"]


def test_which_files_verify_is_pinned():
    for seg_bytes, want in FALLS_BACK.items():
        which = jc.subset_1024() if seg_bytes == 1024 else range(len(jc.files()))
        assert [k for k in which if not jc.model(seg_bytes)[k][2]["verified"]] == want, seg_bytes


def test_what_the_corpus_is_a_witness_of_is_pinned():
    per = {}
    for seg_bytes in SIZES:
        for k, cl in enumerate(jc.classes(seg_bytes)):
            for c in cl:
                if not c.startswith("stable_after"):
                    per.setdefault(c, set()).add(k)
    assert {c: len(v) for c, v in per.items()} == CLASS_FILES
    assert min(CLASS_FILES.values()) >= 2


def test_the_ladder_splits_at_the_eighth_round():
    """The long MCU begins in segment 0, whose exit is right from round 0 on; each segment it covers hands the position on one round later,
    so the segment it ends in -- the s-th it touches -- learns its entry in round s - 1: 9 segments are the most that 8 rounds settle"""
    spans = [jc.longest_span(jc.files()[k]["F"], 64) for k in LADDER]
    assert spans == [6, 6, 7, 7, 8, 8, 9, 9, 10, 10]
    verdicts = [jc.model(64)[k][2]["verified"] for k in LADDER]
    assert verdicts == [s <= 9 for s in spans]
    assert [jc.model(64)[k][2]["stable_after"] for k in LADDER][6:8] == [8, 8]
    for k in LADDER:  # (with 256-byte segments the same MCU touches 2 or 3)
        assert jc.model(256)[k][2]["verified"]


def test_padding_was_decoded_before_it_counted_as_the_end():
    """the witnesses of the padding case: the last MCU begins before the last boundary and ends behind it with 1..7 bits of padding.  With
    the earlier rule (`e >= end_bits`) the last segment decodes padding and the zeros behind the scan as MCUs; in these files that decode
    breaks off (their tables have no code for it) and the file falls back.  With `e + 8 > end_bits` they verify."""
    n = 0
    for seg_bytes in SIZES:
        for k, cl in enumerate(jc.classes(seg_bytes)):
            if "padding_decoded_before_the_fix" in cl:
                F = jc.files()[k]["F"]
                assert jc.model(seg_bytes)[k][2]["verified"] and not js.protocol(F, seg_bytes, fixed=False)["verified"]
                n += 1
    assert n == 10


def test_the_model_is_quick_enough_to_run_everywhere():
    t0 = time.time()
    for seg_bytes in SIZES + (1024,):
        jc.classes(seg_bytes)
    assert time.time() - t0 < 120  # (a few seconds; computed once per process, cached in the corpus module)
