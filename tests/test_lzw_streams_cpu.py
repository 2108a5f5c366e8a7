"""The code-level LZW and byte-level PackBits corpus (lzw_streams.py) without a GPU: the corpus checks that it holds every placement it
was written for, then the plain Python reference (tiff_util.decode) and the host decoder (tiff_lzw.h through rph_tiff_decode_host)
reproduce the expansion of the codes on every valid stream and refuse every refused one, Pillow (libtiff) gives the same bytes wherever
it accepts a stream, and the host decoder runs the whole corpus under ASan + UBSan (tools/fuzz_tiff_host.cpp) before any of it goes to
a device."""
import io
import os
import subprocess

import numpy as np
import pytest

import lzw_streams as ls
import tiff_util as tu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# Streams that the written rule (include/rupphash.h, TIFF section) accepts and libtiff refuses, each with the reason.  Only streams of
# the families "table filled to 4095", "Clear placement", "missing EOI / trailing garbage" and "truncated final string" may stand here.
# libtiff (4.7) decodes every valid stream of the corpus, so the list is empty.
LIBTIFF_REFUSES = {}


def _host(data):
    from rupphash_amd import Engine, RphError

    try:
        return 0, Engine.tiff_decode_host(data)
    except RphError as e:
        return e.status, None


def test_every_family_is_present_and_groups_leave_no_stream_out():
    names = [n for n, _, _ in ls.valid_streams()]
    assert len(names) == len(set(names))
    assert sum(ls.INFO[n]["kind"] == "lzw" for n in names) >= 150 and sum(ls.INFO[n]["kind"] == "packbits" for n in names) >= 80
    for family in ls.FAMILIES:
        assert any(n.startswith(family) for n in names), family
    grouped = [n for g in ls.GROUPS.values() for n in names if n.startswith(g)]
    assert sorted(grouped) == sorted(names)
    refused = [n for n, _ in ls.refused_streams()]
    for family in ls.REFUSED:
        assert family in refused, family
    assert sum(n.startswith("random_") for n in names + refused) >= 100 and sum(n.startswith("pb_random_") for n in names + refused) >= 50
    assert any(n.startswith("random_") for n in refused) and any(n.startswith("pb_random_") for n in refused)


def test_placements_are_where_they_were_put():
    info = ls.INFO
    valid = {n for n, _, _ in ls.valid_streams()}
    assert max(info[n]["top"] for n in valid if n.startswith("random_")) == 4096  # a random list fills the table to its last entry
    for name in ("table_4095_then_clear", "table_4095_segment_ends_on_next_code", "longest_string_3839"):
        assert info[name]["top"] == 4096, name  # the table is filled to its last entry
    lo, hi = info["global_repeated_text"]["lengths"]
    assert 64 <= lo and hi <= 201 and info["global_repeated_text"]["cap"] > 16384 and info["global_one_byte_run"]["cap"] > 16384
    assert {(info[f"bits_offset_{o}_len_{n}"]["offset"] % 4, info[f"bits_offset_{o}_len_{n}"]["comp_len"] % 4) for o in range(4) for n in range(4)} == \
        {(o, n) for o in range(4) for n in range(4)}
    late = info["refuse_code_above_next_after_20000"]  # refused for its code above the next entry, in a global-memory segment
    assert late["cap"] > 16384 and late["good_bytes"] >= 20000 and late["next_there"] < late["code"] < 4096
    assert info["lds_70_strips_of_111"]["strips"] >= 64 and info["lds_70_strips_of_111"]["cap"] % 16
    assert {info[f"strips_mod16_{r}"]["cap"] % 16 for r in range(1, 16)} == set(range(1, 16))
    assert info["pb_every_control_byte"]["controls"] == set(range(256))
    assert info["pb_1500_short_tokens"]["tokens"] >= 1000 and info["pb_40_strips_of_1_byte"]["cap"] == 1
    for n in (63, 64, 65, 127, 128, 129):
        assert info[f"kwkwk_prev_{n}"]["prev_len"] == n


def test_reference_and_host_decoders_reproduce_the_expansion_and_refuse_the_refused():
    for name, data, px in ls.valid_streams():
        st, ref = tu.decode(data)
        assert st == 0 and ref.dtype == np.uint8 and np.array_equal(ref, px), name
        rc, got = _host(data)
        assert rc == 0 and got.dtype == np.uint8 and np.array_equal(got, px), name
    for name, data in ls.refused_streams():
        assert tu.decode(data) == (tu.INVALID, None), name
        assert _host(data) == (tu.INVALID, None), name


def test_libtiff_gives_the_expected_bytes_wherever_it_accepts_a_stream():
    Image = pytest.importorskip("PIL.Image")
    refuses = []
    for name, data, px in ls.valid_streams():
        try:
            im = Image.open(io.BytesIO(data))
            im.load()
        except Exception:
            refuses.append(name)
            continue
        assert np.array_equal(np.asarray(im), px), name
    assert sorted(refuses) == sorted(LIBTIFF_REFUSES)  # (a listed stream that libtiff decodes fails here as well)


def test_host_decoder_on_the_corpus_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """every refused stream is refused by the shared decoders' own bounds checks, and every valid one decoded, without a report"""
    for k, (name, data) in enumerate([(n, d) for n, d, _ in ls.valid_streams()] + ls.refused_streams()):
        (tmp_path / f"s{k:04d}.tif").write_bytes(data)
    # is there a sanitizer runtime at all?  Asked of a trivial program, so that a failure to build the real sources fails the test
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    flags = ["-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    try:
        have = subprocess.run(["g++"] + flags + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode == 0
    except FileNotFoundError:
        have = False
    if not have:
        pytest.skip("no g++ with a sanitizer runtime here")
    exe, csrc = str(tmp_path / "fuzz_tiff_host"), os.path.join(ROOT, "rupphash_amd", "csrc")
    subprocess.check_call(["g++"] + flags + ["-I", csrc, "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tools", "fuzz_tiff_host.cpp"),
                           os.path.join(csrc, "tiff_host.cpp"), "-o", exe])
    r = subprocess.run([exe, str(tmp_path), "4"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "no sanitizer report" in r.stdout, r.stdout + r.stderr[-3000:]
