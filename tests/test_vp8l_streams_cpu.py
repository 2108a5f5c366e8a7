"""The token-level VP8L corpus (vp8l_streams.py) without a GPU: the corpus checks that it holds every placement it was written for, then
the plain Python reference (webp_util.decode), the host decoder (vp8l.h through rph_webp_decode_host) and Pillow (libwebp) each
reproduce the token expansion on every valid stream and refuse every refused one; the host decoder runs the whole corpus under
ASan + UBSan (tools/fuzz_webp_host.cpp) before any of it goes to a device."""
import io
import os
import subprocess

import numpy as np
import pytest

import vp8l_streams as vs
import webp_util as wu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _host(data):
    from rupphash_amd import Engine, RphError

    try:
        return 0, Engine.webp_decode_host(data)
    except RphError as e:
        return e.status, None


def test_every_family_is_present_and_groups_leave_no_stream_out():
    names = [n for n, _, _ in vs.valid_streams()]
    assert len(names) == len(set(names)) >= 250
    for family in vs.FAMILIES:
        assert any(n.startswith(family) for n in names), family
    grouped = [n for g in vs.GROUPS.values() for n in names if n.startswith(g)]
    assert sorted(grouped) == sorted(names)
    refused = [n for n, _ in vs.refused_streams()]
    for family in vs.REFUSED:
        assert family in refused, family
    assert sum(n.startswith("random_") for n in names) >= 100
    assert sum(px.size for _, _, px in vs.valid_streams()) <= 1_600_000
    assert max(px.shape[1] for _, _, px in vs.valid_streams()) >= 190 and min(px.shape[1] for _, _, px in vs.valid_streams()) == 1


def test_bit_start_residues_and_last_bit():
    res = {vs.BITS[n][0] % 32 for n, _, _ in vs.valid_streams()}
    assert res == set(range(32))
    assert {vs.BITS[f"bitstart_{r:02d}"][0] % 32 for r in (0, 1, 31)} == {0, 1, 31}
    name, data, _ = [f for f in vs.valid_streams() if f[0] == "endbit_exact"][0]
    assert vs.BITS[name][1] == 8 * int.from_bytes(data[16:20], "little")  # the last symbol ends on the chunk's last bit
    for name in ("zero_bits_one_literal", "zero_bits_cache_tokens_only"):
        assert vs.BITS[name][0] == vs.BITS[name][1]


def test_alphabets_and_groups_are_as_named():
    for k, alphabet in enumerate(("green", "red", "blue", "alpha", "distance")):
        assert vs.SYMBOLS[f"code_single_{alphabet}"][(0, k)][0] == 1, alphabet
        assert vs.SYMBOLS[f"code_two_{alphabet}"][(0, k)] == (2, 1), alphabet
        assert vs.SYMBOLS[f"code_deep_{alphabet}"][(0, k)] == (16, 15), alphabet  # (the 15-bit codes belong to symbols in use)
    assert all(v[1] == 15 for v in vs.SYMBOLS["dist_max_lit15_copy28"].values())  # (the builder asserts that the literal's four codes are such)
    for name in ("zero_bits_one_literal", "zero_bits_cache_tokens_only"):
        assert all(v[0] <= 1 for v in vs.SYMBOLS[name].values()), name
    for cb in (0, 4):
        # copies that end in front of a block of group 3, whose five codes have one symbol each in the `single` stream
        for kind in ("copies_cross_blocks", "single_symbol_group"):
            assert vs.FACTS[f"groups_cache{cb}_{kind}"]["tokens_of_group_3_behind_a_copy"] >= 1, (cb, kind)
        sym = vs.SYMBOLS[f"groups_cache{cb}_single_symbol_group"]
        assert all(sym[(3, k)][0] <= 1 for k in range(5)) and sym[(3, 0)][0] == 1 and all(sym[(g, 0)][0] > 1 for g in range(3))


def _walk(tokens, w, cb):
    """(token, position, pixels it writes) by the expansion rule"""
    px = []
    for t in tokens:
        at = len(px)
        if t[0] == "ref":
            d = wu.plane_distance(w, t[2])
            for _ in range(t[1]):
                px.append(px[-d])
        else:
            px.append(t[1] if t[0] == "lit" else None)
        yield t, at, px[at:]


def test_random_streams_hold_every_boundary_length_and_cache_collisions_inside_copies():
    lens, dists, collisions, cache_bits, groups = set(), set(), 0, set(), set()
    for name, _, _ in vs.valid_streams():
        if not name.startswith("random_"):
            continue
        tokens, w, cb = vs.TOKENS[name]
        cache_bits.add(cb)
        groups.add(int(name.split("groups")[1]))
        for t, at, px in _walk(tokens, w, cb):
            if t[0] != "ref":
                continue
            lens.add(t[1])
            dists.add(wu.plane_distance(w, t[2]))
            if cb:
                last = {}
                for v in px:
                    if v is not None:
                        k = vs.key(v, cb)
                        collisions += k in last and last[k] > v  # the later pixel of a slot numerically smaller
                        last[k] = v
    assert set(vs.LENS) <= lens and set(vs.DISTS) <= dists and collisions >= 1
    assert cache_bits == set(range(12)) and groups == set(range(1, 10))


def test_named_cache_streams_collide_as_placed():
    for name, _, px in vs.valid_streams():
        if "_copy_collision_" not in name:
            continue
        tokens, w, cb = vs.TOKENS[name]
        k = [i for i, t in enumerate(tokens) if t[0] == "cache"][0]
        (copy, at, cpx), slot = list(_walk(tokens[:k], w, cb))[-1], tokens[k][1]
        inside = [(i, v) for i, v in enumerate(cpx) if vs.key(v, cb) == slot]
        assert copy[0] == "ref" and len(inside) == 2 and inside[0][1] > inside[1][1], name
        assert (inside[0][0] // 64 == inside[1][0] // 64) == ("same_step" in name), name
        assert px.ravel()[at + len(cpx)] == inside[1][1], name


def test_reference_decoder_reproduces_the_expansion_and_refuses_the_refused():
    for name, data, px in vs.valid_streams():
        st, ref = wu.decode(data)
        assert st == 0 and np.array_equal(ref, vs.expected_image(px)), name
    for name, data in vs.refused_streams():
        assert wu.decode(data) == (wu.INVALID, None), name


def test_host_decoder_reproduces_the_expansion_and_refuses_the_refused():
    for name, data, px in vs.valid_streams():
        rc, got = _host(data)
        assert rc == 0 and got.dtype == np.uint8 and np.array_equal(got, vs.expected_image(px)), name
    for name, data in vs.refused_streams():
        assert _host(data) == (wu.INVALID, None), name


def test_libwebp_reproduces_the_expansion_and_refuses_the_refused():
    Image = pytest.importorskip("PIL.Image")

    def pillow(data):
        im = Image.open(io.BytesIO(data))
        im.load()
        return np.asarray(im)

    for name, data, px in vs.valid_streams():
        assert np.array_equal(pillow(data), vs.expected_image(px)), name
    for name, data in vs.refused_streams():
        with pytest.raises(Exception):
            pillow(data)


def test_libwebp_reads_the_pad_byte_behind_a_chunk_and_this_project_does_not():
    """the one place where the written rule is stricter than libwebp (include/rupphash.h, WebP section): a chunk cut to an odd size by
    a byte of zero bits is out of bits here; libwebp reads the container's pad byte for it and decodes the same pixels"""
    Image = pytest.importorskip("PIL.Image")
    name, data = vs.pad_byte_case()
    px = {n: p for n, _, p in vs.valid_streams()}[name]
    assert wu.decode(data) == (wu.INVALID, None) and _host(data) == (wu.INVALID, None)
    im = Image.open(io.BytesIO(data))
    assert np.array_equal(np.asarray(im), vs.expected_image(px))


def test_host_decoder_on_the_corpus_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """every refused stream is refused by the shared decoder's own bounds checks, and every valid one decoded, without a report"""
    for k, (name, data) in enumerate([(n, d) for n, d, _ in vs.valid_streams()] + vs.refused_streams()):
        (tmp_path / f"s{k:04d}.webp").write_bytes(data)
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    flags = ["-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    try:
        have = subprocess.run(["g++"] + flags + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode == 0
    except FileNotFoundError:
        have = False
    if not have:
        pytest.skip("no g++ with a sanitizer runtime here")
    exe, csrc = str(tmp_path / "fuzz_webp_host"), os.path.join(ROOT, "rupphash_amd", "csrc")
    subprocess.check_call(["g++"] + flags + ["-I", csrc, "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tools", "fuzz_webp_host.cpp"),
                           os.path.join(csrc, "webp_host.cpp"), "-o", exe])
    r = subprocess.run([exe, str(tmp_path), "4"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "no sanitizer report" in r.stdout, r.stdout + r.stderr[-3000:]
