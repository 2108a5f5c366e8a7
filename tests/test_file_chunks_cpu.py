"""The corpora of tests/file_chunks.py do what test_file_chunks_gpu.py relies on (no GPU: the library's host-only *_info and *_decode_host
calls and the split rule in Python): every pool has the files it promises; every predicted limit, at its small value, cuts some call into
at least four chunks and is the only limit that binds at some cut; one file alone exceeds the limit and lands in a chunk of its own; a
running sum that equals the limit keeps its file, one below opens the next chunk; the arrangement with damaged files at the chunks' edges
is what it says; no file of a call escapes the comparison, and the comparison notices two swapped result slots."""
import numpy as np
import pytest

import file_chunks as fc


@pytest.mark.parametrize("fmt", fc.FORMATS)
def test_pool_holds_what_the_gpu_tests_rely_on(fmt):
    from rupphash_amd import Engine

    ok, bad, refused = fc.of_kind(fmt, "ok"), fc.of_kind(fmt, "decode"), fc.of_kind(fmt, "parse")
    assert len(ok) >= 25 and len(refused) >= 5
    assert len(bad) >= 3 if fmt in fc.HAS_DECODE_FAILURES else not bad
    info = [getattr(Engine, fmt + "_info")(f.data) for f in ok]
    assert any(w < 128 and h < 128 for w, h, _, _ in info) and any(w > 128 and h > 128 for w, h, _, _ in info)
    assert any(w == 128 or h == 128 for w, h, _, _ in info) and any(max(w, h) > 512 for w, h, _, _ in info)
    assert sum(1 for w, h, _, _ in info if w * h <= 200 * 150) >= 0.85 * len(info)  # mostly small files: a call takes a second or two
    assert any(w < 5 or h < 5 for w, h, _, _ in info)  # valid = 0 with a pixel hash
    if fmt in ("png", "tiff"):  # 16-bit files take the RGBA16 / BLAKE3 path of hash_decoded_images
        assert sum(1 for i in info if i[3] == 16) >= 4 and sum(1 for i in info if i[3] == 8) >= 10
    if fmt == "webp":  # b_off placement: palette files behind the coded images
        assert sum(1 for f in ok if "palette" in f.name) >= 4 and sum(1 for f in ok if "palette" not in f.name) >= 10
    if fmt == "gif":
        frames = [fc.gif_frame_size(f.data) for f in ok]
        assert any(fw * fh > 16384 for fw, fh in frames) and any(fw * fh < 16384 for fw, fh in frames)
        assert sum(1 for f in ok if "interlace" in f.name) >= 3 and any((fw, fh) != i[:2] for (fw, fh), i in zip(frames, info))
    if fmt == "bmp":  # every depth class
        import bmp_streams as bs

        assert all(any(f.name.startswith(v + "_") for f in ok) for v in bs.VARIANTS)
    # a file that fails while it is decoded is as large as the valid ones, not only the rule corpus' 8 x 8
    if bad:
        assert any(f.q["pixels"] > 2000 for f in bad)


@pytest.mark.parametrize("fmt", fc.FORMATS)
def test_every_call_covers_the_pool_and_every_file_is_compared(fmt):
    names = {f.name for f in fc.pool(fmt)}
    for name, call in fc.calls(fmt).items():
        assert 100 <= len(call) <= 170, (name, len(call))
        assert {f.name for f in call} == names, name
    # the comparison walks every position: fake outputs, each file's own, pass; two swapped slots do not
    call = fc.calls(fmt)["shuffled"]
    rng = np.random.default_rng(3)
    dt = dict(hash=(np.uint8, (32,)), quality=(np.float32, ()), coeffs=(np.float32, (256,)), dihedral=(np.uint8, (8, 32)), valid=(np.uint8, ()),
              status=(np.int32, ()), pixel_hash=(np.uint8, (32,)))
    alone = {f.name: {k: rng.integers(0, 200, (1,) + shape).astype(t) for k, (t, shape) in dt.items()} for f in fc.pool(fmt)}
    out = {k: np.concatenate([alone[f.name][k] for f in call]) for k in dt}
    assert fc.compare(out, call, alone) == len(call)
    a, b = next((i, j) for i in range(len(call)) for j in range(i + 1, len(call)) if call[i].name != call[j].name)
    for k in dt:
        swapped = dict(out)
        swapped[k] = out[k].copy()
        swapped[k][[a, b]] = swapped[k][[b, a]]
        with pytest.raises(AssertionError):
            fc.compare(swapped, call, alone)


@pytest.mark.parametrize("fmt", fc.FORMATS)
def test_every_predicted_limit_cuts_and_binds_alone(fmt):
    for key in ("files",) + fc.PREDICTED[fmt]:
        limits = fc.lowered(fmt, key)
        cuts = {name: fc.predict(fmt, call, limits) for name, call in fc.calls(fmt).items()}
        assert max(len(s) for s, _ in cuts.values()) >= 4, key
        for name, (sizes, causes) in cuts.items():
            assert sum(sizes) == sum(1 for f in fc.calls(fmt)[name] if f.kind != "parse") and min(sizes) >= 1
            assert len(sizes) > 1 and all(c == {key} for c in causes[:-1]) and not causes[-1], (key, name)  # the others at their defaults
    # all lowered together: every predicted limit is, at some cut of some call, the only one that would have cut there
    limits = fc.lowered(fmt, *fc.limit_keys(fmt))
    alone = set()
    for call in fc.calls(fmt).values():
        sizes, causes = fc.predict(fmt, call, limits)
        assert len(sizes) >= 4
        alone.update(next(iter(c)) for c in causes if len(c) == 1)
    assert alone == {"files"} | set(fc.PREDICTED[fmt])


@pytest.mark.parametrize("fmt", fc.FORMATS)
def test_one_file_alone_exceeds_the_limit_and_forms_a_chunk_of_its_own(fmt):
    for key in fc.PREDICTED[fmt]:
        limits = fc.lowered(fmt, key)
        large = [f for f in fc.of_kind(fmt, "ok", "decode") if f.q[key] > fc.bound(fmt, key, limits)]
        assert len(large) == 1, key
        for name, call in fc.calls(fmt).items():
            sizes, _ = fc.predict(fmt, call, limits)
            enter = [f for f in call if f.kind != "parse"]
            starts = np.cumsum([0] + sizes)
            at = [k for k, f in enumerate(enter) if f is large[0]]
            assert len(at) >= 2 and all(k in starts and sizes[list(starts).index(k)] == 1 for k in at), (key, name)


@pytest.mark.parametrize("fmt", fc.FORMATS)
def test_a_sum_equal_to_the_limit_keeps_the_file_and_one_below_opens_the_next_chunk(fmt):
    for name, k in (("shuffled", 5), ("descending", 2), ("ascending", 9)):
        call = fc.calls(fmt)[name]
        at, below = fc.exact_fit(fmt, call, k)
        assert fc.predict(fmt, call, at)[0][0] == k and fc.predict(fmt, call, below)[0][0] == k - 1, (name, k)
        for key in fc.PREDICTED[fmt]:  # each limit on its own does the same
            assert fc.predict(fmt, call, fc.lowered(fmt, **{key: at[key]}))[0][0] >= k
            assert fc.predict(fmt, call, fc.lowered(fmt, **{key: below[key]}))[0][0] == k - 1


@pytest.mark.parametrize("fmt", fc.HAS_DECODE_FAILURES)
def test_damaged_files_sit_at_the_edges_of_chunks_and_fill_one(fmt):
    call = fc.calls(fmt)["edges"]
    enter = [f for f in call if f.kind != "parse"]
    for limits in (fc.lowered(fmt, "files"), fc.lowered(fmt, *fc.limit_keys(fmt))):
        sizes, _ = fc.predict(fmt, call, limits)
        starts = np.cumsum([0] + sizes)
        chunks = [enter[a:b] for a, b in zip(starts[:-1], starts[1:])]
        assert any(c[0].kind == "decode" and c[-1].kind == "ok" and len(c) > 1 for c in chunks)
        assert any(c[-1].kind == "decode" and c[0].kind == "ok" and len(c) > 1 for c in chunks)
        assert any(len(c) > 1 and all(f.kind == "decode" for f in c) for c in chunks)


def test_environment_names_every_limit_once():
    assert set(fc.ENV) == set(fc.DEFAULTS) and len(set(fc.ENV.values())) == len(fc.ENV)
    assert fc.environment(fc.DEFAULTS) == {}
    assert fc.environment(fc.lowered("png", "files")) == {"RPH_FILE_CHUNK_FILES": "8"}


def test_tiff_auto_call_is_below_the_ratio_as_a_whole_and_above_it_in_one_chunk():
    call, limits = fc.tiff_auto_call()
    enter = [f for f in call if f.kind != "parse"]
    ratio = lambda files: sum(f.q["raw"] for f in files) / sum(f.q["comp"] for f in files)
    assert ratio(enter) < 16
    sizes, _ = fc.predict("tiff", call, limits)
    starts = np.cumsum([0] + sizes)
    ratios = [ratio(enter[a:b]) for a, b in zip(starts[:-1], starts[1:])]
    assert len(sizes) >= 4 and max(ratios) >= 16 and min(ratios) < 16
