"""The chunk and window splits of the PNG, TIFF, WebP, GIF and BMP batch calls on the device (-m gpu), at limits lowered through the
environment rph_init reads (tests/file_chunks.py: pools, calls, the split rule in Python).  The reference is every distinct pool file
hashed alone on a context with the default limits; every comparison is bit for bit on all seven outputs.  rph_debug_file_chunks tells
what a call did: a test whose override was ignored would otherwise pass on one chunk and prove nothing."""
import contextlib
import functools
import os

import numpy as np
import pytest

import file_chunks as fc

pytestmark = pytest.mark.gpu

HOST, DEVICE, AUTO = 0, 1, 2
SET_MODE = dict(png="png_set_inflate", tiff="tiff_set_decompress", webp="webp_set_entropy", gif="gif_set_decompress")


@contextlib.contextmanager
def engine(limits=None):
    """a context made with `limits` in the environment (read once, by rph_init), closed on the way out; one at a time"""
    from rupphash_amd import Engine

    env = fc.environment(limits or fc.DEFAULTS)
    os.environ.update(env)
    try:
        e = Engine(0)
    finally:
        for k in env:
            del os.environ[k]
    try:
        yield e
    finally:
        e.close()


def batch(e, fmt, files, threads=0):
    return getattr(e, fmt + "_pdq_hash_batch")([f.data for f in files], threads=threads, want_coeffs=True, want_dihedral=True, want_pixel_hash=True)


@functools.lru_cache(maxsize=None)
def alone(fmt):
    """{name: outputs} of every pool file in a call of its own, default limits; the kinds are what the helper says they are"""
    out = {}
    with engine() as e:
        for f in fc.pool(fmt):
            out[f.name] = batch(e, fmt, [f])
            assert e.debug_file_chunks(fmt)[0] == ([] if f.kind == "parse" else [1]), f.name
            assert (out[f.name]["status"][0] == 0) == (f.kind == "ok"), f.name
            for key in fc.KEYS:  # nothing for a file with a status
                assert f.kind == "ok" or key == "status" or not np.asarray(out[f.name][key]).any(), (f.name, key)
    return out


def run(e, fmt, call, threads=0):
    """one call: every file's outputs are what it got alone; the chunks hold every file that parsed, none is empty -> (sizes, windows)"""
    out = batch(e, fmt, call, threads)
    assert fc.compare(out, call, alone(fmt)) == len(call)
    sizes, windows = e.debug_file_chunks(fmt)
    assert sum(sizes) == sum(1 for f in call if f.kind != "parse") and all(s >= 1 for s in sizes)
    return sizes, windows


def predicted_keys(fmt):
    return ("files",) + fc.PREDICTED[fmt]


def check_oversize(fmt, key, call, sizes, limits):
    """the one pool file that alone exceeds the limit sits in a chunk of its own wherever the call has it"""
    large = [f for f in fc.of_kind(fmt, "ok", "decode") if f.q[key] > fc.bound(fmt, key, limits)]
    assert len(large) == 1
    starts = list(np.cumsum([0] + sizes))
    at = [k for k, f in enumerate(f for f in call if f.kind != "parse") if f is large[0]]
    assert at and all(k in starts and sizes[starts.index(k)] == 1 for k in at), key


@pytest.mark.parametrize("fmt", fc.FORMATS)
def test_default_limits_make_one_chunk(fmt):
    with engine() as e:
        for name, call in fc.calls(fmt).items():
            sizes, windows = run(e, fmt, call)
            assert sizes == [sum(1 for f in call if f.kind != "parse")], name
            assert windows == (1 if fmt == "webp" else 0)


@pytest.mark.parametrize("fmt", fc.FORMATS)
def test_each_limit_alone(fmt):
    """only that limit lowered.  A predicted limit: the chunk sizes are the Python rule's, exactly, the oversize file alone in its chunk.
    Compressed bytes and WebP tables: more than one chunk, and half the limit never gives fewer."""
    for key in predicted_keys(fmt):
        limits = fc.lowered(fmt, key)
        with engine(limits) as e:
            for name, call in fc.calls(fmt).items():
                sizes, windows = run(e, fmt, call)
                assert len(sizes) > 1 and sizes == fc.predict(fmt, call, limits)[0], (key, name)
                if key != "files":
                    check_oversize(fmt, key, call, sizes, limits)
                elif fmt == "webp":
                    assert windows == -(-len(call) // limits["files"])
    for key in fc.UNPREDICTED[fmt]:
        limits = fc.lowered(fmt, key)
        counts = []
        for lim in (limits, dict(limits, **{key: limits[key] // 2})):
            with engine(lim) as e:
                counts.append([len(run(e, fmt, call)[0]) for call in fc.calls(fmt).values()])
        assert all(a > 1 and b >= a for a, b in zip(*counts)), (key, counts)


@pytest.mark.parametrize("fmt", fc.FORMATS)
def test_all_limits_lowered_together(fmt):
    """the predicted limits together: the rule's chunks, exactly; then every limit the format reads: more than one chunk"""
    limits = fc.lowered(fmt, *predicted_keys(fmt))
    with engine(limits) as e:
        for name, call in fc.calls(fmt).items():
            sizes, _ = run(e, fmt, call)
            assert len(sizes) > 1 and sizes == fc.predict(fmt, call, limits)[0], name
    with engine(fc.lowered(fmt, *fc.limit_keys(fmt))) as e:
        for name, call in fc.calls(fmt).items():
            sizes, windows = run(e, fmt, call)
            # (a part of a chunk that fits fits as well, so taking all that fits gives the fewest chunks: further limits only add some)
            assert len(sizes) >= len(fc.predict(fmt, call, limits)[0]) > 1, name
            assert fmt != "webp" or 2 <= windows <= len(call)


@pytest.mark.parametrize("fmt", fc.FORMATS)
def test_exact_fit(fmt):
    """every predicted sum of the first chunk equal to its limit at the fifth file: the file stays; one lower: it opens the next chunk"""
    call, k = fc.calls(fmt)["shuffled"], 5
    for limits, first in zip(fc.exact_fit(fmt, call, k), (k, k - 1)):
        with engine(limits) as e:
            sizes, _ = run(e, fmt, call)
            assert sizes[0] == first and sizes == fc.predict(fmt, call, limits)[0]


@pytest.mark.parametrize("fmt", fc.HAS_DECODE_FAILURES)
def test_decode_modes(fmt):
    """host, device and automatic decoding: the same chunks and the same outputs, with files that fail while they are decoded first in a
    chunk, last in a chunk and alone in one (whose hash stage has nothing to do)"""
    limits = fc.lowered(fmt, *predicted_keys(fmt))
    with engine(limits) as e:
        for mode in (HOST, DEVICE, AUTO):
            getattr(e, SET_MODE[fmt])(mode)
            for name in ("ascending", "edges"):
                call = fc.calls(fmt)[name]
                assert run(e, fmt, call)[0] == fc.predict(fmt, call, limits)[0], (mode, name)


def test_bmp_files_the_parser_refuses_at_the_edges_of_the_call():
    limits = fc.lowered("bmp", *predicted_keys("bmp"))
    call = fc.calls("bmp")["edges"]
    assert call[0].kind == call[-1].kind == "parse"
    with engine(limits) as e:
        assert run(e, "bmp", call)[0] == fc.predict("bmp", call, limits)[0]


def test_tiff_auto_mode_is_decided_per_chunk():
    """below 16:1 as a whole (one chunk: the host decompresses everything), at or above it in the chunk of flat files once the call is
    cut (the device decompresses those): the same outputs"""
    call, limits = fc.tiff_auto_call()
    enter = [f for f in call if f.kind != "parse"]
    ratio = lambda files: sum(f.q["raw"] for f in files) / sum(f.q["comp"] for f in files)
    cuts = fc.predict("tiff", call, limits)[0]
    starts = np.cumsum([0] + cuts)
    ratios = [ratio(enter[a:b]) for a, b in zip(starts[:-1], starts[1:])]
    assert ratio(enter) < 16 and max(ratios) >= 16 and min(ratios) < 16
    for lim, want in ((limits, cuts), (None, [len(enter)])):
        with engine(lim) as e:
            e.tiff_set_decompress(AUTO)
            assert run(e, "tiff", call)[0] == want


@pytest.mark.parametrize("fmt", fc.FORMATS)
def test_buffers_kept_across_calls(fmt):
    """descending (the kept buffers start large), ascending (every chunk larger than the one before: the buffers regrow mid-call),
    release, ascending again (everything allocated anew, then regrown)"""
    limits = fc.lowered(fmt, *predicted_keys(fmt))
    with engine(limits) as e:
        for name in ("descending", "ascending", None, "ascending"):
            if name is None:
                getattr(e, fmt + "_release")()
                continue
            call = fc.calls(fmt)[name]
            assert run(e, fmt, call)[0] == fc.predict(fmt, call, limits)[0], name


@pytest.mark.parametrize("limit", [1, 200000])
def test_webp_windows(limit):
    """a parse window ends at the first file that finds the window's tables above their limit; files behind it that were parsed meanwhile
    are thrown away, damaged ones among them, and parsed again.  How far a window overshoots depends on the threads' timing: at least two
    windows, at most one per file.  At limit 1 every file's own tables exceed the limit: the first file of a window is parsed all the
    same, or no file would get its outputs."""
    limits = fc.lowered("webp", webp_window_tables=limit)
    with engine(limits) as e:
        for threads in (1, 3, 16):
            for name in ("shuffled", "edges"):
                call = fc.calls("webp")[name]
                sizes, windows = run(e, "webp", call, threads)
                assert 2 <= windows <= len(call), (threads, name)
                assert len(sizes) >= 2  # (a chunk holds no file of the next window)
