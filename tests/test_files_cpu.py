"""The routing rule of the mixed-file call on the host (no GPU): rph_file_format over a table of magics, near misses and names, its
extension extractor against a Python statement of Rust's Path::extension, the product's RAW table against the names recorded from the
reference (tests/golden/raw_exts.txt), and the function alone under the address and undefined-behaviour sanitizers in a stand-alone
program (tests/cpp/file_format_main.cpp)."""
import ctypes as C
import os
import subprocess

import files_mix as fm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_file_format_table():
    from rupphash_amd import Engine, _lib

    table = fm.format_table()
    assert len(table) > 200
    for data, name, want in table:
        assert Engine.file_format(data, name) == want, (data[:16], name, want)
        if name is not None:  # bytes and str names alike
            assert Engine.file_format(data, name.encode()) == want
    # no bytes at all
    L = _lib.load()
    assert L.rph_file_format(None, 0, None) == fm.NONE and L.rph_file_format(None, 0, b"a.png") == fm.NONE
    assert (_lib.RPH_FORMAT_NONE, _lib.RPH_FORMAT_JPEG, _lib.RPH_FORMAT_PNG, _lib.RPH_FORMAT_TIFF, _lib.RPH_FORMAT_WEBP, _lib.RPH_FORMAT_GIF,
            _lib.RPH_FORMAT_BMP) == (fm.NONE, fm.JPEG, fm.PNG, fm.TIFF, fm.WEBP, fm.GIF, fm.BMP) == tuple(range(7))


def test_every_format_is_ruled_out_by_name_and_found_by_magic():
    """the table's name cases over PNG bytes hold over every other format's magic too"""
    from rupphash_amd import Engine

    for fmt, magics in fm.MAGIC.items():
        for m in magics:
            data = m + b"\x00" * 30
            for ext in fm.raw_exts() + ["jxl", "pdf"]:
                assert Engine.file_format(data, "x." + ext.upper()) == fm.NONE
            for name in ("a.jpg", "a.png", "a.tif", "a.webp", "a.gif", "a.bmp", "a", None, "a.", ".nef", "b.nef/a"):
                assert Engine.file_format(data, name) == fmt, (fmt, name)


def test_extension_is_rusts_path_extension():
    from rupphash_amd import _lib

    L = _lib.load()
    names = list(fm.EXTENSION_NAMES) + [n for _, n, _ in fm.format_table() if n is not None]
    names += ["x" * 4095 + ".nef", "a." + "n" * 4096, "/" * 4000 + "a.b"]
    for name in names:
        raw = name.encode()
        n = C.c_size_t(77)
        p = L.rph_debug_file_extension(raw, C.byref(n))
        got = None if not p else C.string_at(p, n.value).decode()
        assert got == fm.path_extension(name), name
        assert p or n.value == 0
    assert L.rph_debug_file_extension(None, None) is None
    # the Python statement itself, on cases Rust's documentation gives: "foo.rs" -> "rs", "foo.tar.gz" -> "gz", ".bashrc" -> None
    assert [fm.path_extension(s) for s in ("foo.rs", "foo.tar.gz", ".bashrc", "foo", "foo.", "..")] == ["rs", "gz", None, None, "", None]


def test_raw_table_is_the_references():
    from rupphash_amd import _lib

    L = _lib.load()
    want = fm.raw_exts()
    assert len(want) == 14 and len(set(want)) == 14
    got = []
    while True:
        e = L.rph_debug_raw_ext(len(got))
        if e is None:
            break
        got.append(e.decode())
    assert got == want
    assert L.rph_debug_raw_ext(1 << 31) is None


def test_file_format_alone_under_sanitizers(tmp_path):
    """file_format.cpp compiles without HIP and without the rest of the library; the program runs on the host with nothing preloaded"""
    exe = str(tmp_path / "file_format_main")
    # (the sanitizers' runtimes linked statically: the program does not depend on what else the process loads)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", os.path.join(ROOT, "tests", "cpp", "file_format_main.cpp"),
                           os.path.join(ROOT, "rupphash_amd", "csrc", "file_format.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.returncode, r.stdout[-2000:], r.stderr[-2000:])


def test_corpus_routes_to_its_formats():
    """the GPU tests' corpus, as far as the host can tell: every valid and refused file goes to its format, the oddities where they belong"""
    for fi, fmt in enumerate(fm.FORMATS):
        for name, data in fm.valid(fmt):
            assert fm.file_format(data, f"{name}.{fm.ext_of(fmt)}") == fm.file_format(data, None) == fi + 1, (fmt, name)
        assert fm.file_format(fm.refused(fmt), None) == fi + 1
    files, names, misnamed = fm.mix()
    assert len(files) == 6 * fm.PER_FORMAT + 11 and names[misnamed] == "misnamed.jpg"
    assert fm.file_format(files[misnamed], names[misnamed]) == fm.PNG
    raw = names.index("raw_named.NEF")
    assert fm.file_format(files[raw], names[raw]) == fm.NONE and fm.file_format(files[raw], None) == fm.TIFF
    # the sizes the corpus promises: per format a 600 x 400 image; 16-bit and gray + alpha images for PNG and TIFF
    from rupphash_amd import Engine

    for fmt in fm.FORMATS:
        assert (600, 400) in [fm.info(fmt, d) for _, d in fm.valid(fmt)], fmt
    for fmt in ("png", "tiff"):
        layouts = {Engine._file_info(fmt, d)[2:] for _, d in fm.valid(fmt)}
        assert (3, 16) in layouts and (2, 8) in layouts, (fmt, layouts)
