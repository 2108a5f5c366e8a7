// file_format_main.cpp -- rph_file_format (rupphash_amd/csrc/file_format.cpp) as a stand-alone host program, built with
// -fsanitize=address,undefined from that one source file (tests/test_files_cpu.py builds and runs it).  Every input lives in a heap block
// of exactly its size, so a read past the bytes or past a name's terminator is reported.  Exit status 0 and "ok" when every case holds.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/rupphash.h"

static int failures = 0;

// the function on copies of exactly len bytes and exactly strlen(name) + 1 bytes
static int format_of(const std::string &bytes, const char *name)
{
    uint8_t *d = bytes.empty() ? nullptr : (uint8_t *)malloc(bytes.size());
    if (d) memcpy(d, bytes.data(), bytes.size());
    char *nm = nullptr;
    if (name) {
        nm = (char *)malloc(strlen(name) + 1);
        memcpy(nm, name, strlen(name) + 1);
    }
    const int f = rph_file_format(d, bytes.size(), nm);
    free(d);
    free(nm);
    return f;
}

static void expect(const std::string &bytes, const char *name, int want, const char *what)
{
    const int got = format_of(bytes, name);
    if (got != want) {
        failures++;
        printf("FAIL %s: name %s, %zu bytes: got %d, want %d\n", what, name ? name : "(null)", bytes.size(), got, want);
    }
}

static std::string upper(std::string s)
{
    for (char &c : s)
        if (c >= 'a' && c <= 'z') c = (char)(c - 'a' + 'A');
    return s;
}

static std::string mixed(std::string s)
{
    for (size_t k = 1; k < s.size(); k += 2)
        if (s[k] >= 'a' && s[k] <= 'z') s[k] = (char)(s[k] - 'a' + 'A');
    return s;
}

int main()
{
    struct Magic {
        int format;
        std::string bytes;
    };
    const std::vector<Magic> magics = {
        {RPH_FORMAT_PNG, std::string("\x89PNG\r\n\x1a\n", 8)}, {RPH_FORMAT_JPEG, std::string("\xff\xd8\xff", 3)},
        {RPH_FORMAT_GIF, "GIF87a"},                            {RPH_FORMAT_GIF, "GIF89a"},
        {RPH_FORMAT_WEBP, std::string("RIFF\x10\0\0\0WEBP", 12)}, {RPH_FORMAT_TIFF, std::string("MM\0\x2a", 4)},
        {RPH_FORMAT_TIFF, std::string("II\x2a\0", 4)},         {RPH_FORMAT_BMP, "BM"},
    };
    // every magic exactly, with bytes behind it, and every proper prefix of it (the empty one included)
    for (const Magic &m : magics) {
        expect(m.bytes, nullptr, m.format, "magic");
        expect(m.bytes + std::string(40, '\0'), "a.bin", m.format, "magic and more");
        for (size_t n = 0; n < m.bytes.size(); n++) {
            // (a prefix of one magic is no other format's whole magic: "BM" and "MM" / "II" share no start)
            expect(m.bytes.substr(0, n), nullptr, RPH_FORMAT_NONE, "prefix of a magic");
            expect(m.bytes.substr(0, n), "a.png", RPH_FORMAT_NONE, "prefix of a magic, named");
        }
    }
    expect(std::string("RIFF\x10\0\0\0WAVE", 12), nullptr, RPH_FORMAT_NONE, "RIFF without WEBP");
    expect(std::string("RIFF\x10\0\0\0WEB", 11), nullptr, RPH_FORMAT_NONE, "WEBP cut at 11 bytes");
    expect(std::string("II+\0\x08\0\0\0", 8), "a.tif", RPH_FORMAT_NONE, "BigTIFF");
    expect(std::string("MM\0+\0\x08\0\0", 8), "a.tif", RPH_FORMAT_NONE, "BigTIFF, big-endian");
    for (size_t n = 0; n <= 3; n++) expect(std::string("\0\1\2", 3).substr(0, n), nullptr, RPH_FORMAT_NONE, "lengths 0 to 3");
    expect("hello, world", "a.jpg", RPH_FORMAT_NONE, "a known extension over an unknown magic");

    const std::string png = magics[0].bytes + std::string(24, '\0');
    const char *const ruled_out[] = {"nef", "dng", "cr2", "cr3", "arw", "orf", "rw2", "raf", "kdc", "dcr", "pef", "x3f", "srf", "3fr", "jxl", "pdf"};
    for (const char *e : ruled_out) {
        const std::string ext(e);
        for (const std::string &v : {ext, upper(ext), mixed(ext)}) {
            expect(png, ("a." + v).c_str(), RPH_FORMAT_NONE, "a name that rules the file out");
            expect(png, ("dir/b.c." + v).c_str(), RPH_FORMAT_NONE, "a name that rules the file out, in a directory");
        }
        expect(png, ext.c_str(), RPH_FORMAT_PNG, "no '.': no extension");
        expect(png, ("." + ext).c_str(), RPH_FORMAT_PNG, "a leading '.' alone: no extension");
        expect(png, ("a." + ext + "x").c_str(), RPH_FORMAT_PNG, "a longer extension");
        expect(png, ("a." + ext.substr(0, 2)).c_str(), RPH_FORMAT_PNG, "a shorter extension");
        expect(png, ("a." + ext + "/b").c_str(), RPH_FORMAT_PNG, "the extension of a directory");
    }
    for (const char *name : {"a.jpg", "a.tif", "a.dat", "a", ".png", "dir.jpg/a", "a.", "", "/", "..", "a/..", "a/", "."})
        expect(png, name, RPH_FORMAT_PNG, "a name that does not matter");
    expect(png, nullptr, RPH_FORMAT_PNG, "no name");

    // names up to 4 KB whose extension runs to the terminator: a long stem, a long extension, a long path, a known name at the very end
    for (size_t n : {1u, 2u, 3u, 4u, 63u, 64u, 255u, 1024u, 4095u, 4096u}) {
        expect(png, (std::string(n, 'x') + ".nef").c_str(), RPH_FORMAT_NONE, "a long stem");
        expect(png, ("a." + std::string(n, 'n')).c_str(), RPH_FORMAT_PNG, "a long extension");
        expect(png, ("a.nef" + std::string(n, 'f')).c_str(), RPH_FORMAT_PNG, "a long extension that starts like a known one");
        expect(png, (std::string(n, '/') + "a.PDF").c_str(), RPH_FORMAT_NONE, "a long path");
        expect(png, (std::string(n, '.') + "jxl").c_str(), n >= 2 ? RPH_FORMAT_NONE : RPH_FORMAT_PNG, "leading dots");
        expect(png, (std::string(n, '.')).c_str(), RPH_FORMAT_PNG, "dots alone");
    }
    if (failures) {
        printf("%d case(s) failed\n", failures);
        return 1;
    }
    printf("ok\n");
    return 0;
}
