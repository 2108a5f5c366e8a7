// file_format.cpp -- which of the six file pipelines takes a file: the routing of load_image_fast (scanner.rs:461-735) as one rule
// over a file's name and its first bytes.  Host code without a context and without HIP: it compiles alone (tests/cpp/file_format_main.cpp
// builds it under the address and undefined-behaviour sanitizers).  The rule and its derivation: include/rupphash.h (the files section),
// DESIGN.md 4.12.
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../../include/rupphash.h"

namespace {

// scanner.rs:43-46 RAW_EXTS (tests/golden/raw_exts.txt holds the list as recorded from the reference), then the two arms of
// load_image_fast that return their decoder's error without falling through
const char *const RAW_EXTS[] = {"nef", "dng", "cr2", "cr3", "arw", "orf", "rw2", "raf", "kdc", "dcr", "pef", "x3f", "srf", "3fr"};
const char *const NO_FALLTHROUGH_EXTS[] = {"jxl", "pdf"};

inline char ascii_lower(char c) { return (c >= 'A' && c <= 'Z') ? (char)(c - 'A' + 'a') : c; }

// ext[0 .. n) against a lower-case name, ASCII case-insensitively
bool ext_is(const char *ext, size_t n, const char *lower)
{
    if (strlen(lower) != n) return false;
    for (size_t i = 0; i < n; i++)
        if (ascii_lower(ext[i]) != lower[i]) return false;
    return true;
}

bool starts_with(const uint8_t *data, size_t len, const void *magic, size_t n) { return len >= n && memcmp(data, magic, n) == 0; }

}  // namespace

extern "C" {

// Rust's Path::extension on the last component after the last '/': null when the component has no '.', when its only '.' leads it, or
// when it is ".."; else the part after the last '.', which may be empty.  -> a pointer into `name`, *n_out bytes (exported for the tests,
// not in the header)
const char *rph_debug_file_extension(const char *name, size_t *n_out)
{
    if (n_out) *n_out = 0;
    if (!name) return nullptr;
    const char *slash = strrchr(name, '/');
    const char *comp = slash ? slash + 1 : name;
    if (strcmp(comp, "..") == 0) return nullptr;
    const char *dot = strrchr(comp, '.');
    if (!dot || dot == comp) return nullptr;
    if (n_out) *n_out = strlen(dot + 1);
    return dot + 1;
}

// the i-th name of the product's RAW table, null past its end (exported for the tests, not in the header)
const char *rph_debug_raw_ext(uint32_t i) { return i < sizeof(RAW_EXTS) / sizeof(RAW_EXTS[0]) ? RAW_EXTS[i] : nullptr; }

int rph_file_format(const uint8_t *data, size_t len, const char *name)
{
    // 1. the extensions whose arm never reaches the bytes' magic
    size_t n = 0;
    if (const char *ext = rph_debug_file_extension(name, &n)) {
        for (const char *raw : RAW_EXTS)
            if (ext_is(ext, n, raw)) return RPH_FORMAT_NONE;
        for (const char *e : NO_FALLTHROUGH_EXTS)
            if (ext_is(ext, n, e)) return RPH_FORMAT_NONE;
    }
    // 2. image 0.25's guess_format (restated from the published crate: PARITY UNPINNED); a file shorter than its magic matches nothing
    if (!data) return RPH_FORMAT_NONE;
    if (starts_with(data, len, "\x89PNG\r\n\x1a\n", 8)) return RPH_FORMAT_PNG;
    if (starts_with(data, len, "\xff\xd8\xff", 3)) return RPH_FORMAT_JPEG;
    if (starts_with(data, len, "GIF87a", 6) || starts_with(data, len, "GIF89a", 6)) return RPH_FORMAT_GIF;
    if (starts_with(data, len, "RIFF", 4) && len >= 12 && memcmp(data + 8, "WEBP", 4) == 0) return RPH_FORMAT_WEBP;
    if (starts_with(data, len, "MM\x00\x2a", 4) || starts_with(data, len, "II\x2a\x00", 4)) return RPH_FORMAT_TIFF;
    if (starts_with(data, len, "BM", 2)) return RPH_FORMAT_BMP;
    return RPH_FORMAT_NONE;
}

}  // extern "C"
