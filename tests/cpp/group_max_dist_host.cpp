// group_max_dist_host FILE -- rupphash::scanner::groups_max_dist_host (include/rupphash.hpp) on files, groups and pivots that
// tests/test_group_max_dist_cpu.py wrote, one max_dist per group printed on one line.  Needs no device.
//   FILE: u32 n_files, u32 n_groups, u32 with_pivots; per file u8 has_hash, u8 has_features, 32 hash bytes, 256 f32 coefficients;
//   per group u32 count and its members (u32, indices into the files); with_pivots: per group i64, -1 = none
#include <cstdio>
#include <fstream>

#include "rupphash.hpp"

template <class T>
static T get(std::ifstream &in)
{
    T v{};
    in.read(reinterpret_cast<char *>(&v), sizeof v);
    return v;
}

int main(int argc, char **argv)
{
    if (argc != 2) return 2;
    std::ifstream in(argv[1], std::ios::binary);
    const uint32_t n = get<uint32_t>(in), n_groups = get<uint32_t>(in), with_pivots = get<uint32_t>(in);
    std::vector<rupphash::scanner::ScannedFile> files(n);
    for (auto &f : files) {
        const uint8_t has_hash = get<uint8_t>(in), has_features = get<uint8_t>(in);
        const auto hash = get<rupphash::hamminghash::Hash256>(in);
        const auto coefficients = get<std::array<float, 256>>(in);
        if (has_hash) f.pdqhash = hash;
        if (has_features) f.pdq_features = rupphash::pdqhash::PdqFeatures{coefficients};
    }
    std::vector<std::vector<uint32_t>> groups(n_groups);
    for (auto &g : groups) {
        g.resize(get<uint32_t>(in));
        for (auto &m : g) m = get<uint32_t>(in);
    }
    std::optional<std::vector<std::optional<uint32_t>>> pivots;
    if (with_pivots) {
        pivots.emplace(n_groups);
        for (auto &p : *pivots) {
            const int64_t v = get<int64_t>(in);
            if (v >= 0) p = (uint32_t)v;
        }
    }
    if (!in) return 3;
    for (uint32_t d : rupphash::scanner::groups_max_dist_host(files, groups, pivots)) std::printf("%u ", d);
    std::printf("\n");
    return 0;
}
