// ASan/UBSan driver for the host half of the BMP path: every .bmp file of a directory (python tests/bmp_streams.py DIR dumps the valid,
// the Pillow and the damaged corpus) through parse / stage / decode_host (bmp_host.cpp); for the files named behind the rounds also
// every prefix and `rounds` single-byte mutations.  Results are not checked beyond "a file that parses decodes"; the sanitizers are.
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I rupphash_amd/csrc tools/fuzz_bmp_host.cpp \
//         rupphash_amd/csrc/bmp_host.cpp -o fuzz_bmp_host && ./fuzz_bmp_host DIR [rounds [name ...]]
#include <dirent.h>

#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

#include "bmp_host.h"

static int run(const std::vector<uint8_t> &f)
{
    // (an exact-size copy, so that a read past the end is a read past the allocation)
    std::vector<uint8_t> g(f.begin(), f.end());
    g.shrink_to_fit();
    rphb::Parsed p;
    if (rphb::parse(g.data(), g.size(), p) != 0) return 0;
    if ((uint64_t)p.im.w * p.im.h > (1u << 22)) return 0;  // (keep the run short, not the check)
    std::vector<uint8_t> staged((size_t)p.im.src_stride * p.im.h), px;
    rphb::stage(g.data(), p, staged.data());
    rphb::Parsed q;
    if (rphb::decode_host(g.data(), g.size(), q, px) != 0 || px.size() != (size_t)p.im.w * p.im.h * p.im.out_ch) {
        printf("a file that parses does not decode\n");
        return 1;
    }
    return 0;
}

int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    std::mt19937 rng(7);
    DIR *d = opendir(argv[1]);
    if (!d) return 2;
    std::vector<std::pair<std::string, std::vector<uint8_t>>> files;
    while (dirent *e = readdir(d)) {
        std::string n = e->d_name;
        if (n.size() < 4 || n.substr(n.size() - 4) != ".bmp") continue;
        FILE *fp = fopen((std::string(argv[1]) + "/" + n).c_str(), "rb");
        if (!fp) return 2;
        std::vector<uint8_t> b;
        uint8_t buf[65536];
        size_t g;
        while ((g = fread(buf, 1, sizeof buf, fp)) > 0) b.insert(b.end(), buf, buf + g);
        fclose(fp);
        files.emplace_back(n.substr(0, n.size() - 4), b);
    }
    closedir(d);
    const int rounds = argc > 2 ? atoi(argv[2]) : 300;
    long n = 0, named = 0;
    for (auto &nf : files) {
        const std::vector<uint8_t> &f = nf.second;
        if (run(f)) return 1;
        bool small = false;
        for (int a = 3; a < argc; a++) small = small || nf.first == argv[a];
        if (!small) continue;
        named++;
        for (size_t cut = 0; cut < f.size(); cut++, n++)
            if (run(std::vector<uint8_t>(f.begin(), f.begin() + cut))) return 1;
        for (int r = 0; r < rounds; r++, n++) {
            std::vector<uint8_t> g = f;
            g[rng() % g.size()] = (uint8_t)rng();
            if (run(g)) return 1;
        }
    }
    if (named != argc - 3 && argc > 3) {
        printf("a named file is missing\n");
        return 1;
    }
    printf("%zu files, %ld prefixes and mutations of %ld: no sanitizer report\n", files.size(), n, named);
    return 0;
}
