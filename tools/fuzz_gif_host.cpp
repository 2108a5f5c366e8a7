// ASan/UBSan driver for the host half of the GIF path: every .gif file of a directory (python tests/gif_streams.py DIR dumps the valid
// and the damaged corpus), intact and with random damage (bytes overwritten, truncation, bytes inserted, bits flipped behind the
// header, descriptor bytes edited), through parse / join / LZW / expansion (rphg::decode_host).  Results are not checked; the
// sanitizers are.
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I rupphash_amd/csrc tools/fuzz_gif_host.cpp \
//         rupphash_amd/csrc/gif_host.cpp -o fuzz_gif_host && ./fuzz_gif_host DIR [rounds]
#include <dirent.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "gif_host.h"

static void run(const std::vector<uint8_t> &f)
{
    rphg::Parsed p;
    std::vector<uint8_t> px;
    if (rphg::parse(f.data(), f.size(), p) == 0 && ((uint64_t)p.im.w * p.im.h > (1u << 22) || (uint64_t)p.im.fw * p.im.fh > (1u << 22))) return;  // (keep the run short, not the check)
    (void)rphg::decode_host(f.data(), f.size(), p, px);
}

int main(int argc, char **argv)
{
    std::mt19937 rng(7);
    DIR *d = opendir(argv[1]);
    std::vector<std::vector<uint8_t>> files;
    while (dirent *e = readdir(d)) {
        std::string n = e->d_name;
        if (n.size() < 4 || n.substr(n.size() - 4) != ".gif") continue;
        FILE *fp = fopen((std::string(argv[1]) + "/" + n).c_str(), "rb");
        std::vector<uint8_t> b;
        uint8_t buf[65536];
        size_t g;
        while ((g = fread(buf, 1, sizeof buf, fp)) > 0) b.insert(b.end(), buf, buf + g);
        fclose(fp);
        files.push_back(b);
    }
    closedir(d);
    const int rounds = argc > 2 ? atoi(argv[2]) : 200;
    long n = 0;
    for (auto &f : files) {
        run(f);
        if (f.size() < 16) continue;
        const size_t ifd = 6;  // the screen descriptor and the 60 bytes behind it: an edit there changes sizes, flags, tables, descriptors
        for (int r = 0; r < rounds; r++) {
            std::vector<uint8_t> g = f;
            const int kind = rng() % 5;
            if (kind == 0) for (int k = 0; k < 1 + (int)(rng() % 6); k++) g[rng() % g.size()] = (uint8_t)rng();
            else if (kind == 1) g.resize(1 + rng() % g.size());
            else if (kind == 2) g.insert(g.begin() + rng() % g.size(), (uint8_t)rng());
            else if (kind == 3) for (int k = 0; k < 1 + (int)(rng() % 3); k++) g[8 + rng() % (g.size() - 8)] ^= (uint8_t)(1u << (rng() % 8));
            else if (ifd < g.size()) for (int k = 0; k < 1 + (int)(rng() % 2); k++) g[ifd + rng() % std::min<size_t>(g.size() - ifd, 60)] = (uint8_t)rng();
            run(g);
            n++;
        }
    }
    printf("%zu files, %ld damaged variants: no sanitizer report\n", files.size(), n);
    return 0;
}
