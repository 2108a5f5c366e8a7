// ASan/UBSan driver for the host half of the PNG path: every .png file of a directory, intact and with random damage (bytes
// overwritten, truncation, bytes inserted, bits flipped inside the zlib stream with the chunk CRC repaired), through parse / inflate /
// unfilter / expand (rphp::decode_host).  Results are not checked; the sanitizers are.
#include <dirent.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "png_host.h"

static void run(const std::vector<uint8_t> &f)
{
    rphp::Parsed p;
    std::vector<uint8_t> px;
    if (rphp::parse(f.data(), f.size(), p) == 0 && (uint64_t)p.im.w * p.im.h > (1u << 22)) return;  // (keep the run short, not the check)
    (void)rphp::decode_host(f.data(), f.size(), p, px);
}

static void recrc_idat(std::vector<uint8_t> &g, std::mt19937 &rng)
{
    size_t pos = 8;
    while (pos + 12 <= g.size()) {
        const uint32_t n = ((uint32_t)g[pos] << 24) | ((uint32_t)g[pos + 1] << 16) | ((uint32_t)g[pos + 2] << 8) | g[pos + 3];
        if (n > g.size() - pos - 12) return;
        if (memcmp(&g[pos + 4], "IDAT", 4) == 0 && n) {
            g[pos + 8 + rng() % n] ^= (uint8_t)(1u << (rng() % 8));
            const uint32_t c = rphp::crc32(&g[pos + 4], (size_t)n + 4);
            for (int k = 0; k < 4; k++) g[pos + 8 + n + k] = (uint8_t)(c >> (24 - 8 * k));
            return;
        }
        pos += (size_t)n + 12;
    }
}

int main(int argc, char **argv)
{
    std::mt19937 rng(7);
    DIR *d = opendir(argv[1]);
    std::vector<std::vector<uint8_t>> files;
    while (dirent *e = readdir(d)) {
        std::string n = e->d_name;
        if (n.size() < 4 || n.substr(n.size() - 4) != ".png") continue;
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
        for (int r = 0; r < rounds; r++) {
            std::vector<uint8_t> g = f;
            const int kind = rng() % 4;
            if (kind == 0) for (int k = 0; k < 1 + (int)(rng() % 6); k++) g[rng() % g.size()] = (uint8_t)rng();
            else if (kind == 1) g.resize(1 + rng() % g.size());
            else if (kind == 2) g.insert(g.begin() + rng() % g.size(), (uint8_t)rng());
            else for (int k = 0; k < 1 + (int)(rng() % 3); k++) recrc_idat(g, rng);
            run(g);
            n++;
        }
    }
    printf("%zu files, %ld damaged variants: no sanitizer report\n", files.size(), n);
    return 0;
}
