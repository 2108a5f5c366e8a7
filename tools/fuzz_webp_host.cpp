// ASan/UBSan driver for the host half of the WebP path: every .webp file of a directory, intact and with random damage (bytes
// overwritten, truncation, bytes inserted, bits flipped inside the VP8L chunk, its first bytes edited), through container / front /
// entropy decoder / inverse transforms (rphw::decode_host).  vp8l.h is shared with the device kernel, so this is also the first line of
// defence of the device logic.  Results are not checked; the sanitizers are.
#include <dirent.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "webp_host.h"

static void run(const std::vector<uint8_t> &f)
{
    rphw::Parsed p;
    std::vector<uint8_t> px;
    if (rphw::parse(f.data(), f.size(), p) == 0 && (uint64_t)p.im.w * p.im.h > (1u << 22)) return;  // (keep the run short, not the check)
    (void)rphw::decode_host(f.data(), f.size(), p, px);
}

int main(int argc, char **argv)
{
    std::mt19937 rng(7);
    DIR *d = opendir(argv[1]);
    std::vector<std::vector<uint8_t>> files;
    while (dirent *e = readdir(d)) {
        std::string n = e->d_name;
        if (n.size() < 4 || n.substr(n.size() - 4) != "webp") continue;
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
        // the first bytes of the stream, where an edit changes the transforms, the cache and the codes
        for (int r = 0; r < rounds; r++) {
            std::vector<uint8_t> g = f;
            const int kind = rng() % 5;
            if (kind == 0) for (int k = 0; k < 1 + (int)(rng() % 6); k++) g[rng() % g.size()] = (uint8_t)rng();
            else if (kind == 1) g.resize(1 + rng() % g.size());
            else if (kind == 2) g.insert(g.begin() + rng() % g.size(), (uint8_t)rng());
            else if (kind == 3) for (int k = 0; k < 1 + (int)(rng() % 3); k++) g[8 + rng() % (g.size() - 8)] ^= (uint8_t)(1u << (rng() % 8));
            else if (g.size() > 64) for (int k = 0; k < 1 + (int)(rng() % 2); k++) g[20 + rng() % 44] = (uint8_t)rng();
            run(g);
            n++;
        }
    }
    printf("%zu files, %ld damaged variants: no sanitizer report\n", files.size(), n);
    return 0;
}
