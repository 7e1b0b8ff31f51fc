// The tile map of the z-marching launches (waterlily_amd/csrc/wl_tilemap.h) driven on the host: no HIP, no GPU.  Reads a
// script -- one launch shape per line: `nblk tpp` -- and prints, for each of the four variants (map: 0 = contiguous, i.e.
// tile_of is handed tpp = 0, 1 = dealt, handed tpp; rev: 0 / 1), a header line `case nblk tpp map rev dealt` (dealt: what
// tilemap_dealt answers for the tpp handed over), then `lb` and `slot` lines with tile_of's two results for every physical
// workgroup b = 0..nblk-1, and a `tslot` line with tile_slot(lb) for every logical tile.
// tests/test_tilemap_cpu.py builds this under the address and undefined-behaviour sanitizers and checks every property.
#include <cstdio>
#include <sstream>
#include <string>
#include <vector>

#include "wl_tilemap.h"

static void row(const char *name, const std::vector<int> &v) {
    std::fputs(name, stdout);
    for (int x : v) std::printf(" %d", x);
    std::fputc('\n', stdout);
}

int main(int argc, char **argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: tilemap_host script\n"); return 2; }
    std::FILE *f = std::fopen(argv[1], "r");
    if (!f) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    std::string text;
    char buf[4096];
    for (size_t n; (n = std::fread(buf, 1, sizeof buf, f)) > 0;) text.append(buf, n);
    std::fclose(f);
    std::istringstream lines(text);
    std::string line;
    while (std::getline(lines, line)) {
        if (line.empty()) continue;
        std::istringstream in(line);
        int nblk, tpp;
        if (!(in >> nblk >> tpp) || nblk < 1 || tpp < 1) { std::fprintf(stderr, "bad line: %s\n", line.c_str()); return 2; }
        for (int map = 0; map < 2; ++map) {
            for (int rev = 0; rev < 2; ++rev) {
                const int mtpp = map ? tpp : 0;
                std::printf("case %d %d %d %d %d\n", nblk, tpp, map, rev, (int)wl::tilemap_dealt(nblk, mtpp));
                std::vector<int> lb(nblk), slot(nblk), tslot(nblk);
                for (int b = 0; b < nblk; ++b) {
                    lb[b] = slot[b] = -1;
                    wl::tile_of(b, nblk, mtpp, rev, lb[b], slot[b]);
                    tslot[b] = wl::tile_slot(b, nblk);
                }
                row("lb", lb);
                row("slot", slot);
                row("tslot", tslot);
            }
        }
    }
    std::printf("tilemap_host ok\n");
    return 0;
}
