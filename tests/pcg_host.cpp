// pcg!'s scalar steps (waterlily_amd/csrc/wl_pcg_scalars.h) driven on the host: no HIP, no GPU.  Reads a script -- one
// pcg! call per line: `f32 xdef want_r2 it v0 v1 ... v(2*it)`, the dot products in the order the kernels produce them
// (r.z ; then z.eps and r.z' per iteration, r.r after the last) -- drives a PcgS through
// after_init -> (after_mult -> after_update)* -> after_last exactly as op_pcg enqueues them (every step of every iteration
// runs, exits only clear `active`) and prints the state after each step with hexadecimal floats.
// tests/test_pcg_scalars_cpu.py builds this under the address and undefined-behaviour sanitizers and checks every field.
#include <cfloat>
#include <cstdio>
#include <sstream>
#include <string>
#include <vector>

#include "wl_pcg_scalars.h"

static void show(const char *step, const wl::PcgS &s) {
    std::printf("%s %a %a %a %a %d %d %d %d\n", step, s.rho, s.alpha, s.beta, s.r2, s.active, s.xpend, s.nupd, s.r2_valid);
}

int main(int argc, char **argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: pcg_host script\n"); return 2; }
    std::FILE *f = std::fopen(argv[1], "r");
    if (!f) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    std::string text;
    char buf[4096];
    for (size_t n; (n = std::fread(buf, 1, sizeof buf, f)) > 0;) text.append(buf, n);
    std::fclose(f);
    std::istringstream lines(text);
    std::string line;
    int ncase = 0;
    while (std::getline(lines, line)) {
        if (line.empty()) continue;
        std::istringstream in(line);
        int f32, xdef, want_r2, it;
        if (!(in >> f32 >> xdef >> want_r2 >> it) || it < 1) { std::fprintf(stderr, "bad line: %s\n", line.c_str()); return 2; }
        std::vector<double> v;
        for (std::string tok; in >> tok;) v.push_back(std::stod(tok));
        if ((int)v.size() != 1 + 2 * it) { std::fprintf(stderr, "line needs %d values: %s\n", 1 + 2 * it, line.c_str()); return 2; }
        const double eps10 = f32 ? (double)(10.0f * FLT_EPSILON) : 10.0 * DBL_EPSILON;   // (T)10 * eps(T), as op_pcg passes it
        std::printf("case %d\n", ncase++);
        wl::PcgS s;
        s.rho = s.alpha = s.beta = s.r2 = -7.0;   // (a pcg! call starts from whatever the call before left)
        s.active = s.xpend = s.nupd = s.r2_valid = 7;
        wl::pcg_after_init(s, v[0], eps10, f32);
        show("init", s);
        for (int n = 1; n <= it; ++n) {
            const bool last = (n == it);
            const bool xnow = last || !xdef;
            wl::pcg_after_mult(s, v[2 * n - 1], f32);
            show("mult", s);
            if (last) wl::pcg_after_last(s, v[2 * n], f32, want_r2 != 0);
            else wl::pcg_after_update(s, v[2 * n], eps10, f32, xnow);
            show(last ? "last" : "update", s);
        }
    }
    std::printf("pcg_host ok\n");
    return 0;
}
