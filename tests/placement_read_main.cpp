// The arithmetic fig_placement_kernel runs per (read, placement) pair -- fig_placement_column, fig_placement_isz,
// fig_placement_valid, fig_placement_score, compiled as plain C++ -- over a case file, with the kernel's reductions restated as
// one sequential loop per read.  Built with AddressSanitizer and UBSan by tests/test_read_placement.py and run directly.
//
// case file: L | e[L] | T[25] | max_insert Tmin Tmax | insd[max_insert] | gaps, then per gap
//   `n gap_start G0 reads` | 416 flank codes as digits | the string (or `-` for n = 0) | per read `ostar len rev pos sequence`
// (doubles as C99 hex floats).  Output per read whose ostar is not INT32_MIN: `ll_drawn ll_other off_other n_valid`, the doubles as
// 16 hex digits of their bits.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "../figbird_amd/csrc/fig_placement.h"

static double rd(std::istream &in) { std::string t; in >> t; return strtod(t.c_str(), nullptr); }
static uint64_t bits(double v) { uint64_t u; memcpy(&u, &v, 8); return u; }

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    std::ifstream in(argv[1]);
    if (!in) return 2;
    int L; in >> L;
    std::vector<double> e((size_t)L), ome((size_t)L), T(25), lm((size_t)L), le((size_t)L), lt(16);
    for (int k = 0; k < L; k++) { e[(size_t)k] = rd(in); volatile double a = 1 - e[(size_t)k]; ome[(size_t)k] = a; }
    for (int i = 0; i < 25; i++) T[(size_t)i] = rd(in);
    fig_quality_tables(L, e.data(), ome.data(), T.data(), lm.data(), le.data(), lt.data());
    int MI, Tmin, Tmax; in >> MI >> Tmin >> Tmax;
    std::vector<double> insd((size_t)MI), li((size_t)MI);
    for (int s = 0; s < MI; s++) insd[(size_t)s] = rd(in);
    fig_placement_li(MI, insd.data(), li.data());
    const double ninf = -std::numeric_limits<double>::infinity();
    int ngaps; in >> ngaps;
    for (int g = 0; g < ngaps; g++) {
        int n, G0, nreads; long long gap_start;
        in >> n >> gap_start >> G0 >> nreads;
        std::string fls, str; in >> fls >> str;
        if (str == "-") str.clear();
        if ((int)fls.size() != 2 * FIG_P_FLANK || (int)str.size() != n) return 3;
        std::vector<uint8_t> fl(fls.size());
        for (size_t i = 0; i < fls.size(); i++) fl[i] = (uint8_t)(fls[i] - '0');
        for (int r = 0; r < nreads; r++) {
            long long ostar_, pos; int len, rev; std::string seq;
            in >> ostar_ >> len >> rev >> pos >> seq;
            if ((int)seq.size() != len) return 3;
            if (ostar_ == INT32_MIN) continue;
            const int ostar = (int)ostar_;
            const int nw2 = (len + 15) >> 4, nwm = (len + 31) >> 5;
            std::vector<uint32_t> w((size_t)(nw2 + nwm), 0u);             // pack_read's first two sections (fig_pack.h)
            for (int j = 0; j < len; j++) {
                const char c = seq[(size_t)j];
                const int code = c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : c == 'T' ? 3 : 4;
                if (code < 4) w[(size_t)(j >> 4)] |= (uint32_t)code << ((j & 15) * 2);
                else w[(size_t)(nw2 + (j >> 5))] |= 1u << (j & 31);
            }
            double drawn = ninf, best = ninf; int off = INT32_MIN, cnt = 0;
            std::vector<uint8_t> S((size_t)len);
            for (int o = -(len - 1); o <= n - 1; o++) {
                const long long isz = fig_placement_isz(pos, gap_start, G0, n, len, o);
                if (!fig_placement_valid(isz, Tmin, Tmax, MI)) continue;
                for (int j = 0; j < len; j++) S[(size_t)j] = (uint8_t)fig_placement_column(o + j, n, fl.data(), str.data());
                const double v = fig_placement_score(li[(size_t)isz], S.data(), len, rev, w.data(), lm.data(), le.data(), lt.data());
                cnt++;
                if (o == ostar) { drawn = v; continue; }
                if (off == INT32_MIN || v > best) { best = v; off = o; }
            }
            printf("%016" PRIx64 " %016" PRIx64 " %d %d\n", bits(drawn), bits(best), off, cnt);
        }
    }
    return 0;
}
