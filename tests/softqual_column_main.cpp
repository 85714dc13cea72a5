// The arithmetic fig_softqual_kernel runs -- fig_softqual_mz, fig_softqual_weight and fig_softqual_add_read on top of the placement
// functions, compiled as plain C++ -- over a case file, with the kernel's phases restated as sequential loops: per gap and scored
// read the scores of all valid placements, M and Z as the library takes them from the placement pass, the row of weights over
// the offsets -(200-1) .. n-1, then every column against the row.  Built with AddressSanitizer and UBSan by
// tests/test_soft_quality.py and run directly.
//
// case file: that of tests/placement_read_main.cpp.  A second argument `dyadic` replaces the weight of valid placement o of read
// r (counted over all reads of the gap, unscored ones included) by 2^-((o + 1000 + r) % 4), or 0.0 where (o + 1000 + 2 * r) % 3
// is 0: products with a power of two are exact, so a restatement that adds in the same order gives the same bits.
// Output per gap and column: wcount[4] eloglik[4], the doubles as 16 hex digits of their bits.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "../figbird_amd/csrc/fig_softqual.h"

static double rd(std::istream &in) { std::string t; in >> t; return strtod(t.c_str(), nullptr); }
static uint64_t bits(double v) { uint64_t u; memcpy(&u, &v, 8); return u; }

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    const bool dyadic = argc > 2 && !strcmp(argv[2], "dyadic");
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
    const int first = -(FIG_RS_MAXL - 1);                         // the offset of weight index 0
    int ngaps; in >> ngaps;
    for (int g = 0; g < ngaps; g++) {
        int n, G0, nreads; long long gap_start;
        in >> n >> gap_start >> G0 >> nreads;
        std::string fls, str; in >> fls >> str;
        if (str == "-") str.clear();
        if ((int)fls.size() != 2 * FIG_P_FLANK || (int)str.size() != n) return 3;
        std::vector<uint8_t> fl(fls.size());
        for (size_t i = 0; i < fls.size(); i++) fl[i] = (uint8_t)(fls[i] - '0');
        std::vector<double> acc((size_t)n * 8, 0.0), row((size_t)(n + FIG_RS_MAXL - 1));
        for (int r = 0; r < nreads; r++) {
            long long ostar_, pos; int len, rev; std::string seq;
            in >> ostar_ >> len >> rev >> pos >> seq;
            if ((int)seq.size() != len || len > FIG_RS_MAXL) return 3;
            if (ostar_ == INT32_MIN || len == 0) continue;
            const int ostar = (int)ostar_;
            const int nw2 = (len + 15) >> 4, nwm = (len + 31) >> 5;
            std::vector<uint32_t> w((size_t)(nw2 + nwm), 0u);             // pack_read's first two sections (fig_pack.h)
            for (int j = 0; j < len; j++) {
                const char c = seq[(size_t)j];
                const int code = c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : c == 'T' ? 3 : 4;
                if (code < 4) w[(size_t)(j >> 4)] |= (uint32_t)code << ((j & 15) * 2);
                else w[(size_t)(nw2 + (j >> 5))] |= 1u << (j & 31);
            }
            // pass 1 and 2 of the placement kernel: ll_drawn, ll_other, then sum_other
            std::vector<double> lr((size_t)(n + len - 1), 0.0);
            std::vector<uint8_t> valid((size_t)(n + len - 1), 0), S((size_t)len);
            double drawn = ninf, best = ninf;
            for (int o = -(len - 1); o <= n - 1; o++) {
                const long long isz = fig_placement_isz(pos, gap_start, G0, n, len, o);
                if (!fig_placement_valid(isz, Tmin, Tmax, MI)) continue;
                for (int j = 0; j < len; j++) S[(size_t)j] = (uint8_t)fig_placement_column(o + j, n, fl.data(), str.data());
                const double v = fig_placement_score(li[(size_t)isz], S.data(), len, rev, w.data(), lm.data(), le.data(), lt.data());
                valid[(size_t)(o + len - 1)] = 1; lr[(size_t)(o + len - 1)] = v;
                if (o == ostar) drawn = v; else if (v > best) best = v;
            }
            const double Mx = drawn > best ? drawn : best;
            double sum = 0.0;
            if (Mx > ninf)
                for (int o = -(len - 1); o <= n - 1; o++)
                    if (valid[(size_t)(o + len - 1)] && o != ostar && lr[(size_t)(o + len - 1)] > ninf) sum = sum + exp10(lr[(size_t)(o + len - 1)] - Mx);
            double M, Z;
            if (!fig_softqual_mz(drawn, best, sum, M, Z)) continue;
            // phase A: the row of weights
            for (double &p : row) p = 0.0;
            for (int o = -(len - 1); o <= n - 1; o++) {
                if (!valid[(size_t)(o + len - 1)]) continue;
                double p = fig_softqual_weight(lr[(size_t)(o + len - 1)], M, Z);
                if (dyadic) p = (o + 1000 + 2 * r) % 3 == 0 ? 0.0 : 1.0 / (double)(1 << ((o + 1000 + r) % 4));
                row[(size_t)(o - first)] = p;
            }
            // phase B: every column against the row
            for (int x = 0; x < n; x++) {
                double *a = &acc[(size_t)x * 8];
                fig_softqual_add_read(a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], len, rev, w.data(), row.data(), x - first, lm.data(), le.data(), lt.data());
            }
        }
        for (int x = 0; x < n; x++) {
            for (int i = 0; i < 8; i++) printf("%016" PRIx64 "%c", bits(acc[(size_t)x * 8 + i]), i == 7 ? '\n' : ' ');
        }
    }
    return 0;
}
