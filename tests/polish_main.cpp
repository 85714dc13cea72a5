// The pieces fig_polish_kernel runs per (candidate, read) -- fig_polish_counted, fig_polish_shift, fig_polish_column and the band of
// fig_band.h, compiled as plain C++ -- over a case file, in the kernel's form (band_form.h's 16 "lanes" per read, the column codes of
// the EDITED sequence taken from the unedited string through fig_polish_column, the deletion sweep as repeated relaxation, forward only) and,
// beside it, a sequential restatement written out here: the edited string is built, its columns are read with the flanks moved to
// its ends, and ll_c is the greatest cell of the last row of a full matrix filled by the definition in figbird_hip.h.  The two must
// agree bit for bit: exit 4 with a message otherwise.  Then the bookkeeping of the edit planes (fig_polish_host.h) runs a script of
// insertions and removals.  Built with AddressSanitizer and UBSan by tests/test_polish.py and run directly.
//
// case file: L | lm[L] | le[L] | lt[16] | lI[L] | lD[L] | gaps, then per gap `n` | 416 flank codes as digits | the string |
// candidates, then per candidate `kind x b reads`, then per read `ostar len rev` | the sequence; then `BOOK n0 string ops` and per
// op `I y b` or `D y`.
// Output: per candidate and read `C <counted> <ll_c as 16 hex digits>` (0 for a read that is not counted); per bookkeeping op
// `B <return code> <current string> <edit words in hex ...> <edit_end>`.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <limits>
#include <string>
#include <vector>

#include "../figbird_amd/csrc/fig_polish.h"
#include "band_form.h"

static double rd(std::istream &in) { std::string t; in >> t; return strtod(t.c_str(), nullptr); }
static uint64_t bits(double v) { uint64_t u; memcpy(&u, &v, 8); return u; }
static const double NINF = -std::numeric_limits<double>::infinity();
enum { W = FIG_INDEL_W, ND = FIG_INDEL_ND };

struct Tabs { std::vector<double> lm, le, lt, lI, lD; };
struct Read { int o, len, rev; std::vector<uint32_t> w; std::vector<int> code; };

// ---- the kernel's form
static double lane_form(const Read &R, const Tabs &T, int n, const uint8_t *fl, const char *str, int kind, int x, int b) {
    const int len = R.len, oc = fig_polish_shift(R.o, kind, x);
    std::vector<uint8_t> S((size_t)len + 2 * W + 1);
    for (int i = 0; i <= len + 2 * W; i++) S[(size_t)i] = (uint8_t)fig_polish_column(oc - W + i, n, fl, str, kind, x, b);
    double h[16];
    band_form(S.data(), R.w.data(), len, R.rev, T.lm.data(), T.le.data(), T.lt.data(), T.lI.data(), T.lD.data(), h, nullptr, nullptr, nullptr);
    int d_end;
    return fig_indel_end(h, d_end);
}

// ---- the definition, sequentially, over the edited string
static double sequential(const Read &R, const Tabs &T, int n, const uint8_t *fl, const std::string &str, int kind, int x, int b) {
    std::string e = str.substr(0, (size_t)n);
    if (kind == FIG_POLISH_INS) e.insert((size_t)x, 1, "ACGT"[b]); else e.erase((size_t)x, 1);
    const int nc = (int)e.size(), len = R.len;
    const int oc = kind == FIG_POLISH_INS ? (R.o >= x ? R.o + 1 : R.o) : (R.o > x ? R.o - 1 : R.o);
    auto col = [&](int y) {
        if (y < 0) return -y <= 208 ? (int)fl[-y - 1] : 4;
        if (y >= nc) return y - nc < 208 ? (int)fl[208 + (y - nc)] : 4;
        const char c = e[(size_t)y];
        return c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : c == 'T' ? 3 : 4;
    };
    std::vector<double> H((size_t)(len + 1) * ND, 0.0);
    for (int i = 1; i <= len; i++) {
        const int j = i - 1, c4 = R.code[(size_t)j], k = R.rev ? len - 1 - j : j;
        for (int d = -W; d <= W; d++) {
            double diag = H[(size_t)(i - 1) * ND + d + W];
            if (c4 < 4) {
                const int c = col(oc + j + d);
                diag = diag + (c > 3 ? FIG_INDEL_LQ : c == c4 ? T.lm[(size_t)k] : T.le[(size_t)k] + T.lt[(size_t)(c * 4 + c4)]);
            }
            const double ins = d == W ? NINF : H[(size_t)(i - 1) * ND + d + 1 + W] + T.lI[(size_t)k];
            H[(size_t)i * ND + d + W] = diag >= ins ? diag : ins;
        }
        if (i <= len - 1)
            for (int d = -W + 1; d <= W; d++) {
                const double v = H[(size_t)i * ND + d - 1 + W] + T.lD[(size_t)k];
                if (v > H[(size_t)i * ND + d + W]) H[(size_t)i * ND + d + W] = v;
            }
    }
    double best = NINF;
    for (int d = -W; d <= W; d++) if (H[(size_t)len * ND + d + W] > best) best = H[(size_t)len * ND + d + W];
    return best;
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    std::ifstream in(argv[1]);
    if (!in) return 2;
    int L; in >> L;
    Tabs T;
    auto vec = [&](std::vector<double> &v, int n) { v.resize((size_t)n); for (int i = 0; i < n; i++) v[(size_t)i] = rd(in); };
    vec(T.lm, L); vec(T.le, L); vec(T.lt, 16); vec(T.lI, L); vec(T.lD, L);
    int ngaps; in >> ngaps;
    long long scored = 0;
    for (int g = 0; g < ngaps; g++) {
        int n, ncand; std::string fls, str;
        in >> n >> fls >> str >> ncand;
        if ((int)fls.size() != 416 || (int)str.size() != n || n < 1) return 3;
        std::vector<uint8_t> fl(416);
        for (int i = 0; i < 416; i++) fl[(size_t)i] = (uint8_t)(fls[(size_t)i] - '0');
        std::vector<char> sbuf(str.begin(), str.end());                      // exactly n bytes: a read past the string is the sanitizer's
        for (int c = 0; c < ncand; c++) {
            int kind, x, b, nreads;
            in >> kind >> x >> b >> nreads;
            if ((kind == FIG_POLISH_DEL && (x < 0 || x >= n || n < 2)) || (kind == FIG_POLISH_INS && (x < 0 || x > n)) || b < 0 || b > 3) return 3;
            for (int r = 0; r < nreads; r++) {
                Read R; std::string seq;
                in >> R.o >> R.len >> R.rev >> seq;
                const int len = R.len;
                if ((int)seq.size() != len || len < 1 || len > L) return 3;
                const int nw2 = (len + 15) >> 4, nwm = (len + 31) >> 5;
                R.w.assign((size_t)(nw2 + nwm), 0u);
                R.code.resize((size_t)len);
                for (int j = 0; j < len; j++) {
                    const char ch = seq[(size_t)j];
                    const int code = ch == 'A' ? 0 : ch == 'C' ? 1 : ch == 'G' ? 2 : ch == 'T' ? 3 : 4;
                    R.code[(size_t)j] = code;
                    if (code < 4) R.w[(size_t)(j >> 4)] |= (uint32_t)code << ((j & 15) * 2);
                    else R.w[(size_t)(nw2 + (j >> 5))] |= 1u << (j & 31);
                }
                if (!fig_polish_counted(R.o, len, n, kind, x)) { printf("C 0 %016" PRIx64 "\n", (uint64_t)0); continue; }
                const double a = lane_form(R, T, n, fl.data(), sbuf.data(), kind, x, b), s = sequential(R, T, n, fl.data(), str, kind, x, b);
                if (bits(a) != bits(s)) { fprintf(stderr, "gap %d candidate %d read %d: kernel form %a, sequential %a\n", g, c, r, a, s); return 4; }
                printf("C 1 %016" PRIx64 "\n", bits(a));
                scored++;
            }
        }
    }
    std::string tag;
    while (in >> tag) {
        if (tag != "BOOK") return 3;
        int n0, nops; std::string str;
        in >> n0 >> str >> nops;
        if ((int)str.size() != n0) return 3;
        std::vector<int32_t> edit((size_t)n0, 0);
        int32_t edit_end = 0;
        for (int i = 0; i < nops; i++) {
            std::string op; long long y; int b = 0, rc;
            in >> op >> y;
            if (op == "I") { in >> b; rc = fig_polish_insert(edit.data(), n0, &edit_end, y, b); }
            else rc = fig_polish_remove(edit.data(), n0, &edit_end, y);
            const int64_t len = fig_polish_string(edit.data(), n0, edit_end, str.data(), nullptr);
            if (len != fig_polish_length(edit.data(), n0, edit_end)) { fprintf(stderr, "length and string disagree\n"); return 4; }
            std::vector<char> cur((size_t)len);                              // exactly the length: one byte more is the sanitizer's
            fig_polish_string(edit.data(), n0, edit_end, str.data(), cur.data());
            printf("B %d %s", rc, len ? std::string(cur.begin(), cur.end()).c_str() : "-");
            for (int x = 0; x < n0; x++) printf(" %x", (unsigned)edit[(size_t)x]);
            printf(" %x\n", (unsigned)edit_end);
        }
    }
    fprintf(stderr, "scores checked: %lld\n", scored);
    return 0;
}
