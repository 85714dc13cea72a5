// The pieces fig_recruit_kernel runs per candidate read -- fig_placement_column, fig_placement_isz, fig_placement_valid,
// fig_placement_score, the slot order of fig_recruit_host.h and the band of fig_band.h, compiled as plain C++ -- over a case file, in
// the kernel's form (tiles of 256 offsets from -199, four "waves" of 64 lanes with a slot each, the butterfly maximum and the first
// lane of a ballot, two passes, then band_form.h's 16 "lanes" per read with the deletion sweep as repeated relaxation) and, beside
// it, a sequential restatement written out here: one loop over the offsets in ascending order that keeps the first strict maximum,
// the same loop over the offsets outside the window, and a full matrix filled by the definition in figbird_hip.h.  The two must agree in every output
// bit for bit: exit 4 with a message otherwise.  Built with AddressSanitizer and UBSan by tests/test_recruit.py and run directly.
//
// case file: L | lm[L] | le[L] | lt[16] | lI[L] | lD[L] | MI | li[MI] | Tmin Tmax | gaps, then per gap `n gap_start G0 reads` | 416
// flank codes as digits | the string, then per read `pos len rev` | the sequence.  Every read is a candidate.
// Output: per read `R <n_valid> <off_seed> <ll_seed> <off_second> <ll_second> <ll_flat> <ll_gapped> <d_end> <isz_seed>`, doubles as 16
// hex digits; an unseeded read prints n_valid and its ll_seed and zeros.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <limits>
#include <string>
#include <vector>

#include "../figbird_amd/csrc/fig_recruit.h"
#include "band_form.h"

static double rd(std::istream &in) { std::string t; in >> t; return strtod(t.c_str(), nullptr); }
static uint64_t bits(double v) { uint64_t u; memcpy(&u, &v, 8); return u; }
static const double NINF = -std::numeric_limits<double>::infinity();
enum { W = FIG_INDEL_W, ND = FIG_INDEL_ND, NT = FIG_RC_NT, NW = FIG_RC_WAVES };

struct Tabs { std::vector<double> lm, le, lt, lI, lD, li; int Tmin, Tmax, MI; };
struct Read { long long pos; int len, rev; std::vector<uint32_t> w; std::vector<int> code; };
struct Out { int n_valid = 0, off_seed = INT32_MIN, off_second = INT32_MIN, d_end = 0, isz_seed = 0; double ll_seed = NINF, ll_second = 0, ll_flat = 0, ll_gapped = 0; bool seeded = false; };

// ---- the kernel's form
static double wave_max(const double *v) {                                    // fig_p_wave_max over 64 lanes: what lane 0 ends with
    double a[64], b[64];
    memcpy(a, v, sizeof(a));
    for (int m = 32; m >= 1; m >>= 1) {
        for (int l = 0; l < 64; l++) { const double u = a[l ^ m]; b[l] = u > a[l] ? u : a[l]; }
        memcpy(a, b, sizeof(a));
    }
    return a[0];
}

static Out kernel_form(const Read &R, const Tabs &T, int n, long long gap_start, int G0, const uint8_t *fl, const char *str) {
    Out o;
    const int len = R.len;
    const bool left = R.pos < gap_start;
    const long long isz0 = fig_placement_isz(R.pos, gap_start, G0, n, len, 0);
    double pmax[NW][2]; int poff[NW][2], pcnt[NW];                            // [wave][stride 2]: the reduce walks them with a stride, as the kernel's [wave][read]
    int seed = INT32_MIN;
    for (int pass = 0; pass < 2; pass++) {
        for (int w = 0; w < NW; w++) { pmax[w][0] = NINF; poff[w][0] = INT32_MAX; if (pass == 0) pcnt[w] = 0; }
        for (int x0 = -(FIG_RS_MAXL - 1); x0 < n; x0 += NT) {
            std::vector<uint8_t> S((size_t)FIG_P_WIN);
            for (int i = 0; i < FIG_P_WIN; i++) S[(size_t)i] = (uint8_t)fig_placement_column(x0 + i, n, fl, str);
            for (int w = 0; w < NW; w++) {
                double v[64]; bool part[64];
                for (int l = 0; l < 64; l++) {
                    const int tid = w * 64 + l, off = x0 + tid;
                    const long long isz = left ? isz0 + off : isz0 - off;
                    const bool valid = off >= -(len - 1) && off <= n - 1 && fig_placement_valid(isz, T.Tmin, T.Tmax, T.MI);
                    part[l] = valid && (pass == 0 || fig_recruit_outside(off, seed));
                    v[l] = part[l] ? fig_placement_score(T.li[(size_t)isz], &S[(size_t)tid], len, R.rev, R.w.data(), T.lm.data(), T.le.data(), T.lt.data()) : NINF;
                }
                const double wmax = wave_max(v);
                int first = -1, cnt = 0;
                for (int l = 63; l >= 0; l--) { if (part[l]) cnt++; if (part[l] && v[l] == wmax) first = l; }
                if (pass == 0) pcnt[w] += cnt;
                fig_recruit_wave_slot(first >= 0, wmax, x0 + w * 64 + first, pmax[w][0], poff[w][0]);
            }
        }
        double m; int off;
        fig_recruit_reduce(&pmax[0][0], &poff[0][0], NW, 2, m, off);
        if (pass == 0) {
            for (int w = 0; w < NW; w++) o.n_valid += pcnt[w];
            o.ll_seed = m;
            o.seeded = fig_recruit_seeded(o.n_valid, m);
            if (!o.seeded) return o;
            o.off_seed = seed = off;
            o.isz_seed = (int)(left ? isz0 + off : isz0 - off);
        } else { o.ll_second = m; o.off_second = off == INT32_MAX ? INT32_MIN : off; }
    }
    std::vector<uint8_t> B((size_t)len + 2 * W + 1);
    for (int i = 0; i <= len + 2 * W; i++) B[(size_t)i] = (uint8_t)fig_placement_column(seed - W + i, n, fl, str);
    double h[16], flat;
    band_form(B.data(), R.w.data(), len, R.rev, T.lm.data(), T.le.data(), T.lt.data(), T.lI.data(), T.lD.data(), h, nullptr, &flat, nullptr);
    int d_end;
    o.ll_gapped = fig_indel_end(h, d_end);
    o.d_end = o.ll_gapped > NINF ? d_end : 0;
    o.ll_flat = flat;
    return o;
}

// ---- the definition, sequentially
static Out sequential(const Read &R, const Tabs &T, int n, long long gap_start, int G0, const uint8_t *fl, const std::string &str) {
    Out o;
    const int len = R.len;
    auto col = [&](int y) {
        if (y < 0) return -y <= 208 ? (int)fl[-y - 1] : 4;
        if (y >= n) return y - n < 208 ? (int)fl[208 + (y - n)] : 4;
        const char c = str[(size_t)y];
        return c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : c == 'T' ? 3 : 4;
    };
    auto term = [&](int c, int c4, int k) { return c > 3 ? FIG_INDEL_LQ : c == c4 ? T.lm[(size_t)k] : T.le[(size_t)k] + T.lt[(size_t)(c * 4 + c4)]; };
    auto isz_of = [&](int off) { return R.pos < gap_start ? gap_start - R.pos + len + off : R.pos + (n - G0) - gap_start + len - off; };
    auto Lr = [&](int off) {
        double v = T.li[(size_t)isz_of(off)];
        for (int j = 0; j < len; j++) if (R.code[(size_t)j] < 4) v = v + term(col(off + j), R.code[(size_t)j], R.rev ? len - 1 - j : j);
        return v;
    };
    auto valid = [&](int off) { const long long z = isz_of(off); return z >= T.Tmin && z <= T.Tmax && z >= 0 && z < T.MI; };
    bool have = false;
    for (int off = -(len - 1); off <= n - 1; off++) {
        if (!valid(off)) continue;
        o.n_valid++;
        const double v = Lr(off);
        if (!have || v > o.ll_seed) { o.ll_seed = v; o.off_seed = off; have = true; }
    }
    o.seeded = have && o.ll_seed > NINF;
    if (!o.seeded) { o.off_seed = INT32_MIN; if (!have) o.ll_seed = NINF; return o; }
    o.isz_seed = (int)isz_of(o.off_seed);
    have = false; o.ll_second = NINF;
    for (int off = -(len - 1); off <= n - 1; off++) {
        if (!valid(off) || abs(off - o.off_seed) <= W) continue;
        const double v = Lr(off);
        if (!have || v > o.ll_second) { o.ll_second = v; o.off_second = off; have = true; }
    }
    std::vector<double> H((size_t)(len + 1) * ND, 0.0);
    for (int i = 1; i <= len; i++) {
        const int j = i - 1, c4 = R.code[(size_t)j], k = R.rev ? len - 1 - j : j;
        for (int d = -W; d <= W; d++) {
            double diag = H[(size_t)(i - 1) * ND + d + W];
            if (c4 < 4) diag = diag + term(col(o.off_seed + j + d), c4, k);
            const double ins = d == W ? NINF : H[(size_t)(i - 1) * ND + d + 1 + W] + T.lI[(size_t)k];
            H[(size_t)i * ND + d + W] = diag >= ins ? diag : ins;
        }
        if (i <= len - 1)
            for (int d = -W + 1; d <= W; d++) {
                const double v = H[(size_t)i * ND + d - 1 + W] + T.lD[(size_t)k];
                if (v > H[(size_t)i * ND + d + W]) H[(size_t)i * ND + d + W] = v;
            }
        if (c4 < 4) o.ll_flat = o.ll_flat + term(col(o.off_seed + j), c4, k);
    }
    o.ll_gapped = H[(size_t)len * ND + W]; o.d_end = 0;
    for (int a = 1; a <= W; a++)
        for (int d : { -a, a }) if (H[(size_t)len * ND + d + W] > o.ll_gapped) { o.ll_gapped = H[(size_t)len * ND + d + W]; o.d_end = d; }
    if (!(o.ll_gapped > NINF)) o.d_end = 0;
    return o;
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    std::ifstream in(argv[1]);
    if (!in) return 2;
    int L; in >> L;
    Tabs T;
    auto vec = [&](std::vector<double> &v, int n) { v.resize((size_t)n); for (int i = 0; i < n; i++) v[(size_t)i] = rd(in); };
    vec(T.lm, L); vec(T.le, L); vec(T.lt, 16); vec(T.lI, L); vec(T.lD, L);
    in >> T.MI; vec(T.li, T.MI);
    in >> T.Tmin >> T.Tmax;
    int ngaps; in >> ngaps;
    long long checked = 0;
    for (int g = 0; g < ngaps; g++) {
        int n, G0, nreads; long long gap_start; std::string fls, str;
        in >> n >> gap_start >> G0 >> nreads >> fls >> str;
        if ((int)fls.size() != 416 || (int)str.size() != n || n < 1) return 3;
        std::vector<uint8_t> fl(416);
        for (int i = 0; i < 416; i++) fl[(size_t)i] = (uint8_t)(fls[(size_t)i] - '0');
        std::vector<char> sbuf(str.begin(), str.end());                      // exactly n bytes: a read past the string is the sanitizer's
        for (int r = 0; r < nreads; r++) {
            Read R; std::string seq;
            in >> R.pos >> R.len >> R.rev >> seq;
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
            const Out a = kernel_form(R, T, n, gap_start, G0, fl.data(), sbuf.data()), s = sequential(R, T, n, gap_start, G0, fl.data(), str);
            const bool same = a.seeded == s.seeded && a.n_valid == s.n_valid && bits(a.ll_seed) == bits(s.ll_seed) && a.off_seed == s.off_seed &&
                              (!a.seeded || (a.off_second == s.off_second && bits(a.ll_second) == bits(s.ll_second) && bits(a.ll_flat) == bits(s.ll_flat) &&
                                             bits(a.ll_gapped) == bits(s.ll_gapped) && a.d_end == s.d_end && a.isz_seed == s.isz_seed));
            if (!same) {
                fprintf(stderr, "gap %d read %d: kernel form n_valid %d seed %d %a second %d %a flat %a gapped %a d_end %d; sequential n_valid %d seed %d %a second %d %a flat %a gapped %a d_end %d\n",
                        g, r, a.n_valid, a.off_seed, a.ll_seed, a.off_second, a.ll_second, a.ll_flat, a.ll_gapped, a.d_end,
                        s.n_valid, s.off_seed, s.ll_seed, s.off_second, s.ll_second, s.ll_flat, s.ll_gapped, s.d_end);
                return 4;
            }
            if (a.seeded) printf("R %d %d %016" PRIx64 " %d %016" PRIx64 " %016" PRIx64 " %016" PRIx64 " %d %d\n", a.n_valid, a.off_seed, bits(a.ll_seed), a.off_second, bits(a.ll_second),
                                 bits(a.ll_flat), bits(a.ll_gapped), a.d_end, a.isz_seed);
            else printf("R %d %d %016" PRIx64 " %d %016" PRIx64 " %016" PRIx64 " %016" PRIx64 " %d %d\n", a.n_valid, INT32_MIN, bits(a.ll_seed), INT32_MIN, (uint64_t)0, (uint64_t)0, (uint64_t)0, 0, 0);
            checked++;
        }
    }
    fprintf(stderr, "reads checked: %lld\n", checked);
    return 0;
}
