// The pieces the two kernels of fig_alnqual.h run -- the band of fig_band.h, fig_alnqual_walk, fig_alnqual_flat, fig_alnqual_span,
// the nibble map and fig_alnqual_add_read, compiled as plain C++ -- over a case file, in the kernels' form (band_form.h's 16
// "lanes" per read with the deletion sweep as repeated relaxation and back-pointers as two 16-bit masks per row; a map of
// FIG_ALNQ_MAPB bytes per read; per column a walk over the reads in chunks of 64, in order) and, beside it, a sequential restatement of the definition in
// figbird_hip.h written out here (a full matrix, the sweep in ascending d, the steps listed from the end and replayed forwards into
// the planes read by read).  The two must agree in every map entry, every per-read value and every plane, doubles bit for bit: exit 4
// with a message otherwise.  Built with AddressSanitizer and UBSan by tests/test_alnqual.py and run directly.
//
// case file: L | lm[L] | le[L] | lt[16] | lI[L] | lD[L] | gaps, then per gap `n reads` | the n emitted bytes | per aligned read
// `ostar len rev` | len + 14 column codes as digits (column ostar - 7 first) | the sequence (doubles as C99 hex floats, `-inf` as
// strtod reads it).
// Output per gap: per read `R ll_gapped n_ins n_del d_end d_start lo hi M`, M = the len + 14 nibbles of the map as hex digits; then
// per column `C ll[0..3] depth agree skip`; the doubles as 16 hex digits of their bits.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <limits>
#include <string>
#include <vector>

#include "../figbird_amd/csrc/fig_alnqual.h"
#include "band_form.h"

static double rd(std::istream &in) { std::string t; in >> t; return strtod(t.c_str(), nullptr); }
static uint64_t bits(double v) { uint64_t u; memcpy(&u, &v, 8); return u; }
static const double NINF = -std::numeric_limits<double>::infinity();
enum { W = FIG_INDEL_W, ND = FIG_INDEL_ND };

struct Read { int o, len, rev; std::vector<uint8_t> S; std::vector<uint32_t> w; std::vector<int> code; };   // code: 0..3, 4 = outside ACGT
struct Tabs { std::vector<double> lm, le, lt, lI, lD; };
struct Path { double gapped; int n_ins, n_del, d_end, d_start, lo, hi; std::vector<uint8_t> map; };          // map: FIG_ALNQ_MAPB bytes
struct Planes { std::vector<double> ll; std::vector<int> depth, agree, skip; };

// ---- the path kernel's form
static Path lane_form(const Read &R, const Tabs &T) {
    const int len = R.len;
    double h[16];
    std::vector<uint32_t> bpw((size_t)len, 0u);
    band_form(R.S.data(), R.w.data(), len, R.rev, T.lm.data(), T.le.data(), T.lt.data(), T.lI.data(), T.lD.data(), h, bpw.data(), nullptr, nullptr);
    Path p;
    p.map.assign((size_t)FIG_ALNQ_MAPB, 0xff);
    p.gapped = fig_indel_end(h, p.d_end);
    if (p.gapped > NINF) {
        const uint32_t *row = bpw.data();
        auto bpf = [row](int i, int d) { return fig_band_bp(row, i, d); };
        fig_alnqual_walk(bpf, p.map.data(), len, p.d_end, p.d_start, p.n_ins, p.n_del);
    } else fig_alnqual_flat(p.map.data(), len, p.d_start, p.d_end, p.n_ins, p.n_del);
    fig_alnqual_span(R.o, len, p.d_start, p.d_end, p.lo, p.hi);
    return p;
}

// ---- the column kernel's form: a column's accumulators over the reads in chunks of FIG_RS_CHUNK, in order
static Planes column_form(int n, const std::string &str, const std::vector<Read> &reads, const std::vector<Path> &paths, const Tabs &T) {
    Planes P;
    P.ll.assign((size_t)n * 4, 0.0); P.depth.assign((size_t)n, 0); P.agree.assign((size_t)n, 0); P.skip.assign((size_t)n, 0);
    for (int x = 0; x < n; x++) {
        double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
        int depth = 0, agree = 0, skip = 0;
        const int call = fig_alnqual_call_code(str[(size_t)x]);
        for (size_t c0 = 0; c0 < reads.size(); c0 += FIG_RS_CHUNK)
            for (size_t r = c0; r < reads.size() && r < c0 + FIG_RS_CHUNK; r++) {
                const Read &R = reads[r];
                const Path &p = paths[r];
                const int what = fig_alnqual_add_read(a0, a1, a2, a3, x, call, R.o, R.len, R.rev, p.lo, p.hi, R.w.data(), p.map.data(), T.lm.data(), T.le.data(), T.lt.data());
                skip += what == FIG_ALNQ_SKIP; depth += what >= FIG_ALNQ_BASE; agree += what == FIG_ALNQ_AGREE;
            }
        P.ll[(size_t)x * 4] = a0; P.ll[(size_t)x * 4 + 1] = a1; P.ll[(size_t)x * 4 + 2] = a2; P.ll[(size_t)x * 4 + 3] = a3;
        P.depth[(size_t)x] = depth; P.agree[(size_t)x] = agree; P.skip[(size_t)x] = skip;
    }
    return P;
}

// ---- the definition, sequentially: the path of one read as steps, first step first
struct Step { int kind, i, d; };
static Path sequential(const Read &R, const Tabs &T, std::vector<Step> &fwd) {
    const int len = R.len;
    std::vector<double> H((size_t)(len + 1) * ND, 0.0);
    std::vector<int> P((size_t)(len + 1) * ND, -1);
    for (int i = 1; i <= len; i++) {
        const int j = i - 1, c4 = R.code[(size_t)j], k = R.rev ? len - 1 - j : j;
        for (int d = -W; d <= W; d++) {
            double diag = H[(size_t)(i - 1) * ND + d + W];
            if (c4 < 4) {
                const int c = R.S[(size_t)(j + d + W)];
                diag = diag + (c > 3 ? FIG_INDEL_LQ : c == c4 ? T.lm[(size_t)k] : T.le[(size_t)k] + T.lt[(size_t)(c * 4 + c4)]);
            }
            const double ins = d == W ? NINF : H[(size_t)(i - 1) * ND + d + 1 + W] + T.lI[(size_t)k];
            H[(size_t)i * ND + d + W] = diag >= ins ? diag : ins;
            P[(size_t)i * ND + d + W] = diag >= ins ? FIG_ID_DIAG : FIG_ID_INS;
        }
        if (i <= len - 1)
            for (int d = -W + 1; d <= W; d++) {
                const double v = H[(size_t)i * ND + d - 1 + W] + T.lD[(size_t)k];
                if (v > H[(size_t)i * ND + d + W]) { H[(size_t)i * ND + d + W] = v; P[(size_t)i * ND + d + W] = FIG_ID_DEL; }
            }
    }
    static const int order[ND] = {0, -1, 1, -2, 2, -3, 3, -4, 4, -5, 5, -6, 6, -7, 7};
    Path p;
    p.gapped = NINF; p.d_end = 0;
    for (int t = ND - 1; t >= 0; t--) if (H[(size_t)len * ND + order[t] + W] >= p.gapped) { p.gapped = H[(size_t)len * ND + order[t] + W]; p.d_end = order[t]; }
    std::vector<Step> st;
    int d = 0;
    if (p.gapped > NINF) {
        int i = len;
        d = p.d_end;
        while (i > 0) {
            const int q = P[(size_t)i * ND + d + W];
            st.push_back({q, i, d});
            if (q == FIG_ID_DIAG) i--; else if (q == FIG_ID_INS) { i--; d++; } else d--;
        }
    } else {
        p.d_end = 0;
        for (int i = len; i > 0; i--) st.push_back({FIG_ID_DIAG, i, 0});
    }
    p.d_start = d;
    fwd.assign(st.rbegin(), st.rend());
    p.n_ins = p.n_del = 0;
    std::vector<int> nib((size_t)(len + 2 * W), FIG_ALNQ_NONE);
    for (const Step &s : fwd) {
        if (s.kind == FIG_ID_INS) p.n_ins++;
        else if (s.kind == FIG_ID_DEL) p.n_del++;
        else nib[(size_t)(s.i - 1 + s.d + W)] = s.d + W;
    }
    p.lo = R.o + p.d_start; p.hi = R.o + len - 1 + p.d_end;
    p.map.assign((size_t)FIG_ALNQ_MAPB, 0xff);
    for (int c = 0; c < len + 2 * W; c++) p.map[(size_t)(c >> 1)] = (uint8_t)((c & 1) ? (p.map[(size_t)(c >> 1)] & 0x0f) | (nib[(size_t)c] << 4) : (p.map[(size_t)(c >> 1)] & 0xf0) | nib[(size_t)c]);
    return p;
}

// the planes read by read, each read's steps forwards
static Planes sequential_planes(int n, const std::string &str, const std::vector<Read> &reads, const std::vector<std::vector<Step>> &steps, const Tabs &T) {
    Planes P;
    P.ll.assign((size_t)n * 4, 0.0); P.depth.assign((size_t)n, 0); P.agree.assign((size_t)n, 0); P.skip.assign((size_t)n, 0);
    for (size_t r = 0; r < reads.size(); r++) {
        const Read &R = reads[r];
        for (const Step &s : steps[r]) {
            if (s.kind == FIG_ID_INS) continue;
            if (s.kind == FIG_ID_DEL) { const int x = R.o + s.i + s.d - 1; if (x >= 0 && x < n) P.skip[(size_t)x]++; continue; }
            const int j = s.i - 1, x = R.o + j + s.d, c4 = R.code[(size_t)j], k = R.rev ? R.len - 1 - j : j;
            if (x < 0 || x >= n || c4 > 3) continue;
            for (int b = 0; b < 4; b++) P.ll[(size_t)x * 4 + b] = P.ll[(size_t)x * 4 + b] + (c4 == b ? T.lm[(size_t)k] : T.le[(size_t)k] + T.lt[(size_t)(b * 4 + c4)]);
            P.depth[(size_t)x]++;
            const char e = str[(size_t)x];
            if ((e == 'A' && c4 == 0) || (e == 'C' && c4 == 1) || (e == 'G' && c4 == 2) || (e == 'T' && c4 == 3)) P.agree[(size_t)x]++;
        }
    }
    return P;
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
    long long entries = 0;
    for (int g = 0; g < ngaps; g++) {
        int n, nreads; std::string str;
        in >> n >> nreads >> str;
        if (n < 1 || (int)str.size() != n) return 3;
        std::vector<Read> reads((size_t)nreads);
        std::vector<Path> pk, ps;
        std::vector<std::vector<Step>> steps((size_t)nreads);
        for (int r = 0; r < nreads; r++) {
            Read &R = reads[(size_t)r]; std::string win, seq;
            in >> R.o >> R.len >> R.rev >> win >> seq;
            const int len = R.len;
            if ((int)seq.size() != len || (int)win.size() != len + 2 * W || len < 1 || len > L || len > FIG_RS_MAXL) return 3;
            R.S.assign((size_t)len + 2 * W + 2, 4);                              // (+2: the border lane reads one code further)
            for (size_t i = 0; i < win.size(); i++) R.S[i] = (uint8_t)(win[i] - '0');
            const int nw2 = (len + 15) >> 4, nwm = (len + 31) >> 5;
            R.w.assign((size_t)(nw2 + nwm), 0u);                                 // pack_read's first two sections (fig_pack.h)
            R.code.resize((size_t)len);
            for (int j = 0; j < len; j++) {
                const char c = seq[(size_t)j];
                const int code = c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : c == 'T' ? 3 : 4;
                R.code[(size_t)j] = code;
                if (code < 4) R.w[(size_t)(j >> 4)] |= (uint32_t)code << ((j & 15) * 2);
                else R.w[(size_t)(nw2 + (j >> 5))] |= 1u << (j & 31);
            }
            pk.push_back(lane_form(R, T));
            ps.push_back(sequential(R, T, steps[(size_t)r]));
            const Path &a = pk.back(), &b = ps.back();
            if (bits(a.gapped) != bits(b.gapped) || a.n_ins != b.n_ins || a.n_del != b.n_del || a.d_end != b.d_end || a.d_start != b.d_start || a.lo != b.lo || a.hi != b.hi) {
                fprintf(stderr, "gap %d read %d: kernel form %a %d %d %d %d [%d, %d], sequential %a %d %d %d %d [%d, %d]\n", g, r, a.gapped, a.n_ins, a.n_del, a.d_end, a.d_start, a.lo, a.hi,
                        b.gapped, b.n_ins, b.n_del, b.d_end, b.d_start, b.lo, b.hi);
                return 4;
            }
            for (int c = 0; c < len + 2 * W; c++) {
                if (fig_alnqual_nibble(a.map.data(), c) != fig_alnqual_nibble(b.map.data(), c)) {
                    fprintf(stderr, "gap %d read %d window column %d: kernel form %d, sequential %d\n", g, r, c, fig_alnqual_nibble(a.map.data(), c), fig_alnqual_nibble(b.map.data(), c));
                    return 4;
                }
                entries++;
            }
            if (a.map != b.map) { fprintf(stderr, "gap %d read %d: the bytes of the map past its last nibble differ\n", g, r); return 4; }
            printf("R %016" PRIx64 " %d %d %d %d %d %d ", bits(a.gapped), a.n_ins, a.n_del, a.d_end, a.d_start, a.lo, a.hi);
            for (int c = 0; c < len + 2 * W; c++) printf("%x", fig_alnqual_nibble(a.map.data(), c));
            printf("\n");
        }
        const Planes A = column_form(n, str, reads, pk, T), B = sequential_planes(n, str, reads, steps, T);
        for (int x = 0; x < n; x++) {
            bool same = A.depth[(size_t)x] == B.depth[(size_t)x] && A.agree[(size_t)x] == B.agree[(size_t)x] && A.skip[(size_t)x] == B.skip[(size_t)x];
            for (int b = 0; b < 4; b++) same = same && bits(A.ll[(size_t)x * 4 + b]) == bits(B.ll[(size_t)x * 4 + b]);
            if (!same) { fprintf(stderr, "gap %d column %d: the column walk and the read-by-read replay differ\n", g, x); return 4; }
            printf("C %016" PRIx64 " %016" PRIx64 " %016" PRIx64 " %016" PRIx64 " %d %d %d\n", bits(A.ll[(size_t)x * 4]), bits(A.ll[(size_t)x * 4 + 1]), bits(A.ll[(size_t)x * 4 + 2]),
                   bits(A.ll[(size_t)x * 4 + 3]), A.depth[(size_t)x], A.agree[(size_t)x], A.skip[(size_t)x]);
        }
    }
    fprintf(stderr, "map entries checked: %lld\n", entries);
    return 0;
}
