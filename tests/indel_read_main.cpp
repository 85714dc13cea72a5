// The pieces fig_indel_kernel runs per read -- fig_indel_term, fig_indel_cell, fig_indel_relax, fig_indel_end, fig_indel_traceback,
// compiled as plain C++ -- over a case file, in the kernel's form (band_form.h's 16 "lanes" per read: the update from the lane
// above, the deletion sweep as repeated relaxation of all diagonals until none rises, back-pointers as two 16-bit masks per row) and, beside it, a
// sequential restatement of the definition in figbird_hip.h written out here (a full matrix, the sweep in ascending d, a traceback
// that lists steps first and normalises afterwards).  The two must agree bit for bit in every cell, pointer and output: exit 4
// with a message otherwise.  Built with AddressSanitizer and UBSan by tests/test_indel_evidence.py and run directly.
//
// case file: L | lm[L] | le[L] | lt[16] | lI[L] | lD[L] | reads, then per read `ostar len rev` | len + 14 column codes as digits
// (column ostar - 7 first) | the sequence (doubles as C99 hex floats, `-inf` as strtod reads it).
// Output per read: `ll_flat ll_gapped n_ins n_del d_end d_start E`, the doubles as 16 hex digits of their bits, E = the events as
// `I<x>` / `D<x>+<m>` joined by commas in path order from the end (or `-`).
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <limits>
#include <string>
#include <vector>

#include "../figbird_amd/csrc/fig_indel.h"
#include "band_form.h"

static double rd(std::istream &in) { std::string t; in >> t; return strtod(t.c_str(), nullptr); }
static uint64_t bits(double v) { uint64_t u; memcpy(&u, &v, 8); return u; }
static const double NINF = -std::numeric_limits<double>::infinity();
enum { W = FIG_INDEL_W, ND = FIG_INDEL_ND };

struct Events {
    std::string text;
    void ins(int x) { text += (text.empty() ? "I" : ",I") + std::to_string(x); }
    void del(int x, int m) { text += (text.empty() ? "D" : ",D") + std::to_string(x) + "+" + std::to_string(m); }
};

struct Out { double flat, gapped; int n_ins, n_del, d_end, d_start; std::string ev; };

struct Read { int o, len, rev; std::vector<uint8_t> S; std::vector<uint32_t> w; std::vector<int> code; };   // code: 0..3, 4 = outside ACGT

struct Tabs { std::vector<double> lm, le, lt, lI, lD; };

// ---- the kernel's form
static Out lane_form(const Read &R, const Tabs &T, std::vector<double> &Hall, std::vector<uint32_t> &bpw) {
    const int len = R.len;
    double h[16], flat;
    bpw.assign((size_t)len, 0u);
    Hall.assign((size_t)(len + 1) * ND, 0.0);
    band_form(R.S.data(), R.w.data(), len, R.rev, T.lm.data(), T.le.data(), T.lt.data(), T.lI.data(), T.lD.data(), h, bpw.data(), &flat, Hall.data());
    Out o; o.flat = flat;
    o.gapped = fig_indel_end(h, o.d_end);
    o.n_ins = o.n_del = 0; o.d_start = 0;
    if (o.gapped > NINF) {
        Events ev;
        const uint32_t *row = bpw.data();
        auto bpf = [row](int i, int d) { return fig_band_bp(row, i, d); };
        fig_indel_traceback(bpf, R.S.data(), R.w.data(), len, R.rev, R.o, o.d_end, ev, o.d_start, o.n_ins, o.n_del);
        o.ev = ev.text;
    } else o.d_end = 0;
    return o;
}

// ---- the definition, sequentially
static Out sequential(const Read &R, const Tabs &T, std::vector<double> &H, std::vector<int> &P) {
    const int len = R.len;
    H.assign((size_t)(len + 1) * ND, 0.0);
    P.assign((size_t)(len + 1) * ND, -1);
    double flat = 0.0;
    for (int i = 1; i <= len; i++) {
        const int j = i - 1, c4 = R.code[(size_t)j], k = R.rev ? len - 1 - j : j;
        for (int d = -W; d <= W; d++) {
            double diag = H[(size_t)(i - 1) * ND + d + W];
            if (c4 < 4) {
                const int c = R.S[(size_t)(j + d + W)];
                const double t = c > 3 ? FIG_INDEL_LQ : c == c4 ? T.lm[(size_t)k] : T.le[(size_t)k] + T.lt[(size_t)(c * 4 + c4)];
                diag = diag + t;
                if (d == 0) flat = flat + t;
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
    Out o; o.flat = flat;
    static const int order[ND] = {0, -1, 1, -2, 2, -3, 3, -4, 4, -5, 5, -6, 6, -7, 7};
    o.gapped = NINF; o.d_end = 0;
    for (int t = ND - 1; t >= 0; t--) if (H[(size_t)len * ND + order[t] + W] >= o.gapped) { o.gapped = H[(size_t)len * ND + order[t] + W]; o.d_end = order[t]; }
    o.n_ins = o.n_del = 0; o.d_start = 0;
    if (!(o.gapped > NINF)) { o.d_end = 0; return o; }
    // the steps of the path, last first: {kind, i, d} of the cell the step ENDS in
    struct Step { int kind, i, d; };
    std::vector<Step> st;
    int i = len, d = o.d_end;
    while (i > 0) {
        const int p = P[(size_t)i * ND + d + W];
        st.push_back({p, i, d});
        if (p == FIG_ID_DIAG) i--; else if (p == FIG_ID_INS) { i--; d++; } else d--;
    }
    o.d_start = d;
    Events ev;
    long long last_ins = INT64_MIN;
    for (size_t a = 0; a < st.size();) {
        if (st[a].kind == FIG_ID_DIAG) { a++; continue; }
        size_t b = a;
        while (b < st.size() && st[b].kind == st[a].kind) b++;
        const int m = (int)(b - a);
        // the run is steps a .. b-1 (backwards); what precedes it on the path is steps b, b+1, ...
        if (st[a].kind == FIG_ID_INS) {
            o.n_ins += m;
            int i0 = st[b - 1].i - 1;                                    // first inserted base
            int x = R.o + st[a].i + st[a].d;                             // next column after the run
            size_t p = b;
            while (p < st.size() && st[p].kind == FIG_ID_DIAG && R.code[(size_t)(i0 - 1)] == R.code[(size_t)(i0 + m - 1)]) { i0--; x--; p++; }
            if (x != last_ins) ev.ins(x);
            last_ins = x;
        } else {
            o.n_del += m;
            int x = R.o + st[b - 1].i + st[b - 1].d - 1;                 // first deleted column: the next column of the cell before the run
            size_t p = b;
            while (p < st.size() && st[p].kind == FIG_ID_DIAG && R.S[(size_t)(x - 1 - R.o + W)] == R.S[(size_t)(x + m - 1 - R.o + W)]) { x--; p++; }
            ev.del(x, m);
        }
        a = b;
    }
    o.ev = ev.text;
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
    int nreads; in >> nreads;
    long long rounds_checked = 0;
    for (int r = 0; r < nreads; r++) {
        Read R; std::string win, seq;
        in >> R.o >> R.len >> R.rev >> win >> seq;
        const int len = R.len;
        if ((int)seq.size() != len || (int)win.size() != len + 2 * W || len < 1 || len > L) return 3;
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
        std::vector<double> Hk, Hs; std::vector<uint32_t> bpw; std::vector<int> Ps;
        const Out a = lane_form(R, T, Hk, bpw), b = sequential(R, T, Hs, Ps);
        // every cell and pointer of the repeated-relaxation form against the sequential sweep, bit for bit
        for (int i = 1; i <= len; i++)
            for (int q = 0; q < ND; q++) {
                const uint32_t v = bpw[(size_t)(i - 1)] >> q;                // (this check's own decode, not fig_band_bp)
                const int p = (v & 1u) ? FIG_ID_INS : (v & 0x10000u) ? FIG_ID_DEL : FIG_ID_DIAG;
                if (bits(Hk[(size_t)i * ND + q]) != bits(Hs[(size_t)i * ND + q]) || p != Ps[(size_t)i * ND + q]) {
                    fprintf(stderr, "read %d cell (%d, %d): kernel form %a / %d, sequential %a / %d\n", r, i, q - W, Hk[(size_t)i * ND + q], p, Hs[(size_t)i * ND + q], Ps[(size_t)i * ND + q]);
                    return 4;
                }
                rounds_checked++;
            }
        if (bits(a.flat) != bits(b.flat) || bits(a.gapped) != bits(b.gapped) || a.n_ins != b.n_ins || a.n_del != b.n_del || a.d_end != b.d_end ||
            a.d_start != b.d_start || a.ev != b.ev) {
            fprintf(stderr, "read %d: kernel form %a %a %d %d %d %d %s, sequential %a %a %d %d %d %d %s\n", r, a.flat, a.gapped, a.n_ins, a.n_del, a.d_end, a.d_start, a.ev.c_str(),
                    b.flat, b.gapped, b.n_ins, b.n_del, b.d_end, b.d_start, b.ev.c_str());
            return 4;
        }
        if (!(a.gapped >= a.flat)) { fprintf(stderr, "read %d: ll_gapped < ll_flat\n", r); return 4; }
        printf("%016" PRIx64 " %016" PRIx64 " %d %d %d %d %s\n", bits(a.flat), bits(a.gapped), a.n_ins, a.n_del, a.d_end, a.d_start, a.ev.empty() ? "-" : a.ev.c_str());
    }
    fprintf(stderr, "cells checked: %lld\n", rounds_checked);
    return 0;
}
