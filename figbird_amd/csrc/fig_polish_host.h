// fig_polish_host.h -- the device-free half of the polish (fig_batch_polish, include/figbird_hip.h: fig_gap_polish):
// the offset shift, the touched and the counted rule, the listing of sites, best per site, accept and verify, the bookkeeping of
// the edit planes (locate a current cell, insert before it, remove it, apply), and the body of fig_polish_apply.  Pure C++ (no HIP,
// no engine headers): compiled into libfighip.so (fig_abi.hip; the kernel of fig_polish.h calls the marked functions on the device
// too) and into libfighost.so / figfill (host/fig_host.cpp), so that the library, the hosts and the tests share one statement of
// each rule.
#ifndef FIG_POLISH_HOST_H
#define FIG_POLISH_HOST_H
#include <cstdint>
#include "../../include/figbird_hip.h"
#include "fig_indel_host.h"

#define FIG_POLISH_DEL 0                              // kinds of a candidate
#define FIG_POLISH_INS 1
#define FIG_POLISH_MAX_K 7                            // bases one list of inserted bases holds (three bits of the edit word)

// o_c of a drawn offset o under the candidate (kind, x)
FIG_P_HD inline int32_t fig_polish_shift(int32_t o, int kind, int32_t x) {
    return kind == FIG_POLISH_INS ? (o >= x ? o + 1 : o) : (o > x ? o - 1 : o);
}

// n_c
FIG_P_HD inline int32_t fig_polish_ncol(int32_t n, int kind) { return kind == FIG_POLISH_INS ? n + 1 : n - 1; }

// A read of `len` bases drawn at o is touched by an edit at column x iff its band can see it
FIG_P_HD inline bool fig_polish_touched(int32_t o, int32_t len, int32_t x) {
    return (long long)o - (FIG_INDEL_W + 1) <= (long long)x && (long long)x <= (long long)o + len + FIG_INDEL_W;
}

// counted: scored (o is a drawn offset of a gap that is on), touched, aligned under (o, n) and under (o_c, n_c)
FIG_P_HD inline bool fig_polish_counted(int32_t o, int32_t len, int32_t n, int kind, int32_t x) {
    if (!fig_indel_aligned(o, len, n) || !fig_polish_touched(o, len, x)) return false;
    return fig_indel_aligned(fig_polish_shift(o, kind, x), len, fig_polish_ncol(n, kind));
}

// The sites of a round: the called columns in ascending order, then the right junction (x = n); at most FIG_POLISH_MAX_SITES.
// kind[i] is FIG_POLISH_DEL for a 'D' and FIG_POLISH_INS for an 'I'.  Returns how many were listed.
static inline int fig_polish_sites(const char *call, int32_t n, char call_end, int32_t *x, int32_t *kind) {
    int m = 0;
    for (int32_t c = 0; c < n && m < FIG_POLISH_MAX_SITES; c++)
        if (call[c] != '.') { x[m] = c; kind[m] = call[c] == 'D' ? FIG_POLISH_DEL : FIG_POLISH_INS; m++; }
    if (call_end != '.' && m < FIG_POLISH_MAX_SITES) { x[m] = n; kind[m] = FIG_POLISH_INS; m++; }
    return m;
}

// The best of a site's `m` candidates: the greatest T_c, ties to the first
static inline int fig_polish_best(const double *T, int m) {
    int best = 0;
    for (int i = 1; i < m; i++) if (T[i] > T[best]) best = i;
    return best;
}
static inline bool fig_polish_accept(double Tc, double T0) { return Tc > T0; }
static inline bool fig_polish_keep(double Vnew, double Vold) { return Vnew > Vold; }

// ---- the edit planes.  A word: bit 0 removed, bits 1-3 k, bits 4+2i, 5+2i the code of inserted base i.
static inline int fig_polish_k(int32_t w) { return (int)(((uint32_t)w >> 1) & 7u); }
static inline int fig_polish_base(int32_t w, int i) { return (int)(((uint32_t)w >> (4 + 2 * i)) & 3u); }
static inline int32_t fig_polish_word_insert(int32_t w, int p, int b) {          // base b at position p of the list (k < 7)
    const uint32_t u = (uint32_t)w, k = (u >> 1) & 7u, bases = u >> 4;
    const uint32_t lo = bases & ((1u << (2 * p)) - 1u), hi = bases >> (2 * p);
    return (int32_t)((u & 1u) | ((k + 1u) << 1) | ((lo | ((uint32_t)(b & 3) << (2 * p)) | (hi << (2 * p + 2))) << 4));
}
static inline int32_t fig_polish_word_remove(int32_t w, int p) {                 // the base at position p out of the list (p < k)
    const uint32_t u = (uint32_t)w, k = (u >> 1) & 7u, bases = u >> 4;
    const uint32_t lo = bases & ((1u << (2 * p)) - 1u), hi = bases >> (2 * p + 2);
    return (int32_t)((u & 1u) | ((k - 1u) << 1) | ((lo | (hi << (2 * p))) << 4));
}

// The length of the current string of a gap of n0 original columns
static inline int64_t fig_polish_length(const int32_t *edit, int32_t n0, int32_t edit_end) {
    int64_t c = fig_polish_k(edit_end);
    for (int32_t x = 0; x < n0; x++) c += fig_polish_k(edit[x]) + ((edit[x] & 1) ? 0 : 1);
    return c;
}

// Current cell y -> the original column x it belongs to (n0: the list after the last column) and its slot: 0..k-1 an inserted base,
// -1 the column's own base.  y = the current length gives (n0, k of edit_end): the place after the last cell.  False beyond that.
static inline bool fig_polish_locate(const int32_t *edit, int32_t n0, int32_t edit_end, int64_t y, int32_t &x, int &slot) {
    int64_t c = 0;
    if (y < 0) return false;
    for (x = 0; x <= n0; x++) {
        const int32_t w = x < n0 ? edit[x] : edit_end;
        const int k = fig_polish_k(w);
        if (y < c + k) { slot = (int)(y - c); return true; }
        c += k;
        if (x < n0 && !(w & 1)) { if (y == c) { slot = -1; return true; } c++; }
    }
    x = n0; slot = fig_polish_k(edit_end);
    return y == c;
}

// INS before current cell y: 1 done, 0 refused (the list holds FIG_POLISH_MAX_K bases already), -1 no such cell
static inline int fig_polish_insert(int32_t *edit, int32_t n0, int32_t *edit_end, int64_t y, int b) {
    int32_t x; int slot;
    if (!fig_polish_locate(edit, n0, *edit_end, y, x, slot)) return -1;
    int32_t *w = x < n0 ? edit + x : edit_end;
    const int k = fig_polish_k(*w);
    if (k >= FIG_POLISH_MAX_K) return 0;
    *w = fig_polish_word_insert(*w, slot < 0 ? k : slot, b);
    return 1;
}
// whether fig_polish_insert before cell y would be done
static inline bool fig_polish_can_insert(const int32_t *edit, int32_t n0, int32_t edit_end, int64_t y) {
    int32_t x; int slot;
    if (!fig_polish_locate(edit, n0, edit_end, y, x, slot)) return false;
    return fig_polish_k(x < n0 ? edit[x] : edit_end) < FIG_POLISH_MAX_K;
}

// DEL of current cell y: 1 done, -1 no such cell.  (The caller keeps one cell: DEL at a length of 1 is never asked for.)
static inline int fig_polish_remove(int32_t *edit, int32_t n0, int32_t *edit_end, int64_t y) {
    int32_t x; int slot;
    if (!fig_polish_locate(edit, n0, *edit_end, y, x, slot)) return -1;
    int32_t *w = x < n0 ? edit + x : edit_end;
    if (slot < 0) { *w |= 1; return 1; }
    if (slot >= fig_polish_k(*w)) return -1;                                      // (the place after the last cell is no cell)
    *w = fig_polish_word_remove(*w, slot);
    return 1;
}

// The polished string of a gap: the inserted bases of edit[x], then str[x] unless removed; then the bases of edit_end.  Returns its
// length; writes it when dst is given.
static inline int64_t fig_polish_string(const int32_t *edit, int32_t n0, int32_t edit_end, const char *str, char *dst) {
    int64_t c = 0;
    for (int32_t x = 0; x <= n0; x++) {
        const int32_t w = x < n0 ? edit[x] : edit_end;
        for (int i = 0, k = fig_polish_k(w); i < k; i++, c++) if (dst) dst[c] = "ACGT"[fig_polish_base(w, i)];
        if (x < n0 && !(w & 1)) { if (dst) dst[c] = str[x]; c++; }
    }
    return c;
}

// the body of fig_polish_apply (include/figbird_hip.h)
static inline int fig_polish_apply_body(const fig_gap_results *f, const fig_gap_polish *p, int64_t g, char *dst) {
    if (!f || !p || g < 0 || !f->filled_len || !f->str_off || !p->edit || !p->edit_end || !p->polished_len || !p->state) return FIG_EINVAL;
    const int32_t n0 = f->filled_len[g];
    if (!(p->state[g] & FIG_POLISH_ON)) {                                         // an off gap keeps its own bytes
        const int32_t n = p->polished_len[g];
        if (n > 0 && (!f->str || f->str_off[g] + n > f->str_off[g + 1])) return FIG_EINVAL;
        for (int32_t i = 0; dst && i < n; i++) dst[i] = f->str[f->str_off[g] + i];
        return n > 0 ? n : 0;
    }
    if (n0 <= 0 || !f->str || f->str_off[g] + n0 > f->str_off[g + 1]) return FIG_EINVAL;
    const int64_t len = fig_polish_string(p->edit + f->str_off[g], n0, p->edit_end[g], f->str + f->str_off[g], nullptr);
    if (len != p->polished_len[g]) return FIG_EINVAL;
    fig_polish_string(p->edit + f->str_off[g], n0, p->edit_end[g], f->str + f->str_off[g], dst);
    return (int)len;
}

#endif
