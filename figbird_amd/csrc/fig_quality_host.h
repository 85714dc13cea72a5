// fig_quality_host.h -- the device-free half of the per-base quality (fig_batch_quality, include/figbird_hip.h):
// the three log10 tables the kernel adds, the Phred of a column, which gaps have a quality at all, and the bounds check of the
// placements a caller hands in.  Pure C++ (no HIP, no engine headers): compiled into libfighip.so (fig_abi.hip) and into
// libfighost.so / figfill (host/fig_host.cpp), so that the library, the writers and the tests share one statement of each rule.
#ifndef FIG_QUALITY_HOST_H
#define FIG_QUALITY_HOST_H
#include <cmath>
#include <cstdint>
#include <limits>
#include "../../include/figbird_hip.h"

#define FIG_QUAL_MAX_OFFSET (1 << 20)      // a drawn offset o with |o| >= this is FIG_EINVAL: x - o then never overflows an int
#define FIG_QUAL_MAX_PHRED 93              // '~' - 33

// Layout of the table block the kernel stages into LDS: lm[L] | le[L] | lt[16], doubles
static inline int fig_quality_tab_doubles(int L) { return 2 * L + 16; }

// lm[k] = log10(1 - e[k]) (`ome` = the 1 - e[k] doubles of fig_model_tables' h_ome), le[k] = log10(e[k]),
// lt[b * 4 + s] = log10(T[b * 5 + s]): row = true base, column = read base, A..T.  log10(0) = -inf is kept.
static inline void fig_quality_tables(int L, const double *e, const double *ome, const double *T25, double *lm, double *le, double *lt16) {
    for (int k = 0; k < L; k++) { lm[k] = log10(ome[k]); le[k] = log10(e[k]); }
    for (int b = 0; b < 4; b++) for (int s = 0; s < 4; s++) lt16[b * 4 + s] = log10(T25[b * 5 + s]);
}

// The same from a fig_model: 1 - e[k] rounded to a double exactly as fig_model_tables (fig_abi_host.h) rounds it.
static inline void fig_quality_tables_model(const fig_model *m, double *lm, double *le, double *lt16) {
    const int L = m->max_read_length;
    for (int k = 0; k < L; k++) {
        volatile double a = 1 - m->error_pos_dist[k];
        lm[k] = log10(a); le[k] = log10(m->error_pos_dist[k]);
    }
    for (int b = 0; b < 4; b++) for (int s = 0; s < 4; s++) lt16[b * 4 + s] = log10(m->error_type_probs[b * 5 + s]);
}

// Phred of one column: its four log-likelihoods (true base A, C, G, T) and the emitted byte.  Uniform prior, the posterior
// error probability of the called base, rounded to the nearest integer and clamped to 0..93.
static inline uint8_t fig_quality_phred(const double *ll, char c) {
    const int ci = c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : c == 'T' ? 3 : -1;
    if (ci < 0) return 0;
    const double ninf = -std::numeric_limits<double>::infinity();
    double m = ll[0];
    for (int b = 1; b < 4; b++) if (ll[b] > m) m = ll[b];
    if (!(m > ninf)) return 0;
    double w[4], num = 0;
    for (int b = 0; b < 4; b++) w[b] = ll[b] == ninf ? 0.0 : pow(10, ll[b] - m);
    for (int b = 0; b < 4; b++) if (b != ci) num = num + w[b];
    const double perr = num / (num + w[ci]);
    if (perr == 0) return FIG_QUAL_MAX_PHRED;
    const double q = floor(-10 * log10(perr) + 0.5);
    return (uint8_t)(q < 0 ? 0 : q > FIG_QUAL_MAX_PHRED ? FIG_QUAL_MAX_PHRED : q);
}

// FIG_QUAL_ON iff the gap has a string, exactly one draw header and that header's length is the string's, and -- when the
// origins of the support plane are given (has_origin) -- the string was called from this fill's final placement.
static inline uint8_t fig_quality_gap_on(int32_t n, int32_t draw_len_u, int32_t draw_len_p, bool has_origin, int32_t origin) {
    if (n <= 0) return FIG_QUAL_OFF;
    if ((draw_len_u >= 0) == (draw_len_p >= 0)) return FIG_QUAL_OFF;
    if ((draw_len_u >= 0 ? draw_len_u : draw_len_p) != n) return FIG_QUAL_OFF;
    if (has_origin && (!(origin & FIG_SUP_FINAL) || (origin & FIG_SUP_ORIGINAL))) return FIG_QUAL_OFF;
    return FIG_QUAL_ON;
}

// Placements of one gap's `n_reads` reads, draw_pos pointing at the first: INT32_MIN = not drawn, anything else must lie
// inside +-FIG_QUAL_MAX_OFFSET.  Returns the number of drawn reads, or -1.
static inline int64_t fig_quality_check_placements(const int32_t *draw_pos, int64_t n_reads) {
    int64_t drawn = 0;
    for (int64_t r = 0; r < n_reads; r++) {
        const int32_t o = draw_pos[r];
        if (o == INT32_MIN) continue;
        if (o >= FIG_QUAL_MAX_OFFSET || o <= -FIG_QUAL_MAX_OFFSET) return -1;
        drawn++;
    }
    return drawn;
}

#endif
