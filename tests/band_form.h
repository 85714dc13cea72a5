// The forward pass of fig_band.h in the kernels' form, as plain C++, for the stand-alone programs of the four gapped passes
// (indel_read_main.cpp, polish_main.cpp, recruit_read_main.cpp, alnqual_main.cpp): 16 "lanes" per read as arrays of 16, the update
// from the lane above and the sweep's neighbour from the lane below as the row-wise shuffles give them, the deletion sweep as repeated
// relaxation of all diagonals until none rises.  Exit 4 with a message if the border lane ever leaves -inf.
#ifndef FIG_TESTS_BAND_FORM_H
#define FIG_TESTS_BAND_FORM_H
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>

#include "../figbird_amd/csrc/fig_band.h"

// S: the column codes of the read's window, len + 2W + 1 of them (the border lane reads the last); w: the read's words; lm .. lD: the
// five tables.  h: the last row, h[q] = H(len, q - W).  The kernels' two switches are pointers that may be null -- bpw[len]: the
// back-pointers of row i at [i - 1] as fig_band_bp reads them; flat: the ungapped score -- and Hall[(len + 1) * ND], likewise, takes
// every row (rows 1 .. len are written).
static inline void band_form(const uint8_t *S, const uint32_t *w, int len, int rev, const double *lm, const double *le, const double *lt, const double *lI,
                             const double *lD, double (&h)[16], uint32_t *bpw, double *flat, double *Hall) {
    const double ninf = -std::numeric_limits<double>::infinity();
    for (int q = 0; q < 16; q++) h[q] = q < FIG_INDEL_ND ? 0.0 : ninf;
    if (flat) *flat = 0.0;
    for (int i = 1; i <= len; i++) {
        double hn[16], ld = ninf;
        int bp[16];
        for (int q = 0; q < 16; q++) {
            const double up = q < 15 ? h[q + 1] : h[q];                      // __shfl_down(h, 1, 16)
            int s, k;
            const bool ok = fig_rs_base(w, len, rev, i - 1, s, k);
            const double t = fig_indel_term((int)S[i - 1 + q], s, k, lm, le, lt);
            hn[q] = fig_indel_cell(h[q], up, ok, t, lI[k], bp[q]);
            if (flat && q == FIG_INDEL_W && ok) *flat = *flat + t;
            ld = lD[k];
        }
        bool any;
        do {
            any = false;
            double prev[16];
            memcpy(prev, hn, sizeof(prev));
            for (int q = 0; q < 16; q++) {
                const double below = q > 0 ? prev[q - 1] : prev[q];          // __shfl_up(hn, 1, 16)
                const bool rose = i < len && q >= 1 && q < FIG_INDEL_ND && fig_indel_relax(hn[q], below, ld);
                if (rose) { bp[q] = FIG_ID_DEL; any = true; }
            }
        } while (any);
        if (bpw) {
            uint32_t m = 0;
            for (int q = 0; q < 16; q++) m |= (bp[q] == FIG_ID_INS ? 1u << q : 0u) | (bp[q] == FIG_ID_DEL ? 1u << (16 + q) : 0u);
            bpw[i - 1] = m;
        }
        memcpy(h, hn, sizeof(h));
        if (h[15] != ninf) { fprintf(stderr, "the border lane left -inf\n"); exit(4); }
        if (Hall) for (int q = 0; q < FIG_INDEL_ND; q++) Hall[(size_t)i * FIG_INDEL_ND + q] = h[q];
    }
}
#endif
