// fig_indel_host.h -- the device-free half of the indel evidence (fig_batch_indel, include/figbird_hip.h): the two
// log10 tables of the model's insertion and deletion rates, which gaps are on and which reads are aligned, the order in which the
// end diagonals are tried, and the call of a column.  Pure C++ (no HIP, no engine headers): compiled into libfighip.so (fig_abi.hip,
// where the kernel of fig_indel.h calls the marked functions on the device too) and into libfighost.so / figfill
// (host/fig_host.cpp), so that the library, the writers and the tests share one statement of each rule.
#ifndef FIG_INDEL_HOST_H
#define FIG_INDEL_HOST_H
#include <cmath>
#include <cstdint>
#include "../../include/figbird_hip.h"
#include "fig_placement_host.h"

#define FIG_INDEL_ND (2 * FIG_INDEL_W + 1)            // diagonals of the band
#define FIG_INDEL_LQ (-0x1.34413509f79ffp-1)          // log10(1/4), fig_placement.h's FIG_P_LQ
#define FIG_INDEL_MIN_READS 2                         // a call needs this many reads, and more than half of the column's cover

// lI[k] = log10(in_pos_dist[k]) + lq (an inserted read base is uniform over the four bases), lD[k] = log10(del_pos_dist[k]);
// log10(0) = -inf is kept
static inline void fig_indel_tables(int L, const double *ins, const double *del, double *lI, double *lD) {
    for (int k = 0; k < L; k++) { lI[k] = log10(ins[k]) + FIG_INDEL_LQ; lD[k] = log10(del[k]); }
}

// FIG_INDEL_ON iff the gap is FIG_PLACE_ON
static inline uint8_t fig_indel_gap_on(bool unmapped_model, int32_t n, int32_t draw_len_u, int32_t draw_len_p, bool has_origin, int32_t origin) {
    return fig_placement_gap_on(unmapped_model, n, draw_len_u, draw_len_p, has_origin, origin) == FIG_PLACE_ON ? FIG_INDEL_ON : FIG_INDEL_OFF;
}

// A scored read of `len` bases drawn at o is aligned iff the drawn placement touches the string
FIG_P_HD inline bool fig_indel_aligned(int32_t o, int32_t len, int32_t n) {
    return o != INT32_MIN && (long long)o >= -((long long)len - 1) && (long long)o <= (long long)n - 1;
}

// The t-th diagonal in the order ties at the end are settled: 0, -1, +1, -2, +2, ..., -W, +W  (t = 0 .. 2W)
FIG_P_HD inline int fig_indel_end_order(int t) { return t == 0 ? 0 : (t & 1) ? -((t + 1) >> 1) : (t >> 1); }

// The call of a column (or of the right junction): reads that ask for the edit against the reads that span it
static inline bool fig_indel_majority(int32_t reads, int32_t cover) { return reads >= FIG_INDEL_MIN_READS && 2 * (int64_t)reads > (int64_t)cover; }
static inline char fig_indel_call(int32_t del_reads, int32_t ins_reads, int32_t cover) {
    return fig_indel_majority(del_reads, cover) ? 'D' : fig_indel_majority(ins_reads, cover) ? 'I' : '.';
}

#endif
