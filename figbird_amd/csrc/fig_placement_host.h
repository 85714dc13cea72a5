// fig_placement_host.h -- the device-free half of the placement confidence (fig_batch_placement, include/figbird_hip.h;
// DESIGN.md §5d): the log10 table of the insert-size distribution, the insert size of a placement and whether it is valid, which
// gaps are scored at all, and the Phred of a read (the drawn offsets are bounded as the quality's are, fig_quality_host.h).  Pure C++ (no HIP, no engine headers):
// compiled into libfighip.so (fig_abi.hip, where the kernel of fig_placement.h calls the two marked functions on the device too)
// and into libfighost.so / figfill (host/fig_host.cpp), so that the library, the writers and the tests share one statement of
// each rule.
#ifndef FIG_PLACEMENT_HOST_H
#define FIG_PLACEMENT_HOST_H
#include <cmath>
#include <cstdint>
#include <limits>
#include "../../include/figbird_hip.h"
#include "fig_quality_host.h"

#ifdef __HIPCC__
#define FIG_P_HD __host__ __device__
#else
#define FIG_P_HD
#endif

// li[s] = log10(insertLengthDistSmoothed[s]); log10(0) = -inf is kept
static inline void fig_placement_li(int32_t max_insert, const double *insd, double *li) {
    for (int32_t s = 0; s < max_insert; s++) li[s] = log10(insd[s]);
}

// Insert size of read (anchor `pos`, length `len`) placed at offset o of a gap whose string has n bases: the reference's
// tempInsertSize (Figbird.cpp finalize).  64-bit: pos is whatever the caller's SAM line held.
FIG_P_HD inline long long fig_placement_isz(long long pos, long long gap_start, int G0, int n, int len, int o) {
    return pos < gap_start ? gap_start - pos + len + o : pos + (n - G0) - gap_start + len - o;
}

// A placement is valid iff its insert size lies inside the thresholds and inside the table
FIG_P_HD inline bool fig_placement_valid(long long isz, int Tmin, int Tmax, int max_insert) {
    return isz >= Tmin && isz <= Tmax && isz >= 0 && isz < max_insert;
}

// FIG_PLACE_ON iff the model is unmapped-mode, the gap's evidence is its unmapped reads, and the quality's rule holds
static inline uint8_t fig_placement_gap_on(bool unmapped_model, int32_t n, int32_t draw_len_u, int32_t draw_len_p, bool has_origin, int32_t origin) {
    if (!unmapped_model || draw_len_u < 0 || draw_len_p >= 0) return FIG_PLACE_OFF;
    return fig_quality_gap_on(n, draw_len_u, draw_len_p, has_origin, origin) == FIG_QUAL_ON ? FIG_PLACE_ON : FIG_PLACE_OFF;
}

// Phred of one scored read: the posterior probability that it belongs to another valid placement, uniform prior over placements
static inline uint8_t fig_placement_phred(double ll_drawn, double ll_other, double sum_other) {
    const double ninf = -std::numeric_limits<double>::infinity();
    if (!(ll_drawn > ninf)) return 0;
    const double M = ll_drawn > ll_other ? ll_drawn : ll_other;
    const double w = pow(10, ll_drawn - M);
    const double perr = sum_other / (sum_other + w);
    if (perr == 0) return FIG_PLACE_MAX_PQ;
    const double q = floor(-10 * log10(perr) + 0.5);
    return (uint8_t)(q < 0 ? 0 : q > FIG_PLACE_MAX_PQ ? FIG_PLACE_MAX_PQ : q);
}

#endif
