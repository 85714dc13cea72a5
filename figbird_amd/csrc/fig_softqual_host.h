// fig_softqual_host.h -- the device-free half of the per-base quality that sums over read placements (fig_batch_softqual,
// include/figbird_hip.h): which gaps are on, the cut below which a placement carries no weight, and the greatest
// score M and the normaliser Z of a read from the three doubles the placement pass leaves per read.  Pure C++ (no HIP, no engine
// headers): compiled into libfighip.so (fig_abi.hip, where the kernel of fig_softqual.h calls the two marked functions on the
// device too) and into libfighost.so / figfill (host/fig_host.cpp), so that the library, the writers and the tests share one
// statement of each rule.
#ifndef FIG_SOFTQUAL_HOST_H
#define FIG_SOFTQUAL_HOST_H
#include <cmath>
#include <cstdint>
#include <limits>
#include "../../include/figbird_hip.h"
#include "fig_placement_host.h"

#define FIG_SOFTQ_CUT (-300.0)       // a valid placement is active iff Lr(o) - M_r >= this

// FIG_SOFTQ_ON iff the placement's rule holds
static inline uint8_t fig_softqual_gap_on(bool unmapped_model, int32_t n, int32_t draw_len_u, int32_t draw_len_p, bool has_origin, int32_t origin) {
    return fig_placement_gap_on(unmapped_model, n, draw_len_u, draw_len_p, has_origin, origin) == FIG_PLACE_ON ? FIG_SOFTQ_ON : FIG_SOFTQ_OFF;
}

// d = Lr(o) - M_r of a valid placement: -inf and whatever would underflow stay out (a NaN too)
FIG_P_HD inline bool fig_softqual_active(double d) { return d >= FIG_SOFTQ_CUT; }

// M_r and Z_r of a scored read from fig_read_placement's ll_drawn, ll_other and sum_other; false for a read that takes no part
// (no valid placement, or none above -inf).  Z = sum_other + 10^(ll_drawn - M): sum_other holds the terms below the cut as
// well, which change it by less than 1e-297 relative.
FIG_P_HD inline bool fig_softqual_mz(double ll_drawn, double ll_other, double sum_other, double &M, double &Z) {
    const double ninf = -__builtin_inf();
    M = ll_drawn > ll_other ? ll_drawn : ll_other;
    Z = 0.0;
    if (!(M > ninf)) return false;
    Z = sum_other + (ll_drawn > ninf ? exp10(ll_drawn - M) : 0.0);
    return true;
}

#endif
