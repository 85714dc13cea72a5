// fig_recruit_host.h -- the device-free half of the recruiting pass (fig_batch_recruit, include/figbird_hip.h: fig_read_recruit;
// DESIGN.md §5h): which gaps are on and which reads are candidates, the window around the seed that the second-best placement must
// lie outside, the order in which two (score, offset) pairs compete for the seed, the score, the three-way rule and the merge of a
// read into the out planes.  Pure C++ (no HIP, no engine headers): compiled into libfighip.so (fig_abi.hip and fig_recruit_kernel.hip,
// where the kernel of fig_recruit.h calls the marked functions on the device too) and into libfighost.so / figfill
// (host/fig_host.cpp), so that the library, the writers and the tests share one statement of each rule.
#ifndef FIG_RECRUIT_HOST_H
#define FIG_RECRUIT_HOST_H
#include <cmath>
#include <cstdint>
#include <limits>
#include "../../include/figbird_hip.h"
#include "fig_indel_host.h"

// FIG_RECRUIT_ON iff the gap is FIG_PLACE_ON
static inline uint8_t fig_recruit_gap_on(bool unmapped_model, int32_t n, int32_t draw_len_u, int32_t draw_len_p, bool has_origin, int32_t origin) {
    return fig_placement_gap_on(unmapped_model, n, draw_len_u, draw_len_p, has_origin, origin) == FIG_PLACE_ON ? FIG_RECRUIT_ON : FIG_RECRUIT_OFF;
}

// A read of a gap that is on is a candidate iff the fill did not draw it
FIG_P_HD inline bool fig_recruit_candidate(int32_t draw_pos) { return draw_pos == INT32_MIN; }

// The second-best placement is sought among the offsets outside the band around the seed: offsets within it are the same locus
FIG_P_HD inline bool fig_recruit_outside(int o, int off_seed) {
    const long long d = (long long)o - (long long)off_seed;
    return d > FIG_INDEL_W || d < -FIG_INDEL_W;
}

// The order of the seed and of the second: the greater score first, among equal scores the smaller offset.  A slot starts as
// (-inf, INT32_MAX), which every offered pair comes before; fig_recruit_take keeps the earlier of the slot and the offered pair.
FIG_P_HD inline bool fig_recruit_before(double v, int o, double bv, int bo) { return v > bv || (v == bv && o < bo); }
FIG_P_HD inline void fig_recruit_take(double v, int o, double &bv, int &bo) {
    if (fig_recruit_before(v, o, bv, bo)) { bv = v; bo = o; }
}
// The slots of a read's `nw` partial reductions (the kernel: its waves' slots, in wave order) into one
template <typename DP, typename IP>
FIG_P_HD inline void fig_recruit_reduce(DP pv, IP po, int nw, int stride, double &bv, int &bo) {
    bv = pv[0]; bo = po[0];
    for (int w = 1; w < nw; w++) fig_recruit_take(pv[w * stride], po[w * stride], bv, bo);
}

// A candidate is seeded iff it has a valid placement and the best of them is not -inf
FIG_P_HD inline bool fig_recruit_seeded(int n_valid, double ll_seed) { return n_valid > 0 && ll_seed > -__builtin_inf(); }

// score = li[isz(off_seed)] + ll_gapped, one IEEE addition
static inline double fig_recruit_score(double li_seed, double ll_gapped) { return li_seed + ll_gapped; }

// The rule of a seeded candidate, in this order: BELOW unless the fill's own test holds on the gapped score; else AMBIGUOUS unless
// there is no second locus or the seed beats it by more than min_margin; else RECRUITED
static inline uint8_t fig_recruit_rule(double score, int32_t gap_prob_cutoff, double ll_seed, double ll_second, double min_margin) {
    if (!(-score < (double)gap_prob_cutoff)) return FIG_RECRUIT_BELOW;
    if (!(ll_second == -std::numeric_limits<double>::infinity() || ll_seed - ll_second > min_margin)) return FIG_RECRUIT_AMBIGUOUS;
    return FIG_RECRUIT_RECRUITED;
}

// min_margin is the caller's: finite and >= 0
static inline bool fig_recruit_margin_ok(double min_margin) { return std::isfinite(min_margin) && min_margin >= 0; }

// One read into the out planes: a KEPT (or OFF) read keeps the caller's pair, a RECRUITED read gets its seed, every other read is undrawn
static inline void fig_recruit_merge(uint8_t read_state, int32_t draw_pos, int32_t draw_isz, int32_t off_seed, int32_t isz_seed, int32_t &pos_out, int32_t &isz_out) {
    if (read_state == FIG_RECRUIT_KEPT || read_state == FIG_RECRUIT_READ_OFF) { pos_out = draw_pos; isz_out = draw_isz; }
    else if (read_state == FIG_RECRUIT_RECRUITED) { pos_out = off_seed; isz_out = isz_seed; }
    else { pos_out = INT32_MIN; isz_out = 0; }
}

// The character of a read in gaprecruit.txt
static inline char fig_recruit_char(uint8_t read_state) {
    return read_state == FIG_RECRUIT_KEPT ? '.' : read_state == FIG_RECRUIT_RECRUITED ? '+' : read_state == FIG_RECRUIT_BELOW ? '-' : read_state == FIG_RECRUIT_AMBIGUOUS ? '=' : '~';
}

#endif
