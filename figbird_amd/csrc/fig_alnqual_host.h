// fig_alnqual_host.h -- the device-free half of the per-base quality over gapped read alignments (fig_batch_alnqual,
// include/figbird_hip.h): which gaps are on, the flat path of a read whose every gapped path is -inf, the column map
// of a read (one nibble per window column) with its pack and unpack, the span of a path, and what one read adds to one column.  Pure
// C++ (no HIP, no engine headers): compiled into libfighip.so (fig_alnqual_kernel.hip, where the kernels of fig_alnqual.h call the
// marked functions on the device too) and into libfighost.so / figfill (host/fig_host.cpp).  The tables are fig_quality_host.h's and
// fig_indel_host.h's, and so is the Phred.
#ifndef FIG_ALNQUAL_HOST_H
#define FIG_ALNQUAL_HOST_H
#include <cstdint>
#include "../../include/figbird_hip.h"
#include "fig_indel_host.h"
#include "fig_readstage.h"

#define FIG_ALNQ_NONE 15                                                       // the nibble of a window column no DIAG step lands on
#define FIG_ALNQ_MAPB ((((FIG_RS_MAXL + 2 * FIG_INDEL_W + 1) >> 1) + 3) & ~3)  // bytes of a read's map, a whole number of dwords: 108
#define FIG_ALNQ_MAPW (FIG_ALNQ_MAPB / 4)

// FIG_ALNQ_ON iff the gap is FIG_INDEL_ON
static inline uint8_t fig_alnqual_gap_on(bool unmapped_model, int32_t n, int32_t draw_len_u, int32_t draw_len_p, bool has_origin, int32_t origin) {
    return fig_indel_gap_on(unmapped_model, n, draw_len_u, draw_len_p, has_origin, origin) == FIG_INDEL_ON ? FIG_ALNQ_ON : FIG_ALNQ_OFF;
}

// A read of `len` bases has window columns c = x - (o* - W), 0 <= c < len + 2W; this many bytes of its map are in use
FIG_P_HD inline int fig_alnqual_map_bytes(int len) { return (len + 2 * FIG_INDEL_W + 1) >> 1; }

// Nibble c of a map: the even column in the low half of byte c / 2
template <typename MP>
FIG_P_HD inline int fig_alnqual_nibble(MP map, int c) { return (int)((map[c >> 1] >> ((c & 1) * 4)) & 15u); }
template <typename MP>
FIG_P_HD inline void fig_alnqual_set_nibble(MP map, int c, int v) {
    const int sh = (c & 1) * 4;
    map[c >> 1] = (uint8_t)((map[c >> 1] & ~(15u << sh)) | ((unsigned)v << sh));
}

// The flat path: every base on d = 0.  It is the path of a read whose ll_gapped is -inf.  The map's bytes in use are FIG_ALNQ_NONE
// throughout when this is called.
template <typename MP>
FIG_P_HD inline void fig_alnqual_flat(MP map, int len, int &d_start, int &d_end, int &n_ins, int &n_del) {
    for (int j = 0; j < len; j++) fig_alnqual_set_nibble(map, j + FIG_INDEL_W, FIG_INDEL_W);
    d_start = 0; d_end = 0; n_ins = 0; n_del = 0;
}

// The columns a path spans: its first next-column and the column before its last
FIG_P_HD inline void fig_alnqual_span(int o, int len, int d_start, int d_end, int &lo, int &hi) { lo = o + d_start; hi = o + len - 1 + d_end; }

// Column x against one aligned read drawn at o whose path spans [lo, hi] and whose map is `map`.  A column of the span no DIAG step
// lands on is skipped by the read: FIG_ALNQ_SKIP.  Otherwise base j = x - o - d of the read sits on it and, if it is one of ACGT, adds
// fig_quality's terms to the four accumulators (true base A, C, G, T): FIG_ALNQ_BASE, or FIG_ALNQ_AGREE when it is the emitted code
// `call` (4 for a byte outside ACGT).  Everything else is FIG_ALNQ_NOTHING: a column outside the span, a base outside ACGT, and an
// entry that the path kernel cannot have written (a nibble that puts j outside the read).  w, lm, le, lt as for fig_quality_add_read.
// The counts are the caller's: depth counts BASE and AGREE, agree AGREE, skip SKIP.
#define FIG_ALNQ_NOTHING 0
#define FIG_ALNQ_SKIP 1
#define FIG_ALNQ_BASE 2
#define FIG_ALNQ_AGREE 3
template <typename WP, typename MP, typename DP>
FIG_P_HD inline int fig_alnqual_add_read(double &a0, double &a1, double &a2, double &a3, int x, int call, int o, int len, int rev, int lo, int hi, WP w, MP map, DP lm, DP le, DP lt) {
    if (x < lo || x > hi) return FIG_ALNQ_NOTHING;
    const int c = x - o + FIG_INDEL_W;
    if ((unsigned)c >= (unsigned)(len + 2 * FIG_INDEL_W)) return FIG_ALNQ_NOTHING;
    const int nib = fig_alnqual_nibble(map, c);
    if (nib == FIG_ALNQ_NONE) return FIG_ALNQ_SKIP;
    const int j = c - nib;
    if ((unsigned)j >= (unsigned)len) return FIG_ALNQ_NOTHING;
    int s, k;
    if (!fig_rs_base(w, len, rev, j, s, k)) return FIG_ALNQ_NOTHING;
    const double m = lm[k], e = le[k];
    a0 = a0 + (s == 0 ? m : e + lt[0 + s]);
    a1 = a1 + (s == 1 ? m : e + lt[4 + s]);
    a2 = a2 + (s == 2 ? m : e + lt[8 + s]);
    a3 = a3 + (s == 3 ? m : e + lt[12 + s]);
    return s == call ? FIG_ALNQ_AGREE : FIG_ALNQ_BASE;
}

// The code of an emitted byte as agree compares it
FIG_P_HD inline int fig_alnqual_call_code(char c) { return c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : c == 'T' ? 3 : 4; }

#endif
