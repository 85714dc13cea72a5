// fig_band.h -- the banded dynamic program the four gapped passes share (fig_indel.h, fig_polish.h, fig_recruit.h, fig_alnqual.h;
// DESIGN.md §5f): a read is aligned around an offset o on 15 diagonals d = -7 .. +7 against column codes under the run's substitution,
// insertion and deletion tables.  A cell only ADDS entries of the log10 tables the host built (fig_quality_host.h, fig_indel_host.h),
// one IEEE double addition each, and the rest is comparisons: every value is reproducible bit for bit.
//
// The cell update, the relaxation step of the deletion sweep and the end choice are __host__ __device__ functions; a plain C++ build
// compiles the same text (tests/band_form.h runs them in the kernels' form).  Under __HIPCC__: what the four kernels read alike
// (FigBandIn) and the pieces of a kernel that runs the band -- the lI | lD staging, the window fill, the forward pass of one 16-lane
// row and the decode of the back-pointers it leaves.
#ifndef FIG_BAND_H
#define FIG_BAND_H
#include <stdint.h>
#include "fig_indel_host.h"
#include "fig_readstage.h"

#define FIG_ID_NT (4 * FIG_RS_CHUNK)                 // threads of a workgroup; a work item is one chunk of reads
#define FIG_ID_ROW 16                                // lanes of a read: its 15 diagonals and the -inf border above d = +W
#define FIG_ID_GROUP (FIG_ID_NT / FIG_ID_ROW)        // reads in flight at a time
#define FIG_ID_WIN ((FIG_RS_MAXL + 2 * FIG_INDEL_W + 1 + 3) & ~3)   // column codes a read's band can touch (+1: the border lane's read)
#define FIG_ID_DIAG 0                                // back-pointers
#define FIG_ID_INS 1
#define FIG_ID_DEL 2

// The substitution term of read base (s, k) on a column of code c
template <typename DP>
FIG_P_HD inline double fig_indel_term(int c, int s, int k, DP lm, DP le, DP lt) {
    return c > 3 ? FIG_INDEL_LQ : c == s ? lm[k] : le[k] + lt[(c & 3) * 4 + s];
}

// H(i, d) before the deletion sweep, from H(i-1, d) and H(i-1, d+1) (-inf for d = +W): base_ok false = the read base is outside ACGT
FIG_P_HD inline double fig_indel_cell(double h_diag, double h_up, bool base_ok, double t, double lI, int &bp) {
    const double diag = base_ok ? h_diag + t : h_diag;
    const double ins = h_up + lI;
    bp = diag >= ins ? FIG_ID_DIAG : FIG_ID_INS;
    return diag >= ins ? diag : ins;
}

// One relaxation of the deletion sweep: h = H(i, d), below = H(i, d-1).  True iff h rose.  The sequential sweep applies it once per
// diagonal in ascending d; the kernels apply it to all diagonals at once until none rises: round t finishes the chains of t
// deletions, each by the sweep's own additions in the sweep's own order, and max is exact, so the fixed point is the sweep's H bit
// for bit and a cell ends above its first value iff the sweep gave it the DEL pointer (tests/indel_read_main.cpp holds the two
// against each other).
FIG_P_HD inline bool fig_indel_relax(double &h, double below, double lD) {
    const double v = below + lD;
    if (v > h) { h = v; return true; }
    return false;
}

// The end of the path: the greatest of H[q] = H(len, q - W), ties to the first diagonal of fig_indel_end_order
template <typename HP>
FIG_P_HD inline double fig_indel_end(HP H, int &d_end) {
    double best = H[FIG_INDEL_W];
    d_end = 0;
    for (int t = 1; t < FIG_INDEL_ND; t++) {
        const int d = fig_indel_end_order(t);
        const double v = H[d + FIG_INDEL_W];
        if (v > best) { best = v; d_end = d; }
    }
    return best;
}

// The back-pointer of cell (i, d), 1 <= i <= len, from the dwords fig_band_forward leaves: row i at [i - 1], bit q = INS, bit 16 + q =
// DEL of diagonal q - W
FIG_P_HD inline int fig_band_bp(const uint32_t *row, int i, int d) {
    const uint32_t v = row[i - 1] >> (d + FIG_INDEL_W);
    return (v & 1u) ? FIG_ID_INS : (v & 0x10000u) ? FIG_ID_DEL : FIG_ID_DIAG;
}

#ifdef __HIPCC__
// What every kernel that runs the band reads (all device memory; every array is read through an address-space-1 view): the base of
// the indel, polish and alnqual argument structs; FigRecruitArgs holds the same members in its own order (fig_recruit.h).
// FigPostFill::band_in (fig_abi.hip) fills it.
struct FigBandIn {
    const FigDevGap *gaps;           // the resident batch's descriptors: nU, uBase, flankOff
    const int32_t *u_len, *u_aux;
    const int64_t *u_woff;
    const uint32_t *packed;
    const uint8_t *flank;
    const int32_t *draw_pos;         // [n_ureads] the caller's offsets, INT32_MIN = not drawn
    const int32_t *items;            // [gridDim.x * 2] the work items: {gap or candidate, first read of the chunk within the gap}
    const int32_t *ncol;             // [n_gaps] bases of the gap's string
    const int64_t *str_off;          // [n_gaps + 1] the caller's (compacted) string offsets
    const char *str;                 // the caller's strings
    const double *tabs;              // lm[L] | le[L] | lt[16]
    const double *tabs_id;           // lI[L] | lD[L]
    int32_t L;
};

// The host's block lI[L] | lD[L] (fig_indel_tables) into s_id -- lI at 0, lD at FIG_RS_MAXL -- by a workgroup of nt threads, beside
// fig_rs_stage_tables; the caller's next barrier publishes it.
__device__ __forceinline__ void fig_band_stage_id(double (&s_id)[2 * FIG_RS_MAXL], const double *tabs_id, int L, int tid, int nt) {
    for (int i = tid; i < 2 * L; i += nt) s_id[i < L ? i : FIG_RS_MAXL + (i - L)] = ((fig_rs_gcdp)tabs_id)[i];
}

// The window of a read at offset o into S[FIG_ID_WIN], by the 16 lanes of its row: S[x - (o - W)] = column(x) for the len + 2W
// columns the band touches and the one more the border lane reads (its value is -inf whatever it adds).  The caller's next barrier
// publishes it.
template <typename Col>
__device__ __forceinline__ void fig_band_window(uint8_t *S, int o, int len, int q, Col column) {
    for (int i = q; i <= len + 2 * FIG_INDEL_W; i += FIG_ID_ROW) S[i] = (uint8_t)column(o - FIG_INDEL_W + i);
}

// The forward pass.  A read's band lives in one 16-lane row of a wave, four reads per wave: lane q < 15 holds H(i, q - 7) in a
// register and lane 15 the -inf above d = +7.  A row of the band is one step of the wave, which walks to its longest read: the INS
// neighbour H(i-1, d+1) comes from the lane above and the DEL neighbour H(i, d-1) from the lane below by row-wise shuffles, and the
// deletion sweep repeats fig_indel_relax on all diagonals until a ballot says no lane rose.  Every lane of the wave calls it; al
// false = the row has no read.  S: the read's window in LDS (fig_band_window), w: its words.  Returns the lane's H(len, q - 7).
// BACKPOINTERS: the pointers of row i, two ballots' 16-bit slices, into bp_row[i - 1] (fig_band_bp reads them).  FLAT: the sum of
// the lane's own diagonal terms into *flat; lane 7's is the read's ungapped score, d = 0.  A pointer of a switch that is off is null.
template <bool BACKPOINTERS, bool FLAT>
__device__ __forceinline__ double fig_band_forward(fig_rs_lu8p S, fig_rs_lu32p w, bool al, int len, int rev, int q,
                                                   fig_rs_ldp lm, fig_rs_ldp le, fig_rs_ldp lt, fig_rs_ldp lI, fig_rs_ldp lD, uint32_t *bp_row, double *flat) {
    const double ninf = -__builtin_inf();
    int rows = al ? len : 0;                                     // the wave walks to its longest read
    rows = max(rows, __shfl_xor(rows, 16, 64)); rows = max(rows, __shfl_xor(rows, 32, 64));
    double h = q < FIG_INDEL_ND ? 0.0 : ninf;
    double fl = 0.0;
    for (int i = 1; i <= rows; i++) {
        const bool active = al && i <= len;
        const double up = __shfl_down(h, 1, FIG_ID_ROW);         // H(i-1, d+1); lane 14 gets the border's -inf, lane 15 itself
        double hn = h, ld = ninf;
        int bp = FIG_ID_DIAG;
        if (active) {
            int s, k;
            const bool ok = fig_rs_base(w, len, rev, i - 1, s, k);
            const double t = fig_indel_term((int)S[i - 1 + q], s, k, lm, le, lt);
            hn = fig_indel_cell(h, up, ok, t, lI[k], bp);
            if (FLAT && ok) fl = fl + t;
            ld = lD[k];
        }
        const bool sweep = active && i < len && q >= 1 && q < FIG_INDEL_ND;
        bool rose;
        do {
            const double below = __shfl_up(hn, 1, FIG_ID_ROW);
            rose = sweep && fig_indel_relax(hn, below, ld);
            if (BACKPOINTERS && rose) bp = FIG_ID_DEL;
        } while (__ballot(rose));
        if (BACKPOINTERS) {
            const int sh = (int)threadIdx.x & 48;                // the row's 16 bits of the wave's ballot
            const unsigned long long b_ins = __ballot(bp == FIG_ID_INS), b_del = __ballot(bp == FIG_ID_DEL);
            if (active && q == 0) bp_row[i - 1] = (uint32_t)((b_ins >> sh) & 0xffffu) | ((uint32_t)((b_del >> sh) & 0xffffu) << 16);
        }
        h = hn;
    }
    if (FLAT) *flat = fl;
    return h;
}
#endif
#endif
