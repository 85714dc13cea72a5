// fig_polish.h -- the scoring kernel of the polish (fig_batch_polish; include/figbird_hip.h: fig_gap_polish): every
// candidate edit of a round -- one column of a gap's string removed, or one base put before a column -- is scored by the banded
// dynamic program of fig_indel.h over the reads the edit touches, against the edited sequence at the shifted offset.  The band is
// fig_indel.h's own text (fig_indel_term, fig_indel_cell, fig_indel_relax, fig_indel_end): the same additions in the same order, so
// a score is what fig_batch_indel would report for the edited string bit for bit.  The edit enters in one place, the column codes
// (fig_polish_column); there are no back-pointers, no traceback and no atomics.
//
// Like fig_indel_kernel the kernel is compiled in a translation unit of its own (fig_polish_kernel.hip defines FIG_POLISH_KERNEL;
// fig_abi.hip sees the argument struct and fig_polish_launch only).
#ifndef FIG_POLISH_H
#define FIG_POLISH_H
#include <stdint.h>
#include "fig_polish_host.h"
#include "fig_indel.h"

// The code of column y of the edited sequence S_c: fl / str / n are the UNEDITED gap's (fig_placement_column)
template <typename FP, typename SP>
FIG_P_HD inline int fig_polish_column(int y, int n, FP fl, SP str, int kind, int x, int b) {
    if (kind == FIG_POLISH_INS) return y < x ? fig_placement_column(y, n, fl, str) : y == x ? b : fig_placement_column(y - 1, n, fl, str);
    return fig_placement_column(y < x ? y : y + 1, n, fl, str);
}

#ifdef __HIPCC__
// What the kernel reads (all device memory; every array is read through an address-space-1 view) and the one array it writes.
struct FigPolishArgs {
    const FigDevGap *gaps;           // the resident batch's descriptors: nU, uBase, flankOff
    const int32_t *u_len, *u_aux;
    const int64_t *u_woff;
    const uint32_t *packed;
    const uint8_t *flank;
    const int32_t *draw_pos;         // [n_ureads] the round's offsets, INT32_MIN = not drawn
    const int32_t *items;            // [gridDim.x * 2] {candidate, first read of the chunk within the gap}
    const int32_t *cands;            // [n_cands * 4] {gap, kind, x, base code}
    const int64_t *cand_off;         // [n_cands] where the candidate's scores start in `out`
    const int32_t *ncol;             // [n_gaps] columns of the round's string
    const int64_t *str_off;          // [n_gaps + 1] offsets of the round's strings
    const char *str;
    const double *tabs;              // lm[L] | le[L] | lt[16]
    const double *tabs_id;           // lI[L] | lD[L]
    int32_t L;
    double *out;                     // out[cand_off[c] + r]: ll_c of read r of the candidate's gap; zeroed by the caller, written for counted reads
};

// the launch of fig_polish_kernel over `items` work items (fig_polish_kernel.hip)
hipError_t fig_polish_launch(const FigPolishArgs &A, unsigned items, hipStream_t stream);

#ifdef FIG_POLISH_KERNEL
// One workgroup per (candidate, chunk of 64 reads of its gap), the chunk staged in LDS once; 16 reads at a time, a read's band in one
// 16-lane row of a wave exactly as in fig_indel_kernel: lane q < 15 holds H(i, q - 7), lane 15 the -inf above d = +7, the INS
// neighbour comes from the lane above and the DEL neighbour from the lane below by row-wise shuffles, and the deletion sweep repeats
// fig_indel_relax until a ballot says no lane rose.  Forward only; one lane per read takes the end and writes the score.
__global__ void __launch_bounds__(FIG_ID_NT) fig_polish_kernel(FigPolishArgs A) {
    __shared__ double s_tab[FIG_RS_TAB];
    __shared__ double s_id[2 * FIG_RS_MAXL];                     // lI at 0, lD at FIG_RS_MAXL
    __shared__ int4 s_hdr[FIG_RS_CHUNK];                         // {shifted offset, length, reversed, counted}
    __shared__ uint32_t s_w[FIG_RS_CHUNK][FIG_RS_WORDS];
    __shared__ uint8_t s_S[FIG_ID_GROUP][FIG_ID_WIN];            // [y - (o_c - 7)]
    __shared__ double s_H[FIG_ID_GROUP][FIG_ID_ROW];
    const int tid = (int)threadIdx.x, rr = tid / FIG_ID_ROW, q = tid & (FIG_ID_ROW - 1);
    const int c = ((fig_rs_gi32p)A.items)[2 * blockIdx.x], c0 = ((fig_rs_gi32p)A.items)[2 * blockIdx.x + 1];
    const int g = ((fig_rs_gi32p)A.cands)[4 * c], kind = ((fig_rs_gi32p)A.cands)[4 * c + 1], ex = ((fig_rs_gi32p)A.cands)[4 * c + 2], eb = ((fig_rs_gi32p)A.cands)[4 * c + 3];
    fig_rs_ggapp gp = (fig_rs_ggapp)A.gaps + g;
    const int n = ((fig_rs_gi32p)A.ncol)[g];
    const int nc = min(FIG_RS_CHUNK, gp->nU - c0);
    const long long rbase = gp->uBase + c0;
    const long long obase = ((fig_rs_gi64p)A.cand_off)[c] + c0;
    const int L = A.L;
    fig_rs_gu8p fl = (fig_rs_gu8p)A.flank + gp->flankOff;
    fig_rs_gcp str = (fig_rs_gcp)A.str + ((fig_rs_gi64p)A.str_off)[g];
    fig_rs_stage_tables(s_tab, A.tabs, L, tid, FIG_ID_NT);
    for (int i = tid; i < 2 * L; i += FIG_ID_NT) s_id[i < L ? i : FIG_RS_MAXL + (i - L)] = ((fig_rs_gcdp)A.tabs_id)[i];
    fig_rs_ldp lm = (fig_rs_ldp)&s_tab[0], le = (fig_rs_ldp)&s_tab[L], lt = (fig_rs_ldp)&s_tab[2 * FIG_RS_MAXL];
    fig_rs_ldp lI = (fig_rs_ldp)&s_id[0], lD = (fig_rs_ldp)&s_id[FIG_RS_MAXL];
    const double ninf = -__builtin_inf();
    {   // stage the chunk
        int r, o, len;
        if (fig_rs_stage_reads(s_w, tid, nc, L, A.u_len, A.u_woff, A.packed, A.draw_pos, rbase, rbase, r, o, len)) {
            const bool cnt = fig_polish_counted(o, len, n, kind, ex);
            s_hdr[r] = make_int4(cnt ? fig_polish_shift(o, kind, ex) : 0, len, ((fig_rs_gi32p)A.u_aux)[rbase + r] & 1, cnt ? 1 : 0);
        }
    }
    __syncthreads();
    for (int g0 = 0; g0 < nc; g0 += FIG_ID_GROUP) {
        const int r = g0 + rr;
        const int4 h4 = r < nc ? s_hdr[r] : make_int4(0, 0, 0, 0);
        const int o = h4.x, len = h4.y, rev = h4.z;
        const bool al = h4.w != 0;
        fig_rs_lu32p w = (fig_rs_lu32p)&s_w[r < nc ? r : 0][0];
        if (al) for (int i = q; i <= len + 2 * FIG_INDEL_W; i += FIG_ID_ROW) s_S[rr][i] = (uint8_t)fig_polish_column(o - FIG_INDEL_W + i, n, fl, str, kind, ex, eb);
        __syncthreads();
        int rows = al ? len : 0;                                 // the wave walks to its longest read
        rows = max(rows, __shfl_xor(rows, 16, 64)); rows = max(rows, __shfl_xor(rows, 32, 64));
        double h = q < FIG_INDEL_ND ? 0.0 : ninf;
        for (int i = 1; i <= rows; i++) {
            const bool active = al && i <= len;
            const double up = __shfl_down(h, 1, FIG_ID_ROW);     // H(i-1, d+1); lane 14 gets the border's -inf, lane 15 itself
            double hn = h, ld = ninf;
            if (active) {
                int s, k, bp;
                const bool ok = fig_rs_base(w, len, rev, i - 1, s, k);
                const double t = fig_indel_term((int)s_S[rr][i - 1 + q], s, k, lm, le, lt);
                hn = fig_indel_cell(h, up, ok, t, lI[k], bp);
                ld = lD[k];
            }
            const bool sweep = active && i < len && q >= 1 && q < FIG_INDEL_ND;
            bool rose;
            do {
                const double below = __shfl_up(hn, 1, FIG_ID_ROW);
                rose = sweep && fig_indel_relax(hn, below, ld);
            } while (__ballot(rose));
            h = hn;
        }
        s_H[rr][q] = h;
        __syncthreads();
        if (al && q == 0) {
            int d_end;
            ((fig_rs_gdp)A.out)[obase + r] = fig_indel_end((fig_rs_ldp)&s_H[rr][0], d_end);
        }
        __syncthreads();
    }
}
#endif
#endif
#endif
