// fig_polish.h -- the scoring kernel of the polish (fig_batch_polish; include/figbird_hip.h: fig_gap_polish): every
// candidate edit of a round -- one column of a gap's string removed, or one base put before a column -- is scored by the banded
// dynamic program of fig_band.h over the reads the edit touches, against the edited sequence at the shifted offset.  The band is
// the one fig_indel_kernel runs (fig_band_forward): the same additions in the same order, so a score is what fig_batch_indel would
// report for the edited string bit for bit.  The edit enters in one place, the column codes (fig_polish_column); there are no
// back-pointers, no traceback and no atomics.
//
// Like fig_indel_kernel the kernel is compiled in a translation unit of its own (fig_polish_kernel.hip defines FIG_POLISH_KERNEL;
// fig_abi.hip sees the argument struct and fig_polish_launch only).
#ifndef FIG_POLISH_H
#define FIG_POLISH_H
#include <stdint.h>
#include "fig_polish_host.h"
#include "fig_band.h"
#include "fig_placement.h"

// The code of column y of the edited sequence S_c: fl / str / n are the UNEDITED gap's (fig_placement_column)
template <typename FP, typename SP>
FIG_P_HD inline int fig_polish_column(int y, int n, FP fl, SP str, int kind, int x, int b) {
    if (kind == FIG_POLISH_INS) return y < x ? fig_placement_column(y, n, fl, str) : y == x ? b : fig_placement_column(y - 1, n, fl, str);
    return fig_placement_column(y < x ? y : y + 1, n, fl, str);
}

#ifdef __HIPCC__
// What the kernel reads (FigBandIn with the round's offsets and strings; items: {candidate, first read of the chunk within the
// gap}) and the one array it writes.
struct FigPolishArgs : FigBandIn {
    const int32_t *cands;            // [n_cands * 4] {gap, kind, x, base code}
    const int64_t *cand_off;         // [n_cands] where the candidate's scores start in `out`
    double *out;                     // out[cand_off[c] + r]: ll_c of read r of the candidate's gap; zeroed by the caller, written for counted reads
};

// the launch of fig_polish_kernel over `items` work items (fig_polish_kernel.hip)
hipError_t fig_polish_launch(const FigPolishArgs &A, unsigned items, hipStream_t stream);

#ifdef FIG_POLISH_KERNEL
// One workgroup per (candidate, chunk of 64 reads of its gap), the chunk staged in LDS once; 16 reads at a time, a read's band in one
// 16-lane row of a wave (fig_band_forward, forward only); one lane per read takes the end and writes the score.
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
    fig_band_stage_id(s_id, A.tabs_id, L, tid, FIG_ID_NT);
    fig_rs_ldp lm = (fig_rs_ldp)&s_tab[0], le = (fig_rs_ldp)&s_tab[L], lt = (fig_rs_ldp)&s_tab[2 * FIG_RS_MAXL];
    fig_rs_ldp lI = (fig_rs_ldp)&s_id[0], lD = (fig_rs_ldp)&s_id[FIG_RS_MAXL];
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
        if (al) fig_band_window(&s_S[rr][0], o, len, q, [&](int y) { return fig_polish_column(y, n, fl, str, kind, ex, eb); });
        __syncthreads();
        s_H[rr][q] = fig_band_forward<false, false>((fig_rs_lu8p)&s_S[rr][0], w, al, len, rev, q, lm, le, lt, lI, lD, nullptr, nullptr);
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
