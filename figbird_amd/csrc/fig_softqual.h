// fig_softqual.h -- per-base quality that sums over read placements (fig_batch_softqual): fig_quality.h piles every
// drawn read up at its drawn offset with weight 1; here a scored read lies on EVERY valid placement o with the posterior weight
// p_r(o) = 10^(Lr(o) - M_r) / Z_r of the scores fig_placement.h computes, and a column collects the expected read count per base
// (wcount) and the expected log10-likelihood per true base (eloglik).  M_r and Z_r come from the arrays fig_placement_kernel left
// on the device one launch earlier.  The kernel sits beside the fill: it reads the resident batch and writes two planes of its own.
//
// The weight of one placement and the arithmetic of one (column, read, row of weights) are __host__ __device__ functions; a plain
// C++ build compiles the same text.
#ifndef FIG_SOFTQUAL_H
#define FIG_SOFTQUAL_H
#include <stdint.h>
#include "fig_placement.h"
#include "fig_softqual_host.h"

#define FIG_SQ_NT (4 * FIG_RS_CHUNK)                 // threads of a workgroup = columns of a column block
#define FIG_SQ_RG 8                                  // reads of a row group: their weight rows are in LDS together
#define FIG_SQ_NOFF (FIG_SQ_NT + FIG_RS_MAXL - 1)    // offsets that can touch a column block: xb - 199 .. xb + 255
#define FIG_SQ_WIN (FIG_SQ_NOFF + FIG_RS_MAXL - 1)   // columns those placements touch: xb - 199 .. xb + 255 + 199

// p_r(o) of a valid placement with score lr, for a read with greatest score M (above -inf) and normaliser Z: 0.0 below the cut
FIG_P_HD inline double fig_softqual_weight(double lr, double M, double Z) {
    const double d = lr - M;
    if (!fig_softqual_active(d)) return 0.0;
    return exp10(d) / Z;
}

// Column x against one read of `len` bases: prow[top - j] is the weight of the placement that puts base j on the column (the
// caller keeps top - j inside the row for 0 <= j < len; 0.0 = no such active placement).  Bases in ascending j; a base outside
// ACGT and a weight of 0.0 add nothing.  c0..c3: wcount of the column, a0..a3: eloglik.  w: the read's 2-bit words followed by its
// N-mask words; lm / le: log10(1 - e[k]) / log10(e[k]); lt: log10(T[true][read]) as [true * 4 + read].
template <typename WP, typename PP, typename DP>
FIG_P_HD inline void fig_softqual_add_read(double &c0, double &c1, double &c2, double &c3, double &a0, double &a1, double &a2, double &a3,
                                           int len, int rev, WP w, PP prow, int top, DP lm, DP le, DP lt) {
    for (int j = 0; j < len; j++) {
        int s, k;
        const bool acgt = fig_rs_base(w, len, rev, j, s, k);
        const double p = prow[top - j];
        if (!acgt || p == 0.0) continue;
        const double m = lm[k], e = le[k];
        // (+ 0.0 leaves a count as it is; an if-chain on s makes the back end keep the four counts in scratch)
        c0 = c0 + (s == 0 ? p : 0.0); c1 = c1 + (s == 1 ? p : 0.0); c2 = c2 + (s == 2 ? p : 0.0); c3 = c3 + (s == 3 ? p : 0.0);
        a0 = a0 + p * (s == 0 ? m : e + lt[0 + s]);
        a1 = a1 + p * (s == 1 ? m : e + lt[4 + s]);
        a2 = a2 + p * (s == 2 ? m : e + lt[8 + s]);
        a3 = a3 + p * (s == 3 ? m : e + lt[12 + s]);
    }
}

#ifdef __HIPCC__
// What the kernel reads (all device memory; every array is read through an address-space-1 view) and the arrays it writes.
struct FigSoftqArgs {
    const FigDevGap *gaps;           // the resident batch's descriptors: nU, uBase, gapStart, G0, flankOff
    const int32_t *u_len, *u_aux, *u_pos;
    const int64_t *u_woff;
    const uint32_t *packed;
    const uint8_t *flank;
    const int32_t *draw_pos;         // [n_ureads] drawn offset, INT32_MIN = not drawn
    const int32_t *items;            // [gridDim.x * 2] {gap, first column of the block}
    const int32_t *ncol;             // [n_gaps] bases of the gap's string
    const int64_t *str_off;          // [n_gaps + 1] the caller's (compacted) string offsets
    const char *str;                 // the caller's strings
    const double *tabs;              // lm[L] | le[L] | lt[16]
    const double *li;                // [max_insert]
    int32_t L, Tmin, Tmax, max_insert;
    const double *placed;            // ll_drawn | ll_other | sum_other, [n_ureads] each: what fig_placement_kernel wrote for the scored reads
    int64_t n_ureads;
    double *out;                     // wcount | eloglik, `plane` doubles each, [(str_off[g] + x) * 4 + s / b]; then as int32 [gridDim.x]: the
    int64_t plane;                   // active placements whose offset the block owns (each placement is owned by one block)
};

// One workgroup per (gap that is on, block of 256 of its columns); a lane owns column x = xb + tid.  The block's column codes
// xb - 199 .. xb + 255 + 199 are staged once; the gap's reads pass through LDS in chunks of 64 and, within a chunk, in row groups of
// 8.  Phase A deals the 455 offsets that can touch the block over the lanes, read by read (the read is wave-uniform as in
// fig_placement_kernel), and leaves p_r(o) in the read's LDS row.  Phase B: every lane walks the row group's reads in order, j
// ascending, one LDS read of the weight per base -- consecutive lanes, consecutive addresses -- into eight register accumulators.
// No atomics: the order of the additions is fixed.
__global__ void __launch_bounds__(FIG_SQ_NT) fig_softqual_kernel(FigSoftqArgs A) {
    __shared__ double s_tab[FIG_RS_TAB];
    __shared__ int4 s_hdr[FIG_RS_CHUNK];                         // {length (0 = takes no part), reversed, left anchor, -}
    __shared__ long long s_isz0[FIG_RS_CHUNK];                   // insert size at o = 0
    __shared__ double s_M[FIG_RS_CHUNK], s_Z[FIG_RS_CHUNK];
    __shared__ uint32_t s_w[FIG_RS_CHUNK][FIG_RS_WORDS];
    __shared__ uint8_t s_S[(FIG_SQ_WIN + 15) & ~15];
    __shared__ double s_p[FIG_SQ_RG][FIG_SQ_NOFF + 1];
    __shared__ int32_t s_cnt[FIG_SQ_NT / 64];
    __shared__ double *s_out[3];                                 // the gap's wcount and eloglik and the counts: read back at the end, so that
                                                                 // the three do not sit in scalar registers across every loop
    const int tid = (int)threadIdx.x;
    const int g = ((fig_rs_gi32p)A.items)[2 * blockIdx.x], xb = ((fig_rs_gi32p)A.items)[2 * blockIdx.x + 1];
    fig_rs_ggapp gp = (fig_rs_ggapp)A.gaps + g;
    const int n = ((fig_rs_gi32p)A.ncol)[g];
    const int nreads = gp->nU;
    const long long rbase = gp->uBase;
    const long long gap_start = gp->gapStart;
    const int G0 = gp->G0;
    const int L = A.L, Tmin = A.Tmin, Tmax = A.Tmax, max_insert = A.max_insert;
    const long long so = ((fig_rs_gi64p)A.str_off)[g];
    fig_rs_gu8p fl = (fig_rs_gu8p)A.flank + gp->flankOff;
    fig_rs_gcp str = (fig_rs_gcp)A.str + so;
    fig_rs_gcdp li = (fig_rs_gcdp)A.li;
    fig_rs_stage_tables(s_tab, A.tabs, L, tid, FIG_SQ_NT);
    fig_rs_ldp lm = (fig_rs_ldp)&s_tab[0], le = (fig_rs_ldp)&s_tab[L], lt = (fig_rs_ldp)&s_tab[2 * FIG_RS_MAXL];
    const int o_first = xb - (FIG_RS_MAXL - 1);                  // the offset of weight index 0, and the column of s_S[0]
    for (int i = tid; i < FIG_SQ_WIN; i += FIG_SQ_NT) s_S[i] = (uint8_t)fig_placement_column(o_first + i, n, fl, str);
    const int x = xb + tid;
    if (tid == FIG_SQ_NT - 1) { s_out[0] = A.out + so * 4; s_out[1] = A.out + A.plane + so * 4; s_out[2] = A.out + 2 * A.plane; }
    double c0 = 0.0, c1 = 0.0, c2 = 0.0, c3 = 0.0, a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    int cnt = 0;
    for (int ch = 0; ch < nreads; ch += FIG_RS_CHUNK) {
        const int nc = min(FIG_RS_CHUNK, nreads - ch);
        {   // stage the chunk
            int r, o, len;
            if (fig_rs_stage_reads(s_w, tid, nc, L, A.u_len, A.u_woff, A.packed, A.draw_pos, rbase + ch, rbase + ch, r, o, len)) {
                const long long ri = rbase + ch + r;
                double M = 0.0, Z = 0.0;
                bool part = o != INT32_MIN && len > 0;
                if (part) part = fig_softqual_mz(((fig_rs_gcdp)A.placed)[ri], ((fig_rs_gcdp)A.placed)[A.n_ureads + ri], ((fig_rs_gcdp)A.placed)[2 * A.n_ureads + ri], M, Z);
                const long long pos = ((fig_rs_gi32p)A.u_pos)[ri];
                s_hdr[r] = make_int4(part ? len : 0, ((fig_rs_gi32p)A.u_aux)[ri] & 1, pos < gap_start ? 1 : 0, 0);
                s_isz0[r] = fig_placement_isz(pos, gap_start, G0, n, len, 0);
                s_M[r] = M; s_Z[r] = Z;
            }
        }
        __syncthreads();
        for (int r0 = 0; r0 < nc; r0 += FIG_SQ_RG) {
            const int nr = min(FIG_SQ_RG, nc - r0);
            for (int rr = 0; rr < nr; rr++) {                    // phase A: the weight rows of the row group
                const int4 h = s_hdr[r0 + rr];
                const int len = h.x;
                if (len == 0) continue;
                const double M = s_M[r0 + rr], Z = s_Z[r0 + rr];
                for (int oi = tid; oi < FIG_SQ_NOFF; oi += FIG_SQ_NT) {
                    const int o = o_first + oi;
                    // isz(o) = isz(0) + o for a left anchor, isz(0) - o for a right one (fig_placement_isz is linear in o)
                    const long long isz = h.z ? s_isz0[r0 + rr] + o : s_isz0[r0 + rr] - o;
                    const bool valid = o >= -(len - 1) && o <= n - 1 && o + len - 1 >= xb && fig_placement_valid(isz, Tmin, Tmax, max_insert);
                    double p = 0.0;
                    if (valid) p = fig_softqual_weight(fig_placement_score(li[isz], (fig_rs_lu8p)&s_S[oi], len, h.y, (fig_rs_lu32p)&s_w[r0 + rr][0], lm, le, lt), M, Z);
                    cnt += (p != 0.0 && (o >= xb || xb == 0)) ? 1 : 0;
                    s_p[rr][oi] = p;
                }
            }
            __syncthreads();
            if (x < n) {
                for (int rr = 0; rr < nr; rr++) {                // phase B: this lane's column against every read of the row group
                    const int4 h = s_hdr[r0 + rr];
                    fig_softqual_add_read(c0, c1, c2, c3, a0, a1, a2, a3, h.x, h.y, (fig_rs_lu32p)&s_w[r0 + rr][0], (fig_rs_ldp)&s_p[rr][0], tid + FIG_RS_MAXL - 1, lm, le, lt);
                }
            }
            __syncthreads();
        }
    }
    for (int m = 32; m >= 1; m >>= 1) cnt += __shfl_xor(cnt, m, 64);
    if ((tid & 63) == 0) s_cnt[tid >> 6] = cnt;
    __syncthreads();
    if (x < n) {
        fig_rs_gdp wc = (fig_rs_gdp)s_out[0] + (long long)x * 4, el = wc + (long long)(s_out[1] - s_out[0]);
        wc[0] = c0; wc[1] = c1; wc[2] = c2; wc[3] = c3;
        el[0] = a0; el[1] = a1; el[2] = a2; el[3] = a3;
    }
    if (tid == 0) ((fig_rs_gip)s_out[2])[blockIdx.x] = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
}
#endif
#endif
