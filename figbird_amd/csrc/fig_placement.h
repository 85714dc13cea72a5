// fig_placement.h -- placement confidence per drawn unmapped read (fig_batch_placement): every placement of every
// drawn read of a gap is scored against the EMITTED sequence (string + the batch's flank codes) under the run's own error model
// and insert-size distribution, and per read the drawn placement is set against the best other one.  A score only ADDS entries of
// the log10 tables the host built (fig_quality_host.h, fig_placement_host.h), base by base in ascending j, one IEEE double
// addition each, and the rest is comparisons: ll_drawn, ll_other, off_other and n_valid are reproducible bit for bit.  The kernel
// sits beside the fill: it reads the resident batch and writes five arrays of its own.
//
// The arithmetic of one (read, placement) pair is one __host__ __device__ function; a plain C++ build compiles the same text.  The
// kernel is defined where FIG_PLACEMENT_KERNEL is (fig_abi.hip, whose module owns it); the other kernels' units take the column and
// score functions and the wave reductions without it.
#ifndef FIG_PLACEMENT_H
#define FIG_PLACEMENT_H
#include <stdint.h>
#include "fig_placement_host.h"
#include "fig_readstage.h"

#define FIG_P_NT (4 * FIG_RS_CHUNK)  // threads of a workgroup = offsets of a tile (four waves of 64); a work item is one chunk of reads
#define FIG_P_FLANK FIG_FLANK       // flank codes kept either side of a gap (fig_types.h)
#define FIG_P_WIN (FIG_P_NT + FIG_RS_MAXL - 1)       // columns a tile's placements touch
#define FIG_P_LQ (-0x1.34413509f79ffp-1)             // log10(1/4): an N column under a uniform prior over its base

// Column x of the gap's sequence as a code 0..4 (A C G T N): flank codes left of the string and right of it (fl[k-1] = column -k,
// fl[FIG_P_FLANK + k] = column n + k, N beyond the window), the emitted byte in between.
template <typename FP, typename SP>
FIG_P_HD inline int fig_placement_column(int x, int n, FP fl, SP str) {
    if (x < 0) return -x <= FIG_P_FLANK ? (int)fl[-x - 1] : 4;
    if (x >= n) return x - n < FIG_P_FLANK ? (int)fl[FIG_P_FLANK + (x - n)] : 4;
    const char c = (char)str[x];
    return c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : c == 'T' ? 3 : 4;
}

// Lr of one placement: `lr` comes in as li[isz(o)]; base j of the read sits on S[j] (S: column codes from the placement's first
// column on).  w: the read's 2-bit words followed by its N-mask words; lm / le: log10(1 - e[k]) / log10(e[k]);
// lt: log10(T[column][read]) as [column * 4 + read].
template <typename SP, typename WP, typename DP>
FIG_P_HD inline double fig_placement_score(double lr, SP S, int len, int rev, WP w, DP lm, DP le, DP lt) {
    for (int j = 0; j < len; j++) {
        int s, k;
        if (!fig_rs_base(w, len, rev, j, s, k)) continue;
        const int c = (int)S[j];
        lr = lr + (c > 3 ? FIG_P_LQ : c == s ? lm[k] : le[k] + lt[(c & 3) * 4 + s]);
    }
    return lr;
}

#ifdef __HIPCC__
// What the kernel reads (all device memory; every array is read through an address-space-1 view) and the arrays it writes.
struct FigPlaceArgs {
    const FigDevGap *gaps;           // the resident batch's descriptors: nU, uBase, gapStart, G0, flankOff
    const int32_t *u_len, *u_aux, *u_pos;
    const int64_t *u_woff;
    const uint32_t *packed;
    const uint8_t *flank;
    const int32_t *draw_pos;         // [n_ureads] drawn offset, INT32_MIN = not drawn
    const int32_t *items;            // [gridDim.x * 2] {gap, first read of the chunk within the gap}
    const int32_t *ncol;             // [n_gaps] bases of the gap's string
    const int64_t *str_off;          // [n_gaps + 1] the caller's (compacted) string offsets
    const char *str;                 // the caller's strings
    const double *tabs;              // lm[L] | le[L] | lt[16]
    const double *li;                // [max_insert]
    int32_t L, Tmin, Tmax, max_insert;
    double *ll_drawn, *ll_other, *sum_other;   // [n_ureads], written for scored reads only
    int32_t *off_other, *n_valid;
};

__device__ inline double fig_p_wave_max(double v) {
    for (int m = 32; m >= 1; m >>= 1) { const double u = __shfl_xor(v, m, 64); v = u > v ? u : v; }
    return v;
}
__device__ inline double fig_p_wave_sum(double v) {
    for (int m = 32; m >= 1; m >>= 1) v = v + __shfl_xor(v, m, 64);
    return v;
}

#ifdef FIG_PLACEMENT_KERNEL
// One workgroup per (gap that is on, chunk of 64 of its reads).  The chunk's reads are staged in LDS once.  The offsets
// -(200-1) .. n-1 pass in tiles of 256: a lane owns offset o = x0 + tid, the tile's columns x0 .. x0 + 256 + 198 are staged as
// codes, and the waves walk the staged reads -- length, orientation, anchor, drawn offset and every read base are wave-uniform, a
// lane reads its column's code and adds one of five wave-uniform terms.  Pass 1 reduces per read the greatest score over the
// valid placements other than the drawn one, the first offset that attains it, and the number of valid placements: inside a wave
// by shuffles and a ballot, across tiles in the wave's own LDS slot, across the four waves by one thread per read.  Pass 2 scores
// again and sums 10^(Lr - M).  No atomics.
__global__ void __launch_bounds__(FIG_P_NT) fig_placement_kernel(FigPlaceArgs A) {
    __shared__ double s_tab[FIG_RS_TAB];
    __shared__ int4 s_hdr[FIG_RS_CHUNK];                         // {drawn offset, length (0 = not scored), reversed, left anchor}
    __shared__ long long s_isz0[FIG_RS_CHUNK];                   // insert size at o = 0
    __shared__ uint32_t s_w[FIG_RS_CHUNK][FIG_RS_WORDS];
    __shared__ uint8_t s_S[(FIG_P_WIN + 15) & ~15];
    __shared__ double s_pmax[FIG_P_NT / 64][FIG_RS_CHUNK], s_psum[FIG_P_NT / 64][FIG_RS_CHUNK], s_drawn[FIG_RS_CHUNK], s_M[FIG_RS_CHUNK];
    __shared__ int32_t s_poff[FIG_P_NT / 64][FIG_RS_CHUNK], s_pcnt[FIG_P_NT / 64][FIG_RS_CHUNK];
    const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int g = ((fig_rs_gi32p)A.items)[2 * blockIdx.x], c0 = ((fig_rs_gi32p)A.items)[2 * blockIdx.x + 1];
    fig_rs_ggapp gp = (fig_rs_ggapp)A.gaps + g;
    const int n = ((fig_rs_gi32p)A.ncol)[g];
    const int nc = min(FIG_RS_CHUNK, gp->nU - c0);
    const long long rbase = gp->uBase + c0;
    const long long gap_start = gp->gapStart;
    const int G0 = gp->G0;
    const int L = A.L, Tmin = A.Tmin, Tmax = A.Tmax, max_insert = A.max_insert;
    fig_rs_gu8p fl = (fig_rs_gu8p)A.flank + gp->flankOff;
    fig_rs_gcp str = (fig_rs_gcp)A.str + ((fig_rs_gi64p)A.str_off)[g];
    fig_rs_gcdp li = (fig_rs_gcdp)A.li;
    fig_rs_stage_tables(s_tab, A.tabs, L, tid, FIG_P_NT);
    fig_rs_ldp lm = (fig_rs_ldp)&s_tab[0], le = (fig_rs_ldp)&s_tab[L], lt = (fig_rs_ldp)&s_tab[2 * FIG_RS_MAXL];
    const double ninf = -__builtin_inf();
    {   // stage the chunk
        int r, o, len;
        if (fig_rs_stage_reads(s_w, tid, nc, L, A.u_len, A.u_woff, A.packed, A.draw_pos, rbase, rbase, r, o, len)) {
            const long long pos = ((fig_rs_gi32p)A.u_pos)[rbase + r];
            s_hdr[r] = make_int4(o, o == INT32_MIN ? 0 : len, ((fig_rs_gi32p)A.u_aux)[rbase + r] & 1, pos < gap_start ? 1 : 0);
            s_isz0[r] = fig_placement_isz(pos, gap_start, G0, n, len, 0);
        }
        if (tid < FIG_RS_CHUNK) { s_drawn[tid] = ninf; s_M[tid] = ninf; }
        for (int i = tid; i < (FIG_P_NT / 64) * FIG_RS_CHUNK; i += FIG_P_NT) {
            (&s_pmax[0][0])[i] = ninf; (&s_psum[0][0])[i] = 0.0; (&s_poff[0][0])[i] = INT32_MAX; (&s_pcnt[0][0])[i] = 0;
        }
    }
    __syncthreads();
    const int o_first = -(FIG_RS_MAXL - 1);
    for (int pass = 0; pass < 2; pass++) {
        for (int x0 = o_first; x0 < n; x0 += FIG_P_NT) {
            for (int i = tid; i < FIG_P_WIN; i += FIG_P_NT) s_S[i] = (uint8_t)fig_placement_column(x0 + i, n, fl, str);
            __syncthreads();
            const int o = x0 + tid;
            for (int r = 0; r < nc; r++) {
                const int4 h = s_hdr[r];
                const int len = h.y;
                if (len == 0) continue;
                // isz(o) = isz(0) + o for a left anchor, isz(0) - o for a right one (fig_placement_isz is linear in o)
                const long long isz = h.w ? s_isz0[r] + o : s_isz0[r] - o;
                const bool valid = o >= -(len - 1) && o <= n - 1 && fig_placement_valid(isz, Tmin, Tmax, max_insert);
                double v = ninf;
                if (valid) v = fig_placement_score(li[isz], (fig_rs_lu8p)&s_S[tid], len, h.z, (fig_rs_lu32p)&s_w[r][0], lm, le, lt);
                const bool other = valid && o != h.x;
                if (pass == 0) {
                    if (valid && o == h.x) s_drawn[r] = v;
                    const unsigned long long bv = __ballot(valid);
                    const double wmax = fig_p_wave_max(other ? v : ninf);
                    const unsigned long long bm = __ballot(other && v == wmax);
                    if (lane == 0) {
                        s_pcnt[wave][r] += __popcll(bv);
                        if (bm) {
                            const int first = x0 + wave * 64 + (__ffsll((long long)bm) - 1);
                            const double pm = s_pmax[wave][r];
                            if (wmax > pm || (wmax == pm && first < s_poff[wave][r])) { s_pmax[wave][r] = wmax; s_poff[wave][r] = first; }
                        }
                    }
                } else {
                    const double M = s_M[r];
                    const double t = (other && v > ninf && M > ninf) ? exp10(v - M) : 0.0;
                    const double ws = fig_p_wave_sum(t);
                    if (lane == 0) s_psum[wave][r] += ws;
                }
            }
            __syncthreads();
        }
        if (tid < nc && s_hdr[tid].y != 0) {                               // one thread per scored read: the four waves' slots in wave order
            const long long ri = rbase + tid;
            if (pass == 0) {
                double m = s_pmax[0][tid]; int off = s_poff[0][tid], cnt = s_pcnt[0][tid];
                for (int w = 1; w < FIG_P_NT / 64; w++) {
                    const double pm = s_pmax[w][tid]; const int po = s_poff[w][tid];
                    if (pm > m || (pm == m && po < off)) { m = pm; off = po; }
                    cnt += s_pcnt[w][tid];
                }
                const double d = s_drawn[tid];
                s_M[tid] = d > m ? d : m;
                ((fig_rs_gdp)A.ll_drawn)[ri] = d; ((fig_rs_gdp)A.ll_other)[ri] = m;
                ((fig_rs_gip)A.off_other)[ri] = off == INT32_MAX ? INT32_MIN : off; ((fig_rs_gip)A.n_valid)[ri] = cnt;
            } else {
                double s = s_psum[0][tid];
                for (int w = 1; w < FIG_P_NT / 64; w++) s = s + s_psum[w][tid];
                ((fig_rs_gdp)A.sum_other)[ri] = s;
            }
        }
        __syncthreads();
    }
}
#endif
#endif
#endif
