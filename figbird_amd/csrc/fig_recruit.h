// fig_recruit.h -- the kernel of the recruiting pass (fig_batch_recruit; include/figbird_hip.h: fig_read_recruit):
// every UNDRAWN read of a gap is scored on all its placements against the emitted sequence (fig_placement.h's tile loop and
// fig_placement_score), the best valid placement seeds the banded dynamic program of fig_band.h, and the best valid placement
// outside the band around the seed is reported beside it.  A score only ADDS entries of the log10 tables the host built, one IEEE
// double addition each, and the rest is comparisons: every output is reproducible bit for bit.  There is no exp10, no traceback and
// no atomic.  The kernel sits beside the fill: it reads the resident batch and writes nine arrays of its own.
//
// The score of one (read, placement), the band's cell and the order of two (score, offset) pairs are __host__ __device__ functions
// (fig_placement.h, fig_band.h, fig_recruit_host.h); a plain C++ build compiles the same text (tests/recruit_read_main.cpp).  Like
// fig_indel_kernel the kernel is compiled in a translation unit of its own (fig_recruit_kernel.hip defines FIG_RECRUIT_KERNEL;
// fig_abi.hip sees the argument struct and fig_recruit_launch only).
#ifndef FIG_RECRUIT_H
#define FIG_RECRUIT_H
#include <stdint.h>
#include "fig_recruit_host.h"
#include "fig_band.h"
#include "fig_placement.h"

#define FIG_RC_NT FIG_P_NT                           // threads of a workgroup = offsets of a tile; a work item is one chunk of reads
#define FIG_RC_WAVES (FIG_RC_NT / 64)

// What a wave found in one tile for one read -- the greatest score of its lanes that take part and the first offset that attains it --
// into the wave's slot; `any`: some lane took part
FIG_P_HD inline void fig_recruit_wave_slot(bool any, double wmax, int first, double &slot_v, int &slot_o) {
    if (any) fig_recruit_take(wmax, first, slot_v, slot_o);
}

#ifdef __HIPCC__
// What the kernel reads (all device memory; every array is read through an address-space-1 view) and the arrays it writes.  The
// members of FigBandIn in the order this kernel has always had them, u_pos and li among them: with FigBandIn as the struct's base
// the kernel measured 1.4 - 2.4 % slower (profiles/band/README.md); fig_batch_recruit copies them out of a FigBandIn.
struct FigRecruitArgs {
    const FigDevGap *gaps;           // the resident batch's descriptors: nU, uBase, gapStart, G0, flankOff
    const int32_t *u_len, *u_aux, *u_pos;
    const int64_t *u_woff;
    const uint32_t *packed;
    const uint8_t *flank;
    const int32_t *draw_pos;         // [n_ureads] the caller's offsets: INT32_MIN = a candidate
    const int32_t *items;            // [gridDim.x * 2] {gap, first read of the chunk within the gap}
    const int32_t *ncol;             // [n_gaps] bases of the gap's string
    const int64_t *str_off;          // [n_gaps + 1] the caller's (compacted) string offsets
    const char *str;                 // the caller's strings
    const double *tabs;              // lm[L] | le[L] | lt[16]
    const double *tabs_id;           // lI[L] | lD[L]
    const double *li;                // [max_insert]
    int32_t L, Tmin, Tmax, max_insert;
    double *ll_seed, *ll_second, *ll_flat, *ll_gapped;      // [n_ureads]: ll_seed for candidates of positive length, the rest for seeded reads
    int32_t *off_seed, *n_valid, *off_second, *d_end, *isz_seed;
};

// the launch of fig_recruit_kernel over `items` work items (fig_recruit_kernel.hip)
hipError_t fig_recruit_launch(const FigRecruitArgs &A, unsigned items, hipStream_t stream);

#ifdef FIG_RECRUIT_KERNEL
// One workgroup per (gap that is on, chunk of 64 of its reads with a candidate among them), the chunk staged in LDS once; a read that
// is no candidate has length 0 in its header and takes no part.
//
// Passes 0 and 1 are fig_placement_kernel's tile loop: the offsets -(200-1) .. n-1 pass in tiles of 256, a lane owns offset
// o = x0 + tid, the tile's column codes sit in LDS, and the waves walk the staged reads -- length, orientation, anchor and every read
// base are wave-uniform.  Pass 0 reduces per read the greatest score over the valid placements, the first offset that attains it and
// the number of valid placements: inside a wave by a shuffle-max and a ballot, across tiles in the wave's own LDS slot, across the
// four waves by one thread per read.  Pass 1 does the same over the valid offsets outside off_seed +- 7.  A read that is not seeded
// drops out after pass 0.
//
// Then the band: 16 reads at a time, a read's band in one 16-lane row of a wave (fig_band_forward, forward only, with the flat
// score); one lane per read takes the end and writes the read's values.
__global__ void __launch_bounds__(FIG_RC_NT) fig_recruit_kernel(FigRecruitArgs A) {
    __shared__ double s_tab[FIG_RS_TAB];
    __shared__ double s_id[2 * FIG_RS_MAXL];                     // lI at 0, lD at FIG_RS_MAXL
    __shared__ int4 s_hdr[FIG_RS_CHUNK];                         // {off_seed (after pass 0), length (0 = takes no part), reversed, left anchor}
    __shared__ long long s_isz0[FIG_RS_CHUNK];                   // insert size at o = 0
    __shared__ uint32_t s_w[FIG_RS_CHUNK][FIG_RS_WORDS];
    __shared__ uint8_t s_S[(FIG_P_WIN + 15) & ~15];
    __shared__ double s_pmax[FIG_RC_WAVES][FIG_RS_CHUNK];
    __shared__ int32_t s_poff[FIG_RC_WAVES][FIG_RS_CHUNK], s_pcnt[FIG_RC_WAVES][FIG_RS_CHUNK];
    __shared__ uint8_t s_B[FIG_ID_GROUP][FIG_ID_WIN];            // the band's column codes: [x - (off_seed - 7)]
    __shared__ double s_H[FIG_ID_GROUP][FIG_ID_ROW], s_flat[FIG_ID_GROUP];
    const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63, rr = tid / FIG_ID_ROW, q = tid & (FIG_ID_ROW - 1);
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
    fig_rs_stage_tables(s_tab, A.tabs, L, tid, FIG_RC_NT);
    fig_band_stage_id(s_id, A.tabs_id, L, tid, FIG_RC_NT);
    fig_rs_ldp lm = (fig_rs_ldp)&s_tab[0], le = (fig_rs_ldp)&s_tab[L], lt = (fig_rs_ldp)&s_tab[2 * FIG_RS_MAXL];
    fig_rs_ldp lI = (fig_rs_ldp)&s_id[0], lD = (fig_rs_ldp)&s_id[FIG_RS_MAXL];
    const double ninf = -__builtin_inf();
    {   // stage the chunk
        int r, o, len;
        if (fig_rs_stage_reads(s_w, tid, nc, L, A.u_len, A.u_woff, A.packed, A.draw_pos, rbase, rbase, r, o, len)) {
            const long long pos = ((fig_rs_gi32p)A.u_pos)[rbase + r];
            s_hdr[r] = make_int4(INT32_MIN, fig_recruit_candidate(o) ? len : 0, ((fig_rs_gi32p)A.u_aux)[rbase + r] & 1, pos < gap_start ? 1 : 0);
            s_isz0[r] = fig_placement_isz(pos, gap_start, G0, n, len, 0);
        }
        for (int i = tid; i < FIG_RC_WAVES * FIG_RS_CHUNK; i += FIG_RC_NT) { (&s_pmax[0][0])[i] = ninf; (&s_poff[0][0])[i] = INT32_MAX; (&s_pcnt[0][0])[i] = 0; }
    }
    __syncthreads();
    const int o_first = -(FIG_RS_MAXL - 1);
    for (int pass = 0; pass < 2; pass++) {
        for (int x0 = o_first; x0 < n; x0 += FIG_RC_NT) {
            for (int i = tid; i < FIG_P_WIN; i += FIG_RC_NT) s_S[i] = (uint8_t)fig_placement_column(x0 + i, n, fl, str);
            __syncthreads();
            const int o = x0 + tid;
            for (int r = 0; r < nc; r++) {
                const int4 h = s_hdr[r];
                const int len = h.y;
                if (len == 0) continue;
                // isz(o) = isz(0) + o for a left anchor, isz(0) - o for a right one (fig_placement_isz is linear in o)
                const long long isz = h.w ? s_isz0[r] + o : s_isz0[r] - o;
                const bool valid = o >= -(len - 1) && o <= n - 1 && fig_placement_valid(isz, Tmin, Tmax, max_insert);
                const bool part = valid && (pass == 0 || fig_recruit_outside(o, h.x));
                double v = ninf;
                if (part) v = fig_placement_score(li[isz], (fig_rs_lu8p)&s_S[tid], len, h.z, (fig_rs_lu32p)&s_w[r][0], lm, le, lt);
                const unsigned long long bp = __ballot(part);
                const double wmax = fig_p_wave_max(v);
                const unsigned long long bm = __ballot(part && v == wmax);
                if (lane == 0) {
                    if (pass == 0) s_pcnt[wave][r] += __popcll(bp);
                    fig_recruit_wave_slot(bm != 0, wmax, x0 + wave * 64 + (__ffsll((long long)bm) - 1), s_pmax[wave][r], s_poff[wave][r]);
                }
            }
            __syncthreads();
        }
        if (tid < nc && s_hdr[tid].y != 0) {                               // one thread per read: the four waves' slots in wave order
            const long long ri = rbase + tid;
            double m; int off;
            fig_recruit_reduce(&s_pmax[0][tid], &s_poff[0][tid], FIG_RC_WAVES, FIG_RS_CHUNK, m, off);
            if (pass == 0) {
                int cnt = 0;
                for (int w = 0; w < FIG_RC_WAVES; w++) { cnt += s_pcnt[w][tid]; s_pmax[w][tid] = ninf; s_poff[w][tid] = INT32_MAX; }
                const bool seeded = fig_recruit_seeded(cnt, m);
                ((fig_rs_gdp)A.ll_seed)[ri] = m; ((fig_rs_gip)A.n_valid)[ri] = cnt; ((fig_rs_gip)A.off_seed)[ri] = seeded ? off : INT32_MIN;
                if (seeded) {
                    s_hdr[tid].x = off;
                    ((fig_rs_gip)A.isz_seed)[ri] = (int32_t)(s_hdr[tid].w ? s_isz0[tid] + off : s_isz0[tid] - off);
                } else s_hdr[tid].y = 0;
            } else {
                ((fig_rs_gdp)A.ll_second)[ri] = m; ((fig_rs_gip)A.off_second)[ri] = off == INT32_MAX ? INT32_MIN : off;
            }
        }
        __syncthreads();
    }
    // the band of the seeded reads at their seeds
    for (int g0 = 0; g0 < nc; g0 += FIG_ID_GROUP) {
        const int r = g0 + rr;
        const int4 h4 = r < nc ? s_hdr[r] : make_int4(0, 0, 0, 0);
        const int o = h4.x, len = h4.y, rev = h4.z;
        const bool al = len != 0;
        fig_rs_lu32p w = (fig_rs_lu32p)&s_w[r < nc ? r : 0][0];
        if (al) fig_band_window(&s_B[rr][0], o, len, q, [&](int x) { return fig_placement_column(x, n, fl, str); });
        __syncthreads();
        double flat;
        s_H[rr][q] = fig_band_forward<false, true>((fig_rs_lu8p)&s_B[rr][0], w, al, len, rev, q, lm, le, lt, lI, lD, nullptr, &flat);
        if (q == FIG_INDEL_W) s_flat[rr] = flat;
        __syncthreads();
        if (al && q == 0) {
            int d_end;
            const double best = fig_indel_end((fig_rs_ldp)&s_H[rr][0], d_end);
            const long long ri = rbase + r;
            ((fig_rs_gdp)A.ll_flat)[ri] = s_flat[rr]; ((fig_rs_gdp)A.ll_gapped)[ri] = best; ((fig_rs_gip)A.d_end)[ri] = best > ninf ? d_end : 0;
        }
        __syncthreads();
    }
}
#endif
#endif
#endif
