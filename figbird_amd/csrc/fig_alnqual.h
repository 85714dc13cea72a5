// fig_alnqual.h -- per-base quality over gapped read alignments (fig_batch_alnqual): fig_quality's planes with base j
// of a read on the column its best band path puts it on, not on column o + j.  Two kernels.  The path kernel runs fig_band.h's band
// forward with back-pointers as fig_indel_kernel does, walks the back-pointers of every aligned read once and writes which base
// sits on which column: the read's column map, one nibble per window column (fig_alnqual_host.h), its span and the five per-read
// values.  The column kernel is fig_quality_kernel with the map between the column and the base: a lane owns a column, the gap's
// reads pass through LDS in ascending read index, and every sum is fig_quality's sum in fig_quality's order.  No atomics: the
// order of the additions is part of the definition and the three counts of a column belong to its lane.
//
// The walk and the step of one (column, read) pair are __host__ __device__ functions; a plain C++ build compiles the same text
// (tests/alnqual_main.cpp).  The kernels are compiled in a translation unit of their own for fig_indel.h's reason
// (fig_alnqual_kernel.hip defines FIG_ALNQUAL_KERNEL; fig_abi.hip sees the argument structs and the two launches only).
#ifndef FIG_ALNQUAL_H
#define FIG_ALNQUAL_H
#include <stdint.h>
#include "fig_alnqual_host.h"
#include "fig_band.h"
#include "fig_placement.h"

#define FIG_AQ_NT (4 * FIG_RS_CHUNK)                 // threads of a workgroup of either kernel

// The raw steps of the path from (len, d_end) to row 0, as fig_indel_traceback takes them, without its normalisation: a DIAG step
// into (i, d) sets nibble i - 1 + d + W of the map to d + W; an INS step leaves no mark and a DEL step leaves its column
// FIG_ALNQ_NONE.  bp(i, d): the back-pointer of cell (i, d), 1 <= i <= len.  The map's bytes in use are FIG_ALNQ_NONE throughout when
// this is called.  d_start: the diagonal at row 0; n_ins / n_del: INS and DEL steps taken.  The two pointers the update never writes
// (INS on d = +W, DEL on d = -W) end the walk where they end fig_indel_traceback's.
template <typename BP, typename MP>
FIG_P_HD inline void fig_alnqual_walk(BP bp, MP map, int len, int d_end, int &d_start, int &n_ins, int &n_del) {
    int i = len, d = d_end;
    n_ins = 0; n_del = 0;
    while (i > 0) {
        const int p = bp(i, d);
        if (p == FIG_ID_DIAG) { fig_alnqual_set_nibble(map, i - 1 + d + FIG_INDEL_W, d + FIG_INDEL_W); i--; }
        else if (p == FIG_ID_INS) { if (d >= FIG_INDEL_W) break; i--; d++; n_ins++; }
        else { if (d <= -FIG_INDEL_W) break; d--; n_del++; }
    }
    d_start = d;
}

#ifdef __HIPCC__
// What the path kernel reads (FigBandIn; items: {gap, first read of the chunk within the gap}) and the arrays it writes.
struct FigAlnPathArgs : FigBandIn {
    uint32_t *map;                   // [n_ureads * FIG_ALNQ_MAPW]; this and the rest are written for aligned reads only
    int32_t *span;                   // [n_ureads * 2] {first, last column of the path}, not clipped to the string
    double *ll_gapped;               // [n_ureads]
    int32_t *n_ins, *n_del, *d_end, *d_start;
};

// What the column kernel reads and the planes it writes.
struct FigAlnColArgs {
    const FigDevGap *gaps;
    const int32_t *u_len, *u_aux;
    const int64_t *u_woff;
    const uint32_t *packed;
    const int32_t *draw_pos;
    const int32_t *list;             // [gridDim.x] ids of the gaps that are on
    const int32_t *ncol;
    const int64_t *str_off;
    const char *str;
    const double *tabs;
    int32_t L;
    const uint32_t *map;             // the path kernel's
    const int32_t *span;
    double *loglik;                  // [(str_off[g] + x) * 4 + b]
    int32_t *depth, *agree, *skip;   // [str_off[g] + x]
};

// the two launches (fig_alnqual_kernel.hip): `items` chunks, then `gaps` gaps
hipError_t fig_alnqual_path_launch(const FigAlnPathArgs &A, unsigned items, hipStream_t stream);
hipError_t fig_alnqual_column_launch(const FigAlnColArgs &A, unsigned gaps, hipStream_t stream);

#ifdef FIG_ALNQUAL_KERNEL
typedef uint32_t __attribute__((address_space(1))) *fig_aq_gu32w;
typedef const uint8_t __attribute__((address_space(3))) *fig_aq_lu8p;

// fig_indel_kernel's mapping: one workgroup per (gap that is on, chunk of 64 of its reads), 16 reads at a time, a read's band in one
// 16-lane row of a wave (fig_band_forward with back-pointers).  What differs is the end: the 16 lanes of a row blank the read's map
// in LDS, one lane takes the end and walks back into it (the flat path when every gapped path is -inf), and the 16 lanes copy the
// map out, a dword per store.
__global__ void __launch_bounds__(FIG_AQ_NT) fig_alnqual_path_kernel(FigAlnPathArgs A) {
    __shared__ double s_tab[FIG_RS_TAB];
    __shared__ double s_id[2 * FIG_RS_MAXL];                     // lI at 0, lD at FIG_RS_MAXL
    __shared__ int4 s_hdr[FIG_RS_CHUNK];                         // {drawn offset, length, reversed, aligned}
    __shared__ uint32_t s_w[FIG_RS_CHUNK][FIG_RS_WORDS];
    __shared__ uint32_t s_bp[FIG_ID_GROUP][FIG_RS_MAXL];         // row i at [i - 1]: bit q = INS, bit 16 + q = DEL of diagonal q - 7
    __shared__ uint8_t s_S[FIG_ID_GROUP][FIG_ID_WIN];            // [x - (o - 7)]
    __shared__ double s_H[FIG_ID_GROUP][FIG_ID_ROW];
    __shared__ uint32_t s_map[FIG_ID_GROUP][FIG_ALNQ_MAPW];
    const int tid = (int)threadIdx.x, rr = tid / FIG_ID_ROW, q = tid & (FIG_ID_ROW - 1);
    const int g = ((fig_rs_gi32p)A.items)[2 * blockIdx.x], c0 = ((fig_rs_gi32p)A.items)[2 * blockIdx.x + 1];
    fig_rs_ggapp gp = (fig_rs_ggapp)A.gaps + g;
    const int n = ((fig_rs_gi32p)A.ncol)[g];
    const int nc = min(FIG_RS_CHUNK, gp->nU - c0);
    const long long rbase = gp->uBase + c0;
    const int L = A.L;
    fig_rs_gu8p fl = (fig_rs_gu8p)A.flank + gp->flankOff;
    fig_rs_gcp str = (fig_rs_gcp)A.str + ((fig_rs_gi64p)A.str_off)[g];
    fig_rs_stage_tables(s_tab, A.tabs, L, tid, FIG_AQ_NT);
    fig_band_stage_id(s_id, A.tabs_id, L, tid, FIG_AQ_NT);
    fig_rs_ldp lm = (fig_rs_ldp)&s_tab[0], le = (fig_rs_ldp)&s_tab[L], lt = (fig_rs_ldp)&s_tab[2 * FIG_RS_MAXL];
    fig_rs_ldp lI = (fig_rs_ldp)&s_id[0], lD = (fig_rs_ldp)&s_id[FIG_RS_MAXL];
    const double ninf = -__builtin_inf();
    {   // stage the chunk
        int r, o, len;
        if (fig_rs_stage_reads(s_w, tid, nc, L, A.u_len, A.u_woff, A.packed, A.draw_pos, rbase, rbase, r, o, len))
            s_hdr[r] = make_int4(o, len, ((fig_rs_gi32p)A.u_aux)[rbase + r] & 1, fig_indel_aligned(o, len, n) ? 1 : 0);
    }
    __syncthreads();
    for (int g0 = 0; g0 < nc; g0 += FIG_ID_GROUP) {
        const int r = g0 + rr;
        const int4 h4 = r < nc ? s_hdr[r] : make_int4(0, 0, 0, 0);
        const int o = h4.x, len = h4.y, rev = h4.z;
        const bool al = h4.w != 0;
        fig_rs_lu32p w = (fig_rs_lu32p)&s_w[r < nc ? r : 0][0];
        if (al) fig_band_window(&s_S[rr][0], o, len, q, [&](int x) { return fig_placement_column(x, n, fl, str); });
        for (int i = q; i < FIG_ALNQ_MAPW; i += FIG_ID_ROW) s_map[rr][i] = 0xffffffffu;
        __syncthreads();
        s_H[rr][q] = fig_band_forward<true, false>((fig_rs_lu8p)&s_S[rr][0], w, al, len, rev, q, lm, le, lt, lI, lD, &s_bp[rr][0], nullptr);
        __syncthreads();
        if (al && q == 0) {
            int d_end, d_start, n_ins, n_del, lo, hi;
            uint8_t *map = (uint8_t *)&s_map[rr][0];
            const double best = fig_indel_end((fig_rs_ldp)&s_H[rr][0], d_end);
            if (best > ninf) {
                const uint32_t *row = &s_bp[rr][0];
                auto bpf = [row](int i, int d) { return fig_band_bp(row, i, d); };
                fig_alnqual_walk(bpf, map, len, d_end, d_start, n_ins, n_del);
            } else fig_alnqual_flat(map, len, d_start, d_end, n_ins, n_del);
            fig_alnqual_span(o, len, d_start, d_end, lo, hi);
            const long long ri = rbase + r;
            ((fig_rs_gdp)A.ll_gapped)[ri] = best;
            ((fig_rs_gip)A.n_ins)[ri] = n_ins; ((fig_rs_gip)A.n_del)[ri] = n_del; ((fig_rs_gip)A.d_end)[ri] = d_end; ((fig_rs_gip)A.d_start)[ri] = d_start;
            ((fig_rs_gip)A.span)[2 * ri] = lo; ((fig_rs_gip)A.span)[2 * ri + 1] = hi;
        }
        __syncthreads();
        if (al) {
            fig_aq_gu32w dst = (fig_aq_gu32w)A.map + (rbase + r) * FIG_ALNQ_MAPW;
            for (int i = q; i < FIG_ALNQ_MAPW; i += FIG_ID_ROW) dst[i] = s_map[rr][i];
        }
        __syncthreads();
    }
}

// fig_quality_kernel's mapping: one workgroup per gap that is on, a lane owns column x = tid + 256 * i, and per column block the gap's
// reads pass through LDS in chunks of 64 -- header, span, 2-bit and N-mask words, map -- and every lane walks the staged reads in
// order.  Plain stores at the end of the block.
__global__ void __launch_bounds__(FIG_AQ_NT) fig_alnqual_column_kernel(FigAlnColArgs A) {
    __shared__ double s_tab[FIG_RS_TAB];
    __shared__ int4 s_hdr[FIG_RS_CHUNK];                         // {offset, length (0 = takes no part), reversed, -}
    __shared__ int2 s_span[FIG_RS_CHUNK];
    __shared__ uint32_t s_w[FIG_RS_CHUNK][FIG_RS_WORDS];
    __shared__ uint32_t s_map[FIG_RS_CHUNK][FIG_ALNQ_MAPW];
    const int tid = (int)threadIdx.x;
    const int g = ((fig_rs_gi32p)A.list)[blockIdx.x];
    fig_rs_ggapp gp = (fig_rs_ggapp)A.gaps + g;
    const int n = ((fig_rs_gi32p)A.ncol)[g];
    const int nreads = gp->nU;
    const long long rbase = gp->uBase;
    const long long so = ((fig_rs_gi64p)A.str_off)[g];
    const int L = A.L;
    fig_rs_stage_tables(s_tab, A.tabs, L, tid, FIG_AQ_NT);
    fig_rs_ldp lm = (fig_rs_ldp)&s_tab[0], le = (fig_rs_ldp)&s_tab[L], lt = (fig_rs_ldp)&s_tab[2 * FIG_RS_MAXL];
    fig_rs_gdp out = (fig_rs_gdp)A.loglik;
    for (int xb = 0; xb < n; xb += FIG_AQ_NT) {
        const int x = xb + tid;
        const int call = x < n ? fig_alnqual_call_code(((fig_rs_gcp)A.str)[so + x]) : 4;
        double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
        int depth = 0, agree = 0, skip = 0;
        for (int c0 = 0; c0 < nreads; c0 += FIG_RS_CHUNK) {
            const int nc = min(FIG_RS_CHUNK, nreads - c0);
            int r, o, len;
            if (fig_rs_stage_reads(s_w, tid, nc, L, A.u_len, A.u_woff, A.packed, A.draw_pos, rbase + c0, rbase + c0, r, o, len)) {
                const bool al = fig_indel_aligned(o, len, n);
                s_hdr[r] = make_int4(al ? o : 0, al ? len : 0, ((fig_rs_gi32p)A.u_aux)[rbase + c0 + r] & 1, 0);
                // an unaligned read has no entry of the path kernel's: an empty span
                s_span[r] = al ? make_int2(((fig_rs_gi32p)A.span)[2 * (rbase + c0 + r)], ((fig_rs_gi32p)A.span)[2 * (rbase + c0 + r) + 1]) : make_int2(0, -1);
            }
            {   // the maps of the aligned reads: four lanes per read, as the words
                const int rq = tid >> 2;
                if (rq < nc) {
                    const int o4 = ((fig_rs_gi32p)A.draw_pos)[rbase + c0 + rq];
                    const int l4 = min(max(((fig_rs_gi32p)A.u_len)[rbase + c0 + rq], 0), L);
                    if (fig_indel_aligned(o4, l4, n)) {
                        fig_rs_gu32p src = (fig_rs_gu32p)A.map + (rbase + c0 + rq) * FIG_ALNQ_MAPW;
                        const int nw = (fig_alnqual_map_bytes(l4) + 3) >> 2;
                        for (int i = tid & 3; i < nw; i += 4) s_map[rq][i] = src[i];
                    }
                }
            }
            __syncthreads();
            if (x < n) {
                for (int r = 0; r < nc; r++) {
                    const int4 h = s_hdr[r];
                    const int2 sp = s_span[r];
                    const int what = fig_alnqual_add_read(a0, a1, a2, a3, x, call, h.x, h.y, h.z, sp.x, sp.y, (fig_rs_lu32p)&s_w[r][0], (fig_aq_lu8p)&s_map[r][0], lm, le, lt);
                    skip += what == FIG_ALNQ_SKIP; depth += what >= FIG_ALNQ_BASE; agree += what == FIG_ALNQ_AGREE;
                }
            }
            __syncthreads();
        }
        if (x < n) {
            out[(so + x) * 4 + 0] = a0; out[(so + x) * 4 + 1] = a1; out[(so + x) * 4 + 2] = a2; out[(so + x) * 4 + 3] = a3;
            ((fig_rs_gip)A.depth)[so + x] = depth; ((fig_rs_gip)A.agree)[so + x] = agree; ((fig_rs_gip)A.skip)[so + x] = skip;
        }
    }
}
#endif
#endif
#endif
