// fig_quality.h -- per-base quality of filled bases (fig_batch_quality): for every column of a gap string the four
// log10-likelihoods of "the true base is A / C / G / T" given the reads of the gap's final placement, under the run's own error
// model -- errorPosDist[k] (reversed index for reverse-strand unmapped reads, Figbird.cpp:3569-3576) and errorTypeProbs[from][to],
// the tables the E-step weighs placements with.  The kernel only ADDS entries of three log10 tables the host built
// (fig_quality_host.h), read by read in ascending read index, one IEEE double addition each: the plane is reproducible bit for
// bit by any restatement that uses the same tables and order.  It sits beside the fill: it reads the resident batch and writes
// one plane of its own.
//
// The arithmetic of one (column, read) pair is one __host__ __device__ function; a plain C++ build compiles the same text.
#ifndef FIG_QUALITY_H
#define FIG_QUALITY_H
#include <stdint.h>
#include "fig_readstage.h"

#define FIG_Q_HD FIG_RS_HD
#define FIG_Q_MAXL FIG_RS_MAXL       // (the bound tests/quality_column_main.cpp puts on its case file)
#define FIG_Q_NT (4 * FIG_RS_CHUNK)  // threads of a workgroup = columns of a column block

// The read index of base j is len-1-j for an unmapped read whose mate was reverse-complemented, j for every other read;
// `aux` is FigDevReads::aux of the read (unmapped: bit 0 = isReverse; partial: the match column, which says nothing here).
FIG_Q_HD inline int fig_quality_reversed(int is_partial, int aux) { return is_partial ? 0 : (aux & 1); }

// Column x against one read at drawn offset o: base j = x - o of the read, if the read covers the column and the base is one of
// ACGT, adds its term to the four accumulators (true base A, C, G, T).  w: the read's 2-bit words followed by its N-mask words;
// lm / le: log10(1 - e[k]) / log10(e[k]); lt: log10(T[true][read]) as [true * 4 + read].  An undrawn read is passed with len 0.
template <typename WP, typename DP>
FIG_Q_HD inline void fig_quality_add_read(double &a0, double &a1, double &a2, double &a3, int x, int o, int len, int rev, WP w, DP lm, DP le, DP lt) {
    const int j = x - o;
    if ((unsigned)j >= (unsigned)len) return;
    int s, k;
    if (!fig_rs_base(w, len, rev, j, s, k)) return;
    const double m = lm[k], e = le[k];
    a0 = a0 + (s == 0 ? m : e + lt[0 + s]);
    a1 = a1 + (s == 1 ? m : e + lt[4 + s]);
    a2 = a2 + (s == 2 ? m : e + lt[8 + s]);
    a3 = a3 + (s == 3 ? m : e + lt[12 + s]);
}

#ifdef __HIPCC__
// What the kernel reads (all device memory; every array is read through an address-space-1 view) and the plane it writes.
struct FigQualArgs {
    const FigDevGap *gaps;           // the resident batch's descriptors: nU / nP, uBase / pBase
    const int32_t *u_len, *u_aux, *p_len;
    const int64_t *u_woff, *p_woff;
    const uint32_t *packed;
    int64_t n_ureads;                // partial read p of gap g is entry n_ureads + gaps[g].pBase + p of draw_pos
    const int32_t *draw_pos;         // [n_ureads + n_preads] drawn offset, INT32_MIN = not drawn
    const int32_t *list;             // [gridDim.x] ids of the gaps that are on
    const int32_t *ncol;             // [n_gaps] columns of the gap's string
    const uint8_t *partial;          // [n_gaps] 1 = the evidence is the gap's partial reads
    const int64_t *str_off;          // [n_gaps + 1] the caller's (compacted) string offsets
    const double *tabs;              // lm[L] | le[L] | lt[16]
    int32_t L;
    double *loglik;                  // [(str_off[g] + x) * 4 + b]
};

// One workgroup per gap that is on.  A lane owns column x = tid + 256 * i; per column block the gap's reads pass through LDS in
// chunks of 64 (offset, length, reverse bit, 2-bit and N-mask words) and every lane walks the staged reads in order, adding into
// four register accumulators.  No atomics: the order of the additions is part of the definition.
__global__ void __launch_bounds__(FIG_Q_NT) fig_quality_kernel(FigQualArgs A) {
    __shared__ double s_tab[FIG_RS_TAB];
    __shared__ int4 s_hdr[FIG_RS_CHUNK];                         // {offset, length (0 = takes no part), reversed, -}
    __shared__ uint32_t s_w[FIG_RS_CHUNK][FIG_RS_WORDS];
    const int tid = (int)threadIdx.x;
    const int g = ((fig_rs_gi32p)A.list)[blockIdx.x];
    fig_rs_ggapp gp = (fig_rs_ggapp)A.gaps + g;
    const int part = ((fig_rs_gu8p)A.partial)[g];
    const int n = ((fig_rs_gi32p)A.ncol)[g];
    const int nreads = part ? gp->nP : gp->nU;
    const long long rbase = part ? gp->pBase : gp->uBase;        // into the mode's FigDevReads arrays
    const long long dbase = part ? A.n_ureads + rbase : rbase;   // into the draw planes
    const long long so = ((fig_rs_gi64p)A.str_off)[g];
    const int L = A.L;
    fig_rs_stage_tables(s_tab, A.tabs, L, tid, FIG_Q_NT);
    fig_rs_ldp lm = (fig_rs_ldp)&s_tab[0], le = (fig_rs_ldp)&s_tab[L], lt = (fig_rs_ldp)&s_tab[2 * FIG_RS_MAXL];
    const int32_t *rlen = part ? A.p_len : A.u_len;
    const int64_t *rwoff = part ? A.p_woff : A.u_woff;
    fig_rs_gi32p raux = (fig_rs_gi32p)A.u_aux;
    fig_rs_gdp out = (fig_rs_gdp)A.loglik;
    for (int xb = 0; xb < n; xb += FIG_Q_NT) {
        const int x = xb + tid;
        double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
        for (int c0 = 0; c0 < nreads; c0 += FIG_RS_CHUNK) {
            const int nc = min(FIG_RS_CHUNK, nreads - c0);
            int r, o, len;
            if (fig_rs_stage_reads(s_w, tid, nc, L, rlen, rwoff, A.packed, A.draw_pos, rbase + c0, dbase + c0, r, o, len))
                s_hdr[r] = make_int4(o == INT32_MIN ? 0 : o, o == INT32_MIN ? 0 : len, fig_quality_reversed(part, part ? 0 : raux[rbase + c0 + r]), 0);
            __syncthreads();
            if (x < n) {
                for (int r = 0; r < nc; r++) {
                    const int4 h = s_hdr[r];
                    fig_quality_add_read(a0, a1, a2, a3, x, h.x, h.y, h.z, (fig_rs_lu32p)&s_w[r][0], lm, le, lt);
                }
            }
            __syncthreads();
        }
        if (x < n) {
            out[(so + x) * 4 + 0] = a0; out[(so + x) * 4 + 1] = a1; out[(so + x) * 4 + 2] = a2; out[(so + x) * 4 + 3] = a3;
        }
    }
}
#endif
#endif
