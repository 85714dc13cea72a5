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

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#include "fig_types.h"
#define FIG_Q_HD __host__ __device__
#else
#define FIG_Q_HD
#endif

#define FIG_Q_NT 256                 // threads of a workgroup = columns of a column block
#define FIG_Q_CHUNK 64               // reads staged in LDS at a time
#define FIG_Q_WORDS 20               // dwords of a staged read: ceil(200/16) 2-bit words + ceil(200/32) N-mask words (pack_read, fig_pack.h)
#define FIG_Q_MAXL 200               // FIG_MAX_READLEN

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
    const int nw2 = (len + 15) >> 4;
    if ((w[nw2 + (j >> 5)] >> (j & 31)) & 1u) return;
    const int s = (int)((w[j >> 4] >> ((j & 15) * 2)) & 3u);
    const int k = rev ? len - 1 - j : j;
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

typedef const int32_t __attribute__((address_space(1))) *fig_q_gi32p;
typedef const int64_t __attribute__((address_space(1))) *fig_q_gi64p;
typedef const uint8_t __attribute__((address_space(1))) *fig_q_gu8p;
typedef const uint32_t __attribute__((address_space(1))) *fig_q_gu32p;
typedef const double __attribute__((address_space(1))) *fig_q_gcdp;
typedef double __attribute__((address_space(1))) *fig_q_gdp;
typedef const uint32_t __attribute__((address_space(3))) *fig_q_lu32p;
typedef const double __attribute__((address_space(3))) *fig_q_ldp;

// One workgroup per gap that is on.  A lane owns column x = tid + 256 * i; per column block the gap's reads pass through LDS in
// chunks of 64 (offset, length, reverse bit, 2-bit and N-mask words) and every lane walks the staged reads in order, adding into
// four register accumulators.  No atomics: the order of the additions is part of the definition.
__global__ void __launch_bounds__(FIG_Q_NT) fig_quality_kernel(FigQualArgs A) {
    __shared__ double s_tab[2 * FIG_Q_MAXL + 16];
    __shared__ int4 s_hdr[FIG_Q_CHUNK];                          // {offset, length (0 = takes no part), reversed, -}
    __shared__ uint32_t s_w[FIG_Q_CHUNK][FIG_Q_WORDS];
    const int tid = (int)threadIdx.x;
    const int g = ((fig_q_gi32p)A.list)[blockIdx.x];
    const FigDevGap __attribute__((address_space(1))) *gp = (const FigDevGap __attribute__((address_space(1))) *)A.gaps + g;
    const int part = ((fig_q_gu8p)A.partial)[g];
    const int n = ((fig_q_gi32p)A.ncol)[g];
    const int nreads = part ? gp->nP : gp->nU;
    const long long rbase = part ? gp->pBase : gp->uBase;        // into the mode's FigDevReads arrays
    const long long dbase = part ? A.n_ureads + rbase : rbase;   // into the draw planes
    const long long so = ((fig_q_gi64p)A.str_off)[g];
    const int L = A.L;
    fig_q_gcdp tabs = (fig_q_gcdp)A.tabs;
    for (int i = tid; i < 2 * L + 16; i += FIG_Q_NT) s_tab[i < 2 * L ? i : 2 * FIG_Q_MAXL + (i - 2 * L)] = tabs[i];
    fig_q_ldp lm = (fig_q_ldp)&s_tab[0], le = (fig_q_ldp)&s_tab[L], lt = (fig_q_ldp)&s_tab[2 * FIG_Q_MAXL];
    fig_q_gi32p rlen = (fig_q_gi32p)(part ? A.p_len : A.u_len);
    fig_q_gi64p rwoff = (fig_q_gi64p)(part ? A.p_woff : A.u_woff);
    fig_q_gi32p raux = (fig_q_gi32p)A.u_aux, dpos = (fig_q_gi32p)A.draw_pos;
    fig_q_gu32p packed = (fig_q_gu32p)A.packed;
    fig_q_gdp out = (fig_q_gdp)A.loglik;
    for (int xb = 0; xb < n; xb += FIG_Q_NT) {
        const int x = xb + tid;
        double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
        for (int c0 = 0; c0 < nreads; c0 += FIG_Q_CHUNK) {
            const int nc = min(FIG_Q_CHUNK, nreads - c0);
            {   // stage: four lanes per read, five words each
                const int r = tid >> 2, q = tid & 3;
                if (r < nc) {
                    const int o = dpos[dbase + c0 + r];
                    int len = rlen[rbase + c0 + r];
                    len = min(max(len, 0), L);                             // (the packer admits no read longer than the model's L <= 200)
                    const int nw = ((len + 15) >> 4) + ((len + 31) >> 5);
                    const long long wo = rwoff[rbase + c0 + r];
                    for (int w = q; w < nw; w += 4) s_w[r][w] = packed[wo + w];
                    if (q == 0) s_hdr[r] = make_int4(o == INT32_MIN ? 0 : o, o == INT32_MIN ? 0 : len, fig_quality_reversed(part, part ? 0 : raux[rbase + c0 + r]), 0);
                }
            }
            __syncthreads();
            if (x < n) {
                for (int r = 0; r < nc; r++) {
                    const int4 h = s_hdr[r];
                    fig_quality_add_read(a0, a1, a2, a3, x, h.x, h.y, h.z, (fig_q_lu32p)&s_w[r][0], lm, le, lt);
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
