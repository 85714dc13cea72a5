// fig_readstage.h -- what the post-fill kernels (fig_quality.h, fig_placement.h) share: the sizes of a staged chunk of reads, the
// address-space views of their arguments, the decode of one base of a packed read, and the two staging steps -- the log10 table
// block and up to 64 reads' words into LDS.  The decode is __host__ __device__ and the rest sits under __HIPCC__: a plain C++ build
// (tests/*_main.cpp) compiles the same text of the arithmetic.
#ifndef FIG_READSTAGE_H
#define FIG_READSTAGE_H
#include <stdint.h>
#include "fig_types.h"

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define FIG_RS_HD __host__ __device__
#else
#define FIG_RS_HD
#endif

#define FIG_RS_MAXL FIG_MAX_READLEN  // longest read, and entries of lm / le at most
#define FIG_RS_CHUNK 64              // reads staged in LDS at a time: four lanes each of a workgroup of 256
#define FIG_RS_WORDS ((FIG_RS_MAXL + 15) / 16 + (FIG_RS_MAXL + 31) / 32)   // dwords of a staged read: 2-bit words + N-mask words (pack_read, fig_pack.h)
#define FIG_RS_TAB (2 * FIG_RS_MAXL + 16)                                  // doubles of the staged table block: lm at 0, le at L, lt at 2 * FIG_RS_MAXL

// Base j of a packed read of `len` bases (w: its 2-bit words followed by its N-mask words): false for a base outside ACGT, else
// s: its code 0..3 (A C G T) and k: its index into the error tables -- len-1-j for a read whose mate was reverse-complemented
// (Figbird.cpp:3569-3576), j for every other read.  s and k are set on either path and the N bit is the return value alone: an
// early return inside leaves the callers' loops a merge of "N" with the code that the gfx950 back end does not undo.
template <typename WP>
FIG_RS_HD inline bool fig_rs_base(WP w, int len, int rev, int j, int &s, int &k) {
    const int nw2 = (len + 15) >> 4;
    s = (int)((w[j >> 4] >> ((j & 15) * 2)) & 3u);
    k = rev ? len - 1 - j : j;
    return !((w[nw2 + (j >> 5)] >> (j & 31)) & 1u);
}

#ifdef __HIPCC__
typedef const int32_t __attribute__((address_space(1))) *fig_rs_gi32p;
typedef const int64_t __attribute__((address_space(1))) *fig_rs_gi64p;
typedef const uint8_t __attribute__((address_space(1))) *fig_rs_gu8p;
typedef const char __attribute__((address_space(1))) *fig_rs_gcp;
typedef const uint32_t __attribute__((address_space(1))) *fig_rs_gu32p;
typedef const double __attribute__((address_space(1))) *fig_rs_gcdp;
typedef const FigDevGap __attribute__((address_space(1))) *fig_rs_ggapp;
typedef double __attribute__((address_space(1))) *fig_rs_gdp;
typedef int32_t __attribute__((address_space(1))) *fig_rs_gip;
typedef const uint32_t __attribute__((address_space(3))) *fig_rs_lu32p;
typedef const uint8_t __attribute__((address_space(3))) *fig_rs_lu8p;
typedef const double __attribute__((address_space(3))) *fig_rs_ldp;

// The host's block lm[L] | le[L] | lt[16] (fig_quality_host.h) into s_tab[FIG_RS_TAB], by a workgroup of nt threads; the caller's
// next barrier publishes it.
__device__ __forceinline__ void fig_rs_stage_tables(double (&s_tab)[FIG_RS_TAB], const double *tabs, int L, int tid, int nt) {
    fig_rs_gcdp t = (fig_rs_gcdp)tabs;
    for (int i = tid; i < 2 * L + 16; i += nt) s_tab[i < 2 * L ? i : 2 * FIG_RS_MAXL + (i - 2 * L)] = t[i];
}

// The words of the reads first .. first + nc - 1 (nc <= FIG_RS_CHUNK) into s_w, by a workgroup of 4 * FIG_RS_CHUNK threads: four
// lanes per read, five words each.  True for the one lane per read that writes the caller's header of read r: o is the read's
// entry of the draw plane (dfirst: the chunk's first), len its length clamped to 0 .. L (the packer admits no read longer than
// the model's L <= 200).  The caller's next barrier publishes the words.
__device__ __forceinline__ bool fig_rs_stage_reads(uint32_t (&s_w)[FIG_RS_CHUNK][FIG_RS_WORDS], int tid, int nc, int L, const int32_t *rlen, const int64_t *rwoff,
                                                   const uint32_t *packed, const int32_t *draw_pos, long long first, long long dfirst, int &r, int &o, int &len) {
    const int q = tid & 3;
    r = tid >> 2;
    if (r >= nc) return false;
    o = ((fig_rs_gi32p)draw_pos)[dfirst + r];
    len = min(max(((fig_rs_gi32p)rlen)[first + r], 0), L);
    const int nw = ((len + 15) >> 4) + ((len + 31) >> 5);
    fig_rs_gu32p src = (fig_rs_gu32p)packed + ((fig_rs_gi64p)rwoff)[first + r];
    for (int w = q; w < nw; w += 4) s_w[r][w] = src[w];
    return q == 0;
}
#endif
#endif
