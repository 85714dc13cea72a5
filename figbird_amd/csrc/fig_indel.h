// fig_indel.h -- indel evidence per filled base (fig_batch_indel): every aligned read of a gap is realigned around
// its drawn offset by the banded dynamic program of fig_band.h against the EMITTED sequence (string + the batch's flank codes), the
// best path is traced back, its insertions and deletions are moved as far left as they go, and per column the reads that ask for an
// edit and the reads that span the column are counted.  Every output is reproducible bit for bit (fig_band.h).  The kernel sits
// beside the fill: it reads the resident batch and writes arrays of its own.
//
// The traceback with its normalisation is a __host__ __device__ function; a plain C++ build compiles the same text.  The kernel is
// compiled in a translation unit of its own (fig_indel_kernel.hip defines FIG_INDEL_KERNEL; fig_abi.hip sees the argument struct and
// fig_indel_launch only): with it in fig_abi.hip's module the back end scheduled the unchanged fill kernels differently, at the same
// resource figures.
#ifndef FIG_INDEL_H
#define FIG_INDEL_H
#include <stdint.h>
#include "fig_band.h"
#include "fig_placement.h"

// The traceback from (len, d_end) to row 0 and the left-normalised events of the path.  bp(i, d): the back-pointer of cell (i, d),
// 1 <= i <= len; S[x - o + W]: the code of column x; w: the read's words (fig_rs_base).  sink.ins(x): an INS run whose next column is
// x (once per column and read); sink.del(x, m): a DEL run over [x, x + m).  d_start: the diagonal at row 0.
template <typename BP, typename SP, typename WP, typename Sink>
FIG_P_HD inline void fig_indel_traceback(BP bp, SP S, WP w, int len, int rev, int o, int d_end, Sink &sink, int &d_start, int &n_ins, int &n_del) {
    int i = len, d = d_end;
    long long last_ins = INT64_MIN;
    n_ins = 0; n_del = 0;
    while (i > 0) {
        const int p = bp(i, d);
        if (p == FIG_ID_DIAG) { i--; continue; }
        int m = 0;
        if (p == FIG_ID_INS) {
            while (i > 0 && d < FIG_INDEL_W && bp(i, d) == FIG_ID_INS) { i--; d++; m++; }
            if (m == 0) break;                                   // (an INS pointer on d = +W: the update never writes one)
            n_ins += m;
            int i0 = i, x = o + i + d;                           // the run is read bases [i0, i0 + m), the next column x
            while (i0 > 0 && bp(i0, d) == FIG_ID_DIAG) {
                int s0, k0, s1, k1;
                const bool ok0 = fig_rs_base(w, len, rev, i0 - 1, s0, k0), ok1 = fig_rs_base(w, len, rev, i0 + m - 1, s1, k1);
                if (s0 != s1 || ok0 != ok1) break;
                i0--; x--;
            }
            if (x != last_ins) sink.ins(x);
            last_ins = x;
        } else {
            while (d > -FIG_INDEL_W && bp(i, d) == FIG_ID_DEL) { d--; m++; }
            if (m == 0) break;                                   // (a DEL pointer on d = -W: the sweep never writes one)
            n_del += m;
            int i0 = i, x = o + i + d;                           // the run is columns [x, x + m)
            while (i0 > 0 && bp(i0, d) == FIG_ID_DIAG && S[x - 1 - o + FIG_INDEL_W] == S[x + m - 1 - o + FIG_INDEL_W]) { i0--; x--; }
            sink.del(x, m);
        }
    }
    d_start = d;
}

#ifdef __HIPCC__
// What the kernel reads (FigBandIn; items: {gap, first read of the chunk within the gap}) and the arrays it writes.
struct FigIndelArgs : FigBandIn {
    double *ll_flat, *ll_gapped;     // [n_ureads], written for aligned reads only
    int32_t *n_ins, *n_del, *d_end, *d_start;
    int32_t *del_reads, *ins_reads, *cover;   // [str_off[n_gaps]], zeroed by the caller, added to atomically
    int32_t *ins_end;                // [n_gaps], likewise
};

// the launch of fig_indel_kernel over `items` work items (fig_indel_kernel.hip)
hipError_t fig_indel_launch(const FigIndelArgs &A, unsigned items, hipStream_t stream);

#ifdef FIG_INDEL_KERNEL
typedef int32_t __attribute__((address_space(1))) *fig_id_gcnt;

// The events of one read into the gap's planes
struct FigIndelSink {
    fig_id_gcnt del_reads, ins_reads, ins_end;       // the gap's first column / its junction counter
    int n;
    __device__ void add(fig_id_gcnt p) { __hip_atomic_fetch_add(p, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    __device__ void ins(int x) { if (x >= 0 && x < n) add(ins_reads + x); else if (x == n) add(ins_end); }
    __device__ void del(int x, int m) { for (int c = x; c < x + m; c++) if (c >= 0 && c < n) add(del_reads + c); }
};

// One workgroup per (gap that is on, chunk of 64 of its reads), the chunk staged in LDS once; 16 reads at a time, a read's band in
// one 16-lane row of a wave (fig_band_forward, with back-pointers and the flat score).  One lane per read takes the end, walks back
// and adds its events to the planes; the 16 lanes of the row add the cover.
__global__ void __launch_bounds__(FIG_ID_NT) fig_indel_kernel(FigIndelArgs A) {
    __shared__ double s_tab[FIG_RS_TAB];
    __shared__ double s_id[2 * FIG_RS_MAXL];                     // lI at 0, lD at FIG_RS_MAXL
    __shared__ int4 s_hdr[FIG_RS_CHUNK];                         // {drawn offset, length, reversed, aligned}
    __shared__ uint32_t s_w[FIG_RS_CHUNK][FIG_RS_WORDS];
    __shared__ uint32_t s_bp[FIG_ID_GROUP][FIG_RS_MAXL];         // row i at [i - 1]: bit q = INS, bit 16 + q = DEL of diagonal q - 7
    __shared__ uint8_t s_S[FIG_ID_GROUP][FIG_ID_WIN];            // [x - (o - 7)]
    __shared__ double s_H[FIG_ID_GROUP][FIG_ID_ROW], s_flat[FIG_ID_GROUP];
    const int tid = (int)threadIdx.x, rr = tid / FIG_ID_ROW, q = tid & (FIG_ID_ROW - 1);
    const int g = ((fig_rs_gi32p)A.items)[2 * blockIdx.x], c0 = ((fig_rs_gi32p)A.items)[2 * blockIdx.x + 1];
    fig_rs_ggapp gp = (fig_rs_ggapp)A.gaps + g;
    const int n = ((fig_rs_gi32p)A.ncol)[g];
    const int nc = min(FIG_RS_CHUNK, gp->nU - c0);
    const long long rbase = gp->uBase + c0;
    const int L = A.L;
    fig_rs_gu8p fl = (fig_rs_gu8p)A.flank + gp->flankOff;
    const long long soff = ((fig_rs_gi64p)A.str_off)[g];
    fig_rs_gcp str = (fig_rs_gcp)A.str + soff;
    fig_rs_stage_tables(s_tab, A.tabs, L, tid, FIG_ID_NT);
    fig_band_stage_id(s_id, A.tabs_id, L, tid, FIG_ID_NT);
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
        __syncthreads();
        double flat;
        s_H[rr][q] = fig_band_forward<true, true>((fig_rs_lu8p)&s_S[rr][0], w, al, len, rev, q, lm, le, lt, lI, lD, &s_bp[rr][0], &flat);
        if (q == FIG_INDEL_W) s_flat[rr] = flat;
        __syncthreads();
        int lo = 0, hi = -1;
        if (al && q == 0) {
            int d_end, d_start = 0, n_ins = 0, n_del = 0;
            const double best = fig_indel_end((fig_rs_ldp)&s_H[rr][0], d_end);
            if (best > ninf) {
                FigIndelSink sink = { (fig_id_gcnt)A.del_reads + soff, (fig_id_gcnt)A.ins_reads + soff, (fig_id_gcnt)A.ins_end + g, n };
                const uint32_t *row = &s_bp[rr][0];
                auto bpf = [row](int i, int d) { return fig_band_bp(row, i, d); };
                fig_indel_traceback(bpf, (fig_rs_lu8p)&s_S[rr][0], w, len, rev, o, d_end, sink, d_start, n_ins, n_del);
                lo = max(o + d_start, 0); hi = min(o + len - 1 + d_end, n - 1);
            } else d_end = 0;
            const long long ri = rbase + r;
            ((fig_rs_gdp)A.ll_flat)[ri] = s_flat[rr]; ((fig_rs_gdp)A.ll_gapped)[ri] = best;
            ((fig_rs_gip)A.n_ins)[ri] = n_ins; ((fig_rs_gip)A.n_del)[ri] = n_del; ((fig_rs_gip)A.d_end)[ri] = d_end; ((fig_rs_gip)A.d_start)[ri] = d_start;
        }
        lo = __shfl(lo, 0, FIG_ID_ROW); hi = __shfl(hi, 0, FIG_ID_ROW);
        for (int x = lo + q; x <= hi; x += FIG_ID_ROW) __hip_atomic_fetch_add((fig_id_gcnt)A.cover + soff + x, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __syncthreads();
    }
}
#endif
#endif
#endif
