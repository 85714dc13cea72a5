// fig_types.h -- POD descriptors shared by the host packer (fig_pack.h, fig_abi.hip) and the gfx950
// gap-fill engine (fig_engine.h).  Everything here is plain data laid out for HBM:
//  * read bases are packed 2 bits/base (A0 C1 G2 T3) in 32-bit words, 16 bases per word,
//    followed by a 1 bit/base N-mask (32 bases per word); a read's words are contiguous so a
//    wavefront fetches a whole read with one coalesced load of <= 19 dwords (L <= 200);
//  * per-gap flank windows are byte codes (0..4) of the FW bases either side of the gap;
//  * per-gap mutable state lives in a per-workgroup scratch slab (see fig_scratch_layout).
#ifndef FIG_TYPES_H
#define FIG_TYPES_H
#include <stdint.h>

#define FIG_MAX_READLEN 200          // MAX_READLENGTH, Figbird.cpp:18
#define FIG_READ_CAP 3000            // partial_limit / unmapped_limit, Figbird.cpp:114-115
#define FIG_MAX_GAP 100000           // MAX_GAP, Figbird.cpp:30
#define FIG_FLANK 208                // flank window kept per side: >= max(read length, side_limit=30)
#define FIG_DBL_MAX 1.7976931348623157e308
#define FIG_SH_C 32                  // reads per chunk of the shared-factor E-step (fig_engine_shared.h)
#define FIG_SH_SC 4                  // chunks per super-chunk: the (chunk, tile) work items of phase A are dealt over the waves per super-chunk
#define FIG_SH_ONE 16                // operand-select register offset of the constant 1.0 (slots without a regular read)
#define FIG_MLE_FB 208               // doubles of the per-wave factor buffer of the MLE pass (>= FIG_MAX_READLEN)
// LDS-tiled class: doubles of LDS the MLE pass needs to run its LDS form over all ncolE columns: C[5][ncolE], one 16-byte
// packed-consensus record per column, the per-wave factor buffers, the packed consensus words (kc, kn) and slack
#define FIG_TILED_MLE_DOUBLES(ncolE, nw) (7LL * (ncolE) + (long long)(nw) * FIG_MLE_FB + ((ncolE) + 15) / 16 + 16 + 8)

// Path mask of a gap's support plane (FigDevBatch::sup_origin); the values of the public FIG_SUP_* (fig_abi_host.h asserts it)
enum { FIG_ORG_NONE = 0, FIG_ORG_FINAL = 1, FIG_ORG_ORIGINAL = 2, FIG_ORG_TIEBREAK = 4 };

// Control word of one gap in the candidate-parallel scheduler: the begin and replay items publish it (fig_ctl_publish,
// fig_engine_sched.h), the round planner (fig_abi_host.h) reads a snapshot of all of them.
enum { FIG_GAP_FINISHED = 0, FIG_GAP_MORE = 1, FIG_GAP_LOOP_DONE = 2 };   // output written ; candidates left to evaluate ; loop over, the end item is due
// FIG_GAP_*, next candidate index, candidate count; then the reach bit of the probe item (the pre-pass), or, in a fill, the size
// of the chunk the gap's last replay went through (0 after the begin item): what the growth rule doubles (fig_wide_chunk)
struct FigGapCtl { int32_t status, j, range; union { int32_t reach; int32_t last; }; };

// Work items of a round, as the planner lays them out and the kernels read them (one 16-byte load each)
struct alignas(16) FigItem { int32_t gap, j, slot, chunk; };               // evaluate candidate j of the gap into slot; chunk: see below
struct alignas(16) FigEntry { int32_t gap, n, j_planned, stamped; };       // replay the gap's slots 0..n-1; the last two: see below
static_assert(sizeof(FigGapCtl) == 16 && sizeof(FigItem) == 16 && sizeof(FigEntry) == 16, "control words are four int32: buffers and copies are sized by sizeof");
// Continuous form: FigItem::chunk carries the size of the gap's chunk (0: a round of the rounds form, nobody counts), and
// FigEntry::j_planned the gap's j when the round was planned, with stamped = 1 (the replay kernel skips a gap an eval workgroup has replayed).
// A continuation: what the workgroup that replayed a gap's chunk publishes for any workgroup of the launch -- the gap's next
// chunk (candidates j0 .. j0+n-1 into slots 0 .. n-1) or its end item (n = 1).  Written once, then `ready`; items are claimed
// by atomicAdd on `next`.  rank: chunks the gap's loop may still need, this one included (1 for an end item): the scan's order.
enum { FIG_CONT_EVAL = 0, FIG_CONT_END = 1 };
#define FIG_CONT_CAP_MAX 65535       // entries of a lane's array at most: the scan's keys hold an entry's index in 16 bits
struct alignas(16) FigCont { int32_t gap, j0, n, kind; int32_t next, ready, rank, pad; };
// Header of a lane's continuation array (the entries follow it): entries reserved so far; workgroups of the launch that have left;
// published items nobody has claimed yet (idle-driven widening reads it; approximate by design, an item takes 100-500 ms).  Zeroed, entries included, before every eval launch
struct alignas(16) FigContHdr { int32_t tail, exited, open, pad; };
static_assert(sizeof(FigCont) == 32 && sizeof(FigContHdr) == 16, "continuation records: buffers are sized by sizeof");

enum FigCounter {                    // slots of FigDevBatch::counters
    FIG_CNT_PLACE = 0,               // placeReads calls of the candidates the gaps' loops consumed
    FIG_CNT_FLOPS = 1, FIG_CNT_SPEC = 2,         // algorithmic flops: useful work only ; every speculative evaluation executed, discarded ones included
    FIG_CNT_MLE_ALG = 3, FIG_CNT_MLE_EXEC = 4,   // MLE passes: flops credited ; FP64 multiplies executed after pruning (raw totals, only their ratio is reported)
    FIG_CNT_CONT = 5,                // chunks continued inside an eval launch (continuous form)
    FIG_CNT_NARROW = 6,              // of them, widened chunks published narrower because the launch was emptying (FIG_SCHED_LOG reports it)
    // FIG_PROF build: FigEng::prof[i] is counter PROF_LO + i below FIG_PROF_SPLIT, PROF_HI + (i - FIG_PROF_SPLIT) from it on; cycles in barriers; wave-cycles
    FIG_CNT_PROF_LO = 8, FIG_CNT_WAIT = 30, FIG_CNT_WAVE = 31, FIG_CNT_PROF_HI = 32,
    // MLE reuse (fig_mle_reuse_probe, fig_engine_core.h): unmapped placeReads calls that asked ; of them, calls whose consensus was that of
    // the candidate's previous call, so that the pass was skipped (FIG_SCHED_LOG reports both; speculative evaluations included)
    FIG_CNT_MLE_ASKED = 50, FIG_CNT_MLE_REUSED = 51,
    FIG_CNT_N = 64
};
#define FIG_PROF_SLOTS 40
#define FIG_PROF_SPLIT 22

struct FigDevModel {
    int32_t L;                       // maxReadLength
    int32_t Tmin, Tmax, cutoff;      // insertThresholdMin/Max, gapProbCutOff
    int32_t partial_flag, unmapped, script_itr, D, read_length, neg_overlap, partial_len, unm_limit;
    int32_t max_insert;
    double T[25];                    // errorTypeProbs[from][to]
    const double *e;                 // errorPosDist[k]
    const double *ome;               // pair tables: {1-e,e} fwd [2L], rev [2L]; {1-e-ins-del,e} fwd [2L], rev [2L]
    const double *ome1;              // 1 - errorPosDist[k]
    const double *m3;                // 1 - errorPosDist[k] - inPosDist[k] - delPosDist[k]
    const double *insd;              // insertLengthDistSmoothed[max_insert]
    const double *qtab;              // [256] pow(10, -(c-33)/10.0)   (qualityFilter, Figbird.cpp:1791-1792)
    double fmm_up;                   // upper bound of any MLE mismatch factor e[k]*T[from][to], from != to (k-mer prefilter)
};

struct FigDevGap {
    int64_t gapStart, contigLen;
    int32_t G0, stat2, stat3, fillflag;
    int32_t nU; int32_t nP;          // reads of this gap (nP = all lines of the partial file, <= 3001 kept)
    int64_t uBase, pBase;            // first read index in the batch-wide arrays
    int32_t alloc_arg; float gpf1, gpf2; int32_t lgf;
    int64_t flankOff;                // byte offset of this gap's 2*FIG_FLANK flank codes
    int64_t strOff;                  // offset of this gap's result string
    int32_t gapNo; int32_t cls;
    int64_t persistOff;              // this gap's persistent slab (candidate-parallel mode)
    int32_t capGg, rangeCap, nslots, pad;   // pad bit 0: a partial read of the gap holds a base outside ACGT
    int64_t streamOff;               // first dword of this gap's operand-select stream (FigDevBatch::ustream)
};

struct FigDevReads {                 // batch-wide SoA, one entry per read
    const int32_t *pos;              // unmapped: anchor pos ; partial: pos (col 4)
    const int32_t *aux;              // unmapped: isReverse  ; partial: match (col 3)
    const int32_t *clip;             // partial: clipped_index
    const int32_t *refpos;           // partial: mate pos or -1
    const int32_t *len;
    const int64_t *woff;             // word offset of the read's packed bases
    const int64_t *qoff;             // partial: byte offset of the quality string (or NULL)
};

struct FigDevBatch {
    int64_t n_gaps;
    const FigDevGap *gaps;
    const int32_t *order;            // gap indices, most expensive first
    FigDevReads u, p;
    const uint32_t *packed;          // all packed reads
    const uint32_t *ustream;         // operand-select stream of the unmapped reads: per gap [chunk of 32 reads][step j < L][32] 16-bit entries (fig_engine_shared.h)
    const uint8_t *qual;             // partial qualities
    const uint8_t *flank;            // per-gap flank codes
    // outputs
    int32_t *filled_len, *gaptofill; char *str;
    int32_t dbg_max_cand; int32_t *dbg_n_cand; int32_t *dbg_cand_i; double *dbg_cand_lik; int32_t *dbg_n_place;
    int32_t *draw_pos, *draw_isz, *draw_len; int64_t n_ureads;
    int32_t dbg_plane_cols, dbg_plane_reads; double *dbg_counts, *dbg_read_maxlv;   // numeric planes (i)/(ii), parity tests only
    // work queue + counters
    int32_t *queue_head;             // [2] a persistent launch pops from [FigKernArgs::qsel] and zeroes the other for its successor
    unsigned long long *counters;    // [FIG_CNT_N], by FigCounter
    // scratch
    uint8_t *scratch; int64_t scratch_stride;   // one slab per workgroup
    int32_t capG, capR, capP, capC;  // capacities the slab was carved for (columns, unmapped reads, partial reads, candidates)
    int32_t capW, capE;              // weight-buffer doubles, extended-table columns
    uint8_t *persist;                // per-gap persistent slabs
    FigGapCtl *gapctl;               // [n_gaps]
    // continuous form (null / 0: the rounds form): items of the gap's chunk that have finished, [n_gaps]; the lane's
    // continuation array, header first, and the entries it holds
    int32_t *gap_pending; FigContHdr *cont_hdr; FigCont *cont; int32_t cont_cap;
    const uint8_t *ot_preset;        // [n_gaps] 1 = the gap's worker process has set overlap_threshold before it gets to the gap (Figbird.cpp:103, :6317)
    // optional per-base read support (fig_gap_support): the countsGap columns behind the emitted string, [(strOff + x) * 5 + b],
    // and the FIG_ORG_* path mask per gap; both null = off (fig_gap_end takes one uniform branch and stores nothing)
    int32_t *sup_counts, *sup_origin;
};

#endif
