/* figbird_hip.h -- C ABI of libfighip.so, the MI355X (gfx950) gap-fill engine.
 *
 * Drop-in boundary.  The reference has no in-process API: its
 * dispatcher FillGaps.cpp shells out `g++ Figbird.cpp && ./aN.out <16 args>` once per
 * thread (FillGaps.cpp:51-138) and each such process runs the per-gap loop
 * (Figbird.cpp:7329-7440) -> GapFiller::fillGap (Figbird.cpp:6201-6570).  This ABI
 * replaces exactly that: "fill this batch of gaps with this model", as plain C structs of
 * caller-owned host arrays.  No torch types, no C++ types, no global state.
 *
 * Conventions: every function returns 0 (FIG_OK) or a negative FIG_E* code and never
 * exits/throws; all sizes are int64_t; the caller owns every buffer; fig_fill_gaps() is
 * synchronous (the library syncs its own HIP stream before returning); one fig_ctx per
 * GPU, not thread-safe; calls on distinct contexts may run concurrently.
 *
 * There is NO CPU fallback: if no gfx950 device is usable fig_ctx_create() fails with
 * FIG_ENODEV.
 */
#ifndef FIGBIRD_HIP_H
#define FIGBIRD_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FIG_ABI_VERSION 1

#define FIG_OK 0
#define FIG_EINVAL (-1)   /* bad argument / inconsistent batch                      */
#define FIG_ENODEV (-2)   /* no usable HIP device (there is no CPU path)            */
#define FIG_ENOMEM (-3)   /* host or device allocation failed                       */
#define FIG_EHIP (-4)     /* a HIP runtime call or kernel failed                    */
#define FIG_ENOSPC (-5)   /* caller's result string buffer is too small             */
#define FIG_EUNSUP (-6)   /* input outside the supported envelope   */

typedef struct fig_ctx fig_ctx;

/* Model tables = the globals Figbird.cpp builds once per run from myout.sam / stat.txt
 * (A0: Figbird.cpp:47-91, built :846-921, :291-487, :497-844, :1156-1376, :7155-7200),
 * plus the run-level argv of Figbird.cpp main (:6957-6973).  Built on the host by the
 * caller (figfill does it in figbird_amd/csrc/host/fig_host.cpp: build_model). */
typedef struct fig_model {
    int32_t max_read_length;            /* maxReadLength (stat.txt col 3), <= 200            */
    const double *error_pos_dist;       /* errorPosDist[max_read_length]                    */
    const double *in_pos_dist;          /* inPosDist[max_read_length]                       */
    const double *del_pos_dist;         /* delPosDist[max_read_length]                      */
    double error_type_probs[25];        /* errorTypeProbs[5][5], row = from, col = to       */
    const double *insert_len_dist_smoothed; /* insertLengthDistSmoothed[max_insert_size]    */
    int32_t max_insert_size;            /* maxInsertSize                                    */
    int32_t insert_threshold_min;       /* insertThresholdMin (after the partial_len shift) */
    int32_t insert_threshold_max;       /* insertThresholdMax                               */
    int32_t gap_prob_cutoff;            /* gapProbCutOff                                    */
    /* run parameters */
    int32_t partial_flag;               /* argv[5]  */
    int32_t unmapped_flag;              /* argv[6]  */
    int32_t script_itr;                 /* argv[4]  */
    int32_t max_distance;               /* argv[2]  tempmaxDistance (D)                     */
    int32_t read_length;                /* argv[3]  unmapped_read_len                       */
    int32_t neg_overlap;                /* argv[12] gaplen_negative_overlap                 */
    int32_t partial_len;                /* argv[13]                                         */
    int32_t unm_limit;                  /* argv[14] gapthresh (400, FillGaps.cpp:22)        */
} fig_model;

/* One batch of gaps with their binned reads, as GapFiller sees them after
 * parseUnmapped/parsePartial (A2: Figbird.cpp:5661-5842).  SoA + CSR, host memory.
 * Sequences are ASCII; anything outside "ACGT" is treated as N. */
typedef struct fig_gap_batch {
    int64_t n_gaps;
    /* scaffold the gaps live in (Figbird.cpp:6979-7058): upper-case ASCII, concatenated */
    int64_t n_contigs;
    const int64_t *contig_off;          /* [n_contigs+1] offsets into contig_seq            */
    const char *contig_seq;
    /* per gap: gapInfo.txt (contigIdx, gapStart0, len) + stat2.txt + fillflag           */
    const int32_t *gap_contig;          /* [n_gaps]                                         */
    const int64_t *gap_start;           /* [n_gaps] 0-based start of the N run              */
    const int32_t *gap_len;             /* [n_gaps] originalGap                             */
    const int32_t *gap_stat2;           /* [n_gaps*3] fillNotfill, perfectReadGap, perfectReadGaplen */
    const int32_t *gap_fillflag;        /* [n_gaps] 1, or -1 when the gap had > 3000 read pairs (Figbird.cpp:7380-7385) */
    /* unmapped-mate reads (gaps_<g>.sam after parseUnmapped): CSR over gaps              */
    const int64_t *u_read_off;          /* [n_gaps+1] read index range per gap              */
    const int32_t *u_anchor_pos;        /* [n_ureads] pos_reads[] (1-based anchor position) */
    const uint8_t *u_is_reverse;        /* [n_ureads] isReverse[] (1 = mate was reverse-complemented) */
    const int64_t *u_seq_off;           /* [n_ureads+1] offsets into u_seq                  */
    const char *u_seq;                  /* reads_gap[] (already in gap orientation)         */
    /* partial (soft-clipped) reads (partial_gaps_<g>.sam): CSR over gaps, file order      */
    const int64_t *p_read_off;          /* [n_gaps+1]                                       */
    const int32_t *p_clipped_index;     /* [n_preads] col 2                                 */
    const int32_t *p_match;             /* [n_preads] col 3 (1/4 left side, 2/3 right side) */
    const int32_t *p_pos;               /* [n_preads] col 4                                 */
    const int32_t *p_ref_pos;           /* [n_preads] col 6 (mate position or -1)           */
    const int64_t *p_seq_off;           /* [n_preads+1] offsets into p_seq and p_qual       */
    const char *p_seq;
    const char *p_qual;                 /* phred+33, same offsets as p_seq (may be NULL in unmapped mode) */
    /* state the reference carries from gap to gap inside ONE worker process (FillGaps.cpp:456-649 deals the gaps to
     * $num_threads processes, each running Figbird.cpp main over its list in ascending gap order): [n_gaps] 1 when that
     * process has already set its global overlap_threshold (Figbird.cpp:103, :6317) by the time it gets to the gap.
     * NULL = the batch is one process taking the gaps in batch order (numthreads = 1): the library measures the carry
     * itself at upload.  A caller that deals the gaps to several processes, or fills a SHARD of a run (the gap that
     * set the value may be in another shard), uploads, asks fig_batch_probe_reach() which gaps get to :6317, carries
     * the bits along each process's gap list and hands the result to fig_batch_set_ot_preset() before the fill
     * (figfill: fig_host.cpp ot_presets_from_reach).  Only read in partial mode (the reference never reads the
     * global in an unmapped-mode run). */
    const uint8_t *gap_ot_preset;
} fig_gap_batch;

/* Results = what Figbird.cpp writes per gap: the gapout line (:7411-7413) and
 * gaptofill[g] (:6486-6492, :7463-7466). */
typedef struct fig_gap_results {
    int32_t *filled_len;                /* [n_gaps] gapStringLength                         */
    int32_t *gaptofill;                 /* [n_gaps] 0 or the negative-overlap length        */
    int64_t *str_off;                   /* [n_gaps+1] OUT: offsets of each gap string in str */
    char *str;                          /* OUT: concatenated gap strings (ACGTN), not NUL-terminated */
    int64_t str_capacity;               /* bytes available in str                           */
    /* optional parity/debug planes (NULL to disable): per gap, up to dbg_max_cand records
     * {gapEstimate, em_iterations, valid_count, likelihood} = likelihood_arr (Figbird.cpp:6390-6391) */
    int32_t dbg_max_cand;
    int32_t *dbg_n_cand;                /* [n_gaps]                                         */
    int32_t *dbg_cand_i;                /* [n_gaps*dbg_max_cand*3]                          */
    double *dbg_cand_lik;               /* [n_gaps*dbg_max_cand]                            */
    int32_t *dbg_n_place;               /* [n_gaps] placeReads invocations spent on the gap (needs dbg_n_cand)  */
    /* optional per-read final placements for draw.txt (Figbird.cpp:5140, 5381); NULL to disable */
    int32_t *draw_pos;                  /* [n_ureads + n_preads] maxPos-left_maxDistance, or INT32_MIN if the read was not drawn */
    int32_t *draw_isz;                  /* [n_ureads + n_preads] mleInsertSize / newInsertSize */
    int32_t *draw_len;                  /* [n_gaps*2] length argument of the unmapped / partial "S" header, -1 if absent */
    /* optional numeric planes of the parity contract (SURVEY.md §8 preamble), per gap and candidate INDEX j (candidate
     * length = gapMin + j; needs the dbg_cand buffers above; NULL to disable):
     *  (i)  countsGap[x][0..4] as the E-step of the candidate's LAST placeReads call left it (Figbird.cpp:3181-3187 /
     *       :3603-3611), x < min(candidate length, dbg_plane_cols);
     *  (ii) per read, the E-step's maximum log-likelihood over its placements, maxlikelihood_value[r] (:3258-3261 /
     *       :3680-3688; 0 when the read had no placement), r < min(reads of the gap, dbg_plane_reads). */
    int32_t dbg_plane_cols;
    int32_t dbg_plane_reads;
    double *dbg_counts;                 /* [n_gaps*dbg_max_cand*dbg_plane_cols*5]           */
    double *dbg_read_maxlv;             /* [n_gaps*dbg_max_cand*dbg_plane_reads]            */
} fig_gap_results;

/* Optional per-base read support of a fill (fig_fill_resident_ex): for every byte of results->str the five read counts
 * (A, C, G, T, other) of the countsGap column the byte was called from -- the columns as the last computeSequence(check=1)
 * of finalize (Figbird.cpp:4417-4508 called from :4929-5659) consumed them -- and per gap where those counts came from.
 * Call rule: first strict maximum over the five counts; 'N' when the maximum is 0 or the "other" row wins.  An 'N' over a
 * column WITH support was masked afterwards (recheck_sequence / findRegion, :4594-4743).  All zero for a gap whose string is
 * not such a call: never attempted, closed by a negative overlap, or counts cleared with nothing put back (origin NONE). */
#define FIG_SUP_NONE 0       /* the gap's plane is all zero (and only then)                                            */
#define FIG_SUP_FINAL 1      /* pile-up of this fill's final placement: the reads draw_pos reports, at those offsets    */
#define FIG_SUP_ORIGINAL 2   /* restored from the placement at the original gap length (recompute1 / recompute2)        */
#define FIG_SUP_TIEBREAK 4   /* or'ed in: the partial-mode check_update pass ran over the columns (:5575-5590) -- it adds
                              * 10 to one of A..T of a column to settle a near-tie by base quality, or zeroes A..T        */
typedef struct fig_gap_support {
    int32_t *counts;                    /* [str_capacity*5] compacted exactly like str: base x of gap g is at (str_off[g]+x)*5 */
    int32_t *origin;                    /* [n_gaps] FIG_SUP_* mask                                                      */
} fig_gap_support;

/* Optional per-base quality of the filled bases (fig_batch_quality): how likely each emitted base is wrong, under the run's own
 * error model -- errorPosDist[k] (index len-1-j for base j of an unmapped read whose is_reverse bit is set, Figbird.cpp:3569-3576;
 * j for every other read) and errorTypeProbs[from][to], the tables the E-step weighs placements with.
 *
 * Evidence of a gap = that of its support plane: the reads its draw header lists, each at its drawn offset o, base j of the read
 * on column x = o + j for 0 <= x < n = filled_len[g].  draw_len[2g] >= 0: the gap's unmapped reads; draw_len[2g+1] >= 0: its
 * partial reads (never both).  A read whose draw_pos is INT32_MIN and read bases outside ACGT take no part.
 *
 * Tables, built on the host with the C library's log10 (log10(0) = -inf is kept): lm[k] = log10(1 - e[k]),
 * le[k] = log10(e[k]), lt[b][s] = log10(errorTypeProbs[b*5+s]) with b the true base and s the read base, both in A..T.
 * Column log-likelihoods: for true base b and read base s the term is lm[k] if s == b, else le[k] + lt[b][s];
 * LL[x][b] = LL[x][b] + term, from 0.0, the reads of the gap in ascending read index, every + one IEEE double addition.  The
 * device only adds table entries in that order, so the plane is reproducible bit for bit from the tables.
 *
 * Phred of a column with emitted byte c: 0 if c is not one of ACGT; m = max LL, 0 if m == -inf; w[b] = pow(10, LL[b] - m)
 * (-inf gives 0); num = sum of w[b], b != c, in the order A, C, G, T; perr = num / (num + w[c]); 93 if perr == 0, else
 * floor(-10*log10(perr) + 0.5) clamped to 0..93.
 *
 * A gap is FIG_QUAL_ON iff n > 0, exactly one of its two draw_len entries is >= 0 and equals n, and -- when origins are given --
 * its origin has FIG_SUP_FINAL and lacks FIG_SUP_ORIGINAL (FIG_SUP_TIEBREAK does not matter).  Every other gap is FIG_QUAL_OFF:
 * its LL are all 0.0 and its Phred all 0, written by the library whatever the buffers held.
 *
 * Limits of the number: reads are taken as independent, the placement is taken as given, and the prior over bases is uniform.
 * It is therefore an UPPER bound on confidence.  A masked 'N' has quality 0 even where its column has support. */
#define FIG_QUAL_OFF 0
#define FIG_QUAL_ON  1
typedef struct fig_gap_quality {
    double  *loglik;   /* [str_off[n_gaps]*4], base x of gap g at (str_off[g]+x)*4 + b */
    uint8_t *phred;    /* [str_off[n_gaps]]   */
    uint8_t *state;    /* [n_gaps] FIG_QUAL_* */
} fig_gap_quality;

/* Optional placement confidence per drawn unmapped read (fig_batch_placement): could the read have gone elsewhere?  The support and
 * quality planes take the final placement of every read as a fact; in a repeat a read fits several offsets equally well and the
 * MLE pass keeps the first maximum.  This call scores EVERY placement of every drawn read against the emitted sequence, one
 * E-step's worth of work per gap, and reports the drawn placement next to the best other one (what aligners call MAPQ).
 *
 * Sequence of gap g.  n = filled_len[g].  For an integer column x, S(x) is the emitted byte str[str_off[g] + x] for 0 <= x < n,
 * the contig base at gap_start + x for x < 0, the contig base at gap_start + G0 + (x - n) for x >= n; a position outside the
 * contig, or a byte outside ACGT, is N.  (On the device: the 2 x 208 flank codes of the resident batch.)  No column beyond
 * +-(200 - 1) of the string is ever needed.
 *
 * Placements of unmapped read r (length len, anchor pos = u_anchor_pos[r], reverse bit rev): the offsets o in [-(len-1), n-1],
 * base j on column o + j.  Insert size of a placement: pos < gap_start (left anchor): isz(o) = gap_start - pos + len + o;
 * otherwise (right anchor): isz(o) = pos + (n - G0) - gap_start + len - o  (the reference's tempInsertSize, Figbird.cpp finalize).
 * A placement is VALID iff insert_threshold_min <= isz <= insert_threshold_max and 0 <= isz < max_insert_size.
 *
 * Score.  lm, le, lt are fig_gap_quality's tables; li[s] = log10(insertLengthDistSmoothed[s]) (the C library's log10, log10(0) =
 * -inf is kept); lq = -0x1.34413509f79ffp-1 (log10 of 1/4).  Lr(o) = li[isz(o)], then for j = 0 .. len-1 in ascending order
 * Lr = Lr + t_j, each + one IEEE double addition; a read base outside ACGT is skipped; with c = S(o + j), s the read base and
 * k = len-1-j if rev else j:  t_j = lq if c is N;  lm[k] if c == s;  otherwise le[k] + lt[c][s].  Only -inf can meet -inf, so no
 * NaN arises.  The device only adds table entries in that order.
 *
 * A gap is FIG_PLACE_ON iff the model is unmapped-mode, draw_len[2g] >= 0 and draw_len[2g+1] < 0, and fig_gap_quality's rule
 * holds (n > 0, the header equals n, origins given: FINAL without ORIGINAL).  Partial reads are anchored by their clip and are not
 * scored.  A read is SCORED iff its gap is on and draw_pos[r] != INT32_MIN.
 *
 * Per scored read, o* = draw_pos[r] (arrays indexed like the unmapped part of draw_pos):
 *   ll_drawn   Lr(o*), or -inf if o* is not a valid placement
 *   ll_other   the greatest Lr(o) over valid o != o*; -inf if there is none
 *   off_other  the smallest o that attains ll_other; INT32_MIN if there is no valid o != o*
 *   n_valid    the number of valid placements, o* included if it is valid
 *   sum_other  with M = max(ll_drawn, ll_other): 0.0 if M is -inf, otherwise the sum of 10^(Lr(o) - M) over valid o != o* with
 *              Lr(o) > -inf (a sum of positive terms: the device adds them in an order of its own, with its own exp10)
 *   pq         on the host: 0 if ll_drawn is -inf; otherwise w = pow(10, ll_drawn - M), perr = sum_other / (sum_other + w);
 *              60 if perr == 0, else floor(-10*log10(perr) + 0.5) clamped to 0..60
 * The first four are exact by construction.  An unscored read gets ll_drawn = ll_other = sum_other = 0.0, off_other INT32_MIN,
 * n_valid 0 and pq 255 (FIG_PLACE_NONE), written by the library whatever the buffers held.
 *
 * Limits of the number: a uniform prior over the bases of an N column; substitutions only; the other reads' placements do not
 * enter; and the sequence is the EMITTED one, not the one the MLE pass placed against -- after recheck_sequence masks columns a
 * read may now prefer another offset, which is reported (ll_other > ll_drawn, pq 0), not hidden. */
#define FIG_PLACE_OFF 0
#define FIG_PLACE_ON  1
#define FIG_PLACE_NONE 255   /* pq of a read that was not scored */
#define FIG_PLACE_MAX_PQ 60
typedef struct fig_read_placement {
    double  *ll_drawn;   /* [n_ureads] */
    double  *ll_other;   /* [n_ureads] */
    double  *sum_other;  /* [n_ureads] */
    int32_t *off_other;  /* [n_ureads] */
    int32_t *n_valid;    /* [n_ureads] */
    uint8_t *pq;         /* [n_ureads] */
    uint8_t *state;      /* [n_gaps] FIG_PLACE_* */
} fig_read_placement;

/* Optional per-base quality that sums over read placements (fig_batch_softqual).  fig_gap_quality takes the placement of every
 * read as given: a read that fits three offsets equally well is piled up at full weight on the first of them.  Here a scored read
 * counts on every placement by the share of it that could be there.  Every term not redefined below means what it means for
 * fig_gap_quality and fig_read_placement: the sequence S(x) of a gap, the placements o in [-(len-1), n-1], isz(o) and the validity
 * rule, the score Lr(o) with li, lm, le, lt, lq, the index k, the skipping of read bases outside ACGT, and which reads are scored.
 *
 * Gaps.  A gap is FIG_SOFTQ_ON iff it is FIG_PLACE_ON; every other gap is FIG_SOFTQ_OFF: its planes are all 0.0 and its Phred all
 * 0, written by the library whatever the buffers held.
 *
 * Weights of a scored read r.  M_r = the greatest Lr(o) over its valid placements, the drawn one included when it is valid.  A read
 * with no valid placement, or with M_r = -inf, takes no part.  Otherwise d(o) = Lr(o) - M_r (one IEEE subtraction); a valid
 * placement is ACTIVE iff d(o) >= -300 (an exact comparison of exactly reproducible doubles, which keeps -inf and underflow out of
 * what follows); u(o) = 10^d(o); Z_r = the sum of u over the active placements; p_r(o) = u(o) / Z_r.  The library takes Z_r from the
 * placement pass as sum_other + 10^(ll_drawn - M_r): the terms below the cut change it by less than 1e-297 relative.
 *
 * Planes, per column 0 <= x < n of a gap that is on.  The sums run over the scored reads r and their active placements o with
 * j = x - o in [0, len) and base j of the read one of ACGT: s its code, k its table index.
 *   wcount[x][s]   the sum of p_r(o): the expected number of reads that show s on the column (the soft form of the support counts)
 *   eloglik[x][b]  the sum of p_r(o) * t, t = lm[k] if s == b, else le[k] + lt[b][s]: the expected log10-likelihood of true base b
 * A -inf term with an active weight makes the entry -inf.  A column with no contribution is exactly 0.0.  Every term of an entry has
 * one sign; the device adds them read by read in ascending read index and, within a read, in ascending j.
 *
 * phred[x] = the Phred of fig_gap_quality applied to eloglik[x] and the emitted byte.
 *
 * When every read has exactly one active placement and it is the drawn one, p = 1: eloglik is fig_gap_quality's loglik and wcount
 * the A..T columns of the support counts (their fifth, "other" column has no counterpart here).
 *
 * Limits of the number: the score of a placement includes the read's own base on column x against the emitted call (the E-step's
 * circularity); reads are taken as independent; substitutions only; a uniform prior over the bases of an N column; undrawn reads
 * and partial reads take no part. */
#define FIG_SOFTQ_OFF 0
#define FIG_SOFTQ_ON  1
typedef struct fig_gap_softqual {
    double  *wcount;   /* [str_off[n_gaps]*4]  (str_off[g]+x)*4 + s */
    double  *eloglik;  /* [str_off[n_gaps]*4]  (str_off[g]+x)*4 + b */
    uint8_t *phred;    /* [str_off[n_gaps]] */
    uint8_t *state;    /* [n_gaps] FIG_SOFTQ_* */
} fig_gap_softqual;

/* Optional indel evidence per filled base (fig_batch_indel): a gapped realignment of every drawn read.  The planes above score reads
 * against the emitted sequence with substitutions only: a homopolymer that came out one base short shows as a run of mismatches in
 * every read that spans it, and nothing names the missing base.  Here each drawn read is realigned around its drawn offset by a
 * banded dynamic program with the model's own insertion and deletion rates, and per column the reads that ask for an edit are counted.
 * Terms not redefined here mean what they mean for fig_read_placement: the sequence S(x) of a gap, n, the tables lm, le, lt and lq,
 * the index k and the skipping of a read base outside ACGT, which gaps are on and which reads are scored.
 *
 * Gaps and reads.  A gap is FIG_INDEL_ON iff it is FIG_PLACE_ON.  A scored read is ALIGNED iff its drawn offset o* satisfies
 * -(len-1) <= o* <= n-1; the insert size takes no part.  Every other read is unaligned.
 *
 * Tables, built on the host with the C library's log10 (-inf is kept): lI[k] = log10(in_pos_dist[k]) + lq, one IEEE addition (an
 * inserted read base is uniform over the four bases); lD[k] = log10(del_pos_dist[k]).
 *
 * Band.  W = 7 (FIG_INDEL_W), diagonals d in [-7, 7].  Cell (i, d): i read bases are consumed and the next column is x = o* + i + d.
 *   H(0, d) = 0.0 for every d: the start is free.
 *   For i = 1 .. len, with j = i-1 and (s, k) of read base j:
 *     diag = H(i-1, d) if base j is outside ACGT (skipped, nothing added), else H(i-1, d) + t, where with c = S(o* + j + d):
 *            t = lq if c is N, lm[k] if c == s, else le[k] + lt[c][s];
 *     ins  = H(i-1, d+1) + lI[k], or -inf for d = 7;
 *     H(i, d) = diag with back-pointer DIAG if diag >= ins, else ins with back-pointer INS.
 *   Then, for 1 <= i <= len-1 only, in ascending d from -6: v = H(i, d-1) + lD[k], k that of base i-1; if v > H(i, d) (strictly),
 *   H(i, d) = v with back-pointer DEL.
 * Every + is one IEEE double addition; only -inf can meet -inf, so no NaN arises.
 *
 * End.  ll_gapped is the greatest H(len, d); ties go to the first d in the order 0, -1, +1, -2, +2, ..., -7, +7: that d is d_end.
 * ll_flat is the sum along d = 0 alone: the same terms from 0.0, with no INS or DEL; ll_gapped >= ll_flat, exactly.  If ll_gapped
 * is -inf the read reports ll_flat, ll_gapped and zeros: it has no events and no cover.
 *
 * Path and events.  The path is the traceback from (len, d_end) along the back-pointers to row 0, where d is d_start.  An event is a
 * maximal run of INS steps or of DEL steps; n_ins is the number of inserted read bases, n_del the number of deleted columns.  Each
 * event is LEFT-NORMALISED before it is reported, so that the reads of one homopolymer agree on a column:
 *   a DEL run over columns [x, x+m): while the path step before the run is DIAG (some read base on column x-1) and
 *   S(x-1) == S(x+m-1) as codes, x -= 1;
 *   an INS run of read bases [i, i+m) whose next column is x: while the step before the run is DIAG (base i-1 on column x-1) and bases
 *   i-1 and i+m-1 have equal codes and equal N bits, i -= 1 and x -= 1.
 * This never looks past the path's start or another event, and the back-pointers are not changed by it.
 *
 * Planes, over the columns 0 <= x < n of a gap that is on, compacted like str:
 *   del_reads[x]  aligned reads with a normalised DEL run covering x
 *   ins_reads[x]  aligned reads with a normalised INS run whose next column is x
 *   ins_end[g]    the same for next column n, the right junction
 *   cover[x]      aligned reads with finite ll_gapped whose path spans x: o* + d_start <= x <= o* + len - 1 + d_end
 * They are integers: the order of accumulation does not matter.
 *
 * Call (host).  call[x] is 'D' if del_reads[x] >= 2 and 2 * del_reads[x] > cover[x]; else 'I' under the same rule on ins_reads[x];
 * else '.'.  call_end[g] likewise, from ins_end[g] and cover[n-1].
 *
 * Defaults, written by the library whatever the buffers held.  Off gaps: all planes 0, calls '.'.  Unaligned reads:
 * ll_flat = ll_gapped = 0.0, n_ins = n_del = d_end = 0, d_start = INT32_MIN.
 *
 * Limits of the number: the band -- a net shift of 8 or more is not found; no insert-size term -- a read wholly on d != 0 is
 * fig_read_placement's business; a linear gap cost from the position rates only (the length distributions are not in fig_model);
 * 1 - e[k] instead of 1 - e - ins - del under a match, so that a path without indels scores fig_read_placement's terms; reads are
 * taken as independent; partial reads and undrawn reads take no part. */
#define FIG_INDEL_OFF 0
#define FIG_INDEL_ON  1
#define FIG_INDEL_W   7
typedef struct fig_gap_indel {
    double  *ll_flat;    /* [n_ureads] */
    double  *ll_gapped;  /* [n_ureads] */
    int32_t *n_ins;      /* [n_ureads] */
    int32_t *n_del;      /* [n_ureads] */
    int32_t *d_end;      /* [n_ureads] */
    int32_t *d_start;    /* [n_ureads] */
    int32_t *del_reads;  /* [str_off[n_gaps]] */
    int32_t *ins_reads;  /* [str_off[n_gaps]] */
    int32_t *cover;      /* [str_off[n_gaps]] */
    int32_t *ins_end;    /* [n_gaps] */
    char    *call;       /* [str_off[n_gaps]] 'D', 'I' or '.' */
    char    *call_end;   /* [n_gaps] 'I' or '.' */
    uint8_t *state;      /* [n_gaps] FIG_INDEL_* */
} fig_gap_indel;

/* Optional polish of the filled strings (fig_batch_polish): the indel calls of fig_gap_indel that the reads' likelihood confirms are
 * applied, round by round, and the result is verified.  fig_gap_indel says that most reads want a base before column 45; it does not
 * say which base, nor whether the edit raises the reads' likelihood, and it leaves the string as it is.  Every term not redefined
 * here means what it means for fig_gap_indel: S(x), n, the tables, the band with W = 7, ll_gapped, the calls, which gaps are on and
 * which reads are scored and aligned.
 *
 * Candidate edits of a gap whose current string has n columns.  DEL x removes column x (0 <= x < n, n >= 2).  INS x b puts base b,
 * one of ACGT, before column x (0 <= x <= n).  The edited sequence S_c(y) over all integer columns y:
 *   DEL x:    S(y) for y < x, S(y+1) for y >= x;
 *   INS x b:  S(y) for y < x, b for y = x, S(y-1) for y > x;
 * its length is n_c = n -+ 1.  A read's offset under the candidate, o_c: o* + 1 for INS when o* >= x; o* - 1 for DEL when o* > x;
 * otherwise o*.
 *
 * Reads.  A read is TOUCHED iff o* - (W+1) <= x <= o* + len + W: a read that is not touched has the same band contents under S_c
 * and o_c.  A read is COUNTED iff it is scored, touched, aligned under (o*, n) and aligned under (o_c, n_c).
 *
 * Scores.  ll_c(r) is fig_gap_indel's ll_gapped of read r against S_c at o_c: the same cell update, sweep and end order, no
 * traceback; it is reproducible bit for bit.  T_c is the sum of ll_c(r) over the counted reads and T_0 the sum of the unedited
 * ll_gapped(r) over the same reads, both in ascending read index from 0.0, one IEEE addition each.  Only -inf can occur: no NaN.
 *
 * One round, per gap that is on and has not stopped:
 *   1 sites       the columns with call != '.', ascending, then the right junction if call_end != '.'; the first
 *                 FIG_POLISH_MAX_SITES = 16 of them, the rest wait for the next round.  A gap without a site stops.
 *   2 candidates  a 'D' site proposes DEL x; an 'I' site INS x A, INS x C, INS x G, INS x T; call_end the four at x = n.  A site
 *                 is skipped, and the gap gets FIG_POLISH_CAPPED, where the edit cannot be stored: DEL at n = 1, or INS into a list
 *                 of inserted bases that already holds 7 (see edit below).
 *   3 best        per site the candidate of the greatest T_c; ties go to the first of A, C, G, T.
 *   4 accept      the best is accepted iff T_c > T_0; otherwise the gap gets FIG_POLISH_REJECTED.  A gap with no accepted
 *                 candidate stops.
 *   5 apply       the accepted edits of the gap are applied together, right to left, each shifting the offsets of all the gap's
 *                 drawn reads by the rule of o_c.  An edit that can no longer be stored when its turn comes (the two cases of step
 *                 2, after the edits to its right) is dropped and the gap gets FIG_POLISH_CAPPED.
 *   6 verify      the next indel pass runs over the edited strings and offsets.  V_new is the sum of the new ll_gapped and V_old
 *                 the sum of the old, over the gap's reads aligned under both the old and the new (offset, n), in ascending read
 *                 index from 0.0.  The round is kept iff V_new > V_old (FIG_POLISH_EDITED); otherwise the gap takes its previous
 *                 string and offsets back, gets FIG_POLISH_REVERTED and stops.
 *   7 stop        the calls of the verifying pass are the sites of the next round.  A gap that has not stopped after max_rounds
 *                 rounds and still has a call gets FIG_POLISH_CAPPED.
 * rounds[g] counts the rounds in which the gap had a site.
 *
 * Result, in terms of the ORIGINAL columns 0 <= x < n of the caller's string, compacted like str:
 *   edit[x]      bit 0: the column's base is removed; bits 1-3: k, the number of bases inserted immediately before it (0..7);
 *                bits 4+2i, 5+2i: the code (A C G T = 0..3) of inserted base i, leftmost first
 *   edit_end[g]  the same layout for the bases after the last column; bit 0 is never set
 * The polished string is, over x: the inserted bases of edit[x], then str[x] unless removed; then the bases of edit_end[g]
 * (fig_polish_apply).  An insertion before a current cell that is an original column joins the end of that column's list (of
 * edit_end's list for x = n); before a cell that is itself an inserted base it takes that position in the same list.  Removing an
 * inserted base takes it out of its list.
 *   polished_len  [n_gaps] the length of the polished string
 *   draw_pos      [n_ureads] the offsets against the polished strings; INT32_MIN is kept
 *   n_ins, n_del  [n_gaps] inserted bases and removed columns in force at the end
 *   ll_before, ll_after  [n_gaps] the sum of ll_gapped against the original and against the polished string, over the gap's reads
 *                 aligned under both, in ascending read index from 0.0: equal bit for bit for an unedited gap
 *   state         FIG_POLISH_ON | EDITED | REJECTED | REVERTED | CAPPED
 * Off gaps get zeros, their own filled_len and the caller's draw_pos, written by the library whatever the buffers held.
 *
 * Limits: everything fig_gap_indel lists; edits are judged one site at a time against the unedited string of the round and only
 * verified jointly; the read set and the drawn offsets are those of the fill -- nothing is placed again; at most one base per site
 * and round. */
#define FIG_POLISH_ON        1
#define FIG_POLISH_EDITED    2
#define FIG_POLISH_REJECTED  4
#define FIG_POLISH_REVERTED  8
#define FIG_POLISH_CAPPED    16
#define FIG_POLISH_MAX_SITES 16
#define FIG_POLISH_MAX_ROUNDS 8
#define FIG_POLISH_DEFAULT_ROUNDS 4
typedef struct fig_gap_polish {
    int32_t *edit;          /* [str_off[n_gaps]] */
    int32_t *edit_end;      /* [n_gaps] */
    int32_t *polished_len;  /* [n_gaps] */
    int32_t *draw_pos;      /* [n_ureads] */
    int32_t *n_ins;         /* [n_gaps] */
    int32_t *n_del;         /* [n_gaps] */
    int32_t *rounds;        /* [n_gaps] */
    double  *ll_before;     /* [n_gaps] */
    double  *ll_after;      /* [n_gaps] */
    uint8_t *state;         /* [n_gaps] FIG_POLISH_* bits */
} fig_gap_polish;

/* Optional recruiting of the reads the fill rejected (fig_batch_recruit): a gapped placement of every undrawn unmapped read.  The
 * fill draws a read only when its UNGAPPED likelihood clears the run's cutoff, -log10(likelihood) < gap_prob_cutoff.  A read that
 * spans a missing or extra base of the emitted string is a run of mismatches from the error to its end: it fails the cutoff and
 * stays undrawn, and fig_gap_indel and fig_gap_polish, which look at drawn reads only, never see the very reads that carry the
 * evidence.  Here every undrawn read of a gap is placed again with indels allowed, the fill's own threshold is applied to the gapped
 * score, and the result is a draw plane that fig_batch_indel and fig_batch_polish accept as it is.  Every term not named here means
 * what it means for fig_read_placement and fig_gap_indel: S(x), n, the placements o in [-(len-1), n-1], isz(o) and validity; Lr(o),
 * li, lm, le, lt, lq, the index k, the skipping of bases outside ACGT; lI, lD, the band with W = 7, ll_flat, ll_gapped, d_end and its
 * tie order.
 *
 * Gaps and reads.  A gap is FIG_RECRUIT_ON iff it is FIG_PLACE_ON.  A read of an on-gap with draw_pos[r] != INT32_MIN is KEPT; nothing
 * about it is computed.  A read of an on-gap with draw_pos[r] == INT32_MIN is a CANDIDATE.
 *
 * Seed.  n_valid is the number of valid placements; ll_seed the greatest Lr(o) over the valid placements; off_seed the smallest o
 * that attains it.  With no valid placement, or with ll_seed = -inf, the read is NONE and nothing further is computed: it reports
 * n_valid, ll_seed = -inf, off_seed = INT32_MIN and the defaults below.
 *
 * Second.  ll_second is the greatest Lr(o) over the valid o with |o - off_seed| > W (offsets within the band are the same locus) and
 * off_second the smallest such o that attains it; with no such o they are -inf and INT32_MIN.
 *
 * Band.  ll_flat, ll_gapped and d_end are those of fig_gap_indel with o* = off_seed: the same cell update, sweep and end order,
 * forward only, no traceback.  (A valid placement is aligned under (off_seed, n), so the unaligned case does not arise.)
 *
 * Score.  score = li[isz(off_seed)] + ll_gapped, one IEEE addition.
 *
 * Rule (host), in this order:
 *   1  BELOW unless -score < (double)gap_prob_cutoff: the fill's own test, on the gapped score;
 *   2  else AMBIGUOUS unless ll_second is -inf or ll_seed - ll_second > min_margin (one IEEE subtraction);
 *   3  else RECRUITED.
 * min_margin is the caller's, finite and >= 0; 0.0 means "strictly better than any other locus".  No other value is built in.
 *
 * Out planes.  draw_pos[r] is the caller's offset for a KEPT read, off_seed for a RECRUITED read, else INT32_MIN; draw_isz[r] likewise
 * the caller's value, isz(off_seed), or 0.  n_candidates[g] and n_recruited[g] count the gap's candidates and its RECRUITED reads.
 *
 * Defaults, written by the library whatever the buffers held.  Reads of off gaps and KEPT reads: doubles 0.0, offsets INT32_MIN,
 * n_valid and d_end 0, read_state FIG_RECRUIT_READ_OFF or FIG_RECRUIT_KEPT, and the caller's draw values.  Off gaps: counts 0.
 *
 * Every double is a sum of table entries in a fixed order and every integer an exact comparison: all outputs are reproducible bit
 * for bit.  There is no exp10 in this pass.
 *
 * Limits: drawn reads are not moved; the seed is ungapped, so a read with two far-apart indels may seed on the wrong side of both,
 * and the band then finds at most a shift of 7; the support planes, draw.txt and filledContigs.fa remain the fill's; partial mode is
 * off; everything fig_read_placement and fig_gap_indel list. */
#define FIG_RECRUIT_OFF 0
#define FIG_RECRUIT_ON  1
#define FIG_RECRUIT_READ_OFF  0
#define FIG_RECRUIT_KEPT      1
#define FIG_RECRUIT_NONE      2
#define FIG_RECRUIT_BELOW     3
#define FIG_RECRUIT_AMBIGUOUS 4
#define FIG_RECRUIT_RECRUITED 5
typedef struct fig_read_recruit {
    double  *ll_seed;       /* [n_ureads] */
    double  *ll_second;     /* [n_ureads] */
    double  *ll_flat;       /* [n_ureads] */
    double  *ll_gapped;     /* [n_ureads] */
    double  *score;         /* [n_ureads] */
    int32_t *off_seed;      /* [n_ureads] */
    int32_t *off_second;    /* [n_ureads] */
    int32_t *n_valid;       /* [n_ureads] */
    int32_t *d_end;         /* [n_ureads] */
    uint8_t *read_state;    /* [n_ureads] FIG_RECRUIT_READ_OFF .. FIG_RECRUIT_RECRUITED */
    int32_t *draw_pos;      /* [n_ureads] the merged offsets */
    int32_t *draw_isz;      /* [n_ureads] the merged insert sizes */
    int32_t *n_candidates;  /* [n_gaps] */
    int32_t *n_recruited;   /* [n_gaps] */
    uint8_t *state;         /* [n_gaps] FIG_RECRUIT_OFF / FIG_RECRUIT_ON */
} fig_read_recruit;

/* Optional per-base quality over gapped read alignments (fig_batch_alnqual).  fig_gap_quality puts base j of a read on column o + j:
 * a read that spans an indel of the emitted string is then a run of mismatches from the site to its end and lowers the Phred of
 * columns that are correct.  Here every aligned read is piled up along the best path of fig_gap_indel's band, so that each base
 * counts on the column the alignment puts it on.  Terms not named here mean what they mean for fig_gap_quality (lm, le, lt, the
 * index k, the Phred rule) and for fig_gap_indel: S(x), n, which gaps are on, which reads are scored and aligned, the band with
 * W = 7, the cell update, the sweep, the end order, ll_gapped, d_end, d_start, n_ins, n_del.
 *
 * Gaps.  A gap is FIG_ALNQ_ON iff it is FIG_INDEL_ON.
 *
 * Path of an aligned read.  If ll_gapped is finite, fig_gap_indel's traceback from (len, d_end) along the back-pointers as they
 * stand; left-normalisation concerns the reporting of events and takes no part here.  If ll_gapped is -inf, the flat path: d = 0
 * throughout, d_start = d_end = 0, no events.
 *
 * Steps.  A DIAG step into cell (i, d) puts read base j = i-1 on column x = o* + j + d.  An INS step into (i, d) puts base i-1 on
 * no column.  A DEL step into (i, d) says the read SKIPS column x = o* + i + d - 1.  DIAG steps visit strictly increasing columns:
 * a read has at most one base on a column.  The columns of a path are o* + d_start <= x <= o* + len - 1 + d_end, and each of them
 * carries a base of the read or is skipped by it.
 *
 * Planes, over the columns 0 <= x < n of a gap that is on, compacted like str:
 *   loglik[x][b]  from 0.0, the aligned reads in ascending read index: a read with a base s in ACGT on x adds lm[k] if s == b, else
 *                 le[k] + lt[b][s]; every + is one IEEE double addition.  These are fig_gap_quality's terms.
 *   depth[x]      reads with an ACGT base on x
 *   agree[x]      those of depth[x] whose base is the emitted byte; 0 under a byte outside ACGT
 *   skip[x]       reads with a DEL step over x
 *   phred[x]      fig_gap_quality's rule applied to loglik[x] and the emitted byte, unchanged: a column no read puts a base on has
 *                 Phred 1 and shows in skip
 * Per read: ll_gapped, n_ins, n_del, d_end, d_start, equal to what fig_batch_indel returns for the same input.
 *
 * Defaults, written by the library whatever the buffers held.  Off gaps: planes 0, Phred 0.  Unaligned reads: ll_gapped = 0.0,
 * n_ins = n_del = d_end = 0, d_start = INT32_MIN.
 *
 * Every double is a sum of table entries in a fixed order: all outputs are reproducible bit for bit.  For a gap whose aligned reads
 * all have n_ins = n_del = 0 and d_end = 0, loglik and phred are fig_gap_quality's on the same input bit for bit.
 *
 * Limits: the band's limits listed for fig_gap_indel; one best path per read -- no sum over alignments; inserted bases and skipped
 * columns carry no likelihood term; reads are taken as independent and the prior is uniform, as for fig_gap_quality; partial mode
 * is off. */
#define FIG_ALNQ_OFF 0
#define FIG_ALNQ_ON  1
typedef struct fig_gap_alnqual {
    double  *loglik;     /* [str_off[n_gaps]*4]  (str_off[g]+x)*4 + b */
    int32_t *depth;      /* [str_off[n_gaps]] */
    int32_t *agree;      /* [str_off[n_gaps]] */
    int32_t *skip;       /* [str_off[n_gaps]] */
    uint8_t *phred;      /* [str_off[n_gaps]] */
    double  *ll_gapped;  /* [n_ureads] */
    int32_t *n_ins;      /* [n_ureads] */
    int32_t *n_del;      /* [n_ureads] */
    int32_t *d_end;      /* [n_ureads] */
    int32_t *d_start;    /* [n_ureads] */
    uint8_t *state;      /* [n_gaps] FIG_ALNQ_* */
} fig_gap_alnqual;

/* Timing/occupancy facts of the last fig_fill_gaps call (for bench.py). */
typedef struct fig_stats {
    double kernel_ms;                   /* HIP-event time of the fill kernels on the library's stream */
    double h2d_ms, d2h_ms;              /* transfers (0 when the batch was already resident) */
    int64_t packed_bytes;               /* algorithmic input bytes uploaded (2-bit bases + masks + descriptors) */
    int64_t place_calls;                /* placeReads invocations executed on the device     */
    double alg_flops;                   /* algorithmic FP64 flops, counted on device */
    int32_t n_launches;
    int32_t cont_chunks;                /* chunks of candidates continued inside an eval launch (0 under FIG_SCHED=rounds / seq) */
    double spec_flops;                  /* algorithmic flops of every candidate evaluation executed, discarded speculation included */
    double mle_alg_flops;               /* share of the executed evaluations' flops credited to the MLE passes (1 per placement and base) */
    double mle_exec_flops;              /* FP64 multiplies the MLE passes really executed (exact pruning skips the rest) */
} fig_stats;

int fig_version(void);
const char *fig_strerror(int code);

int fig_ctx_create(int device_ordinal, fig_ctx **out);
void fig_ctx_destroy(fig_ctx *ctx);
/* Sets the run-level model.  A batch left resident by fig_batch_upload is DROPPED (it was packed under the previous
 * model: launch classes, capacities and candidate ranges depend on it); upload again before fig_fill_resident. */
int fig_ctx_set_model(fig_ctx *ctx, const fig_model *model);

/* Worst-case bytes of results->str for this batch (sum of per-gap alloc_arg, Figbird.cpp:7395-7398). */
int64_t fig_results_capacity(const fig_model *model, const fig_gap_batch *batch);

/* Upload + pack a batch so that repeated fills run with inputs resident in HBM.
 * fig_fill_gaps(ctx, batch, out) == fig_batch_upload + fig_fill_resident + fig_batch_free. */
int fig_batch_upload(fig_ctx *ctx, const fig_gap_batch *batch);
int fig_fill_resident(fig_ctx *ctx, fig_gap_results *out);
/* fig_fill_resident that also hands back the per-base read support; sup == NULL is fig_fill_resident itself.  FIG_EINVAL
 * when sup is given with counts or origin NULL. */
int fig_fill_resident_ex(fig_ctx *ctx, fig_gap_results *out, const fig_gap_support *sup);
void fig_batch_free(fig_ctx *ctx);
int fig_fill_gaps(fig_ctx *ctx, const fig_gap_batch *batch, fig_gap_results *out);

/* The exact carry of Figbird.cpp's process-global overlap_threshold (:103, :6298-6317; read at :2684, :2760-2766).
 * fig_batch_probe_reach: reach[g] = 1 iff the candidate loop of gap g of the RESIDENT batch gets to :6317 -- it does
 * unless the loop has no candidate, or its first initialize() leaves side_limit < 10 (:6303), or the gap closes by a
 * negative overlap at its first candidate (:6305-6306); measured on the device before any gap is filled (none of it
 * depends on the threshold).  Unmapped-mode runs never read the global: reach is all 0 there and nothing is launched.
 * fig_batch_set_ot_preset: replaces gap_ot_preset of the resident batch ([n_gaps], batch order). */
int fig_batch_probe_reach(fig_ctx *ctx, uint8_t *reach);
int fig_batch_set_ot_preset(fig_ctx *ctx, const uint8_t *preset);

/* Per-base quality of the strings in `filled` against the RESIDENT batch (see fig_gap_quality).  `filled` holds what a fill of that
 * batch returned, or what a caller made by hand: filled_len, str_off, str and the three draw planes.  origin is
 * fig_gap_support::origin, or NULL for no origin test.  Reads the resident batch and the model and writes neither: a
 * fig_fill_resident after it gives the bytes it gave before.  FIG_EINVAL without a resident batch, with a needed pointer NULL,
 * with str_off not leaving filled_len[g] bytes to gap g, or with a drawn offset |o| >= 2^20 in a gap that is on.  With
 * FIG_SCHED_LOG set, one "[figqual]" line on stderr: gaps on, columns, reads, HIP-event milliseconds of the kernel. */
int fig_batch_quality(fig_ctx *ctx, const fig_gap_results *filled, const int32_t *origin, fig_gap_quality *q);

/* Placement confidence of the drawn unmapped reads of `filled` against the RESIDENT batch (see fig_read_placement); `filled` and
 * origin as for fig_batch_quality (draw_isz is not read).  Reads the resident batch and the model and writes neither.  FIG_EINVAL
 * without a resident batch, with a needed pointer NULL, with str_off not leaving filled_len[g] bytes to gap g, or with a drawn
 * offset |o| >= 2^20 in a gap that is on.  With FIG_SCHED_LOG set, one "[figplace]" line on stderr: gaps on, reads scored,
 * placements scored, HIP-event milliseconds of the kernel. */
int fig_batch_placement(fig_ctx *ctx, const fig_gap_results *filled, const int32_t *origin, fig_read_placement *p);

/* Per-base quality summed over read placements, of `filled` against the RESIDENT batch (see fig_gap_softqual); `filled` and origin as
 * for fig_batch_placement, and the same FIG_EINVAL conditions (a NULL member of `out`, or of `placement_or_null` when that is given,
 * included).  Two launches on the library's stream with no host round trip between them: the placement pass into per-call buffers,
 * then the pass that reads them.  placement_or_null, when given, is filled exactly as fig_batch_placement fills it: one call yields
 * both.  Reads the resident batch and the model and writes neither.  With FIG_SCHED_LOG set, one "[figsoftq]" line on stderr: gaps
 * on, columns, reads, active placements, HIP-event milliseconds of each of the two launches. */
int fig_batch_softqual(fig_ctx *ctx, const fig_gap_results *filled, const int32_t *origin,
                       fig_read_placement *placement_or_null, fig_gap_softqual *out);

/* Indel evidence of the drawn unmapped reads of `filled` against the RESIDENT batch (see fig_gap_indel); `filled` and origin as for
 * fig_batch_placement (draw_isz is not read), and the same FIG_EINVAL conditions, a NULL member of `out` included.  Reads the resident
 * batch and the model and writes neither.  With FIG_SCHED_LOG set, one "[figindel]" line on stderr: gaps on, reads aligned, reads
 * with an event, columns called, HIP-event milliseconds of the kernel. */
int fig_batch_indel(fig_ctx *ctx, const fig_gap_results *filled, const int32_t *origin, fig_gap_indel *out);

/* Polish of the strings in `filled` against the RESIDENT batch (see fig_gap_polish); `filled` and origin as for fig_batch_indel.
 * max_rounds: 1..8, or 0 for the default of 4.  FIG_EINVAL under fig_batch_indel's conditions (they hold for the shifted offsets
 * too), with a NULL member of `out`, or with max_rounds outside 0..8.  Reads the resident batch and the model and writes neither;
 * the caller's `filled` is never changed.  At most max_rounds + 1 launches of the indel kernel and max_rounds of the polish kernel.
 * With FIG_SCHED_LOG set, one "[figpolish]" line on stderr: gaps on, rounds, sites, candidates scored, edits accepted, rejected and
 * reverted, HIP-event milliseconds of the indel launches and of the polish launches. */
int fig_batch_polish(fig_ctx *ctx, const fig_gap_results *filled, const int32_t *origin, int max_rounds, fig_gap_polish *out);

/* The polished string of gap g from the caller's strings and the edit planes of `p`: writes polished_len[g] bytes to dst (nothing when
 * dst is NULL) and returns that length, or a negative FIG_E* code.  Needs no context and no device. */
int fig_polish_apply(const fig_gap_results *filled, const fig_gap_polish *p, int64_t g, char *dst);

/* Recruiting of the undrawn unmapped reads of `filled` against the RESIDENT batch (see fig_read_recruit); `filled` and origin as for
 * fig_batch_indel (draw_isz is read: it is carried into the merged plane).  FIG_EINVAL under fig_batch_indel's conditions, with
 * draw_isz or a member of `out` NULL, or with min_margin negative, infinite or NaN.  Reads the resident batch and the model (the cutoff
 * is the gap_prob_cutoff of the model that was set) and writes neither; the caller's `filled` is never changed.  One launch.  With
 * FIG_SCHED_LOG set, one "[figrecruit]" line on stderr: gaps on, candidates, seeded, recruited, below, ambiguous, placements scored,
 * HIP-event milliseconds of the kernel. */
int fig_batch_recruit(fig_ctx *ctx, const fig_gap_results *filled, const int32_t *origin, double min_margin, fig_read_recruit *out);

/* Per-base quality over the gapped alignments of the drawn unmapped reads of `filled` against the RESIDENT batch (see
 * fig_gap_alnqual); `filled` and origin as for fig_batch_indel.  FIG_EINVAL under fig_batch_indel's conditions and with a NULL member
 * of `out`.  Reads the resident batch and the model and writes neither; the caller's `filled` is never changed.  Two launches on the
 * library's stream with no host round trip between them: the paths into per-call buffers, then the columns.  With FIG_SCHED_LOG set,
 * one "[figalnqual]" line on stderr: gaps on, reads aligned, reads with an event, columns, HIP-event milliseconds of each of the two
 * launches. */
int fig_batch_alnqual(fig_ctx *ctx, const fig_gap_results *filled, const int32_t *origin, fig_gap_alnqual *out);

int fig_get_stats(const fig_ctx *ctx, fig_stats *out);

#ifdef __cplusplus
}
#endif
#endif /* FIGBIRD_HIP_H */
