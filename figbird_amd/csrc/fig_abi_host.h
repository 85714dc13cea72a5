// fig_abi_host.h -- the host logic of the C ABI (include/figbird_hip.h) that does not touch a device: error strings, model
// checks and tables, the environment knobs, the round planner of the candidate-parallel scheduler, result compaction.
// Pure C++ (no HIP): compiled into libfighip.so (fig_abi.hip) and into the one-lane emulation the CPU tests run
// (tools/emu/fig_emu_abi.cpp), so that every decision below is made in one place and the CPU suite checks the shipped code.
#ifndef FIG_ABI_HOST_H
#define FIG_ABI_HOST_H
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../include/figbird_hip.h"
#include "fig_types.h"
#include "fig_gaprules.h"
// (fig_engine.h and fig_pack.h must already be included: FigKernArgs, FigLaunchClass and fig_model_fmm come from them)

static_assert(FIG_ORG_NONE == FIG_SUP_NONE && FIG_ORG_FINAL == FIG_SUP_FINAL && FIG_ORG_ORIGINAL == FIG_SUP_ORIGINAL && FIG_ORG_TIEBREAK == FIG_SUP_TIEBREAK,
              "the engine's path mask (fig_types.h) is fig_gap_support::origin");

static inline const char *fig_strerror_text(int code) {
    switch (code) {
        case FIG_OK: return "ok";
        case FIG_EINVAL: return "invalid argument";
        case FIG_ENODEV: return "no usable HIP device (libfighip has no CPU path)";
        case FIG_ENOMEM: return "out of memory";
        case FIG_EHIP: return "HIP runtime error";
        case FIG_ENOSPC: return "result string buffer too small";
        case FIG_EUNSUP: return "input outside the supported envelope";
        default: return "unknown error";
    }
}

// ------------------------------------------------------------------------------------- model
static inline int fig_model_check(const fig_model *m) {
    if (!m || !m->error_pos_dist || !m->in_pos_dist || !m->del_pos_dist || !m->insert_len_dist_smoothed) return FIG_EINVAL;
    if (m->max_read_length <= 0 || m->max_read_length > FIG_MAX_READLEN) return FIG_EUNSUP;
    if (m->max_insert_size <= 0) return FIG_EINVAL;
    if (m->partial_flag && m->unmapped_flag) return FIG_EUNSUP;      // the driver never sets both (RunFigbird.sh:211-216)
    if (m->insert_threshold_min < 0 || m->insert_threshold_max >= m->max_insert_size + 1) return FIG_EINVAL;
    return FIG_OK;
}

// Offsets (in doubles) of the model tables inside the one contiguous vector fig_model_tables() fills; every table starts
// on a 64-byte boundary of it.
struct FigModelOffsets { size_t e, pairs, m3, insd, qtab, ome; };

// Fills `all` with the tables of FigDevModel and `dm` with its scalars.  The pointers of `dm` are set by
// fig_model_point() once the caller knows where `all` lives (the device copy for libfighip, the vector itself for the
// emulation).
static void fig_model_tables(const fig_model *m, std::vector<double> &all, FigModelOffsets &o, FigDevModel &dm) {
    const int L = m->max_read_length;
    std::vector<double> h_e(m->error_pos_dist, m->error_pos_dist + L), h_ome(L), h_m3(L);
    for (int k = 0; k < L; k++) {
        volatile double a = 1 - m->error_pos_dist[k];                 // (1-errorPosDist[k])               Figbird.cpp:3160
        h_ome[k] = a;
        volatile double b = 1 - m->error_pos_dist[k] - m->in_pos_dist[k] - m->del_pos_dist[k];   // Figbird.cpp:3400
        h_m3[k] = b;
    }
    std::vector<double> h_insd(m->insert_len_dist_smoothed, m->insert_len_dist_smoothed + m->max_insert_size);
    h_insd.push_back(0.0);                                            // insertThresholdMax may equal maxInsertSize (:7194)
    std::vector<double> h_qtab(256);
    for (int c = 0; c < 256; c++) { int Q = c - 33; h_qtab[c] = pow(10, -Q / 10.0); }   // qualityFilter, :1791-1792
    // pair tables for scalar loads: kt = {1-e[k], e[k]}, mt = {1-e-ins-del, e[k]}; the reversed copies serve
    // reverse-strand reads (readIndex = len-1-j, Figbird.cpp:3569-3576) as rev[(L-len)+j]
    std::vector<double> pairs((size_t)8 * L);
    for (int k = 0; k < L; k++) {
        pairs[2 * k] = h_ome[k]; pairs[2 * k + 1] = h_e[k];
        pairs[2 * L + 2 * k] = h_ome[L - 1 - k]; pairs[2 * L + 2 * k + 1] = h_e[L - 1 - k];
        pairs[4 * L + 2 * k] = h_m3[k]; pairs[4 * L + 2 * k + 1] = h_e[k];
        pairs[6 * L + 2 * k] = h_m3[L - 1 - k]; pairs[6 * L + 2 * k + 1] = h_e[L - 1 - k];
    }
    all.clear();
    o.e = 0; all.insert(all.end(), h_e.begin(), h_e.end()); while (all.size() % 8) all.push_back(0);
    o.pairs = all.size(); all.insert(all.end(), pairs.begin(), pairs.end()); while (all.size() % 8) all.push_back(0);
    o.m3 = all.size(); all.insert(all.end(), h_m3.begin(), h_m3.end()); while (all.size() % 8) all.push_back(0);
    o.insd = all.size(); all.insert(all.end(), h_insd.begin(), h_insd.end()); while (all.size() % 8) all.push_back(0);
    o.qtab = all.size(); all.insert(all.end(), h_qtab.begin(), h_qtab.end());
    o.ome = all.size(); all.insert(all.end(), h_ome.begin(), h_ome.end());
    dm.L = L; dm.Tmin = m->insert_threshold_min; dm.Tmax = m->insert_threshold_max; dm.cutoff = m->gap_prob_cutoff;
    dm.partial_flag = m->partial_flag; dm.unmapped = m->unmapped_flag; dm.script_itr = m->script_itr; dm.D = m->max_distance;
    dm.read_length = m->read_length; dm.neg_overlap = m->neg_overlap; dm.partial_len = m->partial_len; dm.unm_limit = m->unm_limit;
    dm.max_insert = m->max_insert_size;
    for (int i = 0; i < 25; i++) dm.T[i] = m->error_type_probs[i];
    dm.fmm_up = fig_model_fmm(m);
}

static inline void fig_model_point(FigDevModel &dm, const FigModelOffsets &o, const double *d) {
    dm.e = d + o.e; dm.ome = d + o.pairs; dm.m3 = d + o.m3; dm.insd = d + o.insd; dm.qtab = d + o.qtab;
    dm.ome1 = d + o.ome;
}

// ------------------------------------------------------------------------------------- batch
// the optional debug / draw / support planes of a fill: absent unless the call that launches sets them
static inline void fig_batch_clear_planes(FigDevBatch &db) {
    db.dbg_n_cand = nullptr; db.dbg_cand_i = nullptr; db.dbg_cand_lik = nullptr; db.dbg_max_cand = 0; db.dbg_n_place = nullptr;
    db.draw_pos = db.draw_isz = db.draw_len = nullptr;
    db.dbg_counts = db.dbg_read_maxlv = nullptr; db.dbg_plane_cols = db.dbg_plane_reads = 0;
    db.sup_counts = db.sup_origin = nullptr;
}

// An optional plane of a fill (fig_gap_results' dbg_* / draw_*, fig_gap_support): the FigDevBatch field the engine writes through, where
// the caller wants it, its size, and the byte it is cleared to before the launches (< 0: not cleared, the engine writes all that is read).
struct FigPlane { void **dev; void *host; size_t bytes; int fill; };

// The planes this call asked for, each described once; everything else of db's optional part is switched off.  n_reads:
// unmapped + partial reads of the batch; sup_host: str_total * 5 int32 (one slot per string slot, compacted afterwards).
static std::vector<FigPlane> fig_fill_planes(FigDevBatch &db, int64_t n_reads, int64_t str_total, const fig_gap_results *out, const fig_gap_support *sup, int32_t *sup_host) {
    std::vector<FigPlane> pl;
    auto add = [&](auto *&dev, void *host, size_t bytes, int fill) { pl.push_back(FigPlane{(void **)&dev, host, bytes, fill}); };
    const size_t ng = (size_t)db.n_gaps, nr = (size_t)n_reads;
    fig_batch_clear_planes(db);
    if (out->dbg_n_cand && out->dbg_cand_i && out->dbg_cand_lik && out->dbg_max_cand > 0) {      // candidate trace
        const size_t nc = ng * out->dbg_max_cand;
        db.dbg_max_cand = out->dbg_max_cand;
        add(db.dbg_n_cand, out->dbg_n_cand, ng * 4, 0);
        add(db.dbg_cand_i, out->dbg_cand_i, nc * 12, -1);
        add(db.dbg_cand_lik, out->dbg_cand_lik, nc * 8, -1);
        if (out->dbg_n_place) add(db.dbg_n_place, out->dbg_n_place, ng * 4, 0);
        if (out->dbg_counts && out->dbg_plane_cols > 0) { db.dbg_plane_cols = out->dbg_plane_cols; add(db.dbg_counts, out->dbg_counts, nc * out->dbg_plane_cols * 5 * 8, 0); }
        if (out->dbg_read_maxlv && out->dbg_plane_reads > 0) { db.dbg_plane_reads = out->dbg_plane_reads; add(db.dbg_read_maxlv, out->dbg_read_maxlv, nc * out->dbg_plane_reads * 8, 0); }
    }
    if (out->draw_pos && out->draw_isz && out->draw_len) {
        add(db.draw_pos, out->draw_pos, nr * 4, -1);
        add(db.draw_isz, out->draw_isz, nr * 4, 0);
        add(db.draw_len, out->draw_len, ng * 8, -1);
    }
    if (sup) {                        // per-base read support: zero unless fig_gap_end writes it
        add(db.sup_counts, sup_host, (size_t)str_total * 5 * 4, 0);
        add(db.sup_origin, sup->origin, ng * 4, 0);
    }
    return pl;
}

// fig_stats' counter fields, from a read-back of FigDevBatch::counters
static inline void fig_stats_from_counters(const unsigned long long *cnt, fig_stats &st) {
    st.place_calls = (int64_t)cnt[FIG_CNT_PLACE];
    st.alg_flops = (double)cnt[FIG_CNT_FLOPS]; st.spec_flops = (double)cnt[FIG_CNT_SPEC];
    st.mle_alg_flops = (double)cnt[FIG_CNT_MLE_ALG]; st.mle_exec_flops = (double)cnt[FIG_CNT_MLE_EXEC];
    st.cont_chunks = (int32_t)cnt[FIG_CNT_CONT];
}

// the launch arguments of a class (FigKernArgs, fig_engine.h)
static FigKernArgs fig_kargs_of(const FigLaunchClass &c, int qsel, int sh_on) {
    FigKernArgs A;
    A.capG = c.capG; A.capGl = c.capGl; A.ncolE = c.ncolE; A.Wcap = c.Wcap; A.nteams = c.nteams;
    A.q_begin = c.q_begin; A.q_end = c.q_end; A.qsel = qsel;
    A.tiles = c.tiles; A.tile_step = c.tile_step; A.tile_cols = c.tile_cols; A.tiled_max = c.tiled_max;
    A.sh_on = sh_on;
    return A;
}

// An upload without fig_gap_batch::gap_ot_preset in partial mode: the batch is ONE worker process of the reference taking
// its gaps in batch order -- measure which gaps get to Figbird.cpp:6317 and hand every gap the prefix-OR of its
// predecessors.  Written on the two public calls, which both builds define.
static int fig_ot_carry_measured(fig_ctx *ctx, int64_t ng) {
    std::vector<uint8_t> reach((size_t)ng, 0), preset((size_t)ng, 0);
    int rc;
    if ((rc = fig_batch_probe_reach(ctx, reach.data()))) return rc;
    std::vector<int64_t> ids((size_t)ng);
    for (int64_t g = 0; g < ng; g++) ids[(size_t)g] = g;
    fig_ot_carry(ids, reach.data(), preset.data());
    return fig_batch_set_ot_preset(ctx, preset.data());
}

// Result strings: from one slot per gap at src_off[g] (`src`) to back-to-back in out->str, with out->str_off.
static int fig_compact_results(int64_t ng, const char *src, const int64_t *src_off, fig_gap_results *out) {
    int64_t need = 0;
    for (int64_t g = 0; g < ng; g++) need += out->filled_len[g] > 0 ? out->filled_len[g] : 0;
    if (need > out->str_capacity) return FIG_ENOSPC;
    int64_t o = 0;
    for (int64_t g = 0; g < ng; g++) {
        out->str_off[g] = o;
        int n = out->filled_len[g];
        if (n > 0) { memcpy(out->str + o, src + src_off[g], (size_t)n); o += n; }
    }
    out->str_off[ng] = o;
    return FIG_OK;
}

// The support plane travels with the strings: five int32 per string byte, from the slot at src_off[g] * 5 to
// out->str_off[g] * 5 (after fig_compact_results has set out->str_off).
static void fig_compact_support(int64_t ng, const int32_t *src, const int64_t *src_off, const fig_gap_results *out, int32_t *dst) {
    for (int64_t g = 0; g < ng; g++) {
        int n = out->filled_len[g];
        if (n > 0) memcpy(dst + out->str_off[g] * 5, src + src_off[g] * 5, (size_t)n * 5 * sizeof(int32_t));
    }
}

// fig_fill_gaps: upload + fill + free, on the public calls
static int fig_fill_gaps_once(fig_ctx *ctx, const fig_gap_batch *batch, fig_gap_results *out) {
    int rc = fig_batch_upload(ctx, batch);
    if (rc) return rc;
    rc = fig_fill_resident(ctx, out);
    fig_batch_free(ctx);
    return rc;
}

// ------------------------------------------------------------------------------------- knobs
// Every environment variable the ABI layer reads, in one place.  The scheduling knobs hold for one fig_fill_resident call:
// it reads them on the calling thread before any lane thread starts and passes them down.  sh_on holds for a context
// (the value read at fig_ctx_create).  fig_batch_upload reads `log` for its class listing.
struct FigKnobs {
    bool seq;            // FIG_SCHED=seq: whole gaps, one workgroup each
    // FIG_SCHED=rounds: every chunk of every gap is a host round (eval launch + replay launch), the default in partial mode.
    // FIG_SCHED=continuous, the default in unmapped mode: the
    // eval launch replays a gap when its chunk is done and continues it in place (fig_engine_sched.h: fig_item_continue); the
    // host's rounds start the gaps and mop up.  Its knobs: FIG_CONT_CAP=<n> caps the lane's continuation array (tests: 1 forces
    // the fall-back to host rounds); FIG_CONT_LIVE=<percent> a chunk of n is continued while live workgroups * 100 >= n * percent
    // (0: always -- one workgroup may then run a whole chain of chunks alone); FIG_CONT_PRIO=0 hands continuations out oldest
    // first instead of longest remaining chain first
    bool cont; int cont_cap, cont_live, cont_prio;
    // FIG_WIDE=0|grow|idle|both: wide chunks for the gaps that keep running, in the continuous form only (fig_engine_sched.h:
    // fig_wide_chunk).  grow: a continued chunk may be twice the gap's last one; idle: it may take the workgroups that would
    // find nothing to do; 0: the schedule without it, launch for launch.  Default: grow in unmapped mode (DESIGN 5b has the
    // measurements), 0 in partial mode, whose gaps stop after a fifth of their candidates.  FIG_SLOTS_WIDE=<n>, read at
    // fig_batch_upload: the wide cap W -- a gap owns min(its candidates, W) slots; default 256, never below the 64 base slots
    // FIG_WIDE_MAX_ACTIVE=<n>, default 96: growth only while the lane's largest active set so far is at most n gaps.  A lane
    // with hundreds of active gaps is throughput-bound, not chain-bound: grown chunks there only add discarded evaluations and
    // more gaps' reads in flight (2 048 gaps: +6 % with growth everywhere); 96 is where fig_plan_round starts
    // lengthening its rounds for the same reason.  Idle-driven widening needs no gate: such a lane has no spare workgroups
    int wide, slots_wide, wide_max_active;
    bool lanes_serial;   // FIG_LANES=serial: the class lanes one after the other on the calling thread
    bool log;            // FIG_SCHED_LOG
    int minc;            // FIG_MIN_CHUNK: candidates per gap and round, at least
    double ipw;          // FIG_ITEMS_PER_WG: items per resident workgroup and round (partial-mode pass, 8 192 gaps: 6 -> 4 052 gaps/s, 12 -> 3 887, 24 -> 3 875, 48 -> 3 668: shorter rounds discard fewer candidates past an early stop; unmapped, measured on the bench batch: 4 -> 34.4 s, 8 -> 29.7, 12 -> 29.1, 16 -> 29.2 per step)
    // FIG_ESTEP=pair: the pair-chain E-step everywhere (A/B runs, tests); FIG_SH_CHUNKS=<1..4>: chunks per super-chunk of the
    // shared-factor E-step (fig_engine_shared.h; default 4: bench step 24.3 s with 2, 23.9 s with 4)
    int sh_on;
    // FIG_MLE_REUSE=0: every unmapped placeReads call runs its MLE pass; default (on, unmapped mode only): a call whose E-step
    // consensus equals that of the candidate's previous call takes the previous pass's outputs (fig_engine_core.h: fig_mle_reuse_*)
    int mle_reuse;
};

#define FIG_WIDE_DEFAULT_UNMAPPED FIG_WIDE_GROW
#define FIG_SLOTS_WIDE_MAX 4096      // FIG_SLOTS_WIDE at most
static FigKnobs fig_knobs_from_env(int unmapped) {
    FigKnobs k;
    const char *sched = getenv("FIG_SCHED"), *ser = getenv("FIG_LANES"), *mc = getenv("FIG_MIN_CHUNK"), *ipw = getenv("FIG_ITEMS_PER_WG");
    const char *ev = getenv("FIG_ESTEP"), *sc = getenv("FIG_SH_CHUNKS");
    k.seq = sched && strcmp(sched, "seq") == 0;
    const char *cc = getenv("FIG_CONT_CAP"), *cl = getenv("FIG_CONT_LIVE"), *cp = getenv("FIG_CONT_PRIO");
    k.cont = sched ? strcmp(sched, "continuous") == 0 : unmapped != 0;      // partial mode stays with the rounds: its items take ~1 ms, and the hand-over costs its 8 192-gap pass 15 %
    k.cont_cap = cc ? std::max(1, atoi(cc)) : FIG_CONT_CAP_MAX;
    k.cont_live = cl ? std::max(0, atoi(cl)) : 100;
    k.cont_prio = cp ? (atoi(cp) != 0) : 1;
    const char *wd = getenv("FIG_WIDE"), *sw = getenv("FIG_SLOTS_WIDE");
    k.wide = !wd ? (unmapped ? FIG_WIDE_DEFAULT_UNMAPPED : 0) : !strcmp(wd, "grow") ? FIG_WIDE_GROW : !strcmp(wd, "idle") ? FIG_WIDE_IDLE : !strcmp(wd, "both") ? (FIG_WIDE_GROW | FIG_WIDE_IDLE) : 0;
    if (!k.cont) k.wide = 0;
    k.slots_wide = sw ? atoi(sw) : 256;
    const char *wa = getenv("FIG_WIDE_MAX_ACTIVE");
    k.wide_max_active = wa ? std::max(0, atoi(wa)) : 96;
    k.lanes_serial = ser && strcmp(ser, "serial") == 0;
    k.log = getenv("FIG_SCHED_LOG") != nullptr;
    k.minc = mc ? std::max(1, atoi(mc)) : 16;
    k.ipw = ipw ? std::max(1.0, atof(ipw)) : (unmapped ? 12.0 : 6.0);
    k.sh_on = (ev && !strcmp(ev, "pair")) ? 0 : (sc ? std::max(1, std::min(FIG_SH_SC, atoi(sc))) : FIG_SH_SC);
    const char *mr = getenv("FIG_MLE_REUSE");
    k.mle_reuse = unmapped != 0 && !(mr && !strcmp(mr, "0"));
    return k;
}

// ------------------------------------------------------------------------------------- round planner
// One round of the candidate-parallel scheduler (fig_engine_sched.h) for one class lane: which active gaps take part and
// how many candidates each of them evaluates.  One entry per admitted gap (one replay each), one item per evaluation.
struct FigRound { std::vector<FigItem> items; std::vector<FigEntry> entries; int chunk = 0, n_active = 0; };

// ids: the lane's gaps in cost order; ctl: gapctl snapshot of the batch; capacity: workgroups the device holds for this class;
// nsplit: lanes the class runs as; slots_cap: candidate slots of a gap's chunk; n_active_max: the lane's largest active set so far
// (in/out).  n_active == 0 on return: nothing left, no round.  wide_mode / wide_cap (FIG_WIDE, FIG_SLOTS_WIDE): a gap that
// comes back with j > 0 has had its last chunk (FigGapCtl::last) consumed to its end and may get a wider one by the rule of
// fig_wide_chunk -- grown in any round, and up to the lane's share of workgroups the round leaves idle when the round admits
// every active gap and still holds fewer items than that share.  A gap's first chunk (j == 0) and everything with
// wide_cap <= slots_cap or wide_mode 0 is as without it; growth is off once the lane's active set has been above wide_max_active.
static inline int fig_wide_for_lane(int wide_mode, int n_active_max, int wide_max_active) {      // FIG_WIDE bits in force for a lane (FIG_WIDE_MAX_ACTIVE)
    return n_active_max > wide_max_active ? (wide_mode & ~FIG_WIDE_GROW) : wide_mode;
}

static void fig_plan_round(const std::vector<int> &ids, const FigGapCtl *ctl, int capacity, int nsplit, int slots_cap, int wide_mode, int wide_cap, int wide_max_active, int minc, double ipw_base,
                           int &n_active_max, FigRound &R) {
    R.items.clear(); R.entries.clear();
    R.chunk = 0; R.n_active = 0;
    for (int g : ids) if (ctl[g].status == FIG_GAP_MORE) R.n_active++;
    if (R.n_active == 0) return;
    // Candidates per gap this round: proportional to the candidates the gap still has, so that all gaps of the class
    // finish in about the same round and every round carries ~12 items per resident workgroup (of both lanes of a split class).  A gap that stops
    // early discards at most chunk-1 evaluations.
    long long rem_total = 0;
    for (int g : ids) if (ctl[g].status == FIG_GAP_MORE) rem_total += std::max(0, ctl[g].range - ctl[g].j);
    // Round size: `ipw_base` items per resident workgroup while the lane has about a hundred active gaps (the 512-gap bench
    // batch: 12 is its optimum), growing with the lane's number of active gaps (its maximum so far) up to 8x.  Measured on one box (round 3,
    // profiles/round3/largefill_*): the 2048-gap fill of the bench recipe takes 111.9 s with 12 items per workgroup and
    // round (121 rounds per lane of 1920 items over 385 active gaps: every round ends with a tail of the long items of
    // the most expensive gaps), 99.8 s with 48 and 98.5 s with 96 -- while 48 costs the 512-gap batch 3 %.
    n_active_max = std::max(n_active_max, R.n_active);
    wide_mode = fig_wide_for_lane(wide_mode, n_active_max, wide_max_active);
    const double ipw = ipw_base * std::min(8.0, std::max(1.0, n_active_max / 96.0));      // by the lane's largest active set: the rounds stay long to the end of a big fill
    const double share = rem_total > 0 ? (ipw * capacity / (double)std::max(1, nsplit)) / (double)rem_total : 1.0;
    // Admission: a gap gets at least `minc` candidates in a round it takes part in, and gaps are admitted in cost order
    // until the round is full.  With thousands of active gaps the proportional share alone would hand every gap a few
    // candidates per round: hundreds of rounds per gap and, worse, hundreds of DIFFERENT gaps in flight at once, whose
    // reads then miss the L2 (a 2048-gap fill ran at 0.33 of peak against 0.37 for 512 gaps).  Workgroups that pop
    // neighbouring items work on the same gap's reads.
    const double target = ipw * capacity / (double)std::max(1, nsplit);
    long long total = 0;
    for (int g : ids) {
        if (ctl[g].status != FIG_GAP_MORE) continue;
        if ((double)total >= 1.25 * target) break;           // the rest waits for a later round
        int j = ctl[g].j, range = ctl[g].range;
        int want = (int)std::ceil((range - j) * share);
        want = std::min(std::max(want, minc), slots_cap);
        int n = std::max(0, std::min(want, range - j));       // (0: replayed with nothing to evaluate: the replay closes the gap)
        if (j > 0 && n > 0 && (wide_mode & FIG_WIDE_GROW) && wide_cap > slots_cap)
            n = std::max(n, fig_wide_chunk(FigWide{FIG_WIDE_GROW, slots_cap, wide_cap}, 1, ctl[g].last, wide_cap, range - j, 1, 0));
        total += n;
        R.entries.push_back(FigEntry{g, n, 0, 0});
    }
    if ((wide_mode & FIG_WIDE_IDLE) && wide_cap > slots_cap && (int)R.entries.size() == R.n_active) {
        long long spare = (long long)(capacity / std::max(1, nsplit)) - total;      // workgroups of the lane's share this round leaves without an item
        for (FigEntry &en : R.entries) {
            const int j = ctl[en.gap].j, left = ctl[en.gap].range - j;
            if (spare <= 0) break;
            if (j == 0 || en.n == 0) continue;
            const int n = fig_wide_chunk(FigWide{FIG_WIDE_IDLE, slots_cap, wide_cap}, en.n, en.n, wide_cap, left, 1, (int)std::min<long long>(en.n + spare, wide_cap));
            if (n > en.n) { spare -= n - en.n; total += n - en.n; en.n = n; }
        }
    }
    for (const FigEntry &en : R.entries) R.chunk = std::max(R.chunk, en.n);
    // items gap-major in descending-cost gap order (longest processing time first keeps the round's tail short)
    for (const FigEntry &en : R.entries)
        for (int k = en.n - 1; k >= 0; k--) R.items.push_back(FigItem{en.gap, ctl[en.gap].j + k, k, 0});
}

// The continuous form of a planned round: every item carries the size of its gap's chunk (the workgroup that finishes the
// chunk's last item replays the gap), every entry the j it was planned at (the replay kernel then takes only the gaps no
// eval workgroup replayed: those with nothing to evaluate).  Returns the number of such entries.
static int fig_round_stamp(FigRound &R, const FigGapCtl *ctl) {
    size_t pos = 0; int n_empty = 0;
    for (FigEntry &en : R.entries) {
        en.j_planned = ctl[en.gap].j; en.stamped = 1;
        if (en.n == 0) n_empty++;
        for (int k = 0; k < en.n; k++) R.items[pos++].chunk = en.n;
    }
    return n_empty;
}

// Entries of a lane's continuation array: enough for every gap of `ids` to go through its whole range within one launch in chunks
// of `minc` (FIG_MIN_CHUNK as it stands at upload), plus the end item and the last short chunk.  A fill with a smaller
// FIG_MIN_CHUNK may find the array full; the gap is then left to the host's next round.
// (Wide chunks only make a gap's chunks fewer.)
static int fig_cont_capacity(const std::vector<int> &ids, const std::vector<FigDevGap> &gaps, int minc) {
    long long n = 0;
    for (int g : ids) n += gaps[(size_t)g].rangeCap / std::max(1, minc) + 3;
    return (int)std::min<long long>(std::max<long long>(n, 1), FIG_CONT_CAP_MAX);
}

// Items / entries a lane's buffers hold: a round has at most one chunk per gap, a chunk at most the gap's slots; one more
// record per gap for the entries and the end list.
static size_t fig_lane_items(const std::vector<int> &ids, const std::vector<FigDevGap> &gaps) {
    size_t n = 0;
    for (int g : ids) n += (size_t)gaps[(size_t)g].nslots + 1;
    return std::max<size_t>(n, 1);
}

#endif
