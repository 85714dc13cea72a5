// figfill -- drop-in for the reference's gap-fill stage.  RunFigbird.sh:352/:480 runs
//   g++ -std=c++11 -pthread FillGaps.cpp && ./a.out <15 args>
// figfill takes the same 15 positional arguments (FillGaps.cpp:419-433), reads the same
// files Preprocess.cpp left behind and writes the same outputs (Temp/filledContigs.fa,
// gapout.txt, draw.txt, Ncount.txt) -- but instead of fanning out `g++ Figbird.cpp`
// processes it builds the model once, packs every gap into one batch and hands it to the
// MI355X engine through the C ABI of include/figbird_hip.h.  Exit codes follow the
// reference: message on stderr + exit(1).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include <chrono>
#include <thread>

#include "fig_host.h"
#include "fig_sam.h"

using namespace fighost;

// Eight calls of the ABI a library behind figfill may lack (the one-lane emulation of the CPU tests implements the calls it was
// written against): bound weakly, and asking for what they compute without them is an error before anything is filled or written.
extern "C" int fig_fill_resident_ex(fig_ctx *, fig_gap_results *, const fig_gap_support *) __attribute__((weak));
extern "C" int fig_batch_quality(fig_ctx *, const fig_gap_results *, const int32_t *, fig_gap_quality *) __attribute__((weak));
extern "C" int fig_batch_placement(fig_ctx *, const fig_gap_results *, const int32_t *, fig_read_placement *) __attribute__((weak));
extern "C" int fig_batch_softqual(fig_ctx *, const fig_gap_results *, const int32_t *, fig_read_placement *, fig_gap_softqual *) __attribute__((weak));
extern "C" int fig_batch_indel(fig_ctx *, const fig_gap_results *, const int32_t *, fig_gap_indel *) __attribute__((weak));
extern "C" int fig_batch_polish(fig_ctx *, const fig_gap_results *, const int32_t *, int, fig_gap_polish *) __attribute__((weak));
extern "C" int fig_batch_recruit(fig_ctx *, const fig_gap_results *, const int32_t *, double, fig_read_recruit *) __attribute__((weak));
extern "C" int fig_batch_alnqual(fig_ctx *, const fig_gap_results *, const int32_t *, fig_gap_alnqual *) __attribute__((weak));

// The optional outputs: read from the environment once, in main(), and passed down.
//   FIGFILL_SUPPORT=1    also the per-base read support and <tmp>/gapsupport.txt
//   FIGFILL_QUALITY=1    the fill with the support call (for the origins), then fig_batch_quality, and <tmp>/gapquality.txt
//   FIGFILL_PLACEMENT=1  the fill with the support call, then fig_batch_placement, and <tmp>/gapplacement.txt
//   FIGFILL_SOFTQUALITY=1  the fill with the support call, then fig_batch_softqual, and <tmp>/gapsoftquality.txt
//   FIGFILL_INDEL=1      the fill with the support call, then fig_batch_indel, and <tmp>/gapindel.txt
//   FIGFILL_POLISH=1     the fill with the support call, then fig_batch_polish (FIGFILL_POLISH_ROUNDS=<k>: its max_rounds), and
//                        <tmp>/gappolished.txt; filledContigs.fa keeps the unpolished strings
//   FIGFILL_RECRUIT=1    the fill with the support call, then fig_batch_recruit (FIGFILL_RECRUIT_MARGIN=<x>: its min_margin, default
//                        0), and <tmp>/gaprecruit.txt; FIGFILL_INDEL and FIGFILL_POLISH then run on the merged draw plane, every
//                        other pass and every other file sees the fill's own
//   FIGFILL_ALNQUALITY=1 the fill with the support call, then fig_batch_alnqual on the end of the chain -- the fill's strings and draw
//                        plane, the merged plane under FIGFILL_RECRUIT=1, the polished strings with the polish's shifted offsets under
//                        FIGFILL_POLISH=1 (n is then the polished length) -- and <tmp>/gapalnquality.txt
//   FIGFILL_QUALITY_MINPQ=<k> (only together with FIGFILL_QUALITY=1): the quality leaves out scored reads with pq < k
struct Wants {
    bool support_file = false, quality = false, placement_file = false, softquality = false, indel = false, polish = false, recruit = false, alnquality = false;
    double recruit_margin = 0.0;
    bool recruit_margin_bad = false;                                            // FIGFILL_RECRUIT_MARGIN is set and is no finite number >= 0
    int min_pq = -1;                                                            // -1 = not set
    int polish_rounds = 0;                                                      // 0 = the library's default
    bool placement() const { return placement_file || min_pq >= 0; }            // the call is needed for the file and for the filter
    bool support() const { return support_file || quality || placement() || softquality || indel || polish || recruit || alnquality; }
};

static Wants wants_from_env() {
    auto is1 = [](const char *name) { const char *s = getenv(name); return s && atoi(s) == 1; };
    Wants w;
    w.support_file = is1("FIGFILL_SUPPORT"); w.quality = is1("FIGFILL_QUALITY"); w.placement_file = is1("FIGFILL_PLACEMENT"); w.softquality = is1("FIGFILL_SOFTQUALITY");
    w.indel = is1("FIGFILL_INDEL"); w.polish = is1("FIGFILL_POLISH"); w.recruit = is1("FIGFILL_RECRUIT");
    w.alnquality = is1("FIGFILL_ALNQUALITY");
    if (const char *m = getenv("FIGFILL_RECRUIT_MARGIN")) {
        if (w.recruit) {
            char *e = nullptr;
            const double v = strtod(m, &e);
            if (e == m || *e != 0 || !(v >= 0) || v > 1.7976931348623157e308) w.recruit_margin_bad = true; else w.recruit_margin = v;
        }
    }
    if (const char *k = getenv("FIGFILL_POLISH_ROUNDS")) w.polish_rounds = w.polish ? atoi(k) : 0;
    const char *s = getenv("FIGFILL_QUALITY_MINPQ");
    w.min_pq = s && *s && w.quality ? atoi(s) : -1;
    return w;
}

// the placement confidence of the fill `fr` just returned (the batch still resident): R.place_pq / R.place_state
static int placement_resident(fig_ctx *ctx, const fig_gap_results *fr, Results &R, int64_t ng, int64_t nu) {
    const size_t m = (size_t)std::max<int64_t>(nu, 1);
    R.place_pq.assign(m, FIG_PLACE_NONE); R.place_state.assign((size_t)std::max<int64_t>(ng, 1), 0);
    std::vector<double> d(m * 3, 0.0);
    std::vector<int32_t> i(m * 2, 0);
    fig_read_placement rp;
    rp.ll_drawn = d.data(); rp.ll_other = d.data() + m; rp.sum_other = d.data() + 2 * m; rp.off_other = i.data(); rp.n_valid = i.data() + m;
    rp.pq = R.place_pq.data(); rp.state = R.place_state.data();
    return fig_batch_placement(ctx, fr, R.sup_origin.data(), &rp);
}

// the per-base quality of the fill `fr` just returned (the batch still resident): R.qual_phred / R.qual_state.  With
// min_pq >= 0 the call sees a copy of the draw plane in which the scored reads below the bound are not drawn.
static int quality_resident(fig_ctx *ctx, const fig_gap_results *fr, Results &R, int64_t ng, int64_t nu, int min_pq) {
    R.qual_phred.assign((size_t)std::max<int64_t>(fr->str_capacity, 1), 0); R.qual_state.assign((size_t)std::max<int64_t>(ng, 1), 0);
    std::vector<double> ll((size_t)std::max<int64_t>(fr->str_off[ng], 1) * 4, 0.0);
    fig_gap_quality gq; gq.loglik = ll.data(); gq.phred = R.qual_phred.data(); gq.state = R.qual_state.data();
    if (min_pq < 0) return fig_batch_quality(ctx, fr, R.sup_origin.data(), &gq);
    std::vector<int32_t> kept(R.draw_pos);
    for (int64_t r = 0; r < nu; r++) if (R.place_pq[(size_t)r] != FIG_PLACE_NONE && R.place_pq[(size_t)r] < min_pq) kept[(size_t)r] = INT32_MIN;
    fig_gap_results f2 = *fr; f2.draw_pos = kept.data();
    return fig_batch_quality(ctx, &f2, R.sup_origin.data(), &gq);
}

// the quality summed over placements of the fill `fr` just returned (the batch still resident): R.softq_phred / R.softq_state
static int softquality_resident(fig_ctx *ctx, const fig_gap_results *fr, Results &R, int64_t ng) {
    R.softq_phred.assign((size_t)std::max<int64_t>(fr->str_capacity, 1), 0); R.softq_state.assign((size_t)std::max<int64_t>(ng, 1), 0);
    std::vector<double> pl((size_t)std::max<int64_t>(fr->str_off[ng], 1) * 8, 0.0);
    fig_gap_softqual sq; sq.wcount = pl.data(); sq.eloglik = pl.data() + pl.size() / 2; sq.phred = R.softq_phred.data(); sq.state = R.softq_state.data();
    return fig_batch_softqual(ctx, fr, R.sup_origin.data(), nullptr, &sq);
}

// the indel evidence of the fill `fr` just returned (the batch still resident): R.indel_call / R.indel_call_end / R.indel_state
static int indel_resident(fig_ctx *ctx, const fig_gap_results *fr, Results &R, int64_t ng, int64_t nu) {
    const size_t m = (size_t)std::max<int64_t>(nu, 1), t = (size_t)std::max<int64_t>(fr->str_off[ng], 1), gm = (size_t)std::max<int64_t>(ng, 1);
    R.indel_call.assign(t, '.'); R.indel_call_end.assign(gm, '.'); R.indel_state.assign(gm, 0);
    std::vector<double> d(m * 2, 0.0);
    std::vector<int32_t> i(m * 4 + t * 3 + gm, 0);
    fig_gap_indel gi;
    gi.ll_flat = d.data(); gi.ll_gapped = d.data() + m; gi.n_ins = i.data(); gi.n_del = i.data() + m; gi.d_end = i.data() + 2 * m; gi.d_start = i.data() + 3 * m;
    gi.del_reads = i.data() + 4 * m; gi.ins_reads = gi.del_reads + t; gi.cover = gi.ins_reads + t; gi.ins_end = gi.cover + t;
    gi.call = &R.indel_call[0]; gi.call_end = &R.indel_call_end[0]; gi.state = R.indel_state.data();
    return fig_batch_indel(ctx, fr, R.sup_origin.data(), &gi);
}

// the polish of the fill `fr` just returned (the batch still resident): R.polish_str and the four per-gap arrays
static int polish_resident(fig_ctx *ctx, const fig_gap_results *fr, Results &R, int64_t ng, int64_t nu, int rounds) {
    const size_t m = (size_t)std::max<int64_t>(nu, 1), t = (size_t)std::max<int64_t>(fr->str_off[ng], 1), gm = (size_t)std::max<int64_t>(ng, 1);
    R.polish_str.assign(gm, std::string()); R.polish_len.assign(gm, 0); R.polish_nins.assign(gm, 0); R.polish_ndel.assign(gm, 0); R.polish_state.assign(gm, 0);
    R.polish_pos.assign(m, INT32_MIN);
    std::vector<int32_t> i(t + 2 * gm, 0);
    std::vector<double> d(2 * gm, 0.0);
    fig_gap_polish gp;
    gp.edit = i.data(); gp.draw_pos = R.polish_pos.data(); gp.edit_end = i.data() + t; gp.rounds = gp.edit_end + gm;
    gp.polished_len = R.polish_len.data(); gp.n_ins = R.polish_nins.data(); gp.n_del = R.polish_ndel.data();
    gp.ll_before = d.data(); gp.ll_after = d.data() + gm; gp.state = R.polish_state.data();
    const int rc = fig_batch_polish(ctx, fr, R.sup_origin.data(), rounds, &gp);
    for (int64_t g = 0; !rc && g < ng; g++) {
        if (R.polish_len[(size_t)g] <= 0) continue;
        R.polish_str[(size_t)g].assign((size_t)R.polish_len[(size_t)g], 'N');
        if (fig_polish_apply(fr, &gp, g, &R.polish_str[(size_t)g][0]) != R.polish_len[(size_t)g]) return FIG_EINVAL;
    }
    return rc;
}

// the recruiting of the undrawn reads of the fill `fr` just returned (the batch still resident): R.recruit_*; R.recruit_pos /
// R.recruit_isz are whole draw planes, the partial reads' part the fill's own
static int recruit_resident(fig_ctx *ctx, const fig_gap_results *fr, Results &R, int64_t ng, int64_t nu, double margin) {
    const size_t m = (size_t)std::max<int64_t>(nu, 1), gm = (size_t)std::max<int64_t>(ng, 1);
    R.recruit_read.assign(m, FIG_RECRUIT_READ_OFF); R.recruit_off.assign(m, INT32_MIN); R.recruit_ncand.assign(gm, 0); R.recruit_nrec.assign(gm, 0);
    R.recruit_pos = R.draw_pos; R.recruit_isz = R.draw_isz;
    std::vector<double> d(m * 5, 0.0);
    std::vector<int32_t> i(m * 3, 0);
    std::vector<uint8_t> st(gm, 0);
    fig_read_recruit rc;
    rc.ll_seed = d.data(); rc.ll_second = d.data() + m; rc.ll_flat = d.data() + 2 * m; rc.ll_gapped = d.data() + 3 * m; rc.score = d.data() + 4 * m;
    rc.off_seed = R.recruit_off.data(); rc.off_second = i.data(); rc.n_valid = i.data() + m; rc.d_end = i.data() + 2 * m;
    rc.read_state = R.recruit_read.data(); rc.draw_pos = R.recruit_pos.data(); rc.draw_isz = R.recruit_isz.data();
    rc.n_candidates = R.recruit_ncand.data(); rc.n_recruited = R.recruit_nrec.data(); rc.state = st.data();
    return fig_batch_recruit(ctx, fr, R.sup_origin.data(), margin, &rc);
}

// the quality over gapped alignments of `fr` (the batch still resident): R.alnq_*.  `fr` is the end of the chain: the fill's own
// result, or that with the merged draw plane after a recruit.  After a polish the call sees a fig_gap_results made by hand of the
// polished strings and the polish's shifted offsets, as Polish.result() of the Python binding makes it.
static int alnqual_resident(fig_ctx *ctx, const fig_gap_results *fr, Results &R, int64_t ng, int64_t nu, int64_t nr, bool polished) {
    const size_t m = (size_t)std::max<int64_t>(nu, 1), gm = (size_t)std::max<int64_t>(ng, 1);
    fig_gap_results f2 = *fr;
    std::vector<int32_t> dpos, dlen;
    std::string str;
    R.alnq_len.assign(fr->filled_len, fr->filled_len + ng); R.alnq_len.resize(gm, 0);
    R.alnq_off.assign(fr->str_off, fr->str_off + ng + 1);
    if (polished) {
        dpos.assign(fr->draw_pos, fr->draw_pos + std::max<int64_t>(nr, 1)); dlen.assign(fr->draw_len, fr->draw_len + std::max<int64_t>(2 * ng, 1));
        for (int64_t r = 0; r < nu; r++) dpos[(size_t)r] = R.polish_pos[(size_t)r];
        for (int64_t g = 0; g < ng; g++) {
            R.alnq_off[(size_t)g] = (int64_t)str.size();
            if (R.polish_state[(size_t)g] & FIG_POLISH_ON) {
                str += R.polish_str[(size_t)g];
                R.alnq_len[(size_t)g] = R.polish_len[(size_t)g]; dlen[(size_t)(2 * g)] = R.polish_len[(size_t)g];
            } else if (fr->filled_len[g] > 0) str.append(fr->str + fr->str_off[g], (size_t)fr->filled_len[g]);      // a gap that is off keeps its own bytes
        }
        R.alnq_off[(size_t)ng] = (int64_t)str.size();
        if (str.empty()) str.assign(1, 'N');
        f2.filled_len = R.alnq_len.data(); f2.str_off = R.alnq_off.data(); f2.str = &str[0]; f2.str_capacity = (int64_t)str.size();
        f2.draw_pos = dpos.data(); f2.draw_len = dlen.data();
    }
    const size_t t = (size_t)std::max<int64_t>(R.alnq_off[(size_t)ng], 1);
    R.alnq_phred.assign(t, 0); R.alnq_state.assign(gm, 0);
    std::vector<double> d(t * 4 + m, 0.0);
    std::vector<int32_t> i(t * 3 + m * 4, 0);
    fig_gap_alnqual aq;
    aq.loglik = d.data(); aq.ll_gapped = d.data() + t * 4;
    aq.depth = i.data(); aq.agree = i.data() + t; aq.skip = i.data() + 2 * t;
    aq.n_ins = i.data() + 3 * t; aq.n_del = aq.n_ins + m; aq.d_end = aq.n_del + m; aq.d_start = aq.d_end + m;
    aq.phred = R.alnq_phred.data(); aq.state = R.alnq_state.data();
    return fig_batch_alnqual(ctx, &f2, R.sup_origin.data(), &aq);
}

// The fill of the batch `fb` (nu unmapped + np partial reads) resident in ctx, as both the single-device path and a shard run it:
// R is sized, `fr` -- zeroed by the caller, who may have set its dbg_* fields -- becomes the view of R the library fills, then
// the fill (with R.sup_counts / R.sup_origin when `w` needs the support call) and the passes beside it that `w` asks for.
// Returns 0, or the failing call's code with its name in `what`.
static const char *const FILL_CALL = "fig_fill_resident";
static int fill_batch(fig_ctx *ctx, const fig_model *fm, const fig_gap_batch *fb, int64_t nu, int64_t np, const Wants &w, Results &R, fig_gap_results &fr,
                      fig_stats *st, const char *&what) {
    const int64_t ng = fb->n_gaps, nr = nu + np, cap = fig_results_capacity(fm, fb);
    R.filled_len.assign(ng, 0); R.gaptofill.assign(ng, 0); R.str_off.assign(ng + 1, 0); R.str.assign((size_t)std::max<int64_t>(cap, 1), 'N');
    R.draw_pos.assign((size_t)std::max<int64_t>(nr, 1), INT32_MIN); R.draw_isz.assign((size_t)std::max<int64_t>(nr, 1), 0); R.draw_len.assign((size_t)std::max<int64_t>(ng * 2, 1), -1);
    fr.filled_len = R.filled_len.data(); fr.gaptofill = R.gaptofill.data(); fr.str_off = R.str_off.data();
    fr.str = &R.str[0]; fr.str_capacity = (int64_t)R.str.size();
    fr.draw_pos = R.draw_pos.data(); fr.draw_isz = R.draw_isz.data(); fr.draw_len = R.draw_len.data();
    what = FILL_CALL;
    int rc;
    if (!w.support()) rc = fig_fill_resident(ctx, &fr);
    else if (!fig_fill_resident_ex) { fprintf(stderr, "figfill: FIGFILL_SUPPORT=1 needs fig_fill_resident_ex, which the library behind this build does not export\n"); rc = FIG_EUNSUP; }
    else {
        R.sup_counts.assign((size_t)std::max<int64_t>(fr.str_capacity, 1) * 5, 0); R.sup_origin.assign((size_t)std::max<int64_t>(ng, 1), 0);
        fig_gap_support fs; fs.counts = R.sup_counts.data(); fs.origin = R.sup_origin.data();
        rc = fig_fill_resident_ex(ctx, &fr, &fs);
    }
    fig_get_stats(ctx, st);
    if (!rc && w.placement()) { what = "fig_batch_placement"; rc = placement_resident(ctx, &fr, R, ng, nu); }
    if (!rc && w.quality) { what = "fig_batch_quality"; rc = quality_resident(ctx, &fr, R, ng, nu, w.min_pq); }
    if (!rc && w.softquality) { what = "fig_batch_softqual"; rc = softquality_resident(ctx, &fr, R, ng); }
    if (!rc && w.recruit) { what = "fig_batch_recruit"; rc = recruit_resident(ctx, &fr, R, ng, nu, w.recruit_margin); }
    fig_gap_results fpost = fr;                              // what the indel pass and the polish see: the merged plane after a recruit
    if (!rc && w.recruit) { fpost.draw_pos = R.recruit_pos.data(); fpost.draw_isz = R.recruit_isz.data(); }
    if (!rc && w.indel) { what = "fig_batch_indel"; rc = indel_resident(ctx, &fpost, R, ng, nu); }
    if (!rc && w.polish) { what = "fig_batch_polish"; rc = polish_resident(ctx, &fpost, R, ng, nu, w.polish_rounds); }
    if (!rc && w.alnquality) { what = "fig_batch_alnqual"; rc = alnqual_resident(ctx, &fpost, R, ng, nu, nr, w.polish); }
    return rc;
}

// every file of a run
static bool write_outputs(const RunArgs &a, const Scaffold &sc, const Batch &B, const Results &R, const Wants &w, std::string &err) {
    return write_gapout(a, B, R, err) && write_draw(a, B, R, err) && write_gaploads(a, B, err) && write_scaffold(a, sc, B, R, err) &&
           (!w.support_file || write_support(a, B, R, err)) && (!w.quality || write_quality(a, B, R, err)) && (!w.placement_file || write_placement(a, B, R, err)) &&
           (!w.softquality || write_softquality(a, B, R, err)) && (!w.indel || write_indel(a, B, R, err)) &&
           (!w.polish || write_polished(a, B, R, err)) && (!w.recruit || write_recruit(a, B, R, err)) &&
           (!w.alnquality || write_alnquality(a, B, R, err));
}

static int fail(const std::string &m) { fprintf(stderr, "%s\n", m.c_str()); return 1; }

// ---- N GPUs of one node from this process (FIGFILL_DEVICES=0,1,...; the reference starts its own workers too,
// FillGaps.cpp:668-679): the gaps are dealt longest-processing-time-first on estimated cost (fig_host.h; the role of
// FillGaps.cpp:456-649), one host thread per GPU creates its own fig_ctx (contexts are independent, include/figbird_hip.h)
// and fills its shard through fig_fill_gaps with no exchange on the data path; the shard results meet in host memory in
// global gap / read order, so the writers below see exactly what a single-GPU run hands them.
struct ShardRun { Wants w; std::vector<int64_t> ids; Batch sub; Results R; fig_stats st; int rc = 0; std::string err; fig_ctx *ctx = nullptr; std::vector<uint8_t> reach, preset; };

static void shard_fail(ShardRun *S, int rc, const std::string &what) {
    S->rc = rc; S->err = what + ": " + fig_strerror(rc);
    if (S->ctx) { fig_ctx_destroy(S->ctx); S->ctx = nullptr; }
}

// phase 1: context, model, upload, and which of the shard's gaps get to Figbird.cpp:6317 (fig_batch_probe_reach)
static void shard_open(int device, const fig_model *fm, const Scaffold *sc, ShardRun *S) {
    memset(&S->st, 0, sizeof(S->st));
    fig_gap_batch fb; S->sub.view(fb, *sc);
    const int64_t ng = fb.n_gaps;
    S->reach.assign((size_t)std::max<int64_t>(ng, 1), 0);
    if (ng == 0) return;
    int rc = fig_ctx_create(device, &S->ctx);
    if (rc) { S->ctx = nullptr; return shard_fail(S, rc, std::string("fig_ctx_create(") + std::to_string(device) + ")"); }
    if ((rc = fig_ctx_set_model(S->ctx, fm))) return shard_fail(S, rc, "fig_ctx_set_model");
    if ((rc = fig_batch_upload(S->ctx, &fb))) return shard_fail(S, rc, std::string("fig_batch_upload on device ") + std::to_string(device));
    if ((rc = fig_batch_probe_reach(S->ctx, S->reach.data()))) return shard_fail(S, rc, "fig_batch_probe_reach");
}

// phase 2: the carry worked out over ALL shards (S->preset, shard order), then the fill
static void shard_fill(int device, const fig_model *fm, const Scaffold *sc, ShardRun *S) {
    fig_gap_batch fb; S->sub.view(fb, *sc);
    const int64_t ng = fb.n_gaps;
    if (ng == 0 || !S->ctx) return;
    int rc = fig_batch_set_ot_preset(S->ctx, S->preset.data());
    if (rc) return shard_fail(S, rc, "fig_batch_set_ot_preset");
    fig_gap_results fr; memset(&fr, 0, sizeof(fr));
    const char *what;
    rc = fill_batch(S->ctx, fm, &fb, (int64_t)S->sub.u_anchor_pos.size(), (int64_t)S->sub.p_pos.size(), S->w, S->R, fr, &S->st, what);
    if (rc) return shard_fail(S, rc, std::string(what) + " on device " + std::to_string(device));
    fig_ctx_destroy(S->ctx); S->ctx = nullptr;
}

// Fill B over `devices`; on success R holds the whole gap set in global order.  Returns 0 or 1 (message in err).
static int fill_multi(const std::vector<int> &devices, const RunArgs &a, const Scaffold &sc, Batch &B, const fig_model &fm, const Wants &w, Results &R,
                      fig_stats &st, std::string &err) {
    const int world = (int)devices.size();
    const int64_t ng = (int64_t)B.gap_contig.size();
    std::vector<std::vector<int64_t>> shards = partition_lpt(estimate_cost(B, a, fm.max_read_length), world);
    std::vector<ShardRun> runs((size_t)world);
    for (int r = 0; r < world; r++) { runs[r].w = w; runs[r].ids = shards[r]; make_shard(B, shards[r], runs[r].sub); }
    const bool serial = getenv("FIGFILL_SERIAL") != nullptr;   // test knob: one shard after the other (the CPU emulation library keeps global state)
    auto phase = [&](void (*fn)(int, const fig_model *, const Scaffold *, ShardRun *)) {
        if (serial) { for (int r = 0; r < world; r++) fn(devices[r], &fm, &sc, &runs[r]); return; }
        std::vector<std::thread> th;
        for (int r = 0; r < world; r++) th.emplace_back(fn, devices[r], &fm, &sc, &runs[r]);
        for (auto &t : th) t.join();
    };
    auto failed = [&]() { for (int r = 0; r < world; r++) if (runs[r].rc) { err = "figfill: " + runs[r].err; for (auto &q : runs) if (q.ctx) { fig_ctx_destroy(q.ctx); q.ctx = nullptr; } return true; } return false; };
    phase(shard_open);
    if (failed()) return 1;
    {   // the one exchange before the fill: every shard's reach bits, carried along the reference's worker processes
        std::vector<uint8_t> reach((size_t)std::max<int64_t>(ng, 1), 0);
        for (int r = 0; r < world; r++) for (size_t k = 0; k < runs[r].ids.size(); k++) reach[(size_t)runs[r].ids[k]] = runs[r].reach[k];
        ot_presets_from_reach(B, reach.data());
        for (int r = 0; r < world; r++) { runs[r].preset.assign(std::max<size_t>(runs[r].ids.size(), 1), 0); for (size_t k = 0; k < runs[r].ids.size(); k++) runs[r].preset[k] = B.gap_ot_preset[(size_t)runs[r].ids[k]]; }
    }
    phase(shard_fill);
    if (failed()) return 1;
    // ---- merge in global gap order (strings compacted as fig_fill_gaps leaves them) and global read order
    const int64_t NU = (int64_t)B.u_anchor_pos.size(), NP = (int64_t)B.p_pos.size();
    R.filled_len.assign(ng, 0); R.gaptofill.assign(ng, 0); R.str_off.assign(ng + 1, 0);
    R.draw_pos.assign((size_t)std::max<int64_t>(NU + NP, 1), INT32_MIN); R.draw_isz.assign((size_t)std::max<int64_t>(NU + NP, 1), 0); R.draw_len.assign((size_t)std::max<int64_t>(ng * 2, 1), -1);
    std::vector<int> owner((size_t)ng, -1); std::vector<int64_t> local((size_t)ng, 0);
    for (int r = 0; r < world; r++) for (size_t k = 0; k < runs[r].ids.size(); k++) { owner[runs[r].ids[k]] = r; local[runs[r].ids[k]] = (int64_t)k; }
    memset(&st, 0, sizeof(st));
    for (int r = 0; r < world; r++) {
        st.kernel_ms = std::max(st.kernel_ms, runs[r].st.kernel_ms); st.place_calls += runs[r].st.place_calls; st.alg_flops += runs[r].st.alg_flops;
        st.n_launches += runs[r].st.n_launches;
    }
    R.str.clear();
    const bool support = w.support(), quality = w.quality, placement = w.placement();
    if (support) R.sup_origin.assign((size_t)std::max<int64_t>(ng, 1), 0);
    if (placement) { R.place_pq.assign((size_t)std::max<int64_t>(NU, 1), FIG_PLACE_NONE); R.place_state.assign((size_t)std::max<int64_t>(ng, 1), 0); }
    if (quality) R.qual_state.assign((size_t)std::max<int64_t>(ng, 1), 0);
    if (w.softquality) R.softq_state.assign((size_t)std::max<int64_t>(ng, 1), 0);
    if (w.indel) { R.indel_call_end.assign((size_t)std::max<int64_t>(ng, 1), '.'); R.indel_state.assign((size_t)std::max<int64_t>(ng, 1), 0); }
    if (w.polish) {
        const size_t gm = (size_t)std::max<int64_t>(ng, 1);
        R.polish_str.assign(gm, std::string()); R.polish_len.assign(gm, 0); R.polish_nins.assign(gm, 0); R.polish_ndel.assign(gm, 0); R.polish_state.assign(gm, 0);
    }
    if (w.recruit) {
        R.recruit_read.assign((size_t)std::max<int64_t>(NU, 1), FIG_RECRUIT_READ_OFF); R.recruit_off.assign((size_t)std::max<int64_t>(NU, 1), INT32_MIN);
        R.recruit_ncand.assign((size_t)std::max<int64_t>(ng, 1), 0); R.recruit_nrec.assign((size_t)std::max<int64_t>(ng, 1), 0);
    }
    if (w.alnquality) { R.alnq_len.assign((size_t)std::max<int64_t>(ng, 1), 0); R.alnq_off.assign((size_t)ng + 1, 0); R.alnq_state.assign((size_t)std::max<int64_t>(ng, 1), 0); }
    for (int64_t g = 0; g < ng; g++) {
        const ShardRun &S = runs[owner[g]]; const int64_t k = local[g];
        R.filled_len[g] = S.R.filled_len[k]; R.gaptofill[g] = S.R.gaptofill[k];
        R.str_off[g] = (int64_t)R.str.size();
        R.str.append(S.R.str, (size_t)S.R.str_off[k], (size_t)(S.R.str_off[k + 1] - S.R.str_off[k]));
        if (support) {                                    // the plane travels with the string: five counts per byte
            R.sup_counts.insert(R.sup_counts.end(), S.R.sup_counts.begin() + S.R.str_off[k] * 5, S.R.sup_counts.begin() + S.R.str_off[k + 1] * 5);
            R.sup_origin[g] = S.R.sup_origin[k];
        }
        if (quality) {                                    // and so does the Phred: one byte per string byte
            R.qual_phred.insert(R.qual_phred.end(), S.R.qual_phred.begin() + S.R.str_off[k], S.R.qual_phred.begin() + S.R.str_off[k + 1]);
            R.qual_state[g] = S.R.qual_state[k];
        }
        if (w.softquality) {
            R.softq_phred.insert(R.softq_phred.end(), S.R.softq_phred.begin() + S.R.str_off[k], S.R.softq_phred.begin() + S.R.str_off[k + 1]);
            R.softq_state[g] = S.R.softq_state[k];
        }
        if (w.indel) {
            R.indel_call.append(S.R.indel_call, (size_t)S.R.str_off[k], (size_t)(S.R.str_off[k + 1] - S.R.str_off[k]));
            R.indel_call_end[g] = S.R.indel_call_end[k]; R.indel_state[g] = S.R.indel_state[k];
        }
        if (w.polish) {                                   // the polished strings are per gap already
            R.polish_str[g] = S.R.polish_str[k]; R.polish_len[g] = S.R.polish_len[k]; R.polish_nins[g] = S.R.polish_nins[k]; R.polish_ndel[g] = S.R.polish_ndel[k];
            R.polish_state[g] = S.R.polish_state[k];
        }
        if (w.alnquality) {                               // the Phred travels with the string that was scored: its own offsets
            R.alnq_off[g] = (int64_t)R.alnq_phred.size();
            R.alnq_phred.insert(R.alnq_phred.end(), S.R.alnq_phred.begin() + S.R.alnq_off[k], S.R.alnq_phred.begin() + S.R.alnq_off[k + 1]);
            R.alnq_len[g] = S.R.alnq_len[k]; R.alnq_state[g] = S.R.alnq_state[k];
        }
        R.draw_len[2 * g] = S.R.draw_len[2 * k]; R.draw_len[2 * g + 1] = S.R.draw_len[2 * k + 1];
        const int64_t nu = B.u_read_off[g + 1] - B.u_read_off[g], np = B.p_read_off[g + 1] - B.p_read_off[g];
        const int64_t snu = (int64_t)S.sub.u_anchor_pos.size();
        for (int64_t i = 0; i < nu; i++) { R.draw_pos[B.u_read_off[g] + i] = S.R.draw_pos[S.sub.u_read_off[k] + i]; R.draw_isz[B.u_read_off[g] + i] = S.R.draw_isz[S.sub.u_read_off[k] + i]; }
        if (placement) {                                  // one pq per unmapped read, in the order of the draw plane
            for (int64_t i = 0; i < nu; i++) R.place_pq[B.u_read_off[g] + i] = S.R.place_pq[S.sub.u_read_off[k] + i];
            R.place_state[g] = S.R.place_state[k];
        }
        if (w.recruit) {                                  // state and seed per unmapped read, in the order of the draw plane; the counts per gap
            for (int64_t i = 0; i < nu; i++) { R.recruit_read[B.u_read_off[g] + i] = S.R.recruit_read[S.sub.u_read_off[k] + i]; R.recruit_off[B.u_read_off[g] + i] = S.R.recruit_off[S.sub.u_read_off[k] + i]; }
            R.recruit_ncand[g] = S.R.recruit_ncand[k]; R.recruit_nrec[g] = S.R.recruit_nrec[k];
        }
        for (int64_t i = 0; i < np; i++) { R.draw_pos[NU +B.p_read_off[g] + i] = S.R.draw_pos[snu + S.sub.p_read_off[k] + i]; R.draw_isz[NU + B.p_read_off[g] + i] = S.R.draw_isz[snu + S.sub.p_read_off[k] + i]; }
    }
    R.str_off[ng] = (int64_t)R.str.size();
    if (w.alnquality) { R.alnq_off[(size_t)ng] = (int64_t)R.alnq_phred.size(); if (R.alnq_phred.empty()) R.alnq_phred.assign(1, 0); }
    if (R.str.empty()) R.str.assign(1, 'N');
    if (support && R.sup_counts.empty()) R.sup_counts.assign(5, 0);
    if (quality && R.qual_phred.empty()) R.qual_phred.assign(1, 0);
    if (w.softquality && R.softq_phred.empty()) R.softq_phred.assign(1, 0);
    return 0;
}

int main(int argc, char **argv) {
    if (argc < 16) {
        fprintf(stderr, "usage: figfill <contigs.fa> <maxDistance> <readLen> <scriptItr> <partialFlag> <unmapped> <numThreads> "
                        "<myout.sam> <tmp/> <gaps/> <negOverlap> <partialReadLen> <trim> <setInputMean> <insertSize>\n");
        return 1;
    }
    RunArgs a;
    a.contigFile = argv[1]; a.D = atoi(argv[2]); a.read_length = atoi(argv[3]); a.script_itr = atoi(argv[4]);
    a.partial_flag = atoi(argv[5]); a.unmapped = atoi(argv[6]); a.num_threads = atoi(argv[7]); a.mapFile = argv[8];
    a.tmp = argv[9]; a.gapsDir = argv[10]; a.neg_overlap = atoi(argv[11]); a.partial_len = atoi(argv[12]);
    a.trim = atoi(argv[13]); a.setinputmean = atoi(argv[14]); a.isz = atoi(argv[15]);
    a.unm_limit = 400;                                   // gapthresh, FillGaps.cpp:22
    const char *dev_env = getenv("FIGFILL_DEVICE");
    int device = dev_env ? atoi(dev_env) : 0;
    std::vector<int> devices;                            // FIGFILL_DEVICES=0,1,...,7: one shard, host thread and fig_ctx per listed GPU
    if (const char *dl = getenv("FIGFILL_DEVICES")) {
        const char *q = dl;
        while (true) {
            char *e; long v = strtol(q, &e, 10);
            if (e == q || v < 0) { devices.clear(); break; }
            devices.push_back((int)v);
            if (*e == 0) break;
            if (*e != ',') { devices.clear(); break; }           // trailing garbage ("0,1x") is an error, not a shorter list
            q = e + 1;
        }
        if (devices.empty()) return fail("figfill: FIGFILL_DEVICES must be a comma-separated list of GPU ordinals");
    }
    const Wants w = wants_from_env();
    if (w.placement() && !fig_batch_placement)
        return fail("figfill: FIGFILL_PLACEMENT=1 and FIGFILL_QUALITY_MINPQ need fig_batch_placement, which the library behind this build does not export");
    if (w.softquality && !fig_batch_softqual) return fail("figfill: FIGFILL_SOFTQUALITY=1 needs fig_batch_softqual, which the library behind this build does not export");
    if (w.indel && !fig_batch_indel) return fail("figfill: FIGFILL_INDEL=1 needs fig_batch_indel, which the library behind this build does not export");
    if (w.polish && !fig_batch_polish) return fail("figfill: FIGFILL_POLISH=1 needs fig_batch_polish, which the library behind this build does not export");
    if (w.recruit && !fig_batch_recruit) return fail("figfill: FIGFILL_RECRUIT=1 needs fig_batch_recruit, which the library behind this build does not export");
    if (w.alnquality && !fig_batch_alnqual) return fail("figfill: FIGFILL_ALNQUALITY=1 needs fig_batch_alnqual, which the library behind this build does not export");
    if (w.recruit_margin_bad) return fail("figfill: FIGFILL_RECRUIT_MARGIN must be a finite number >= 0");
    if (w.quality && !fig_batch_quality) return fail("figfill: FIGFILL_QUALITY=1 needs fig_batch_quality, which the library behind this build does not export");
    setenv("GPU_MAX_HW_QUEUES", "8", 0);                 // one hardware queue per scheduler lane; before any thread or HIP call (fig_abi.hip: fig_ctx_create)
    auto t0 = std::chrono::steady_clock::now();

    std::string err;
    Scaffold sc;
    if (!load_scaffold(a.contigFile, sc, err)) return fail(err);
    Batch B;
    // FIGFILL_SAM="<maxD1>:<frag.sam>[;<maxD2>:<jump.sam>]": ingest the aligner's SAM in this process (the binning of
    // Preprocess.cpp, fig_sam.h) and hand the per-gap reads to the fill in memory -- no gaps_<g>.sam / partial_gaps_<g>.sam
    // files.  The run-level files (gapInfo/stat/stat2.txt, myout.sam) are still written: the model is built from them.
    if (const char *spec = getenv("FIGFILL_SAM")) {
        std::string sp(spec);
        std::vector<std::pair<int, std::string>> libs;
        size_t p = 0;
        while (p < sp.size()) { size_t e = sp.find(';', p); if (e == std::string::npos) e = sp.size(); std::string it = sp.substr(p, e - p); size_t c = it.find(':');
                                if (c != std::string::npos) libs.emplace_back(atoi(it.substr(0, c).c_str()), it.substr(c + 1)); p = e + 1; }
        if (libs.empty() || (a.unmapped == 1 && libs.size() < 2)) return fail("figfill: FIGFILL_SAM needs <maxD>:<frag.sam> and, in unmapped mode, ;<maxD>:<jump.sam>");
        figsam::Binned frag, jump;
        for (size_t k = 0; k < libs.size() && k < 2; k++) {
            figsam::Args pa;
            pa.contigFile = a.contigFile; pa.maxDistance = libs[k].first; pa.samflag = (int)k + 1; pa.mapFile = libs[k].second; pa.outFile = a.mapFile;
            pa.filledContigFile = a.contigFile; pa.reads1 = "r_1.fastq"; pa.reads2 = "r_2.fastq"; pa.gapsDir = a.gapsDir; pa.tmpDir = a.tmp; pa.default_setting = 1;
            if (k == 1 && a.unmapped != 1) break;
            if (figsam::preprocess(pa, k == 0 ? frag : jump, err, 2)) return fail(err);
        }
        if (!load_batch_mem(a, sc, a.unmapped == 1 ? &jump.gap_files : nullptr, &frag.partial_files, B, err)) return fail(err);
    } else if (!load_batch(a, sc, B, err)) return fail(err);
    printf("Total # of gaps = %zu\n", B.gap_contig.size());
    for (const std::string &m : B.messages) printf("%s\n", m.c_str());
    Model M;
    if (!build_model(a, sc, M, err)) return fail(err);

    fig_model fm; M.fill(fm, a);
    fig_gap_batch fb; B.view(fb, sc);
    if (devices.size() > 1) {
        Results R; fig_stats st;
        if (fill_multi(devices, a, sc, B, fm, w, R, st, err)) return fail(err);
        if (!write_outputs(a, sc, B, R, w, err)) return fail(err);
        double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        printf("Time taken = %g seconds (%zu GPUs; slowest shard's device kernels %.3f ms, %lld placeReads calls)\n", secs, devices.size(), st.kernel_ms, (long long)st.place_calls);
        printf("======================================\n");
        printf("Iteration %d ends successfully\n", a.script_itr);
        printf("======================================\n");
        return 0;
    }
    if (devices.size() == 1) device = devices[0];
    fig_ctx *ctx = nullptr;
    int rc = fig_ctx_create(device, &ctx);
    if (rc) return fail(std::string("figfill: fig_ctx_create: ") + fig_strerror(rc));
    rc = fig_ctx_set_model(ctx, &fm);
    if (rc) { fig_ctx_destroy(ctx); return fail(std::string("figfill: fig_ctx_set_model: ") + fig_strerror(rc)); }

    Results R;
    const int64_t ng = fb.n_gaps;
    fig_gap_results fr; memset(&fr, 0, sizeof(fr));
    // optional candidate trace for the parity tests (FIGFILL_TRACE=<file>)
    const char *trace = getenv("FIGFILL_TRACE");
    std::vector<int32_t> dn, di; std::vector<double> dl;
    const int maxc = 2048;
    if (trace) {
        dn.assign((size_t)std::max<int64_t>(ng, 1), 0); di.assign((size_t)std::max<int64_t>(ng, 1) * maxc * 3, 0); dl.assign((size_t)std::max<int64_t>(ng, 1) * maxc, 0);
        fr.dbg_max_cand = maxc; fr.dbg_n_cand = dn.data(); fr.dbg_cand_i = di.data(); fr.dbg_cand_lik = dl.data();
    }
    // upload; measure which gaps get to Figbird.cpp:6317; carry that along the reference's $num_threads worker processes
    // (overlap_threshold, :103); fill
    rc = fig_batch_upload(ctx, &fb);
    if (!rc && ng > 0) {
        std::vector<uint8_t> reach((size_t)ng, 0);
        rc = fig_batch_probe_reach(ctx, reach.data());
        if (!rc) { ot_presets_from_reach(B, reach.data()); rc = fig_batch_set_ot_preset(ctx, B.gap_ot_preset.data()); }
    }
    fig_stats st; memset(&st, 0, sizeof(st));
    const char *what = FILL_CALL;
    if (!rc) rc = fill_batch(ctx, &fm, &fb, (int64_t)B.u_anchor_pos.size(), (int64_t)B.p_pos.size(), w, R, fr, &st, what);
    fig_ctx_destroy(ctx);
    if (rc) return fail(std::string("figfill: ") + (what == FILL_CALL ? "fill" : what) + ": " + fig_strerror(rc));

    if (!write_outputs(a, sc, B, R, w, err)) return fail(err);
    if (trace) {
        FILE *f = fopen(trace, "w");
        if (f) {
            fprintf(f, "MODEL\t%d\t%d\t%d\t%a\t%a\t%a\n", M.cutoff, M.Tmin, M.Tmax, M.insertSizeMean, M.leftSD, M.rightSD);
            for (int64_t g = 0; g < ng; g++)
                for (int k = 0; k < dn[g] && k < maxc; k++)
                    fprintf(f, "CAND\t%d\t%d\t%d\t%a\t%d\n", (int)g, di[(g * maxc + k) * 3], di[(g * maxc + k) * 3 + 1], dl[g * maxc + k], di[(g * maxc + k) * 3 + 2]);
            fprintf(f, "STATS\t%lld\t%.17g\n", (long long)st.place_calls, st.alg_flops);
            fprintf(f, "LAUNCHES\t%d\n", (int)st.n_launches);      // kernel launches of the fill (the emulation reports its launch classes)
            fclose(f);
        }
    }
    double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    printf("Time taken = %g seconds (device kernels %.3f ms, %lld placeReads calls)\n", secs, st.kernel_ms, (long long)st.place_calls);
    printf("======================================\n");
    printf("Iteration %d ends successfully\n", a.script_itr);
    printf("======================================\n");
    return 0;
}
