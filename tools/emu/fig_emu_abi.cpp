// fig_emu_abi.cpp -- TEST INFRASTRUCTURE ONLY (CPU unit tests, `-m "not gpu"`).
//
// Implements the C ABI of include/figbird_hip.h by compiling the device engine
// (figbird_amd/csrc/fig_engine.h) for the host with FIG_EMU: ONE emulated lane per
// workgroup, barriers are no-ops.  It lets the CPU test-suite check the engine's control
// logic, packing and host plumbing against the oracle without a GPU.  It is never linked
// into libfighip.so or figfill; the product fails with FIG_ENODEV when no GPU is present.
#define FIG_EMU 1
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../include/figbird_hip.h"
#include "../../figbird_amd/csrc/fig_engine.h"
#include "../../figbird_amd/csrc/fig_pack.h"
#include "../../figbird_amd/csrc/fig_abi_host.h"

struct fig_ctx {
    bool have_model = false;
    fig_model hm;
    FigDevModel dm;
    std::vector<double> tabs;            // the model tables dm points into
    bool have_batch = false;
    FigPacked K;
    fig_stats stats;
};

extern "C" int fig_version(void) { return FIG_ABI_VERSION; }
extern "C" const char *fig_strerror(int code) { return fig_strerror_text(code); }
extern "C" int fig_ctx_create(int, fig_ctx **out) { *out = new fig_ctx(); memset(&(*out)->stats, 0, sizeof(fig_stats)); return FIG_OK; }
extern "C" void fig_ctx_destroy(fig_ctx *c) { delete c; }
extern "C" void fig_batch_free(fig_ctx *c) { if (c) { c->K = FigPacked(); c->have_batch = false; } }
extern "C" int fig_get_stats(const fig_ctx *c, fig_stats *o) { *o = c->stats; return FIG_OK; }
extern "C" int64_t fig_results_capacity(const fig_model *m, const fig_gap_batch *b) { return fig_pack_results_capacity(m, b); }

extern "C" int fig_ctx_set_model(fig_ctx *ctx, const fig_model *m) {
    if (!ctx) return FIG_EINVAL;
    if (int rc = fig_model_check(m)) return rc;
    fig_batch_free(ctx);                 // a resident batch was packed under the previous model
    ctx->hm = *m;
    FigModelOffsets o;
    fig_model_tables(m, ctx->tabs, o, ctx->dm);
    fig_model_point(ctx->dm, o, ctx->tabs.data());
    ctx->have_model = true;
    return FIG_OK;
}

extern "C" int fig_batch_upload(fig_ctx *ctx, const fig_gap_batch *b) {
    if (!ctx || !b || !ctx->have_model) return FIG_EINVAL;
    ctx->K = FigPacked();
    {   // the wide cap as the library takes it (no budget here: host memory), but never below THIS build's base width: FIG_EMU_CHUNK=<c>
        // makes min(c, 64) the base (emu_run), so that a small FIG_SLOTS_WIDE lets small cases run into the cap
        int base = ctx->K.nslots;
        if (const char *ce = getenv("FIG_EMU_CHUNK")) base = std::min(std::max(1, atoi(ce)), base);
        const FigKnobs kn = fig_knobs_from_env(ctx->hm.unmapped_flag);
        ctx->K.nslots_wide = kn.wide ? std::max(base, std::min(kn.slots_wide, FIG_SLOTS_WIDE_MAX)) : base;      // wide slots only where the fill would widen, as in the library
    }
    int rc = fig_pack(&ctx->hm, b, sizeof(FigState), ctx->K);
    if (rc) return rc;
    ctx->have_batch = true;
    const int64_t ng = ctx->K.n_gaps;
    if (!ctx->K.ot_given && ctx->hm.partial_flag && ng > 0) return fig_ot_carry_measured(ctx, ng);
    return FIG_OK;
}

static int emu_run(fig_ctx *ctx, fig_gap_results *out, uint8_t *probe_reach);

extern "C" int fig_fill_resident(fig_ctx *ctx, fig_gap_results *out) {
    if (!ctx || !out || !ctx->have_batch) return FIG_EINVAL;
    return emu_run(ctx, out, nullptr);
}

extern "C" int fig_batch_probe_reach(fig_ctx *ctx, uint8_t *reach) {
    if (!ctx || !reach || !ctx->have_batch) return FIG_EINVAL;
    memset(reach, 0, (size_t)ctx->K.n_gaps);
    if (!ctx->hm.partial_flag || ctx->K.n_gaps == 0) return FIG_OK;
    return emu_run(ctx, nullptr, reach);
}
extern "C" int fig_batch_set_ot_preset(fig_ctx *ctx, const uint8_t *preset) {
    if (!ctx || !preset || !ctx->have_batch) return FIG_EINVAL;
    for (int64_t g = 0; g < ctx->K.n_gaps; g++) ctx->K.ot_preset[(size_t)g] = preset[g] ? 1 : 0;
    return FIG_OK;
}

// out != nullptr: the fill; probe_reach != nullptr: the reach pre-pass (fig_probe_kernel's role)
static int emu_run(fig_ctx *ctx, fig_gap_results *out, uint8_t *probe_reach) {
    fig_gap_results none; memset(&none, 0, sizeof(none));
    if (!out) out = &none;
    FigPacked &K = ctx->K;
    int64_t ng = K.n_gaps;
    FigDevBatch B; memset(&B, 0, sizeof(B));
    B.n_gaps = ng; B.gaps = K.gaps.data(); B.order = K.order.data();
    B.u.pos = K.u_pos.data(); B.u.aux = K.u_aux.data(); B.u.len = K.u_len.data(); B.u.woff = K.u_woff.data();
    B.p.pos = K.p_pos.data(); B.p.aux = K.p_aux.data(); B.p.clip = K.p_clip.data(); B.p.refpos = K.p_ref.data();
    B.p.len = K.p_len.data(); B.p.woff = K.p_woff.data(); B.p.qoff = K.p_qoff.data();
    B.packed = K.packed.data(); B.qual = K.qual.data(); B.flank = K.flank.data();
    std::vector<int32_t> fl(ng + 1, 0), gtf(ng + 1, 0);
    std::vector<char> str((size_t)K.str_total + 8, 'N');
    B.filled_len = fl.data(); B.gaptofill = gtf.data(); B.str = str.data();
    // the optional planes are written in place: the engine's pointers are the caller's buffers
    for (const FigPlane &pl : fig_fill_planes(B, (int64_t)(K.u_pos.size() + K.p_pos.size()), K.str_total, out, nullptr, nullptr)) {
        *pl.dev = pl.host;
        if (pl.fill >= 0) memset(pl.host, pl.fill, pl.bytes);
    }
    B.n_ureads = (int64_t)K.u_pos.size();
    int32_t qh = 0; unsigned long long counters[FIG_CNT_N] = {0};
    B.queue_head = &qh; B.counters = counters;
    long long stride = fig_scratch_layout(nullptr, K.capG, K.capR, K.capP, K.capC, K.capW, K.capE, nullptr);
    std::vector<unsigned char> slab((size_t)stride + 64, 0);
    B.scratch = slab.data(); B.scratch_stride = stride;
    B.capG = K.capG; B.capR = K.capR; B.capP = K.capP; B.capC = K.capC; B.capW = K.capW; B.capE = K.capE;
    std::vector<unsigned char> persist((size_t)K.persist_total + 256, 0);
    B.persist = persist.data();
    std::vector<FigGapCtl> ctl((size_t)ng + 1, FigGapCtl{0, 0, 0, 0});
    B.gapctl = ctl.data();
    B.ot_preset = K.ot_preset.data();
    const FigDevModel &M = ctx->dm;
    const FigKnobs knobs = fig_knobs_from_env(M.unmapped);
    for (const FigLaunchClass &c : K.classes) {
        // one emulated lane = one wave of width 1, one team; the engine always runs its LDS-table code path here
        FigKernArgs A = fig_kargs_of(c, 0, 0);
        A.nteams = 1;
        A.mle_reuse = probe_reach ? 0 : knobs.mle_reuse;      // as the library's launches (launch_kind, fig_abi.hip)
        // LDS-tiled form of a class (fig_pack.h): what the packer chose, or forced on every class by FIG_EMU_TILES=<n> so that the
        // tile logic of the E-step is exercised on small gaps too
        if (const char *ft = getenv("FIG_EMU_TILES")) {
            A.tiles = atoi(ft);
            if (A.tiles > 0) { A.tile_step = ((c.ncolE + A.tiles - 1) / A.tiles + 7) & ~7; A.tile_cols = (A.tile_step + M.L + 8 + 7) & ~7; }
            fprintf(stderr, "[figemu] class ncolE=%d: LDS-tiled E-step forced, tiles=%d step=%d cols=%d\n", c.ncolE, A.tiles, A.tile_step, A.tile_cols);
        }
        FigEng E;
        fig_eng_ident(E, 0, 1, 1);
        E.M = &ctx->dm; E.B = &B; E.flops = 0; E.mle_alg = 0; E.mle_exec = 0;
        fig_scratch_layout(slab.data(), K.capG, K.capR, K.capP, K.capC, K.capW, K.capE, &E.scr);
        // the "LDS" of the workgroup: the layout is asked for its size first, then laid out again on the buffer of that size
        double sizing[1]; fig_lds = sizing;
        std::vector<double> lds((size_t)(fig_eng_carve(E, M, A, true) + 7) / 8, 0.0);
        fig_lds = lds.data();
        fig_eng_carve(E, M, A, true);
        const FigScr work = E.scr;
        auto poison = [&] { memset(slab.data(), 0xA5, slab.size()); memset(lds.data(), 0xA5, lds.size() * sizeof(double)); };
        // the work items of fig_engine_sched.h, in the order the kernels of fig_abi.hip would pop them
        const std::vector<int> ids(K.order.begin() + c.q_begin, K.order.begin() + c.q_end);
        if (probe_reach) {
            for (int gi : ids) { fig_item_probe<true>(E, work, gi); probe_reach[gi] = ctl[gi].reach ? 1 : 0; }
        } else if (knobs.seq) {
            for (int gi : ids) fig_item_fill<true>(E, work, gi);
        } else {
            // candidate-parallel schedule: the rounds fig_plan_round lays out, executed in order
            for (int gi : ids) fig_item_begin<true>(E, work, gi);
            // Knobs as in the library, with a stand-in of 8 resident workgroups for the device's capacity: small enough that
            // the admission cut-off leaves gaps waiting in batches of a few dozen gaps.  Results do not depend on it, nor on
            // the chunk -- that is the invariant under test.  FIG_EMU_CHUNK=<n>: exactly min(n, nslots, range - j)
            // candidates per admitted gap and round.  Wide chunks (FIG_WIDE): the rule of fig_wide_chunk on top, with these base
            // slots and FIG_SLOTS_WIDE as at upload; under FIG_EMU_CHUNK only when FIG_WIDE is set explicitly (the sizes stay
            // fixed otherwise).  The one workgroup here is never idle: `spare` is 0.
            int minc = knobs.minc, slots_cap = K.nslots, wide = knobs.wide;
            if (const char *ce = getenv("FIG_EMU_CHUNK")) { minc = std::max(1, atoi(ce)); slots_cap = std::min(minc, K.nslots); if (!getenv("FIG_WIDE")) wide = 0; }
            slots_cap = std::min(slots_cap, K.nslots_wide);      // (a batch uploaded under a smaller FIG_EMU_CHUNK than this fill's)
            FigRound R;
            int n_active_max = 0;
            while (true) {
                fig_plan_round(ids, ctl.data(), 8, c.nsplit, slots_cap, wide, K.nslots_wide, knobs.wide_max_active, minc, knobs.ipw, n_active_max, R);
                const FigWide fw{fig_wide_for_lane(wide, n_active_max, knobs.wide_max_active), slots_cap, K.nslots_wide};
                if (!R.n_active) break;
                if (!knobs.cont) {       // FIG_SCHED=rounds: all items of the round, then all replays
                    for (const FigItem &it : R.items) { poison(); fig_item_eval<true>(E, work, it); }      // every item starts from poisoned scratch + LDS
                    for (const FigEntry &en : R.entries) { poison(); fig_item_replay(E, work, en); }
                    continue;
                }
                // the continuous order: a gap is replayed as soon as its chunk is done, its next chunk follows at once and its
                // end item after the last -- the kernel's hand-over with one workgroup, through the same functions
                fig_round_stamp(R, ctl.data());
                size_t pos = 0;
                for (const FigEntry &en : R.entries) {
                    for (int k = 0; k < en.n; k++) { poison(); fig_item_eval<true>(E, work, R.items[pos++]); }
                    if (en.n == 0) { poison(); fig_item_replay(E, work, en); continue; }      // (the replay kernel's share)
                    FigCont nx; nx.n = en.n;
                    while (true) {
                        poison(); fig_item_continue(E, work, en.gap, nx.n, minc, fw, 0, nx);
                        if (nx.kind == FIG_CONT_END) { poison(); fig_item_end<true>(E, work, nx.gap); break; }
                        counters[FIG_CNT_CONT]++;
                        for (int k = nx.n - 1; k >= 0; k--) { poison(); fig_item_eval<true>(E, work, FigItem{nx.gap, nx.j0 + k, k, nx.n}); }
                    }
                }
            }
            for (int gi : ids) if (ctl[gi].status == FIG_GAP_LOOP_DONE) { poison(); fig_item_end<true>(E, work, gi); }
        }
        counters[FIG_CNT_FLOPS] += E.flops; counters[FIG_CNT_MLE_ALG] += E.mle_alg; counters[FIG_CNT_MLE_EXEC] += E.mle_exec;
    }
    if (probe_reach) return FIG_OK;
    counters[FIG_CNT_SPEC] = counters[FIG_CNT_FLOPS];      // this build reports no speculation overhead
    if (knobs.log && knobs.mle_reuse) fprintf(stderr, "[figsched] MLE passes reused: %llu of %llu placeReads calls executed\n", counters[FIG_CNT_MLE_REUSED], counters[FIG_CNT_MLE_ASKED]);
    fig_stats_from_counters(counters, ctx->stats);
    ctx->stats.packed_bytes = K.packed_bytes(); ctx->stats.n_launches = (int)K.classes.size();
    for (int64_t g = 0; g < ng; g++) { out->filled_len[g] = fl[g]; out->gaptofill[g] = gtf[g]; }
    return fig_compact_results(ng, str.data(), K.str_off.data(), out);
}

// Test-only view of the round planner (tests/test_abi_and_host.py): one round on a hand-made gapctl snapshot.  items /
// entries take up to cap_ints ints each; returns n_active, or -1 when they do not fit.
extern "C" int fig_emu_plan_round_wide(const int *ids, int n_ids, const int32_t *ctl, int capacity, int nsplit, int slots_cap, int wide_mode, int wide_cap, int wide_max_active, int minc, double ipw,
                                       int *n_active_max, int *items, int *n_items, int *entries, int *n_entries, int cap_ints, int *chunk);
extern "C" int fig_emu_plan_round(const int *ids, int n_ids, const int32_t *ctl, int capacity, int nsplit, int slots_cap, int minc, double ipw,
                                  int *n_active_max, int *items, int *n_items, int *entries, int *n_entries, int cap_ints, int *chunk) {
    return fig_emu_plan_round_wide(ids, n_ids, ctl, capacity, nsplit, slots_cap, 0, slots_cap, 0, minc, ipw, n_active_max, items, n_items, entries, n_entries, cap_ints, chunk);      // (its slots_cap is both caps: a hard one)
}

// The same with the wide cap and the FIG_WIDE bits of its own (tests/test_wide_chunks.py); the fourth int32 of a ctl row is FigGapCtl::last.
extern "C" int fig_emu_plan_round_wide(const int *ids, int n_ids, const int32_t *ctl, int capacity, int nsplit, int slots_cap, int wide_mode, int wide_cap, int wide_max_active, int minc, double ipw,
                                       int *n_active_max, int *items, int *n_items, int *entries, int *n_entries, int cap_ints, int *chunk) {
    FigRound R;
    fig_plan_round(std::vector<int>(ids, ids + n_ids), (const FigGapCtl *)ctl, capacity, nsplit, slots_cap, wide_mode, wide_cap, wide_max_active, minc, ipw, *n_active_max, R);   // (rows of four int32, as FigGapCtl is)
    if ((int)R.items.size() * 4 > cap_ints || (int)R.entries.size() * 4 > cap_ints) return -1;
    memcpy(items, R.items.data(), R.items.size() * sizeof(FigItem)); memcpy(entries, R.entries.data(), R.entries.size() * sizeof(FigEntry));
    *n_items = (int)R.items.size(); *n_entries = (int)R.entries.size(); *chunk = R.chunk;
    return R.n_active;
}

extern "C" int fig_fill_gaps(fig_ctx *ctx, const fig_gap_batch *batch, fig_gap_results *out) { return fig_fill_gaps_once(ctx, batch, out); }

// Test-only views of the chunk functions of fig_engine_sched.h (tests/test_wide_chunks.py)
extern "C" int fig_emu_cont_chunk(int minc, int last, int slots, int left) { return fig_cont_chunk(minc, last, slots, left); }
extern "C" int fig_emu_wide_chunk(int mode, int minc, int last, int base, int W, int slots, int left, int consumed_all, int spare) {
    return fig_wide_chunk(FigWide{mode, base, W}, minc, last, slots, left, consumed_all, spare);
}
extern "C" int fig_emu_wide_rank(int mode, int minc, int n, int base, int W, int slots, int left) { return fig_wide_rank(FigWide{mode, base, W}, minc, n, slots, left); }
