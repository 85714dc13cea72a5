// fig_abi.hip -- libfighip.so: the C ABI of include/figbird_hip.h on top of the gfx950 engine.
//
// Host side here = the "packer" role of Figbird.cpp's per-gap loop (Figbird.cpp:7329-7440):
// findFrac/alloc_arg (:6879-6906, :7393-7400), flank extraction, 2-bit read packing, cost
// sorting; then persistent-workgroup launches of fig_fill_kernel, one launch per LDS class.
// There is no CPU compute path in this library.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>
#include <chrono>
#include <thread>
#include <mutex>

#include "../../include/figbird_hip.h"
#include "fig_engine.h"
#include "fig_pack.h"
#include "fig_abi_host.h"
#include "fig_quality.h"
#include "fig_quality_host.h"
#define FIG_PLACEMENT_KERNEL
#include "fig_placement.h"
#include "fig_softqual.h"
#include "fig_indel.h"
#include "fig_polish.h"
#include "fig_recruit.h"
#include "fig_alnqual.h"

// ------------------------------------------------------------------------------------- kernel
#ifdef FIG_PROF
#define FIG_PROF_BEGIN() const unsigned long long _k0 = __builtin_readcyclecounter()
#define FIG_PROF_FLUSH() do { if (E.lane == 0) { atomicAdd(&B.counters[FIG_CNT_WAIT], E.wait_cycles); atomicAdd(&B.counters[FIG_CNT_WAVE], (unsigned long long)__builtin_readcyclecounter() - _k0); \
    for (int i = 0; i < FIG_PROF_SLOTS; i++) if (E.prof[i]) atomicAdd(&B.counters[i < FIG_PROF_SPLIT ? FIG_CNT_PROF_LO + i : FIG_CNT_PROF_HI + (i - FIG_PROF_SPLIT)], E.prof[i]); } } while (0)
#else
#define FIG_PROF_BEGIN() ((void)0)
#define FIG_PROF_FLUSH() ((void)0)
#endif

// What depends on the launch (thread identity, the workgroup's slab); the LDS / slab layout is fig_eng_carve (fig_engine.h).
FIG_D void fig_eng_init(FigEng &E, const FigDevModel &M, const FigDevBatch &B, const FigKernArgs &A, bool lds_tab, FigScr &work) {
    fig_eng_ident(E, threadIdx.x, blockDim.x, 64);
    E.M = &M; E.B = &B;
    E.flops = 0; E.mle_alg = 0; E.mle_exec = 0; E.wait_cycles = 0;
    for (int i = 0; i < FIG_PROF_SLOTS; i++) E.prof[i] = 0;
    unsigned char *slab = B.scratch + (long long)blockIdx.x * B.scratch_stride;
    fig_scratch_layout(slab, B.capG, B.capR, B.capP, B.capC, B.capW, B.capE, &work);
    E.scr = work;
    fig_eng_carve(E, M, A, lds_tab);
}

// Prologue of the five persistent kernels.  Every persistent launch pops from one of its lane's two queue heads and zeroes the
// other for its successor.
FIG_D void fig_kernel_begin(FigEng &E, const FigDevModel &M, const FigDevBatch &B, const FigKernArgs &A, bool lds_tab, FigScr &work) {
    fig_eng_init(E, M, B, A, lds_tab, work);
    if (blockIdx.x == 0 && threadIdx.x == 0) B.queue_head[A.qsel ^ 1] = 0;      // the next launch of this lane pops from the other head
}

// Next index of the launch's work queue, the same in every lane of the workgroup.
FIG_D int fig_queue_pop(FigEng &E, const FigDevBatch &B, const FigKernArgs &A) {
    if (E.tid == 0) E.S->bc_i = atomicAdd(B.queue_head + A.qsel, 1);
    __syncthreads();
    const int qi = E.S->bc_i;
    __syncthreads();
    return qi;
}

// The loop of the persistent kernels: the workgroup pops queue positions until the launch's items are used up and hands each
// to `body`, one of the work-item functions of fig_engine_sched.h.  `src()` names the items, v[first .. end); it is asked at
// every pop, which leaves the three values in the kernel arguments instead of in registers that live across the items.
template <typename T> struct FigItemSrc { const T *v; int first, end; };
FIG_D FigItemSrc<int32_t> fig_src_order(const FigDevBatch &B, const FigKernArgs &A) { return {B.order, A.q_begin, A.q_end}; }   // the class's gaps, by cost

template <typename Src, typename Body>
FIG_D void fig_pop_loop(FigEng &E, const FigDevBatch &B, const FigKernArgs &A, Src src, Body body) {
    while (true) {
        const int qi = fig_queue_pop(E, B, A);
        const auto s = src();
        if (s.first + qi >= s.end) break;
        body(s.v[s.first + qi]);
    }
}

// Epilogue: algorithmic flops and the MLE-pass accounting
FIG_D void fig_kernel_flush(const FigEng &E, const FigDevBatch &B) {
    if (E.flops) atomicAdd(&B.counters[FIG_CNT_FLOPS], E.flops);
    if (E.mle_alg) atomicAdd(&B.counters[FIG_CNT_MLE_ALG], E.mle_alg);
    if (E.lane == 0 && E.mle_exec) atomicAdd(&B.counters[FIG_CNT_MLE_EXEC], E.mle_exec);
}

// ---- sequential mode: whole gaps, one workgroup each (FIG_SCHED=seq)
template <bool LDS_TAB, int NT>
__global__ void __launch_bounds__(NT, (NT <= 256 ? 2 : 1)) fig_fill_kernel(FigDevModel M, FigDevBatch B, FigKernArgs A) {
    FigEng E; FigScr work;
    fig_kernel_begin(E, M, B, A, LDS_TAB, work);
    FIG_PROF_BEGIN();
    fig_pop_loop(E, B, A, [&] { return fig_src_order(B, A); }, [&](int gi) { fig_item_fill<LDS_TAB>(E, work, gi); });
    FIG_PROF_FLUSH();
    fig_kernel_flush(E, B);
}

// ---- candidate-parallel mode, kernel 1: setup + analyzeGap + checkGapReads per gap; skipped gaps finish here
template <bool LDS_TAB, int NT>
__global__ void __launch_bounds__(NT, (NT <= 256 ? 2 : 1)) fig_begin_kernel(FigDevModel M, FigDevBatch B, FigKernArgs A) {
    FigEng E; FigScr work;
    fig_kernel_begin(E, M, B, A, LDS_TAB, work);
    fig_pop_loop(E, B, A, [&] { return fig_src_order(B, A); }, [&](int gi) { fig_item_begin<LDS_TAB>(E, work, gi); });
    fig_kernel_flush(E, B);
}

// ---- pre-pass (partial mode): per gap, does its candidate loop get to Figbird.cpp:6317?  -> FigGapCtl::reach
template <bool LDS_TAB, int NT>
__global__ void __launch_bounds__(NT, (NT <= 256 ? 2 : 1)) fig_probe_kernel(FigDevModel M, FigDevBatch B, FigKernArgs A) {
    FigEng E; FigScr work;
    fig_kernel_begin(E, M, B, A, LDS_TAB, work);
    fig_pop_loop(E, B, A, [&] { return fig_src_order(B, A); }, [&](int gi) { fig_item_probe<LDS_TAB>(E, work, gi); });
}

// ---- the continuous form of the eval launch (fig_engine_sched.h: fig_item_continue): hand-over between workgroups.
// Workgroups of one gap sit on different XCDs, whose L2s are not coherent with each other: everything one workgroup leaves for
// another (a candidate's slot, the replayed state, a continuation) is followed by a device-scope fence of every lane that wrote,
// then one device-scope atomic of lane 0; the reader does the atomic first and the fence after it.  No workgroup ever waits for
// another: nothing below spins, and every loop's trip count is fixed when it is entered.
FIG_D int fig_ld_acquire(const int32_t *p) { return __hip_atomic_load(p, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT); }
FIG_D int fig_ld_relaxed(const int32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// One more item of the gap's chunk of n is done.  True, in every lane, in the one workgroup that finished the chunk; it leaves
// the gap's count at zero for the next chunk, which nobody starts before this workgroup (or the host) has published it.
FIG_D bool fig_chunk_finished(FigEng &E, const FigDevBatch &B, int gi, int n) {
    __threadfence();
    __syncthreads();
    if (E.tid == 0) {
        const int done = __hip_atomic_fetch_add(B.gap_pending + gi, 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) + 1;
        if (done == n) __hip_atomic_store(B.gap_pending + gi, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        E.S->bc_i = done == n;
    }
    __syncthreads();
    const bool last = E.S->bc_i != 0;
    __syncthreads();
    if (last) __threadfence();
    return last;
}

// Publish `c` if the lane's array has room -- and, for a chunk, if enough workgroups of the launch are still there to take
// it: a workgroup that found nothing to claim has left for good, and a chunk published to an emptying launch would run
// item after item in the few that remain.  Otherwise the gap stays as the replay left it (FIG_GAP_MORE / FIG_GAP_LOOP_DONE)
// for the host's next round.
FIG_D void fig_cont_publish(FigEng &E, const FigDevBatch &B, const FigKernArgs &A, const FigCont &c) {
    __threadfence();
    __syncthreads();
    if (E.tid == 0) {
        bool ok = true;
        int n = c.n, rank = c.rank;
        if (c.kind == FIG_CONT_EVAL) {
            const long long live = (long long)gridDim.x - fig_ld_relaxed(&B.cont_hdr->exited);
            ok = live * 100 >= (long long)n * A.cont_live;
            // a widened chunk the emptying launch can no longer take: as many candidates as there are workgroups left, if that is
            // still the chunk the gap would have had without the widening (c.pad); else the host's, like any other
            if (!ok && n > c.pad && A.cont_live > 0) {
                const long long fit = live * 100 / A.cont_live;
                // (rank: the narrower chunk leaves candidates for at least one more chunk than fig_wide_rank counted for the wide
                // one; the exact count needs the gap's slots and range, which the publisher no longer has -- the rank only orders claims)
                if (fit >= c.pad && fit >= 1) { n = (int)(fit < n ? fit : n); rank = rank + 1; ok = true; atomicAdd(&B.counters[FIG_CNT_NARROW], 1ull); }
            }
        }
        if (ok) {
            const int idx = atomicAdd(&B.cont_hdr->tail, 1);
            if (idx < B.cont_cap) {
                FigCont *e = B.cont + idx;
                e->gap = c.gap; e->j0 = c.j0; e->n = n; e->kind = c.kind; e->next = 0; e->rank = rank; e->pad = 0;
                atomicAdd(&B.cont_hdr->open, n);
                __hip_atomic_store(&e->ready, 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
                if (c.kind == FIG_CONT_EVAL) atomicAdd(&B.counters[FIG_CNT_CONT], 1ull);
            }
        }
    }
    __syncthreads();
}

// Idle-driven widening (FIG_WIDE_IDLE): workgroups of the launch that would find nothing to claim once everything unclaimed is
// handed out -- live workgroups less the host-planned items not yet popped and the published items not yet claimed.  A
// snapshot of three counters, the same in every lane; nothing depends on its being exact.
FIG_D int fig_cont_spare(FigEng &E, const FigDevBatch &B, const FigKernArgs &A, int n_items) {
    if (E.tid == 0) {
        const long long live = (long long)gridDim.x - fig_ld_relaxed(&B.cont_hdr->exited);
        const long long popped = fig_ld_relaxed(B.queue_head + A.qsel), open = fig_ld_relaxed(&B.cont_hdr->open);
        const long long waiting = (popped < n_items ? n_items - popped : 0) + (open > 0 ? open : 0);
        E.S->bc_i = live > waiting ? (int)(live - waiting) : 0;
    }
    __syncthreads();
    const int spare = E.S->bc_i;
    __syncthreads();
    return spare;
}

// Claim one item of the continuations published so far: the entry whose gap has the longest chain of chunks ahead (FIG_CONT_PRIO=0:
// the oldest), `k` = the item's place in it.  False: a whole scan found nothing to claim.  An entry not yet ready is skipped,
// not waited for -- its publisher scans after publishing and sees it.  The snapshot of the tail bounds the scan; a claim can be
// lost only to an entry that is used up from then on, so the scan is repeated at most once per entry.
FIG_D bool fig_cont_pop(FigEng &E, const FigDevBatch &B, const FigKernArgs &A, FigCont &out, int &k) {
    FigState &S = *E.S;
    if (E.tid == 0) { const int t = fig_ld_relaxed(&B.cont_hdr->tail); S.bc_j = t < B.cont_cap ? t : B.cont_cap; }
    __syncthreads();
    const int tail = S.bc_j;
    __syncthreads();
    for (int pass = 0; pass <= tail; pass++) {      // (each lost claim uses an entry up: at most `tail` of them, then one scan that finds nothing or claims)
        if (E.tid == 0) S.bc_i = -1;
        __syncthreads();
        int best = -1;
        for (int i = E.tid; i < tail; i += E.nt) {
            const FigCont *e = B.cont + i;
            if (!fig_ld_acquire(&e->ready)) continue;
            if (fig_ld_relaxed(&e->next) >= e->n) continue;
            const int rank = A.cont_prio ? (e->rank < 32767 ? e->rank : 32767) : 0;
            const int key = rank * 65536 + (FIG_CONT_CAP_MAX - i);
            best = key > best ? key : best;
        }
        if (best >= 0) atomicMax(&S.bc_i, best);
        __syncthreads();
        const int key = S.bc_i;
        if (key < 0) { __syncthreads(); return false; }
        const int idx = FIG_CONT_CAP_MAX - (key & 65535);
        if (E.tid == 0) S.bc_j = atomicAdd(&B.cont[idx].next, 1);
        __syncthreads();
        k = S.bc_j;
        __syncthreads();
        if (k < B.cont[idx].n) { if (E.tid == 0) atomicSub(&B.cont_hdr->open, 1); __threadfence(); out = B.cont[idx]; return true; }
    }
    return false;
}

// ---- kernel 2: speculative candidate evaluations; items = FigItem records (passed as int4 *, like fig_replay_kernel's: the symbols stay)
// Continuous form (A.cont): the host-planned items first, then whatever the launch's own workgroups publish, until a scan finds nothing.
static_assert(sizeof(FigItem) == sizeof(int4) && sizeof(FigEntry) == sizeof(int4), "item records travel as int4");
template <bool LDS_TAB, int NT>
__global__ void __launch_bounds__(NT, (NT <= 256 ? 2 : 1)) fig_eval_kernel(FigDevModel M, FigDevBatch B, FigKernArgs A, const int4 *items, int n_items) {
    FigEng E; FigScr work;
    fig_kernel_begin(E, M, B, A, LDS_TAB, work);
    FIG_PROF_BEGIN();
    auto eval = [&](FigItem it) {
        fig_item_eval<LDS_TAB>(E, work, it);
        if (A.cont && it.chunk > 0 && fig_chunk_finished(E, B, it.gap, it.chunk)) {
            FigCont nx;
            const int spare = (A.wide & FIG_WIDE_IDLE) ? fig_cont_spare(E, B, A, n_items) : 0;
            fig_item_continue(E, work, it.gap, it.chunk, A.minc, FigWide{A.wide, A.wide_base, A.wide_cap}, spare, nx);
            fig_cont_publish(E, B, A, nx);
        }
    };
    fig_pop_loop(E, B, A, [&] { return FigItemSrc<FigItem>{(const FigItem *)items, 0, n_items}; }, eval);
    if (A.cont) {
        FigCont c; int k;
        while (fig_cont_pop(E, B, A, c, k)) {
            if (c.kind == FIG_CONT_END) fig_item_end<LDS_TAB>(E, work, c.gap);
            else eval(FigItem{c.gap, c.j0 + k, k, c.n});
        }
        if (E.tid == 0) atomicAdd(&B.cont_hdr->exited, 1);
    }
    FIG_PROF_FLUSH();
    fig_kernel_flush(E, B);
}

// ---- kernel 3: replay the bookkeeping of the speculated candidates in order, one workgroup per entry
// One wave, no class: it touches FigState alone, and its launch asks for no more LDS than that.  fig_eng_carve would place gs /
// rb / plb behind FigState, outside that request, so this kernel keeps them null (a stray use faults instead of corrupting).
__global__ void __launch_bounds__(64) fig_replay_kernel(FigDevModel M, FigDevBatch B, const int4 *entries, int n) {
    if ((int)blockIdx.x >= n) return;
    FigEng E{}; FigScr work{};
    fig_eng_ident(E, threadIdx.x, blockDim.x, 64);
    E.M = &M; E.B = &B; E.nteams = 1; E.S = (FigState *)fig_lds;
    const FigEntry en = ((const FigEntry *)entries)[blockIdx.x];
    if (en.stamped) {                    // continuous form: an eval workgroup has replayed every gap that had a chunk; the gap's j has moved on
        const FigGapCtl c = B.gapctl[en.gap];
        if (c.status != FIG_GAP_MORE || c.j != en.j_planned || en.n != 0) return;
    }
    fig_item_replay(E, work, en);
}

// ---- kernel 4: fallbacks + finalize + output for the gaps whose loop is done; list = gap ids
template <bool LDS_TAB, int NT>
__global__ void __launch_bounds__(NT, (NT <= 256 ? 2 : 1)) fig_end_kernel(FigDevModel M, FigDevBatch B, FigKernArgs A, const int *list, int n) {
    FigEng E; FigScr work;
    fig_kernel_begin(E, M, B, A, LDS_TAB, work);
    fig_pop_loop(E, B, A, [&] { return FigItemSrc<int>{list, 0, n}; }, [&](int gi) { fig_item_end<LDS_TAB>(E, work, gi); });
    fig_kernel_flush(E, B);
}

// ---- upload-time kernel: the operand-select stream of the shared-factor E-step (fig_engine_shared.h).  Entry (read r, chain
// step j) = 0x1000 | 2 * (4 * reverse + base_j): the value M0 takes so that `v_mul_f64 p, v[F0:F0+1], p` in VGPR-index mode
// multiplies by the factor f[orientation][base].  Reads the fast path cannot take (an N base, a length other than L) and the
// empty slots of a gap's last chunk select the constant 1.0.  Layout per gap: [chunk of 32 reads][step][32 reads] 16-bit
// entries, two per dword.  One block per gap.
__global__ void __launch_bounds__(256) fig_stream_kernel(FigDevModel M, FigDevBatch B, uint32_t *out) {
    for (long long gi = blockIdx.x; gi < B.n_gaps; gi += gridDim.x) {
        const FigDevGap &g = B.gaps[gi];
        const int L = M.L;
        const long long n = (long long)((g.nU + FIG_SH_C - 1) / FIG_SH_C) * L * (FIG_SH_C / 2);
        for (long long i = threadIdx.x; i < n; i += blockDim.x) {
            const int sp = (int)(i % (FIG_SH_C / 2));
            const long long cj = i / (FIG_SH_C / 2);
            const int j = (int)(cj % L);
            uint32_t v = 0;
            for (int h = 0; h < 2; h++) {
                const long long r = (cj / L) * FIG_SH_C + 2 * sp + h;
                unsigned e = 0x1000u | FIG_SH_ONE;
                if (r < g.nU) {
                    const long long idx = g.uBase + r;
                    const int len = B.u.len[idx], aux = B.u.aux[idx];
                    if (len == L && !(aux & 2)) {
                        const uint32_t w = B.packed[B.u.woff[idx] + (j >> 4)];
                        e = 0x1000u | (2u * (4u * (unsigned)(aux & 1) + ((w >> ((j & 15) * 2)) & 3u)));
                    }
                }
                v |= e << (16 * h);
            }
            out[g.streamOff + i] = v;
        }
    }
}

// ------------------------------------------------------------------------------------- context
#define FIG_HIP(call) do { hipError_t _e = (call); if (_e != hipSuccess) { ctx->last_hip = (int)_e; return FIG_EHIP; } } while (0)

struct DevBuf { void *p = nullptr; };

// Device buffers that live for one call: whatever way the call returns, they are freed.
struct FigTmpBufs {
    std::vector<void *> bufs;
    ~FigTmpBufs() { for (void *p : bufs) hipFree(p); }
    void *alloc(size_t n) { void *p = nullptr; if (hipMalloc(&p, n ? n : 8) != hipSuccess) return nullptr; bufs.push_back(p); return p; }
};

// Per-class scheduling lane: the classes of a batch run concurrently, each on its own stream with its own work
// queue head, scratch slabs and item buffers, so that the tail of one class's round is filled by the other
// classes' workgroups.
struct FigLane { hipStream_t stream = nullptr; hipEvent_t done = nullptr; int32_t *queue_head = nullptr; uint8_t *scratch = nullptr; FigItem *d_items = nullptr; FigEntry *d_entries = nullptr; size_t cap = 0;   // cap: items / entries the buffers hold
                 FigGapCtl *h_ctl = nullptr; FigItem *h_items = nullptr; FigEntry *h_entries = nullptr; int qsel = 0;   // h_*: pinned, so the copies run on the DMA engines and never wait for a CU
                 uint8_t *d_cont = nullptr; int cont_cap = 0; int wide = 0; };   // continuation array of the lane's eval launches: FigContHdr, then cont_cap entries

struct fig_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    int n_cu = 0;
    int last_hip = 0;
    bool have_model = false;
    FigDevModel dm;
    DevBuf d_model_tabs;
    fig_model hm;
    std::vector<double> h_ins, h_del; // in_pos_dist / del_pos_dist of the model (hm's pointers are the caller's and need not outlive the call)
    // resident batch
    bool have_batch = false;
    FigDevBatch db;
    std::vector<int32_t> h_order;
    struct Cls { FigLaunchClass c; int blocks; int capacity; };
    std::vector<Cls> classes;
    std::vector<DevBuf> bufs;
    int64_t n_gaps = 0, n_ureads = 0, n_preads = 0, str_total = 0;
    std::vector<int64_t> h_str_off;
    int nslots = 32, nslots_wide = 32;    // base slots of a gap's chunk; the wide cap the resident batch was packed with (FIG_SLOTS_WIDE, possibly halved at upload)
    std::vector<FigLane> lanes;
    fig_stats stats;
    int sh_on = FIG_SH_SC;            // FIG_ESTEP / FIG_SH_CHUNKS, read once at fig_ctx_create
    FigKnobs fill_knobs;              // the knobs of the fill under way (the lanes' launches read the continuous form's from here)
    std::vector<uint8_t> h_ot;        // host copy of db.ot_preset
    uint8_t *d_ot = nullptr;
};

static int dev_alloc(fig_ctx *ctx, size_t bytes, void **out) {
    DevBuf b;
    if (bytes == 0) bytes = 8;
    hipError_t e = hipMalloc(&b.p, bytes);
    if (e != hipSuccess) { ctx->last_hip = (int)e; return FIG_ENOMEM; }
    ctx->bufs.push_back(b);
    *out = b.p;
    return FIG_OK;
}

template <typename T>
static int dev_upload(fig_ctx *ctx, const std::vector<T> &v, const T **out) {
    void *p = nullptr;
    int rc = dev_alloc(ctx, v.size() * sizeof(T), &p);
    if (rc) return rc;
    if (!v.empty()) {
        hipError_t e = hipMemcpyAsync(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, ctx->stream);
        if (e != hipSuccess) { ctx->last_hip = (int)e; return FIG_EHIP; }
    }
    *out = (const T *)p;
    return FIG_OK;
}

extern "C" int fig_version(void) { return FIG_ABI_VERSION; }

extern "C" const char *fig_strerror(int code) { return fig_strerror_text(code); }

extern "C" int fig_ctx_create(int device_ordinal, fig_ctx **out) {
    if (!out) return FIG_EINVAL;
    *out = nullptr;
    // A fill runs up to nine streams (one per class lane + the context's own); the HIP runtime maps streams onto
    // GPU_MAX_HW_QUEUES hardware queues (default 4), and two lanes' persistent kernels on one queue serialise.  Asking for 8
    // is worth 1 % of the bench step.  Only effective when this is the process's first HIP call (figfill); a host that
    // initialises HIP earlier sets the variable itself (bench.py and figfill_mp do).
    static std::once_flag env_once;   // contexts may be created from several host threads (figfill with FIGFILL_DEVICES sets it in main() already)
    std::call_once(env_once, [] { setenv("GPU_MAX_HW_QUEUES", "8", 0); });
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return FIG_ENODEV;
    if (device_ordinal < 0 || device_ordinal >= n) return FIG_ENODEV;
    if (hipSetDevice(device_ordinal) != hipSuccess) return FIG_ENODEV;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device_ordinal) != hipSuccess) return FIG_ENODEV;
    fig_ctx *ctx = new (std::nothrow) fig_ctx();
    if (!ctx) return FIG_ENOMEM;
    ctx->device = device_ordinal;
    ctx->n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    if (hipStreamCreate(&ctx->stream) != hipSuccess || hipEventCreate(&ctx->ev0) != hipSuccess || hipEventCreate(&ctx->ev1) != hipSuccess) {
        delete ctx;
        return FIG_EHIP;
    }
    memset(&ctx->stats, 0, sizeof(ctx->stats));
    ctx->sh_on = fig_knobs_from_env(0).sh_on;
    *out = ctx;
    return FIG_OK;
}

static void free_batch(fig_ctx *ctx) {
    for (auto &b : ctx->bufs) if (b.p) hipFree(b.p);
    ctx->bufs.clear();
    ctx->d_ot = nullptr;
    ctx->have_batch = false;
    ctx->classes.clear();
    for (auto &l : ctx->lanes) { if (l.stream) hipStreamDestroy(l.stream); if (l.done) hipEventDestroy(l.done); if (l.h_ctl) hipHostFree(l.h_ctl); if (l.h_items) hipHostFree(l.h_items); if (l.h_entries) hipHostFree(l.h_entries); }
    ctx->lanes.clear();
}

extern "C" void fig_batch_free(fig_ctx *ctx) {
    if (!ctx) return;
    hipSetDevice(ctx->device);
    free_batch(ctx);
}

extern "C" void fig_ctx_destroy(fig_ctx *ctx) {
    if (!ctx) return;
    hipSetDevice(ctx->device);
    free_batch(ctx);
    if (ctx->d_model_tabs.p) hipFree(ctx->d_model_tabs.p);
    if (ctx->ev0) hipEventDestroy(ctx->ev0);
    if (ctx->ev1) hipEventDestroy(ctx->ev1);
    if (ctx->stream) hipStreamDestroy(ctx->stream);
    delete ctx;
}

extern "C" int fig_ctx_set_model(fig_ctx *ctx, const fig_model *m) {
    if (!ctx) return FIG_EINVAL;
    if (int rc = fig_model_check(m)) return rc;
    hipSetDevice(ctx->device);
    free_batch(ctx);                  // a resident batch was packed (classes, capacities, candidate ranges) under the previous model
    ctx->hm = *m;
    ctx->h_ins.assign(m->in_pos_dist, m->in_pos_dist + m->max_read_length);
    ctx->h_del.assign(m->del_pos_dist, m->del_pos_dist + m->max_read_length);
    std::vector<double> all;
    FigModelOffsets o;
    fig_model_tables(m, all, o, ctx->dm);
    if (ctx->d_model_tabs.p) { hipFree(ctx->d_model_tabs.p); ctx->d_model_tabs.p = nullptr; }
    if (hipMalloc(&ctx->d_model_tabs.p, all.size() * sizeof(double)) != hipSuccess) return FIG_ENOMEM;
    if (hipMemcpy(ctx->d_model_tabs.p, all.data(), all.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) return FIG_EHIP;
    fig_model_point(ctx->dm, o, (const double *)ctx->d_model_tabs.p);
    ctx->have_model = true;
    return FIG_OK;
}

extern "C" int64_t fig_results_capacity(const fig_model *m, const fig_gap_batch *b) {
    if (!m || !b) return FIG_EINVAL;
    return fig_pack_results_capacity(m, b);
}

enum FigKind { FIG_K_FILL, FIG_K_BEGIN, FIG_K_EVAL, FIG_K_END, FIG_K_PROBE };   // sequential fill, begin, eval (items), end (list), probe (reach bits)

// one persistent launch of kernel `k` with the class's LDS size
template <typename... P, typename... Args>
static hipError_t launch_one(void (*k)(P...), size_t lds, int nt, int blocks, hipStream_t stream, Args... args) {
    hipError_t e = hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k, dim3(blocks), dim3(nt), lds, stream, args...);
    return hipGetLastError();
}

template <bool LDS_TAB, int NT>
static hipError_t launch_kind(fig_ctx *ctx, const fig_ctx::Cls &c, const FigDevBatch &db, hipStream_t stream, FigKind kind, int blocks, const void *list, int n, int qsel, int wide) {
    FigKernArgs A = fig_kargs_of(c.c, qsel, ctx->sh_on);
    if (kind == FIG_K_EVAL) { const FigKnobs &kn = ctx->fill_knobs; A.cont = kn.cont && db.cont_cap > 0; A.minc = kn.minc; A.cont_live = kn.cont_live; A.cont_prio = kn.cont_prio;
                              A.wide = A.cont ? wide : 0; A.wide_base = ctx->nslots; A.wide_cap = ctx->nslots_wide; }
    if (kind != FIG_K_PROBE) A.mle_reuse = ctx->fill_knobs.mle_reuse;      // the kernels of a fill (the reach pre-pass is partial mode's: off there)
    switch (kind) {
        case FIG_K_FILL: return launch_one(fig_fill_kernel<LDS_TAB, NT>, c.c.lds, NT, blocks, stream, ctx->dm, db, A);
        case FIG_K_BEGIN: return launch_one(fig_begin_kernel<LDS_TAB, NT>, c.c.lds, NT, blocks, stream, ctx->dm, db, A);
        case FIG_K_PROBE: return launch_one(fig_probe_kernel<LDS_TAB, NT>, c.c.lds, NT, blocks, stream, ctx->dm, db, A);
        case FIG_K_EVAL: return launch_one(fig_eval_kernel<LDS_TAB, NT>, c.c.lds, NT, blocks, stream, ctx->dm, db, A, (const int4 *)list, n);
        case FIG_K_END: return launch_one(fig_end_kernel<LDS_TAB, NT>, c.c.lds, NT, blocks, stream, ctx->dm, db, A, (const int *)list, n);
    }
    return hipErrorInvalidValue;
}

static hipError_t launch_any(fig_ctx *ctx, const fig_ctx::Cls &c, const FigDevBatch &db, hipStream_t stream, FigKind kind, int blocks, const void *list, int n, int qsel = 0, int wide = 0) {
    if (c.c.tiles > 0) return launch_kind<true, 512>(ctx, c, db, stream, kind, blocks, list, n, qsel, wide);      // LDS-tiled: the LDS code path with a streamed table
    if (c.c.lds_tab) return c.c.nt == 256 ? launch_kind<true, 256>(ctx, c, db, stream, kind, blocks, list, n, qsel, wide) : launch_kind<true, 512>(ctx, c, db, stream, kind, blocks, list, n, qsel, wide);
    return launch_kind<false, 512>(ctx, c, db, stream, kind, blocks, list, n, qsel, wide);
}

// One attempt of fig_batch_upload with the wide cap `wide_cap` (>= the base slots; `wide_asked`: what the knobs asked for, for the log)
static int fig_upload_once(fig_ctx *ctx, const fig_gap_batch *b, int wide_cap, int wide_asked) {
    free_batch(ctx);
    const fig_model *m = &ctx->hm;
    hipEventRecord(ctx->ev0, ctx->stream);
    FigPacked K;
    const FigKnobs up_knobs = fig_knobs_from_env(0);
    K.nslots_wide = std::max(K.nslots, wide_cap);
    int prc = fig_pack(m, b, sizeof(FigState), K);
    if (prc) return prc;
    // The persistent slab with wide slots: within a quarter of the device memory that is free now, and allocated before anything
    // else, so that an upload that succeeds with the base slots still does -- the wide cap is halved down to the base until it fits.
    void *persist_mem = nullptr;
    const int wide_first = K.nslots_wide;
    K.nslots_wide = K.nslots; fig_pack_persist(K, sizeof(FigState));
    const int64_t persist_base = K.persist_total;      // (what the slab takes with the base slots, for the log)
    K.nslots_wide = wide_first; fig_pack_persist(K, sizeof(FigState));
    size_t mem_free = 0, mem_total = 0;
    if (hipMemGetInfo(&mem_free, &mem_total) != hipSuccess) mem_free = 0;
    while (true) {
        const bool fits = (size_t)K.persist_total + 256 <= mem_free / 4 || K.nslots_wide <= K.nslots;
        if (fits && hipMalloc(&persist_mem, (size_t)K.persist_total + 256) == hipSuccess) break;
        persist_mem = nullptr; (void)hipGetLastError();
        if (K.nslots_wide <= K.nslots) return FIG_ENOMEM;
        K.nslots_wide = std::max(K.nslots, K.nslots_wide / 2);
        fig_pack_persist(K, sizeof(FigState));
    }
    { DevBuf pb; pb.p = persist_mem; ctx->bufs.push_back(pb); }
    int64_t ng = K.n_gaps;
    ctx->h_order = K.order; ctx->h_str_off = K.str_off;
    ctx->str_total = K.str_total; ctx->n_gaps = ng;
    ctx->n_ureads = (int64_t)K.u_pos.size(); ctx->n_preads = (int64_t)K.p_pos.size();
    ctx->classes.clear();
    const bool log = up_knobs.log;
    if (log) fprintf(stderr, "[figsched] persistent slab: %lld B with %d base slots per gap, %lld B with min(candidates, %d) slots per gap%s\n", (long long)persist_base, K.nslots,
                     (long long)K.persist_total, K.nslots_wide, K.nslots_wide < wide_asked ? " (FIG_SLOTS_WIDE halved: what was asked for does not fit, the slab in a quarter of the free device memory or a later allocation)" : "");
    for (const FigLaunchClass &lc : K.classes) {
        fig_ctx::Cls c;
        c.c = lc;
        int per_cu = (int)std::max<size_t>(1, std::min<size_t>((160 * 1024) / std::max<size_t>(lc.lds, 1), (size_t)(2048 / lc.nt)));
        per_cu = std::min(per_cu, 8);
        c.capacity = ctx->n_cu * per_cu;
        c.blocks = std::min<int>(lc.q_end - lc.q_begin, c.capacity);
        if (log) fprintf(stderr, "[figsched] class: capG=%d capGl=%d ncolE=%d Wcap=%d nt=%d nteams=%d lds_tab=%d tiles=%d tile_cols=%d lds=%zu gaps=%d per_cu=%d blocks=%d (FigState %zu B)\n",
                                             lc.capG, lc.capGl, lc.ncolE, lc.Wcap, lc.nt, lc.nteams, (int)lc.lds_tab, lc.tiles, lc.tile_cols, lc.lds, lc.q_end - lc.q_begin, per_cu, c.blocks, sizeof(FigState));
        ctx->classes.push_back(c);
    }
    int64_t stride = fig_scratch_layout(nullptr, K.capG, K.capR, K.capP, K.capC, K.capW, K.capE, nullptr);
    stride = (stride + 255) & ~255LL;

    // ---- upload
    FigDevBatch &db = ctx->db;
    memset(&db, 0, sizeof(db));
    db.n_gaps = ng;
    int rc;
#define UP(vec, field) do { rc = dev_upload(ctx, K.vec, &db.field); if (rc) return rc; } while (0)
    UP(gaps, gaps); UP(order, order); UP(packed, packed); UP(qual, qual); UP(flank, flank);
    UP(u_pos, u.pos); UP(u_aux, u.aux); UP(u_len, u.len); UP(u_woff, u.woff);
    UP(p_pos, p.pos); UP(p_aux, p.aux); UP(p_clip, p.clip); UP(p_ref, p.refpos); UP(p_len, p.len); UP(p_woff, p.woff); UP(p_qoff, p.qoff);
#undef UP
    db.u.clip = nullptr; db.u.refpos = nullptr; db.u.qoff = nullptr;
    void *p;
    if (m->unmapped_flag) {
        if ((rc = dev_alloc(ctx, (size_t)K.stream_total * 4, &p))) return rc;
        db.ustream = (const uint32_t *)p;
        // every entry starts as "select the constant 1.0" in both halves: a slot the kernel does not write never switches indexing off
        FIG_HIP(hipMemsetD32Async((hipDeviceptr_t)p, (int)(((0x1000u | FIG_SH_ONE) << 16) | (0x1000u | FIG_SH_ONE)), (size_t)K.stream_total, ctx->stream));
        if (ng > 0) {
            hipLaunchKernelGGL(fig_stream_kernel, dim3((unsigned)std::min<int64_t>(ng, 4096)), dim3(256), 0, ctx->stream, ctx->dm, db, (uint32_t *)p);
            FIG_HIP(hipGetLastError());
        }
    }
    if ((rc = dev_alloc(ctx, (size_t)ng * 4, &p))) return rc; db.filled_len = (int32_t *)p;
    if ((rc = dev_alloc(ctx, (size_t)ng * 4, &p))) return rc; db.gaptofill = (int32_t *)p;
    if ((rc = dev_alloc(ctx, (size_t)K.str_total, &p))) return rc; db.str = (char *)p;
    if ((rc = dev_alloc(ctx, 64 * (ctx->classes.size() + 1), &p))) return rc; db.queue_head = (int32_t *)p;
    if ((rc = dev_alloc(ctx, FIG_CNT_N * sizeof(unsigned long long), &p))) return rc; db.counters = (unsigned long long *)p;
    size_t total_blocks = 0;
    for (const fig_ctx::Cls &c : ctx->classes) total_blocks += (size_t)c.capacity;
    if ((rc = dev_alloc(ctx, (size_t)stride * std::max<size_t>(total_blocks, 1), &p))) return rc; db.scratch = (uint8_t *)p;
    db.persist = (uint8_t *)persist_mem;
    if ((rc = dev_alloc(ctx, (size_t)std::max<int64_t>(ng, 1) * sizeof(FigGapCtl), &p))) return rc; db.gapctl = (FigGapCtl *)p;
    if ((rc = dev_alloc(ctx, (size_t)std::max<int64_t>(ng, 1) * 4, &p))) return rc; db.gap_pending = (int32_t *)p;
    if ((rc = dev_alloc(ctx, (size_t)std::max<int64_t>(ng, 1), &p))) return rc; ctx->d_ot = (uint8_t *)p; db.ot_preset = ctx->d_ot;
    ctx->h_ot = K.ot_preset;
    FIG_HIP(hipMemcpyAsync(ctx->d_ot, ctx->h_ot.data(), (size_t)std::max<int64_t>(ng, 1), hipMemcpyHostToDevice, ctx->stream));
    ctx->nslots = K.nslots; ctx->nslots_wide = K.nslots_wide;
    {   size_t blk = 0;
        for (size_t ci = 0; ci < ctx->classes.size(); ci++) {
            const fig_ctx::Cls &c = ctx->classes[ci];
            ctx->lanes.push_back(FigLane());          // pushed first: free_batch reclaims whatever was created when a later step fails
            FigLane &l = ctx->lanes.back();
            if (hipStreamCreate(&l.stream) != hipSuccess || hipEventCreateWithFlags(&l.done, hipEventDisableTiming) != hipSuccess) return FIG_EHIP;
            l.queue_head = db.queue_head + 16 * (ci + 1);
            l.scratch = db.scratch + (size_t)stride * blk; blk += (size_t)c.capacity;
            const std::vector<int> lane_ids(K.order.begin() + c.c.q_begin, K.order.begin() + c.c.q_end);
            l.cap = fig_lane_items(lane_ids, K.gaps);
            if ((rc = dev_alloc(ctx, l.cap * sizeof(FigItem), &p))) return rc; l.d_items = (FigItem *)p;
            if ((rc = dev_alloc(ctx, l.cap * sizeof(FigEntry), &p))) return rc; l.d_entries = (FigEntry *)p;
            l.cont_cap = fig_cont_capacity(lane_ids, K.gaps, up_knobs.minc);
            if ((rc = dev_alloc(ctx, sizeof(FigContHdr) + (size_t)l.cont_cap * sizeof(FigCont), &p))) return rc; l.d_cont = (uint8_t *)p;
            if (hipHostMalloc((void **)&l.h_ctl, (size_t)std::max<int64_t>(ng, 1) * sizeof(FigGapCtl), hipHostMallocDefault) != hipSuccess) return FIG_ENOMEM;
            if (hipHostMalloc((void **)&l.h_items, l.cap * sizeof(FigItem), hipHostMallocDefault) != hipSuccess) return FIG_ENOMEM;
            if (hipHostMalloc((void **)&l.h_entries, l.cap * sizeof(FigEntry), hipHostMallocDefault) != hipSuccess) return FIG_ENOMEM;
        }
    }
    db.scratch_stride = stride;
    db.capG = K.capG; db.capR = K.capR; db.capP = K.capP; db.capC = K.capC; db.capW = K.capW; db.capE = K.capE;
    db.n_ureads = ctx->n_ureads;
    FIG_HIP(hipMemsetAsync(db.counters, 0, FIG_CNT_N * sizeof(unsigned long long), ctx->stream));
    FIG_HIP(hipMemsetAsync(db.queue_head, 0, 64 * (ctx->classes.size() + 1), ctx->stream));
    hipEventRecord(ctx->ev1, ctx->stream);
    FIG_HIP(hipStreamSynchronize(ctx->stream));
    float ms = 0; hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1);
    ctx->stats.h2d_ms = ms;
    ctx->stats.packed_bytes = K.packed_bytes();
    ctx->have_batch = true;
    if (!K.ot_given && m->partial_flag && ng > 0 && (rc = fig_ot_carry_measured(ctx, ng))) { free_batch(ctx); return rc; }
    return FIG_OK;
}

// Wide slots (FIG_SLOTS_WIDE) only where the fill would widen: the mode's FIG_WIDE as the knobs stand at upload (a partial-mode
// batch keeps the 64 base slots unless FIG_SCHED=continuous and FIG_WIDE ask otherwise; a fill that asks for widening on such
// a batch gets none).  An upload must not fail where it succeeds with the base slots: when any allocation of an attempt fails,
// the attempt is repeated with half the wide cap, down to the base.
extern "C" int fig_batch_upload(fig_ctx *ctx, const fig_gap_batch *b) {
    if (!ctx || !b) return FIG_EINVAL;
    if (!ctx->have_model) return FIG_EINVAL;
    hipSetDevice(ctx->device);
    const FigKnobs kn = fig_knobs_from_env(ctx->hm.unmapped_flag);
    const int base = FigPacked().nslots;
    const int asked = kn.wide ? std::max(base, std::min(kn.slots_wide, FIG_SLOTS_WIDE_MAX)) : base;
    for (int w = asked;; w = std::max(base, w / 2)) {
        const int rc = fig_upload_once(ctx, b, w, asked);
        if (rc != FIG_ENOMEM || w <= base) return rc;
        (void)hipGetLastError();
    }
}

// Per gap of the resident batch: 1 iff the gap's candidate loop gets to Figbird.cpp:6317 (fig_engine_sched.h: fig_gap_probe).
// Partial mode: one cheap launch per class (setup + the first initialize(), no EM); unmapped mode: all 0 (overlap_threshold is
// never read there, see fig_gap_probe).
extern "C" int fig_batch_probe_reach(fig_ctx *ctx, uint8_t *reach) {
    if (!ctx || !reach || !ctx->have_batch) return FIG_EINVAL;
    hipSetDevice(ctx->device);
    const int64_t ng = ctx->n_gaps;
    memset(reach, 0, (size_t)ng);
    if (!ctx->hm.partial_flag || ng == 0) return FIG_OK;
    FigDevBatch db = ctx->db;
    fig_batch_clear_planes(db);
    FIG_HIP(hipMemsetAsync(db.gapctl, 0, (size_t)ng * sizeof(FigGapCtl), ctx->stream));
    for (const fig_ctx::Cls &c : ctx->classes) {
        FIG_HIP(hipMemsetAsync(db.queue_head, 0, 8, ctx->stream));
        FIG_HIP(launch_any(ctx, c, db, ctx->stream, FIG_K_PROBE, c.blocks, nullptr, 0));
    }
    std::vector<FigGapCtl> ctl((size_t)ng);
    FIG_HIP(hipMemcpyAsync(ctl.data(), db.gapctl, (size_t)ng * sizeof(FigGapCtl), hipMemcpyDeviceToHost, ctx->stream));
    FIG_HIP(hipStreamSynchronize(ctx->stream));
    for (int64_t g = 0; g < ng; g++) reach[g] = ctl[g].reach ? 1 : 0;
    return FIG_OK;
}

// Replaces fig_gap_batch::gap_ot_preset of the resident batch (a caller that fills a shard of a run: probe every shard,
// exchange the bits, carry them along the reference's worker processes -- fig_gaprules.h -- and set the result here).
extern "C" int fig_batch_set_ot_preset(fig_ctx *ctx, const uint8_t *preset) {
    if (!ctx || !preset || !ctx->have_batch) return FIG_EINVAL;
    hipSetDevice(ctx->device);
    const int64_t ng = ctx->n_gaps;
    for (int64_t g = 0; g < ng; g++) ctx->h_ot[(size_t)g] = preset[g] ? 1 : 0;
    if (ng > 0) { FIG_HIP(hipMemcpy(ctx->d_ot, ctx->h_ot.data(), (size_t)ng, hipMemcpyHostToDevice)); }
    return FIG_OK;
}

// Candidate-parallel scheduling of one class (see fig_engine_sched.h).  Host-driven rounds: begin -> {eval chunk,
// replay}* -> end, every round as fig_plan_round (fig_abi_host.h) lays it out.  Returns the number of kernel launches, or
// -1 on a HIP error (ctx->last_hip set).
static int run_class_parallel(fig_ctx *ctx, const fig_ctx::Cls &c, FigLane &ln, const FigKnobs &knobs) {
    FigDevBatch db = ctx->db;
    db.queue_head = ln.queue_head; db.scratch = ln.scratch;
    db.cont_hdr = (FigContHdr *)ln.d_cont; db.cont = (FigCont *)(ln.d_cont + sizeof(FigContHdr));
    db.cont_cap = knobs.cont ? std::min(ln.cont_cap, knobs.cont_cap) : 0;
    const size_t cont_bytes = sizeof(FigContHdr) + (size_t)db.cont_cap * sizeof(FigCont);
    hipStream_t stream = ln.stream;
    hipSetDevice(ctx->device);
    int nl = 0;
    hipError_t e;
    auto fail = [&](hipError_t er) { ctx->last_hip = (int)er; return -1; };
    const int capacity = std::max(1, c.capacity);      // workgroups the device holds for this class (not capped by the gap count)
    // every persistent launch pops from one of the lane's two queue heads and zeroes the other for its successor
    auto launch = [&](FigKind kind, int n_work, const void *list) {
        hipError_t er = launch_any(ctx, c, db, stream, kind, std::min(capacity, n_work), list, n_work, ln.qsel, ln.wide);
        ln.qsel ^= 1; nl++;
        return er;
    };
    if ((e = launch(FIG_K_BEGIN, c.c.q_end - c.c.q_begin, nullptr)) != hipSuccess) return fail(e);
    FigGapCtl *ctl = ln.h_ctl;
    const size_t ctl_bytes = (size_t)ctx->n_gaps * sizeof(FigGapCtl);
    const std::vector<int> ids(ctx->h_order.begin() + c.c.q_begin, ctx->h_order.begin() + c.c.q_end);   // cost-sorted
    FigRound R;
    auto now = [] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    const double t_start = now();
    double t_prev = now(); int round = 0, last_items = 0, last_active = 0, last_chunk = 0, n_active_max = 0;
    while (true) {
        if ((e = hipMemcpyAsync(ctl, db.gapctl, ctl_bytes, hipMemcpyDeviceToHost, stream)) != hipSuccess) return fail(e);
        if ((e = hipStreamSynchronize(stream)) != hipSuccess) return fail(e);
        fig_plan_round(ids, ctl, capacity, c.c.nsplit, ctx->nslots, knobs.wide, ctx->nslots_wide, knobs.wide_max_active, knobs.minc, knobs.ipw, n_active_max, R);
        ln.wide = fig_wide_for_lane(knobs.wide, n_active_max, knobs.wide_max_active);      // (the eval launch of this round widens as the planner did)
        if (knobs.log) { double t = now(); fprintf(stderr, "[figsched] capG=%d round %d: active=%d chunk=%d items=%d blocks=%d  %.1f ms\n", c.c.capG, round, last_active, last_chunk, last_items, capacity, t - t_prev); t_prev = t; }
        round++;
        if (R.n_active == 0) break;
        if (ln.cap < R.items.size() || ln.cap < R.entries.size()) return fail(hipErrorOutOfMemory);
        // continuous form: the eval launch replays every gap that has a chunk and goes on with it; the replay launch is left the gaps with nothing to evaluate
        const int n_empty = knobs.cont ? fig_round_stamp(R, ctl) : 0;
        const int n_items = (int)R.items.size(), n_ent = (int)R.entries.size();
        const size_t items_bytes = R.items.size() * sizeof(FigItem), ent_bytes = R.entries.size() * sizeof(FigEntry);
        last_items = n_items; last_active = R.n_active; last_chunk = R.chunk;
        if (n_items > 0) {
            memcpy(ln.h_items, R.items.data(), items_bytes);
            if ((e = hipMemcpyAsync(ln.d_items, ln.h_items, items_bytes, hipMemcpyHostToDevice, stream)) != hipSuccess) return fail(e);
            if (knobs.cont && (e = hipMemsetAsync(ln.d_cont, 0, cont_bytes, stream)) != hipSuccess) return fail(e);
            if ((e = launch(FIG_K_EVAL, n_items, ln.d_items)) != hipSuccess) return fail(e);
        }
        if (knobs.cont && n_empty == 0) continue;
        memcpy(ln.h_entries, R.entries.data(), ent_bytes);
        if ((e = hipMemcpyAsync(ln.d_entries, ln.h_entries, ent_bytes, hipMemcpyHostToDevice, stream)) != hipSuccess) return fail(e);
        hipLaunchKernelGGL(fig_replay_kernel, dim3(n_ent), dim3(64), sizeof(FigState) + 64, stream, ctx->dm, db, (const int4 *)ln.d_entries, n_ent);
        if ((e = hipGetLastError()) != hipSuccess) return fail(e);
        nl++;
    }
    std::vector<int> endlist;
    for (int g : ids) if (ctl[g].status == FIG_GAP_LOOP_DONE) endlist.push_back(g);
    if (!endlist.empty()) {
        if ((e = hipStreamSynchronize(stream)) != hipSuccess) return fail(e);      // h_items is reused: the last round's upload must have left it
        memcpy(ln.h_items, endlist.data(), endlist.size() * sizeof(int));      // (a gap id per gap of the lane: the item buffers hold nslots + 1 records per gap)
        if ((e = hipMemcpyAsync(ln.d_items, ln.h_items, endlist.size() * sizeof(int), hipMemcpyHostToDevice, stream)) != hipSuccess) return fail(e);
        if ((e = launch(FIG_K_END, (int)endlist.size(), ln.d_items)) != hipSuccess) return fail(e);
        if (knobs.log) { const double t0 = now(); hipStreamSynchronize(stream); fprintf(stderr, "[figsched] capG=%d end kernel: %d gaps, %.1f ms (lane done at %.1f ms since its first round)\n", c.c.capG, (int)endlist.size(), now() - t0, now() - t_start); }
    }
    return nl;
}

extern "C" int fig_fill_resident(fig_ctx *ctx, fig_gap_results *out) { return fig_fill_resident_ex(ctx, out, nullptr); }

extern "C" int fig_fill_resident_ex(fig_ctx *ctx, fig_gap_results *out, const fig_gap_support *sup) {
    if (!ctx || !out || !ctx->have_batch) return FIG_EINVAL;
    if (!out->filled_len || !out->gaptofill || !out->str_off || (!out->str && ctx->str_total > 0)) return FIG_EINVAL;
    if (sup && (!sup->counts || !sup->origin)) return FIG_EINVAL;
    hipSetDevice(ctx->device);
    int64_t ng = ctx->n_gaps;
    FigDevBatch &db = ctx->db;
    // the optional planes live in per-call device buffers
    FigTmpBufs tmp;
    std::vector<int32_t> hsup(sup ? (size_t)ctx->str_total * 5 : 0);
    const std::vector<FigPlane> planes = fig_fill_planes(db, ctx->n_ureads + ctx->n_preads, ctx->str_total, out, sup, hsup.data());
    auto clear = [&](void *p, int v, size_t n) { return n ? hipMemsetAsync(p, v, n, ctx->stream) : hipSuccess; };
    auto fetch = [&](void *dst, const void *src, size_t n) { return n ? hipMemcpyAsync(dst, src, n, hipMemcpyDeviceToHost, ctx->stream) : hipSuccess; };
    for (const FigPlane &pl : planes) {
        if (!(*pl.dev = tmp.alloc(pl.bytes))) return FIG_ENOMEM;
        if (pl.fill >= 0) FIG_HIP(clear(*pl.dev, pl.fill, pl.bytes));
    }
    FIG_HIP(clear(db.counters, 0, FIG_CNT_N * sizeof(unsigned long long)));
    // a previous call that failed half-way may have left queue heads / ping-pong selectors inconsistent: start clean
    FIG_HIP(clear(db.queue_head, 0, 64 * (ctx->classes.size() + 1)));
    for (auto &l : ctx->lanes) l.qsel = 0;
    FIG_HIP(clear(db.filled_len, 0, (size_t)std::max<int64_t>(ng, 1) * 4));
    FIG_HIP(clear(db.gaptofill, 0, (size_t)std::max<int64_t>(ng, 1) * 4));
    FIG_HIP(clear(db.str, 'N', (size_t)ctx->str_total));
    FIG_HIP(clear(db.gapctl, 0, (size_t)std::max<int64_t>(ng, 1) * sizeof(FigGapCtl)));
    FIG_HIP(clear(db.gap_pending, 0, (size_t)std::max<int64_t>(ng, 1) * 4));      // (a lane's continuation array is cleared before each of its eval launches)
    FIG_HIP(hipEventRecord(ctx->ev0, ctx->stream));
    int nl = 0;
    const FigKnobs knobs = fig_knobs_from_env(ctx->dm.unmapped);      // read here, on the caller's thread: the lane threads only get the values
    ctx->fill_knobs = knobs;
    if (knobs.seq) {
        for (const fig_ctx::Cls &c : ctx->classes) {
            FIG_HIP(clear(db.queue_head, 0, 4));
            FIG_HIP(launch_any(ctx, c, db, ctx->stream, FIG_K_FILL, c.blocks, nullptr, 0));
            nl++;
        }
    } else {
        // one host thread + stream per class; every lane starts after ev0 and the main stream joins them before ev1
        const size_t nc = ctx->classes.size();
        std::vector<int> rcs(nc, 0);
        for (size_t ci = 0; ci < nc; ci++) FIG_HIP(hipStreamWaitEvent(ctx->lanes[ci].stream, ctx->ev0, 0));
        if (nc <= 1 || knobs.lanes_serial) {
            for (size_t ci = 0; ci < nc; ci++) rcs[ci] = run_class_parallel(ctx, ctx->classes[ci], ctx->lanes[ci], knobs);
        } else {
            std::vector<std::thread> th;
            for (size_t ci = 0; ci < nc; ci++) th.emplace_back([&, ci] { rcs[ci] = run_class_parallel(ctx, ctx->classes[ci], ctx->lanes[ci], knobs); });
            for (auto &t : th) t.join();
        }
        for (size_t ci = 0; ci < nc; ci++) {
            if (rcs[ci] < 0) { hipDeviceSynchronize(); return FIG_EHIP; }      // (last_hip set by the lane)
            nl += rcs[ci];
            FIG_HIP(hipEventRecord(ctx->lanes[ci].done, ctx->lanes[ci].stream));
            FIG_HIP(hipStreamWaitEvent(ctx->stream, ctx->lanes[ci].done, 0));
        }
    }
    FIG_HIP(hipEventRecord(ctx->ev1, ctx->stream)); FIG_HIP(hipStreamSynchronize(ctx->stream));
    float ms = 0; FIG_HIP(hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
    ctx->stats.kernel_ms = ms; ctx->stats.n_launches = nl;
    // ---- results back
    FIG_HIP(hipEventRecord(ctx->ev0, ctx->stream));
    std::vector<char> hstr((size_t)ctx->str_total);
    unsigned long long cnt[FIG_CNT_N] = {0};
    FIG_HIP(fetch(out->filled_len, db.filled_len, (size_t)ng * 4)); FIG_HIP(fetch(out->gaptofill, db.gaptofill, (size_t)ng * 4));
    FIG_HIP(fetch(hstr.data(), db.str, (size_t)ctx->str_total));
    FIG_HIP(fetch(cnt, db.counters, sizeof(cnt)));
    for (const FigPlane &pl : planes) FIG_HIP(fetch(pl.host, *pl.dev, pl.bytes));
    FIG_HIP(hipEventRecord(ctx->ev1, ctx->stream)); FIG_HIP(hipStreamSynchronize(ctx->stream));
    FIG_HIP(hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
    ctx->stats.d2h_ms = ms;
#ifdef FIG_PROF
    { auto prof = [&](int i) { return cnt[i < FIG_PROF_SPLIT ? FIG_CNT_PROF_LO + i : FIG_CNT_PROF_HI + (i - FIG_PROF_SPLIT)]; };
      const unsigned long long wave = cnt[FIG_CNT_WAVE];
      const char *nm[14] = {"A.wait", "B.wait", "-", "M.finish", "PR.pre", "PR.estep", "PR.mid", "PR.mle", "PR.post", "A.chain", "A.logexp", "A.work", "B.work", "M.chains"};
      for (int i = 0; i < 14; i++) fprintf(stderr, "[figprof] %-9s %8.1f Gcycles = %5.1f %% of wave-cycles\n", nm[i], prof(i) / 1e9, wave ? 100.0 * prof(i) / wave : 0.0);
      const char *mn[4] = {"M.setup", "M.hint", "M.rounds", "M.surv"};
      for (int i = 0; i < 4; i++) fprintf(stderr, "[figprof] %-9s %8.1f Gcycles = %5.1f %% of wave-cycles\n", mn[i], prof(14 + i) / 1e9, wave ? 100.0 * prof(14 + i) / wave : 0.0);
      fprintf(stderr, "[figprof] raw slots:"); for (int i = 0; i < FIG_PROF_SLOTS; i++) fprintf(stderr, " %d:%.1f", i, prof(i) / 1e9); fprintf(stderr, "\n");
      fprintf(stderr, "[figprof] barrier wait %.3f of %.3f wave-Gcycles = %.1f %%\n", cnt[FIG_CNT_WAIT] / 1e9, wave / 1e9, wave ? 100.0 * cnt[FIG_CNT_WAIT] / wave : 0.0); }
#endif
    if (knobs.log) fprintf(stderr, "[figsched] useful flops %.4g, speculative evaluations executed %.4g (%.1f %% discarded)\n", (double)cnt[FIG_CNT_FLOPS], (double)cnt[FIG_CNT_SPEC], cnt[FIG_CNT_SPEC] ? 100.0 * (1.0 - ((double)cnt[FIG_CNT_FLOPS] / (double)cnt[FIG_CNT_SPEC])) : 0.0);
    if (knobs.log && knobs.wide) fprintf(stderr, "[figsched] widened chunks narrowed to the live workgroups: %llu\n", cnt[FIG_CNT_NARROW]);
    if (knobs.log && knobs.mle_reuse) fprintf(stderr, "[figsched] MLE passes reused: %llu of %llu placeReads calls executed (%.1f %%)\n", cnt[FIG_CNT_MLE_REUSED], cnt[FIG_CNT_MLE_ASKED], cnt[FIG_CNT_MLE_ASKED] ? 100.0 * (double)cnt[FIG_CNT_MLE_REUSED] / (double)cnt[FIG_CNT_MLE_ASKED] : 0.0);
    fig_stats_from_counters(cnt, ctx->stats);
    int rc = fig_compact_results(ng, hstr.data(), ctx->h_str_off.data(), out);
    if (!rc && sup) fig_compact_support(ng, hsup.data(), ctx->h_str_off.data(), out, sup->counts);
    return rc;
}

// What the two passes beside the fill, fig_batch_quality and fig_batch_placement, do alike: per-call device buffers, the library's
// stream, nothing of the resident batch or the model is written.  open() checks the context and the caller's strings and fetches
// what the host needs; up() / alloc() own the device buffers; run() is the event-timed launch and the way back.
struct FigPostFill {
    fig_ctx *ctx = nullptr;
    const fig_gap_results *f = nullptr;
    int64_t total = 0;                         // bytes of the caller's strings
    std::vector<FigDevGap> hg;                 // the gap descriptors (read ranges, anchors)
    std::vector<double> tabs;                  // lm[L] | le[L] | lt[16] of the model's e[k] / 1 - e[k] as the device holds them
    std::vector<double> tabs_id;               // lI[L] | lD[L] (band_in)
    FigTmpBufs tmp;
    bool oom = false;
    float ms = 0;

    int open(fig_ctx *c, const fig_gap_results *filled, std::vector<double> *insd = nullptr) {      // insd: the insert-size table as well
        ctx = c; f = filled;
        if (!ctx || !f || !ctx->have_batch || !ctx->have_model) return FIG_EINVAL;
        if (!f->filled_len || !f->str_off || !f->draw_pos || !f->draw_len) return FIG_EINVAL;
        hipSetDevice(ctx->device);
        const int64_t ng = ctx->n_gaps;
        if (f->str_off[0] < 0) return FIG_EINVAL;
        for (int64_t g = 0; g < ng; g++) if (f->str_off[g + 1] < f->str_off[g]) return FIG_EINVAL;
        total = f->str_off[ng];
        if (total > 0 && !f->str) return FIG_EINVAL;
        const int L = ctx->dm.L;
        hg.resize((size_t)ng);
        std::vector<double> he((size_t)L), home((size_t)L);
        tabs.resize((size_t)fig_quality_tab_doubles(L));
        if (ng > 0) FIG_HIP(fetch(hg.data(), ctx->db.gaps, (size_t)ng * sizeof(FigDevGap)));
        FIG_HIP(fetch(he.data(), ctx->dm.e, (size_t)L * sizeof(double)));
        FIG_HIP(fetch(home.data(), ctx->dm.ome1, (size_t)L * sizeof(double)));
        if (insd) { insd->resize((size_t)ctx->dm.max_insert); FIG_HIP(fetch(insd->data(), ctx->dm.insd, insd->size() * sizeof(double))); }
        FIG_HIP(hipStreamSynchronize(ctx->stream));
        fig_quality_tables(L, he.data(), home.data(), ctx->dm.T, tabs.data(), tabs.data() + L, tabs.data() + 2 * L);
        return FIG_OK;
    }
    // A gap that is on, its string of n bytes and its reads base .. base + cnt - 1 of `limit`: how many of them are drawn, or -1
    // where the caller's offsets or draw plane do not hold what the kernel will index with
    int64_t drawn_reads(int64_t g, int32_t n, int64_t base, int64_t cnt, int64_t limit) const {
        if (n > (1 << 30) || f->str_off[g] + n > f->str_off[g + 1] || base < 0 || cnt < 0 || base + cnt > limit) return -1;
        return fig_quality_check_placements(f->draw_pos + base, cnt);
    }
    hipError_t fetch(void *dst, const void *src, size_t bytes) { return hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream); }
    void *alloc(size_t bytes) { void *p = tmp.alloc(bytes); oom = oom || !p; return p; }
    template <typename T> const T *up(const T *src, size_t count) {
        void *p = alloc(count * sizeof(T));
        if (p && count && hipMemcpyAsync(p, src, count * sizeof(T), hipMemcpyHostToDevice, ctx->stream) != hipSuccess) { oom = true; return nullptr; }
        return (const T *)p;
    }
    // the lengths of the unmapped reads as the kernels clamp them, 0 .. L
    int read_lengths(std::vector<int32_t> &hlen) {
        const int64_t nu = ctx->n_ureads;
        hlen.assign((size_t)std::max<int64_t>(nu, 1), 0);
        if (nu > 0) { FIG_HIP(fetch(hlen.data(), ctx->db.u.len, (size_t)nu * sizeof(int32_t))); FIG_HIP(hipStreamSynchronize(ctx->stream)); }
        for (int32_t &l : hlen) l = std::min(std::max(l, 0), ctx->dm.L);
        return FIG_OK;
    }
    // What the four kernels that run the band read alike (fig_band.h): the resident batch, f's offsets and strings, the work items,
    // the gaps' columns and the two table blocks.  T: whose table blocks, built once (a polish round uploads into buffers of its
    // own and takes the call's tables)
    void band_in(FigBandIn &B, const std::vector<int32_t> &items, const std::vector<int32_t> &ncol) { band_in(B, items, ncol, *this); }
    void band_in(FigBandIn &B, const std::vector<int32_t> &items, const std::vector<int32_t> &ncol, FigPostFill &T) {
        const FigDevBatch &db = ctx->db;
        const int64_t ng = ctx->n_gaps;
        const int L = ctx->dm.L;
        if (T.tabs_id.empty()) {
            T.tabs_id.resize((size_t)(2 * L));
            fig_indel_tables(L, ctx->h_ins.data(), ctx->h_del.data(), T.tabs_id.data(), T.tabs_id.data() + L);
        }
        B.gaps = db.gaps; B.u_len = db.u.len; B.u_aux = db.u.aux; B.u_woff = db.u.woff; B.packed = db.packed; B.flank = db.flank; B.L = L;
        B.draw_pos = up(f->draw_pos, (size_t)ctx->n_ureads);
        B.items = up(items.data(), items.size());
        B.ncol = up(ncol.data(), (size_t)ng);
        B.str_off = up(f->str_off, (size_t)(ng + 1));
        B.str = up(f->str, (size_t)f->str_off[ng]);
        B.tabs = up(T.tabs.data(), T.tabs.size());
        B.tabs_id = up(T.tabs_id.data(), T.tabs_id.size());
    }
    // the launch between the context's two events, then `back` (the copies to the host) and the wait; FIG_ENOMEM if an up() / alloc() failed
    template <typename Launch, typename Back> int run(Launch launch, Back back) {
        if (oom) { hipStreamSynchronize(ctx->stream); return FIG_ENOMEM; }
        FIG_HIP(hipEventRecord(ctx->ev0, ctx->stream));
        launch();
        FIG_HIP(hipGetLastError());
        FIG_HIP(hipEventRecord(ctx->ev1, ctx->stream));
        FIG_HIP(back());
        FIG_HIP(hipStreamSynchronize(ctx->stream));
        FIG_HIP(hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
        return FIG_OK;
    }
};
#define FIG_TRY(call) do { const int _rc = (call); if (_rc != FIG_OK) return _rc; } while (0)

// The work items over cnt reads: per chunk of FIG_RS_CHUNK an item {id, first read of the chunk} if of_interest(r) holds for a read r
// of the chunk -- a chunk with no read of interest is no work item.  of_interest sees every read once, in ascending order.
template <typename Pred> static void fig_chunk_items(std::vector<int32_t> &items, int64_t id, int64_t cnt, Pred of_interest) {
    for (int64_t c0 = 0; c0 < cnt; c0 += FIG_RS_CHUNK) {
        bool any = false;
        for (int64_t r = c0; r < std::min<int64_t>(c0 + FIG_RS_CHUNK, cnt); r++) { const bool a = of_interest(r); any = any || a; }
        if (any) { items.push_back((int32_t)id); items.push_back((int32_t)c0); }
    }
}

// Per-base quality of a fill's strings (fig_quality.h: the kernel; fig_quality_host.h: tables, Phred, which gaps are on)
extern "C" int fig_batch_quality(fig_ctx *ctx, const fig_gap_results *f, const int32_t *origin, fig_gap_quality *q) {
    if (!q || !q->loglik || !q->phred || !q->state || (f && !f->draw_isz)) return FIG_EINVAL;
    FigPostFill P;
    FIG_TRY(P.open(ctx, f));
    const int64_t ng = ctx->n_gaps, total = P.total, nr = ctx->n_ureads + ctx->n_preads;
    const FigDevBatch &db = ctx->db;
    // which gaps are on, and the bounds of what the kernel will index with
    std::vector<int32_t> list, ncol((size_t)std::max<int64_t>(ng, 1), 0);
    std::vector<uint8_t> part((size_t)std::max<int64_t>(ng, 1), 0);
    int64_t cols = 0, reads = 0;
    for (int64_t g = 0; g < ng; g++) {
        const int32_t n = f->filled_len[g], lu = f->draw_len[2 * g], lp = f->draw_len[2 * g + 1];
        q->state[g] = fig_quality_gap_on(n, lu, lp, origin != nullptr, origin ? origin[g] : 0);
        if (q->state[g] != FIG_QUAL_ON) continue;
        const bool p = lp >= 0;
        const int64_t base = p ? ctx->n_ureads + P.hg[(size_t)g].pBase : P.hg[(size_t)g].uBase, cnt = p ? P.hg[(size_t)g].nP : P.hg[(size_t)g].nU;
        const int64_t drawn = P.drawn_reads(g, n, base, cnt, nr);
        if (drawn < 0) return FIG_EINVAL;
        list.push_back((int32_t)g); ncol[(size_t)g] = n; part[(size_t)g] = p ? 1 : 0;
        cols += n; reads += drawn;
    }
    if (total > 0) memset(q->loglik, 0, (size_t)total * 4 * sizeof(double));
    if (total > 0) memset(q->phred, 0, (size_t)total);
    if (!list.empty()) {
        FigQualArgs A;
        A.gaps = db.gaps; A.u_len = db.u.len; A.u_aux = db.u.aux; A.p_len = db.p.len; A.u_woff = db.u.woff; A.p_woff = db.p.woff;
        A.packed = db.packed; A.n_ureads = ctx->n_ureads; A.L = ctx->dm.L;
        A.draw_pos = P.up(f->draw_pos, (size_t)nr);
        A.list = P.up(list.data(), list.size());
        A.ncol = P.up(ncol.data(), (size_t)ng);
        A.partial = P.up(part.data(), (size_t)ng);
        A.str_off = P.up(f->str_off, (size_t)(ng + 1));
        A.tabs = P.up(P.tabs.data(), P.tabs.size());
        A.loglik = (double *)P.alloc((size_t)total * 4 * sizeof(double));
        if (A.loglik) FIG_HIP(hipMemsetAsync(A.loglik, 0, (size_t)total * 4 * sizeof(double), ctx->stream));
        FIG_TRY(P.run([&] { hipLaunchKernelGGL(fig_quality_kernel, dim3((unsigned)list.size()), dim3(FIG_Q_NT), 0, ctx->stream, A); },
                      [&] { return P.fetch(q->loglik, A.loglik, (size_t)total * 4 * sizeof(double)); }));
    }
    for (int32_t g : list)
        for (int64_t i = f->str_off[g], e = f->str_off[g] + ncol[(size_t)g]; i < e; i++) q->phred[i] = fig_quality_phred(q->loglik + i * 4, f->str[i]);
    if (fig_knobs_from_env(ctx->dm.unmapped).log)
        fprintf(stderr, "[figqual] gaps on %zu of %lld, columns %lld, reads %lld, kernel %.3f ms\n", list.size(), (long long)ng, (long long)cols, (long long)reads, P.ms);
    return FIG_OK;
}

// The placement pass as fig_batch_placement and fig_batch_softqual both run it: prepare() decides which gaps are on, bounds what the
// kernel will index with, lists the work items and uploads; launch() is the kernel; fetch() / finish() bring the five arrays back
// and fill the caller's struct.
struct FigPlacePass {
    std::vector<int32_t> items, ncol;
    std::vector<uint8_t> scored, state;
    std::vector<double> li, hd;
    std::vector<int32_t> hi;
    int64_t gaps_on = 0, reads = 0, placements = 0, cols = 0, nu = 0;
    FigPlaceArgs A;
    double *dd = nullptr;
    int32_t *di = nullptr;

    int prepare(FigPostFill &P, const int32_t *origin, const std::vector<double> &insd) {
        fig_ctx *ctx = P.ctx;
        const fig_gap_results *f = P.f;
        const int64_t ng = ctx->n_gaps;
        const FigDevBatch &db = ctx->db;
        const int MI = ctx->dm.max_insert;
        nu = ctx->n_ureads;
        li.resize((size_t)MI);
        fig_placement_li(MI, insd.data(), li.data());
        ncol.assign((size_t)std::max<int64_t>(ng, 1), 0);
        state.assign((size_t)std::max<int64_t>(ng, 1), FIG_PLACE_OFF);
        scored.assign((size_t)std::max<int64_t>(nu, 1), 0);
        for (int64_t g = 0; g < ng; g++) {
            const int32_t n = f->filled_len[g];
            state[(size_t)g] = fig_placement_gap_on(ctx->dm.unmapped != 0, n, f->draw_len[2 * g], f->draw_len[2 * g + 1], origin != nullptr, origin ? origin[g] : 0);
            if (state[(size_t)g] != FIG_PLACE_ON) continue;
            const int64_t base = P.hg[(size_t)g].uBase, cnt = P.hg[(size_t)g].nU;
            const int64_t drawn = P.drawn_reads(g, n, base, cnt, nu);
            if (drawn < 0) return FIG_EINVAL;
            gaps_on++; ncol[(size_t)g] = n; reads += drawn; cols += n;
            for (int64_t r = 0; r < cnt; r++) scored[(size_t)(base + r)] = f->draw_pos[base + r] != INT32_MIN;
            fig_chunk_items(items, g, cnt, [&](int64_t r) { return scored[(size_t)(base + r)] != 0; });
        }
        if (items.empty()) return FIG_OK;
        A.gaps = db.gaps; A.u_len = db.u.len; A.u_aux = db.u.aux; A.u_pos = db.u.pos; A.u_woff = db.u.woff; A.packed = db.packed; A.flank = db.flank;
        A.L = ctx->dm.L; A.Tmin = ctx->dm.Tmin; A.Tmax = ctx->dm.Tmax; A.max_insert = MI;
        A.draw_pos = P.up(f->draw_pos, (size_t)nu);
        A.items = P.up(items.data(), items.size());
        A.ncol = P.up(ncol.data(), (size_t)ng);
        A.str_off = P.up(f->str_off, (size_t)(ng + 1));
        A.str = P.up(f->str, (size_t)P.total);
        A.tabs = P.up(P.tabs.data(), P.tabs.size());
        A.li = P.up(li.data(), li.size());
        dd = (double *)P.alloc((size_t)nu * 3 * sizeof(double));
        di = (int32_t *)P.alloc((size_t)nu * 2 * sizeof(int32_t));
        A.ll_drawn = dd; A.ll_other = dd + nu; A.sum_other = dd + 2 * nu; A.off_other = di; A.n_valid = di + nu;
        hd.resize((size_t)nu * 3); hi.resize((size_t)nu * 2);
        return FIG_OK;
    }
    void launch(hipStream_t stream) { hipLaunchKernelGGL(fig_placement_kernel, dim3((unsigned)(items.size() / 2)), dim3(FIG_P_NT), 0, stream, A); }
    hipError_t fetch(FigPostFill &P) { const hipError_t e = P.fetch(hd.data(), dd, hd.size() * sizeof(double)); return e != hipSuccess ? e : P.fetch(hi.data(), di, hi.size() * sizeof(int32_t)); }
    // the caller's struct: the unscored reads' values everywhere, then what the kernel left for the scored ones (`launched`: fetch() has run)
    void finish(fig_read_placement *p, int64_t ng, bool launched) {
        for (int64_t g = 0; g < ng; g++) p->state[g] = state[(size_t)g];
        for (int64_t r = 0; r < nu; r++) {
            p->ll_drawn[r] = 0.0; p->ll_other[r] = 0.0; p->sum_other[r] = 0.0; p->off_other[r] = INT32_MIN; p->n_valid[r] = 0; p->pq[r] = FIG_PLACE_NONE;
        }
        placements = 0;
        if (!launched) return;
        for (int64_t r = 0; r < nu; r++) {
            if (!scored[(size_t)r]) continue;
            p->ll_drawn[r] = hd[(size_t)r]; p->ll_other[r] = hd[(size_t)(nu + r)]; p->sum_other[r] = hd[(size_t)(2 * nu + r)];
            p->off_other[r] = hi[(size_t)r]; p->n_valid[r] = hi[(size_t)(nu + r)];
            p->pq[r] = fig_placement_phred(p->ll_drawn[r], p->ll_other[r], p->sum_other[r]);
            placements += p->n_valid[r];
        }
    }
};
static bool fig_placement_members(const fig_read_placement *p) { return p->ll_drawn && p->ll_other && p->sum_other && p->off_other && p->n_valid && p->pq && p->state; }

// Placement confidence per drawn unmapped read (fig_placement.h: the kernel; fig_placement_host.h: li, insert size, validity, which
// gaps are on, Phred)
extern "C" int fig_batch_placement(fig_ctx *ctx, const fig_gap_results *f, const int32_t *origin, fig_read_placement *p) {
    if (!p || !fig_placement_members(p)) return FIG_EINVAL;
    FigPostFill P;
    std::vector<double> insd;
    FIG_TRY(P.open(ctx, f, &insd));
    FigPlacePass PP;
    FIG_TRY(PP.prepare(P, origin, insd));
    const bool work = !PP.items.empty();
    if (work) FIG_TRY(P.run([&] { PP.launch(ctx->stream); }, [&] { return PP.fetch(P); }));
    PP.finish(p, ctx->n_gaps, work);
    if (fig_knobs_from_env(ctx->dm.unmapped).log)
        fprintf(stderr, "[figplace] gaps on %lld of %lld, reads scored %lld, placements scored %lld, kernel %.3f ms\n", (long long)PP.gaps_on, (long long)ctx->n_gaps, (long long)PP.reads, (long long)PP.placements, P.ms);
    return FIG_OK;
}

// Per-base quality summed over read placements (fig_softqual.h: the kernel; fig_softqual_host.h: which gaps are on, the cut, M / Z):
// the placement pass into per-call buffers, then the pass that reads them, back to back on the library's stream.
extern "C" int fig_batch_softqual(fig_ctx *ctx, const fig_gap_results *f, const int32_t *origin, fig_read_placement *pl, fig_gap_softqual *out) {
    if (!out || !out->wcount || !out->eloglik || !out->phred || !out->state) return FIG_EINVAL;
    if (pl && !fig_placement_members(pl)) return FIG_EINVAL;
    FigPostFill P;
    std::vector<double> insd;
    FIG_TRY(P.open(ctx, f, &insd));
    FigPlacePass PP;
    FIG_TRY(PP.prepare(P, origin, insd));
    const int64_t ng = ctx->n_gaps, total = P.total;
    for (int64_t g = 0; g < ng; g++) out->state[g] = PP.state[(size_t)g] == FIG_PLACE_ON ? FIG_SOFTQ_ON : FIG_SOFTQ_OFF;
    if (total > 0) { memset(out->wcount, 0, (size_t)total * 4 * sizeof(double)); memset(out->eloglik, 0, (size_t)total * 4 * sizeof(double)); memset(out->phred, 0, (size_t)total); }
    const bool work = !PP.items.empty();
    float ms_place = 0, ms_soft = 0;
    int64_t active = 0;
    if (work) {
        std::vector<int32_t> blocks;                             // {gap, first column} of every block of 256 columns of every gap that is on
        for (int64_t g = 0; g < ng; g++)
            if (PP.state[(size_t)g] == FIG_PLACE_ON) for (int32_t xb = 0; xb < PP.ncol[(size_t)g]; xb += FIG_SQ_NT) { blocks.push_back((int32_t)g); blocks.push_back(xb); }
        const size_t nb = blocks.size() / 2, plane = (size_t)total * 4;
        FigSoftqArgs A;
        const FigPlaceArgs &Q = PP.A;
        A.gaps = Q.gaps; A.u_len = Q.u_len; A.u_aux = Q.u_aux; A.u_pos = Q.u_pos; A.u_woff = Q.u_woff; A.packed = Q.packed; A.flank = Q.flank;
        A.draw_pos = Q.draw_pos; A.ncol = Q.ncol; A.str_off = Q.str_off; A.str = Q.str; A.tabs = Q.tabs; A.li = Q.li;
        A.L = Q.L; A.Tmin = Q.Tmin; A.Tmax = Q.Tmax; A.max_insert = Q.max_insert;
        A.placed = PP.dd; A.n_ureads = PP.nu;
        A.items = P.up(blocks.data(), blocks.size());
        double *dp = (double *)P.alloc(plane * 2 * sizeof(double) + nb * sizeof(int32_t));
        A.out = dp; A.plane = (int64_t)plane;
        std::vector<int32_t> hact(nb, 0);
        struct Ev { hipEvent_t e = nullptr; ~Ev() { if (e) hipEventDestroy(e); } } mid;       // between the two launches
        if (P.oom) { hipStreamSynchronize(ctx->stream); return FIG_ENOMEM; }
        FIG_HIP(hipEventCreate(&mid.e));
        FIG_HIP(hipMemsetAsync(dp, 0, plane * 2 * sizeof(double), ctx->stream));
        FIG_HIP(hipEventRecord(ctx->ev0, ctx->stream));
        PP.launch(ctx->stream);
        FIG_HIP(hipGetLastError());
        FIG_HIP(hipEventRecord(mid.e, ctx->stream));
        hipLaunchKernelGGL(fig_softqual_kernel, dim3((unsigned)nb), dim3(FIG_SQ_NT), 0, ctx->stream, A);
        FIG_HIP(hipGetLastError());
        FIG_HIP(hipEventRecord(ctx->ev1, ctx->stream));
        FIG_HIP(P.fetch(out->wcount, dp, plane * sizeof(double)));
        FIG_HIP(P.fetch(out->eloglik, dp + plane, plane * sizeof(double)));
        FIG_HIP(P.fetch(hact.data(), dp + 2 * plane, nb * sizeof(int32_t)));
        if (pl) FIG_HIP(PP.fetch(P));
        FIG_HIP(hipStreamSynchronize(ctx->stream));
        FIG_HIP(hipEventElapsedTime(&ms_place, ctx->ev0, mid.e));
        FIG_HIP(hipEventElapsedTime(&ms_soft, mid.e, ctx->ev1));
        for (int32_t a : hact) active += a;
    }
    if (pl) PP.finish(pl, ng, work);
    for (int64_t g = 0; g < ng; g++)
        if (out->state[g] == FIG_SOFTQ_ON)
            for (int64_t i = f->str_off[g], e = f->str_off[g] + PP.ncol[(size_t)g]; i < e; i++) out->phred[i] = fig_quality_phred(out->eloglik + i * 4, f->str[i]);
    if (fig_knobs_from_env(ctx->dm.unmapped).log)
        fprintf(stderr, "[figsoftq] gaps on %lld of %lld, columns %lld, reads %lld, active placements %lld, placement kernel %.3f ms, softqual kernel %.3f ms\n",
                (long long)PP.gaps_on, (long long)ng, (long long)PP.cols, (long long)PP.reads, (long long)active, ms_place, ms_soft);
    return FIG_OK;
}

// Indel evidence per filled base (fig_indel.h: the kernel and the path; fig_indel_host.h: tables, which gaps are on, which reads are
// aligned, the call)
struct FigIndelInfo { int64_t gaps_on = 0, reads = 0, events = 0, called = 0; float ms = 0; };
// The pass itself, as fig_batch_indel and every round of fig_batch_polish run it: `out` has every member
static int fig_indel_pass(fig_ctx *ctx, const fig_gap_results *f, const int32_t *origin, fig_gap_indel *out, FigIndelInfo &info) {
    FigPostFill P;
    FIG_TRY(P.open(ctx, f));
    const int64_t ng = ctx->n_gaps, total = P.total, nu = ctx->n_ureads;
    std::vector<int32_t> hlen;
    FIG_TRY(P.read_lengths(hlen));
    // which gaps are on, which of their reads are aligned, and the bounds of what the kernel will index with
    std::vector<int32_t> items, ncol((size_t)std::max<int64_t>(ng, 1), 0);
    std::vector<uint8_t> aligned((size_t)std::max<int64_t>(nu, 1), 0);
    int64_t gaps_on = 0, reads = 0, events = 0, called = 0;
    for (int64_t g = 0; g < ng; g++) {
        const int32_t n = f->filled_len[g];
        out->state[g] = fig_indel_gap_on(ctx->dm.unmapped != 0, n, f->draw_len[2 * g], f->draw_len[2 * g + 1], origin != nullptr, origin ? origin[g] : 0);
        if (out->state[g] != FIG_INDEL_ON) continue;
        const int64_t base = P.hg[(size_t)g].uBase, cnt = P.hg[(size_t)g].nU;
        if (P.drawn_reads(g, n, base, cnt, nu) < 0) return FIG_EINVAL;
        gaps_on++; ncol[(size_t)g] = n;
        fig_chunk_items(items, g, cnt, [&](int64_t r) {
            const bool a = fig_indel_aligned(f->draw_pos[base + r], hlen[(size_t)(base + r)], n);
            aligned[(size_t)(base + r)] = a; reads += a;
            return a;
        });
    }
    for (int64_t r = 0; r < nu; r++) { out->ll_flat[r] = 0.0; out->ll_gapped[r] = 0.0; out->n_ins[r] = 0; out->n_del[r] = 0; out->d_end[r] = 0; out->d_start[r] = INT32_MIN; }
    for (int64_t i = 0; i < total; i++) { out->del_reads[i] = 0; out->ins_reads[i] = 0; out->cover[i] = 0; out->call[i] = '.'; }
    for (int64_t g = 0; g < ng; g++) { out->ins_end[g] = 0; out->call_end[g] = '.'; }
    if (!items.empty()) {
        FigIndelArgs A;
        P.band_in(A, items, ncol);
        double *dd = (double *)P.alloc((size_t)nu * 2 * sizeof(double));
        int32_t *di = (int32_t *)P.alloc((size_t)nu * 4 * sizeof(int32_t));
        const size_t ncnt = (size_t)total * 3 + (size_t)ng;                   // del_reads | ins_reads | cover | ins_end
        int32_t *dc = (int32_t *)P.alloc(ncnt * sizeof(int32_t));
        A.ll_flat = dd; A.ll_gapped = dd + nu; A.n_ins = di; A.n_del = di + nu; A.d_end = di + 2 * nu; A.d_start = di + 3 * nu;
        A.del_reads = dc; A.ins_reads = dc + total; A.cover = dc + 2 * total; A.ins_end = dc + 3 * total;
        if (dc) FIG_HIP(hipMemsetAsync(dc, 0, ncnt * sizeof(int32_t), ctx->stream));
        std::vector<double> hd((size_t)nu * 2);
        std::vector<int32_t> hi((size_t)nu * 4);
        FIG_TRY(P.run([&] { fig_indel_launch(A, (unsigned)(items.size() / 2), ctx->stream); },
                      [&] {
                          hipError_t e = P.fetch(hd.data(), dd, hd.size() * sizeof(double));
                          if (e == hipSuccess) e = P.fetch(hi.data(), di, hi.size() * sizeof(int32_t));
                          if (e == hipSuccess && total > 0) e = P.fetch(out->del_reads, A.del_reads, (size_t)total * sizeof(int32_t));
                          if (e == hipSuccess && total > 0) e = P.fetch(out->ins_reads, A.ins_reads, (size_t)total * sizeof(int32_t));
                          if (e == hipSuccess && total > 0) e = P.fetch(out->cover, A.cover, (size_t)total * sizeof(int32_t));
                          return e != hipSuccess ? e : P.fetch(out->ins_end, A.ins_end, (size_t)ng * sizeof(int32_t));
                      }));
        for (int64_t r = 0; r < nu; r++) {
            if (!aligned[(size_t)r]) continue;
            out->ll_flat[r] = hd[(size_t)r]; out->ll_gapped[r] = hd[(size_t)(nu + r)];
            out->n_ins[r] = hi[(size_t)r]; out->n_del[r] = hi[(size_t)(nu + r)]; out->d_end[r] = hi[(size_t)(2 * nu + r)]; out->d_start[r] = hi[(size_t)(3 * nu + r)];
            events += out->n_ins[r] + out->n_del[r] > 0;
        }
        for (int64_t g = 0; g < ng; g++) {
            if (out->state[g] != FIG_INDEL_ON) continue;
            const int64_t s0 = f->str_off[g], n = ncol[(size_t)g];
            for (int64_t i = s0; i < s0 + n; i++) { out->call[i] = fig_indel_call(out->del_reads[i], out->ins_reads[i], out->cover[i]); called += out->call[i] != '.'; }
            out->call_end[g] = fig_indel_majority(out->ins_end[g], out->cover[s0 + n - 1]) ? 'I' : '.';
            called += out->call_end[g] != '.';
        }
    }
    info.gaps_on = gaps_on; info.reads = reads; info.events = events; info.called = called; info.ms = P.ms;
    return FIG_OK;
}
static bool fig_indel_members(const fig_gap_indel *out) {
    return out->ll_flat && out->ll_gapped && out->n_ins && out->n_del && out->d_end && out->d_start && out->del_reads && out->ins_reads &&
           out->cover && out->ins_end && out->call && out->call_end && out->state;
}
extern "C" int fig_batch_indel(fig_ctx *ctx, const fig_gap_results *f, const int32_t *origin, fig_gap_indel *out) {
    if (!out || !fig_indel_members(out)) return FIG_EINVAL;
    FigIndelInfo info;
    FIG_TRY(fig_indel_pass(ctx, f, origin, out, info));
    if (fig_knobs_from_env(ctx->dm.unmapped).log)
        fprintf(stderr, "[figindel] gaps on %lld of %lld, reads aligned %lld, reads with an event %lld, columns called %lld, kernel %.3f ms\n",
                (long long)info.gaps_on, (long long)ctx->n_gaps, (long long)info.reads, (long long)info.events, (long long)info.called, info.ms);
    return FIG_OK;
}

// Polish of the filled strings (fig_polish.h: the scoring kernel; fig_polish_host.h: every rule of the loop and the edit planes).
// The loop works on copies: per gap that is on its current string, the offsets of its reads, the latest pass's ll_gapped and calls.
// Every round is one launch of the polish kernel over all gaps' candidates and one indel pass over all gaps' edited strings.
extern "C" int fig_batch_polish(fig_ctx *ctx, const fig_gap_results *f, const int32_t *origin, int max_rounds, fig_gap_polish *out) {
    if (!out || !out->edit || !out->edit_end || !out->polished_len || !out->draw_pos || !out->n_ins || !out->n_del || !out->rounds ||
        !out->ll_before || !out->ll_after || !out->state) return FIG_EINVAL;
    if (max_rounds < 0 || max_rounds > FIG_POLISH_MAX_ROUNDS) return FIG_EINVAL;
    if (max_rounds == 0) max_rounds = FIG_POLISH_DEFAULT_ROUNDS;
    FigPostFill P;
    FIG_TRY(P.open(ctx, f));
    const int64_t ng = ctx->n_gaps, total = P.total, nu = ctx->n_ureads;
    const size_t gm = (size_t)std::max<int64_t>(ng, 1), um = (size_t)std::max<int64_t>(nu, 1);
    // the buffers of an indel pass; the first runs over the caller's strings and checks them as fig_batch_indel does
    struct Pass {
        std::vector<double> ll_flat, ll; std::vector<int32_t> ri, pl, ie; std::string call, call_end; std::vector<uint8_t> st;
        fig_gap_indel gi;
        void size(size_t um, size_t t, size_t gm) {
            ll_flat.assign(um, 0.0); ll.assign(um, 0.0); ri.assign(um * 4, 0); pl.assign(std::max<size_t>(t, 1) * 3, 0); ie.assign(gm, 0);
            call.assign(std::max<size_t>(t, 1), '.'); call_end.assign(gm, '.'); st.assign(gm, 0);
            const size_t tt = std::max<size_t>(t, 1);
            gi.ll_flat = ll_flat.data(); gi.ll_gapped = ll.data(); gi.n_ins = ri.data(); gi.n_del = ri.data() + um; gi.d_end = ri.data() + 2 * um; gi.d_start = ri.data() + 3 * um;
            gi.del_reads = pl.data(); gi.ins_reads = pl.data() + tt; gi.cover = pl.data() + 2 * tt; gi.ins_end = ie.data();
            gi.call = &call[0]; gi.call_end = &call_end[0]; gi.state = st.data();
        }
    } I;
    I.size(um, (size_t)total, gm);
    FigIndelInfo info;
    float ms_indel = 0, ms_polish = 0;
    FIG_TRY(fig_indel_pass(ctx, f, origin, &I.gi, info));
    ms_indel += info.ms;
    std::vector<int32_t> hlen;
    FIG_TRY(P.read_lengths(hlen));
    // the working copies
    std::vector<std::string> cur(gm), calls(gm);
    std::vector<char> call_end(gm, '.');
    std::vector<uint8_t> active(gm, 0);
    std::vector<int32_t> wpos(um, INT32_MIN), wlen(gm, 0), wdl(2 * gm, -1);
    std::vector<double> curll(I.ll);
    const std::vector<double> ll0(I.ll);
    if (nu > 0) memcpy(wpos.data(), f->draw_pos, (size_t)nu * sizeof(int32_t));
    for (int64_t i = 0; i < total; i++) out->edit[i] = 0;
    int64_t gaps_on = 0, n_sites = 0, n_cands = 0, n_acc = 0, n_rej = 0, n_rev = 0;
    for (int64_t g = 0; g < ng; g++) {
        const bool on = I.st[(size_t)g] == FIG_INDEL_ON;
        out->state[g] = on ? FIG_POLISH_ON : 0; out->edit_end[g] = 0; out->polished_len[g] = f->filled_len[g];
        out->n_ins[g] = 0; out->n_del[g] = 0; out->rounds[g] = 0; out->ll_before[g] = 0.0; out->ll_after[g] = 0.0;
        wlen[(size_t)g] = f->filled_len[g]; wdl[2 * (size_t)g] = f->draw_len[2 * g]; wdl[2 * (size_t)g + 1] = f->draw_len[2 * g + 1];
        if (!on) continue;
        gaps_on++; active[(size_t)g] = 1;
        cur[(size_t)g].assign(f->str + f->str_off[g], (size_t)f->filled_len[g]);
        calls[(size_t)g].assign(I.call, (size_t)f->str_off[g], (size_t)f->filled_len[g]);
        call_end[(size_t)g] = I.call_end[(size_t)g];
    }
    std::vector<int64_t> wso((size_t)ng + 1, 0);
    std::string wstr;
    // the round's strings back to back (nothing for a gap that is off) and the working copies as a fig_gap_results
    auto working = [&] {
        wstr.clear();
        for (int64_t g = 0; g < ng; g++) { wso[(size_t)g] = (int64_t)wstr.size(); if (out->state[g] & FIG_POLISH_ON) wstr += cur[(size_t)g]; }
        wso[(size_t)ng] = (int64_t)wstr.size();
        if (wstr.empty()) wstr.push_back('N');
        fig_gap_results wf;
        memset(&wf, 0, sizeof(wf));
        wf.filled_len = wlen.data(); wf.str_off = wso.data(); wf.str = &wstr[0]; wf.str_capacity = (int64_t)wstr.size();
        wf.draw_pos = wpos.data(); wf.draw_isz = f->draw_isz; wf.draw_len = wdl.data();
        return wf;
    };
    struct Site { int32_t x, kind; int first, m; };               // its candidates are first .. first + m - 1
    struct Saved { int64_t g; std::string str; std::vector<int32_t> pos, edit; int32_t edit_end; };
    int rounds_run = 0;
    for (int round = 1; round <= max_rounds; round++) {
        std::vector<int32_t> cands, items;
        std::vector<int64_t> cand_off;
        std::vector<std::vector<Site>> sites(gm);
        int64_t out_len = 0;
        for (int64_t g = 0; g < ng; g++) {
            if (!active[(size_t)g]) continue;
            const int32_t n = (int32_t)cur[(size_t)g].size(), n0 = f->filled_len[g];
            int32_t sx[FIG_POLISH_MAX_SITES], sk[FIG_POLISH_MAX_SITES];
            const int m = fig_polish_sites(calls[(size_t)g].data(), n, call_end[(size_t)g], sx, sk);
            if (m == 0) { active[(size_t)g] = 0; continue; }
            out->rounds[g]++; n_sites += m;
            const int64_t nU = P.hg[(size_t)g].nU;
            for (int i = 0; i < m; i++) {
                const bool can = sk[i] == FIG_POLISH_DEL ? n >= 2 : fig_polish_can_insert(out->edit + f->str_off[g], n0, out->edit_end[g], sx[i]);
                if (!can) { out->state[g] |= FIG_POLISH_CAPPED; continue; }
                const int nb = sk[i] == FIG_POLISH_DEL ? 1 : 4;
                sites[(size_t)g].push_back({sx[i], sk[i], (int)cand_off.size(), nb});
                for (int b = 0; b < nb; b++) {
                    cands.push_back((int32_t)g); cands.push_back(sk[i]); cands.push_back(sx[i]); cands.push_back(b);
                    cand_off.push_back(out_len); out_len += nU;
                }
            }
            if (sites[(size_t)g].empty()) active[(size_t)g] = 0;
        }
        if (cands.empty()) break;
        rounds_run++;
        n_cands += (int64_t)cand_off.size();
        if (cand_off.size() > (size_t)INT32_MAX / 4) return FIG_EUNSUP;
        for (size_t c = 0; c < cand_off.size(); c++) {            // a candidate's items: the chunks of its gap's reads with a counted read
            const int64_t g = cands[4 * c], base = P.hg[(size_t)g].uBase;
            const int32_t n = (int32_t)cur[(size_t)g].size();
            fig_chunk_items(items, (int64_t)c, P.hg[(size_t)g].nU, [&](int64_t r) {
                return fig_polish_counted(wpos[(size_t)(base + r)], hlen[(size_t)(base + r)], n, cands[4 * c + 1], cands[4 * c + 2]);
            });
        }
        std::vector<double> sc((size_t)std::max<int64_t>(out_len, 1), 0.0);
        if (!items.empty()) {
            const fig_gap_results wf = working();
            FigPostFill Q;                                        // the round's own device buffers, over the working copies
            Q.ctx = ctx; Q.f = &wf;
            std::vector<int32_t> ncol(gm, 0);
            for (int64_t g = 0; g < ng; g++) if (out->state[g] & FIG_POLISH_ON) ncol[(size_t)g] = (int32_t)cur[(size_t)g].size();
            FigPolishArgs A;
            Q.band_in(A, items, ncol, P);
            A.cands = Q.up(cands.data(), cands.size());
            A.cand_off = Q.up(cand_off.data(), cand_off.size());
            A.out = (double *)Q.alloc((size_t)out_len * sizeof(double));
            if (A.out) FIG_HIP(hipMemsetAsync(A.out, 0, (size_t)out_len * sizeof(double), ctx->stream));
            FIG_TRY(Q.run([&] { fig_polish_launch(A, (unsigned)(items.size() / 2), ctx->stream); },
                          [&] { return Q.fetch(sc.data(), A.out, (size_t)out_len * sizeof(double)); }));
            ms_polish += Q.ms;
        }
        // best per site, accept, apply
        std::vector<Saved> saved;
        for (int64_t g = 0; g < ng; g++) {
            if (sites[(size_t)g].empty()) continue;
            const int64_t base = P.hg[(size_t)g].uBase, cnt = P.hg[(size_t)g].nU, s0 = f->str_off[g];
            const int32_t n = (int32_t)cur[(size_t)g].size(), n0 = f->filled_len[g];
            std::vector<std::pair<const Site *, int>> acc;        // the site and the base of its accepted candidate
            for (const Site &s : sites[(size_t)g]) {
                double T[4], T0 = 0.0;
                for (int b = 0; b < s.m; b++) T[b] = 0.0;
                for (int64_t r = 0; r < cnt; r++) {
                    if (!fig_polish_counted(wpos[(size_t)(base + r)], hlen[(size_t)(base + r)], n, s.kind, s.x)) continue;
                    T0 = T0 + curll[(size_t)(base + r)];
                    for (int b = 0; b < s.m; b++) T[b] = T[b] + sc[(size_t)(cand_off[(size_t)(s.first + b)] + r)];
                }
                const int best = fig_polish_best(T, s.m);
                if (fig_polish_accept(T[best], T0)) { acc.push_back({&s, best}); n_acc++; }
                else { out->state[g] |= FIG_POLISH_REJECTED; n_rej++; }
            }
            if (acc.empty()) { active[(size_t)g] = 0; continue; }
            saved.push_back({g, cur[(size_t)g], std::vector<int32_t>(wpos.begin() + base, wpos.begin() + base + cnt),
                             std::vector<int32_t>(out->edit + s0, out->edit + s0 + n0), out->edit_end[g]});
            int applied = 0;
            for (size_t a = acc.size(); a-- > 0;) {               // right to left
                const Site &s = *acc[a].first;
                std::string &str = cur[(size_t)g];
                if (s.kind == FIG_POLISH_DEL) {
                    if (str.size() < 2) { out->state[g] |= FIG_POLISH_CAPPED; continue; }
                    fig_polish_remove(out->edit + s0, n0, &out->edit_end[g], s.x);
                    str.erase((size_t)s.x, 1);
                } else {
                    if (fig_polish_insert(out->edit + s0, n0, &out->edit_end[g], s.x, acc[a].second) != 1) { out->state[g] |= FIG_POLISH_CAPPED; continue; }
                    str.insert((size_t)s.x, 1, "ACGT"[acc[a].second]);
                }
                for (int64_t r = 0; r < cnt; r++) if (wpos[(size_t)(base + r)] != INT32_MIN) wpos[(size_t)(base + r)] = fig_polish_shift(wpos[(size_t)(base + r)], s.kind, s.x);
                applied++;
            }
            if (!applied) { saved.pop_back(); active[(size_t)g] = 0; }                                 // every accepted edit was dropped
        }
        if (saved.empty()) break;
        // verify: the next pass over the edited strings
        for (int64_t g = 0; g < ng; g++) if (out->state[g] & FIG_POLISH_ON) { wlen[(size_t)g] = (int32_t)cur[(size_t)g].size(); wdl[2 * (size_t)g] = wlen[(size_t)g]; }
        const fig_gap_results wf = working();
        Pass V;
        V.size(um, (size_t)wso[(size_t)ng], gm);
        FIG_TRY(fig_indel_pass(ctx, &wf, origin, &V.gi, info));
        ms_indel += info.ms;
        for (int64_t g = 0; g < ng; g++) if ((out->state[g] & FIG_POLISH_ON) && V.st[(size_t)g] != FIG_INDEL_ON) return FIG_EHIP;      // (cannot happen: n >= 1 and the header follows n)
        for (const Saved &S : saved) {
            const int64_t g = S.g, base = P.hg[(size_t)g].uBase, cnt = P.hg[(size_t)g].nU, s0 = f->str_off[g];
            const int32_t n_old = (int32_t)S.str.size(), n_new = (int32_t)cur[(size_t)g].size();
            double Vn = 0.0, Vo = 0.0;
            for (int64_t r = 0; r < cnt; r++) {
                if (!fig_indel_aligned(S.pos[(size_t)r], hlen[(size_t)(base + r)], n_old) || !fig_indel_aligned(wpos[(size_t)(base + r)], hlen[(size_t)(base + r)], n_new)) continue;
                Vn = Vn + V.ll[(size_t)(base + r)]; Vo = Vo + curll[(size_t)(base + r)];
            }
            if (fig_polish_keep(Vn, Vo)) {
                out->state[g] |= FIG_POLISH_EDITED;
                for (int64_t r = 0; r < cnt; r++) curll[(size_t)(base + r)] = V.ll[(size_t)(base + r)];
                calls[(size_t)g].assign(V.call, (size_t)wso[(size_t)g], (size_t)n_new);
                call_end[(size_t)g] = V.call_end[(size_t)g];
            } else {
                out->state[g] |= FIG_POLISH_REVERTED; n_rev++;
                cur[(size_t)g] = S.str;
                std::copy(S.pos.begin(), S.pos.end(), wpos.begin() + base);
                std::copy(S.edit.begin(), S.edit.end(), out->edit + s0);
                out->edit_end[g] = S.edit_end;
                wlen[(size_t)g] = n_old; wdl[2 * (size_t)g] = n_old;
                active[(size_t)g] = 0;
            }
        }
    }
    for (int64_t g = 0; g < ng; g++) {
        if (!(out->state[g] & FIG_POLISH_ON)) continue;
        if (active[(size_t)g] && (calls[(size_t)g].find_first_not_of('.') != std::string::npos || call_end[(size_t)g] != '.')) out->state[g] |= FIG_POLISH_CAPPED;
        const int64_t base = P.hg[(size_t)g].uBase, cnt = P.hg[(size_t)g].nU, s0 = f->str_off[g];
        const int32_t n0 = f->filled_len[g], n1 = (int32_t)cur[(size_t)g].size();
        out->polished_len[g] = n1;
        out->n_ins[g] = fig_polish_k(out->edit_end[g]);
        for (int32_t x = 0; x < n0; x++) { out->n_ins[g] += fig_polish_k(out->edit[s0 + x]); out->n_del[g] += out->edit[s0 + x] & 1; }
        double lb = 0.0, la = 0.0;
        for (int64_t r = 0; r < cnt; r++) {
            if (!fig_indel_aligned(f->draw_pos[base + r], hlen[(size_t)(base + r)], n0) || !fig_indel_aligned(wpos[(size_t)(base + r)], hlen[(size_t)(base + r)], n1)) continue;
            lb = lb + ll0[(size_t)(base + r)]; la = la + curll[(size_t)(base + r)];
        }
        out->ll_before[g] = lb; out->ll_after[g] = la;
    }
    for (int64_t r = 0; r < nu; r++) out->draw_pos[r] = wpos[(size_t)r];
    if (fig_knobs_from_env(ctx->dm.unmapped).log)
        fprintf(stderr, "[figpolish] gaps on %lld of %lld, rounds %d, sites %lld, candidates scored %lld, edits accepted %lld, rejected %lld, rounds reverted %lld, indel kernels %.3f ms, polish kernels %.3f ms\n",
                (long long)gaps_on, (long long)ng, rounds_run, (long long)n_sites, (long long)n_cands, (long long)n_acc, (long long)n_rej, (long long)n_rev, ms_indel, ms_polish);
    return FIG_OK;
}

extern "C" int fig_polish_apply(const fig_gap_results *filled, const fig_gap_polish *p, int64_t g, char *dst) { return fig_polish_apply_body(filled, p, g, dst); }

// Recruiting of the reads the fill rejected (fig_recruit.h: the kernel; fig_recruit_host.h: which gaps are on, which reads are
// candidates, the score, the rule and the merge).  One launch over the chunks that hold a candidate.
extern "C" int fig_batch_recruit(fig_ctx *ctx, const fig_gap_results *f, const int32_t *origin, double min_margin, fig_read_recruit *out) {
    if (!out || !out->ll_seed || !out->ll_second || !out->ll_flat || !out->ll_gapped || !out->score || !out->off_seed || !out->off_second || !out->n_valid ||
        !out->d_end || !out->read_state || !out->draw_pos || !out->draw_isz || !out->n_candidates || !out->n_recruited || !out->state) return FIG_EINVAL;
    if (!fig_recruit_margin_ok(min_margin) || (f && !f->draw_isz)) return FIG_EINVAL;
    FigPostFill P;
    std::vector<double> insd;
    FIG_TRY(P.open(ctx, f, &insd));
    const int64_t ng = ctx->n_gaps, nu = ctx->n_ureads;
    const int MI = ctx->dm.max_insert;
    std::vector<int32_t> hlen;
    FIG_TRY(P.read_lengths(hlen));
    // which gaps are on, which of their reads are candidates, and the bounds of what the kernel will index with
    std::vector<int32_t> items, ncol((size_t)std::max<int64_t>(ng, 1), 0);
    std::vector<uint8_t> rstate((size_t)std::max<int64_t>(nu, 1), FIG_RECRUIT_READ_OFF);
    int64_t gaps_on = 0, cands = 0, seeded = 0, recruited = 0, below = 0, ambiguous = 0, placements = 0;
    for (int64_t g = 0; g < ng; g++) {
        const int32_t n = f->filled_len[g];
        out->state[g] = fig_recruit_gap_on(ctx->dm.unmapped != 0, n, f->draw_len[2 * g], f->draw_len[2 * g + 1], origin != nullptr, origin ? origin[g] : 0);
        out->n_candidates[g] = 0; out->n_recruited[g] = 0;
        if (out->state[g] != FIG_RECRUIT_ON) continue;
        const int64_t base = P.hg[(size_t)g].uBase, cnt = P.hg[(size_t)g].nU;
        if (P.drawn_reads(g, n, base, cnt, nu) < 0) return FIG_EINVAL;
        gaps_on++; ncol[(size_t)g] = n;
        fig_chunk_items(items, g, cnt, [&](int64_t r) {
            const bool c = fig_recruit_candidate(f->draw_pos[base + r]);
            rstate[(size_t)(base + r)] = c ? FIG_RECRUIT_NONE : FIG_RECRUIT_KEPT;
            out->n_candidates[g] += c;
            return c;
        });
        cands += out->n_candidates[g];
    }
    const double ninf = -std::numeric_limits<double>::infinity();
    for (int64_t r = 0; r < nu; r++) {
        out->ll_seed[r] = 0.0; out->ll_second[r] = 0.0; out->ll_flat[r] = 0.0; out->ll_gapped[r] = 0.0; out->score[r] = 0.0;
        out->off_seed[r] = INT32_MIN; out->off_second[r] = INT32_MIN; out->n_valid[r] = 0; out->d_end[r] = 0; out->read_state[r] = rstate[(size_t)r];
        if (rstate[(size_t)r] == FIG_RECRUIT_NONE) out->ll_seed[r] = ninf;
        fig_recruit_merge(rstate[(size_t)r], f->draw_pos[r], f->draw_isz[r], INT32_MIN, 0, out->draw_pos[r], out->draw_isz[r]);
    }
    if (!items.empty()) {
        std::vector<double> li((size_t)MI);
        fig_placement_li(MI, insd.data(), li.data());
        FigBandIn B;
        P.band_in(B, items, ncol);
        FigRecruitArgs A;                                         // its own member order (fig_recruit.h)
        A.gaps = B.gaps; A.u_len = B.u_len; A.u_aux = B.u_aux; A.u_woff = B.u_woff; A.packed = B.packed; A.flank = B.flank; A.L = B.L;
        A.draw_pos = B.draw_pos; A.items = B.items; A.ncol = B.ncol; A.str_off = B.str_off; A.str = B.str; A.tabs = B.tabs; A.tabs_id = B.tabs_id;
        A.u_pos = ctx->db.u.pos; A.Tmin = ctx->dm.Tmin; A.Tmax = ctx->dm.Tmax; A.max_insert = MI;
        A.li = P.up(li.data(), li.size());
        double *dd = (double *)P.alloc((size_t)nu * 4 * sizeof(double));
        int32_t *di = (int32_t *)P.alloc((size_t)nu * 5 * sizeof(int32_t));
        A.ll_seed = dd; A.ll_second = dd + nu; A.ll_flat = dd + 2 * nu; A.ll_gapped = dd + 3 * nu;
        A.off_seed = di; A.n_valid = di + nu; A.off_second = di + 2 * nu; A.d_end = di + 3 * nu; A.isz_seed = di + 4 * nu;
        std::vector<double> hd((size_t)nu * 4);
        std::vector<int32_t> hi((size_t)nu * 5);
        FIG_TRY(P.run([&] { fig_recruit_launch(A, (unsigned)(items.size() / 2), ctx->stream); },
                      [&] { const hipError_t e = P.fetch(hd.data(), dd, hd.size() * sizeof(double)); return e != hipSuccess ? e : P.fetch(hi.data(), di, hi.size() * sizeof(int32_t)); }));
        // the kernel wrote ll_seed, off_seed and n_valid for the candidates of positive length and the rest for the seeded ones
        for (int64_t g = 0; g < ng; g++) {
            if (out->state[g] != FIG_RECRUIT_ON) continue;
            for (int64_t r = P.hg[(size_t)g].uBase, e = r + P.hg[(size_t)g].nU; r < e; r++) {
                if (rstate[(size_t)r] != FIG_RECRUIT_NONE || hlen[(size_t)r] == 0) continue;
                out->n_valid[r] = hi[(size_t)(nu + r)];
                placements += out->n_valid[r];
                if (!fig_recruit_seeded(out->n_valid[r], hd[(size_t)r])) continue;
                seeded++;
                out->ll_seed[r] = hd[(size_t)r]; out->ll_second[r] = hd[(size_t)(nu + r)]; out->ll_flat[r] = hd[(size_t)(2 * nu + r)]; out->ll_gapped[r] = hd[(size_t)(3 * nu + r)];
                out->off_seed[r] = hi[(size_t)r]; out->off_second[r] = hi[(size_t)(2 * nu + r)]; out->d_end[r] = hi[(size_t)(3 * nu + r)];
                const int32_t isz = hi[(size_t)(4 * nu + r)];
                if (isz < 0 || isz >= MI) return FIG_EHIP;                       // (the kernel reports valid placements only)
                out->score[r] = fig_recruit_score(li[(size_t)isz], out->ll_gapped[r]);
                const uint8_t s = fig_recruit_rule(out->score[r], ctx->dm.cutoff, out->ll_seed[r], out->ll_second[r], min_margin);
                out->read_state[r] = s;
                fig_recruit_merge(s, f->draw_pos[r], f->draw_isz[r], out->off_seed[r], isz, out->draw_pos[r], out->draw_isz[r]);
                recruited += s == FIG_RECRUIT_RECRUITED; below += s == FIG_RECRUIT_BELOW; ambiguous += s == FIG_RECRUIT_AMBIGUOUS;
                out->n_recruited[g] += s == FIG_RECRUIT_RECRUITED;
            }
        }
    }
    if (fig_knobs_from_env(ctx->dm.unmapped).log)
        fprintf(stderr, "[figrecruit] gaps on %lld of %lld, candidates %lld, seeded %lld, recruited %lld, below %lld, ambiguous %lld, placements scored %lld, kernel %.3f ms\n",
                (long long)gaps_on, (long long)ng, (long long)cands, (long long)seeded, (long long)recruited, (long long)below, (long long)ambiguous, (long long)placements, P.ms);
    return FIG_OK;
}

// Per-base quality over gapped read alignments (fig_alnqual.h: the two kernels and the walk; fig_alnqual_host.h: which gaps are on,
// the map, the span, the step of a column).  The path kernel over the chunks that hold an aligned read, then the column kernel over the
// gaps that are on, back to back on the library's stream.
extern "C" int fig_batch_alnqual(fig_ctx *ctx, const fig_gap_results *f, const int32_t *origin, fig_gap_alnqual *out) {
    if (!out || !out->loglik || !out->depth || !out->agree || !out->skip || !out->phred || !out->ll_gapped || !out->n_ins || !out->n_del || !out->d_end ||
        !out->d_start || !out->state) return FIG_EINVAL;
    FigPostFill P;
    FIG_TRY(P.open(ctx, f));
    const int64_t ng = ctx->n_gaps, total = P.total, nu = ctx->n_ureads;
    std::vector<int32_t> hlen;
    FIG_TRY(P.read_lengths(hlen));
    // which gaps are on, which of their reads are aligned, and the bounds of what the kernels will index with
    std::vector<int32_t> items, list, ncol((size_t)std::max<int64_t>(ng, 1), 0);
    std::vector<uint8_t> aligned((size_t)std::max<int64_t>(nu, 1), 0);
    int64_t reads = 0, events = 0, cols = 0;
    for (int64_t g = 0; g < ng; g++) {
        const int32_t n = f->filled_len[g];
        out->state[g] = fig_alnqual_gap_on(ctx->dm.unmapped != 0, n, f->draw_len[2 * g], f->draw_len[2 * g + 1], origin != nullptr, origin ? origin[g] : 0);
        if (out->state[g] != FIG_ALNQ_ON) continue;
        const int64_t base = P.hg[(size_t)g].uBase, cnt = P.hg[(size_t)g].nU;
        if (P.drawn_reads(g, n, base, cnt, nu) < 0) return FIG_EINVAL;
        list.push_back((int32_t)g); ncol[(size_t)g] = n; cols += n;
        fig_chunk_items(items, g, cnt, [&](int64_t r) {
            const bool a = fig_indel_aligned(f->draw_pos[base + r], hlen[(size_t)(base + r)], n);
            aligned[(size_t)(base + r)] = a; reads += a;
            return a;
        });
    }
    for (int64_t r = 0; r < nu; r++) { out->ll_gapped[r] = 0.0; out->n_ins[r] = 0; out->n_del[r] = 0; out->d_end[r] = 0; out->d_start[r] = INT32_MIN; }
    if (total > 0) memset(out->loglik, 0, (size_t)total * 4 * sizeof(double));
    for (int64_t i = 0; i < total; i++) { out->depth[i] = 0; out->agree[i] = 0; out->skip[i] = 0; out->phred[i] = 0; }
    float ms_path = 0, ms_col = 0;
    if (!list.empty()) {
        FigAlnPathArgs A;
        P.band_in(A, items, ncol);
        A.map = (uint32_t *)P.alloc((size_t)std::max<int64_t>(nu, 1) * FIG_ALNQ_MAPW * sizeof(uint32_t));
        double *dd = (double *)P.alloc((size_t)std::max<int64_t>(nu, 1) * sizeof(double));
        int32_t *di = (int32_t *)P.alloc((size_t)std::max<int64_t>(nu, 1) * 6 * sizeof(int32_t));
        A.ll_gapped = dd; A.n_ins = di; A.n_del = di + nu; A.d_end = di + 2 * nu; A.d_start = di + 3 * nu; A.span = di + 4 * nu;
        FigAlnColArgs B;
        B.gaps = A.gaps; B.u_len = A.u_len; B.u_aux = A.u_aux; B.u_woff = A.u_woff; B.packed = A.packed; B.L = A.L;
        B.draw_pos = A.draw_pos; B.ncol = A.ncol; B.str_off = A.str_off; B.str = A.str; B.tabs = A.tabs; B.map = A.map; B.span = A.span;
        B.list = P.up(list.data(), list.size());
        B.loglik = (double *)P.alloc((size_t)total * 4 * sizeof(double));
        int32_t *dc = (int32_t *)P.alloc((size_t)total * 3 * sizeof(int32_t));                // depth | agree | skip
        B.depth = dc; B.agree = dc + total; B.skip = dc + 2 * total;
        std::vector<double> hd((size_t)nu);
        std::vector<int32_t> hi((size_t)nu * 4);
        struct Ev { hipEvent_t e = nullptr; ~Ev() { if (e) hipEventDestroy(e); } } mid;       // between the two launches
        if (P.oom) { hipStreamSynchronize(ctx->stream); return FIG_ENOMEM; }
        FIG_HIP(hipEventCreate(&mid.e));
        FIG_HIP(hipMemsetAsync(B.loglik, 0, (size_t)total * 4 * sizeof(double), ctx->stream));
        FIG_HIP(hipMemsetAsync(dc, 0, (size_t)total * 3 * sizeof(int32_t), ctx->stream));
        FIG_HIP(hipEventRecord(ctx->ev0, ctx->stream));
        if (!items.empty()) FIG_HIP(fig_alnqual_path_launch(A, (unsigned)(items.size() / 2), ctx->stream));
        FIG_HIP(hipEventRecord(mid.e, ctx->stream));
        FIG_HIP(fig_alnqual_column_launch(B, (unsigned)list.size(), ctx->stream));
        FIG_HIP(hipEventRecord(ctx->ev1, ctx->stream));
        FIG_HIP(P.fetch(out->loglik, B.loglik, (size_t)total * 4 * sizeof(double)));
        FIG_HIP(P.fetch(out->depth, B.depth, (size_t)total * sizeof(int32_t)));
        FIG_HIP(P.fetch(out->agree, B.agree, (size_t)total * sizeof(int32_t)));
        FIG_HIP(P.fetch(out->skip, B.skip, (size_t)total * sizeof(int32_t)));
        if (nu > 0) { FIG_HIP(P.fetch(hd.data(), dd, hd.size() * sizeof(double))); FIG_HIP(P.fetch(hi.data(), di, hi.size() * sizeof(int32_t))); }
        FIG_HIP(hipStreamSynchronize(ctx->stream));
        FIG_HIP(hipEventElapsedTime(&ms_path, ctx->ev0, mid.e));
        FIG_HIP(hipEventElapsedTime(&ms_col, mid.e, ctx->ev1));
        for (int64_t r = 0; r < nu; r++) {
            if (!aligned[(size_t)r]) continue;
            out->ll_gapped[r] = hd[(size_t)r];
            out->n_ins[r] = hi[(size_t)r]; out->n_del[r] = hi[(size_t)(nu + r)]; out->d_end[r] = hi[(size_t)(2 * nu + r)]; out->d_start[r] = hi[(size_t)(3 * nu + r)];
            events += out->n_ins[r] + out->n_del[r] > 0;
        }
        for (int32_t g : list)
            for (int64_t i = f->str_off[g], e = f->str_off[g] + ncol[(size_t)g]; i < e; i++) out->phred[i] = fig_quality_phred(out->loglik + i * 4, f->str[i]);
    }
    if (fig_knobs_from_env(ctx->dm.unmapped).log)
        fprintf(stderr, "[figalnqual] gaps on %zu of %lld, reads aligned %lld, reads with an event %lld, columns %lld, path kernel %.3f ms, column kernel %.3f ms\n",
                list.size(), (long long)ng, (long long)reads, (long long)events, (long long)cols, ms_path, ms_col);
    return FIG_OK;
}

extern "C" int fig_fill_gaps(fig_ctx *ctx, const fig_gap_batch *batch, fig_gap_results *out) { return fig_fill_gaps_once(ctx, batch, out); }

extern "C" int fig_get_stats(const fig_ctx *ctx, fig_stats *out) {
    if (!ctx || !out) return FIG_EINVAL;
    *out = ctx->stats;
    return FIG_OK;
}
