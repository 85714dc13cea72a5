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

// ------------------------------------------------------------------------------------- kernel
#ifdef FIG_PROF
#define FIG_PROF_BEGIN() const unsigned long long _k0 = __builtin_readcyclecounter()
#define FIG_PROF_FLUSH() do { if (E.lane == 0) { atomicAdd(&B.counters[30], E.wait_cycles); atomicAdd(&B.counters[31], (unsigned long long)__builtin_readcyclecounter() - _k0); \
    for (int i = 0; i < 22; i++) if (E.prof[i]) atomicAdd(&B.counters[8 + i], E.prof[i]); \
    for (int i = 22; i < 40; i++) if (E.prof[i]) atomicAdd(&B.counters[32 + (i - 22)], E.prof[i]); } } while (0)
#else
#define FIG_PROF_BEGIN() ((void)0)
#define FIG_PROF_FLUSH() ((void)0)
#endif

// What depends on the launch (thread identity, the workgroup's slab); the LDS / slab layout is fig_eng_carve (fig_engine.h).
FIG_D void fig_eng_init(FigEng &E, const FigDevModel &M, const FigDevBatch &B, const FigKernArgs &A, bool lds_tab, FigScr &work) {
    E.tid = threadIdx.x; E.nt = blockDim.x;
    E.lane = threadIdx.x & 63; E.wave = threadIdx.x >> 6; E.nw = (blockDim.x + 63) >> 6; E.wsz = 64;
    E.M = &M; E.B = &B;
    E.flops = 0; E.mle_alg = 0; E.mle_exec = 0; E.wait_cycles = 0;
    for (int i = 0; i < 40; i++) E.prof[i] = 0;
    unsigned char *slab = B.scratch + (long long)blockIdx.x * B.scratch_stride;
    fig_scratch_layout(slab, B.capG, B.capR, B.capP, B.capC, B.capW, B.capE, &work);
    E.scr = work;
    fig_eng_carve(E, M, A, lds_tab);
}

FIG_D void fig_persist_of(const FigDevBatch &B, const FigDevGap &g, FigPersist &P) {
    fig_persist_layout(B.persist + g.persistOff, g.capGg, g.nU, g.nP, g.rangeCap, g.nslots, sizeof(FigState), &P);
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

// Epilogue: algorithmic flops, and the MLE-pass accounting (raw totals incl. discarded speculation; only their ratio is
// reported): [3] credited, [4] executed
FIG_D void fig_kernel_flush(const FigEng &E, const FigDevBatch &B) {
    if (E.flops) atomicAdd(&B.counters[1], E.flops);
    if (E.mle_alg) atomicAdd(&B.counters[3], E.mle_alg);
    if (E.lane == 0 && E.mle_exec) atomicAdd(&B.counters[4], E.mle_exec);
}

// ---- sequential mode: whole gaps, one workgroup each (FIG_SCHED=seq)
template <bool LDS_TAB, int NT>
__global__ void __launch_bounds__(NT, (NT <= 256 ? 2 : 1)) fig_fill_kernel(FigDevModel M, FigDevBatch B, FigKernArgs A) {
    FigEng E; FigScr work;
    fig_kernel_begin(E, M, B, A, LDS_TAB, work);
    FIG_PROF_BEGIN();
    while (true) {
        const int qi = A.q_begin + fig_queue_pop(E, B, A);
        if (qi >= A.q_end) break;
        E.g = &B.gaps[B.order[qi]];
        FigPersist P; fig_persist_of(B, *E.g, P);
        fig_bind(E, work, P, FIG_BIND_SEQ, 0, E.g->capGg);
        fig_fill_gap<LDS_TAB>(E);
    }
    FIG_PROF_FLUSH();
    fig_kernel_flush(E, B);
}

// ---- candidate-parallel mode, kernel 1: setup + analyzeGap + checkGapReads per gap; skipped gaps finish here
template <bool LDS_TAB, int NT>
__global__ void __launch_bounds__(NT, (NT <= 256 ? 2 : 1)) fig_begin_kernel(FigDevModel M, FigDevBatch B, FigKernArgs A) {
    FigEng E; FigScr work;
    fig_kernel_begin(E, M, B, A, LDS_TAB, work);
    while (true) {
        const int qi = A.q_begin + fig_queue_pop(E, B, A);
        if (qi >= A.q_end) break;
        int gi = B.order[qi];
        E.g = &B.gaps[gi];
        FigPersist P; fig_persist_of(B, *E.g, P);
        fig_bind(E, work, P, FIG_BIND_SEQ, 0, E.g->capGg);
        fig_gap_begin<LDS_TAB>(E);
        if (!E.S->L.inr) {                               // not filled (:6227): one pass without EM, then output
            while (!E.S->L.done) { fig_eval_candidate<LDS_TAB>(E); fig_loop_step(E); }
            fig_gap_end<LDS_TAB>(E);
            if (E.tid == 0) { B.gapctl[gi * 4] = 0; }
        } else {
            fig_state_save(E, P);
            if (E.tid == 0) { B.gapctl[gi * 4] = E.S->L.done ? 2 : 1; B.gapctl[gi * 4 + 1] = E.S->L.j; B.gapctl[gi * 4 + 2] = E.S->L.range; }
        }
        __syncthreads();
    }
    fig_kernel_flush(E, B);
}

// ---- pre-pass (partial mode): per gap, does its candidate loop get to Figbird.cpp:6317?  -> gapctl[gi*4+3]
template <bool LDS_TAB, int NT>
__global__ void __launch_bounds__(NT, (NT <= 256 ? 2 : 1)) fig_probe_kernel(FigDevModel M, FigDevBatch B, FigKernArgs A) {
    FigEng E; FigScr work;
    fig_kernel_begin(E, M, B, A, LDS_TAB, work);
    while (true) {
        const int qi = A.q_begin + fig_queue_pop(E, B, A);
        if (qi >= A.q_end) break;
        int gi = B.order[qi];
        E.g = &B.gaps[gi];
        FigPersist P; fig_persist_of(B, *E.g, P);
        fig_bind(E, work, P, FIG_BIND_SEQ, 0, E.g->capGg);
        const int reach = fig_gap_probe<LDS_TAB>(E);
        if (E.tid == 0) B.gapctl[gi * 4 + 3] = reach;
        __syncthreads();
    }
}

// ---- kernel 2: speculative candidate evaluations; items = {gap, candidate index j, slot, -}
template <bool LDS_TAB, int NT>
__global__ void __launch_bounds__(NT, (NT <= 256 ? 2 : 1)) fig_eval_kernel(FigDevModel M, FigDevBatch B, FigKernArgs A, const int4 *items, int n_items) {
    FigEng E; FigScr work;
    fig_kernel_begin(E, M, B, A, LDS_TAB, work);
    FIG_PROF_BEGIN();
    while (true) {
        const int qi = fig_queue_pop(E, B, A);
        if (qi >= n_items) break;
        int4 it = items[qi];
        E.g = &B.gaps[it.x];
        FigPersist P; fig_persist_of(B, *E.g, P);
        fig_spec_eval<LDS_TAB>(E, work, P, it.y, it.z, E.g->capGg);
        __syncthreads();
    }
    FIG_PROF_FLUSH();
    fig_kernel_flush(E, B);
}

// ---- kernel 3: replay the bookkeeping of the speculated candidates in order; entries = {gap, n slots, -, -}
// One wave, no class: it touches FigState alone, and its launch asks for no more LDS than that.  fig_eng_carve would place gs /
// rb / plb behind FigState, outside that request, so this kernel keeps them null (a stray use faults instead of corrupting).
__global__ void __launch_bounds__(64) fig_replay_kernel(FigDevModel M, FigDevBatch B, const int4 *entries, int n) {
    if ((int)blockIdx.x >= n) return;
    FigEng E; FigScr work;
    memset(&work, 0, sizeof(work));
    E.tid = threadIdx.x; E.nt = blockDim.x; E.lane = threadIdx.x & 63; E.wave = 0; E.nw = 1; E.wsz = 64;
    E.M = &M; E.B = &B; E.capG = 0; E.flops = 0; E.mle_alg = 0; E.mle_exec = 0; E.wait_cycles = 0; E.ncolE = 0; E.xoff = 0; E.Wcap = 0; E.nteams = 1; E.sh_on = 0;
    E.pq = nullptr; E.q4 = nullptr; E.wbuf = nullptr; E.gs = nullptr; E.rb = nullptr; E.plb = nullptr; E.off_plb = 0; E.pq_lds = 0; E.w_lds = 0;
    E.off_pq = E.off_q4 = E.off_w = 0; E.tiles = E.tile_step = E.tile_cols = 0; E.lds_tw = 0;
    E.S = (FigState *)fig_lds;
    int4 en = entries[blockIdx.x];
    E.g = &B.gaps[en.x];
    FigPersist P; fig_persist_of(B, *E.g, P);
    fig_spec_replay(E, work, P, en.y, E.g->capGg);
    if (E.tid == 0) { B.gapctl[en.x * 4] = E.S->L.done ? 2 : 1; B.gapctl[en.x * 4 + 1] = E.S->L.j; B.gapctl[en.x * 4 + 2] = E.S->L.range; }
}

// ---- kernel 4: fallbacks + finalize + output for the gaps whose loop is done; list = gap ids
template <bool LDS_TAB, int NT>
__global__ void __launch_bounds__(NT, (NT <= 256 ? 2 : 1)) fig_end_kernel(FigDevModel M, FigDevBatch B, FigKernArgs A, const int *list, int n) {
    FigEng E; FigScr work;
    fig_kernel_begin(E, M, B, A, LDS_TAB, work);
    while (true) {
        const int qi = fig_queue_pop(E, B, A);
        if (qi >= n) break;
        int gi = list[qi];
        E.g = &B.gaps[gi];
        FigPersist P; fig_persist_of(B, *E.g, P);
        fig_bind(E, work, P, FIG_BIND_SEQ, 0, E.g->capGg);
        fig_state_load(E, P);
        fig_gap_end<LDS_TAB>(E);
        if (E.tid == 0) B.gapctl[gi * 4] = 0;
        __syncthreads();
    }
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

struct DevBuf {
    void *p = nullptr; size_t n = 0;
};

// Per-class scheduling lane: the classes of a batch run concurrently, each on its own stream with its own work
// queue head, scratch slabs and item buffers, so that the tail of one class's round is filled by the other
// classes' workgroups.
struct FigLane { hipStream_t stream = nullptr; hipEvent_t done = nullptr; int32_t *queue_head = nullptr; uint8_t *scratch = nullptr; int *d_items = nullptr, *d_entries = nullptr; size_t cap = 0;
                 int32_t *h_ctl = nullptr; int *h_items = nullptr, *h_entries = nullptr; int qsel = 0; };   // h_*: pinned, so the copies run on the DMA engines and never wait for a CU

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
    // resident batch
    bool have_batch = false;
    FigDevBatch db;
    std::vector<FigDevGap> h_gaps;
    std::vector<int32_t> h_order;
    struct Cls { FigLaunchClass c; int blocks; int capacity; };
    std::vector<Cls> classes;
    std::vector<DevBuf> bufs;
    int64_t n_gaps = 0, n_ureads = 0, n_preads = 0, str_total = 0;
    std::vector<int64_t> h_str_off;
    int nslots = 32;
    std::vector<FigLane> lanes;
    fig_stats stats;
    int sh_on = FIG_SH_SC;            // FIG_ESTEP / FIG_SH_CHUNKS, read once at fig_ctx_create
    std::vector<uint8_t> h_ot;        // host copy of db.ot_preset
    uint8_t *d_ot = nullptr;
};

static int dev_alloc(fig_ctx *ctx, size_t bytes, void **out) {
    DevBuf b;
    if (bytes == 0) bytes = 8;
    hipError_t e = hipMalloc(&b.p, bytes);
    if (e != hipSuccess) { ctx->last_hip = (int)e; return FIG_ENOMEM; }
    b.n = bytes;
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
static hipError_t launch_kind(fig_ctx *ctx, const fig_ctx::Cls &c, const FigDevBatch &db, hipStream_t stream, FigKind kind, int blocks, const void *list, int n, int qsel) {
    const FigKernArgs A = fig_kargs_of(c.c, qsel, ctx->sh_on);
    switch (kind) {
        case FIG_K_FILL: return launch_one(fig_fill_kernel<LDS_TAB, NT>, c.c.lds, NT, blocks, stream, ctx->dm, db, A);
        case FIG_K_BEGIN: return launch_one(fig_begin_kernel<LDS_TAB, NT>, c.c.lds, NT, blocks, stream, ctx->dm, db, A);
        case FIG_K_PROBE: return launch_one(fig_probe_kernel<LDS_TAB, NT>, c.c.lds, NT, blocks, stream, ctx->dm, db, A);
        case FIG_K_EVAL: return launch_one(fig_eval_kernel<LDS_TAB, NT>, c.c.lds, NT, blocks, stream, ctx->dm, db, A, (const int4 *)list, n);
        case FIG_K_END: return launch_one(fig_end_kernel<LDS_TAB, NT>, c.c.lds, NT, blocks, stream, ctx->dm, db, A, (const int *)list, n);
    }
    return hipErrorInvalidValue;
}

static hipError_t launch_any(fig_ctx *ctx, const fig_ctx::Cls &c, const FigDevBatch &db, hipStream_t stream, FigKind kind, int blocks, const void *list, int n, int qsel = 0) {
    if (c.c.tiles > 0) return launch_kind<true, 512>(ctx, c, db, stream, kind, blocks, list, n, qsel);      // LDS-tiled: the LDS code path with a streamed table
    if (c.c.lds_tab) return c.c.nt == 256 ? launch_kind<true, 256>(ctx, c, db, stream, kind, blocks, list, n, qsel) : launch_kind<true, 512>(ctx, c, db, stream, kind, blocks, list, n, qsel);
    return launch_kind<false, 512>(ctx, c, db, stream, kind, blocks, list, n, qsel);
}

extern "C" int fig_batch_upload(fig_ctx *ctx, const fig_gap_batch *b) {
    if (!ctx || !b) return FIG_EINVAL;
    if (!ctx->have_model) return FIG_EINVAL;
    hipSetDevice(ctx->device);
    free_batch(ctx);
    const fig_model *m = &ctx->hm;
    hipEventRecord(ctx->ev0, ctx->stream);
    FigPacked K;
    int prc = fig_pack(m, b, sizeof(FigState), K);
    if (prc) return prc;
    int64_t ng = K.n_gaps;
    ctx->h_gaps = K.gaps; ctx->h_order = K.order; ctx->h_str_off = K.str_off;
    ctx->str_total = K.str_total; ctx->n_gaps = ng;
    ctx->n_ureads = (int64_t)K.u_pos.size(); ctx->n_preads = (int64_t)K.p_pos.size();
    ctx->classes.clear();
    const bool log = fig_knobs_from_env(0).log;
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
    int capG_s = K.capG, capR = K.capR, capP = K.capP, capC = K.capC;
    int64_t str_total = K.str_total;
    int64_t stride = fig_scratch_layout(nullptr, capG_s, capR, capP, capC, K.capW, K.capE, nullptr);
    stride = (stride + 255) & ~255LL;
    std::vector<FigDevGap> &gaps = K.gaps; std::vector<int32_t> &order = K.order;
    std::vector<uint32_t> &packed = K.packed; std::vector<uint8_t> &qual = K.qual, &flank = K.flank;
    std::vector<int32_t> &u_pos = K.u_pos, &u_aux = K.u_aux, &u_len = K.u_len, &p_pos = K.p_pos, &p_aux = K.p_aux, &p_clip = K.p_clip, &p_ref = K.p_ref, &p_len = K.p_len;
    std::vector<int64_t> &u_woff = K.u_woff, &p_woff = K.p_woff, &p_qoff = K.p_qoff;

    // ---- upload
    FigDevBatch &db = ctx->db;
    memset(&db, 0, sizeof(db));
    db.n_gaps = ng;
    int rc;
#define UP(vec, field) do { rc = dev_upload(ctx, vec, &db.field); if (rc) return rc; } while (0)
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
    if ((rc = dev_alloc(ctx, (size_t)str_total, &p))) return rc; db.str = (char *)p;
    if ((rc = dev_alloc(ctx, 64 * (ctx->classes.size() + 1), &p))) return rc; db.queue_head = (int32_t *)p;
    if ((rc = dev_alloc(ctx, 512, &p))) return rc; db.counters = (unsigned long long *)p;
    size_t total_blocks = 0;
    for (const fig_ctx::Cls &c : ctx->classes) total_blocks += (size_t)c.capacity;
    if ((rc = dev_alloc(ctx, (size_t)stride * std::max<size_t>(total_blocks, 1), &p))) return rc; db.scratch = (uint8_t *)p;
    if ((rc = dev_alloc(ctx, (size_t)K.persist_total + 256, &p))) return rc; db.persist = (uint8_t *)p;
    if ((rc = dev_alloc(ctx, (size_t)std::max<int64_t>(ng, 1) * 16, &p))) return rc; db.gapctl = (int32_t *)p;
    if ((rc = dev_alloc(ctx, (size_t)std::max<int64_t>(ng, 1), &p))) return rc; ctx->d_ot = (uint8_t *)p; db.ot_preset = ctx->d_ot;
    ctx->h_ot = K.ot_preset;
    FIG_HIP(hipMemcpyAsync(ctx->d_ot, ctx->h_ot.data(), (size_t)std::max<int64_t>(ng, 1), hipMemcpyHostToDevice, ctx->stream));
    ctx->nslots = K.nslots;
    {   size_t blk = 0;
        for (size_t ci = 0; ci < ctx->classes.size(); ci++) {
            const fig_ctx::Cls &c = ctx->classes[ci];
            ctx->lanes.push_back(FigLane());          // pushed first: free_batch reclaims whatever was created when a later step fails
            FigLane &l = ctx->lanes.back();
            if (hipStreamCreate(&l.stream) != hipSuccess || hipEventCreateWithFlags(&l.done, hipEventDisableTiming) != hipSuccess) return FIG_EHIP;
            l.queue_head = db.queue_head + 16 * (ci + 1);
            l.scratch = db.scratch + (size_t)stride * blk; blk += (size_t)c.capacity;
            l.cap = (size_t)std::max(c.c.q_end - c.c.q_begin, 1) * 4 * (size_t)(K.nslots + 1);
            if ((rc = dev_alloc(ctx, l.cap * 4, &p))) return rc; l.d_items = (int *)p;
            if ((rc = dev_alloc(ctx, l.cap * 4, &p))) return rc; l.d_entries = (int *)p;
            if (hipHostMalloc((void **)&l.h_ctl, (size_t)std::max<int64_t>(ng, 1) * 16, hipHostMallocDefault) != hipSuccess) return FIG_ENOMEM;
            if (hipHostMalloc((void **)&l.h_items, l.cap * 4, hipHostMallocDefault) != hipSuccess) return FIG_ENOMEM;
            if (hipHostMalloc((void **)&l.h_entries, l.cap * 4, hipHostMallocDefault) != hipSuccess) return FIG_ENOMEM;
        }
    }
    db.scratch_stride = stride;
    db.capG = capG_s; db.capR = capR; db.capP = capP; db.capC = capC; db.capW = K.capW; db.capE = K.capE;
    db.n_ureads = ctx->n_ureads;
    FIG_HIP(hipMemsetAsync(db.counters, 0, 512, ctx->stream));
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
    FIG_HIP(hipMemsetAsync(db.gapctl, 0, (size_t)ng * 16, ctx->stream));
    for (const fig_ctx::Cls &c : ctx->classes) {
        FIG_HIP(hipMemsetAsync(db.queue_head, 0, 8, ctx->stream));
        FIG_HIP(launch_any(ctx, c, db, ctx->stream, FIG_K_PROBE, c.blocks, nullptr, 0));
    }
    std::vector<int32_t> ctl((size_t)ng * 4);
    FIG_HIP(hipMemcpyAsync(ctl.data(), db.gapctl, (size_t)ng * 16, hipMemcpyDeviceToHost, ctx->stream));
    FIG_HIP(hipStreamSynchronize(ctx->stream));
    for (int64_t g = 0; g < ng; g++) reach[g] = ctl[(size_t)g * 4 + 3] ? 1 : 0;
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
    hipStream_t stream = ln.stream;
    hipSetDevice(ctx->device);
    int nl = 0;
    hipError_t e;
    auto fail = [&](hipError_t er) { ctx->last_hip = (int)er; return -1; };
    const int capacity = std::max(1, c.capacity);      // workgroups the device holds for this class (not capped by the gap count)
    // every persistent launch pops from one of the lane's two queue heads and zeroes the other for its successor
    auto launch = [&](FigKind kind, int n_work, const void *list) {
        hipError_t er = launch_any(ctx, c, db, stream, kind, std::min(capacity, n_work), list, n_work, ln.qsel);
        ln.qsel ^= 1; nl++;
        return er;
    };
    if ((e = launch(FIG_K_BEGIN, c.c.q_end - c.c.q_begin, nullptr)) != hipSuccess) return fail(e);
    int32_t *ctl = ln.h_ctl;
    const size_t ctl_n = (size_t)ctx->n_gaps * 4;
    const std::vector<int> ids(ctx->h_order.begin() + c.c.q_begin, ctx->h_order.begin() + c.c.q_end);   // cost-sorted
    FigRound R;
    auto now = [] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    const double t_start = now();
    double t_prev = now(); int round = 0, last_items = 0, last_active = 0, last_chunk = 0, n_active_max = 0;
    while (true) {
        if ((e = hipMemcpyAsync(ctl, db.gapctl, ctl_n * 4, hipMemcpyDeviceToHost, stream)) != hipSuccess) return fail(e);
        if ((e = hipStreamSynchronize(stream)) != hipSuccess) return fail(e);
        fig_plan_round(ids, ctl, capacity, c.c.nsplit, ctx->nslots, knobs.minc, knobs.ipw, n_active_max, R);
        if (knobs.log) { double t = now(); fprintf(stderr, "[figsched] capG=%d round %d: active=%d chunk=%d items=%d blocks=%d  %.1f ms\n", c.c.capG, round, last_active, last_chunk, last_items, capacity, t - t_prev); t_prev = t; }
        round++;
        if (R.n_active == 0) break;
        if (ln.cap < R.items.size() || ln.cap < R.entries.size()) return fail(hipErrorOutOfMemory);
        const int n_items = (int)(R.items.size() / 4), n_ent = (int)(R.entries.size() / 4);
        last_items = n_items; last_active = R.n_active; last_chunk = R.chunk;
        if (n_items > 0) {
            memcpy(ln.h_items, R.items.data(), R.items.size() * 4);
            if ((e = hipMemcpyAsync(ln.d_items, ln.h_items, R.items.size() * 4, hipMemcpyHostToDevice, stream)) != hipSuccess) return fail(e);
            if ((e = launch(FIG_K_EVAL, n_items, ln.d_items)) != hipSuccess) return fail(e);
        }
        memcpy(ln.h_entries, R.entries.data(), R.entries.size() * 4);
        if ((e = hipMemcpyAsync(ln.d_entries, ln.h_entries, R.entries.size() * 4, hipMemcpyHostToDevice, stream)) != hipSuccess) return fail(e);
        hipLaunchKernelGGL(fig_replay_kernel, dim3(n_ent), dim3(64), sizeof(FigState) + 64, stream, ctx->dm, db, (const int4 *)ln.d_entries, n_ent);
        if ((e = hipGetLastError()) != hipSuccess) return fail(e);
        nl++;
    }
    std::vector<int> endlist;
    for (int g : ids) if (ctl[(size_t)g * 4] == 2) endlist.push_back(g);
    if (!endlist.empty()) {
        if ((e = hipStreamSynchronize(stream)) != hipSuccess) return fail(e);      // h_items is reused: the last round's upload must have left it
        memcpy(ln.h_items, endlist.data(), endlist.size() * 4);
        if ((e = hipMemcpyAsync(ln.d_items, ln.h_items, endlist.size() * 4, hipMemcpyHostToDevice, stream)) != hipSuccess) return fail(e);
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
    // optional debug / draw planes live in per-call device buffers
    std::vector<void *> tmp;
    auto talloc = [&](size_t n, void **p) -> int { if (hipMalloc(p, n ? n : 8) != hipSuccess) return FIG_ENOMEM; tmp.push_back(*p); return FIG_OK; };
    auto tfree = [&]() { for (void *p : tmp) hipFree(p); };
    fig_batch_clear_planes(db);
    void *p;
    if (out->dbg_n_cand && out->dbg_cand_i && out->dbg_cand_lik && out->dbg_max_cand > 0) {
        db.dbg_max_cand = out->dbg_max_cand;
        if (talloc((size_t)ng * 4, &p)) { tfree(); return FIG_ENOMEM; } db.dbg_n_cand = (int32_t *)p;
        if (talloc((size_t)ng * out->dbg_max_cand * 12, &p)) { tfree(); return FIG_ENOMEM; } db.dbg_cand_i = (int32_t *)p;
        if (talloc((size_t)ng * out->dbg_max_cand * 8, &p)) { tfree(); return FIG_ENOMEM; } db.dbg_cand_lik = (double *)p;
        hipMemsetAsync(db.dbg_n_cand, 0, (size_t)ng * 4, ctx->stream);
        if (out->dbg_n_place) { if (talloc((size_t)ng * 4, &p)) { tfree(); return FIG_ENOMEM; } db.dbg_n_place = (int32_t *)p; hipMemsetAsync(db.dbg_n_place, 0, (size_t)ng * 4, ctx->stream); }
        if (out->dbg_counts && out->dbg_plane_cols > 0) {
            const size_t n = (size_t)ng * out->dbg_max_cand * out->dbg_plane_cols * 5 * 8;
            if (talloc(n, &p)) { tfree(); return FIG_ENOMEM; } db.dbg_counts = (double *)p; db.dbg_plane_cols = out->dbg_plane_cols;
            hipMemsetAsync(db.dbg_counts, 0, n, ctx->stream);
        }
        if (out->dbg_read_maxlv && out->dbg_plane_reads > 0) {
            const size_t n = (size_t)ng * out->dbg_max_cand * out->dbg_plane_reads * 8;
            if (talloc(n, &p)) { tfree(); return FIG_ENOMEM; } db.dbg_read_maxlv = (double *)p; db.dbg_plane_reads = out->dbg_plane_reads;
            hipMemsetAsync(db.dbg_read_maxlv, 0, n, ctx->stream);
        }
    }
    int64_t nr = ctx->n_ureads + ctx->n_preads;
    if (out->draw_pos && out->draw_isz && out->draw_len) {
        if (talloc((size_t)nr * 4, &p)) { tfree(); return FIG_ENOMEM; } db.draw_pos = (int32_t *)p;
        if (talloc((size_t)nr * 4, &p)) { tfree(); return FIG_ENOMEM; } db.draw_isz = (int32_t *)p;
        if (talloc((size_t)ng * 8, &p)) { tfree(); return FIG_ENOMEM; } db.draw_len = (int32_t *)p;
        hipMemsetAsync(db.draw_isz, 0, (size_t)nr * 4, ctx->stream);
    }
    const size_t sup_n = (size_t)ctx->str_total * 5;
    if (sup) {                        // per-base read support: one slot per string slot, zero unless fig_gap_end writes it
        if (talloc(sup_n * 4, &p)) { tfree(); return FIG_ENOMEM; } db.sup_counts = (int32_t *)p;
        if (talloc((size_t)ng * 4, &p)) { tfree(); return FIG_ENOMEM; } db.sup_origin = (int32_t *)p;
        hipMemsetAsync(db.sup_counts, 0, sup_n * 4, ctx->stream);
        hipMemsetAsync(db.sup_origin, 0, (size_t)ng * 4, ctx->stream);
    }
    hipMemsetAsync(db.counters, 0, 512, ctx->stream);
    // a previous call that failed half-way may have left queue heads / ping-pong selectors inconsistent: start clean
    hipMemsetAsync(db.queue_head, 0, 64 * (ctx->classes.size() + 1), ctx->stream);
    for (auto &l : ctx->lanes) l.qsel = 0;
    hipMemsetAsync(db.filled_len, 0, (size_t)std::max<int64_t>(ng, 1) * 4, ctx->stream);
    hipMemsetAsync(db.gaptofill, 0, (size_t)std::max<int64_t>(ng, 1) * 4, ctx->stream);
    hipMemsetAsync(db.str, 'N', (size_t)ctx->str_total, ctx->stream);
    hipMemsetAsync(db.gapctl, 0, (size_t)std::max<int64_t>(ng, 1) * 16, ctx->stream);
    hipEventRecord(ctx->ev0, ctx->stream);
    int nl = 0;
    const FigKnobs knobs = fig_knobs_from_env(ctx->dm.unmapped);      // read here, on the caller's thread: the lane threads only get the values
    if (knobs.seq) {
        for (size_t ci = 0; ci < ctx->classes.size(); ci++) {
            const fig_ctx::Cls &c = ctx->classes[ci];
            hipMemsetAsync(db.queue_head, 0, 4, ctx->stream);
            hipError_t e = launch_any(ctx, c, db, ctx->stream, FIG_K_FILL, c.blocks, nullptr, 0);
            if (e != hipSuccess) { ctx->last_hip = (int)e; tfree(); return FIG_EHIP; }
            nl++;
        }
    } else {
        // one host thread + stream per class; every lane starts after ev0 and the main stream joins them before ev1
        const size_t nc = ctx->classes.size();
        std::vector<int> rcs(nc, 0);
        ctx->db = db;
        for (size_t ci = 0; ci < nc; ci++) hipStreamWaitEvent(ctx->lanes[ci].stream, ctx->ev0, 0);
        if (nc <= 1 || knobs.lanes_serial) {
            for (size_t ci = 0; ci < nc; ci++) rcs[ci] = run_class_parallel(ctx, ctx->classes[ci], ctx->lanes[ci], knobs);
        } else {
            std::vector<std::thread> th;
            for (size_t ci = 0; ci < nc; ci++) th.emplace_back([&, ci] { rcs[ci] = run_class_parallel(ctx, ctx->classes[ci], ctx->lanes[ci], knobs); });
            for (auto &t : th) t.join();
        }
        for (size_t ci = 0; ci < nc; ci++) {
            if (rcs[ci] < 0) { hipDeviceSynchronize(); tfree(); return FIG_EHIP; }
            nl += rcs[ci];
            hipEventRecord(ctx->lanes[ci].done, ctx->lanes[ci].stream);
            hipStreamWaitEvent(ctx->stream, ctx->lanes[ci].done, 0);
        }
    }
    hipEventRecord(ctx->ev1, ctx->stream);
    hipError_t e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) { ctx->last_hip = (int)e; tfree(); return FIG_EHIP; }
    float ms = 0; hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1);
    ctx->stats.kernel_ms = ms; ctx->stats.n_launches = nl;
    // ---- results back
    hipEventRecord(ctx->ev0, ctx->stream);
    std::vector<char> hstr((size_t)ctx->str_total);
    hipMemcpyAsync(out->filled_len, db.filled_len, (size_t)ng * 4, hipMemcpyDeviceToHost, ctx->stream);
    hipMemcpyAsync(out->gaptofill, db.gaptofill, (size_t)ng * 4, hipMemcpyDeviceToHost, ctx->stream);
    if (ctx->str_total) hipMemcpyAsync(hstr.data(), db.str, (size_t)ctx->str_total, hipMemcpyDeviceToHost, ctx->stream);
    unsigned long long cnt[64] = {0};
    hipMemcpyAsync(cnt, db.counters, 512, hipMemcpyDeviceToHost, ctx->stream);
    if (db.dbg_n_cand) {
        hipMemcpyAsync(out->dbg_n_cand, db.dbg_n_cand, (size_t)ng * 4, hipMemcpyDeviceToHost, ctx->stream);
        hipMemcpyAsync(out->dbg_cand_i, db.dbg_cand_i, (size_t)ng * out->dbg_max_cand * 12, hipMemcpyDeviceToHost, ctx->stream);
        hipMemcpyAsync(out->dbg_cand_lik, db.dbg_cand_lik, (size_t)ng * out->dbg_max_cand * 8, hipMemcpyDeviceToHost, ctx->stream);
        if (db.dbg_n_place) hipMemcpyAsync(out->dbg_n_place, db.dbg_n_place, (size_t)ng * 4, hipMemcpyDeviceToHost, ctx->stream);
        if (db.dbg_counts) hipMemcpyAsync(out->dbg_counts, db.dbg_counts, (size_t)ng * out->dbg_max_cand * out->dbg_plane_cols * 5 * 8, hipMemcpyDeviceToHost, ctx->stream);
        if (db.dbg_read_maxlv) hipMemcpyAsync(out->dbg_read_maxlv, db.dbg_read_maxlv, (size_t)ng * out->dbg_max_cand * out->dbg_plane_reads * 8, hipMemcpyDeviceToHost, ctx->stream);
    }
    if (db.draw_pos) {
        hipMemcpyAsync(out->draw_pos, db.draw_pos, (size_t)nr * 4, hipMemcpyDeviceToHost, ctx->stream);
        hipMemcpyAsync(out->draw_isz, db.draw_isz, (size_t)nr * 4, hipMemcpyDeviceToHost, ctx->stream);
        hipMemcpyAsync(out->draw_len, db.draw_len, (size_t)ng * 8, hipMemcpyDeviceToHost, ctx->stream);
    }
    std::vector<int32_t> hsup(sup ? sup_n : 0);
    if (sup) {
        if (sup_n) hipMemcpyAsync(hsup.data(), db.sup_counts, sup_n * 4, hipMemcpyDeviceToHost, ctx->stream);
        hipMemcpyAsync(sup->origin, db.sup_origin, (size_t)ng * 4, hipMemcpyDeviceToHost, ctx->stream);
    }
    hipEventRecord(ctx->ev1, ctx->stream);
    e = hipStreamSynchronize(ctx->stream);
    tfree();
    if (e != hipSuccess) { ctx->last_hip = (int)e; return FIG_EHIP; }
    hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1);
    ctx->stats.d2h_ms = ms;
#ifdef FIG_PROF
    { const char *nm[14] = {"A.wait", "B.wait", "-", "M.finish", "PR.pre", "PR.estep", "PR.mid", "PR.mle", "PR.post", "A.chain", "A.logexp", "A.work", "B.work", "M.chains"};
      for (int i = 0; i < 14; i++) fprintf(stderr, "[figprof] %-9s %8.1f Gcycles = %5.1f %% of wave-cycles\n", nm[i], cnt[8 + i] / 1e9, cnt[31] ? 100.0 * cnt[8 + i] / cnt[31] : 0.0);
      { const char *mn[4] = {"M.setup", "M.hint", "M.rounds", "M.surv"};
        for (int i = 0; i < 4; i++) fprintf(stderr, "[figprof] %-9s %8.1f Gcycles = %5.1f %% of wave-cycles\n", mn[i], cnt[22 + i] / 1e9, cnt[31] ? 100.0 * cnt[22 + i] / cnt[31] : 0.0); }
      fprintf(stderr, "[figprof] raw slots:"); for (int i = 0; i < 22; i++) fprintf(stderr, " %d:%.1f", i, cnt[8 + i] / 1e9); for (int i = 22; i < 40; i++) fprintf(stderr, " %d:%.1f", i, cnt[32 + i - 22] / 1e9); fprintf(stderr, "\n");
      fprintf(stderr, "[figprof] barrier wait %.3f of %.3f wave-Gcycles = %.1f %%\n", cnt[30] / 1e9, cnt[31] / 1e9, cnt[31] ? 100.0 * cnt[30] / cnt[31] : 0.0); }
#endif
    if (knobs.log) fprintf(stderr, "[figsched] useful flops %.4g, speculative evaluations executed %.4g (%.1f %% discarded)\n", (double)cnt[1], (double)cnt[2], cnt[2] ? 100.0 * (1.0 - ((double)cnt[1] / (double)cnt[2])) : 0.0);
    ctx->stats.place_calls = (int64_t)cnt[0];
    ctx->stats.alg_flops = (double)cnt[1];
    ctx->stats.spec_flops = (double)cnt[2];
    ctx->stats.mle_alg_flops = (double)cnt[3];
    ctx->stats.mle_exec_flops = (double)cnt[4];
    int rc = fig_compact_results(ng, hstr.data(), ctx->h_str_off.data(), out);
    if (!rc && sup) fig_compact_support(ng, hsup.data(), ctx->h_str_off.data(), out, sup->counts);
    return rc;
}

extern "C" int fig_fill_gaps(fig_ctx *ctx, const fig_gap_batch *batch, fig_gap_results *out) { return fig_fill_gaps_once(ctx, batch, out); }

extern "C" int fig_get_stats(const fig_ctx *ctx, fig_stats *out) {
    if (!ctx || !out) return FIG_EINVAL;
    *out = ctx->stats;
    return FIG_OK;
}
