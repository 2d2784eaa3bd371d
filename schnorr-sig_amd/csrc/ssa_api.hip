// C ABI (include/schnorr_sig_amd.h) over the HIP kernels in ssa_kernels.hpp.
// No CPU compute path exists here: every entry point launches kernels on the context's
// device or fails with an SSA_ERR_* code.
#define SSA_KERNELS_DEFINE 1
#include "ssa_ctx.hpp"
#include "ssa_keycache.hpp"
#include "ssa_keyed.hpp"
#include "ssa_aggregate.hpp"
#include "ssa_aggcache.hpp"
#include "ssa_aggregator.hpp"
#include "ssa_aggverifier.hpp"

#include <sys/random.h>

#include <atomic>
#include <climits>
#include <functional>
#include <initializer_list>
#include <memory>
#include <mutex>
#include <thread>

static const unsigned char k_default_params[SSA_PARAMS_LENGTH] = {
#include "../params/params_default.inc"
};

extern "C" const char *ssa_strerror(int rc) {
    switch (rc) {
        case SSA_OK: return "ok";
        case SSA_INVALID_PUBLIC_KEY: return "The public key is not an element of the prime subgroup.";
        case SSA_INVALID_SIGNATURE: return "The signature is invalid or was incorrectly computed.";
        case SSA_MALFORMED: return "malformed input (the reference would panic)";
        case SSA_ERR_ARG: return "invalid argument";
        case SSA_ERR_HIP: return "HIP runtime error";
        case SSA_ERR_PARAMS: return "invalid parameter blob";
        case SSA_ERR_NO_DEVICE: return "no HIP device";
        case SSA_ERR_TABLE: return "a precomputed table failed its self-check";
        default: return "unknown";
    }
}

extern "C" const void *ssa_default_params(void) { return k_default_params; }

extern "C" int ssa_abi_version(void) { return SSA_ABI_VERSION; }

// The comb table depends on the device, the generator and its geometry only, and it is up to 17.7 GB: contexts of one
// process share it (reference-counted; ssa_multi_create with several contexts per device, the tests' many engines, a
// binding that makes a context per thread).  Built at the first acquisition on the acquiring context's stream,
// synchronously, under the registry's lock, and checked row by row before it is handed out (ssa_selfcheck.hpp);
// read-only afterwards.  A table that fails an on-demand check (ssa_ctx_selfcheck) is RETIRED: out of the registry, so
// that no later context gets it, and freed with the last reference of the contexts that still hold it.
struct SharedGtab {
    int device = 0;
    u32 bits = 0;
    u64 gen[12] = {};
    u64 *d_gtab = nullptr;
    int refs = 0;
    int builds = 0;           // builds this table took (1; 2 when the first one failed its check)
    bool retired = false;
};
static std::mutex g_gtab_mu;
static std::vector<SharedGtab *> g_gtabs;

// The live contexts of this process per device, twins not counted: a call is split over the two streams (DESIGN.md
// section 33) only while its context is the one context of its device.  A process that keeps several there overlaps
// its calls itself, and the parts of two split calls get in each other's way (profiles/r30/README.md).
static std::mutex g_live_mu;
static std::map<int, int> g_live_ctxs;
static void live_ctxs_add(int device, int d) {
    std::lock_guard<std::mutex> lock(g_live_mu);
    g_live_ctxs[device] += d;
}
static int live_ctxs_on(int device) {
    std::lock_guard<std::mutex> lock(g_live_mu);
    return g_live_ctxs[device];
}

static inline size_t gtab_bytes(u32 bits) { return gtab_entries(bits) * 12 * sizeof(u64); }

// ssa_debug_corrupt_table_builds: the next n comb builds of the process get one word flipped before their check
static std::atomic<int> g_corrupt_builds{0};

static int debug_corrupt_build(ssa_ctx *ctx, SharedGtab *g) {
    int n = g_corrupt_builds.load();
    while (n > 0 && !g_corrupt_builds.compare_exchange_weak(n, n - 1)) {
    }
    if (n <= 0) return 0;
    // a mid-table row (window count / 2, digit 12345 -- never the header row), word 7 (y, limb 1)
    u64 *p = g->d_gtab + 12 * (((size_t)(gtab_windows(g->bits) / 2) << g->bits) + 12345) + 7, v = 0;
    HIP_TRY(hipMemcpyAsync(&v, p, sizeof v, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    v ^= 1ull << 17;
    HIP_TRY(hipMemcpyAsync(p, &v, sizeof v, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return 0;
}

// the table of `bits`-bit windows for this generator on this device: an existing one, or a new one (nullptr: no memory,
// or -- *bad_table set -- a table that failed its check twice)
static SharedGtab *gtab_acquire(ssa_ctx *ctx, const DevParams &hp, u32 bits, bool *bad_table) {
    std::lock_guard<std::mutex> lock(g_gtab_mu);
    u64 gen[12];
    for (int i = 0; i < 6; i++) {
        gen[i] = hp.gen_x[i];
        gen[6 + i] = hp.gen_y[i];
    }
    for (SharedGtab *g : g_gtabs)
        if (g->device == ctx->device && g->bits == bits && std::memcmp(g->gen, gen, sizeof gen) == 0) {
            g->refs++;
            return g;
        }
    SharedGtab *g = new SharedGtab();
    g->device = ctx->device;
    g->bits = bits;
    std::memcpy(g->gen, gen, sizeof gen);
    // base entries by double-and-add (90 112 of them for 24-bit windows), then one affine addition per entry
    // (ssa_kernels.hpp)
    void *gbase = nullptr;
    bool ok = hipMalloc((void **)&g->d_gtab, gtab_bytes(bits)) == hipSuccess &&
              hipMalloc(&gbase, gbase_entries(bits) * 12 * sizeof(u64)) == hipSuccess;
    if (ok) {
        // every row is checked before the table is handed out: a table that fails is rebuilt once in the same
        // allocation, then given up (the caller moves on to the next smaller width)
        bool clean = false;
        for (int b = 0; b < 2 && ok && !clean; b++) {
            hipLaunchKernelGGL(ssa_k_gbase, dim3(grid_for(gbase_entries(bits), 256)), dim3(256), 0, ctx->stream,
                               ctx->d_params, (u64 *)gbase, bits);
            hipLaunchKernelGGL(ssa_k_gtable, dim3(grid_for(gtab_entries(bits) / 8, 256)), dim3(256), 0, ctx->stream,
                               (const u64 *)gbase, g->d_gtab, bits);
            g->builds++;
            ok = hipGetLastError() == hipSuccess && hipStreamSynchronize(ctx->stream) == hipSuccess &&
                 debug_corrupt_build(ctx, g) == 0;
            uint64_t res[2] = {0, 0};
            ok = ok && ssa_internal_gtab_check(ctx, g->d_gtab, bits, res) == 0;
            clean = ok && res[0] == 0;
        }
        if (ok && !clean) {
            *bad_table = true;
            ok = false;
        }
    } else {
        (void)hipGetLastError();      // an allocation that did not fit is not a sticky error: the caller tries a smaller table
    }
    if (gbase) (void)hipFree(gbase);
    if (!ok) {
        if (g->d_gtab) (void)hipFree(g->d_gtab);
        delete g;
        return nullptr;
    }
    g->refs = 1;
    g_gtabs.push_back(g);
    return g;
}

// (a retired table is no longer in the registry: the search finds nothing, the table is freed all the same)
static void gtab_release(SharedGtab *g) {
    if (!g) return;
    std::lock_guard<std::mutex> lock(g_gtab_mu);
    if (--g->refs > 0) return;
    forget_handle(g_gtabs, g);
    (void)hipSetDevice(g->device);
    (void)hipFree(g->d_gtab);
    delete g;
}

static int validate_params(const DevParams &p) {
    if (std::memcmp(p.magic, "SSAPARM1", 8) != 0) return SSA_ERR_PARAMS;
    if (p.n_rounds == 0 || p.n_rounds > 8) return SSA_ERR_PARAMS;
    if (p.rate_off != 0 && p.rate_off != 4) return SSA_ERR_PARAMS;
    if (p.cap_len_idx < -1 || p.cap_len_idx > 11) return SSA_ERR_PARAMS;
    if (p.pad_mode > 1 || p.digest_off > 8) return SSA_ERR_PARAMS;
    for (int i = 0; i < 144; i++)
        if (p.mds[i] >= FP_P) return SSA_ERR_PARAMS;
    for (int i = 0; i < 96; i++)
        if (p.ark1[i] >= FP_P || p.ark2[i] >= FP_P) return SSA_ERR_PARAMS;
    for (int i = 0; i < 6; i++)
        if (p.gen_x[i] >= FP_P || p.gen_y[i] >= FP_P) return SSA_ERR_PARAMS;
    return 0;
}

// A variable of the environment into a knob, if it is set and its value passes the knob's rule (true; otherwise the
// knob keeps what it has): a number in [lo, hi] -- read with strtoull, or with atoi where the rule is on an int --, one
// of a set, or a boolean (non-zero: true).
template <class T>
static bool env_u64(const char *name, uint64_t lo, uint64_t hi, T &knob) {
    const char *e = std::getenv(name);
    const uint64_t v = e ? std::strtoull(e, nullptr, 10) : 0;
    if (!e || v < lo || v > hi) return false;
    knob = (T)v;
    return true;
}
template <class T>
static bool env_int(const char *name, int lo, int hi, T &knob) {
    const char *e = std::getenv(name);
    const int v = e ? std::atoi(e) : 0;
    if (!e || v < lo || v > hi) return false;
    knob = (T)v;
    return true;
}
template <class T>
static void env_one_of(const char *name, std::initializer_list<int> set, T &knob) {
    int v = 0;
    if (env_int(name, INT_MIN, INT_MAX, v) && std::find(set.begin(), set.end(), v) != set.end()) knob = (T)v;
}
static void env_flag(const char *name, bool &knob) {
    int v = 0;
    if (env_int(name, INT_MIN, INT_MAX, v)) knob = v != 0;
}

// Everything a context takes from the environment, read HERE and once, when the context is created: one line per
// variable.  *gtab_bits and *hbm_budget_bytes are the caller's arguments: the environment overrides a zero only.
static void ctx_read_env(ssa_ctx *ctx, uint32_t *gtab_bits, uint64_t *hbm_budget_bytes) {
    CtxKnobs &k = ctx->knobs;
    if (env_u64("SSA_COOP_MAX_N", 0, UINT64_MAX, k.coop_max_n)) k.coop_max_n_torsion = k.coop_max_n;   // both crossovers
    env_u64("SSA_MSM_SMALL_MAX", 0, UINT64_MAX, k.msm_small_max);
    env_one_of("SSA_VERIFY_BLOCK", {64, 128, 256}, k.verify_block);
    env_u64("SSA_LANE_SLICE", 256, UINT64_MAX, k.lane_slice);        // lanes per slice of the per-lane kernels (workspace bound)
    env_u64("SSA_MSM_SLICE", 256, (uint64_t)1 << 23, k.msm_slice);   // signatures per slice of the MSM-form pipeline
    env_u64("SSA_AGG_BLOCK", 1, (uint64_t)1 << 30, k.agg_block);     // tests: lanes per block of the sharded half-aggregation
    env_int("SSA_MSM_TREE_GROUP", 2, 64, k.msm_tree_group);
    env_int("SSA_TAIL_PIECES", 0, VP_MAX, k.tail_pieces);            // pieces of a tail group's work (0 / 1: no end game)
    env_int("SSA_TAIL_GENS", 1, 8, k.tail_gens);                     // tail groups, in generations of resident waves
    env_flag("SSA_TAIL_UNIFORM", k.tail_uniform);
    env_int("SSA_TAIL_MIN_MAIN", INT_MIN, INT_MAX, k.tail_min_main);
    env_flag("SSA_TAIL_REVERSED", k.tail_reversed);
    env_int("SSA_TAIL_WAVES", INT_MIN, INT_MAX, k.tail_waves_override);   // tests: a small "generation"
    env_flag("SSA_MSM_OVERLAP", k.msm_overlap);
    env_int("SSA_PIPELINE_CHUNKS", 1, 8, k.pipeline_chunks);
    env_flag("SSA_TWO_STREAMS", ctx->two_streams);
    env_u64("SSA_SPLIT_MIN", 0, UINT64_MAX, k.split_min);            // one-slice calls below this many lanes are not split
    env_int("SSA_SPLIT_FRAC", 0, 8, k.split_frac);                   // the short part's share in 1/16ths (0: no split)
    env_flag("SSA_SPLIT_TAIL_B", k.split_tail_b);
    env_flag("SSA_SPLIT_ALONE", k.split_alone);                      // 0: split also beside other contexts of the device
    uint64_t mb = 0;
    if (*hbm_budget_bytes == 0 && env_u64("SSA_HBM_BUDGET_MB", 0, UINT64_MAX, mb)) *hbm_budget_bytes = mb << 20;
    if (*gtab_bits == 0) env_one_of("SSA_GTAB_BITS", {16, 20, 22, 24}, *gtab_bits);
}

// gtab_bits: window width of the comb for G (16, 20, 22 or 24; 0 = the widest whose table fits the budget; the
// environment's SSA_GTAB_BITS overrides 0).  hbm_budget_bytes: what the library may spend on tables that are a pure
// speed-for-memory trade (the comb for G, per-key combs of a key set); 0 = a tenth of the device memory that is free
// when the context is created (SSA_HBM_BUDGET_MB overrides 0).  An allocation that fails falls back to the next
// smaller table instead of failing the context: the 16-bit comb (100 MB) is the floor.
// inherit: the knobs of the context whose twin this one becomes -- then nothing is read from the environment.
static int ctx_create(ssa_ctx **out, int device, const void *params, size_t params_len, uint32_t gtab_bits,
                      uint64_t hbm_budget_bytes, const CtxKnobs *inherit) {
    if (!out) return SSA_ERR_ARG;
    *out = nullptr;
    if (gtab_bits != 0 && gtab_bits != 16 && gtab_bits != 20 && gtab_bits != 22 && gtab_bits != 24) return SSA_ERR_ARG;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count == 0) return SSA_ERR_NO_DEVICE;
    if (device < 0 || device >= count) return SSA_ERR_ARG;
    DevParams hp;
    if (params) {
        if (params_len != sizeof(DevParams)) return SSA_ERR_PARAMS;
        std::memcpy(&hp, params, sizeof hp);
    } else {
        std::memcpy(&hp, k_default_params, sizeof hp);
    }
    // the built-in blob is the builder's own instance (Rescue constants and generator are NOT upstream's: DESIGN.md
    // "parity unpinned"); a context created from it says so (ssa_ctx_uses_default_params)
    const bool is_default = std::memcmp(&hp, k_default_params, sizeof hp) == 0;
    if (int rc = validate_params(hp)) return rc;
    hp.flags = 0;  // derived flags are the library's, not the caller's
    bool small_mds = true;
    for (int i = 0; i < 144; i++) small_mds = small_mds && hp.mds[i] <= 0xffffffffull;
    if (small_mds) hp.flags |= PRM_FLAG_SMALL_MDS;
    bool tiny_mds = true;      // entries below 2^16 (the usual circulant of single-digit integers): carry-free MDS rows
    for (int i = 0; i < 144; i++) tiny_mds = tiny_mds && hp.mds[i] < 0x10000ull;
    if (tiny_mds) hp.flags |= PRM_FLAG_TINY_MDS;
    HIP_TRY(hipSetDevice(device));
    // owned here until it is handed out: every early return destroys what exists of it
    std::unique_ptr<ssa_ctx, decltype(&ssa_ctx_destroy)> guard(new ssa_ctx(), ssa_ctx_destroy);
    ssa_ctx *ctx = guard.get();
    ctx->device = device;
    ctx->default_params = is_default;
    if (inherit) ctx->knobs = *inherit;
    else ctx_read_env(ctx, &gtab_bits, &hbm_budget_bytes);
    HIP_TRY(hipStreamCreateWithFlags(&ctx->own_stream, hipStreamNonBlocking));
    HIP_TRY(hipStreamCreateWithFlags(&ctx->copy_stream, hipStreamNonBlocking));
    for (auto &st : ctx->hash_stream) HIP_TRY(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    HIP_TRY(hipEventCreateWithFlags(&ctx->pipe_start, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&ctx->order_ev, hipEventDisableTiming));
    for (int i = 0; i < 8; i++) {
        HIP_TRY(hipEventCreateWithFlags(&ctx->copy_done[i], hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&ctx->hash_done[i], hipEventDisableTiming));
    }
    ctx->stream = ctx->own_stream;
    if (!inherit) {   // the waves of ssa_k_verify that are resident at once: the size of its end game
        hipDeviceProp_t prop;
        int occ = 0;
        if (hipGetDeviceProperties(&prop, device) == hipSuccess &&
            hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, ssa_k_verify, 256, 0) == hipSuccess && occ > 0)
            ctx->knobs.verify_waves = (unsigned)prop.multiProcessorCount * (unsigned)occ * 4u;
        (void)hipGetLastError();
        if (ctx->knobs.tail_waves_override) ctx->knobs.verify_waves = ctx->knobs.tail_waves_override;
    }
    HIP_TRY(hipMalloc((void **)&ctx->d_params, sizeof(DevParams)));
    HIP_TRY(hipMemcpy(ctx->d_params, &hp, sizeof hp, hipMemcpyHostToDevice));
    ctx->h_params = hp;
    // HBM budget of the speed-for-memory tables, and the comb geometry it allows
    if (hbm_budget_bytes == 0) {
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) free_b = 0;
        hbm_budget_bytes = free_b / 10;
    }
    ctx->hbm_budget = hbm_budget_bytes;
    // the comb table of this generator on this device: shared by every context that asks for the same geometry.
    // Forced width: that one first; automatic: the widest within the budget.  Either way a failed allocation moves on
    // to the next smaller table.
    // A table that fails its check twice counts as one that did not fit; no clean table at all is SSA_ERR_TABLE.
    static const u32 k_widths[4] = {24, 22, 20, 16};
    bool bad_table = false;
    for (u32 wbits : k_widths) {
        if (gtab_bits ? wbits > gtab_bits : (wbits > 16 && gtab_bytes(wbits) > hbm_budget_bytes)) continue;
        ctx->gtab_share = gtab_acquire(ctx, hp, wbits, &bad_table);
        if (ctx->gtab_share) break;
    }
    if (!ctx->gtab_share) return bad_table ? SSA_ERR_TABLE : SSA_ERR_HIP;
    if (ctx->ws_fail.reserve(64)) return SSA_ERR_HIP;
    ctx->d_gtab = ctx->gtab_share->d_gtab;
    ctx->gtab_bits = ctx->gtab_share->bits;
    // the generator must be a point of the prime-order subgroup: on the curve, [q]G == O (through the comb table
    // just built), G != O -- otherwise every verification would run on some other curve or a small subgroup
    unsigned gen_ok = 0;
    hipLaunchKernelGGL(ssa_k_check_generator, dim3(1), dim3(64), 0, ctx->stream, ctx->d_params,
                       (const u64 *)ctx->d_gtab, (unsigned *)ctx->ws_fail.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(&gen_ok, ctx->ws_fail.p, sizeof gen_ok, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (gen_ok != 1u) return SSA_ERR_PARAMS;
    if (!inherit) {
        live_ctxs_add(device, 1);
        ctx->counted_live = true;
    }
    *out = guard.release();
    return 0;
}

extern "C" int ssa_ctx_create_ex(ssa_ctx **out, int device, const void *params, size_t params_len, uint32_t gtab_bits,
                                 uint64_t hbm_budget_bytes) {
    return ctx_create(out, device, params, params_len, gtab_bits, hbm_budget_bytes, nullptr);
}

extern "C" int ssa_ctx_create(ssa_ctx **out, int device, const void *params, size_t params_len) {
    return ssa_ctx_create_ex(out, device, params, params_len, 0u, 0ull);
}

// The second set of streams and workspaces of a context (calls of more than one slice alternate between the two, so
// that the tail of one slice's kernels -- the last wave of every SIMD runs alone, the XCDs finish 1.5-4 % apart: 0.9 ms
// of a 26.6 ms ssa_k_verify, 0.35 of an 8 ms ssa_k_hash -- is filled by the next slice's): a context of its own on the
// same device, blob and comb table (the registry hands the table out again: no second copy), owned by `ctx`.  It reads
// no environment: it is created from the knobs of `ctx` and takes them again at every call (the debug setters).
ssa_ctx *ssa_internal_twin(ssa_ctx *ctx) {
    if (ctx->is_twin || !ctx->two_streams) return nullptr;
    if (!ctx->twin) {
        DevParams hp = ctx->h_params;
        hp.flags = 0;
        if (ctx_create(&ctx->twin, ctx->device, &hp, sizeof hp, ctx->gtab_bits, ctx->hbm_budget, &ctx->knobs) != 0) {
            ctx->two_streams = false;          // no memory for a second workspace: one stream, as before
            return nullptr;
        }
        ctx->twin->is_twin = true;
    }
    ctx->twin->knobs = ctx->knobs;
    return ctx->twin;
}

// every live handle of a dead context gives its device memory back and forgets the context
template <class T, class F>
static void orphan_handles(std::vector<T *> &v, F &&release) {
    for (T *h : v) {
        release(h);
        h->ctx = nullptr;
    }
    v.clear();
}

extern "C" void ssa_ctx_destroy(ssa_ctx *ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    if (ctx->twin) {
        ssa_ctx_destroy(ctx->twin);
        ctx->twin = nullptr;
    }
    if (ctx->counted_live) live_ctxs_add(ctx->device, -1);
    // a key set that outlives its context (garbage-collection order of a binding) must not touch the dead stream:
    // its tables are freed here, the handle stays valid for ssa_keyset_destroy and is refused everywhere else
    orphan_handles(ctx->keysets, [](ssa_keyset *ks) { ks->release_all(); });
    orphan_handles(ctx->signer_sets, [](ssa_signer_set *ss) { ss->wipe_release(); });
    orphan_handles(ctx->keycaches, [](ssa_keycache *kc) { kc->release_all(); });
    orphan_handles(ctx->aggregators, [](ssa_aggregator *ag) { agx_release_all(*ag); });
    orphan_handles(ctx->aggverifiers, [](ssa_aggverifier *av) { agx_release_all(*av); });
    for (auto &kv : ctx->timed)
        for (auto &t : kv.second) timed_destroy(t);
    for_each_devbuf(ctx, [](DevBuf &b) { b.release(); });
    for_each_hostbuf(ctx, [](HostBuf &b) { b.release(); });
    if (ctx->d_params) (void)hipFree(ctx->d_params);
    gtab_release(ctx->gtab_share);
    ctx->gtab_share = nullptr;
    ctx->d_gtab = nullptr;
    for (auto &ev : ctx->copy_done)
        if (ev) (void)hipEventDestroy(ev);
    for (auto &ev : ctx->hash_done)
        if (ev) (void)hipEventDestroy(ev);
    if (ctx->pipe_start) (void)hipEventDestroy(ctx->pipe_start);
    if (ctx->order_ev) (void)hipEventDestroy(ctx->order_ev);
    if (ctx->agm_plan_ev) (void)hipEventDestroy(ctx->agm_plan_ev);
    for (auto &st : ctx->hash_stream)
        if (st) (void)hipStreamDestroy(st);
    if (ctx->copy_stream) (void)hipStreamDestroy(ctx->copy_stream);
    if (ctx->own_stream) (void)hipStreamDestroy(ctx->own_stream);
    delete ctx;
}

// What the context holds on the device: out[0] window bits and out[1] windows of the comb for G, out[2] its bytes
// (shared by the contexts of a process), out[3] bytes of this context's workspaces and staging buffers as reserved so
// far (its second stream's included), out[4] lanes per slice of the per-lane kernels, out[5] signatures per slice of
// the MSM form, out[6] the HBM budget of the speed-for-memory tables, out[7] 1 when slices alternate between two streams.
extern "C" int ssa_ctx_info(const ssa_ctx *ctx, uint64_t out[8]) {
    if (!ctx || !out) return SSA_ERR_ARG;
    auto reserved = [](const ssa_ctx *c) {
        uint64_t sum = 0;
        for_each_devbuf(c, [&](const DevBuf &b) { sum += b.cap; });
        return sum;
    };
    out[0] = ctx->gtab_bits;
    out[1] = gtab_windows(ctx->gtab_bits);
    out[2] = gtab_bytes(ctx->gtab_bits);
    out[3] = reserved(ctx) + (ctx->twin ? reserved(ctx->twin) : 0);
    out[4] = ctx->knobs.lane_slice;
    out[5] = ctx->knobs.msm_slice;
    out[6] = ctx->hbm_budget;
    out[7] = ctx->two_streams && !ctx->is_twin ? 1 : 0;
    return 0;
}

// The exact check of the context's tables on demand: the comb for G and, once built, the
// constant-time table.  A comb that fails is retired from the registry (contexts created afterwards build a new one;
// this one keeps its reference until it is destroyed).
extern "C" int ssa_ctx_selfcheck(ssa_ctx *ctx, uint32_t flags, uint64_t out[8]) {
    if (!ctx || !out || flags != 0) return SSA_ERR_ARG;
    HIP_TRY(hipSetDevice(ctx->device));
    uint64_t g[2], c[3] = {0, 0, ~0ull};
    if (int rc = ssa_internal_gtab_check(ctx, ctx->d_gtab, ctx->gtab_bits, g)) return rc;
    // the constant-time table only behind a clean comb: its offset rows are checked by a walk of the comb, and a wrong
    // header word would misdirect that walk
    if (g[0] == 0)
        if (int rc = ssa_internal_ctab_selfcheck(ctx, c)) return rc;
    out[0] = gtab_entries(ctx->gtab_bits);
    out[1] = g[0];
    out[2] = g[1];
    out[3] = c[0];
    out[4] = c[1];
    out[5] = c[2];
    out[6] = (uint64_t)ctx->gtab_share->builds;
    out[7] = ctx->gtab_bits;
    if (g[0]) {
        std::lock_guard<std::mutex> lock(g_gtab_mu);
        SharedGtab *sg = ctx->gtab_share;
        if (!sg->retired) {
            sg->retired = true;
            forget_handle(g_gtabs, sg);
        }
    }
    return g[0] || c[1] ? SSA_ERR_TABLE : SSA_OK;
}

extern "C" int ssa_ctx_uses_default_params(const ssa_ctx *ctx) { return ctx ? (ctx->default_params ? 1 : 0) : SSA_ERR_ARG; }

extern "C" int ssa_ctx_set_stream(ssa_ctx *ctx, void *hip_stream) {
    if (!ctx) return SSA_ERR_ARG;
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    ctx->stream = hip_stream ? (hipStream_t)hip_stream : ctx->own_stream;
    return 0;
}

// Ordering between the context's stream and a stream of the caller, without a host synchronisation (one event each way).
extern "C" int ssa_ctx_stream_release(ssa_ctx *ctx, void *consumer_stream) {
    if (!ctx) return SSA_ERR_ARG;
    HIP_TRY(hipSetDevice(ctx->device));
    if ((hipStream_t)consumer_stream == ctx->stream) return 0;      // same stream: already ordered
    HIP_TRY(hipEventRecord(ctx->order_ev, ctx->stream));
    HIP_TRY(hipStreamWaitEvent((hipStream_t)consumer_stream, ctx->order_ev, 0));
    return 0;
}

extern "C" int ssa_ctx_stream_acquire(ssa_ctx *ctx, void *producer_stream) {
    if (!ctx) return SSA_ERR_ARG;
    HIP_TRY(hipSetDevice(ctx->device));
    if ((hipStream_t)producer_stream == ctx->stream) return 0;
    HIP_TRY(hipEventRecord(ctx->order_ev, (hipStream_t)producer_stream));
    HIP_TRY(hipStreamWaitEvent(ctx->stream, ctx->order_ev, 0));
    return 0;
}

extern "C" int ssa_ctx_sync(ssa_ctx *ctx) {
    if (!ctx) return SSA_ERR_ARG;
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return 0;
}

extern "C" int ssa_ctx_enable_timing(ssa_ctx *ctx, int on) {
    if (!ctx) return SSA_ERR_ARG;
    ctx->knobs.timing = on != 0;
    return 0;
}

extern "C" int ssa_ctx_read_timing(ssa_ctx *ctx, const char *kernel, double *avg_ms, uint64_t *launches) {
    if (!ctx || !kernel) return SSA_ERR_ARG;
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    double total = 0;
    uint64_t cnt = 0;
    // the context's own launches and, after calls of more than one slice, its twin's (whose launches overlap the
    // context's: their event times are then not exclusive -- DESIGN.md section 5).  A one-slice call split over the two
    // streams has ONE entry per key, kept by the context: the span from the earlier start to the
    // later end of its two launches of that kernel.  The two keys of such a call overlap by design -- part B's
    // ssa_k_verify runs under part A's ssa_k_hash -- so their times do not add up to the call's.
    for (ssa_ctx *c : {ctx, ctx->twin}) {
        if (!c) continue;
        if (c != ctx) HIP_TRY(hipStreamSynchronize(c->stream));
        auto it = c->timed.find(kernel);
        if (it == c->timed.end()) continue;
        for (auto &t : it->second) {
            float ms = 0;
            if (timed_ms(t, &ms)) {
                total += ms;
                cnt++;
            }
            timed_destroy(t);
        }
        c->timed.erase(it);
    }
    if (avg_ms) *avg_ms = cnt ? total / (double)cnt : 0.0;
    if (launches) *launches = cnt;
    return 0;
}

// test hook: the last entry of `kernel` that a split call recorded, read and left in place:
// out[0] the entry's span as ssa_ctx_read_timing will count it, out[1] part A's launch alone, out[2] part B's (ms).
// SSA_ERR_ARG: no such entry.
extern "C" int ssa_debug_split_timing(ssa_ctx *ctx, const char *kernel, double out[3]) {
    if (!ctx || !kernel || !out) return SSA_ERR_ARG;
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    const auto it = ctx->timed.find(kernel);
    if (it == ctx->timed.end()) return SSA_ERR_ARG;
    for (auto t = it->second.rbegin(); t != it->second.rend(); ++t) {
        if (!t->start2) continue;
        float span = 0, a = 0, b = 0;
        if (!timed_ms(*t, &span)) return SSA_ERR_HIP;
        HIP_TRY(hipEventElapsedTime(&a, t->start, t->stop));
        HIP_TRY(hipEventElapsedTime(&b, t->start2, t->stop2));
        out[0] = span;
        out[1] = a;
        out[2] = b;
        return 0;
    }
    return SSA_ERR_ARG;
}

// ------------------------------------------------------------------ device entry points
extern "C" int ssa_hash_message_many_device(ssa_ctx *ctx, const uint8_t *d_sigs, const uint8_t *d_pks,
                                            const uint8_t *d_msgs, const uint64_t *d_msg_off,
                                            size_t msg_stride, size_t msg_len, size_t n,
                                            uint8_t *d_digests_out) {
    const MsgView mv{d_msgs, d_msg_off, msg_stride, msg_len};
    if (!ctx || (n && (!d_sigs || !d_pks || !d_digests_out))) return SSA_ERR_ARG;
    if (int rc = check_msgs(mv, n)) return rc;
    if (n == 0) return 0;
    HIP_TRY(hipSetDevice(ctx->device));
    return timed_launch(ctx, "ssa_k_hash", [&] {
        hipLaunchKernelGGL(ssa_k_hash, dim3(grid_for(n, 256)), dim3(256), 0, ctx->stream, ctx->d_params,
                           d_sigs, d_pks, mv, n, (u64 *)nullptr, d_digests_out, (const u32 *)nullptr, 0u);
    });
}

extern "C" int ssa_rescue_hash_many_device(ssa_ctx *ctx, const uint64_t *d_felts, uint32_t felts_per_row,
                                           size_t n, uint64_t *d_digests_out) {
    if (!ctx || (n && (!d_digests_out || (felts_per_row && !d_felts)))) return SSA_ERR_ARG;
    if (n == 0) return 0;
    HIP_TRY(hipSetDevice(ctx->device));
    return timed_launch(ctx, "ssa_k_rescue", [&] {
        hipLaunchKernelGGL(ssa_k_rescue, dim3(grid_for(n, 256)), dim3(256), 0, ctx->stream, ctx->d_params,
                           (const u64 *)d_felts, felts_per_row, n, (u64 *)d_digests_out);
    });
}

// one chunk of challenge hashes on `hs` (the shared upload pipeline of the host-buffer entry points)
int ssa_internal_hash_chunk(ssa_ctx *ctx, hipStream_t hs, const DevBatch &b, size_t cnt, uint64_t *d_h) {
    hipLaunchKernelGGL(ssa_k_hash, dim3(grid_for(cnt, 256)), dim3(256), 0, hs, ctx->d_params, b.sigs, b.pks, b.msgs, cnt,
                       (u64 *)d_h, (u8 *)nullptr, (const u32 *)nullptr, 0u);
    HIP_TRY(hipGetLastError());
    return 0;
}

int ssa_internal_hash_scalars(ssa_ctx *ctx, const DevBatch &b, size_t n) {
    if (ctx->ws_h.reserve(n * 4 * sizeof(u64))) return SSA_ERR_HIP;
    return timed_launch(ctx, "ssa_k_hash", [&] {
        hipLaunchKernelGGL(ssa_k_hash, dim3(grid_for(n, 256)), dim3(256), 0, ctx->stream, ctx->d_params,
                           b.sigs, b.pks, b.msgs, n, (u64 *)ctx->ws_h.p, (u8 *)nullptr, (const u32 *)nullptr, 0u);
    });
}

int ssa_internal_hash_scalars_digests(ssa_ctx *ctx, const DevBatch &b, size_t n, uint64_t *d_h, uint8_t *d_dig) {
    return timed_launch(ctx, "ssa_k_hash", [&] {
        hipLaunchKernelGGL(ssa_k_hash, dim3(grid_for(n, 256)), dim3(256), 0, ctx->stream, ctx->d_params,
                           b.sigs, b.pks, b.msgs, n, (u64 *)d_h, (u8 *)d_dig, (const u32 *)nullptr, 0u);
    });
}

// The end game of an ssa_k_verify launch over cnt lanes: which groups run in pieces, where their work is cut.  The cuts
// follow instruction counts (a doubling 2642 VALU instructions, a mixed addition 3738; the table build ~57 k in front of
// the first pass, the comb for G and the comparison ~45 k behind the last): the first piece is half of a lane's work, the
// next a quarter, ... the last two equal (SSA_TAIL_UNIFORM=1: equal pieces); a piece never spans the two passes of
// SSA_FLAG_CHECK_TORSION.
struct TailKnobs {
    unsigned pieces, gens, waves, block, min_main;
    bool uniform, reversed;
};
static TailPlan tail_plan_of(const TailKnobs &kn, size_t cnt, uint32_t flags) {
    const TailKnobs *ctx = &kn;
    TailPlan tp{};
    const bool torsion = (flags & SSA_FLAG_CHECK_TORSION) != 0;
    tp.whole[0] = 0u | 2u | 4u | ((u32)LADDER_STEPS_Q << 16);
    tp.whole[1] = 1u | 2u | 4u | ((u32)LADDER_STEPS << 16);
    const u32 n_groups = (u32)((cnt + 63) / 64);
    const unsigned cap = torsion ? (unsigned)VP_MAX - 1u : (unsigned)VP_MAX;      // (the pass boundary is one more cut)
    const unsigned want = ctx->pieces < cap ? ctx->pieces : cap;
    const u32 tail0 = ctx->gens * ctx->waves;
    if (want < 2 || ctx->block != 256 || tail0 == 0 || n_groups < tail0 + ctx->min_main * ctx->waves) return tp;
    const u32 main_groups = ((n_groups - tail0) / 4u) * 4u;
    tp.main_blocks = main_groups / 4u;
    tp.tail_groups = ((n_groups - main_groups + 3u) / 4u) * 4u;
    // the lane's work as one sequence of steps: [pass 0 windows] [pass 1 windows], with the table build in front and the
    // comb + comparison behind
    const double DBL = 2642.0, ADD = 3738.0, TABLE = 57000.0, TAIL = 45000.0;
    struct Step { int pass, it; double cost; };
    std::vector<Step> steps;
    for (int pass = torsion ? 0 : 1; pass < 2; pass++)
        for (int it = 0; it < (pass == 0 ? LADDER_STEPS_Q : LADDER_STEPS); it++)
            steps.push_back({pass, it, (pass == 0 ? (double)QNAF_GAP[it + 1] : 5.0) * DBL + ADD});
    double total = TABLE + TAIL;
    for (const Step &st : steps) total += st.cost;
    // cumulative targets of the pieces
    std::vector<double> target;
    double frac = 0.0, f = 0.5;
    for (unsigned k = 0; k + 1 < want; k++) {
        frac += ctx->uniform ? 1.0 / (double)want : f;
        if (k + 2 < want) f *= 0.5;
        target.push_back(total * frac);
    }
    // cut in front of the step that would cross a target (and between the passes, always)
    std::vector<std::pair<size_t, size_t>> pieces;
    size_t cur = 0, tix = 0;
    double acc = TABLE;
    for (size_t idx = 0; idx < steps.size(); idx++) {
        bool cut = false;
        if (idx > cur) {
            if (steps[idx].pass != steps[idx - 1].pass) cut = true;
            else if (tix < target.size() && acc + steps[idx].cost * 0.5 >= target[tix]) cut = true;
        }
        if (cut) {
            pieces.push_back({cur, idx});
            cur = idx;
        }
        while (tix < target.size() && acc + steps[idx].cost * 0.5 >= target[tix]) tix++;     // targets reached
        acc += steps[idx].cost;
    }
    pieces.push_back({cur, steps.size()});
    if (pieces.size() < 2 || pieces.size() > (size_t)VP_MAX) return tp;        // (n_pieces stays 0: no end game)
    for (const auto &pc : pieces) {
        const int pass = steps[pc.first].pass, lo = steps[pc.first].it, hi = steps[pc.second - 1].it + 1;
        const int n_steps = pass == 0 ? LADDER_STEPS_Q : LADDER_STEPS;
        tp.ph[tp.n_pieces++] = (u32)pass | (lo == 0 ? 2u : 0u) | (hi == n_steps ? 4u : 0u) | ((u32)lo << 8) | ((u32)hi << 16);
    }
    tp.reversed = ctx->reversed ? 1u : 0u;
    return tp;
}
static TailPlan tail_plan(const ssa_ctx *ctx, size_t cnt, uint32_t flags) {
    return tail_plan_of({ctx->knobs.tail_pieces, ctx->knobs.tail_gens, ctx->knobs.verify_waves, ctx->knobs.verify_block, ctx->knobs.tail_min_main,
                         ctx->knobs.tail_uniform, ctx->knobs.tail_reversed}, cnt, flags);
}

// the plan for explicit knobs: no context and no device needed, so the host logic is tested on the CPU
// (tests/test_tail_plan.py: the pieces cover every window of every pass exactly once and never span two passes, the
// grid is what the kernel assumes).  out: n_pieces, tail_groups, main_blocks, grid blocks, ph[0..7], whole[0..1].
extern "C" int ssa_debug_tail_plan(unsigned waves, unsigned pieces, unsigned gens, int uniform, unsigned min_main, size_t n,
                                   uint32_t flags, uint32_t out[14]) {
    if (!out) return SSA_ERR_ARG;
    const TailPlan tp = tail_plan_of({pieces, gens, waves, 256u, min_main, uniform != 0, false}, n, flags);
    out[0] = tp.n_pieces;
    out[1] = tp.tail_groups;
    out[2] = tp.main_blocks;
    out[3] = tp.n_pieces ? tail_grid_blocks(tp) : (uint32_t)((n + 255) / 256);
    for (int k = 0; k < VP_MAX; k++) out[4 + k] = tp.ph[k];
    out[12] = tp.whole[0];
    out[13] = tp.whole[1];
    return 0;
}

// A one-slice call of the lane kernels as two unequal parts on the context's two streams: part A,
// lanes [0, nA), stays on the caller's stream and ends alone; part B, the nB lanes behind it, runs on the twin's.
// nA + nB = n, nA is a multiple of 256 (a whole number of ssa_k_hash and ssa_k_verify workgroups: B's lanes start at a
// workgroup of their own), nB <= nA; nB = 0: the call is not split -- the split is off (frac 0), the call is short
// (n < min_n) or takes the cooperative kernel, or there is no second stream.
struct SplitKnobs {
    size_t min_n;
    unsigned frac;       // the short part's share in 1/16ths: 1..8
    bool coop, twin;     // the call takes the cooperative kernel; a twin is there to run part B
};
static void split_plan_of(const SplitKnobs &kn, size_t n, size_t *nA, size_t *nB) {
    *nA = n;
    *nB = 0;
    if (kn.frac == 0 || kn.frac > 8 || kn.coop || !kn.twin || n < kn.min_n) return;
    const size_t want_b = n / 16 * kn.frac + n % 16 * kn.frac / 16;       // n * frac / 16
    const size_t a = (n - want_b + 255) / 256 * 256;
    if (a >= n) return;                                                   // (nothing left behind a whole workgroup)
    *nA = a;
    *nB = n - a;
}
// the plan for explicit knobs, like ssa_debug_tail_plan (tests/test_split_plan.py): out[0] = nA, out[1] = nB
extern "C" int ssa_debug_split_plan(size_t n, uint32_t flags, size_t split_min, unsigned split_frac, size_t coop_max_n,
                                    size_t coop_max_n_torsion, int twin, uint64_t out[2]) {
    if (!out) return SSA_ERR_ARG;
    size_t nA, nB;
    split_plan_of({split_min, split_frac, takes_coop_of(coop_max_n, coop_max_n_torsion, n, flags), twin != 0}, n, &nA, &nB);
    out[0] = nA;
    out[1] = nB;
    return 0;
}
// test hook: the split's knobs on this context (its twin takes them at the next call); a negative value leaves a knob alone
extern "C" int ssa_debug_split_config(ssa_ctx *ctx, int64_t split_min, int split_frac, int tail_b, int alone) {
    if (!ctx || split_frac > 8) return SSA_ERR_ARG;
    if (alone >= 0) ctx->knobs.split_alone = alone != 0;
    if (split_min >= 0) ctx->knobs.split_min = (size_t)split_min;
    if (split_frac >= 0) ctx->knobs.split_frac = (unsigned)split_frac;
    if (tail_b >= 0) ctx->knobs.split_tail_b = tail_b != 0;
    return 0;
}

// One ssa_k_verify launch over cnt lanes on c->stream, in two steps: verify_grid plans it (end_game: it may have one) and
// zeroes c's end-game flags on the stream; verify_kernel is the launch itself -- the lanes' challenge scalars at d_h,
// their tables at d_tab, the end-game buffers c's own -- for whoever times it.
struct VerifyGrid {
    TailPlan tp;
    unsigned blocks;
};
static int verify_grid(ssa_ctx *c, size_t cnt, uint32_t flags, bool end_game, VerifyGrid *g) {
    g->tp = end_game ? tail_plan(c, cnt, flags) : tail_plan_of({0u, 0u, 0u, c->knobs.verify_block, 0u, false, false}, cnt, flags);
    g->blocks = grid_for(cnt, c->knobs.verify_block);
    if (g->tp.n_pieces) {
        if (c->tail_done.reserve(2 * (size_t)g->tp.tail_groups * sizeof(u32)) ||       // finished pieces, claimed pieces
            c->tail_park.reserve((size_t)g->tp.tail_groups * PARK_WORDS * 64 * sizeof(u64)))
            return SSA_ERR_HIP;
        HIP_TRY(hipMemsetAsync(c->tail_done.p, 0, 2 * (size_t)g->tp.tail_groups * sizeof(u32), c->stream));
        g->blocks = tail_grid_blocks(g->tp);
    }
    return 0;
}
static void verify_kernel(ssa_ctx *c, const VerifyGrid &g, const DevBatch &s, const u64 *d_h, u64 *d_tab, size_t cnt,
                          uint32_t flags, uint8_t *d_status_out, unsigned long long *d_fail) {
    hipLaunchKernelGGL(ssa_k_verify, dim3(g.blocks), dim3(c->knobs.verify_block), 0, c->stream, s.sigs, s.pks, s.pk_inf, d_h,
                       (const u64 *)c->d_gtab, d_tab, cnt, flags, d_status_out, d_fail, g.tp, (u32 *)c->tail_done.p,
                       (u64 *)c->tail_park.p);
}

// ssa_k_verify over n lanes whose challenge scalars are in d_h, in slices of at most ctx->knobs.lane_slice lanes: the 4 KB
// per-lane table workspace never exceeds one slice (the caller has reserved it).  *d_fail is added to.
static int verify_slices(ssa_ctx *ctx, const DevBatch &b, const u64 *d_h, size_t n, uint32_t flags, uint8_t *d_status_out,
                         unsigned long long *d_fail) {
    return for_dev_slices(b, n, ctx->knobs.lane_slice, [&](size_t lo, size_t cnt, const DevBatch &s) {
        VerifyGrid g;
        if (int rc = verify_grid(ctx, cnt, flags, true, &g)) return rc;
        return timed_launch(ctx, "ssa_k_verify", [&] {
            verify_kernel(ctx, g, s, d_h + 4 * lo, (u64 *)ctx->ws_tab.p, cnt, flags, d_status_out + lo, d_fail);
        });
    });
}

int ssa_internal_verify_hashed(ssa_ctx *ctx, const DevBatch &b, const uint64_t *d_h, size_t n, uint32_t flags,
                               uint8_t *d_status_out, unsigned long long *d_fail) {
    const size_t slice = ctx->knobs.lane_slice < n ? ctx->knobs.lane_slice : n;
    if (ctx->ws_tab.reserve(slice * (size_t)(PTAB_ENTRIES * PTAB_ENTRY_U64) * sizeof(u64))) return SSA_ERR_HIP;
    return verify_slices(ctx, b, (const u64 *)d_h, n, flags, d_status_out, d_fail);
}

// hash + verification of ONE slice (cnt <= c->knobs.lane_slice lanes) on c->stream with c's workspaces; *d_fail is added to
static int verify_one_slice(ssa_ctx *c, const DevBatch &b, size_t cnt, uint32_t flags, uint8_t *d_status_out,
                            unsigned long long *d_fail) {
    if (c->ws_h.reserve(cnt * 4 * sizeof(u64))) return SSA_ERR_HIP;
    if (c->ws_tab.reserve(cnt * (size_t)(PTAB_ENTRIES * PTAB_ENTRY_U64) * sizeof(u64))) return SSA_ERR_HIP;
    int rc = timed_launch(c, "ssa_k_hash", [&] {
        hipLaunchKernelGGL(ssa_k_hash, dim3(grid_for(cnt, 256)), dim3(256), 0, c->stream, c->d_params, b.sigs, b.pks,
                           b.msgs, cnt, (u64 *)c->ws_h.p, (u8 *)nullptr, (const u32 *)nullptr, 0u);
    });
    if (rc) return rc;
    return verify_slices(c, b, (const u64 *)c->ws_h.p, cnt, flags, d_status_out, d_fail);
}

// ONE slice as two parts (split_plan_of): hash + verification of lanes [0, nA) on ctx->stream and of
// the nB lanes behind them on tw->stream, into disjoint lane ranges of ctx's OWN ws_h and ws_tab (sized for the slice, as
// for an unsplit call), of the one status array and into the one counter.  Of the twin only the stream and the end-game
// buffers are used.  Stream events are the only ordering: tw->stream starts behind everything queued on ctx->stream
// before the call, and ctx->stream continues behind both parts, on an error return too.  B's launches are queued in front
// of A's verifier: B's short hash ends early, its verifier runs under the end of A's hash, and its ladder is resident when
// every wave of A's first generation builds its table.  With timing on, each key gets ONE entry for its two launches.
static int verify_split(ssa_ctx *ctx, ssa_ctx *tw, const DevBatch &b, size_t nA, size_t nB, uint32_t flags,
                        uint8_t *d_status_out, unsigned long long *d_fail) {
    constexpr size_t TAB_WORDS = (size_t)(PTAB_ENTRIES * PTAB_ENTRY_U64);
    const size_t n = nA + nB;
    if (ctx->ws_h.reserve(n * 4 * sizeof(u64)) || ctx->ws_tab.reserve(n * TAB_WORDS * sizeof(u64))) return SSA_ERR_HIP;
    u64 *h = (u64 *)ctx->ws_h.p, *tab = (u64 *)ctx->ws_tab.p;
    const DevBatch bB = b.slice(nA);
    HIP_TRY(hipEventRecord(ctx->order_ev, ctx->stream));
    HIP_TRY(hipStreamWaitEvent(tw->stream, ctx->order_ev, 0));
    TimedLaunch th{}, tv{};
    const bool timing = ctx->knobs.timing;
    auto mark = [&](hipEvent_t *ev, hipStream_t st) {
        if (!timing) return 0;
        HIP_TRY(hipEventCreate(ev));
        HIP_TRY(hipEventRecord(*ev, st));
        return 0;
    };
    auto hash = [&](ssa_ctx *c, const DevBatch &s, size_t cnt, u64 *d_h, hipEvent_t *start, hipEvent_t *stop) {
        if (int r = mark(start, c->stream)) return r;
        hipLaunchKernelGGL(ssa_k_hash, dim3(grid_for(cnt, 256)), dim3(256), 0, c->stream, c->d_params, s.sigs, s.pks, s.msgs,
                           cnt, d_h, (u8 *)nullptr, (const u32 *)nullptr, 0u);
        HIP_TRY(hipGetLastError());
        return mark(stop, c->stream);
    };
    auto verify = [&](ssa_ctx *c, const DevBatch &s, size_t lo, size_t cnt, bool end_game, hipEvent_t *start, hipEvent_t *stop) {
        VerifyGrid g;
        if (int r = verify_grid(c, cnt, flags, end_game, &g)) return r;
        if (int r = mark(start, c->stream)) return r;
        verify_kernel(c, g, s, h + 4 * lo, tab + lo * TAB_WORDS, cnt, flags, d_status_out + lo, d_fail);
        HIP_TRY(hipGetLastError());
        return mark(stop, c->stream);
    };
    int rc = hash(ctx, b, nA, h, &th.start, &th.stop);
    if (rc == 0) rc = hash(tw, bB, nB, h + 4 * nA, &th.start2, &th.stop2);
    if (rc == 0) rc = verify(tw, bB, nA, nB, ctx->knobs.split_tail_b, &tv.start2, &tv.stop2);
    if (rc == 0) rc = verify(ctx, b, 0, nA, true, &tv.start, &tv.stop);
    if (timing && rc == 0) {
        ctx->timed["ssa_k_hash"].push_back(th);
        ctx->timed["ssa_k_verify"].push_back(tv);
    } else {
        timed_destroy(th);
        timed_destroy(tv);
    }
    if (hipEventRecord(tw->order_ev, tw->stream) != hipSuccess || hipStreamWaitEvent(ctx->stream, tw->order_ev, 0) != hipSuccess)
        return rc ? rc : SSA_ERR_HIP;
    return rc;
}

// the kernels of one verification batch on ctx->stream; *d_fail is added to, not reset.  may_split: a one-slice batch may
// run as two parts on the two streams (verify_split) -- the EXPORTED ssa_verify_many_device alone says so, not the
// library's own uses of it (ssa_internal_verify_many_device): the host forms drive the context and its twin from two
// threads (run_host_slices), where nobody else may reach into the twin, and none of the other forms was measured.
static int verify_launch(ssa_ctx *ctx, const DevBatch &b, size_t n, uint32_t flags, uint8_t *d_status_out,
                         unsigned long long *d_fail, bool may_split = false) {
    // small batches: one wave per signature (low latency); large ones: one lane per signature (throughput)
    if (takes_coop(ctx, n, flags)) {
        return timed_launch(ctx, "ssa_k_verify_coop", [&] {
            hipLaunchKernelGGL(ssa_k_verify_coop, dim3((unsigned)n), dim3(128), 0, ctx->stream, ctx->d_params, b.sigs,
                               b.pks, b.pk_inf, b.msgs, (const u64 *)ctx->d_gtab, n, flags, d_status_out, d_fail);
        });
    }
    // The per-lane workspaces (32 B of challenge scalar, 4 KB of table) are sized for ONE slice of at most
    // ctx->knobs.lane_slice lanes, whatever n is (4.3 GB of tables at the default 2^20; the reference takes slices of any
    // length, src/batch.rs:31-50): a larger batch runs slice after slice, into the caller's one status array and the one
    // rejection counter.  At n <= lane_slice this is the single pair of launches it always was.
    const size_t slice = ctx->knobs.lane_slice < n ? ctx->knobs.lane_slice : n;
    if (n <= slice) {
        // one slice: two unequal parts on the two streams where the split is on, the call is long enough and the context
        // has its device to itself (the twin is made only for such a call), otherwise the single pair of launches
        if (may_split && ctx->knobs.split_frac && n >= ctx->knobs.split_min && (!ctx->knobs.split_alone || live_ctxs_on(ctx->device) == 1)) {
            ssa_ctx *tw = ssa_internal_twin(ctx);
            size_t nA, nB;
            split_plan_of({ctx->knobs.split_min, ctx->knobs.split_frac, false, tw != nullptr}, n, &nA, &nB);
            if (nB) return verify_split(ctx, tw, b, nA, nB, flags, d_status_out, d_fail);
        }
        return verify_one_slice(ctx, b, n, flags, d_status_out, d_fail);
    }
    // More than one slice: the slices alternate between the context's stream and its twin's (a second set of
    // workspaces), so that one slice's kernels fill the tails of the other's -- ordered after everything queued on
    // ctx->stream before the call, and ctx->stream continues after both.
    ssa_ctx *tw = ssa_internal_twin(ctx);
    if (tw) {
        HIP_TRY(hipEventRecord(ctx->order_ev, ctx->stream));
        HIP_TRY(hipStreamWaitEvent(tw->stream, ctx->order_ev, 0));
    }
    int rc = 0;
    size_t j = 0;
    for (size_t lo = 0; lo < n && rc == 0; lo += slice, j++) {
        const size_t cnt = n - lo < slice ? n - lo : slice;
        ssa_ctx *c = (tw && (j & 1u)) ? tw : ctx;
        rc = verify_one_slice(c, b.slice(lo), cnt, flags, d_status_out + lo, d_fail);
    }
    if (tw) {     // (also on an error: whatever was queued on the twin's stream is still ordered before the caller's next step)
        if (hipEventRecord(tw->order_ev, tw->stream) != hipSuccess ||
            hipStreamWaitEvent(ctx->stream, tw->order_ev, 0) != hipSuccess)
            return rc ? rc : SSA_ERR_HIP;
    }
    return rc;
}

static int verify_many_device(ssa_ctx *ctx, const DevBatch &b, size_t n, uint32_t flags, uint8_t *d_status_out,
                              uint64_t *d_n_fail_out, bool may_split) {
    if (int rc = check_dev_batch(ctx, b, n, d_status_out)) return rc;
    unsigned long long *d_fail;
    if (int rc = reset_fail_counter(ctx, d_n_fail_out, &d_fail)) return rc;
    if (n == 0) return 0;
    return verify_launch(ctx, b, n, flags, d_status_out, d_fail, may_split);
}

// the exported call: the one place that lets a one-slice batch run as two parts (may_split)
extern "C" int ssa_verify_many_device(ssa_ctx *ctx, const uint8_t *d_sigs, const uint8_t *d_pks,
                                      const uint8_t *d_pk_inf, const uint8_t *d_msgs,
                                      const uint64_t *d_msg_off, size_t msg_stride, size_t msg_len,
                                      size_t n, uint32_t flags, uint8_t *d_status_out,
                                      uint64_t *d_n_fail_out) {
    return verify_many_device(ctx, {d_sigs, d_pks, d_pk_inf, {d_msgs, d_msg_off, msg_stride, msg_len}}, n, flags,
                              d_status_out, d_n_fail_out, true);
}

// ssa_verify_many_device as the one-slice worker of the library's other forms (the keyed records, host and device; the
// small batches of the screened forms): the same checks and launches, never split -- those forms were not measured, and
// the host ones drive the context and its twin from two threads
int ssa_internal_verify_many_device(ssa_ctx *ctx, const uint8_t *d_sigs, const uint8_t *d_pks, const uint8_t *d_pk_inf,
                                    const uint8_t *d_msgs, const uint64_t *d_msg_off, size_t msg_stride, size_t msg_len,
                                    size_t n, uint32_t flags, uint8_t *d_status_out, uint64_t *d_n_fail_out) {
    return verify_many_device(ctx, {d_sigs, d_pks, d_pk_inf, {d_msgs, d_msg_off, msg_stride, msg_len}}, n, flags,
                              d_status_out, d_n_fail_out, false);
}

// the throughput (variable-time) signer's launch; arguments checked by the caller (ssa_sign.hip)
int ssa_internal_sign_vartime(ssa_ctx *ctx, const uint8_t *d_sks, const uint8_t *d_nonces, const MsgView &mv, size_t n,
                              uint8_t *d_pks_out, uint8_t *d_sigs_out) {
    return timed_launch(ctx, "ssa_k_sign", [&] {
        hipLaunchKernelGGL(ssa_k_sign, dim3(grid_for(n, 256)), dim3(256), 0, ctx->stream, ctx->d_params,
                           (const u64 *)ctx->d_gtab, d_sks, d_nonces, mv, n, d_pks_out, d_sigs_out);
    });
}

// the throughput signer of a signer set (ssa_sign_many_indexed_device); arguments checked by the caller (ssa_sign.hip)
int ssa_internal_sign_indexed_vartime(ssa_ctx *ctx, const ssa_signer_set *ss, const uint32_t *d_key_idx,
                                      const uint8_t *d_nonces, const MsgView &mv, size_t n, bool keyed, uint8_t *d_out,
                                      uint8_t *d_status_out) {
    return timed_launch(ctx, "ssa_k_sign_indexed", [&] {
        hipLaunchKernelGGL(ssa_k_sign_indexed, dim3(grid_for(n, 256)), dim3(256), 0, ctx->stream, ctx->d_params,
                           (const u64 *)ctx->d_gtab, ss->view(), d_key_idx, d_nonces, mv, n, keyed ? 1u : 0u, d_out,
                           d_status_out);
    });
}

extern "C" int ssa_keygen_sign_many_device(ssa_ctx *ctx, const uint8_t *d_sks, const uint8_t *d_nonces,
                                           const uint8_t *d_msgs, const uint64_t *d_msg_off,
                                           size_t msg_stride, size_t msg_len, size_t n,
                                           uint8_t *d_pks_out, uint8_t *d_sigs_out) {
    return ssa_keygen_sign_many_ex_device(ctx, d_sks, d_nonces, d_msgs, d_msg_off, msg_stride, msg_len, n, 0u, d_pks_out,
                                          d_sigs_out);
}

extern "C" int ssa_decompress_many_device(ssa_ctx *ctx, const uint8_t *d_compressed, size_t n,
                                          uint8_t *d_pks_out, uint8_t *d_pk_inf_out, uint8_t *d_status_out) {
    if (!ctx || (n && (!d_compressed || !d_pks_out || !d_status_out)) || n > SSA_MAX_BATCH) return SSA_ERR_ARG;
    if (n == 0) return 0;
    HIP_TRY(hipSetDevice(ctx->device));
    return timed_launch(ctx, "ssa_k_decompress", [&] {
        hipLaunchKernelGGL(ssa_k_decompress, dim3(grid_for(n, 256)), dim3(256), 0, ctx->stream, d_compressed, n,
                           d_pks_out, d_pk_inf_out, d_status_out);
    });
}

// ------------------------------------------------------------------ host entry points
// ONE slice (n <= ctx->knobs.lane_slice, or a batch for the cooperative kernel) from host buffers.  A large one takes the shared
// upload + hash pipeline (ssa_ctx.hpp: pipelined_upload_hash), then ONE verification launch over the whole slice: the
// ladder kernel keeps its full-size grid, only the first chunk's upload is exposed, and the statuses come back through
// page-locked memory.
static int verify_many_host_one(ssa_ctx *ctx, const HostBatch &b, size_t n, uint32_t flags, uint8_t *status_out,
                                uint64_t *n_fail_out) {
    // (only the lane kernels read the hashes the pipeline leaves)
    return status_host_one(ctx, b, n, nullptr, !takes_coop(ctx, n, flags), true, status_out, n_fail_out,
                           [&](const StagedInputs &s, u8 *d_status, unsigned long long *d_fail) {
        HIP_TRY(hipMemsetAsync(d_fail, 0, sizeof(unsigned long long), ctx->stream));
        if (!s.hashed) return verify_launch(ctx, s.batch, n, flags, d_status, d_fail);
        // (the pipeline hashed the whole slice into ws_h, 32 B per lane, while it was uploading)
        return ssa_internal_verify_hashed(ctx, s.batch, (const uint64_t *)ctx->ws_h.p, n, flags, d_status, d_fail);
    });
}

extern "C" int ssa_verify_many(ssa_ctx *ctx, const uint8_t *sigs, const uint8_t *pks, const uint8_t *pk_inf,
                               const uint8_t *msgs, const uint64_t *msg_off, size_t msg_stride,
                               size_t msg_len, size_t n, uint32_t flags, uint8_t *status_out,
                               uint64_t *n_fail_out) {
    const HostBatch b{sigs, pks, pk_inf, msgs, msg_off, msg_stride, msg_len};
    if (int rc = check_host_batch(ctx, b, n, status_out)) return rc;
    if (n_fail_out) *n_fail_out = 0;
    if (n == 0) return 0;
    HIP_TRY(hipSetDevice(ctx->device));
    return run_host_slices_counted(ctx, b, n, ctx->knobs.lane_slice, n_fail_out,
                                   [&](ssa_ctx *c, size_t lo, size_t cnt, const HostBatch &s, uint64_t *nf) {
                                       return verify_many_host_one(c, s, cnt, flags, status_out + lo, nf);
                                   });
}

extern "C" int ssa_verify_batch(ssa_ctx *ctx, const uint8_t *sigs, const uint8_t *pks, const uint8_t *pk_inf,
                                const uint8_t *msgs, const uint64_t *msg_off, size_t msg_stride, size_t msg_len,
                                size_t n, uint32_t flags) {
    if (n == 0) return ctx ? SSA_OK : SSA_ERR_ARG;  // empty batch verifies (src/batch.rs)
    std::vector<uint8_t> status(n);
    uint64_t nf = 0;
    // the reference's verify_batch decompresses R with its flag byte (src/batch.rs:104)
    if (int rc = ssa_verify_many(ctx, sigs, pks, pk_inf, msgs, msg_off, msg_stride, msg_len, n,
                                 flags | SSA_FLAG_SIG_FLAG_BYTE, status.data(), &nf))
        return rc;
    if (nf == 0) return SSA_OK;
    // the reference panics on an undecodable input before it compares anything (src/batch.rs:67,104): SSA_MALFORMED
    // dominates; then the subgroup check of SSA_FLAG_CHECK_TORSION (an extension: src/batch.rs has none)
    bool any_pk = false;
    for (uint8_t s : status) {
        if (s == SSA_MALFORMED) return SSA_MALFORMED;
        any_pk = any_pk || s == SSA_INVALID_PUBLIC_KEY;
    }
    return any_pk ? SSA_INVALID_PUBLIC_KEY : SSA_INVALID_SIGNATURE;
}

extern "C" int ssa_verify(ssa_ctx *ctx, const uint8_t sig[SSA_SIGNATURE_LENGTH],
                          const uint8_t pk[SSA_AFFINE_PK_LENGTH], const uint8_t *msg, size_t msg_len,
                          uint32_t flags) {
    uint8_t st = SSA_MALFORMED;
    if (int rc = ssa_verify_many(ctx, sig, pk, nullptr, msg, nullptr, msg_len, msg_len, 1, flags, &st, nullptr))
        return rc;
    return st;
}

extern "C" int ssa_hash_message_many(ssa_ctx *ctx, const uint8_t *sigs, const uint8_t *pks, const uint8_t *msgs,
                                     const uint64_t *msg_off, size_t msg_stride, size_t msg_len, size_t n,
                                     uint8_t *digests_out) {
    if (!ctx || (n && (!sigs || !pks || !digests_out))) return SSA_ERR_ARG;
    if (int rc = check_msgs({msgs, msg_off, msg_stride, msg_len}, n)) return rc;
    if (int rc = check_host_offsets(msg_off, n)) return rc;
    if (n == 0) return 0;
    HostCall hc(ctx);
    const u8 *d_sigs = hc.in(ctx->st_sigs, sigs, n * 81), *d_pks = hc.in(ctx->st_pks, pks, n * 96);
    const MsgView mv = hc.msgs(msgs, msg_off, msg_stride, msg_len, n);
    u8 *d_out = hc.out(ctx->st_aux, digests_out, n * 32);
    return hc.finish([&] {
        return ssa_hash_message_many_device(ctx, d_sigs, d_pks, mv.msgs, mv.off, msg_stride, msg_len, n, d_out);
    });
}

extern "C" int ssa_rescue_hash_many(ssa_ctx *ctx, const uint64_t *felts, uint32_t felts_per_row, size_t n,
                                    uint64_t *digests_out) {
    if (!ctx || (n && (!digests_out || (felts_per_row && !felts)))) return SSA_ERR_ARG;
    if (n == 0) return 0;
    HostCall hc(ctx);
    const uint64_t *d_felts = hc.in<uint64_t>(ctx->st_aux, felts, n * (size_t)felts_per_row * 8);
    u8 *d_out = hc.out(ctx->st_aux2, digests_out, n * 32);
    return hc.finish([&] { return ssa_rescue_hash_many_device(ctx, d_felts, felts_per_row, n, (uint64_t *)d_out); });
}

extern "C" int ssa_keygen_sign_many(ssa_ctx *ctx, const uint8_t *sks, const uint8_t *nonces,
                                    const uint8_t *msgs, const uint64_t *msg_off, size_t msg_stride,
                                    size_t msg_len, size_t n, uint8_t *pks_out, uint8_t *sigs_out) {
    if (n && !pks_out) return SSA_ERR_ARG;
    return ssa_keygen_sign_many_ex(ctx, sks, nonces, msgs, msg_off, msg_stride, msg_len, n, 0u, pks_out, sigs_out);
}

extern "C" int ssa_decompress_many(ssa_ctx *ctx, const uint8_t *compressed, size_t n, uint8_t *pks_out,
                                   uint8_t *pk_inf_out, uint8_t *status_out) {
    if (!ctx || (n && (!compressed || !pks_out || !status_out))) return SSA_ERR_ARG;
    if (n == 0) return 0;
    HostCall hc(ctx);
    const u8 *d_in = hc.in(ctx->st_sigs, compressed, n * 49);
    u8 *d_pks = hc.out(ctx->st_aux, pks_out, n * 96), *d_inf = hc.out(ctx->st_aux2, pk_inf_out, n, 16),
       *d_status = hc.out(ctx->st_status, status_out, n, 16);
    return hc.finish([&] { return ssa_decompress_many_device(ctx, d_in, n, d_pks, d_inf, d_status); });
}

// one slice of KeyedSignature records (n <= ctx->knobs.lane_slice) from host buffers (b: the messages only)
static int verify_keyed_host_one(ssa_ctx *ctx, const uint8_t *keyed, const HostBatch &b, size_t n, uint32_t flags,
                                 uint8_t *status_out, uint64_t *n_fail_out) {
    HostCall hc(ctx);
    const u8 *d_keyed = hc.in(ctx->st_keyed, keyed, n * 130);
    u8 *d_sigs = hc.out(ctx->st_sigs, nullptr, n * 81), *d_pks = hc.out(ctx->st_pks, nullptr, n * 96),
       *d_inf = hc.out(ctx->st_inf, nullptr, n, 16), *d_status = hc.out(ctx->st_status, status_out, n, 16);
    hc.step([&] {
        hipLaunchKernelGGL(ssa_k_unpack_keyed, dim3(grid_for(n, 256)), dim3(256), 0, ctx->stream, d_keyed, n, d_pks, d_inf,
                           d_sigs);
        HIP_TRY(hipGetLastError());
        return 0;
    });
    const MsgView mv = hc.msgs(b.msgs, b.msg_off, b.msg_stride, b.msg_len, n);
    unsigned long long nf = 0, *d_fail = (unsigned long long *)ctx->ws_fail.p;
    hc.copy_back(&nf, d_fail, sizeof nf);
    if (int rc = hc.finish([&] {
            return ssa_internal_verify_many_device(ctx, d_sigs, d_pks, d_inf, mv.msgs, mv.off, b.msg_stride, b.msg_len, n, flags,
                                                   d_status, (uint64_t *)d_fail);
        }))
        return rc;
    if (n_fail_out) *n_fail_out = nf;
    return 0;
}

extern "C" int ssa_verify_keyed_many(ssa_ctx *ctx, const uint8_t *keyed, const uint8_t *msgs,
                                     const uint64_t *msg_off, size_t msg_stride, size_t msg_len, size_t n,
                                     uint32_t flags, uint8_t *status_out, uint64_t *n_fail_out) {
    if (!ctx || (n && (!keyed || !status_out))) return SSA_ERR_ARG;
    if (int rc = check_msgs({msgs, msg_off, msg_stride, msg_len}, n)) return rc;
    if (int rc = check_host_offsets(msg_off, n)) return rc;
    if (n_fail_out) *n_fail_out = 0;
    if (n == 0) return 0;
    HIP_TRY(hipSetDevice(ctx->device));
    const HostBatch b{nullptr, nullptr, nullptr, msgs, msg_off, msg_stride, msg_len};
    return run_host_slices_counted(ctx, b, n, ctx->knobs.lane_slice, n_fail_out,
                                   [&](ssa_ctx *c, size_t lo, size_t cnt, const HostBatch &s, uint64_t *nf) {
                                       return verify_keyed_host_one(c, keyed + 130 * lo, s, cnt, flags, status_out + lo, nf);
                                   });
}

// ------------------------------------------------------------------ keyed context

// ssa_k_keyset_build over m keys on the context's stream (every caller's launch; the key-table repair of
// ssa_keycheck.hpp lives in another translation unit)
int ssa_internal_keyset_build(ssa_ctx *ctx, const uint8_t *d_pks, const uint8_t *d_pk_inf, size_t m, uint64_t *d_tab,
                              uint8_t *d_status) {
    return timed_launch(ctx, "ssa_k_keyset_build", [&] {
        hipLaunchKernelGGL(ssa_k_keyset_build, dim3(grid_for(m, 256)), dim3(256), 0, ctx->stream, d_pks, d_pk_inf, m,
                           (u64 *)d_tab, d_status);
    });
}

extern "C" int ssa_keyset_create_device(ssa_ctx *ctx, const uint8_t *d_pks, const uint8_t *d_pk_inf, size_t m,
                                        uint32_t flags, ssa_keyset **out) {
    if (!ctx || !out || !d_pks || m == 0 || m > 0xffffffffull || flags > SSA_KEYSET_LADDER) return SSA_ERR_ARG;
    *out = nullptr;
    HIP_TRY(hipSetDevice(ctx->device));
    // owned here until it is registered and handed out: every early return destroys it
    std::unique_ptr<ssa_keyset, decltype(&ssa_keyset_destroy)> guard(new ssa_keyset(), ssa_keyset_destroy);
    ssa_keyset *ks = guard.get();
    ks->ctx = ctx;
    ks->m = m;
    if (ks->tab.reserve(m * (size_t)(PTAB_ENTRIES * PTAB_ENTRY_U64) * sizeof(u64)) || ks->status.reserve(m + 16) ||
        ks->pks.reserve(m * 96) || ks->inf.reserve(m + 16))
        return SSA_ERR_HIP;
    // the hash kernel reads the keys (x, y_0) through the index: keep a copy so that the caller's buffer can go; the
    // flags are kept beside them (all zero without d_pk_inf): bytes and flag are what ssa_keyset_selfcheck trusts
    HIP_TRY(hipMemcpyAsync(ks->pks.p, d_pks, m * 96, hipMemcpyDeviceToDevice, ctx->stream));
    HIP_TRY(d_pk_inf ? hipMemcpyAsync(ks->inf.p, d_pk_inf, m, hipMemcpyDeviceToDevice, ctx->stream)
                     : hipMemsetAsync(ks->inf.p, 0, m, ctx->stream));
    if (int rc = ssa_internal_keyset_build(ctx, (const u8 *)ks->pks.p, (const u8 *)ks->inf.p, m, (u64 *)ks->tab.p,
                                           (u8 *)ks->status.p))
        return rc;
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    // few keys: a comb table per key (no doublings at verification time); many keys: the ladder tables only
    // (100 MB per key: AUTO takes the combs while they fit the context's HBM budget and 16 GiB, and falls back to the
    // ladder tables when the allocation fails; SSA_KEYSET_COMB insists and reports the failure)
    const size_t comb_bytes = m * KTAB_ENTRIES_PER_KEY * 12 * sizeof(u64);
    const size_t comb_cap = ctx->hbm_budget < ((uint64_t)16 << 30) ? (size_t)ctx->hbm_budget : ((size_t)16 << 30);
    ks->comb = flags == SSA_KEYSET_COMB || (flags == SSA_KEYSET_AUTO && comb_bytes <= comb_cap);
    DevBuf kbase;                                      // 32 x 256 base rows (768 KB) per key, only while the combs are assembled
    if (ks->comb && (ks->ktab.reserve(comb_bytes) || kbase.reserve(m * KBASE_ENTRIES_PER_KEY * 12 * sizeof(u64)))) {
        kbase.release();
        ks->ktab.release();
        (void)hipGetLastError();
        if (flags == SSA_KEYSET_COMB) return SSA_ERR_HIP;
        ks->comb = false;
    }
    if (ks->comb) {
        const int rc = timed_launch(ctx, "ssa_k_keycomb_build", [&] {
            hipLaunchKernelGGL(ssa_k_keycomb_base, dim3(grid_for(m * KBASE_ENTRIES_PER_KEY, 256)), dim3(256), 0,
                               ctx->stream, (const u8 *)ks->pks.p, (const u8 *)ks->inf.p, (const u8 *)ks->status.p, m,
                               (u64 *)kbase.p);
            hipLaunchKernelGGL(ssa_k_keycomb_build, dim3(grid_for(m * (KTAB_ENTRIES_PER_KEY / 8), 256)), dim3(256), 0,
                               ctx->stream, (const u64 *)kbase.p, m, (u64 *)ks->ktab.p);
        });
        const bool synced = hipStreamSynchronize(ctx->stream) == hipSuccess;
        kbase.release();
        if (rc != 0 || !synced) return rc ? rc : SSA_ERR_HIP;
    }
    ctx->keysets.push_back(ks);
    *out = guard.release();
    return 0;
}

extern "C" int ssa_keyset_create(ssa_ctx *ctx, const uint8_t *pks, const uint8_t *pk_inf, size_t m, uint32_t flags,
                                 ssa_keyset **out) {
    if (!ctx || !out || !pks || m == 0) return SSA_ERR_ARG;
    HostCall hc(ctx);
    const u8 *d_pks = hc.in(ctx->st_pks, pks, m * 96), *d_inf = pk_inf ? hc.in(ctx->st_inf, pk_inf, m) : nullptr;
    return hc.finish([&] { return ssa_keyset_create_device(ctx, d_pks, d_inf, m, flags, out); });
}

extern "C" void ssa_keyset_destroy(ssa_keyset *ks) {
    if (!ks) return;
    if (ks->ctx) {
        (void)hipSetDevice(ks->ctx->device);
        (void)hipStreamSynchronize(ks->ctx->stream);
        forget_handle(ks->ctx->keysets, ks);
        ks->release_all();
    }
    delete ks;
}

extern "C" int ssa_keyset_status(ssa_keyset *ks, uint8_t *status_out) {
    if (!ks || !ks->ctx || !status_out) return SSA_ERR_ARG;
    HostCall hc(ks->ctx);
    hc.copy_back(status_out, ks->status.p, ks->m);
    return hc.finish([] { return 0; });
}

extern "C" int ssa_verify_many_indexed_device(ssa_ctx *ctx, ssa_keyset *ks, const uint32_t *d_key_idx,
                                              const uint8_t *d_sigs, const uint8_t *d_msgs, const uint64_t *d_msg_off,
                                              size_t msg_stride, size_t msg_len, size_t n, uint32_t flags,
                                              uint8_t *d_status_out, uint64_t *d_n_fail_out) {
    const MsgView mv{d_msgs, d_msg_off, msg_stride, msg_len};
    if (!ctx || !ks || ks->ctx != ctx || (n && (!d_key_idx || !d_sigs || !d_status_out))) return SSA_ERR_ARG;
    if (int rc = check_msgs(mv, n)) return rc;
    unsigned long long *d_fail;
    if (int rc = reset_fail_counter(ctx, d_n_fail_out, &d_fail)) return rc;
    if (n == 0) return 0;
    if (ctx->ws_h.reserve(n * 4 * sizeof(u64))) return SSA_ERR_HIP;
    int rc = timed_launch(ctx, "ssa_k_hash", [&] {
        hipLaunchKernelGGL(ssa_k_hash, dim3(grid_for(n, 256)), dim3(256), 0, ctx->stream, ctx->d_params, d_sigs,
                           (const u8 *)ks->pks.p, mv, n, (u64 *)ctx->ws_h.p, (u8 *)nullptr, d_key_idx, (u32)ks->m);
    });
    if (rc) return rc;
    if (ks->comb)
        return timed_launch(ctx, "ssa_k_verify_keyed", [&] {
            hipLaunchKernelGGL(ssa_k_verify_keyed_comb, dim3(grid_for(n, 256)), dim3(256), 0, ctx->stream, d_sigs,
                               d_key_idx, (const u64 *)ks->ktab.p, (const u8 *)ks->status.p, (u32)ks->m,
                               (const u64 *)ctx->ws_h.p, (const u64 *)ctx->d_gtab, n, flags, d_status_out, d_fail);
        });
    return timed_launch(ctx, "ssa_k_verify_keyed", [&] {
        hipLaunchKernelGGL(ssa_k_verify_keyed, dim3(grid_for(n, 256)), dim3(256), 0, ctx->stream, d_sigs, d_key_idx,
                           (const u64 *)ks->tab.p, (const u8 *)ks->status.p, (u32)ks->m, (const u64 *)ctx->ws_h.p,
                           (const u64 *)ctx->d_gtab, n, flags, d_status_out, d_fail);
    });
}

extern "C" int ssa_verify_many_indexed(ssa_ctx *ctx, ssa_keyset *ks, const uint32_t *key_idx, const uint8_t *sigs,
                                       const uint8_t *msgs, const uint64_t *msg_off, size_t msg_stride, size_t msg_len,
                                       size_t n, uint32_t flags, uint8_t *status_out, uint64_t *n_fail_out) {
    if (!ctx || !ks || ks->ctx != ctx || (n && (!key_idx || !sigs || !status_out))) return SSA_ERR_ARG;
    if (int rc = check_msgs({msgs, msg_off, msg_stride, msg_len}, n)) return rc;
    if (int rc = check_host_offsets(msg_off, n)) return rc;
    if (n_fail_out) *n_fail_out = 0;
    if (n == 0) return 0;
    HostCall hc(ctx);
    const u8 *d_sigs = hc.in(ctx->st_sigs, sigs, n * 81);
    const uint32_t *d_idx = hc.in<uint32_t>(ctx->st_aux, key_idx, n * sizeof(uint32_t));
    const MsgView mv = hc.msgs(msgs, msg_off, msg_stride, msg_len, n);
    u8 *d_status = hc.out(ctx->st_status, status_out, n, 16);
    unsigned long long nf = 0, *d_fail = (unsigned long long *)ctx->ws_fail.p;
    hc.copy_back(&nf, d_fail, sizeof nf);
    if (int rc = hc.finish([&] {
            return ssa_verify_many_indexed_device(ctx, ks, d_idx, d_sigs, mv.msgs, mv.off, msg_stride, msg_len, n, flags,
                                                  d_status, (uint64_t *)d_fail);
        }))
        return rc;
    if (n_fail_out) *n_fail_out = nf;
    return 0;
}

// ------------------------------------------------------------------ key dedup
// what the dedup entry points report (a CallStats of four words): distinct keys summed over slices, slices on the keyed
// route, slices that fell back, lanes that hit the probe bound
static void dedup_stats_add(CallStats *stats, uint64_t distinct, bool keyed, uint64_t bound_hits) {
    const uint64_t d[4] = {distinct, keyed ? 1u : 0u, keyed ? 0u : 1u, bound_hits};
    if (stats) stats->add(d);
}

static int dedup_fingerprint_key(ssa_ctx *ctx) {
    if (ctx->dedup_key_set) return 0;
    uint8_t *p = (uint8_t *)ctx->dedup_key;
    for (size_t got = 0; got < sizeof ctx->dedup_key;) {
        const ssize_t r = getrandom(p + got, sizeof ctx->dedup_key - got, 0);
        if (r <= 0) return SSA_ERR_HIP;
        got += (size_t)r;
    }
    ctx->dedup_key_set = true;
    return 0;
}

// the words of a key's table of sixteen multiples
constexpr size_t TAB_WORDS = (size_t)(PTAB_ENTRIES * PTAB_ENTRY_U64), TAB_BYTES = TAB_WORDS * sizeof(u64);

// Where the keys of a slice are, and with that what identifies a key (ssa_dedup.hpp): 96-byte affine keys with their
// optional pk_inf bytes, or (keyed non-null; the other two unused) the 49 compressed bytes of wire keys `stride` bytes
// apart: in front of 130-byte wire records (ssa_keyed.hpp), or side by side (stride 49: DESIGN.md section 23)
struct KeySource {
    const uint8_t *pks, *pk_inf, *keyed;
    uint32_t stride = 130;
};

// The distinct keys of cnt <= lane_slice lanes on ctx->stream, into the context's workspaces: dd_idx (a key index per
// lane), dd_reps (the representative lane of each key).  Synchronises the stream ONCE to read u and the number of lanes
// that hit the probe bound: the policy of the caller needs u on the host.
// A caller with a hook queues its own launches behind dd_k_index and in front of that read-back: they read u from
// d_stats[1] on the device, and what they leave in d_stats[2] and d_stats[3] comes back in the same copy (extra[]).
struct DedupHook {
    std::function<int(unsigned long long *d_stats)> queue;
    unsigned long long extra[2] = {0, 0};
};
static int dedup_slice(ssa_ctx *ctx, const KeySource &src, size_t cnt, uint64_t *u_out, uint64_t *bound_hits_out,
                       DedupHook *hook = nullptr) {
    if (int rc = dedup_fingerprint_key(ctx)) return rc;
    const size_t cap = dd_slots_for(cnt), nb = grid_for(cnt, DD_BLOCK);
    if (ctx->dd_slots.reserve(cap * sizeof(u64)) || ctx->dd_rep.reserve(cnt * sizeof(u32)) ||
        ctx->dd_num.reserve(cnt * sizeof(u32)) || ctx->dd_reps.reserve(cnt * sizeof(u32)) ||
        ctx->dd_idx.reserve(cnt * sizeof(u32)) || ctx->dd_blk.reserve(2 * nb * sizeof(u32)) || ctx->dd_stats.reserve(64))
        return SSA_ERR_HIP;
    unsigned long long *d_stats = (unsigned long long *)ctx->dd_stats.p;
    u32 *blk_cnt = (u32 *)ctx->dd_blk.p, *blk_off = blk_cnt + nb;
    int rc = timed_launch(ctx, "dedup", [&] {
        (void)hipMemsetAsync(ctx->dd_slots.p, 0xff, cap * sizeof(u64), ctx->stream);
        (void)hipMemsetAsync(d_stats, 0, (hook ? 4 : 2) * sizeof(unsigned long long), ctx->stream);
        const dim3 grid((unsigned)nb), block(DD_BLOCK);
        const u64 k0 = ctx->dedup_key[0], k1 = ctx->dedup_key[1];
        u64 *slots = (u64 *)ctx->dd_slots.p;
        const u32 mask = (u32)(cap - 1), bound = (u32)ctx->knobs.dedup_probe_bound;
        u32 *rep = (u32 *)ctx->dd_rep.p;
        if (src.keyed)
            hipLaunchKernelGGL(ky_k_insert, grid, block, 0, ctx->stream, src.keyed, src.stride, (u32)cnt, k0, k1, slots, mask,
                               bound, rep, blk_cnt, d_stats);
        else
            hipLaunchKernelGGL(dd_k_insert, grid, block, 0, ctx->stream, src.pks, src.pk_inf, (u32)cnt, k0, k1, slots, mask,
                               bound, rep, blk_cnt, d_stats);
        hipLaunchKernelGGL(dd_k_scan, dim3(1), dim3(DD_BLOCK), 0, ctx->stream, (const u32 *)blk_cnt, (u32)nb, blk_off,
                           d_stats);
        hipLaunchKernelGGL(dd_k_number, dim3((unsigned)nb), dim3(DD_BLOCK), 0, ctx->stream, (const u32 *)ctx->dd_rep.p,
                           (u32)cnt, (const u32 *)blk_off, (u32 *)ctx->dd_num.p, (u32 *)ctx->dd_reps.p);
        hipLaunchKernelGGL(dd_k_index, dim3((unsigned)nb), dim3(DD_BLOCK), 0, ctx->stream, (const u32 *)ctx->dd_rep.p,
                           (const u32 *)ctx->dd_num.p, (u32)cnt, (u32 *)ctx->dd_idx.p);
    });
    if (rc) return rc;
    if (hook)
        if ((rc = hook->queue(d_stats))) return rc;
    unsigned long long st[4] = {0, 0, 0, 0};
    HIP_TRY(hipMemcpyAsync(st, d_stats, (hook ? 4 : 2) * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (st[1] == 0 || st[1] > cnt) return SSA_ERR_HIP;      // (never: every lane has a representative)
    if (hook) {
        hook->extra[0] = st[2];
        hook->extra[1] = st[3];
    }
    *bound_hits_out = st[0];
    *u_out = st[1];
    return 0;
}

// Rows [0, m) of pks / inf (and of wire, unless nullptr: only a wire cache keeps the 49 bytes) from the keys of the
// representative lanes reps[0, m) of a slice of cnt lanes, and what ssa_k_verify does once per LANE done once per KEY
// over those rows: limb and curve checks, the subgroup check, the sixteen multiples -- status (0 / 1 / 3 per key) and
// tab.  Affine keys are copied (timed as `gather_stage`: the caller's), wire keys decompressed.
static int key_rows_build(ssa_ctx *ctx, const KeySource &src, const char *gather_stage, const u32 *reps, size_t m, size_t cnt,
                          u64 *pks, u8 *inf, u64 *wire, u64 *tab, u8 *status) {
    const int rc = timed_launch(ctx, src.keyed ? "ssa_k_keyed_decompress" : gather_stage, [&] {
        if (src.keyed)
            hipLaunchKernelGGL(ky_k_decompress, dim3(grid_for(m, 256)), dim3(256), 0, ctx->stream, src.keyed, src.stride, reps,
                               (u32)m, (u32)cnt, pks, inf, wire);
        else
            hipLaunchKernelGGL(dd_k_gather, dim3(grid_for(m * 12, DD_BLOCK)), dim3(DD_BLOCK), 0, ctx->stream, src.pks,
                               src.pk_inf, reps, (u32)m, pks, inf);
    });
    if (rc) return rc;
    return ssa_internal_keyset_build(ctx, (const u8 *)pks, (const u8 *)inf, m, tab, status);
}

// The u keys dedup_slice found in a slice of cnt lanes, compacted and checked once each, in the context's own
// workspaces: ctx->dd_pks, ctx->dd_inf, ctx->dd_kstatus and the tables in ctx->ws_tab (the lanes' table workspace: u
// tables never need more than one per lane)
static int dedup_check_keys(ssa_ctx *ctx, const KeySource &src, uint64_t u, size_t cnt) {
    if (ctx->dd_pks.reserve(u * 96) || ctx->dd_inf.reserve(u + 16) || ctx->dd_kstatus.reserve(u + 16) ||
        ctx->ws_tab.reserve(u * TAB_BYTES))
        return SSA_ERR_HIP;
    return key_rows_build(ctx, src, "dedup_gather", (const u32 *)ctx->dd_reps.p, (size_t)u, cnt, (u64 *)ctx->dd_pks.p,
                          (u8 *)ctx->dd_inf.p, nullptr, (u64 *)ctx->ws_tab.p, (u8 *)ctx->dd_kstatus.p);
}

// The two ends of the keyed route, shared with ssa_verify_many_screened (ssa_msm.hip), which puts
// the segmented MSM between them.  ssa_internal_dedup_keys: the distinct keys of one slice (cnt <= ctx->knobs.lane_slice
// lanes) checked once each: ctx->dd_idx (a key index per lane) and what dedup_check_keys leaves; synchronises the
// stream once, for u.
int ssa_internal_dedup_keys(ssa_ctx *ctx, const uint8_t *d_pks, const uint8_t *d_pk_inf, size_t cnt, uint64_t *u_out,
                            uint64_t *bound_hits_out) {
    const KeySource src{d_pks, d_pk_inf, nullptr};
    if (int rc = dedup_slice(ctx, src, cnt, u_out, bound_hits_out)) return rc;
    return dedup_check_keys(ctx, src, *u_out, cnt);
}

// ssa_k_verify_keyed over n lanes against the u keys dedup_check_keys left in the context; *d_fail is added to
int ssa_internal_verify_keyed(ssa_ctx *ctx, const uint8_t *d_sigs, const uint32_t *d_key_idx, uint64_t u,
                              const uint64_t *d_h, size_t n, uint32_t flags, uint8_t *d_status_out,
                              unsigned long long *d_fail) {
    return ssa_internal_verify_keyed_view(ctx, d_sigs, d_key_idx, ctx_key_view(ctx, u), d_h, n, flags, d_status_out, d_fail);
}

// the same against keys named by a view: the lanes' key numbers are d_lane_key (the view's own, or a gathered copy)
int ssa_internal_verify_keyed_view(ssa_ctx *ctx, const uint8_t *d_sigs, const uint32_t *d_lane_key, const KeyView &kv,
                                   const uint64_t *d_h, size_t n, uint32_t flags, uint8_t *d_status_out,
                                   unsigned long long *d_fail) {
    return timed_launch(ctx, "ssa_k_verify_keyed", [&] {
        hipLaunchKernelGGL(ssa_k_verify_keyed, dim3(grid_for(n, 256)), dim3(256), 0, ctx->stream, d_sigs, d_lane_key,
                           (const u64 *)kv.tab, (const u8 *)kv.status, (u32)kv.n_keys, (const u64 *)d_h,
                           (const u64 *)ctx->d_gtab, n, flags, d_status_out, d_fail);
    });
}

// ONE slice (cnt <= ctx->knobs.lane_slice lanes) of the lane kernels' route on ctx->stream with ctx's workspaces; hashed: the
// challenge scalars are already in ctx->ws_h.  *d_fail is added to.
static int dedup_verify_slice(ssa_ctx *ctx, const DevBatch &b, size_t cnt, uint32_t flags, bool hashed,
                              uint8_t *d_status_out, unsigned long long *d_fail, CallStats *stats) {
    const double ratio = ctx->knobs.dedup_ratio[(flags & SSA_FLAG_CHECK_TORSION) ? 1 : 0];
    uint64_t u = cnt, hits = 0;
    // (a threshold of 0 sends every slice to the fallback: the keys are then counted only for the statistics)
    if (ratio > 0 || stats)
        if (int rc = dedup_slice(ctx, {b.pks, b.pk_inf, nullptr}, cnt, &u, &hits)) return rc;
    const bool keyed = (double)u < ratio * (double)cnt;
    dedup_stats_add(stats, u, keyed, hits);
    if (!keyed) {       // (nearly) every key is distinct: the path of ssa_verify_many
        if (!hashed) return verify_one_slice(ctx, b, cnt, flags, d_status_out, d_fail);
        if (ctx->ws_tab.reserve(cnt * TAB_BYTES)) return SSA_ERR_HIP;
        return verify_slices(ctx, b, (const u64 *)ctx->ws_h.p, cnt, flags, d_status_out, d_fail);
    }
    if (int rc = dedup_check_keys(ctx, {b.pks, b.pk_inf, nullptr}, u, cnt)) return rc;
    if (ctx->ws_h.reserve(cnt * 4 * sizeof(u64))) return SSA_ERR_HIP;
    if (!hashed) {
        const int rc = timed_launch(ctx, "ssa_k_hash", [&] {
            hipLaunchKernelGGL(ssa_k_hash, dim3(grid_for(cnt, 256)), dim3(256), 0, ctx->stream, ctx->d_params, b.sigs, b.pks,
                               b.msgs, cnt, (u64 *)ctx->ws_h.p, (u8 *)nullptr, (const u32 *)nullptr, 0u);
        });
        if (rc) return rc;
    }
    return ssa_internal_verify_keyed(ctx, b.sigs, (const u32 *)ctx->dd_idx.p, u, (const uint64_t *)ctx->ws_h.p, cnt, flags,
                                     d_status_out, d_fail);
}

// A batch for the cooperative kernel takes the path of ssa_verify_many unchanged; its keys are counted, slice by slice,
// only for a caller that asked for the statistics.
static int dedup_count_only(ssa_ctx *ctx, const DevBatch &b, size_t n, CallStats *stats) {
    if (!stats) return 0;
    return for_dev_slices(b, n, ctx->knobs.lane_slice, [&](size_t, size_t cnt, const DevBatch &s) {
        uint64_t u = 0, hits = 0;
        if (int rc = dedup_slice(ctx, {s.pks, s.pk_inf, nullptr}, cnt, &u, &hits)) return rc;
        dedup_stats_add(stats, u, false, hits);
        return 0;
    });
}

extern "C" int ssa_verify_many_dedup_device(ssa_ctx *ctx, const uint8_t *d_sigs, const uint8_t *d_pks,
                                            const uint8_t *d_pk_inf, const uint8_t *d_msgs, const uint64_t *d_msg_off,
                                            size_t msg_stride, size_t msg_len, size_t n, uint32_t flags,
                                            uint8_t *d_status_out, uint64_t *d_n_fail_out, uint64_t stats_out[4]) {
    const DevBatch b{d_sigs, d_pks, d_pk_inf, {d_msgs, d_msg_off, msg_stride, msg_len}};
    if (int rc = check_dev_batch(ctx, b, n, d_status_out)) return rc;
    CallStats st(4);
    st.out(stats_out);      // (still empty: the caller's words are zeroed)
    unsigned long long *d_fail;
    if (int rc = reset_fail_counter(ctx, d_n_fail_out, &d_fail)) return rc;
    if (n == 0) return 0;
    int rc = 0;
    if (takes_coop(ctx, n, flags)) {
        rc = dedup_count_only(ctx, b, n, stats_out ? &st : nullptr);
        if (rc == 0) rc = verify_launch(ctx, b, n, flags, d_status_out, d_fail);
    } else {
        // slice after slice on the context's stream (each slice's policy waits for its u: the slices of this form do not
        // alternate between two streams)
        rc = for_dev_slices(b, n, ctx->knobs.lane_slice, [&](size_t lo, size_t cnt, const DevBatch &s) {
            return dedup_verify_slice(ctx, s, cnt, flags, false, d_status_out + lo, d_fail, stats_out ? &st : nullptr);
        });
    }
    if (rc) return rc;
    st.out(stats_out);
    return 0;
}

// ONE slice from host buffers: the shell of verify_many_host_one (status_host_one) around the dedup pipeline
static int dedup_host_one(ssa_ctx *ctx, const HostBatch &b, size_t n, uint32_t flags, uint8_t *status_out,
                          uint64_t *n_fail_out, CallStats *stats) {
    const bool lane_kernels = !takes_coop(ctx, n, flags);
    return status_host_one(ctx, b, n, nullptr, lane_kernels, true, status_out, n_fail_out,
                           [&](const StagedInputs &s, u8 *d_status, unsigned long long *d_fail) {
        HIP_TRY(hipMemsetAsync(d_fail, 0, sizeof(unsigned long long), ctx->stream));
        if (lane_kernels) return dedup_verify_slice(ctx, s.batch, n, flags, s.hashed, d_status, d_fail, stats);
        if (int r = dedup_count_only(ctx, s.batch, n, stats)) return r;
        return verify_launch(ctx, s.batch, n, flags, d_status, d_fail);
    });
}

extern "C" int ssa_verify_many_dedup(ssa_ctx *ctx, const uint8_t *sigs, const uint8_t *pks, const uint8_t *pk_inf,
                                     const uint8_t *msgs, const uint64_t *msg_off, size_t msg_stride, size_t msg_len,
                                     size_t n, uint32_t flags, uint8_t *status_out, uint64_t *n_fail_out,
                                     uint64_t stats_out[4]) {
    const HostBatch b{sigs, pks, pk_inf, msgs, msg_off, msg_stride, msg_len};
    if (int rc = check_host_batch(ctx, b, n, status_out)) return rc;
    if (n_fail_out) *n_fail_out = 0;
    CallStats st(4);
    st.out(stats_out);      // (still empty: the caller's words are zeroed)
    if (n == 0) return 0;
    HIP_TRY(hipSetDevice(ctx->device));
    const int rc = run_host_slices_counted(ctx, b, n, ctx->knobs.lane_slice, n_fail_out,
                                           [&](ssa_ctx *c, size_t lo, size_t cnt, const HostBatch &s, uint64_t *nf) {
                                               return dedup_host_one(c, s, cnt, flags, status_out + lo, nf,
                                                                     stats_out ? &st : nullptr);
                                           });
    if (rc) return rc;
    st.out(stats_out);
    return 0;
}

extern "C" int ssa_debug_dedup_device(ssa_ctx *ctx, const uint8_t *d_pks, const uint8_t *d_pk_inf, size_t n,
                                      uint32_t *d_key_idx_out, uint64_t out[2]) {
    if (!ctx || !d_pks || !out || n == 0 || n > SSA_MAX_BATCH || n > ctx->knobs.lane_slice) return SSA_ERR_ARG;
    HIP_TRY(hipSetDevice(ctx->device));
    if (int rc = dedup_slice(ctx, {d_pks, d_pk_inf, nullptr}, n, &out[0], &out[1])) return rc;
    if (d_key_idx_out) {
        HIP_TRY(hipMemcpyAsync(d_key_idx_out, ctx->dd_idx.p, n * sizeof(uint32_t), hipMemcpyDeviceToDevice, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
    }
    return 0;
}

extern "C" int ssa_debug_dedup_config(ssa_ctx *ctx, double max_distinct_ratio, uint32_t probe_bound) {
    if (!ctx || max_distinct_ratio > 2.0 || max_distinct_ratio != max_distinct_ratio) return SSA_ERR_ARG;
    ctx->knobs.dedup_ratio[0] = max_distinct_ratio < 0 ? DEDUP_RATIO_NO_CHECK : max_distinct_ratio;
    ctx->knobs.dedup_ratio[1] = max_distinct_ratio < 0 ? DEDUP_RATIO_CHECK : max_distinct_ratio;
    ctx->knobs.dedup_probe_bound = probe_bound ? probe_bound : DEDUP_PROBE_BOUND;
    return 0;
}

// ------------------------------------------------------------------ key cache
extern "C" int ssa_keycache_create(ssa_ctx *ctx, size_t capacity, ssa_keycache **out) {
    return ssa_keycache_create_ex(ctx, capacity, 0u, out);
}

extern "C" int ssa_keycache_create_ex(ssa_ctx *ctx, size_t capacity, uint32_t flags, ssa_keycache **out) {
    if (out) *out = nullptr;
    if (flags & ~SSA_KEYCACHE_WIRE) return SSA_ERR_ARG;
    if (!ctx || !out || capacity == 0 || capacity > KC_MAX_CAPACITY) return SSA_ERR_ARG;
    HIP_TRY(hipSetDevice(ctx->device));
    ssa_keycache *kc = new ssa_keycache();
    kc->ctx = ctx;
    kc->capacity = capacity;
    kc->n_slots = dd_slots_for(capacity);
    kc->wire_mode = (flags & SSA_KEYCACHE_WIRE) != 0;
    kc->rows.ctx = ctx;
    kc->rows.m = capacity;
    // everything the cache will ever hold, now: no call that uses it allocates for it
    if (kc->rows.tab.reserve_exact(capacity * TAB_BYTES) || kc->rows.status.reserve_exact(capacity + 16) ||
        kc->rows.pks.reserve_exact(capacity * 96) || kc->inf.reserve_exact(capacity + 16) ||
        kc->slots.reserve_exact(kc->n_slots * sizeof(u64)) ||
        (kc->wire_mode && kc->wire.reserve_exact(capacity * KY_WIRE_WORDS * sizeof(u64))) ||
        hipMemsetAsync(kc->slots.p, 0xff, kc->n_slots * sizeof(u64), ctx->stream) != hipSuccess ||
        hipStreamSynchronize(ctx->stream) != hipSuccess) {
        (void)hipGetLastError();
        kc->release_all();
        delete kc;
        return SSA_ERR_HIP;
    }
    ctx->keycaches.push_back(kc);
    *out = kc;
    return 0;
}

extern "C" void ssa_keycache_destroy(ssa_keycache *kc) {
    if (!kc) return;
    if (kc->ctx) {
        (void)hipSetDevice(kc->ctx->device);
        (void)hipStreamSynchronize(kc->ctx->stream);
        forget_handle(kc->ctx->keycaches, kc);
        kc->release_all();
    }
    delete kc;
}

// every slot empty again, on the context's stream (behind whatever still reads the cache): the rows stay where they are
// and are handed out again from row 0
static int keycache_reset(ssa_keycache *kc) {
    HIP_TRY(hipMemsetAsync(kc->slots.p, 0xff, kc->n_slots * sizeof(u64), kc->ctx->stream));
    kc->held = 0;
    kc->clears++;
    return 0;
}

extern "C" int ssa_keycache_clear(ssa_keycache *kc) {
    if (!kc || !kc->ctx) return SSA_ERR_ARG;
    HIP_TRY(hipSetDevice(kc->ctx->device));
    return keycache_reset(kc);
}

extern "C" int ssa_keycache_info(ssa_keycache *kc, uint64_t out[4]) {
    if (!kc || !kc->ctx || !out) return SSA_ERR_ARG;
    out[0] = kc->capacity;
    out[1] = kc->held;
    out[2] = kc->clears;
    out[3] = kc->device_bytes();
    return 0;
}

extern "C" int ssa_debug_keycache_plan(uint64_t capacity, uint64_t held, uint64_t u, uint64_t m, uint32_t *plan_out) {
    if (!plan_out || capacity == 0 || capacity > KC_MAX_CAPACITY || held > capacity || m > u || u > SSA_MAX_BATCH)
        return SSA_ERR_ARG;
    *plan_out = (uint32_t)kc_plan(capacity, held, u, m);
    return 0;
}

extern "C" int ssa_debug_keycache_keep(uint64_t capacity, uint64_t u, uint64_t m, const uint64_t hist[64],
                                       uint64_t out[2]) {
    if (!hist || !out || capacity == 0 || capacity > KC_MAX_CAPACITY || m > u || u > capacity) return SSA_ERR_ARG;
    uint64_t total = 0;
    for (int a = 0; a < KC_AGE_BINS; a++) {
        if (hist[a] > capacity) return SSA_ERR_ARG;
        total += hist[a];
    }
    if (total > capacity) return SSA_ERR_ARG;      // more rows than the cache has
    uint64_t age = 0, kept = 0;
    if (!kc_keep(capacity, u, m, hist, &age, &kept)) return SSA_ERR_ARG;      // hist[0] > u - m: no slice leaves that
    out[0] = age;
    out[1] = kept;
    return 0;
}

// ------------------------------------------------------------------ eviction by compaction
// The compaction's scratch, sized for `capacity` rows when the policy is chosen: two totals of dd_k_scan, the 64 age
// counts, remap[] and the lists of holes and movers (a u32 per row each), and per workgroup of rows two counts and two
// offsets
struct EvictWs {
    unsigned long long *totals;
    u32 *hist, *remap, *holes, *movers, *blk;
    size_t nb_max;
};
static size_t evict_ws_bytes(size_t capacity) {
    return 512 + (3 * capacity + 4 * (size_t)grid_for(capacity, DD_BLOCK)) * sizeof(u32);
}
static EvictWs evict_ws_of(ssa_keycache *kc) {
    u8 *p = (u8 *)kc->evict_ws.p;
    EvictWs w;
    w.totals = (unsigned long long *)p;
    w.hist = (u32 *)(p + 64);
    w.remap = (u32 *)(p + 512);
    w.holes = w.remap + kc->capacity;
    w.movers = w.holes + kc->capacity;
    w.blk = w.movers + kc->capacity;
    w.nb_max = grid_for(kc->capacity, DD_BLOCK);
    return w;
}

extern "C" int ssa_keycache_set_eviction(ssa_keycache *kc, uint32_t policy) {
    if (!kc || !kc->ctx || (policy != SSA_KEYCACHE_EVICT_CLEAR && policy != SSA_KEYCACHE_EVICT_RECENT)) return SSA_ERR_ARG;
    if (policy == SSA_KEYCACHE_EVICT_RECENT && kc->policy != policy) {
        HIP_TRY(hipSetDevice(kc->ctx->device));
        // everything the policy will ever need, now: no call that uses the cache allocates for it
        if (!kc->stamps.p &&
            (kc->stamps.reserve_exact(kc->capacity * sizeof(u32)) || kc->evict_ws.reserve_exact(evict_ws_bytes(kc->capacity)))) {
            (void)hipGetLastError();
            kc->stamps.release();
            kc->evict_ws.release();
            return SSA_ERR_HIP;
        }
        // the rows already held count as used now
        if (kc->held)
            HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)kc->stamps.p, (int)(u32)kc->epoch, kc->held, kc->ctx->stream));
    }
    kc->policy = policy;
    return 0;
}

extern "C" int ssa_keycache_eviction_info(ssa_keycache *kc, uint64_t out[8]) {
    if (!kc || !kc->ctx || !out) return SSA_ERR_ARG;
    out[0] = kc->policy;
    out[1] = kc->compactions;
    out[2] = kc->dropped;
    out[3] = kc->last_kept;
    out[4] = kc->last_moved;
    out[5] = kc->epoch;
    out[6] = out[7] = 0;
    return 0;
}

// Rows [base, base + m) of the cache, complete, get their slots (kc_k_publish / ky_k_publish: *d_unpublished += rows
// that found none).  A bare launch: the caller times it.
static void keycache_publish_launch(ssa_ctx *ctx, ssa_keycache *kc, size_t base, size_t m, unsigned long long *d_unpublished) {
    const dim3 grid(grid_for(m, DD_BLOCK)), block(DD_BLOCK);
    const u64 k0 = ctx->dedup_key[0], k1 = ctx->dedup_key[1];
    u64 *slots = (u64 *)kc->slots.p;
    const u32 mask = (u32)(kc->n_slots - 1), bound = (u32)ctx->knobs.dedup_probe_bound;
    if (kc->wire_mode)
        hipLaunchKernelGGL(ky_k_publish, grid, block, 0, ctx->stream, (const u64 *)kc->wire.p, (u32)base, (u32)m, k0, k1, slots,
                           mask, bound, d_unpublished);
    else
        hipLaunchKernelGGL(kc_k_publish, grid, block, 0, ctx->stream, (const u64 *)kc->rows.pks.p, (const u8 *)kc->inf.p,
                           (u32)base, (u32)m, k0, k1, slots, mask, bound, d_unpublished);
}

// A full SSA_KEYCACHE_EVICT_RECENT cache makes room for the m misses of a slice of u distinct keys (m <= u <= capacity,
// held + m > capacity): the rows used most recently stay, packed into rows [0, K), the slots are rebuilt over them and
// the slice's found[] follows its hits to their new rows; kc->held = K.  Two read-backs (the ages, the number of rows to
// move): a compaction is the rare path.  *done = false, and nothing changed, when the ages say that no keep rule
// applies (kc_keep): the caller clears.
static int keycache_compact(ssa_ctx *ctx, ssa_keycache *kc, uint64_t u, uint64_t m, u32 *found,
                            unsigned long long *d_unpublished, bool *done) {
    static_assert(TAB_WORDS % 2 == 0 && KY_WIRE_WORDS <= 16, "kc_k_evict_move");
    *done = false;
    const EvictWs w = evict_ws_of(kc);
    const u32 held = (u32)kc->held, epoch = (u32)kc->epoch, nb = grid_for(held, DD_BLOCK);
    if (held == 0 || held > kc->capacity || nb > w.nb_max) return SSA_ERR_HIP;      // (never: the plan saw held + m > capacity)
    u32 *stamps = (u32 *)kc->stamps.p, *hole_cnt = w.blk, *mover_cnt = hole_cnt + w.nb_max, *hole_off = mover_cnt + w.nb_max,
        *mover_off = hole_off + w.nb_max;
    int rc = timed_launch(ctx, "keycache_compact", [&] {
        (void)hipMemsetAsync(kc->evict_ws.p, 0, 512, ctx->stream);
        hipLaunchKernelGGL(kc_k_age_hist, dim3(nb), dim3(DD_BLOCK), 0, ctx->stream, (const u32 *)stamps, held, epoch, w.hist);
    });
    if (rc) return rc;
    u32 h32[KC_AGE_BINS];
    HIP_TRY(hipMemcpyAsync(h32, w.hist, sizeof h32, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    uint64_t hist[KC_AGE_BINS], age = 0, kept = 0, total = 0;
    for (int a = 0; a < KC_AGE_BINS; a++) total += hist[a] = h32[a];
    if (total != held) return SSA_ERR_HIP;      // (never)
    if (!kc_keep(kc->capacity, u, m, hist, &age, &kept)) return 0;
    const u32 K = (u32)kept, max_age = (u32)age;
    rc = timed_launch(ctx, "keycache_compact", [&] {
        hipLaunchKernelGGL(kc_k_evict_count, dim3(nb), dim3(DD_BLOCK), 0, ctx->stream, (const u32 *)stamps, held, epoch,
                           max_age, K, hole_cnt, mover_cnt);
        hipLaunchKernelGGL(dd_k_scan, dim3(1), dim3(DD_BLOCK), 0, ctx->stream, (const u32 *)hole_cnt, nb, hole_off, w.totals);
        hipLaunchKernelGGL(dd_k_scan, dim3(1), dim3(DD_BLOCK), 0, ctx->stream, (const u32 *)mover_cnt, nb, mover_off,
                           w.totals + 1);
    });
    if (rc) return rc;
    unsigned long long tot[3] = {0, 0, 0};
    HIP_TRY(hipMemcpyAsync(tot, w.totals, sizeof tot, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    const u32 n_move = (u32)tot[1];
    if (tot[1] != tot[2] || tot[1] > K || tot[1] > held - K) return SSA_ERR_HIP;      // (never: as many holes as movers)
    rc = timed_launch(ctx, "keycache_compact", [&] {
        hipLaunchKernelGGL(kc_k_evict_assign, dim3(nb), dim3(DD_BLOCK), 0, ctx->stream, (const u32 *)stamps, held, epoch,
                           max_age, K, (const u32 *)hole_off, (const u32 *)mover_off, (u32)kc->capacity, w.holes, w.movers,
                           w.remap);
        if (n_move)
            hipLaunchKernelGGL(kc_k_evict_move, dim3(grid_for(n_move, DD_BLOCK / 64)), dim3(DD_BLOCK), 0, ctx->stream,
                               (const u32 *)w.movers, (const u32 *)w.holes, n_move, held, K, (u32)TAB_WORDS, (u64 *)kc->rows.tab.p,
                               (u64 *)kc->rows.pks.p, (u8 *)kc->inf.p, (u8 *)kc->rows.status.p, stamps, (u64 *)kc->wire.p,
                               kc->wire_mode ? (u32)KY_WIRE_WORDS : 0u, w.remap);
        (void)hipMemsetAsync(kc->slots.p, 0xff, kc->n_slots * sizeof(u64), ctx->stream);
        if (K) keycache_publish_launch(ctx, kc, 0, K, d_unpublished);
        hipLaunchKernelGGL(kc_k_remap, dim3(grid_for(u, DD_BLOCK)), dim3(DD_BLOCK), 0, ctx->stream, found, (u32)u,
                           (const u32 *)w.remap, held);
    });
    if (rc) return rc;
    kc->compactions++;
    kc->dropped += held - K;
    kc->last_kept = K;
    kc->last_moved = n_move;
    kc->held = K;
    *done = true;
    return 0;
}

// Where the keys of a slice that uses the cache go (plan: KC_PLAN_INSERT or KC_PLAN_CLEAR), the ONE place that handles a
// full cache, for affine and wire caches alike: the m misses behind the rows held; or, the cache being full, behind the
// rows a compaction kept (SSA_KEYCACHE_EVICT_RECENT); or all u keys of the slice from row 0 of a cleared cache (key j of
// the dedup takes row j).  ks[0..2] = hits, keys to insert, automatic evictions.
struct KcPlace {
    size_t base = 0, fresh = 0;
    const u32 *reps = nullptr;      // the representative lanes of the keys to insert
    bool all_new = false;           // the cache was cleared for this slice
    bool republished = false;       // a compaction published rows again: *d_unpublished counts
};
static int keycache_place(ssa_ctx *ctx, ssa_keycache *kc, int plan, uint64_t u, uint64_t m, u32 *found, const u32 *miss_rep,
                          unsigned long long *d_unpublished, uint64_t ks[4], KcPlace *pl) {
    pl->base = kc->held;
    pl->fresh = (size_t)m;
    pl->reps = miss_rep;
    if (plan == KC_PLAN_CLEAR) {
        bool compacted = false;
        if (kc->policy == SSA_KEYCACHE_EVICT_RECENT)
            if (int rc = keycache_compact(ctx, kc, u, m, found, d_unpublished, &compacted)) return rc;
        if (compacted) {
            pl->base = kc->held;
            pl->republished = kc->held > 0;
        } else {
            if (int rc = keycache_reset(kc)) return rc;
            pl->base = 0;
            pl->fresh = (size_t)u;
            pl->reps = (const u32 *)ctx->dd_reps.p;
            pl->all_new = true;
        }
        ks[2] = 1;
    }
    ks[0] = u - pl->fresh;
    ks[1] = pl->fresh;
    return 0;
}

// rows base .. base + fresh are built and published: they are held, and used now
static int keycache_placed(ssa_keycache *kc, const KcPlace &pl) {
    kc->held = pl.base + pl.fresh;
    if (kc->policy == SSA_KEYCACHE_EVICT_RECENT && pl.fresh)
        HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)((u32 *)kc->stamps.p + pl.base), (int)(u32)kc->epoch, pl.fresh,
                                  kc->ctx->stream));
    return 0;
}

// the stamps and the epoch a look-up writes on its hits: a new epoch per slice under SSA_KEYCACHE_EVICT_RECENT, else none
static u32 *keycache_new_epoch(ssa_keycache *kc) {
    if (kc->policy != SSA_KEYCACHE_EVICT_RECENT) return nullptr;
    kc->epoch++;
    return (u32 *)kc->stamps.p;
}

// The look-up of a slice's u distinct keys (u is read from d_stats[1] on the device) in the cache: found[j] = the row of
// key j or KC_MISS_BIT | its number among the misses, miss_rep[t] = the representative lane of miss t, d_stats[2] = m.
// Rows hit get the cache's epoch in stamps (nullptr: the policy keeps none).
static int keycache_lookup(ssa_ctx *ctx, ssa_keycache *kc, const KeySource &src, size_t cnt, unsigned long long *d_stats,
                           u32 *found, u32 *miss_rep, u32 *blk_cnt, u32 *stamps) {
    const size_t nb = grid_for(cnt, DD_BLOCK);
    u32 *blk_off = blk_cnt + nb;
    return timed_launch(ctx, "keycache_lookup", [&] {
        const dim3 grid((unsigned)nb), block(DD_BLOCK);
        const u32 *reps = (const u32 *)ctx->dd_reps.p;
        const unsigned long long *stats = d_stats;
        const u64 k0 = ctx->dedup_key[0], k1 = ctx->dedup_key[1];
        const u64 *slots = (const u64 *)kc->slots.p;
        const u32 mask = (u32)(kc->n_slots - 1), bound = (u32)ctx->knobs.dedup_probe_bound, held = (u32)kc->held,
                  epoch = (u32)kc->epoch;
        if (src.keyed)
            hipLaunchKernelGGL(ky_k_lookup, grid, block, 0, ctx->stream, src.keyed, src.stride, reps, (u32)cnt, stats, k0, k1,
                               slots, mask, bound, (const u64 *)kc->wire.p, held, found, blk_cnt, stamps, epoch);
        else
            hipLaunchKernelGGL(kc_k_lookup, grid, block, 0, ctx->stream, src.pks, src.pk_inf, reps, (u32)cnt, stats, k0, k1,
                               slots, mask, bound, (const u64 *)kc->rows.pks.p, (const u8 *)kc->inf.p, held, found, blk_cnt,
                               stamps, epoch);
        hipLaunchKernelGGL(dd_k_scan, dim3(1), dim3(DD_BLOCK), 0, ctx->stream, (const u32 *)blk_cnt, (u32)nb, blk_off,
                           d_stats + 1);
        hipLaunchKernelGGL(kc_k_number, grid, block, 0, ctx->stream, reps, (u32)cnt, stats, (const u32 *)blk_off, found,
                           miss_rep);
    });
}

// ONE slice of cnt lanes through the cache, for affine keys and wire records alike (a wire cache for wire records: the
// callers check): the distinct keys found and looked up, the misses checked and inserted -- or the cache cleared or
// compacted first, or bypassed (kc_plan).  One synchronisation, the one of the dedup.  For wire records the signatures
// are split off in front and every lane's key bytes and flag expanded out of the rows behind: *b (required for records,
// unused otherwise).  Dense wire keys (src.stride == 49: no records, nothing to split) are not expanded here either: *rows
// says where the rows are that kv->lane_key numbers -- the cache's, or under a bypass the context's own -- and the
// caller gathers from them.
struct KeyRows {
    const u64 *pks;
    const u8 *inf;
};
static int keycache_slice(ssa_ctx *ctx, ssa_keycache *kc, const KeySource &src, size_t cnt, DevBatch *b, KeyView *kv,
                          uint64_t *u_out, uint64_t *bound_hits_out, uint64_t ks[4], const unsigned long long **d_unpublished,
                          KeyRows *rows = nullptr) {
    const bool records = src.keyed != nullptr && src.stride == 130;
    if (records && !b) return SSA_ERR_ARG;
    const size_t nb = grid_for(cnt, DD_BLOCK);
    if (ctx->kc_found.reserve(cnt * sizeof(u32)) || ctx->kc_missrep.reserve(cnt * sizeof(u32)) ||
        ctx->kc_blk.reserve(2 * nb * sizeof(u32)) || ctx->kc_lane_row.reserve(cnt * sizeof(u32)))
        return SSA_ERR_HIP;
    if (records && (ctx->ky_sigs.reserve(cnt * 81 + 16) || ctx->ky_pks.reserve(cnt * 96) || ctx->ky_inf.reserve(cnt + 16)))
        return SSA_ERR_HIP;
    u32 *found = (u32 *)ctx->kc_found.p, *miss_rep = (u32 *)ctx->kc_missrep.p;
    int rc = 0;
    if (records) {
        rc = timed_launch(ctx, "keyed_split", [&] {
            hipLaunchKernelGGL(ky_k_split, dim3(grid_for((cnt * 81 + 3) / 4, 256)), dim3(256), 0, ctx->stream, src.keyed, cnt,
                               (u8 *)ctx->ky_sigs.p);
        });
        if (rc) return rc;
    }
    const size_t held = kc->held;
    u32 *stamps = keycache_new_epoch(kc);
    DedupHook hook;
    // d_stats: [0] lanes at the probe bound, [1] u, [2] m (dd_k_scan writes its total one word on), [3] unpublished rows
    hook.queue = [&](unsigned long long *d_stats) {
        return keycache_lookup(ctx, kc, src, cnt, d_stats, found, miss_rep, (u32 *)ctx->kc_blk.p, stamps);
    };
    uint64_t u = 0;
    if ((rc = dedup_slice(ctx, src, cnt, &u, bound_hits_out, &hook))) return rc;
    const uint64_t m = hook.extra[0];
    if (m > u) return SSA_ERR_HIP;      // (never)
    *u_out = u;
    ks[0] = ks[1] = ks[2] = ks[3] = 0;
    *d_unpublished = nullptr;
    const int plan = kc_plan(kc->capacity, held, u, m);
    u64 *c_pks = (u64 *)kc->rows.pks.p;
    u8 *c_inf = (u8 *)kc->inf.p;
    const u64 *row_pks = c_pks;       // the rows kv->lane_key numbers
    const u8 *row_inf = c_inf;
    if (plan == KC_PLAN_BYPASS) {       // more keys than rows: the u keys into the context's own workspaces
        ks[3] = 1;
        if ((rc = dedup_check_keys(ctx, src, u, cnt))) return rc;
        *kv = ctx_key_view(ctx, u);
        row_pks = (const u64 *)ctx->dd_pks.p;
        row_inf = (const u8 *)ctx->dd_inf.p;
    } else {
        unsigned long long *d_unpub = (unsigned long long *)ctx->dd_stats.p + 3;
        KcPlace pl;
        if ((rc = keycache_place(ctx, kc, plan, u, m, found, miss_rep, d_unpub, ks, &pl))) return rc;
        const size_t base = pl.base, fresh = pl.fresh;
        if (fresh) {        // rows base .. base + fresh: the keys, their checks and tables, then (complete) their slots
            if ((rc = key_rows_build(ctx, src, "keycache_insert", pl.reps, fresh, cnt, c_pks + 12 * base, c_inf + base,
                                     src.keyed ? (u64 *)kc->wire.p + KY_WIRE_WORDS * base : nullptr,
                                     (u64 *)kc->rows.tab.p + base * TAB_WORDS, (u8 *)kc->rows.status.p + base)))
                return rc;
            if ((rc = timed_launch(ctx, "keycache_insert", [&] { keycache_publish_launch(ctx, kc, base, fresh, d_unpub); })))
                return rc;
            if ((rc = keycache_placed(kc, pl))) return rc;
        }
        if (fresh || pl.republished) *d_unpublished = d_unpub;
        rc = timed_launch(ctx, "keycache_map", [&] {
            hipLaunchKernelGGL(kc_k_map, dim3((unsigned)nb), dim3(DD_BLOCK), 0, ctx->stream, (const u32 *)ctx->dd_idx.p,
                               (const u32 *)found, (u32)cnt, (u32)base, pl.all_new ? 1u : 0u, (u32 *)ctx->kc_lane_row.p);
        });
        if (rc) return rc;
        *kv = {(const uint32_t *)ctx->kc_lane_row.p, (const uint64_t *)kc->rows.tab.p, (const uint8_t *)kc->rows.status.p,
               (uint32_t)kc->capacity};
    }
    if (rows) *rows = {row_pks, row_inf};
    if (!records) return 0;
    rc = timed_launch(ctx, "keyed_expand", [&] {
        hipLaunchKernelGGL(ky_k_expand, dim3(grid_for(cnt * 12, 256)), dim3(256), 0, ctx->stream, kv->lane_key, row_pks,
                           row_inf, kv->n_keys, (u32)cnt, (u64 *)ctx->ky_pks.p, (u8 *)ctx->ky_inf.p);
    });
    if (rc) return rc;
    b->sigs = (const u8 *)ctx->ky_sigs.p;
    b->pks = (const u8 *)ctx->ky_pks.p;
    b->pk_inf = (const u8 *)ctx->ky_inf.p;
    return 0;
}

int ssa_internal_keycache_slice(ssa_ctx *ctx, ssa_keycache *kc, const uint8_t *d_pks, const uint8_t *d_pk_inf, size_t cnt,
                                KeyView *kv, uint64_t *u_out, uint64_t *bound_hits_out, uint64_t ks[4],
                                const unsigned long long **d_unpublished) {
    return keycache_slice(ctx, kc, {d_pks, d_pk_inf, nullptr}, cnt, nullptr, kv, u_out, bound_hits_out, ks, d_unpublished);
}

// ------------------------------------------------------------------ wire records through a wire cache
int ssa_internal_keyed_cache_slice(ssa_ctx *ctx, ssa_keycache *kc, const uint8_t *d_keyed, size_t cnt, DevBatch *b,
                                   KeyView *kv, uint64_t *u_out, uint64_t *bound_hits_out, uint64_t ks[4],
                                   const unsigned long long **d_unpublished) {
    if (!d_keyed || !b) return SSA_ERR_ARG;
    return keycache_slice(ctx, kc, {nullptr, nullptr, d_keyed}, cnt, b, kv, u_out, bound_hits_out, ks, d_unpublished);
}

int ssa_internal_unpack_keyed(ssa_ctx *ctx, const uint8_t *d_keyed, size_t n, DevBatch *b) {
    if (ctx->ky_sigs.reserve(n * 81 + 16) || ctx->ky_pks.reserve(n * 96) || ctx->ky_inf.reserve(n + 16)) return SSA_ERR_HIP;
    b->sigs = (const u8 *)ctx->ky_sigs.p;
    b->pks = (const u8 *)ctx->ky_pks.p;
    b->pk_inf = (const u8 *)ctx->ky_inf.p;
    return timed_launch(ctx, "ssa_k_unpack_keyed", [&] {
        hipLaunchKernelGGL(ssa_k_unpack_keyed, dim3(grid_for(n, 256)), dim3(256), 0, ctx->stream, d_keyed, n,
                           (u8 *)ctx->ky_pks.p, (u8 *)ctx->ky_inf.p, (u8 *)ctx->ky_sigs.p);
    });
}

// ------------------------------------------------------------------ several GPUs from one process
// The path shards by signature with no data-path exchange (each verification reads only its own
// record), so a host caller that owns the whole batch needs no collective at all: contiguous shards,
// one context and one host thread per device, rejection counts summed on the host.
struct ssa_multi {
    std::vector<ssa_ctx *> ctxs;
};

extern "C" int ssa_multi_create(ssa_multi **out, const int *devices, int n_devices, const void *params,
                                size_t params_len) {
    if (!out || !devices || n_devices <= 0) return SSA_ERR_ARG;
    *out = nullptr;
    ssa_multi *m = new ssa_multi();
    for (int i = 0; i < n_devices; i++) {
        ssa_ctx *c = nullptr;
        int rc = ssa_ctx_create(&c, devices[i], params, params_len);
        if (rc != 0) {
            for (ssa_ctx *x : m->ctxs) ssa_ctx_destroy(x);
            delete m;
            return rc;
        }
        m->ctxs.push_back(c);
    }
    *out = m;
    return 0;
}

extern "C" void ssa_multi_destroy(ssa_multi *m) {
    if (!m) return;
    for (ssa_ctx *c : m->ctxs) ssa_ctx_destroy(c);
    delete m;
}

extern "C" int ssa_multi_verify_many(ssa_multi *m, const uint8_t *sigs, const uint8_t *pks, const uint8_t *pk_inf,
                                     const uint8_t *msgs, const uint64_t *msg_off, size_t msg_stride,
                                     size_t msg_len, size_t n, uint32_t flags, uint8_t *status_out,
                                     uint64_t *n_fail_out) {
    if (!m || m->ctxs.empty() || (n && (!sigs || !pks || !status_out))) return SSA_ERR_ARG;
    if (n_fail_out) *n_fail_out = 0;
    if (n == 0) return 0;
    const size_t world = m->ctxs.size();
    const HostBatch b{sigs, pks, pk_inf, msgs, msg_off, msg_stride, msg_len};
    std::vector<int> rcs(world, 0);
    std::vector<uint64_t> fails(world, 0);
    std::vector<std::thread> threads;
    const size_t base = n / world, rem = n % world;
    for (size_t r = 0; r < world; r++) {
        const size_t lo = r * base + (r < rem ? r : rem), cnt = base + (r < rem ? 1 : 0);
        threads.emplace_back([&, r, lo, cnt] {
            if (cnt == 0) return;
            std::vector<uint64_t> off;
            const HostBatch s = b.slice(lo, cnt, off);
            rcs[r] = ssa_verify_many(m->ctxs[r], s.sigs, s.pks, s.pk_inf, s.msgs, s.msg_off, msg_stride, msg_len, cnt, flags,
                                     status_out + lo, &fails[r]);
        });
    }
    for (auto &t : threads) t.join();
    uint64_t total = 0;
    for (size_t r = 0; r < world; r++) {
        if (rcs[r] != 0) return rcs[r];
        total += fails[r];
    }
    if (n_fail_out) *n_fail_out = total;
    return 0;
}

// verify_batch in its MSM form over several devices: every device runs the bucket MSM on its
// contiguous shard and returns ONE point and ONE scalar; device 0 adds them up -- one Jacobian addition per shard --
// computes [sum s_i e_i]G and compares x coordinates (src/batch.rs:98-100,123-129).  The only cross-device traffic
// is 24 words per shard.
extern "C" int ssa_multi_verify_batch_msm(ssa_multi *m, const uint8_t *sigs, const uint8_t *pks, const uint8_t *pk_inf,
                                          const uint8_t *msgs, const uint64_t *msg_off, size_t msg_stride,
                                          size_t msg_len, size_t n, const uint8_t *coeffs) {
    if (!m || m->ctxs.empty() || (n && (!sigs || !pks))) return SSA_ERR_ARG;
    if (int rc = check_msgs({msgs, msg_off, msg_stride, msg_len}, n)) return rc;
    if (n == 0) return SSA_OK;
    const size_t world = m->ctxs.size();
    const HostBatch b{sigs, pks, pk_inf, msgs, msg_off, msg_stride, msg_len};
    std::vector<int> rcs(world, 0);
    std::vector<uint64_t> parts(24 * world, 0);
    std::vector<std::thread> threads;
    const size_t base = n / world, rem = n % world;
    for (size_t r = 0; r < world; r++) {
        const size_t lo = r * base + (r < rem ? r : rem), cnt = base + (r < rem ? 1 : 0);
        threads.emplace_back([&, r, lo, cnt] {
            // (an empty shard still produces its record -- the identity, 0 and the magic word: an unwritten slot is not one)
            std::vector<uint64_t> off;
            const HostBatch s = b.slice(lo, cnt, off);
            rcs[r] = ssa_verify_batch_msm_partial(m->ctxs[r], s.sigs, s.pks, s.pk_inf, s.msgs, s.msg_off, msg_stride, msg_len,
                                                  cnt, coeffs ? coeffs + 32 * lo : nullptr, &parts[24 * r]);
        });
    }
    for (auto &t : threads) t.join();
    for (size_t r = 0; r < world; r++)
        if (rcs[r] != 0) return rcs[r];
    return ssa_msm_combine(m->ctxs[0], parts.data(), world);
}

// ------------------------------------------------------------------ half-aggregation (ssa_aggregate.hpp)
// ctx->ag_misc: the MSM's record and e_agg of the single-aggregate calls
constexpr size_t AG_REC = 0, AG_E = 256, AG_MISC_BYTES = 512;
static inline u8 *ag_misc(ssa_ctx *ctx, size_t off) { return (u8 *)ctx->ag_misc.p + off; }

// One pass of the tree as ag_transcript launches it: `count` workgroups that follow the plan's descriptors at byte desc_off
// of ctx->agm_plan; or, desc_off == AG_UNIFORM, the uniform cut of the count nodes of ONE aggregate, top_n its n on the
// pass of one workgroup and 0 before.
constexpr size_t AG_UNIFORM = ~(size_t)0;
struct AgPass {
    size_t desc_off;
    u32 count, top_n;
    unsigned groups() const { return desc_off == AG_UNIFORM ? (count + AG_TREE_SPAN - 1) / AG_TREE_SPAN : count; }
};
// the passes over `nodes` (>= 1) nodes of one aggregate of n lanes: nothing to upload.  The nodes are the n leaves, or
// the ceil(n / B) tops of its blocks of B lanes: the root hashes n either way.
static std::vector<AgPass> ag_uniform_passes(size_t nodes, size_t n) {
    std::vector<AgPass> passes;
    for (size_t count = nodes;; count = passes.back().groups()) {
        const bool top = count <= AG_TREE_SPAN;
        passes.push_back({AG_UNIFORM, (u32)count, top ? (u32)n : 0u});
        if (top) return passes;
    }
}
static std::vector<AgPass> ag_uniform_passes(size_t n) { return ag_uniform_passes(n, n); }

// The transcript over the n (>= 1) lanes of a call, on ctx->stream, in two halves.  d_first: the k + 1 prefix sums of an
// uploaded plan (agm_upload_plan), and ctx->agm_map receives the lane map; nullptr: one aggregate, no plan, no lane map.
// The front: the R's and the challenge hashes.  d_wire != nullptr: the R's come out of the wire form and are laid out at
// stride 81 in ctx->ag_sigs first, and *d_sigs then points there; else they stand so in *d_sigs.  ONE launch of ssa_k_hash
// leaves the raw digests in ctx->ag_dig and, with_h, the challenge scalars mod q in ctx->ws_h (d_h_out: there instead --
// a slice of a larger call's scalars).
static int ag_transcript_front(ssa_ctx *ctx, const u8 *d_wire, const u8 **d_sigs, const u8 *d_pks, const MsgView &mv,
                               size_t n, bool with_h, const u32 *d_first, size_t k, u64 *d_h_out = nullptr) {
    if ((d_wire && ctx->ag_sigs.reserve(n * 81 + 16)) || (d_first && ctx->agm_map.reserve(n * 4)) ||
        ctx->ag_dig.reserve(n * 32) || (with_h && ctx->ws_h.reserve(n * 32)))
        return SSA_ERR_HIP;
    if (with_h) d_h_out = (u64 *)ctx->ws_h.p;
    if (d_wire) {
        const int rc = timed_launch(ctx, d_first ? "ag_k_expand_many" : "ag_k_expand", [&] {
            if (d_first)
                hipLaunchKernelGGL(ag_k_lane_map, dim3(grid_for(n, 256)), dim3(256), 0, ctx->stream, d_first, (u32)k, n,
                                   (u32 *)ctx->agm_map.p);
            hipLaunchKernelGGL(ag_k_expand, dim3(grid_for((n * 81 + 3) / 4, 256)), dim3(256), 0, ctx->stream, d_wire,
                               d_first ? (const u32 *)ctx->agm_map.p : (const u32 *)nullptr, n, (u8 *)ctx->ag_sigs.p);
        });
        if (rc) return rc;
        *d_sigs = (const u8 *)ctx->ag_sigs.p;
    } else if (d_first) {       // a plan over signatures (ssa_aggregates_many): the lane map alone
        const int rc = timed_launch(ctx, "ag_k_lane_map", [&] {
            hipLaunchKernelGGL(ag_k_lane_map, dim3(grid_for(n, 256)), dim3(256), 0, ctx->stream, d_first, (u32)k, n,
                               (u32 *)ctx->agm_map.p);
        });
        if (rc) return rc;
    }
    return timed_launch(ctx, "ssa_k_hash", [&] {
        hipLaunchKernelGGL(ssa_k_hash, dim3(grid_for(n, 256)), dim3(256), 0, ctx->stream, ctx->d_params, *d_sigs, d_pks, mv, n,
                           d_h_out, (u8 *)ctx->ag_dig.p, (const u32 *)nullptr, 0u);
    });
}

// From digests on: d_dig holds the raw digest of every lane (four words), d_sigs the lanes at stride 81 (only the flag
// byte of R is read); the coefficients a_i go into ctx->ag_coeffs (n x 16 bytes).  `passes` from the uploaded plan, or
// ag_uniform_passes.  One launch per stage and tree pass.  Nothing here reads keys, messages or the lanes' positions in
// the caller's batch: lanes gathered out of a larger one take the same route.
static int ag_transcript_from_digests(ssa_ctx *ctx, const u64 *d_dig, const u8 *d_sigs, size_t n, const u32 *d_first,
                                      size_t k, const std::vector<AgPass> &passes) {
    size_t widest = 1;                  // nodes a pass writes (a top workgroup writes a root instead)
    for (const AgPass &p : passes) widest = std::max(widest, (size_t)p.groups());
    if (ctx->agm_roots.reserve(k * 32) || ctx->ag_nodes.reserve(std::max(n, widest) * 32) ||
        ctx->ag_nodes2.reserve(widest * 32) || ctx->ag_coeffs.reserve(n * 16))
        return SSA_ERR_HIP;
    const u32 *d_map = d_first ? (const u32 *)ctx->agm_map.p : nullptr;
    int rc = timed_launch(ctx, "ag_k_leaf", [&] {
        hipLaunchKernelGGL(ag_k_leaf, dim3(grid_for(n, 256)), dim3(256), 0, ctx->stream, ctx->d_params, d_dig, d_sigs, n,
                           (u64 *)ctx->ag_nodes.p);
    });
    if (rc) return rc;
    // passes of AG_TREE_LEVELS levels between the two node buffers; a top workgroup writes its aggregate's root instead
    rc = timed_launch(ctx, "ag_k_tree", [&] {
        const u64 *in = (const u64 *)ctx->ag_nodes.p;
        u64 *ping = (u64 *)ctx->ag_nodes2.p, *pong = (u64 *)ctx->ag_nodes.p;
        for (const AgPass &p : passes) {
            const AgTreeDesc *desc =
                p.desc_off == AG_UNIFORM ? nullptr : (const AgTreeDesc *)((const u8 *)ctx->agm_plan.p + p.desc_off);
            hipLaunchKernelGGL(ag_k_tree, dim3(p.groups()), dim3(256), 0, ctx->stream, ctx->d_params, in, desc, p.count,
                               p.top_n, ping, (u64 *)ctx->agm_roots.p);
            in = ping;
            std::swap(ping, pong);
        }
    });
    if (rc) return rc;
    return timed_launch(ctx, "ag_k_coeff", [&] {
        hipLaunchKernelGGL(ag_k_coeff, dim3(grid_for(n, 256)), dim3(256), 0, ctx->stream, ctx->d_params,
                           (const u64 *)ctx->agm_roots.p, d_map, d_first, n, (u64 *)ctx->ag_coeffs.p, (u64)0);
    });
}

// Both halves: what every call that starts from signatures or a wire form runs.
static int ag_transcript(ssa_ctx *ctx, const u8 *d_wire, const u8 *d_sigs, const u8 *d_pks, const MsgView &mv, size_t n,
                         bool with_h, const u32 *d_first, size_t k, const std::vector<AgPass> &passes) {
    if (int rc = ag_transcript_front(ctx, d_wire, &d_sigs, d_pks, mv, n, with_h, d_first, k)) return rc;
    return ag_transcript_from_digests(ctx, (const u64 *)ctx->ag_dig.p, d_sigs, n, d_first, k, passes);
}

// sum a_i e_i mod q over n lanes at stride 81 with the coefficients of ctx->ag_coeffs, into ag_misc(ctx, AG_E).
// d_status != nullptr: the checks of msm_k_prepare too (ag_k_fold), *d_fail counts the lanes that fail one.
static int ag_fold(ssa_ctx *ctx, const u8 *d_sigs, const u8 *d_pks, const u8 *d_pk_inf, size_t n, u8 *d_status,
                   unsigned long long *d_fail) {
    const unsigned n_blocks = grid_for(n, 256);
    if (ctx->ag_partials.reserve((size_t)n_blocks * 32) || ctx->ag_misc.reserve(AG_MISC_BYTES)) return SSA_ERR_HIP;
    return timed_launch(ctx, "ag_k_fold", [&] {
        hipLaunchKernelGGL(ag_k_fold, dim3(n_blocks), dim3(256), 0, ctx->stream, d_sigs, d_pks, d_pk_inf,
                           (const u64 *)ctx->ag_coeffs.p, n, (u64 *)ctx->ag_partials.p, d_status, d_fail);
        hipLaunchKernelGGL(ag_k_fold_finish, dim3(1), dim3(256), 0, ctx->stream, (const u64 *)ctx->ag_partials.p, n_blocks,
                           ag_misc(ctx, AG_E));
    });
}

// sliced: the forms of DESIGN.md section 25, any n <= SSA_MAX_BATCH; every other call takes one MSM slice at most
static int agg_check_args(const ssa_ctx *ctx, const MsgView &mv, size_t n, bool sliced = false) {
    if (int rc = check_msgs(mv, n)) return rc;
    return !sliced && n > ctx->knobs.msm_slice ? SSA_ERR_ARG : 0;
}

// What a producer call returns once the fold has counted: the stream is synchronised and *d_fail read.  Refused
// (*st_out != 0): d_agg_out is zeroed and *st_out is SSA_MALFORMED or, screened, the smallest nonzero status.
static int ag_refusal(ssa_ctx *ctx, size_t n, bool screened, const u8 *d_status, const unsigned long long *d_fail,
                      u8 *d_agg_out, int *st_out) {
    *st_out = SSA_OK;
    unsigned long long nf = 0;
    HIP_TRY(hipMemcpyAsync(&nf, d_fail, sizeof nf, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (!nf) return 0;
    HIP_TRY(hipMemsetAsync(d_agg_out, 0, SSA_AGGREGATE_LENGTH(n), ctx->stream));
    int st = SSA_MALFORMED;
    if (screened) {
        std::vector<uint8_t> h(n);
        HIP_TRY(hipMemcpyAsync(h.data(), d_status, n, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        for (uint8_t v : h)
            if (v && (int)v < st) st = v;
    }
    *st_out = st;
    return 0;
}

// the caller's status buffer, or ctx->ag_status reserved for n lanes (nullptr: the reserve failed)
static u8 *ag_status_buf(ssa_ctx *ctx, u8 *d_status_out, size_t n) {
    if (d_status_out) return d_status_out;
    return ctx->ag_status.reserve(n + 16) ? nullptr : (u8 *)ctx->ag_status.p;
}

// the host form of ssa_aggregate_many and of its sliced twin: staging and copies back are the same
static int aggregate_many_host(ssa_ctx *ctx, const uint8_t *sigs, const uint8_t *pks, const uint8_t *pk_inf,
                               const uint8_t *msgs, const uint64_t *msg_off, size_t msg_stride, size_t msg_len, size_t n,
                               uint32_t flags, uint8_t *agg_out, uint8_t *status_out, uint64_t *n_fail_out, bool sliced) {
    if (!ctx || !agg_out || (flags & ~SSA_AGG_CHECK) || (n && (!sigs || !pks))) return SSA_ERR_ARG;
    if (int rc = agg_check_args(ctx, {msgs, msg_off, msg_stride, msg_len}, n, sliced)) return rc;
    if (int rc = check_host_offsets(msg_off, n)) return rc;
    if (n_fail_out) *n_fail_out = 0;
    if (n == 0) {
        std::memset(agg_out, 0, 32);
        return SSA_OK;
    }
    HostCall hc(ctx);
    const DevBatch b = hc.lanes({sigs, pks, pk_inf, msgs, msg_off, msg_stride, msg_len}, n * 81, n);
    u8 *d_agg = hc.out(ctx->st_aux, agg_out, SSA_AGGREGATE_LENGTH(n), 16);
    u8 *d_status = hc.out(ctx->st_status, status_out, n, 16);
    unsigned long long nf = 0;
    hc.copy_back(&nf, ctx->ws_fail.p, sizeof nf);
    int st = SSA_OK;       // a refusal is a result, not an error: the zeroed aggregate and the statuses still come back
    const int rc = hc.finish([&] {
        const int r = (sliced ? ssa_aggregate_many_sliced_device : ssa_aggregate_many_device)(
            ctx, b.sigs, b.pks, b.pk_inf, b.msgs.msgs, b.msgs.off, msg_stride, msg_len, n, flags, d_agg, d_status, nullptr);
        if (r > 0) st = r;
        return r > 0 ? 0 : r;
    });
    if (rc) return rc;
    if (n_fail_out) *n_fail_out = nf;
    return st;
}

extern "C" int ssa_aggregate_many(ssa_ctx *ctx, const uint8_t *sigs, const uint8_t *pks, const uint8_t *pk_inf,
                                  const uint8_t *msgs, const uint64_t *msg_off, size_t msg_stride, size_t msg_len, size_t n,
                                  uint32_t flags, uint8_t *agg_out, uint8_t *status_out, uint64_t *n_fail_out) {
    return aggregate_many_host(ctx, sigs, pks, pk_inf, msgs, msg_off, msg_stride, msg_len, n, flags, agg_out, status_out,
                               n_fail_out, false);
}

// ------------------------------------------------------------------ filtering half-aggregation
// d_kept[0, *m_out) = the lanes of d_status[0, n) whose byte is zero, ascending, and zeros up to n; *m_out their number.
// av_keep_enqueue only enqueues the three launches and says where on the device the number will stand; av_keep then
// synchronises the stream: the number is read from the device.
static int av_keep_enqueue(ssa_ctx *ctx, const u8 *d_status, size_t n, u32 *d_kept, const u32 **d_m_out) {
    const unsigned nb = grid_for(n, AV_BLOCK);
    if (ctx->av_blk.reserve((2 * (size_t)nb + 1) * sizeof(u32))) return SSA_ERR_HIP;
    u32 *blk_cnt = (u32 *)ctx->av_blk.p, *blk_off = blk_cnt + nb;
    *d_m_out = blk_off + nb;
    return timed_launch(ctx, "av_k_keep", [&] {
        hipLaunchKernelGGL(av_k_keep_count, dim3(nb), dim3(AV_BLOCK), 0, ctx->stream, d_status, (u32)n, blk_cnt);
        hipLaunchKernelGGL(av_k_keep_scan, dim3(1), dim3(AV_BLOCK), 0, ctx->stream, (const u32 *)blk_cnt, nb, blk_off);
        hipLaunchKernelGGL(av_k_keep_list, dim3(nb), dim3(AV_BLOCK), 0, ctx->stream, d_status, (u32)n, (const u32 *)blk_off,
                           nb, d_kept);
    });
}
static int av_keep(ssa_ctx *ctx, const u8 *d_status, size_t n, u32 *d_kept, uint64_t *m_out) {
    const u32 *d_m = nullptr;
    if (int rc = av_keep_enqueue(ctx, d_status, n, d_kept, &d_m)) return rc;
    u32 m = 0;
    HIP_TRY(hipMemcpyAsync(&m, d_m, sizeof m, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    *m_out = m;
    return 0;
}

// The aggregate of the m (>= 1) listed lanes into d_agg_out, from the raw digests of all lanes in ctx->ag_dig and the
// signatures at d_sigs + stride * lane + off.  A lane's digest does not depend on its place, so the kept lanes'
// signatures and digests side by side are what the transcript of those lanes handed in alone starts from; keys and
// messages are not needed again.
static int av_aggregate_kept(ssa_ctx *ctx, const u8 *d_sigs, u32 stride, u32 off, const u32 *d_kept, size_t m, u8 *d_agg_out) {
    if (ctx->av_sigs.reserve(m * 81 + 16) || ctx->av_dig.reserve(m * 32)) return SSA_ERR_HIP;
    const u8 *k_sigs = (const u8 *)ctx->av_sigs.p;
    int rc = timed_launch(ctx, "av_k_gather", [&] {
        hipLaunchKernelGGL(av_k_gather_sigs, dim3(grid_for((m * 81 + 3) / 4, 256)), dim3(256), 0, ctx->stream, d_sigs, stride,
                           off, d_kept, m, (u8 *)ctx->av_sigs.p);
        hipLaunchKernelGGL(av_k_gather_dig, dim3(grid_for(2 * m, 256)), dim3(256), 0, ctx->stream,
                           (const u64 *)ctx->ag_dig.p, d_kept, m, (u64 *)ctx->av_dig.p);
    });
    if (rc) return rc;
    if ((rc = ag_transcript_from_digests(ctx, (const u64 *)ctx->av_dig.p, k_sigs, m, nullptr, 1, ag_uniform_passes(m))))
        return rc;
    // (every kept lane passed the screen: e_i < q, and the fold has nothing left to check)
    if ((rc = ag_fold(ctx, k_sigs, nullptr, nullptr, m, nullptr, nullptr))) return rc;
    return timed_launch(ctx, "ag_k_pack", [&] {
        hipLaunchKernelGGL(ag_k_pack, dim3(grid_for((m * 49 + 3) / 4, 256)), dim3(256), 0, ctx->stream, k_sigs, m, d_agg_out);
        (void)hipMemcpyAsync(d_agg_out + 49 * m, ag_misc(ctx, AG_E), 32, hipMemcpyDeviceToDevice, ctx->stream);
    });
}

// The tail of every filtering aggregate, behind the n statuses: the kept lanes are listed (av_keep, one synchronisation
// for |K|), *n_kept_out says how many, the caller's aggregate is zeroed behind what they will take, `between` (if any)
// runs with |K|, and the kept lanes -- signatures at d_sigs + stride * lane + off -- are aggregated.
static int av_finish_kept(ssa_ctx *ctx, const u8 *d_status, size_t n, const u8 *d_sigs, u32 stride, u32 off, u8 *d_agg_out,
                          u32 *d_kept_out, uint64_t *n_kept_out, const std::function<int(size_t)> &between = nullptr) {
    uint64_t m = 0;
    if (int rc = av_keep(ctx, d_status, n, d_kept_out, &m)) return rc;
    *n_kept_out = m;
    // everything behind the aggregate of the kept lanes is zero; with none kept, that is the empty aggregate
    const size_t used = m ? SSA_AGGREGATE_LENGTH(m) : 0;
    if (used < SSA_AGGREGATE_LENGTH(n))
        HIP_TRY(hipMemsetAsync(d_agg_out + used, 0, SSA_AGGREGATE_LENGTH(n) - used, ctx->stream));
    if (between)
        if (int rc = between(m)) return rc;
    if (m == 0) return SSA_OK;
    return av_aggregate_kept(ctx, d_sigs, stride, off, d_kept_out, m, d_agg_out);
}

// Two synchronisations: the screen's (for its segment verdicts; none at n <= msm_small_max) and one for |K|.
extern "C" int ssa_aggregate_valid_many_device(ssa_ctx *ctx, const uint8_t *d_sigs, const uint8_t *d_pks,
                                               const uint8_t *d_pk_inf, const uint8_t *d_msgs, const uint64_t *d_msg_off,
                                               size_t msg_stride, size_t msg_len, size_t n, uint8_t *d_agg_out,
                                               uint32_t *d_kept_out, uint64_t *n_kept_out, uint8_t *d_status_out) {
    const DevBatch b{d_sigs, d_pks, d_pk_inf, {d_msgs, d_msg_off, msg_stride, msg_len}};
    if (!ctx || !d_agg_out || !d_kept_out || !n_kept_out || (n && (!d_sigs || !d_pks))) return SSA_ERR_ARG;
    if (int rc = agg_check_args(ctx, b.msgs, n)) return rc;
    *n_kept_out = 0;
    HIP_TRY(hipSetDevice(ctx->device));
    if (n == 0) {
        HIP_TRY(hipMemsetAsync(d_agg_out, 0, 32, ctx->stream));
        return SSA_OK;
    }
    u8 *d_status = ag_status_buf(ctx, d_status_out, n);
    if (!d_status) return SSA_ERR_HIP;
    // ONE challenge hash over all n lanes: the scalars mod q for the screen, the raw digests for the transcript
    if (int rc = ag_transcript_front(ctx, nullptr, &d_sigs, d_pks, b.msgs, n, true, nullptr, 1)) return rc;
    // The screen reads ws_h and writes neither it nor ag_dig: with ready hashes msm_run_one and
    // ssa_internal_verify_hashed launch no ssa_k_hash, the gather of failing segments copies the scalars into scr_in, and
    // no ag_* buffer belongs to it.
    if (int rc = ssa_internal_screen_hashed(ctx, b, n, (const uint64_t *)ctx->ws_h.p, d_status, nullptr)) return rc;
    return av_finish_kept(ctx, d_status, n, d_sigs, 81, 0, d_agg_out, d_kept_out, n_kept_out);
}

extern "C" int ssa_aggregate_valid_many(ssa_ctx *ctx, const uint8_t *sigs, const uint8_t *pks, const uint8_t *pk_inf,
                                        const uint8_t *msgs, const uint64_t *msg_off, size_t msg_stride, size_t msg_len,
                                        size_t n, uint8_t *agg_out, uint32_t *kept_out, uint64_t *n_kept_out,
                                        uint8_t *status_out) {
    if (!ctx || !agg_out || !kept_out || !n_kept_out || (n && (!sigs || !pks))) return SSA_ERR_ARG;
    if (int rc = agg_check_args(ctx, {msgs, msg_off, msg_stride, msg_len}, n)) return rc;
    if (int rc = check_host_offsets(msg_off, n)) return rc;
    *n_kept_out = 0;
    if (n == 0) {
        std::memset(agg_out, 0, 32);
        return SSA_OK;
    }
    HostCall hc(ctx);
    const DevBatch b = hc.lanes({sigs, pks, pk_inf, msgs, msg_off, msg_stride, msg_len}, n * 81, n);
    u8 *d_agg = hc.out(ctx->st_aux, agg_out, SSA_AGGREGATE_LENGTH(n), 16);
    u32 *d_kept = (u32 *)hc.out(ctx->st_aux2, kept_out, n * sizeof(u32));
    u8 *d_status = hc.out(ctx->st_status, status_out, n, 16);
    return hc.finish([&] {
        return ssa_aggregate_valid_many_device(ctx, b.sigs, b.pks, b.pk_inf, b.msgs.msgs, b.msgs.off, msg_stride, msg_len, n,
                                               d_agg, d_kept, n_kept_out, d_status);
    });
}

// tests: the compaction alone, from a host status vector
extern "C" int ssa_debug_aggregate_keep(ssa_ctx *ctx, const uint8_t *status, size_t n, uint32_t *kept_out,
                                        uint64_t *n_kept_out) {
    if (!ctx || !n_kept_out || (n && (!status || !kept_out)) || n > SSA_MAX_BATCH) return SSA_ERR_ARG;
    *n_kept_out = 0;
    if (n == 0) return SSA_OK;
    HostCall hc(ctx);
    const u8 *d_status = hc.in(ctx->st_status, status, n);
    u32 *d_kept = (u32 *)hc.out(ctx->st_aux2, kept_out, n * sizeof(u32));
    return hc.finish([&] { return av_keep(ctx, d_status, n, d_kept, n_kept_out); });
}

extern "C" int ssa_verify_aggregate_device(ssa_ctx *ctx, const uint8_t *d_agg, const uint8_t *d_pks, const uint8_t *d_pk_inf,
                                           const uint8_t *d_msgs, const uint64_t *d_msg_off, size_t msg_stride,
                                           size_t msg_len, size_t n, uint32_t *d_verdict_out) {
    const MsgView mv{d_msgs, d_msg_off, msg_stride, msg_len};
    if (!ctx || !d_agg || !d_verdict_out || (n && !d_pks)) return SSA_ERR_ARG;
    if (int rc = agg_check_args(ctx, mv, n)) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    if (n) {
        if (ctx->ag_misc.reserve(AG_MISC_BYTES)) return SSA_ERR_HIP;
        if (int rc = ag_transcript(ctx, d_agg, nullptr, d_pks, mv, n, true, nullptr, 1, ag_uniform_passes(n))) return rc;
        // the MSM of ssa_verify_batch_msm over (R_i, e = 0) with the transcript's coefficients, reduced to its record
        const DevBatch b{(const u8 *)ctx->ag_sigs.p, d_pks, d_pk_inf, mv};
        if (int rc = ssa_internal_msm_record(ctx, b, n, (const u8 *)ctx->ag_coeffs.p, 16, (const uint64_t *)ctx->ws_h.p,
                                             (uint64_t *)ag_misc(ctx, AG_REC)))
            return rc;
    }
    return timed_launch(ctx, "ag_k_finish", [&] {       // (the empty aggregate has no record: the kernel reads none)
        hipLaunchKernelGGL(ag_k_finish, dim3(1), dim3(64), 0, ctx->stream, (const u64 *)ag_misc(ctx, AG_REC), d_agg,
                           (const u32 *)nullptr, n, 0u, (const u64 *)ctx->d_gtab, d_verdict_out);
    });
}

static int verify_aggregate_host(ssa_ctx *ctx, const uint8_t *agg, const uint8_t *pks, const uint8_t *pk_inf,
                                 const uint8_t *msgs, const uint64_t *msg_off, size_t msg_stride, size_t msg_len, size_t n,
                                 bool sliced) {
    if (!ctx || !agg || (n && !pks)) return SSA_ERR_ARG;
    if (int rc = agg_check_args(ctx, {msgs, msg_off, msg_stride, msg_len}, n, sliced)) return rc;
    if (int rc = check_host_offsets(msg_off, n)) return rc;
    HostCall hc(ctx);
    const DevBatch b = hc.lanes({agg, pks, pk_inf, msgs, msg_off, msg_stride, msg_len}, SSA_AGGREGATE_LENGTH(n), n);
    uint32_t v = SSA_MALFORMED, *d_verdict = (uint32_t *)((char *)ctx->ws_fail.p + 32);
    hc.copy_back(&v, d_verdict, sizeof v);
    const int rc = hc.finish([&] {
        return (sliced ? ssa_verify_aggregate_sliced_device : ssa_verify_aggregate_device)(
            ctx, b.sigs, b.pks, b.pk_inf, b.msgs.msgs, b.msgs.off, msg_stride, msg_len, n, d_verdict);
    });
    return rc ? rc : (int)v;
}

extern "C" int ssa_verify_aggregate(ssa_ctx *ctx, const uint8_t *agg, const uint8_t *pks, const uint8_t *pk_inf,
                                    const uint8_t *msgs, const uint64_t *msg_off, size_t msg_stride, size_t msg_len,
                                    size_t n) {
    return verify_aggregate_host(ctx, agg, pks, pk_inf, msgs, msg_off, msg_stride, msg_len, n, false);
}

// ------------------------------------------------------------------ sliced and sharded half-aggregation
// The transcript's tree is defined level by level, so an aligned run of B = 2^t leaves is a whole subtree: a shard (a
// slice of one context, a device, a rank) reduces ITS lanes to one 32-byte top per block of B, whoever holds all the tops
// finishes the tree and hashes the root with the total n, and every shard derives its lanes' coefficients from the root
// and the lanes' places in the aggregate.  What is left is linear: a partial sum a_i e_i mod q per shard for the producer,
// one MSM record per shard for the validator.  The four steps below take any number of lanes and walk them in pieces of
// at most one MSM slice; the primitives of the ABI, the sliced calls and the ssa_multi calls are these steps in a row.
static inline size_t pow2_floor(size_t v) {
    size_t p = 1;
    while (p <= v / 2) p *= 2;
    return p;
}
static inline bool is_pow2(size_t v) { return v && !(v & (v - 1)); }
static inline bool aligned8(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 7u) == 0; }
// lanes per block of the sliced and ssa_multi calls: the largest power of two within the MSM slice, or the tests' knob
static size_t ags_block(const ssa_ctx *ctx) {
    return pow2_floor(ctx->knobs.agg_block ? ctx->knobs.agg_block : ctx->knobs.msm_slice);
}
// lanes per piece of a walk: a power of two, so whole blocks of B -- one MSM slice, or one block where a block is larger
static size_t ags_piece(const ssa_ctx *ctx, size_t B = 1) { return std::max(B, pow2_floor(ctx->knobs.msm_slice)); }

// Step 1.  The n_s lanes at d_lanes (signatures at stride 81 or R's at stride 49; the shard's first lane stands on a
// multiple of B in its aggregate) -> ceil(n_s / B) tops at d_tops_out, and with d_h_out the n_s challenge scalars mod q.
// Per piece: ag_k_expand for R's, ONE ssa_k_hash, ONE ag_k_leaf and log2(B) launches of ag_k_level (fewer once one node
// is left), between ctx->ag_nodes and ctx->ag_nodes2; the last launch writes the tops where they go.
static int ags_tops(ssa_ctx *ctx, const u8 *d_lanes, u32 stride, const u8 *d_pks, const MsgView &mv, size_t n_s, size_t B,
                    u64 *d_tops_out, u64 *d_h_out) {
    const DevBatch b{nullptr, d_pks, nullptr, mv};
    const size_t piece = ags_piece(ctx, B);
    for (size_t lo = 0; lo < n_s; lo += piece) {
        const size_t cnt = std::min(piece, n_s - lo);
        const DevBatch s = b.slice(lo);
        const u8 *d_sigs = d_lanes + (size_t)stride * lo;
        if (int rc = ag_transcript_front(ctx, stride == 49 ? d_sigs : nullptr, &d_sigs, s.pks, s.msgs, cnt, false, nullptr, 1,
                                         d_h_out ? d_h_out + 4 * lo : nullptr))
            return rc;
        unsigned launches = 0;
        for (size_t c = cnt, l = B; l > 1 && c > 1; l /= 2, c = (c + 1) / 2) launches++;
        if (ctx->ag_nodes.reserve(cnt * 32) || ctx->ag_nodes2.reserve((cnt + 1) / 2 * 32)) return SSA_ERR_HIP;
        u64 *const dst = d_tops_out + 4 * (lo / B), *bufs[2] = {(u64 *)ctx->ag_nodes.p, (u64 *)ctx->ag_nodes2.p};
        int rc = timed_launch(ctx, "ag_k_leaf", [&] {
            hipLaunchKernelGGL(ag_k_leaf, dim3(grid_for(cnt, 256)), dim3(256), 0, ctx->stream, ctx->d_params,
                               (const u64 *)ctx->ag_dig.p, d_sigs, cnt, launches ? bufs[0] : dst);
        });
        if (rc) return rc;
        if (!launches) continue;
        rc = timed_launch(ctx, "ag_k_level", [&] {
            size_t c = cnt;
            for (unsigned l = 0; l < launches; l++, c = (c + 1) / 2)
                hipLaunchKernelGGL(ag_k_level, dim3(grid_for((c + 1) / 2, 256)), dim3(256), 0, ctx->stream, ctx->d_params,
                                   (const u64 *)bufs[l & 1u], c, l + 1 == launches ? dst : bufs[(l + 1) & 1u]);
        });
        if (rc) return rc;
    }
    return 0;
}

// Step 2.  The n_tops (>= 1) tops of an aggregate of n lanes -> its root: the passes of ag_k_tree over them, and the
// last workgroup hashes n.
static int ags_root(ssa_ctx *ctx, const u64 *d_tops, size_t n_tops, size_t n, u64 *d_root_out) {
    const std::vector<AgPass> passes = ag_uniform_passes(n_tops, n);
    const size_t widest = passes[0].groups();
    if (ctx->ag_nodes.reserve(widest * 32) || ctx->ag_nodes2.reserve(widest * 32)) return SSA_ERR_HIP;
    return timed_launch(ctx, "ag_k_tree", [&] {
        const u64 *in = d_tops;
        u64 *ping = (u64 *)ctx->ag_nodes2.p, *pong = (u64 *)ctx->ag_nodes.p;
        for (const AgPass &p : passes) {
            hipLaunchKernelGGL(ag_k_tree, dim3(p.groups()), dim3(256), 0, ctx->stream, ctx->d_params, in,
                               (const AgTreeDesc *)nullptr, p.count, p.top_n, ping, d_root_out);
            in = ping;
            std::swap(ping, pong);
        }
    });
}

// the coefficients of cnt lanes whose first stands at `lane0` of its aggregate, from the root at d_root, into ctx->ag_coeffs
static int ags_coeffs(ssa_ctx *ctx, const u64 *d_root, size_t cnt, size_t lane0) {
    if (ctx->ag_coeffs.reserve(cnt * 16)) return SSA_ERR_HIP;
    return timed_launch(ctx, "ag_k_coeff", [&] {
        hipLaunchKernelGGL(ag_k_coeff, dim3(grid_for(cnt, 256)), dim3(256), 0, ctx->stream, ctx->d_params, d_root,
                           (const u32 *)nullptr, (const u32 *)nullptr, cnt, (u64 *)ctx->ag_coeffs.p, (u64)lane0);
    });
}

// Step 3, producer.  The n_s signatures of b, the first at `lane0` of the aggregate: d_e_out (32 bytes) = sum a_i e_i mod
// q over them, d_rs_out their 49 n_s bytes of R's; d_status != nullptr: the checks of ag_k_fold, *d_fail is added to.
static int ags_fold(ssa_ctx *ctx, const DevBatch &b, size_t n_s, size_t lane0, const u64 *d_root, u8 *d_e_out, u8 *d_rs_out,
                    u8 *d_status, unsigned long long *d_fail) {
    if (n_s == 0) {
        HIP_TRY(hipMemsetAsync(d_e_out, 0, 32, ctx->stream));
        return 0;
    }
    const size_t piece = ags_piece(ctx), k = (n_s + piece - 1) / piece;
    if (ctx->ags_parts.reserve(k * 32) || ctx->ag_partials.reserve((size_t)grid_for(std::min(piece, n_s), 256) * 32))
        return SSA_ERR_HIP;
    if (int rc = for_dev_slices(b, n_s, piece, [&](size_t lo, size_t cnt, const DevBatch &s) {
            if (int rc = ags_coeffs(ctx, d_root, cnt, lane0 + lo)) return rc;
            const unsigned n_blocks = grid_for(cnt, 256);
            return timed_launch(ctx, "ag_k_fold", [&] {
                hipLaunchKernelGGL(ag_k_fold, dim3(n_blocks), dim3(256), 0, ctx->stream, s.sigs, s.pks, s.pk_inf,
                                   (const u64 *)ctx->ag_coeffs.p, cnt, (u64 *)ctx->ag_partials.p,
                                   d_status ? d_status + lo : (u8 *)nullptr, d_fail);
                hipLaunchKernelGGL(ag_k_fold_finish, dim3(1), dim3(256), 0, ctx->stream, (const u64 *)ctx->ag_partials.p,
                                   n_blocks, k == 1 ? d_e_out : (u8 *)ctx->ags_parts.p + 32 * (lo / piece));
                hipLaunchKernelGGL(ag_k_pack, dim3(grid_for((cnt * 49 + 3) / 4, 256)), dim3(256), 0, ctx->stream, s.sigs, cnt,
                                   d_rs_out + 49 * lo);
            });
        }))
        return rc;
    if (k == 1) return 0;
    return timed_launch(ctx, "ag_k_fold", [&] {
        hipLaunchKernelGGL(ag_k_fold_finish, dim3(1), dim3(256), 0, ctx->stream, (const u64 *)ctx->ags_parts.p, (u32)k, d_e_out);
    });
}

// Step 3, validator.  The n_s R's at d_rs49 with their keys and messages (b; its sigs are not read) and challenge scalars
// d_h (nullptr: hashed again), the first at `lane0` of the aggregate: d_rec_out = the record of the MSM over (R_i, e = 0)
// with the transcript's coefficients -- per piece through ssa_internal_msm_record, the pieces' records added up.  A piece
// of at most msm_small_max lanes goes through msm_k_small, which hashes for itself: that is what the messages are for.
// expanded: ctx->ag_sigs still holds the R's at stride 81 from the walk of the tops (one piece in all).
static int ags_record(ssa_ctx *ctx, const u8 *d_rs49, const DevBatch &b, const u64 *d_h, size_t n_s, size_t lane0,
                      const u64 *d_root, u64 *d_rec_out, bool expanded = false) {
    const size_t piece = ags_piece(ctx), k = n_s ? (n_s + piece - 1) / piece : 1;
    if (k > 4096) return SSA_ERR_ARG;
    if (ctx->ags_recs.reserve(k * 24 * sizeof(u64)) || ctx->ag_coeffs.reserve(16)) return SSA_ERR_HIP;
    for (size_t lo = 0, j = 0; j < k; lo += piece, j++) {
        const size_t cnt = std::min(piece, n_s - lo);
        if (cnt && !(expanded && k == 1)) {
            if (ctx->ag_sigs.reserve(cnt * 81 + 16)) return SSA_ERR_HIP;
            const int rc = timed_launch(ctx, "ag_k_expand", [&] {
                hipLaunchKernelGGL(ag_k_expand, dim3(grid_for((cnt * 81 + 3) / 4, 256)), dim3(256), 0, ctx->stream,
                                   d_rs49 + 49 * lo, (const u32 *)nullptr, cnt, (u8 *)ctx->ag_sigs.p);
            });
            if (rc) return rc;
        }
        if (cnt)
            if (int rc = ags_coeffs(ctx, d_root, cnt, lane0 + lo)) return rc;
        DevBatch s = b.slice(lo);
        s.sigs = (const u8 *)ctx->ag_sigs.p;
        if (int rc = ssa_internal_msm_record(ctx, s, cnt, (const u8 *)ctx->ag_coeffs.p, 16,
                                             d_h ? (const uint64_t *)(d_h + 4 * lo) : nullptr,
                                             k == 1 ? (uint64_t *)d_rec_out : (uint64_t *)ctx->ags_recs.p + 24 * j))
            return rc;
    }
    return k == 1 ? 0 : ssa_internal_msm_sum_records(ctx, (const uint64_t *)ctx->ags_recs.p, k, false, (uint64_t *)d_rec_out);
}

// ---- the primitives: each only enqueues on the context's stream
extern "C" int ssa_aggregate_shard_tops_device(ssa_ctx *ctx, const uint8_t *d_lanes, uint32_t lane_stride,
                                               const uint8_t *d_pks, const uint8_t *d_msgs, const uint64_t *d_msg_off,
                                               size_t msg_stride, size_t msg_len, size_t n_s, size_t block_lanes,
                                               uint8_t *d_tops_out, uint64_t *d_h_out) {
    const MsgView mv{d_msgs, d_msg_off, msg_stride, msg_len};
    if (!ctx || (lane_stride != 81 && lane_stride != 49) || !is_pow2(block_lanes) || block_lanes > SSA_MAX_BATCH ||
        (n_s && (!d_lanes || !d_pks || !d_tops_out)) || !aligned8(d_tops_out) || !aligned8(d_h_out))
        return SSA_ERR_ARG;
    if (int rc = check_msgs(mv, n_s)) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    return ags_tops(ctx, d_lanes, lane_stride, d_pks, mv, n_s, block_lanes, (u64 *)d_tops_out, (u64 *)d_h_out);
}

extern "C" int ssa_aggregate_root_device(ssa_ctx *ctx, const uint8_t *d_tops, size_t n_tops, size_t n, size_t block_lanes,
                                         uint8_t *d_root_out) {
    if (!ctx || !d_tops || !d_root_out || !aligned8(d_tops) || !aligned8(d_root_out) || n == 0 || n > SSA_MAX_BATCH ||
        n_tops == 0 || n_tops > n)
        return SSA_ERR_ARG;
    if (block_lanes && (!is_pow2(block_lanes) || n_tops != (n + block_lanes - 1) / block_lanes)) return SSA_ERR_ARG;
    HIP_TRY(hipSetDevice(ctx->device));
    return ags_root(ctx, (const u64 *)d_tops, n_tops, n, (u64 *)d_root_out);
}

extern "C" int ssa_aggregate_shard_fold_device(ssa_ctx *ctx, const uint8_t *d_sigs, const uint8_t *d_pks,
                                               const uint8_t *d_pk_inf, size_t n_s, size_t lane0, const uint8_t *d_root,
                                               uint8_t *d_e_out, uint8_t *d_rs_out, uint8_t *d_status_out,
                                               uint64_t *d_n_fail_out) {
    if (!ctx || !d_root || !aligned8(d_root) || !d_e_out || n_s > SSA_MAX_BATCH || lane0 > SSA_MAX_BATCH - n_s ||
        (n_s && (!d_sigs || !d_rs_out || (d_status_out && !d_pks))))
        return SSA_ERR_ARG;
    unsigned long long *d_fail;
    if (int rc = reset_fail_counter(ctx, d_n_fail_out, &d_fail)) return rc;
    return ags_fold(ctx, {d_sigs, d_pks, d_pk_inf, {}}, n_s, lane0, (const u64 *)d_root, d_e_out, d_rs_out, d_status_out,
                    d_fail);
}

extern "C" int ssa_verify_aggregate_shard_device(ssa_ctx *ctx, const uint8_t *d_rs49, const uint8_t *d_pks,
                                                 const uint8_t *d_pk_inf, const uint8_t *d_msgs, const uint64_t *d_msg_off,
                                                 size_t msg_stride, size_t msg_len, const uint64_t *d_h, size_t n_s,
                                                 size_t lane0, const uint8_t *d_root, uint64_t *d_record_out) {
    const MsgView mv{d_msgs, d_msg_off, msg_stride, msg_len};
    if (!ctx || !d_root || !aligned8(d_root) || !d_record_out || n_s > SSA_MAX_BATCH || lane0 > SSA_MAX_BATCH - n_s ||
        (n_s && (!d_rs49 || !d_pks)))
        return SSA_ERR_ARG;
    if (int rc = check_msgs(mv, n_s)) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    return ags_record(ctx, d_rs49, {nullptr, d_pks, d_pk_inf, mv}, (const u64 *)d_h, n_s, lane0, (const u64 *)d_root,
                      (u64 *)d_record_out);
}

extern "C" int ssa_aggregate_combine_device(ssa_ctx *ctx, const uint8_t *d_partials32, size_t k, uint8_t *d_e_agg_out) {
    if (!ctx || !d_partials32 || !aligned8(d_partials32) || !d_e_agg_out || k == 0 || k > 4096) return SSA_ERR_ARG;
    HIP_TRY(hipSetDevice(ctx->device));
    return timed_launch(ctx, "ag_k_fold", [&] {
        hipLaunchKernelGGL(ag_k_fold_finish, dim3(1), dim3(256), 0, ctx->stream, (const u64 *)d_partials32, (u32)k, d_e_agg_out);
    });
}

extern "C" int ssa_verify_aggregate_combine_device(ssa_ctx *ctx, const uint64_t *d_records24, size_t k,
                                                   const uint8_t *d_e_agg, size_t n, uint32_t *d_verdict_out) {
    if (!ctx || !d_e_agg || !d_verdict_out || n > SSA_MAX_BATCH || (n && (!d_records24 || k == 0 || k > 4096)))
        return SSA_ERR_ARG;
    HIP_TRY(hipSetDevice(ctx->device));
    if (ctx->ag_misc.reserve(AG_MISC_BYTES)) return SSA_ERR_HIP;
    if (n)
        if (int rc = ssa_internal_msm_sum_records(ctx, d_records24, k, true, (uint64_t *)ag_misc(ctx, AG_REC))) return rc;
    return timed_launch(ctx, "ag_k_finish", [&] {
        hipLaunchKernelGGL(ag_k_finish_scalar, dim3(1), dim3(64), 0, ctx->stream, (const u64 *)ag_misc(ctx, AG_REC), d_e_agg,
                           n == 0 ? 1u : 0u, (const u64 *)ctx->d_gtab, d_verdict_out);
    });
}

// ---- one context, any n <= SSA_MAX_BATCH: the slices are the shards
// tops of all n lanes into ctx->ags_tops and the root into ctx->agm_roots; d_h_out as ags_tops
static int ags_root_of(ssa_ctx *ctx, const u8 *d_lanes, u32 stride, const u8 *d_pks, const MsgView &mv, size_t n,
                       u64 *d_h_out) {
    const size_t B = ags_block(ctx), n_tops = (n + B - 1) / B;
    if (ctx->ags_tops.reserve(n_tops * 32) || ctx->agm_roots.reserve(32)) return SSA_ERR_HIP;
    if (int rc = ags_tops(ctx, d_lanes, stride, d_pks, mv, n, B, (u64 *)ctx->ags_tops.p, d_h_out)) return rc;
    return ags_root(ctx, (const u64 *)ctx->ags_tops.p, n_tops, n, (u64 *)ctx->agm_roots.p);
}

// The producer of one aggregate behind both device forms: they differ in how the lanes become e_agg and the R's.  One
// MSM slice at most: ag_transcript, ag_fold, and ag_k_pack once the aggregate is not refused.  sliced (any n <=
// SSA_MAX_BATCH): ags_root_of, and ags_fold packs the R's piece by piece.  Synchronises the stream: the status it returns
// is read from the device.
static int ag_produce(ssa_ctx *ctx, const DevBatch &b, size_t n, uint32_t flags, uint8_t *d_agg_out, uint8_t *d_status_out,
                      uint64_t *d_n_fail_out, bool sliced) {
    if (!ctx || !d_agg_out || (flags & ~SSA_AGG_CHECK) || (n && (!b.sigs || !b.pks))) return SSA_ERR_ARG;
    if (int rc = agg_check_args(ctx, b.msgs, n, sliced)) return rc;
    unsigned long long *d_fail;
    if (int rc = reset_fail_counter(ctx, d_n_fail_out, &d_fail)) return rc;
    if (n == 0) {
        HIP_TRY(hipMemsetAsync(d_agg_out, 0, 32, ctx->stream));
        return SSA_OK;
    }
    u8 *d_status = ag_status_buf(ctx, d_status_out, n);
    if (!d_status || (sliced && ctx->ag_misc.reserve(AG_MISC_BYTES))) return SSA_ERR_HIP;
    const bool screened = (flags & SSA_AGG_CHECK) != 0;
    if (screened)
        if (int rc = ssa_verify_batch_screened_device(ctx, b.sigs, b.pks, b.pk_inf, b.msgs.msgs, b.msgs.off, b.msgs.stride,
                                                      b.msgs.len, n, nullptr, 0, d_status, (uint64_t *)d_fail))
            return rc;
    u8 *d_fold_status = screened ? (u8 *)nullptr : d_status;
    if (sliced) {
        if (int rc = ags_root_of(ctx, b.sigs, 81, b.pks, b.msgs, n, nullptr)) return rc;
        if (int rc = ags_fold(ctx, b, n, 0, (const u64 *)ctx->agm_roots.p, ag_misc(ctx, AG_E), d_agg_out, d_fold_status, d_fail))
            return rc;
    } else {
        if (int rc = ag_transcript(ctx, nullptr, b.sigs, b.pks, b.msgs, n, false, nullptr, 1, ag_uniform_passes(n))) return rc;
        if (int rc = ag_fold(ctx, b.sigs, b.pks, b.pk_inf, n, d_fold_status, d_fail)) return rc;
    }
    int st;
    if (int rc = ag_refusal(ctx, n, screened, d_status, d_fail, d_agg_out, &st)) return rc;
    if (st) return st;     // refused: no aggregate
    if (!sliced) {
        hipLaunchKernelGGL(ag_k_pack, dim3(grid_for((n * 49 + 3) / 4, 256)), dim3(256), 0, ctx->stream, b.sigs, n, d_agg_out);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipMemcpyAsync(d_agg_out + 49 * n, ag_misc(ctx, AG_E), 32, hipMemcpyDeviceToDevice, ctx->stream));
    return SSA_OK;
}

extern "C" int ssa_aggregate_many_device(ssa_ctx *ctx, const uint8_t *d_sigs, const uint8_t *d_pks, const uint8_t *d_pk_inf,
                                         const uint8_t *d_msgs, const uint64_t *d_msg_off, size_t msg_stride,
                                         size_t msg_len, size_t n, uint32_t flags, uint8_t *d_agg_out,
                                         uint8_t *d_status_out, uint64_t *d_n_fail_out) {
    return ag_produce(ctx, {d_sigs, d_pks, d_pk_inf, {d_msgs, d_msg_off, msg_stride, msg_len}}, n, flags, d_agg_out,
                      d_status_out, d_n_fail_out, false);
}

extern "C" int ssa_aggregate_many_sliced_device(ssa_ctx *ctx, const uint8_t *d_sigs, const uint8_t *d_pks,
                                                const uint8_t *d_pk_inf, const uint8_t *d_msgs, const uint64_t *d_msg_off,
                                                size_t msg_stride, size_t msg_len, size_t n, uint32_t flags,
                                                uint8_t *d_agg_out, uint8_t *d_status_out, uint64_t *d_n_fail_out) {
    return ag_produce(ctx, {d_sigs, d_pks, d_pk_inf, {d_msgs, d_msg_off, msg_stride, msg_len}}, n, flags, d_agg_out,
                      d_status_out, d_n_fail_out, true);
}

extern "C" int ssa_aggregate_many_sliced(ssa_ctx *ctx, const uint8_t *sigs, const uint8_t *pks, const uint8_t *pk_inf,
                                         const uint8_t *msgs, const uint64_t *msg_off, size_t msg_stride, size_t msg_len,
                                         size_t n, uint32_t flags, uint8_t *agg_out, uint8_t *status_out,
                                         uint64_t *n_fail_out) {
    return aggregate_many_host(ctx, sigs, pks, pk_inf, msgs, msg_off, msg_stride, msg_len, n, flags, agg_out, status_out,
                               n_fail_out, true);
}

// Only enqueues.  The challenge scalars of all n lanes stay in ctx->ws_h between the two walks (32 bytes per lane);
// everything else is one piece's workspace.
extern "C" int ssa_verify_aggregate_sliced_device(ssa_ctx *ctx, const uint8_t *d_agg, const uint8_t *d_pks,
                                                  const uint8_t *d_pk_inf, const uint8_t *d_msgs, const uint64_t *d_msg_off,
                                                  size_t msg_stride, size_t msg_len, size_t n, uint32_t *d_verdict_out) {
    const MsgView mv{d_msgs, d_msg_off, msg_stride, msg_len};
    if (!ctx || !d_agg || !d_verdict_out || (n && !d_pks)) return SSA_ERR_ARG;
    if (int rc = agg_check_args(ctx, mv, n, true)) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    if (n) {
        if (ctx->ag_misc.reserve(AG_MISC_BYTES) || ctx->ws_h.reserve(n * 32)) return SSA_ERR_HIP;
        if (int rc = ags_root_of(ctx, d_agg, 49, d_pks, mv, n, (u64 *)ctx->ws_h.p)) return rc;
        if (int rc = ags_record(ctx, d_agg, {nullptr, d_pks, d_pk_inf, mv}, (const u64 *)ctx->ws_h.p, n, 0,
                                (const u64 *)ctx->agm_roots.p, (u64 *)ag_misc(ctx, AG_REC), n <= ags_piece(ctx, ags_block(ctx))))
            return rc;
    }
    return timed_launch(ctx, "ag_k_finish", [&] {
        hipLaunchKernelGGL(ag_k_finish, dim3(1), dim3(64), 0, ctx->stream, (const u64 *)ag_misc(ctx, AG_REC), d_agg,
                           (const u32 *)nullptr, n, 0u, (const u64 *)ctx->d_gtab, d_verdict_out);
    });
}

extern "C" int ssa_verify_aggregate_sliced(ssa_ctx *ctx, const uint8_t *agg, const uint8_t *pks, const uint8_t *pk_inf,
                                           const uint8_t *msgs, const uint64_t *msg_off, size_t msg_stride, size_t msg_len,
                                           size_t n) {
    return verify_aggregate_host(ctx, agg, pks, pk_inf, msgs, msg_off, msg_stride, msg_len, n, true);
}

// ------------------------------------------------------------------ streaming aggregator (ssa_aggregator.hpp)
// The rules of both streaming objects (AgxStore: ssa_aggregator, ssa_aggverifier), each written once.
// B of a block_lanes argument: 0 means AG_TREE_SPAN, otherwise a power of two from 2 to AG_TREE_SPAN; 0: refused
static size_t agx_block(uint64_t block_lanes) {
    const uint64_t B = block_lanes ? block_lanes : AG_TREE_SPAN;
    return is_pow2((size_t)B) && B >= 2 && B <= AG_TREE_SPAN ? (size_t)B : 0;
}

// the lanes an n_take argument takes of the object: SIZE_MAX means all held, more than are held is refused
static int agx_take(const ssa_ctx *ctx, const AgxStore *s, size_t n_take, size_t *n_out) {
    if (!ctx || !s || s->ctx != ctx) return SSA_ERR_ARG;
    *n_out = n_take == SIZE_MAX ? s->held : n_take;
    return *n_out > s->held ? SSA_ERR_ARG : 0;
}

// (the caller puts *out on the context's list of live objects of the type)
template <class T>
static int agx_create(ssa_ctx *ctx, size_t capacity, size_t block_lanes, uint32_t flags, T **out) {
    if (out) *out = nullptr;
    const size_t B = agx_block(block_lanes);
    if (!ctx || !out || (flags & ~T::kCreateFlags) || capacity == 0 || capacity > SSA_MAX_BATCH || !B) return SSA_ERR_ARG;
    HIP_TRY(hipSetDevice(ctx->device));
    T *obj = new T();
    obj->ctx = ctx;
    obj->flags = flags;
    obj->capacity = capacity;
    obj->block = B;
    // everything the object will ever hold, now: no push or finish allocates for it
    for (const AgxStore::Buf &b : agx_bufs(*obj))
        if (b.buf->reserve_exact(b.bytes)) {
            (void)hipGetLastError();
            agx_release_all(*obj);
            delete obj;
            return SSA_ERR_HIP;
        }
    *out = obj;
    return 0;
}

template <class T>
static void agx_destroy(T *obj, std::vector<T *> ssa_ctx::*live) {
    if (!obj) return;
    if (obj->ctx) {
        (void)hipSetDevice(obj->ctx->device);
        (void)hipStreamSynchronize(obj->ctx->stream);
        forget_handle(obj->ctx->*live, obj);
        agx_release_all(*obj);
    }
    delete obj;
}

extern "C" int ssa_debug_aggregator_plan(uint64_t held, uint64_t m, uint64_t block_lanes, uint64_t out[4]) {
    const size_t B = agx_block(block_lanes);
    if (!out || !B || held > SSA_MAX_BATCH || m > SSA_MAX_BATCH - held) return SSA_ERR_ARG;
    const AgxPlan p = agx_plan(held, m, B);
    out[0] = p.first;
    out[1] = p.count;
    out[2] = p.tail_first;
    out[3] = p.tail_len;
    return 0;
}

// the eight words of ssa_debug_aggregator_bytes_ex: each optional column has its own word, whichever flags are set
static int agx_bytes_words(size_t capacity, size_t block_lanes, uint32_t flags, uint64_t w[8]) {
    const size_t B = agx_block(block_lanes);
    if ((flags & ~ssa_aggregator::kCreateFlags) || capacity == 0 || capacity > SSA_MAX_BATCH || !B) return SSA_ERR_ARG;
    ssa_aggregator a;          // (never allocated: agx_bufs only says what create would reserve)
    a.capacity = capacity;
    a.block = B;
    a.flags = flags;
    std::fill(w, w + 8, (uint64_t)0);
    size_t k = 0;
    for (const AgxStore::Buf &b : agx_bufs(a)) {
        if (b.buf == &a.keys) k = 4;
        if (b.buf == &a.adm) k = 5;
        if (b.buf == &a.index) k = 6;
        w[k++] = b.bytes;
    }
    return 0;
}

// (five words, as before the admission column and the leaf index existed: their flags are accepted, neither is reported
// here)
extern "C" int ssa_debug_aggregator_bytes(size_t capacity, size_t block_lanes, uint32_t flags, uint64_t out[5]) {
    uint64_t w[8];
    if (!out) return SSA_ERR_ARG;
    if (int rc = agx_bytes_words(capacity, block_lanes, flags, w)) return rc;
    std::copy(w, w + 5, out);
    return 0;
}

extern "C" int ssa_debug_aggregator_bytes_ex(size_t capacity, size_t block_lanes, uint32_t flags, uint64_t out[8]) {
    return out ? agx_bytes_words(capacity, block_lanes, flags, out) : SSA_ERR_ARG;
}

extern "C" int ssa_aggregator_create(ssa_ctx *ctx, size_t capacity, size_t block_lanes, uint32_t flags, ssa_aggregator **out) {
    const int rc = agx_create(ctx, capacity, block_lanes, flags, out);
    if (rc == 0) ctx->aggregators.push_back(*out);
    return rc;
}

extern "C" void ssa_aggregator_destroy(ssa_aggregator *ag) { agx_destroy(ag, &ssa_ctx::aggregators); }

// Nothing on the device needs clearing: every array is written before it is read, up to `held` (the admission column
// too: it is forgotten with the lanes).
extern "C" int ssa_aggregator_reset(ssa_aggregator *ag) {
    if (!ag || !ag->ctx) return SSA_ERR_ARG;
    ag->held = 0;
    ag->pushes = ag->offered = ag->dropped = ag->finishes = 0;
    ag->index_void();        // (the leaf index: cleared by the next index_sync or look-up, not here)
    return 0;
}

extern "C" int ssa_aggregator_info(ssa_aggregator *ag, uint64_t out[8]) {
    if (!ag || !ag->ctx || !out) return SSA_ERR_ARG;
    out[0] = ag->held;
    out[1] = ag->capacity;
    out[2] = ag->block;
    out[3] = ag->pushes;
    out[4] = ag->offered;
    out[5] = ag->dropped;
    out[6] = ag->held / ag->block;
    out[7] = ag->finishes;
    return 0;
}

// what every form of push refuses before anything is enqueued or counted.  sigs, pks: the inputs that must not be null
// when n != 0 (records: both the records).  keyed: the lanes are KeyedSignature records -- the only push that carries the
// wire key an object with a key column holds.
static int agx_push_args(const ssa_ctx *ctx, const ssa_aggregator *ag, const MsgView &mv, size_t n, uint32_t flags,
                         const void *sigs, const void *pks, const uint64_t *n_kept_out, bool keyed = false) {
    if (!ctx || !ag || ag->ctx != ctx || !n_kept_out || (flags & ~SSA_AGGR_NO_SCREEN) || (n && (!sigs || !pks)) ||
        (ag->hold_keys() && !keyed))
        return SSA_ERR_ARG;
    if (int rc = agg_check_args(ctx, mv, n)) return rc;
    return n > ag->capacity - ag->held ? SSA_ERR_ARG : 0;      // by n, not by the kept count: never applied in part
}

// The blocks [first, first + count) of an object (a streaming aggregator or aggregate verifier: its leaves, its tops, its
// B), complete since this push, reduced to their tops.  B = 512: ONE launch of ag_k_tree over that range of the leaves, a
// workgroup per block (the uniform cut, no top).  Smaller B: log2 B launches of ag_k_level over the count * B leaves --
// every level is even, no node moves up unchanged -- between ctx->ag_nodes and ctx->ag_nodes2; the first reads the
// object's leaves, the last writes the object's tops.
static int agx_reduce_blocks(const AgxStore &s, const AgxPlan &p) {
    ssa_ctx *ctx = s.ctx;
    const size_t B = s.block, cnt = (size_t)p.count * B;
    const u64 *src = (const u64 *)s.leaves.p + 4 * (size_t)p.first * B;
    u64 *dst = (u64 *)s.tops.p + 4 * (size_t)p.first;
    if (B == AG_TREE_SPAN)
        return timed_launch(ctx, "ag_k_tree", [&] {
            hipLaunchKernelGGL(ag_k_tree, dim3((unsigned)p.count), dim3(256), 0, ctx->stream, ctx->d_params, src,
                               (const AgTreeDesc *)nullptr, (u32)cnt, 0u, dst, (u64 *)nullptr);
        });
    unsigned launches = 0;
    for (size_t l = B; l > 1; l /= 2) launches++;
    if (ctx->ag_nodes.reserve(cnt / 2 * 32) || ctx->ag_nodes2.reserve(cnt / 4 * 32 + 32)) return SSA_ERR_HIP;
    u64 *bufs[2] = {(u64 *)ctx->ag_nodes.p, (u64 *)ctx->ag_nodes2.p};
    return timed_launch(ctx, "ag_k_level", [&] {
        size_t c = cnt;
        const u64 *in = src;
        for (unsigned l = 0; l < launches; l++, c /= 2) {
            u64 *o = l + 1 == launches ? dst : bufs[l & 1u];
            hipLaunchKernelGGL(ag_k_level, dim3(grid_for(c / 2, 256)), dim3(256), 0, ctx->stream, ctx->d_params, in, c, o);
            in = o;
        }
    });
}

// The root of the first n (>= 1) lanes of an object (its leaves, its tops, its B) into ctx->agm_roots: the stored tops of
// the n / B complete blocks are copied into ctx->ags_tops, the ragged block [B (n / B), n) is reduced behind them by one
// workgroup of ag_k_tree -- into the workspace, never into the object: with n below the lanes held that slot is a complete
// block's top -- and ags_root finishes the tree.
static int agx_root(const AgxStore &s, size_t n) {
    ssa_ctx *ctx = s.ctx;
    const DevBuf &leaves = s.leaves, &tops = s.tops;
    const AgxPlan p = agx_plan(0, n, s.block);       // p.count stored tops, then the ragged block's
    const size_t n_tops = (size_t)p.count + (p.tail_len ? 1 : 0);
    if (ctx->ags_tops.reserve(n_tops * 32) || ctx->agm_roots.reserve(32)) return SSA_ERR_HIP;
    u64 *d_tops = (u64 *)ctx->ags_tops.p;
    if (p.count)
        HIP_TRY(hipMemcpyAsync(d_tops, tops.p, (size_t)p.count * 32, hipMemcpyDeviceToDevice, ctx->stream));
    if (p.tail_len) {        // fewer than B <= 512 leaves: one workgroup, the odd-node rule, no root
        const int rc = timed_launch(ctx, "ag_k_tree", [&] {
            hipLaunchKernelGGL(ag_k_tree, dim3(1), dim3(256), 0, ctx->stream, ctx->d_params,
                               (const u64 *)leaves.p + 4 * (size_t)p.tail_first, (const AgTreeDesc *)nullptr,
                               (u32)p.tail_len, 0u, d_tops + 4 * (size_t)p.count, (u64 *)nullptr);
        });
        if (rc) return rc;
    }
    return ags_root(ctx, d_tops, n_tops, n, (u64 *)ctx->agm_roots.p);
}

// The tail of every push, behind the n statuses of its admission (with the raw digests of all n lanes in ctx->ag_dig):
// the kept lanes are listed (av_keep, one synchronisation for their number), appended -- the lanes are records of
// `stride` bytes at d_recs with the signature at `off`, and an object with a key column keeps the records' first 49
// bytes -- the blocks this push completed are reduced, and the object counts the push.  adm_class (SSA_ADM_*): what this
// kind of push establishes of a lane it keeps; an object with an admission column records it for the m kept lanes, one
// memset behind the append (the count is on the host by then).
static int agx_admit(ssa_ctx *ctx, ssa_aggregator *ag, const u8 *d_status, size_t n, const u8 *d_recs, u32 stride, u32 off,
                     u32 adm_class, uint64_t *n_kept_out) {
    if (ctx->agx_kept.reserve(n * sizeof(u32))) return SSA_ERR_HIP;
    uint64_t m = 0;
    if (int rc = av_keep(ctx, d_status, n, (u32 *)ctx->agx_kept.p, &m)) return rc;
    if (m) {
        int rc = timed_launch(ctx, "agx_k_append", [&] {
            hipLaunchKernelGGL(agx_k_append, dim3(grid_for(m, 256)), dim3(256), 0, ctx->stream, ctx->d_params, d_recs, stride,
                               off, (const u64 *)ctx->ag_dig.p, (const u32 *)ctx->agx_kept.p, (size_t)m, ag->held,
                               (u64 *)ag->leaves.p, (u64 *)ag->scal.p, (u8 *)ag->wire.p,
                               ag->hold_keys() ? (u8 *)ag->keys.p : (u8 *)nullptr);
        });
        if (rc) return rc;
        if (ag->hold_adm()) HIP_TRY(hipMemsetAsync((u8 *)ag->adm.p + ag->held, (int)adm_class, m, ctx->stream));
        const AgxPlan p = agx_plan(ag->held, m, ag->block);
        if (p.count)
            if ((rc = agx_reduce_blocks(*ag, p))) return rc;
    }
    // (only now: a launch that could not be enqueued leaves the object as it was -- what it wrote lies behind `held`)
    ag->held += m;
    ag->pushes++;
    ag->offered += n;
    ag->dropped += n - m;
    *n_kept_out = m;
    return SSA_OK;
}

// Synchronises the stream as ssa_aggregate_valid_many_device does: once inside the screen (not at all with
// SSA_AGGR_NO_SCREEN or for at most msm_small_max lanes) and once for the kept count, which the object keeps on the host
// from then on.
extern "C" int ssa_aggregator_push_device(ssa_ctx *ctx, ssa_aggregator *ag, const uint8_t *d_sigs, const uint8_t *d_pks,
                                          const uint8_t *d_pk_inf, const uint8_t *d_msgs, const uint64_t *d_msg_off,
                                          size_t msg_stride, size_t msg_len, size_t n, uint32_t flags, uint8_t *d_status_out,
                                          uint64_t *n_kept_out) {
    const DevBatch b{d_sigs, d_pks, d_pk_inf, {d_msgs, d_msg_off, msg_stride, msg_len}};
    if (int rc = agx_push_args(ctx, ag, b.msgs, n, flags, d_sigs, d_pks, n_kept_out)) return rc;
    *n_kept_out = 0;
    HIP_TRY(hipSetDevice(ctx->device));
    if (n == 0) {
        ag->pushes++;
        return SSA_OK;
    }
    u8 *d_status = ag_status_buf(ctx, d_status_out, n);
    if (!d_status) return SSA_ERR_HIP;
    // ONE challenge hash over the n lanes: the raw digests for the leaves and, screened, the scalars mod q for the screen
    const bool screen = !(flags & SSA_AGGR_NO_SCREEN);
    if (int rc = ag_transcript_front(ctx, nullptr, &d_sigs, d_pks, b.msgs, n, screen, nullptr, 1)) return rc;
    if (screen) {
        if (int rc = ssa_internal_screen_hashed(ctx, b, n, (const uint64_t *)ctx->ws_h.p, d_status, nullptr)) return rc;
    } else {
        const int rc = timed_launch(ctx, "agx_k_check", [&] {
            hipLaunchKernelGGL(agx_k_check, dim3(grid_for(n, 256)), dim3(256), 0, ctx->stream, d_sigs, d_pks, d_pk_inf, n,
                               d_status);
        });
        if (rc) return rc;
    }
    return agx_admit(ctx, ag, d_status, n, d_sigs, 81, 0, screen ? SSA_ADM_SCREENED : SSA_ADM_UNSCREENED, n_kept_out);
}

extern "C" int ssa_aggregator_push(ssa_ctx *ctx, ssa_aggregator *ag, const uint8_t *sigs, const uint8_t *pks,
                                   const uint8_t *pk_inf, const uint8_t *msgs, const uint64_t *msg_off, size_t msg_stride,
                                   size_t msg_len, size_t n, uint32_t flags, uint8_t *status_out, uint64_t *n_kept_out) {
    if (int rc = agx_push_args(ctx, ag, {msgs, msg_off, msg_stride, msg_len}, n, flags, sigs, pks, n_kept_out)) return rc;
    if (int rc = check_host_offsets(msg_off, n)) return rc;
    if (n == 0) return ssa_aggregator_push_device(ctx, ag, nullptr, nullptr, nullptr, nullptr, nullptr, msg_stride, msg_len, 0,
                                                  flags, nullptr, n_kept_out);
    HostCall hc(ctx);
    const DevBatch b = hc.lanes({sigs, pks, pk_inf, msgs, msg_off, msg_stride, msg_len}, n * 81, n);
    u8 *d_status = hc.out(ctx->st_status, status_out, n, 16);
    return hc.finish([&] {
        return ssa_aggregator_push_device(ctx, ag, b.sigs, b.pks, b.pk_inf, b.msgs.msgs, b.msgs.off, msg_stride, msg_len, n,
                                          flags, d_status, n_kept_out);
    });
}

// e_agg of n (>= 1) lanes whose scalars stand at d_scal, four words per lane, lane i at place i of the aggregate, under
// the root in ctx->agm_roots: agx_k_coeff_fold per piece of at most one MSM slice, ag_k_fold_finish per piece and over
// the pieces, into ag_misc(ctx, AG_E).  What finish runs on the object's scalars and finish_select on the gathered ones.
static int agx_fold(ssa_ctx *ctx, const u64 *d_scal, size_t n) {
    const size_t piece = ags_piece(ctx), k = (n + piece - 1) / piece;
    if (ctx->ag_misc.reserve(AG_MISC_BYTES) || ctx->ags_parts.reserve(k * 32) ||
        ctx->ag_partials.reserve((size_t)grid_for(std::min(piece, n), 256) * 32))
        return SSA_ERR_HIP;
    const u64 *d_root = (const u64 *)ctx->agm_roots.p;
    for (size_t lo = 0, j = 0; lo < n; lo += piece, j++) {
        const size_t cnt = std::min(piece, n - lo);
        const unsigned n_blocks = grid_for(cnt, 256);
        int rc = timed_launch(ctx, "agx_k_coeff_fold", [&] {
            hipLaunchKernelGGL(agx_k_coeff_fold, dim3(n_blocks), dim3(256), 0, ctx->stream, ctx->d_params, d_root,
                               d_scal + 4 * lo, cnt, (u64)lo, (u64 *)ctx->ag_partials.p);
        });
        if (rc) return rc;
        rc = timed_launch(ctx, "ag_k_fold_finish", [&] {
            hipLaunchKernelGGL(ag_k_fold_finish, dim3(1), dim3(256), 0, ctx->stream, (const u64 *)ctx->ag_partials.p, n_blocks,
                               k == 1 ? ag_misc(ctx, AG_E) : (u8 *)ctx->ags_parts.p + 32 * j);
        });
        if (rc) return rc;
    }
    if (k > 1) {
        const int rc = timed_launch(ctx, "ag_k_fold_finish", [&] {
            hipLaunchKernelGGL(ag_k_fold_finish, dim3(1), dim3(256), 0, ctx->stream, (const u64 *)ctx->ags_parts.p, (u32)k,
                               ag_misc(ctx, AG_E));
        });
        if (rc) return rc;
    }
    return SSA_OK;
}

// Only enqueues on the context's stream: every size it needs is on the host.  Reads the object, writes workspaces of the
// context and the caller's buffer.
extern "C" int ssa_aggregator_finish_device(ssa_ctx *ctx, ssa_aggregator *ag, size_t n_take, uint8_t *d_agg_out) {
    size_t n;
    if (int rc = agx_take(ctx, ag, n_take, &n)) return rc;
    if (!d_agg_out) return SSA_ERR_ARG;
    HIP_TRY(hipSetDevice(ctx->device));
    ag->finishes++;
    if (n == 0) {
        HIP_TRY(hipMemsetAsync(d_agg_out, 0, 32, ctx->stream));
        return SSA_OK;
    }
    if (int rc = agx_root(*ag, n)) return rc;
    if (int rc = agx_fold(ctx, (const u64 *)ag->scal.p, n)) return rc;
    HIP_TRY(hipMemcpyAsync(d_agg_out, ag->wire.p, 49 * n, hipMemcpyDeviceToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(d_agg_out + 49 * n, ag_misc(ctx, AG_E), 32, hipMemcpyDeviceToDevice, ctx->stream));
    return SSA_OK;
}

extern "C" int ssa_aggregator_finish(ssa_ctx *ctx, ssa_aggregator *ag, size_t n_take, uint8_t *agg_out) {
    size_t n;
    if (int rc = agx_take(ctx, ag, n_take, &n)) return rc;
    if (!agg_out) return SSA_ERR_ARG;
    HostCall hc(ctx);
    u8 *d_agg = hc.out(ctx->st_aux, agg_out, SSA_AGGREGATE_LENGTH(n), 16);
    return hc.finish([&] { return ssa_aggregator_finish_device(ctx, ag, n, d_agg); });
}

// ---- the key column (SSA_AGGR_HOLD_KEYS49)
// Only enqueues: one device-to-device copy.  Changes no state of the object.
extern "C" int ssa_aggregator_keys_device(ssa_ctx *ctx, ssa_aggregator *ag, size_t n_take, uint8_t *d_keys49_out) {
    size_t n;
    if (int rc = agx_take(ctx, ag, n_take, &n)) return rc;
    if (!ag->hold_keys() || (n && !d_keys49_out)) return SSA_ERR_ARG;
    if (n == 0) return SSA_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipMemcpyAsync(d_keys49_out, ag->keys.p, 49 * n, hipMemcpyDeviceToDevice, ctx->stream));
    return SSA_OK;
}

extern "C" int ssa_aggregator_keys(ssa_ctx *ctx, ssa_aggregator *ag, size_t n_take, uint8_t *keys49_out) {
    size_t n;
    if (int rc = agx_take(ctx, ag, n_take, &n)) return rc;
    if (!ag->hold_keys() || (n && !keys49_out)) return SSA_ERR_ARG;
    if (n == 0) return SSA_OK;
    HostCall hc(ctx);
    u8 *d_keys = hc.out(ctx->st_aux, keys49_out, 49 * n, 16);
    return hc.finish([&] { return ssa_aggregator_keys_device(ctx, ag, n, d_keys); });
}

// ---- the admission column (SSA_AGGR_HOLD_ADMISSION)
// Only enqueues: one device-to-device copy.  Changes no state of the object.
extern "C" int ssa_aggregator_admission_device(ssa_ctx *ctx, ssa_aggregator *ag, size_t n_take, uint8_t *d_adm_out) {
    size_t n;
    if (int rc = agx_take(ctx, ag, n_take, &n)) return rc;
    if (!ag->hold_adm() || (n && !d_adm_out)) return SSA_ERR_ARG;
    if (n == 0) return SSA_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipMemcpyAsync(d_adm_out, ag->adm.p, n, hipMemcpyDeviceToDevice, ctx->stream));
    return SSA_OK;
}

extern "C" int ssa_aggregator_admission(ssa_ctx *ctx, ssa_aggregator *ag, size_t n_take, uint8_t *adm_out) {
    size_t n;
    if (int rc = agx_take(ctx, ag, n_take, &n)) return rc;
    if (!ag->hold_adm() || (n && !adm_out)) return SSA_ERR_ARG;
    if (n == 0) return SSA_OK;
    HostCall hc(ctx);
    u8 *d_adm = hc.out(ctx->st_aux, adm_out, n, 16);
    return hc.finish([&] { return ssa_aggregator_admission_device(ctx, ag, n, d_adm); });
}

// ---- removing lanes in place (the move and its hazard: agx_k_move in ssa_aggregator.hpp)
// (a first_changed of 0 is planned as the front drop of held - new_held lanes: see the header)
extern "C" int ssa_debug_aggregator_remove_plan(uint64_t held, uint64_t first_changed, uint64_t new_held,
                                                uint64_t block_lanes, uint64_t out[4]) {
    const size_t B = agx_block(block_lanes);
    if (!out || !B || held > SSA_MAX_BATCH || new_held > held || first_changed > new_held) return SSA_ERR_ARG;
    const AgxRemovePlan p = agx_remove_plan(held, first_changed, new_held, B, first_changed == 0);
    out[0] = p.unchanged;
    out[1] = p.moved;
    out[2] = p.first;
    out[3] = p.count;
    return 0;
}

// The staging of P gathered lanes (a piece of the move, a selection) in `buf`: P leaves, P scalars, 49 P bytes of R's and
// -- with_keys -- 49 P bytes of keys behind the R's part rounded up to a dword (each part dword-aligned, and more);
// -- with_adm -- P bytes of admission classes behind everything else (bytes: any alignment does).
struct AgxStage {
    u64 *leaves, *scal;
    u8 *wire, *keys, *adm;
};
static int agx_stage_layout(DevBuf &buf, size_t P, bool with_keys, AgxStage *st, bool with_adm = false) {
    const size_t wire_part = with_keys ? (49 * P + 3) & ~(size_t)3 : 49 * P;
    const size_t front = 64 * P + wire_part + (with_keys ? 49 * P : 0);
    if (buf.reserve(front + 16 + (with_adm ? P + 16 : 0))) return SSA_ERR_HIP;
    st->leaves = (u64 *)buf.p;
    st->scal = st->leaves + 4 * P;
    st->wire = (u8 *)(st->scal + 4 * P);
    st->keys = with_keys ? st->wire + wire_part : nullptr;
    st->adm = with_adm ? (u8 *)buf.p + front + 16 : nullptr;
    return 0;
}

// The m kept lanes of an object -- ascending: d_kept[c], or c + (held - m) for a front drop, which has no list
// (d_kept == nullptr) -- take the places [0, m).  f: the first place whose content changes.  Only enqueues.  The move is
// in place and cannot be undone: once its first launch is enqueued, an error leaves the object EMPTY, never half-moved.
static int agx_remove_apply(ssa_aggregator *ag, const u32 *d_kept, size_t f, size_t m) {
    ssa_ctx *ctx = ag->ctx;
    const size_t held = ag->held, B = ag->block, shift = d_kept ? 0 : held - m;
    if (m == held) return SSA_OK;
    const AgxRemovePlan p = agx_remove_plan(held, f, m, B, !d_kept);
    const size_t P = f < m ? std::min(ags_piece(ctx), m - f) : 0, top0 = shift / B;
    const bool tops_overlap = p.moved && top0 < p.moved;
    const bool hold = ag->hold_keys(), hold_adm = ag->hold_adm();
    AgxStage st{};
    if ((P && agx_stage_layout(ctx->agx_stage, P, hold, &st, hold_adm)) || (tops_overlap && ctx->ags_tops.reserve((size_t)p.moved * 32)))
        return SSA_ERR_HIP;
    u64 *st_leaves = st.leaves, *st_scal = st.scal;
    u8 *st_wire = st.wire, *st_keys = st.keys, *st_adm = st.adm;
    u64 *leaves = (u64 *)ag->leaves.p, *scal = (u64 *)ag->scal.p, *tops = (u64 *)ag->tops.p;
    u8 *wire = (u8 *)ag->wire.p, *keys = hold ? (u8 *)ag->keys.p : nullptr, *adm = hold_adm ? (u8 *)ag->adm.p : nullptr;
    const int rc = [&]() -> int {
        for (size_t c0 = f; c0 < m; c0 += P) {
            const size_t cnt = std::min(P, m - c0);
            const int r = timed_launch(ctx, "agx_k_move", [&] {
                hipLaunchKernelGGL(agx_k_move, dim3(grid_for(cnt, 256)), dim3(256), 0, ctx->stream, d_kept, shift, c0, cnt,
                                   (const u64 *)leaves, (const u64 *)scal, (const u8 *)wire, (const u8 *)keys, (const u8 *)adm,
                                   st_leaves, st_scal, st_wire, st_keys, st_adm);
            });
            if (r) return r;
            // behind the gather on the stream, in front of the next piece's: places [c0, c0 + cnt) alone are written
            HIP_TRY(hipMemcpyAsync(leaves + 4 * c0, st_leaves, 32 * cnt, hipMemcpyDeviceToDevice, ctx->stream));
            HIP_TRY(hipMemcpyAsync(scal + 4 * c0, st_scal, 32 * cnt, hipMemcpyDeviceToDevice, ctx->stream));
            HIP_TRY(hipMemcpyAsync(wire + 49 * c0, st_wire, 49 * cnt, hipMemcpyDeviceToDevice, ctx->stream));
            if (hold) HIP_TRY(hipMemcpyAsync(keys + 49 * c0, st_keys, 49 * cnt, hipMemcpyDeviceToDevice, ctx->stream));
            if (hold_adm) HIP_TRY(hipMemcpyAsync(adm + c0, st_adm, cnt, hipMemcpyDeviceToDevice, ctx->stream));
        }
        if (p.moved) {       // new block b is old block b + top0; a copy onto its own source goes through a workspace
            const size_t bytes = (size_t)p.moved * 32;
            if (tops_overlap) {
                HIP_TRY(hipMemcpyAsync(ctx->ags_tops.p, tops + 4 * top0, bytes, hipMemcpyDeviceToDevice, ctx->stream));
                HIP_TRY(hipMemcpyAsync(tops, ctx->ags_tops.p, bytes, hipMemcpyDeviceToDevice, ctx->stream));
            } else {
                HIP_TRY(hipMemcpyAsync(tops, tops + 4 * top0, bytes, hipMemcpyDeviceToDevice, ctx->stream));
            }
        }
        return p.count ? agx_reduce_blocks(*ag, AgxPlan{p.first, p.count, 0, 0}) : 0;
    }();
    ag->held = rc ? 0 : m;
    ag->index_void();        // the lanes moved (or, after an error, left): the leaf index is rebuilt when it is next asked
    return rc;
}

// Only enqueues on the context's stream: every size it needs is on the host.
extern "C" int ssa_aggregator_drop_front(ssa_ctx *ctx, ssa_aggregator *ag, size_t n) {
    size_t k;
    if (int rc = agx_take(ctx, ag, n, &k)) return rc;
    if (k == 0) return SSA_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    return agx_remove_apply(ag, nullptr, 0, ag->held - k);
}

// what both forms of remove refuse before anything is enqueued
static int agx_remove_args(const ssa_ctx *ctx, const ssa_aggregator *ag, const uint8_t *drop, size_t n_bytes,
                           const uint64_t *n_kept_out) {
    return !ctx || !ag || ag->ctx != ctx || !n_kept_out || n_bytes != ag->held || (n_bytes && !drop) ? SSA_ERR_ARG : 0;
}

// The removal by a byte mask on the device (the arguments checked, lanes held).  Synchronises the stream once, for the
// kept count and the first place that changes, which are read from the device together; from then on every size is on
// the host.  d_refuse (remove_indices; nullptr: none): a word read under the same synchronisation -- nonzero refuses the
// call with SSA_ERR_ARG before the move begins, the object unchanged.
static int agx_remove_masked(ssa_ctx *ctx, ssa_aggregator *ag, const uint8_t *d_drop, const u32 *d_refuse,
                             uint64_t *n_kept_out) {
    const size_t held = ag->held;
    if (ctx->agx_kept.reserve(held * sizeof(u32)) || ctx->agx_first.reserve(sizeof(u32))) return SSA_ERR_HIP;
    u32 *d_kept = (u32 *)ctx->agx_kept.p, *d_first = (u32 *)ctx->agx_first.p;
    const u32 *d_m = nullptr;
    // a lane is kept iff its byte is zero: the status-vector convention av_keep lists by
    if (int rc = av_keep_enqueue(ctx, d_drop, held, d_kept, &d_m)) return rc;
    const int rc = timed_launch(ctx, "agx_k_first_changed", [&] {
        hipLaunchKernelGGL(agx_k_first_changed, dim3(grid_for(held + 1, 256)), dim3(256), 0, ctx->stream,
                           (const u32 *)d_kept, d_m, held, d_first);
    });
    if (rc) return rc;
    u32 m = 0, f = 0, refuse = 0;
    HIP_TRY(hipMemcpyAsync(&m, d_m, sizeof m, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(&f, d_first, sizeof f, hipMemcpyDeviceToHost, ctx->stream));
    if (d_refuse) HIP_TRY(hipMemcpyAsync(&refuse, d_refuse, sizeof refuse, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (refuse) return SSA_ERR_ARG;
    if (m > held || f > m) return SSA_ERR_HIP;        // (cannot be: the list is of `held` bytes)
    *n_kept_out = m;
    return agx_remove_apply(ag, d_kept, f, m);
}

extern "C" int ssa_aggregator_remove_device(ssa_ctx *ctx, ssa_aggregator *ag, const uint8_t *d_drop, size_t n_bytes,
                                            uint64_t *n_kept_out) {
    if (int rc = agx_remove_args(ctx, ag, d_drop, n_bytes, n_kept_out)) return rc;
    *n_kept_out = 0;
    if (ag->held == 0) return SSA_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    return agx_remove_masked(ctx, ag, d_drop, nullptr, n_kept_out);
}

extern "C" int ssa_aggregator_remove(ssa_ctx *ctx, ssa_aggregator *ag, const uint8_t *drop, size_t n_bytes,
                                     uint64_t *n_kept_out) {
    if (int rc = agx_remove_args(ctx, ag, drop, n_bytes, n_kept_out)) return rc;
    if (n_bytes == 0) return ssa_aggregator_remove_device(ctx, ag, nullptr, 0, n_kept_out);
    HostCall hc(ctx);
    const u8 *d_drop = hc.in(ctx->st_status, drop, n_bytes);
    return hc.finish([&] { return ssa_aggregator_remove_device(ctx, ag, d_drop, n_bytes, n_kept_out); });
}

// ---- a selection of held lanes in the caller's order (the gather and the validity decision:
// agx_k_select in ssa_aggregator.hpp)
// ctx->agx_sel_bits: the flag word, the result word of the host forms, and from byte 16 on one bit per held lane
constexpr size_t AGX_SEL_FLAG = 0, AGX_SEL_RESULT = 4, AGX_SEL_BITS = 16;
static size_t agx_sel_bytes(size_t held) { return AGX_SEL_BITS + 4 * ((held + 31) / 32); }
static u32 *agx_sel_word(ssa_ctx *ctx, size_t off) { return (u32 *)((u8 *)ctx->agx_sel_bits.p + off); }

// what every form of a selection refuses before anything is enqueued.  device: the list lies in device memory
static int agx_select_args(const ssa_ctx *ctx, const ssa_aggregator *ag, const uint32_t *order, size_t m, bool device) {
    if (!ctx || !ag || ag->ctx != ctx || m > ag->held || (m && !order)) return SSA_ERR_ARG;
    return device && (reinterpret_cast<uintptr_t>(order) & 3u) ? SSA_ERR_ARG : 0;
}
static int agx_finish_select_args(const ssa_ctx *ctx, const ssa_aggregator *ag, const uint32_t *order, size_t m,
                                  const uint8_t *agg_out, const uint8_t *keys49_out, bool device) {
    if (int rc = agx_select_args(ctx, ag, order, m, device)) return rc;
    return !agg_out || m > ctx->knobs.msm_slice || (keys49_out && !ag->hold_keys()) ? SSA_ERR_ARG : 0;
}

// flag, result word and the bitmap of `held` lanes, cleared on the stream: the call that uses them clears them
static int agx_select_clear(ssa_ctx *ctx, size_t held) {
    if (ctx->agx_sel_bits.reserve(agx_sel_bytes(held))) return SSA_ERR_HIP;
    HIP_TRY(hipMemsetAsync(ctx->agx_sel_bits.p, 0, agx_sel_bytes(held), ctx->stream));
    return 0;
}

// Only enqueues on the context's stream: every size it needs is on the host, and whether the list is valid is decided
// and acted upon on the device (agx_k_select raises the flag, agx_k_select_verdict zeroes the outputs of a refused list
// and writes *d_result_out).  Reads the object, writes workspaces of the context and the caller's buffers.  `finishes`
// counts every call that passed the argument checks: what the device decides later is not known here.
extern "C" int ssa_aggregator_finish_select_device(ssa_ctx *ctx, ssa_aggregator *ag, const uint32_t *d_order, size_t m,
                                                   uint8_t *d_agg_out, uint8_t *d_keys49_out, uint32_t *d_result_out) {
    if (int rc = agx_finish_select_args(ctx, ag, d_order, m, d_agg_out, d_keys49_out, true)) return rc;
    if (!d_result_out) return SSA_ERR_ARG;
    HIP_TRY(hipSetDevice(ctx->device));
    ag->finishes++;
    if (m == 0) {
        HIP_TRY(hipMemsetAsync(d_agg_out, 0, 32, ctx->stream));
        HIP_TRY(hipMemsetAsync(d_result_out, 0, sizeof(uint32_t), ctx->stream));
        return SSA_OK;
    }
    const bool with_keys = d_keys49_out != nullptr;
    AgxStage st{};
    if (agx_stage_layout(ctx->agx_sel_stage, m, with_keys, &st) || ctx->agm_roots.reserve(32)) return SSA_ERR_HIP;
    if (int rc = agx_select_clear(ctx, ag->held)) return rc;
    u32 *d_flag = agx_sel_word(ctx, AGX_SEL_FLAG);
    int rc = timed_launch(ctx, "agx_k_select", [&] {
        hipLaunchKernelGGL(agx_k_select, dim3(grid_for(m, 256)), dim3(256), 0, ctx->stream, d_order, m, ag->held,
                           agx_sel_word(ctx, AGX_SEL_BITS), d_flag, (const u64 *)ag->leaves.p, (const u64 *)ag->scal.p,
                           (const u8 *)ag->wire.p, with_keys ? (const u8 *)ag->keys.p : (const u8 *)nullptr, st.leaves,
                           st.scal, st.wire, st.keys);
    });
    if (rc) return rc;
    // the tree over the m gathered leaves from the bottom (no stored top speaks of this order), then finish's fold
    if ((rc = ags_root(ctx, st.leaves, m, m, (u64 *)ctx->agm_roots.p))) return rc;
    if ((rc = agx_fold(ctx, st.scal, m))) return rc;
    HIP_TRY(hipMemcpyAsync(d_agg_out, st.wire, 49 * m, hipMemcpyDeviceToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(d_agg_out + 49 * m, ag_misc(ctx, AG_E), 32, hipMemcpyDeviceToDevice, ctx->stream));
    if (with_keys) HIP_TRY(hipMemcpyAsync(d_keys49_out, st.keys, 49 * m, hipMemcpyDeviceToDevice, ctx->stream));
    const size_t n_agg = SSA_AGGREGATE_LENGTH(m), n_keys = with_keys ? 49 * m : 0;
    return timed_launch(ctx, "agx_k_select_verdict", [&] {
        hipLaunchKernelGGL(agx_k_select_verdict, dim3(std::min(grid_for(n_agg, 256), 4096u)), dim3(256), 0, ctx->stream,
                           (const u32 *)d_flag, d_agg_out, n_agg, d_keys49_out, n_keys, d_result_out);
    });
}

// The flag comes back with the results, under the one synchronisation a host form needs anyway.
extern "C" int ssa_aggregator_finish_select(ssa_ctx *ctx, ssa_aggregator *ag, const uint32_t *order, size_t m,
                                            uint8_t *agg_out, uint8_t *keys49_out) {
    if (int rc = agx_finish_select_args(ctx, ag, order, m, agg_out, keys49_out, false)) return rc;
    HostCall hc(ctx);
    const u32 *d_order = hc.in<u32>(ctx->agx_sel_order, order, m * sizeof(u32));
    u8 *d_agg = hc.out(ctx->st_aux, agg_out, SSA_AGGREGATE_LENGTH(m), 16);
    u8 *d_keys = keys49_out ? hc.out(ctx->st_aux2, keys49_out, 49 * m, 16) : nullptr;
    // (reserved here at the size the device form asks for: the result word does not move under it)
    if (hc.ok() && ctx->agx_sel_bits.reserve(agx_sel_bytes(ag->held))) hc.rc = SSA_ERR_HIP;
    if (!hc.ok()) return hc.rc;
    u32 refused = 0, *d_result = agx_sel_word(ctx, AGX_SEL_RESULT);
    hc.copy_back(&refused, d_result, sizeof refused);
    if (int rc = hc.finish([&] { return ssa_aggregator_finish_select_device(ctx, ag, d_order, m, d_agg, d_keys, d_result); }))
        return rc;
    return refused ? SSA_ERR_ARG : SSA_OK;
}

// remove with a list in place of a mask: the list is validated as a selection's (agx_k_mark), one small kernel turns the
// bitmap into the byte mask, and from there on it is the path of remove_device -- which reads the flag under the one
// synchronisation it makes for the kept count, before the move begins.  No slice limit: nothing here is per-slice.
extern "C" int ssa_aggregator_remove_indices_device(ssa_ctx *ctx, ssa_aggregator *ag, const uint32_t *d_order, size_t m,
                                                    uint64_t *n_kept_out) {
    if (int rc = agx_select_args(ctx, ag, d_order, m, true)) return rc;
    if (!n_kept_out) return SSA_ERR_ARG;
    const size_t held = ag->held;
    *n_kept_out = held;
    if (m == 0) return SSA_OK;       // (then nothing is removed, and nothing is launched)
    HIP_TRY(hipSetDevice(ctx->device));
    if (ctx->agx_sel_mask.reserve(held)) return SSA_ERR_HIP;
    if (int rc = agx_select_clear(ctx, held)) return rc;
    u32 *d_flag = agx_sel_word(ctx, AGX_SEL_FLAG), *d_bits = agx_sel_word(ctx, AGX_SEL_BITS);
    u8 *d_mask = (u8 *)ctx->agx_sel_mask.p;
    int rc = timed_launch(ctx, "agx_k_mark", [&] {
        hipLaunchKernelGGL(agx_k_mark, dim3(grid_for(m, 256)), dim3(256), 0, ctx->stream, d_order, m, held, d_bits, d_flag);
    });
    if (rc) return rc;
    rc = timed_launch(ctx, "agx_k_bits_to_mask", [&] {
        hipLaunchKernelGGL(agx_k_bits_to_mask, dim3(grid_for(held, 256)), dim3(256), 0, ctx->stream, (const u32 *)d_bits,
                           held, d_mask);
    });
    if (rc) return rc;
    return agx_remove_masked(ctx, ag, d_mask, d_flag, n_kept_out);
}

extern "C" int ssa_aggregator_remove_indices(ssa_ctx *ctx, ssa_aggregator *ag, const uint32_t *order, size_t m,
                                             uint64_t *n_kept_out) {
    if (int rc = agx_select_args(ctx, ag, order, m, false)) return rc;
    if (!n_kept_out) return SSA_ERR_ARG;
    if (m == 0) return ssa_aggregator_remove_indices_device(ctx, ag, nullptr, 0, n_kept_out);
    HostCall hc(ctx);
    const u32 *d_order = hc.in<u32>(ctx->agx_sel_order, order, m * sizeof(u32));
    return hc.finish([&] { return ssa_aggregator_remove_indices_device(ctx, ag, d_order, m, n_kept_out); });
}

// ---- the leaf column and the leaf index (the kernels and their arguments: agi_k_insert,
// agi_k_lookup in ssa_aggregator.hpp)
// Only enqueues: one device-to-device copy.  Changes no state of the object.  Every aggregator has the column.
extern "C" int ssa_aggregator_leaves_device(ssa_ctx *ctx, ssa_aggregator *ag, size_t n_take, uint8_t *d_ids32_out) {
    size_t n;
    if (int rc = agx_take(ctx, ag, n_take, &n)) return rc;
    if (n && !d_ids32_out) return SSA_ERR_ARG;
    if (n == 0) return SSA_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipMemcpyAsync(d_ids32_out, ag->leaves.p, 32 * n, hipMemcpyDeviceToDevice, ctx->stream));
    return SSA_OK;
}

extern "C" int ssa_aggregator_leaves(ssa_ctx *ctx, ssa_aggregator *ag, size_t n_take, uint8_t *ids32_out) {
    size_t n;
    if (int rc = agx_take(ctx, ag, n_take, &n)) return rc;
    if (n && !ids32_out) return SSA_ERR_ARG;
    if (n == 0) return SSA_OK;
    HostCall hc(ctx);
    u8 *d_ids = hc.out(ctx->st_aux, ids32_out, 32 * n, 16);
    return hc.finish([&] { return ssa_aggregator_leaves_device(ctx, ag, n, d_ids); });
}

// what both forms of leaves_select refuse before anything is enqueued (a list may name a place twice, so m is bounded by
// the batch limit, not by the lanes held)
static int agx_leaves_select_args(const ssa_ctx *ctx, const ssa_aggregator *ag, const uint32_t *order, size_t m,
                                  const uint8_t *ids32_out, bool device) {
    if (!ctx || !ag || ag->ctx != ctx || m > SSA_MAX_BATCH || (m && (!order || !ids32_out))) return SSA_ERR_ARG;
    return device && (reinterpret_cast<uintptr_t>(order) & 3u) ? SSA_ERR_ARG : 0;
}

// Only enqueues.  The gather goes into a workspace of the context (the caller's buffer may lie at any alignment), one
// copy puts it out, and agx_k_select_verdict -- the verdict of finish_select -- zeroes the output of a list with an index
// out of range and writes *d_result_out.
extern "C" int ssa_aggregator_leaves_select_device(ssa_ctx *ctx, ssa_aggregator *ag, const uint32_t *d_order, size_t m,
                                                   uint8_t *d_ids32_out, uint32_t *d_result_out) {
    if (int rc = agx_leaves_select_args(ctx, ag, d_order, m, d_ids32_out, true)) return rc;
    if (m && (!d_result_out || (reinterpret_cast<uintptr_t>(d_result_out) & 3u))) return SSA_ERR_ARG;
    if (m == 0) return SSA_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    if (ctx->agx_sel_stage.reserve(32 * m) || ctx->agx_sel_bits.reserve(agx_sel_bytes(ag->held))) return SSA_ERR_HIP;
    u32 *d_flag = agx_sel_word(ctx, AGX_SEL_FLAG);
    u64 *d_stage = (u64 *)ctx->agx_sel_stage.p;
    HIP_TRY(hipMemsetAsync(d_flag, 0, sizeof(u32), ctx->stream));
    const int rc = timed_launch(ctx, "agx_k_leaves_select", [&] {
        hipLaunchKernelGGL(agx_k_leaves_select, dim3(grid_for(m, 256)), dim3(256), 0, ctx->stream, d_order, m, ag->held, d_flag,
                           (const u64 *)ag->leaves.p, d_stage);
    });
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(d_ids32_out, d_stage, 32 * m, hipMemcpyDeviceToDevice, ctx->stream));
    return timed_launch(ctx, "agx_k_select_verdict", [&] {
        hipLaunchKernelGGL(agx_k_select_verdict, dim3(std::min(grid_for(32 * m, 256), 4096u)), dim3(256), 0, ctx->stream,
                           (const u32 *)d_flag, d_ids32_out, 32 * m, (u8 *)nullptr, (size_t)0, d_result_out);
    });
}

extern "C" int ssa_aggregator_leaves_select(ssa_ctx *ctx, ssa_aggregator *ag, const uint32_t *order, size_t m,
                                            uint8_t *ids32_out) {
    if (int rc = agx_leaves_select_args(ctx, ag, order, m, ids32_out, false)) return rc;
    if (m == 0) return SSA_OK;
    HostCall hc(ctx);
    const u32 *d_order = hc.in<u32>(ctx->agx_sel_order, order, m * sizeof(u32));
    u8 *d_ids = hc.out(ctx->st_aux, ids32_out, 32 * m, 16);
    // (reserved here at the size the device form asks for: the result word does not move under it)
    if (hc.ok() && ctx->agx_sel_bits.reserve(agx_sel_bytes(ag->held))) hc.rc = SSA_ERR_HIP;
    if (!hc.ok()) return hc.rc;
    u32 refused = 0, *d_result = agx_sel_word(ctx, AGX_SEL_RESULT);
    hc.copy_back(&refused, d_result, sizeof refused);
    if (int rc = hc.finish([&] { return ssa_aggregator_leaves_select_device(ctx, ag, d_order, m, d_ids, d_result); })) return rc;
    return refused ? SSA_ERR_ARG : SSA_OK;
}

// what every call of the index refuses: an object without SSA_AGGR_HOLD_INDEX above all
static int agi_args(const ssa_ctx *ctx, const ssa_aggregator *ag) {
    return !ctx || !ag || ag->ctx != ctx || !ag->hold_index() ? SSA_ERR_ARG : 0;
}

// The index brought up to date with the lanes held (the arguments checked).  Only enqueues: a stale table is cleared --
// the slots to all-ones, the counter behind them to zero: two memsets of one allocation -- and lanes [indexed, held) are
// inserted by one launch.  The host state moves only when everything was enqueued.
static int agi_sync(ssa_ctx *ctx, ssa_aggregator *ag) {
    const size_t slots = ag->index_slots();
    if (int rc = dedup_fingerprint_key(ctx)) return rc;      // (drawn at the first use by anyone: before any slot is picked)
    if (ag->stale) {
        HIP_TRY(hipMemsetAsync(ag->index_table(), 0xFF, 8 * slots, ctx->stream));
        HIP_TRY(hipMemsetAsync(ag->index_over(), 0, 8, ctx->stream));
        ag->stale = false;
        ag->indexed = 0;
        ag->rebuilds++;
    }
    if (ag->indexed < ag->held) {
        const u32 lo = (u32)ag->indexed, hi = (u32)ag->held;
        const int rc = timed_launch(ctx, "agi_k_insert", [&] {
            hipLaunchKernelGGL(agi_k_insert, dim3(grid_for(hi - lo, DD_BLOCK)), dim3(DD_BLOCK), 0, ctx->stream,
                               (const u64 *)ag->leaves.p, lo, hi, ctx->dedup_key[0], ctx->dedup_key[1], ag->index_table(),
                               (u32)(slots - 1), (u32)ctx->knobs.dedup_probe_bound, ag->index_over());
        });
        if (rc) {
            ag->index_void();
            return rc;
        }
        ag->indexed = ag->held;
    }
    return SSA_OK;
}

extern "C" int ssa_aggregator_index_sync(ssa_ctx *ctx, ssa_aggregator *ag) {
    if (int rc = agi_args(ctx, ag)) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    return agi_sync(ctx, ag);
}

static int agi_lookup_args(const ssa_ctx *ctx, const ssa_aggregator *ag, const uint8_t *ids32, size_t n,
                           const uint32_t *places_out, const void *n_unknown_out, bool device) {
    if (int rc = agi_args(ctx, ag)) return rc;
    if (!n_unknown_out || n > SSA_MAX_BATCH || (n && (!ids32 || !places_out))) return SSA_ERR_ARG;
    return device && ((reinterpret_cast<uintptr_t>(places_out) | reinterpret_cast<uintptr_t>(n_unknown_out)) & 3u) ? SSA_ERR_ARG
                                                                                                                    : 0;
}

// Only enqueues on the context's stream: the index is brought up to date (agi_sync), the count word is cleared, and one
// launch answers the n ids.  n == 0 launches nothing and leaves the index as it is.
extern "C" int ssa_aggregator_lookup_device(ssa_ctx *ctx, ssa_aggregator *ag, const uint8_t *d_ids32, size_t n,
                                            uint32_t *d_places_out, uint32_t *d_n_unknown_out) {
    if (int rc = agi_lookup_args(ctx, ag, d_ids32, n, d_places_out, d_n_unknown_out, true)) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipMemsetAsync(d_n_unknown_out, 0, sizeof(uint32_t), ctx->stream));
    if (n == 0) return SSA_OK;
    if (int rc = agi_sync(ctx, ag)) return rc;
    ag->lookups++;
    ag->looked_up += n;
    return timed_launch(ctx, "agi_k_lookup", [&] {
        hipLaunchKernelGGL(agi_k_lookup, dim3(grid_for(n, DD_BLOCK)), dim3(DD_BLOCK), 0, ctx->stream, d_ids32, (u32)n,
                           (const u64 *)ag->leaves.p, (u32)ag->indexed, ctx->dedup_key[0], ctx->dedup_key[1],
                           (const u64 *)ag->index_table(), (u32)(ag->index_slots() - 1), (u32)ctx->knobs.dedup_probe_bound,
                           d_places_out, d_n_unknown_out);
    });
}

// The count word travels behind the places in one workspace and comes back with them under the one synchronisation.
extern "C" int ssa_aggregator_lookup(ssa_ctx *ctx, ssa_aggregator *ag, const uint8_t *ids32, size_t n, uint32_t *places_out,
                                     uint64_t *n_unknown_out) {
    if (int rc = agi_lookup_args(ctx, ag, ids32, n, places_out, n_unknown_out, false)) return rc;
    *n_unknown_out = 0;
    if (n == 0) return SSA_OK;
    HostCall hc(ctx);
    const u8 *d_ids = hc.in(ctx->st_sigs, ids32, 32 * n);
    u8 *d_places = hc.out(ctx->st_aux, places_out, 4 * n, 16);
    if (!hc.ok()) return hc.rc;
    u32 unknown = 0, *d_unknown = (u32 *)(d_places + 4 * n);
    hc.copy_back(&unknown, d_unknown, sizeof unknown);
    if (int rc = hc.finish([&] { return ssa_aggregator_lookup_device(ctx, ag, d_ids, n, (u32 *)d_places, d_unknown); })) return rc;
    *n_unknown_out = unknown;
    return SSA_OK;
}

// Synchronises the context's stream once: word [4] is a counter on the device.
extern "C" int ssa_aggregator_index_info(ssa_ctx *ctx, ssa_aggregator *ag, uint64_t out[8]) {
    if (int rc = agi_args(ctx, ag)) return rc;
    if (!out) return SSA_ERR_ARG;
    HIP_TRY(hipSetDevice(ctx->device));
    unsigned long long over = 0;
    if (!ag->stale) {        // (a stale table's counter is cleared with it, before anything counts again)
        HIP_TRY(hipMemcpyAsync(&over, ag->index_over(), sizeof over, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
    }
    out[0] = ag->index_slots();
    out[1] = ag->indexed;
    out[2] = ag->stale ? 1 : 0;
    out[3] = ag->rebuilds;
    out[4] = over;
    out[5] = ag->lookups;
    out[6] = ag->looked_up;
    out[7] = 0;
    return SSA_OK;
}

// ------------------------------------------------------------------ streaming aggregate verifier (ssa_aggverifier.hpp)
extern "C" int ssa_aggverifier_create(ssa_ctx *ctx, size_t capacity, size_t block_lanes, uint32_t flags, ssa_aggverifier **out) {
    const int rc = agx_create(ctx, capacity, block_lanes, flags, out);
    if (rc == 0) ctx->aggverifiers.push_back(*out);
    return rc;
}

extern "C" void ssa_aggverifier_destroy(ssa_aggverifier *av) { agx_destroy(av, &ssa_ctx::aggverifiers); }

// Nothing on the device needs clearing: every array is written before it is read, up to `held` (kst: the rule of
// ssa_aggverifier.hpp -- with `keyed` off its bytes are not read until the next cached push has zeroed or written them).
extern "C" int ssa_aggverifier_reset(ssa_aggverifier *av) {
    if (!av || !av->ctx) return SSA_ERR_ARG;
    av->held = 0;
    av->pushes = av->pushed = av->finishes = av->cached = 0;
    av->keyed = av->mixed = false;
    av->mixed_pushes.clear();
    return 0;
}

extern "C" int ssa_aggverifier_info(ssa_aggverifier *av, uint64_t out[8]) {
    if (!av || !av->ctx || !out) return SSA_ERR_ARG;
    out[0] = av->held;
    out[1] = av->capacity;
    out[2] = av->block;
    out[3] = av->pushes;
    out[4] = av->pushed;
    out[5] = av->cached;              // lanes pushed through a key cache (the lanes marked bad are known on the device alone)
    out[6] = av->held / av->block;
    out[7] = av->finishes;
    return 0;
}

// what both forms of push refuse before anything is enqueued or counted
static int agv_push_args(const ssa_ctx *ctx, const ssa_aggverifier *av, const MsgView &mv, size_t n, const void *rs49,
                         const void *pks) {
    if (!ctx || !av || av->ctx != ctx || (n && (!rs49 || !pks))) return SSA_ERR_ARG;
    if (int rc = agg_check_args(ctx, mv, n)) return rc;
    return n > av->capacity - av->held ? SSA_ERR_ARG : 0;
}

// The body of every push behind its argument checks, n lanes over the keys U = d_pks / d_pk_inf as agv_k_append
// reads them (the caller's, or what a wire cache expanded).  through_cache: the lanes' kst bytes are already written
// (agc_k_expand, enqueued in front); otherwise a keyed object gets them zeroed here.  Only enqueues; no lanes: the push
// is counted and nothing is enqueued.
static int agv_push_body(ssa_ctx *ctx, ssa_aggverifier *av, const u8 *d_rs49, const u8 *d_pks, const u8 *d_pk_inf,
                         const MsgView &mv, size_t n, bool through_cache) {
    if (n == 0) {
        av->pushes++;
        return SSA_OK;
    }
    // ONE challenge hash over the n lanes: the raw digests for the leaves (ctx->ag_dig) and the scalars mod q (ctx->ws_h)
    const u8 *d_sigs = nullptr;
    if (int rc = ag_transcript_front(ctx, d_rs49, &d_sigs, d_pks, mv, n, true, nullptr, 1)) return rc;
    int rc = timed_launch(ctx, "agv_k_append", [&] {
        hipLaunchKernelGGL(agv_k_append, dim3(grid_for(n, 256)), dim3(256), 0, ctx->stream, ctx->d_params, d_sigs, d_pks,
                           d_pk_inf, (const u64 *)ctx->ag_dig.p, (const u64 *)ctx->ws_h.p, n, av->held, (u64 *)av->leaves.p,
                           (u64 *)av->h.p, (u64 *)av->rpts.p, (u64 *)av->ppts.p, (u8 *)av->bad.p);
    });
    if (rc) return rc;
    const AgxPlan p = agx_plan(av->held, n, av->block);
    if (p.count)
        if ((rc = agx_reduce_blocks(*av, p))) return rc;
    // a plain push into a keyed object: its lanes' keys are "not checked"
    if (av->keyed && !through_cache) HIP_TRY(hipMemsetAsync((u8 *)av->kst.p + av->held, 0, n, ctx->stream));
    // a push that took no lane from a pool into an object that holds such lanes: none of its lanes is known
    if (av->mixed) HIP_TRY(hipMemsetAsync((u8 *)av->known.p + av->held, 0, n, ctx->stream));
    // (only now: a launch that could not be enqueued leaves the object as it was -- what it wrote lies behind `held`)
    av->held += n;
    av->pushes++;
    av->pushed += n;
    if (through_cache) av->cached += n;
    return SSA_OK;
}

// Only enqueues: every lane is appended, so the count is the caller's n and nothing is read back.
extern "C" int ssa_aggverifier_push_device(ssa_ctx *ctx, ssa_aggverifier *av, const uint8_t *d_rs49, const uint8_t *d_pks,
                                           const uint8_t *d_pk_inf, const uint8_t *d_msgs, const uint64_t *d_msg_off,
                                           size_t msg_stride, size_t msg_len, size_t n) {
    const MsgView mv{d_msgs, d_msg_off, msg_stride, msg_len};
    if (int rc = agv_push_args(ctx, av, mv, n, d_rs49, d_pks)) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    return agv_push_body(ctx, av, d_rs49, d_pks, d_pk_inf, mv, n, false);
}

extern "C" int ssa_aggverifier_push(ssa_ctx *ctx, ssa_aggverifier *av, const uint8_t *rs49, const uint8_t *pks,
                                    const uint8_t *pk_inf, const uint8_t *msgs, const uint64_t *msg_off, size_t msg_stride,
                                    size_t msg_len, size_t n) {
    if (int rc = agv_push_args(ctx, av, {msgs, msg_off, msg_stride, msg_len}, n, rs49, pks)) return rc;
    if (int rc = check_host_offsets(msg_off, n)) return rc;
    if (n == 0) return ssa_aggverifier_push_device(ctx, av, nullptr, nullptr, nullptr, nullptr, nullptr, msg_stride, msg_len, 0);
    HostCall hc(ctx);
    const DevBatch b = hc.lanes({rs49, pks, pk_inf, msgs, msg_off, msg_stride, msg_len}, n * 49, n);
    const int rc = hc.finish([&] {
        return ssa_aggverifier_push_device(ctx, av, b.sigs, b.pks, b.pk_inf, b.msgs.msgs, b.msgs.off, msg_stride, msg_len, n);
    });
    if (rc) return rc;
    // nothing is copied back, so finish() did not wait: the staging buffers are free for the next call only once the
    // kernels that read them are done
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return SSA_OK;
}

// The record of the MSM over the first n (>= 1) held lanes, at d_rec_out: the root of those lanes (agx_root), then per
// piece of at most one MSM slice agv_k_scalars fills the bucket pipeline's inputs from the object (e = 0 on every lane: the
// partial sums are zeroed), ssa_internal_msm_record_prepared runs the rest, and the pieces' records are added up as
// ags_record adds them.
static int agv_record(ssa_ctx *ctx, const ssa_aggverifier *av, size_t n, u64 *d_rec_out) {
    const size_t piece = ags_piece(ctx), k = (n + piece - 1) / piece;
    if (k > 4096) return SSA_ERR_ARG;
    if (ctx->ags_recs.reserve(k * 24 * sizeof(u64))) return SSA_ERR_HIP;
    if (int rc = agx_root(*av, n)) return rc;
    const u64 *d_root = (const u64 *)ctx->agm_roots.p;      // (only now: agx_root reserves it)
    for (size_t lo = 0, j = 0; j < k; lo += piece, j++) {
        const size_t cnt = std::min(piece, n - lo);
        const int rc = ssa_internal_msm_record_prepared(ctx, cnt, 16, [&](const MsmFill &f) {
            return timed_launch(ctx, "agv_k_scalars", [&] {
                (void)hipMemsetAsync(f.partials, 0, (size_t)f.n_blocks * 32, ctx->stream);
                hipLaunchKernelGGL(agv_k_scalars, dim3(f.n_blocks), dim3(256), 0, ctx->stream, ctx->d_params, d_root,
                                   (const u64 *)av->h.p + 4 * lo, (const u64 *)av->rpts.p + 12 * lo,
                                   (const u64 *)av->ppts.p + 12 * lo, (const u8 *)av->bad.p + lo, cnt, (u64)lo, f.sh, f.wa,
                                   f.points, f.digits, f.flags);
            });
        }, k == 1 ? (uint64_t *)d_rec_out : (uint64_t *)ctx->ags_recs.p + 24 * j);
        if (rc) return rc;
    }
    return k == 1 ? 0 : ssa_internal_msm_sum_records(ctx, (const uint64_t *)ctx->ags_recs.p, k, false, (uint64_t *)d_rec_out);
}

// ---- a prefix that holds known lanes (the kernels: ssa_aggverifier.hpp)
// ctx->agv_misc: the flag word of a push, the result word of the host forms, the flag word of a finish, S, e_agg - S
constexpr size_t AGV_PUSH_FLAG = 0, AGV_RESULT = 4, AGV_FIN_FLAG = 8, AGV_S = 32, AGV_D = 64, AGV_MISC_BYTES = 96;
static u8 *agv_misc(ssa_ctx *ctx, size_t off) { return (u8 *)ctx->agv_misc.p + off; }

// The ascending list of the unknown places of the first n (>= 1) held lanes into ctx->agv_pos, its length at *d_m_out
// (on the device): the compaction of av_keep over the known bytes -- a lane is listed iff its byte is zero.
static int agv_list_unknown(ssa_ctx *ctx, const ssa_aggverifier *av, size_t n, const u32 **d_m_out) {
    if (ctx->agv_pos.reserve(n * sizeof(u32))) return SSA_ERR_HIP;
    return av_keep_enqueue(ctx, (const u8 *)av->known.p, n, (u32 *)ctx->agv_pos.p, d_m_out);
}

// S of the first n (>= 1) held lanes under the root in ctx->agm_roots, 32 bytes at d_s32_out: agx_fold with
// agv_k_known_fold in place of agx_k_coeff_fold.  The finish's flag word is cleared in front and raised by a known lane
// marked bad or a list of more than u_cap unknown places (*d_m: agv_list_unknown's count).
static int agv_known_sum(ssa_ctx *ctx, const ssa_aggverifier *av, size_t n, const u32 *d_m, size_t u_cap, u8 *d_s32_out) {
    const size_t piece = ags_piece(ctx), k = (n + piece - 1) / piece;
    if (ctx->ags_parts.reserve(k * 32) || ctx->ag_partials.reserve((size_t)grid_for(std::min(piece, n), 256) * 32))
        return SSA_ERR_HIP;
    const u64 *d_root = (const u64 *)ctx->agm_roots.p;
    u32 *d_flag = (u32 *)agv_misc(ctx, AGV_FIN_FLAG);
    HIP_TRY(hipMemsetAsync(d_flag, 0, sizeof(u32), ctx->stream));
    for (size_t lo = 0, j = 0; lo < n; lo += piece, j++) {
        const size_t cnt = std::min(piece, n - lo);
        const unsigned n_blocks = grid_for(cnt, 256);
        int rc = timed_launch(ctx, "agv_k_known_fold", [&] {
            hipLaunchKernelGGL(agv_k_known_fold, dim3(n_blocks), dim3(256), 0, ctx->stream, ctx->d_params, d_root,
                               (const u64 *)av->h.p + 4 * lo, (const u8 *)av->known.p + lo, (const u8 *)av->bad.p + lo, cnt,
                               (u64)lo, d_m, (u32)u_cap, (u64 *)ctx->ag_partials.p, d_flag);
        });
        if (rc) return rc;
        rc = timed_launch(ctx, "ag_k_fold_finish", [&] {
            hipLaunchKernelGGL(ag_k_fold_finish, dim3(1), dim3(256), 0, ctx->stream, (const u64 *)ctx->ag_partials.p, n_blocks,
                               k == 1 ? d_s32_out : (u8 *)ctx->ags_parts.p + 32 * j);
        });
        if (rc) return rc;
    }
    if (k > 1) {
        const int rc = timed_launch(ctx, "ag_k_fold_finish", [&] {
            hipLaunchKernelGGL(ag_k_fold_finish, dim3(1), dim3(256), 0, ctx->stream, (const u64 *)ctx->ags_parts.p, (u32)k,
                               d_s32_out);
        });
        if (rc) return rc;
    }
    return SSA_OK;
}

// The record of the MSM over the unknown lanes of the first n held lanes, at d_rec_out, under the root in
// ctx->agm_roots: agv_record with agv_k_scalars_at over the u_cap (>= 1) rows of the list of unknown places
// (agv_list_unknown: ctx->agv_pos, its length at *d_m), in pieces of at most one MSM slice.
static int agv_record_listed(ssa_ctx *ctx, const ssa_aggverifier *av, const u32 *d_m, size_t u_cap, u64 *d_rec_out) {
    const size_t piece = ags_piece(ctx), k = (u_cap + piece - 1) / piece;
    if (k > 4096) return SSA_ERR_ARG;
    if (ctx->ags_recs.reserve(k * 24 * sizeof(u64))) return SSA_ERR_HIP;
    const u64 *d_root = (const u64 *)ctx->agm_roots.p;
    const u32 *d_list = (const u32 *)ctx->agv_pos.p;
    for (size_t lo = 0, j = 0; j < k; lo += piece, j++) {
        const size_t cnt = std::min(piece, u_cap - lo);
        const int rc = ssa_internal_msm_record_prepared(ctx, cnt, 16, [&](const MsmFill &f) {
            return timed_launch(ctx, "agv_k_scalars_at", [&] {
                (void)hipMemsetAsync(f.partials, 0, (size_t)f.n_blocks * 32, ctx->stream);
                hipLaunchKernelGGL(agv_k_scalars_at, dim3(f.n_blocks), dim3(256), 0, ctx->stream, ctx->d_params, d_root,
                                   (const u64 *)av->h.p, (const u64 *)av->rpts.p, (const u64 *)av->ppts.p,
                                   (const u8 *)av->bad.p, d_list, d_m, lo, cnt, f.sh, f.wa, f.points, f.digits, f.flags);
            });
        }, k == 1 ? (uint64_t *)d_rec_out : (uint64_t *)ctx->ags_recs.p + 24 * j);
        if (rc) return rc;
    }
    return k == 1 ? 0 : ssa_internal_msm_sum_records(ctx, (const uint64_t *)ctx->ags_recs.p, k, false, (uint64_t *)d_rec_out);
}

// finish for a prefix of n (>= 1) lanes that holds known lanes: the root; the unknown lanes' record (none: no MSM);
// S over the known lanes; then [e_agg - S]G against the record by ag_k_finish_scalar -- agv_k_known_close forms the
// difference, leaves a non-canonical e_agg as it is and carries the flag into the record's malformed word -- or, without
// a record, the verdict of agv_k_known_close itself.  Only enqueues.
static int agv_finish_mixed(ssa_ctx *ctx, const ssa_aggverifier *av, const u8 *d_e_agg, size_t n, u32 *d_verdict_out) {
    const size_t u_cap = av->unknown_cap(n);
    if (ctx->agv_misc.reserve(AGV_MISC_BYTES)) return SSA_ERR_HIP;
    if (int rc = agx_root(*av, n)) return rc;
    u64 *d_rec = u_cap ? (u64 *)ag_misc(ctx, AG_REC) : nullptr;
    const u32 *d_m = nullptr;
    if (int rc = agv_list_unknown(ctx, av, n, &d_m)) return rc;
    if (u_cap)
        if (int rc = agv_record_listed(ctx, av, d_m, u_cap, d_rec)) return rc;
    if (int rc = agv_known_sum(ctx, av, n, d_m, u_cap, agv_misc(ctx, AGV_S))) return rc;
    int rc = timed_launch(ctx, "agv_k_known_close", [&] {
        hipLaunchKernelGGL(agv_k_known_close, dim3(1), dim3(64), 0, ctx->stream, d_e_agg, (const u8 *)agv_misc(ctx, AGV_S),
                           (const u32 *)agv_misc(ctx, AGV_FIN_FLAG), d_rec, agv_misc(ctx, AGV_D), d_verdict_out);
    });
    if (rc || !u_cap) return rc;
    return timed_launch(ctx, "ag_k_finish", [&] {
        hipLaunchKernelGGL(ag_k_finish_scalar, dim3(1), dim3(64), 0, ctx->stream, (const u64 *)d_rec,
                           (const u8 *)agv_misc(ctx, AGV_D), 0u, (const u64 *)ctx->d_gtab, d_verdict_out);
    });
}

// Only enqueues on the context's stream: every size it needs is on the host.  Reads the object, writes workspaces of the
// context and the caller's verdict word.
extern "C" int ssa_aggverifier_finish_device(ssa_ctx *ctx, ssa_aggverifier *av, const uint8_t *d_e_agg, size_t n_take,
                                             uint32_t *d_verdict_out) {
    size_t n;
    if (int rc = agx_take(ctx, av, n_take, &n)) return rc;
    if (!d_e_agg || !d_verdict_out) return SSA_ERR_ARG;
    HIP_TRY(hipSetDevice(ctx->device));
    if (ctx->ag_misc.reserve(AG_MISC_BYTES)) return SSA_ERR_HIP;
    av->finishes++;
    const bool mixed = av->prefix_mixed(n);      // (then n >= 1) known lanes in the prefix: DESIGN.md section 34
    if (n && !mixed)
        if (int rc = agv_record(ctx, av, n, (u64 *)ag_misc(ctx, AG_REC))) return rc;
    // the exact comparison of ssa_verify_aggregate_combine_device; the empty aggregate has no record: the kernel reads none
    const int rc = mixed ? agv_finish_mixed(ctx, av, d_e_agg, n, d_verdict_out) : timed_launch(ctx, "ag_k_finish", [&] {
        hipLaunchKernelGGL(ag_k_finish_scalar, dim3(1), dim3(64), 0, ctx->stream, (const u64 *)ag_misc(ctx, AG_REC), d_e_agg,
                           n == 0 ? 1u : 0u, (const u64 *)ctx->d_gtab, d_verdict_out);
    });
    if (rc || !av->keyed || n == 0) return rc;       // (no lane, no key: the rule of the empty aggregate stands)
    // the key decides: the fold of the key statuses of the prefix, behind the comparison
    return timed_launch(ctx, "agv_k_key_verdict", [&] {
        hipLaunchKernelGGL(agv_k_key_verdict, dim3(grid_for(n, AGV_KST_SPAN)), dim3(256), 0, ctx->stream,
                           (const u8 *)av->kst.p, n, d_verdict_out);
    });
}

extern "C" size_t ssa_debug_aggverifier_key_span(void) { return AGV_KST_SPAN; }

extern "C" int ssa_aggverifier_finish(ssa_ctx *ctx, ssa_aggverifier *av, const uint8_t *e_agg32, size_t n_take) {
    size_t n;
    if (int rc = agx_take(ctx, av, n_take, &n)) return rc;
    if (!e_agg32) return SSA_ERR_ARG;
    HostCall hc(ctx);
    const u8 *d_e = hc.in(ctx->st_aux, e_agg32, 32);
    uint32_t v = SSA_MALFORMED, *d_verdict = (uint32_t *)((char *)ctx->ws_fail.p + 32);
    hc.copy_back(&v, d_verdict, sizeof v);
    const int rc = hc.finish([&] { return ssa_aggverifier_finish_device(ctx, av, d_e, n, d_verdict); });
    return rc ? rc : (int)v;
}

// tests: the summed record of finish without the comparison (no lanes, no record: SSA_ERR_ARG).  Only enqueues.
extern "C" int ssa_debug_aggverifier_record(ssa_ctx *ctx, ssa_aggverifier *av, size_t n_take, uint64_t *d_record24_out) {
    size_t n;
    if (int rc = agx_take(ctx, av, n_take, &n)) return rc;
    if (n == 0 || !d_record24_out || !aligned8(d_record24_out)) return SSA_ERR_ARG;
    HIP_TRY(hipSetDevice(ctx->device));
    if (!av->prefix_mixed(n)) return agv_record(ctx, av, n, (u64 *)d_record24_out);
    // known lanes in the prefix: the record of its unknown lanes alone (none of those either, no record)
    const size_t u_cap = av->unknown_cap(n);
    if (u_cap == 0) return SSA_ERR_ARG;
    if (int rc = agx_root(*av, n)) return rc;
    const u32 *d_m = nullptr;
    if (int rc = agv_list_unknown(ctx, av, n, &d_m)) return rc;
    return agv_record_listed(ctx, av, d_m, u_cap, (u64 *)d_record24_out);
}

// tests: S of the first n_take held lanes (32 bytes, little-endian, canonical; zero without a known lane).  Only enqueues.
extern "C" int ssa_debug_aggverifier_known_sum(ssa_ctx *ctx, ssa_aggverifier *av, size_t n_take, uint8_t *d_s32_out) {
    size_t n;
    if (int rc = agx_take(ctx, av, n_take, &n)) return rc;
    if (!d_s32_out) return SSA_ERR_ARG;
    HIP_TRY(hipSetDevice(ctx->device));
    if (!av->prefix_mixed(n)) {
        HIP_TRY(hipMemsetAsync(d_s32_out, 0, 32, ctx->stream));
        return SSA_OK;
    }
    if (ctx->agv_misc.reserve(AGV_MISC_BYTES)) return SSA_ERR_HIP;
    if (int rc = agx_root(*av, n)) return rc;
    const u32 *d_m = nullptr;
    if (int rc = agv_list_unknown(ctx, av, n, &d_m)) return rc;
    return agv_known_sum(ctx, av, n, d_m, av->unknown_cap(n), d_s32_out);
}

// ---- a block against the pool: known lanes from a streaming aggregator, the rest with the call
// what every form of a mixed push refuses before anything is enqueued or counted.  n lanes, u of them unknown, the
// places at `places` (device: in device memory).  The u compact lanes are checked as a plain push of u lanes is.
static int agv_mixed_args(const ssa_ctx *ctx, const ssa_aggverifier *av, const ssa_aggregator *ag, const uint32_t *places,
                          size_t n, size_t u, const MsgView &mv, const void *rs49, const void *pks, bool device) {
    if (!ctx || !av || !ag || av->ctx != ctx || ag->ctx != ctx || (n && !places) || u > n || (u && (!rs49 || !pks)))
        return SSA_ERR_ARG;
    if (device && (reinterpret_cast<uintptr_t>(places) & 3u)) return SSA_ERR_ARG;
    if (int rc = agg_check_args(ctx, mv, u)) return rc;
    return n > ctx->knobs.msm_slice || n > av->capacity - av->held ? SSA_ERR_ARG : 0;
}

// What a mixed push through a key cache adds to the body (all zero: the push of section 34, which
// then enqueues exactly what it did): require > 0 -- the pool's admission column is read and a known lane below the
// class is refused (agv_k_classify_adm in place of agv_k_classify); d_kst -- the dense key statuses of the u compact
// lanes, scattered to their places behind agv_k_append_at (agv_k_kst_at); the object is keyed by then.
struct AgvMixedCached {
    u32 require = 0;
    const u8 *d_kst = nullptr;
};

// The body of both forms behind the argument checks.  Only enqueues: whether the list is valid is decided on the device
// (agv_k_classify, agv_k_mixed_close) and lands in *d_result_out.
static int agv_push_mixed_body(ssa_ctx *ctx, ssa_aggverifier *av, const ssa_aggregator *ag, const u32 *d_places, size_t n,
                               size_t u, const u8 *d_rs49, const u8 *d_pks, const u8 *d_pk_inf, const MsgView &mv,
                               u32 *d_result_out, const AgvMixedCached &mc = {}) {
    if (n == 0) {
        HIP_TRY(hipMemsetAsync(d_result_out, 0, sizeof(u32), ctx->stream));
        av->pushes++;
        return SSA_OK;
    }
    if (ctx->agv_keep.reserve(n + 16) || ctx->agv_pos.reserve(n * sizeof(u32)) || ctx->agv_misc.reserve(AGV_MISC_BYTES))
        return SSA_ERR_HIP;
    const size_t held = av->held;
    // the first mixed push of the object: none of the lanes held so far is known (the rule in ssa_aggverifier.hpp)
    if (!av->mixed && held) HIP_TRY(hipMemsetAsync(av->known.p, 0, held, ctx->stream));
    u32 *d_flag = (u32 *)agv_misc(ctx, AGV_PUSH_FLAG);
    HIP_TRY(hipMemsetAsync(d_flag, 0, sizeof(u32), ctx->stream));
    u8 *d_keep = (u8 *)ctx->agv_keep.p;
    u32 *d_pos = (u32 *)ctx->agv_pos.p;
    int rc = mc.require ? timed_launch(ctx, "agv_k_classify_adm", [&] {
        hipLaunchKernelGGL(agv_k_classify_adm, dim3(grid_for(n, 256)), dim3(256), 0, ctx->stream, d_places, n, held, ag->held,
                           (const u64 *)ag->leaves.p, (const u64 *)ag->scal.p, (const u8 *)ag->adm.p, mc.require,
                           (u64 *)av->leaves.p, (u64 *)av->h.p, (u64 *)av->rpts.p, (u64 *)av->ppts.p, (u8 *)av->bad.p,
                           av->keyed ? (u8 *)av->kst.p : (u8 *)nullptr, (u8 *)av->known.p, d_keep, d_flag);
    }) : timed_launch(ctx, "agv_k_classify", [&] {
        hipLaunchKernelGGL(agv_k_classify, dim3(grid_for(n, 256)), dim3(256), 0, ctx->stream, d_places, n, held, ag->held,
                           (const u64 *)ag->leaves.p, (const u64 *)ag->scal.p, (u64 *)av->leaves.p, (u64 *)av->h.p,
                           (u64 *)av->rpts.p, (u64 *)av->ppts.p, (u8 *)av->bad.p, av->keyed ? (u8 *)av->kst.p : (u8 *)nullptr,
                           (u8 *)av->known.p, d_keep, d_flag);
    });
    if (rc) return rc;
    // the unknown positions, ascending, and their number -- which stays on the device
    const u32 *d_m = nullptr;
    if ((rc = av_keep_enqueue(ctx, d_keep, n, d_pos, &d_m))) return rc;
    if (u) {
        // ONE challenge hash over the u lanes the call brought, as the plain push's over its n
        const u8 *d_sigs = nullptr;
        if ((rc = ag_transcript_front(ctx, d_rs49, &d_sigs, d_pks, mv, u, true, nullptr, 1))) return rc;
        rc = timed_launch(ctx, "agv_k_append_at", [&] {
            hipLaunchKernelGGL(agv_k_append_at, dim3(grid_for(u, 256)), dim3(256), 0, ctx->stream, ctx->d_params, d_sigs, d_pks,
                               d_pk_inf, (const u64 *)ctx->ag_dig.p, (const u64 *)ctx->ws_h.p, u, (const u32 *)d_pos, d_m, held,
                               (u64 *)av->leaves.p, (u64 *)av->h.p, (u64 *)av->rpts.p, (u64 *)av->ppts.p, (u8 *)av->bad.p);
        });
        if (rc) return rc;
        // the unknown lanes' key statuses to their true places: behind the classification, which wrote zeros there
        if (mc.d_kst) {
            rc = timed_launch(ctx, "agv_k_kst_at", [&] {
                hipLaunchKernelGGL(agv_k_kst_at, dim3(grid_for(u, 256)), dim3(256), 0, ctx->stream, mc.d_kst, u,
                                   (const u32 *)d_pos, d_m, (u8 *)av->kst.p + held);
            });
            if (rc) return rc;
        }
    }
    rc = timed_launch(ctx, "agv_k_mixed_close", [&] {
        hipLaunchKernelGGL(agv_k_mixed_close, dim3(std::min(grid_for(n, 256), 1024u)), dim3(256), 0, ctx->stream, d_m, (u32)u,
                           (const u32 *)d_flag, n, (u8 *)av->bad.p + held, d_result_out);
    });
    if (rc) return rc;
    const AgxPlan p = agx_plan(held, n, av->block);
    if (p.count)
        if ((rc = agx_reduce_blocks(*av, p))) return rc;
    // (only now: a launch that could not be enqueued leaves the object as it was -- what it wrote lies behind `held`)
    av->mixed = true;
    if (n > u) av->mixed_pushes.push_back({held, n, u});
    av->held += n;
    av->pushes++;
    av->pushed += n;
    if (mc.d_kst) av->cached += u;
    return SSA_OK;
}

extern "C" int ssa_aggverifier_push_mixed_device(ssa_ctx *ctx, ssa_aggverifier *av, ssa_aggregator *ag,
                                                 const uint32_t *d_places, size_t n, const uint8_t *d_rs49,
                                                 const uint8_t *d_pks, const uint8_t *d_pk_inf, const uint8_t *d_msgs,
                                                 const uint64_t *d_msg_off, size_t msg_stride, size_t msg_len, size_t u,
                                                 uint32_t *d_result_out) {
    const MsgView mv{d_msgs, d_msg_off, msg_stride, msg_len};
    if (int rc = agv_mixed_args(ctx, av, ag, d_places, n, u, mv, d_rs49, d_pks, true)) return rc;
    if (!d_result_out) return SSA_ERR_ARG;
    HIP_TRY(hipSetDevice(ctx->device));
    return agv_push_mixed_body(ctx, av, ag, d_places, n, u, d_rs49, d_pks, d_pk_inf, mv, d_result_out);
}

// The list is on the host: everything a device would refuse is refused here, before a launch.
extern "C" int ssa_aggverifier_push_mixed(ssa_ctx *ctx, ssa_aggverifier *av, ssa_aggregator *ag, const uint32_t *places,
                                          size_t n, const uint8_t *rs49, const uint8_t *pks, const uint8_t *pk_inf,
                                          const uint8_t *msgs, const uint64_t *msg_off, size_t msg_stride, size_t msg_len,
                                          size_t u) {
    if (int rc = agv_mixed_args(ctx, av, ag, places, n, u, {msgs, msg_off, msg_stride, msg_len}, rs49, pks, false)) return rc;
    if (int rc = check_host_offsets(msg_off, u)) return rc;
    size_t sentinels = 0;
    for (size_t i = 0; i < n; i++) {
        if (places[i] == SSA_AGGV_UNKNOWN) sentinels++;
        else if (places[i] >= ag->held) return SSA_ERR_ARG;
    }
    if (sentinels != u) return SSA_ERR_ARG;
    HostCall hc(ctx);
    const u32 *d_places = hc.in<u32>(ctx->agv_places, places, n * sizeof(u32));
    DevBatch b{};
    if (u) b = hc.lanes({rs49, pks, pk_inf, msgs, msg_off, msg_stride, msg_len}, u * 49, u);
    // (reserved here at the size the body asks for: the result word does not move under it)
    if (hc.ok() && ctx->agv_misc.reserve(AGV_MISC_BYTES)) hc.rc = SSA_ERR_HIP;
    if (!hc.ok()) return hc.rc;
    u32 refused = 0, *d_result = (u32 *)agv_misc(ctx, AGV_RESULT);
    hc.copy_back(&refused, d_result, sizeof refused);
    const int rc = hc.finish([&] {
        return agv_push_mixed_body(ctx, av, ag, d_places, n, u, b.sigs, b.pks, b.pk_inf, {b.msgs.msgs, b.msgs.off, msg_stride, msg_len},
                                   d_result);
    });
    if (rc) return rc;
    return refused ? SSA_ERR_HIP : SSA_OK;      // (cannot be: the list was checked above)
}

extern "C" int ssa_aggverifier_push_known_device(ssa_ctx *ctx, ssa_aggverifier *av, ssa_aggregator *ag,
                                                 const uint32_t *d_places, size_t m, uint32_t *d_result_out) {
    return ssa_aggverifier_push_mixed_device(ctx, av, ag, d_places, m, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0, 0,
                                             d_result_out);
}

extern "C" int ssa_aggverifier_push_known(ssa_ctx *ctx, ssa_aggverifier *av, ssa_aggregator *ag, const uint32_t *places,
                                          size_t m) {
    return ssa_aggverifier_push_mixed(ctx, av, ag, places, m, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0, 0);
}

// ---- several devices in one process: every device takes a contiguous run of whole blocks, block counts differ by at
// most one.  One host thread per device and walk; two joins: the tops come in (32 bytes per block), the root goes out.
// The root, the sum of the partial scalars and the combination run on device 0.
struct AgsShard {
    size_t lo = 0, cnt = 0;            // lanes [lo, lo + cnt) of the call
    DevBatch dev{};                    // the shard's inputs on its device, staged by the first walk
    std::vector<uint64_t> off;         // its rebased offset table
    int rc = 0;
};
static std::vector<AgsShard> ags_split(size_t n, size_t B, size_t world) {
    std::vector<AgsShard> sh(world);
    const size_t blocks = (n + B - 1) / B, base = blocks / world, rem = blocks % world;
    for (size_t r = 0; r < world; r++) {
        const size_t b0 = r * base + std::min(r, rem), nb = base + (r < rem ? 1 : 0);
        sh[r].lo = std::min(b0 * B, n);
        sh[r].cnt = std::min((b0 + nb) * B, n) - sh[r].lo;
    }
    return sh;
}
// fn(r) for every shard that has lanes, each on a thread of its own; the first error
template <class F>
static int ags_each_device(std::vector<AgsShard> &sh, F &&fn) {
    std::vector<std::thread> threads;
    for (size_t r = 0; r < sh.size(); r++)
        if (sh[r].cnt) threads.emplace_back([&, r] { sh[r].rc = fn(r); });
    for (auto &t : threads) t.join();
    for (const AgsShard &s : sh)
        if (s.rc) return s.rc;
    return 0;
}
// the first walk of both calls: shard r's lanes (lanes: signatures or R's of the whole call at `stride`), keys, flags
// and messages staged on its device, its tops into tops (host, 4 words per block of the call)
static int ags_multi_tops(ssa_multi *m, std::vector<AgsShard> &sh, const HostBatch &b, const uint8_t *lanes, u32 stride,
                          size_t B, bool with_h, std::vector<uint64_t> &tops) {
    return ags_each_device(sh, [&](size_t r) {
        ssa_ctx *c = m->ctxs[r];
        AgsShard &s = sh[r];
        const HostBatch hb = b.slice(s.lo, s.cnt, s.off);
        HostCall hc(c);
        s.dev.sigs = hc.in(c->st_sigs, lanes + (size_t)stride * s.lo, s.cnt * stride);
        s.dev.pks = hc.in(c->st_pks, hb.pks, s.cnt * 96);
        s.dev.pk_inf = hb.pk_inf ? hc.in(c->st_inf, hb.pk_inf, s.cnt) : nullptr;
        s.dev.msgs = hc.msgs(hb.msgs, hb.msg_off, hb.msg_stride, hb.msg_len, s.cnt);
        const size_t n_tops = (s.cnt + B - 1) / B;
        u64 *d_tops = (u64 *)hc.out(c->ags_tops, tops.data() + 4 * (s.lo / B), n_tops * 32);
        if (with_h && hc.ok() && c->ws_h.reserve(s.cnt * 32)) hc.rc = SSA_ERR_HIP;
        return hc.finish([&] {
            return ags_tops(c, s.dev.sigs, stride, s.dev.pks, s.dev.msgs, s.cnt, B, d_tops, with_h ? (u64 *)c->ws_h.p : nullptr);
        });
    });
}
// the first join: all tops to device 0, the root back to the host
static int ags_multi_root(ssa_ctx *c0, const std::vector<uint64_t> &tops, size_t n, uint64_t root[4]) {
    HostCall hc(c0);
    const u64 *d_tops = hc.in<u64>(c0->ags_tops, tops.data(), tops.size() * sizeof(uint64_t));
    u64 *d_root = (u64 *)hc.out(c0->agm_roots, root, 32);
    return hc.finish([&] { return ags_root(c0, d_tops, tops.size() / 4, n, d_root); });
}

extern "C" int ssa_multi_aggregate_many(ssa_multi *m, const uint8_t *sigs, const uint8_t *pks, const uint8_t *pk_inf,
                                        const uint8_t *msgs, const uint64_t *msg_off, size_t msg_stride, size_t msg_len,
                                        size_t n, uint32_t flags, uint8_t *agg_out, uint8_t *status_out,
                                        uint64_t *n_fail_out) {
    if (!m || m->ctxs.empty() || !agg_out || (flags & ~SSA_AGG_CHECK) || (n && (!sigs || !pks))) return SSA_ERR_ARG;
    if (int rc = check_msgs({msgs, msg_off, msg_stride, msg_len}, n)) return rc;
    if (int rc = check_host_offsets(msg_off, n)) return rc;
    if (n_fail_out) *n_fail_out = 0;
    if (n == 0) {
        std::memset(agg_out, 0, 32);
        return SSA_OK;
    }
    ssa_ctx *c0 = m->ctxs[0];
    const size_t world = m->ctxs.size(), B = ags_block(c0);
    const HostBatch b{sigs, pks, pk_inf, msgs, msg_off, msg_stride, msg_len};
    const bool screened = (flags & SSA_AGG_CHECK) != 0;
    std::vector<AgsShard> sh = ags_split(n, B, world);
    std::vector<uint8_t> own_status(status_out ? 0 : n);
    uint8_t *status = status_out ? status_out : own_status.data();
    std::vector<uint64_t> fails(world, 0), tops(4 * ((n + B - 1) / B), 0), parts(4 * world, 0);
    if (screened)      // the statuses of ssa_verify_batch_screened, every device its own lanes (before anything is staged)
        if (int rc = ags_each_device(sh, [&](size_t r) {
                std::vector<uint64_t> off;
                const HostBatch hb = b.slice(sh[r].lo, sh[r].cnt, off);
                return ssa_verify_batch_screened(m->ctxs[r], hb.sigs, hb.pks, hb.pk_inf, hb.msgs, hb.msg_off, msg_stride,
                                                 msg_len, sh[r].cnt, nullptr, status + sh[r].lo, &fails[r]);
            }))
            return rc;
    if (int rc = ags_multi_tops(m, sh, b, sigs, 81, B, false, tops)) return rc;
    uint64_t root[4];
    if (int rc = ags_multi_root(c0, tops, n, root)) return rc;
    // the second walk: the root to every device, its partial scalar, R's, statuses and count back
    if (int rc = ags_each_device(sh, [&](size_t r) {
            ssa_ctx *c = m->ctxs[r];
            const AgsShard &s = sh[r];
            HostCall hc(c);
            const u64 *d_root = hc.in<u64>(c->agm_roots, root, 32);
            u8 *d_e = hc.out(c->ag_misc, &parts[4 * r], 32, AG_MISC_BYTES);
            u8 *d_rs = hc.out(c->st_aux, agg_out + 49 * s.lo, 49 * s.cnt, 16);
            u8 *d_status = screened ? nullptr : hc.out(c->st_status, status + s.lo, s.cnt, 16);
            unsigned long long *d_fail = (unsigned long long *)c->ws_fail.p;
            if (!screened) hc.copy_back(&fails[r], d_fail, sizeof(uint64_t));
            return hc.finish([&] {
                HIP_TRY(hipMemsetAsync(d_fail, 0, sizeof(unsigned long long), c->stream));
                return ags_fold(c, s.dev, s.cnt, s.lo, d_root, d_e, d_rs, d_status, d_fail);
            });
        }))
        return rc;
    uint64_t nf = 0;
    for (uint64_t f : fails) nf += f;
    if (n_fail_out) *n_fail_out = nf;
    if (nf) {          // refused: no aggregate, the smallest nonzero status
        std::memset(agg_out, 0, SSA_AGGREGATE_LENGTH(n));
        int st = SSA_MALFORMED;
        if (screened)
            for (size_t i = 0; i < n; i++)
                if (status[i] && (int)status[i] < st) st = status[i];
        return st;
    }
    HostCall hc(c0);
    const u8 *d_parts = hc.in(c0->st_aux, parts.data(), 32 * world);
    u8 *d_e = hc.out(c0->ag_misc, agg_out + 49 * n, 32, AG_MISC_BYTES);
    return hc.finish([&] { return ssa_aggregate_combine_device(c0, d_parts, world, d_e); });
}

extern "C" int ssa_multi_verify_aggregate(ssa_multi *m, const uint8_t *agg, const uint8_t *pks, const uint8_t *pk_inf,
                                          const uint8_t *msgs, const uint64_t *msg_off, size_t msg_stride, size_t msg_len,
                                          size_t n) {
    if (!m || m->ctxs.empty() || !agg || (n && !pks)) return SSA_ERR_ARG;
    if (int rc = check_msgs({msgs, msg_off, msg_stride, msg_len}, n)) return rc;
    if (int rc = check_host_offsets(msg_off, n)) return rc;
    ssa_ctx *c0 = m->ctxs[0];
    if (n == 0) return ssa_verify_aggregate(c0, agg, pks, pk_inf, msgs, msg_off, msg_stride, msg_len, 0);
    const size_t world = m->ctxs.size(), B = ags_block(c0);
    const HostBatch b{nullptr, pks, pk_inf, msgs, msg_off, msg_stride, msg_len};
    std::vector<AgsShard> sh = ags_split(n, B, world);
    std::vector<uint64_t> tops(4 * ((n + B - 1) / B), 0), recs(SSA_MSM_PARTIAL_WORDS * world, 0);
    for (size_t r = 0; r < world; r++) recs[SSA_MSM_PARTIAL_WORDS * r + 23] = SSA_MSM_RECORD_MAGIC;   // a device without lanes: the empty shard's record
    if (int rc = ags_multi_tops(m, sh, b, agg, 49, B, true, tops)) return rc;
    uint64_t root[4];
    if (int rc = ags_multi_root(c0, tops, n, root)) return rc;
    if (int rc = ags_each_device(sh, [&](size_t r) {
            ssa_ctx *c = m->ctxs[r];
            const AgsShard &s = sh[r];
            HostCall hc(c);
            const u64 *d_root = hc.in<u64>(c->agm_roots, root, 32);
            u64 *d_rec = (u64 *)hc.out(c->ag_misc, &recs[SSA_MSM_PARTIAL_WORDS * r], SSA_MSM_PARTIAL_WORDS * sizeof(u64),
                                       AG_MISC_BYTES);
            return hc.finish([&] { return ags_record(c, s.dev.sigs, s.dev, (const u64 *)c->ws_h.p, s.cnt, s.lo, d_root, d_rec); });
        }))
        return rc;
    HostCall hc(c0);
    const u64 *d_recs = hc.in<u64>(c0->st_aux, recs.data(), recs.size() * sizeof(uint64_t));
    const u8 *d_e = hc.in(c0->st_aux2, agg + 49 * n, 32);
    uint32_t v = SSA_MALFORMED, *d_verdict = (uint32_t *)((char *)c0->ws_fail.p + 32);
    hc.copy_back(&v, d_verdict, sizeof v);
    const int rc = hc.finish([&] { return ssa_verify_aggregate_combine_device(c0, d_recs, world, d_e, n, d_verdict); });
    return rc ? rc : (int)v;
}

// tests: the coefficients of n_s lanes whose first stands at lane0, from a root in host memory -> n_s x 16 bytes
extern "C" int ssa_debug_aggregate_shard_coeffs(ssa_ctx *ctx, const uint8_t root[32], size_t n_s, size_t lane0,
                                                uint8_t *coeffs16_out) {
    if (!ctx || !root || n_s > SSA_MAX_BATCH || lane0 > SSA_MAX_BATCH - n_s || (n_s && !coeffs16_out)) return SSA_ERR_ARG;
    if (n_s == 0) return 0;
    HostCall hc(ctx);
    const u64 *d_root = hc.in<u64>(ctx->agm_roots, root, 32);
    (void)hc.out(ctx->ag_coeffs, coeffs16_out, n_s * 16);
    return hc.finish([&] { return ags_coeffs(ctx, d_root, n_s, lane0); });
}

// ------------------------------------------------------------------ many aggregates in one call
// The plan on the device (ctx->agm_plan): k + 1 prefix sums, then the tree's descriptors pass after pass.  The host copy
// lives in the context; the event says when the last upload has read it.  pfirst_off != nullptr (the producer, DESIGN.md
// section 26): the k + 1 partial offsets follow the descriptors, at that byte of the plan.
static int agm_upload_plan(ssa_ctx *ctx, const AgPlan &pl, std::vector<AgPass> &passes, size_t *pfirst_off = nullptr) {
    if (!ctx->agm_plan_ev) HIP_TRY(hipEventCreateWithFlags(&ctx->agm_plan_ev, hipEventDisableTiming));
    else HIP_TRY(hipEventSynchronize(ctx->agm_plan_ev));
    std::vector<uint32_t> &h = ctx->agm_plan_host;
    h.assign(pl.first.begin(), pl.first.end());
    while (h.size() & 3u) h.push_back(0u);             // descriptors are four words: keep them 16-byte aligned
    passes.clear();
    for (const auto &pass : pl.passes) {
        passes.push_back({h.size() * sizeof(uint32_t), (u32)pass.size(), 0u});
        for (const AgTreeDesc &d : pass) h.insert(h.end(), {d.first, d.count, d.slot, d.top_n});
    }
    if (pfirst_off) {
        *pfirst_off = h.size() * sizeof(uint32_t);
        h.insert(h.end(), pl.pfirst.begin(), pl.pfirst.end());
    }
    if (ctx->agm_plan.reserve(h.size() * sizeof(uint32_t))) return SSA_ERR_HIP;
    HIP_TRY(hipMemcpyAsync(ctx->agm_plan.p, h.data(), h.size() * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipEventRecord(ctx->agm_plan_ev, ctx->stream));
    return 0;
}

// arguments of both forms: the plan from the caller's counts; *n_out = the lanes in all
static int agm_check_args(const ssa_ctx *ctx, const void *aggs, const uint64_t *counts, size_t k, const void *pks,
                          const MsgView &mv, const void *verdicts_out, AgPlan &pl, size_t *n_out) {
    *n_out = 0;
    if (!ctx) return SSA_ERR_ARG;
    if (k == 0) return 0;
    if (!aggs || !counts || !verdicts_out || k > SSA_MAX_BATCH) return SSA_ERR_ARG;
    if (int rc = ag_plan(counts, k, ctx->knobs.msm_slice, ctx->knobs.msm_small_max, pl)) return rc;
    *n_out = pl.first[k];
    if (*n_out && !pks) return SSA_ERR_ARG;
    return check_msgs(mv, *n_out);
}

static int agm_run(ssa_ctx *ctx, const AgPlan &pl, const uint8_t *d_aggs, size_t k, const uint8_t *d_pks,
                   const uint8_t *d_pk_inf, const MsgView &mv, size_t n, uint32_t *d_verdicts_out) {
    HIP_TRY(hipSetDevice(ctx->device));
    std::vector<AgPass> passes;
    if (int rc = agm_upload_plan(ctx, pl, passes)) return rc;
    const u32 *d_first = (const u32 *)ctx->agm_plan.p;
    // the R's at stride 81 into ctx->ag_sigs, the challenge scalars into ctx->ws_h, the coefficients into ctx->ag_coeffs
    if (n)
        if (int rc = ag_transcript(ctx, d_aggs, nullptr, d_pks, mv, n, true, d_first, k, passes)) return rc;
    if (!d_verdicts_out) return 0;       // (ssa_debug_aggregates_many_coeffs: the transcript alone)
    const DevBatch b{(const u8 *)ctx->ag_sigs.p, d_pks, d_pk_inf, mv};
    for (const AgGroup &g : pl.groups) {
        if (!g.bucket) {
            const uint64_t *d_recs = nullptr;
            if (int rc = ssa_internal_msm_agg_small(ctx, b.slice(g.lane0), g.lanes,
                                                    (const u8 *)ctx->ag_coeffs.p + 16 * (size_t)g.lane0, d_first, g.agg0,
                                                    g.aggs, &d_recs))
                return rc;
            const int rc = timed_launch(ctx, "ag_k_finish", [&] {
                hipLaunchKernelGGL(ag_k_finish, dim3(g.aggs), dim3(64), 0, ctx->stream, (const u64 *)d_recs, d_aggs, d_first,
                                   (size_t)0, g.agg0, (const u64 *)ctx->d_gtab, d_verdicts_out);
            });
            if (rc) return rc;
            continue;
        }
        // the padded group: R's | keys | challenge scalars | coefficients, then the byte arrays
        const size_t m = (size_t)g.aggs * g.seg_lanes;
        auto al = [](size_t v) { return (v + 255) & ~(size_t)255; };
        const size_t o_pks = al(m * 81 + 16), o_h = o_pks + m * 96, o_co = o_h + m * 32, in_total = o_co + m * 16;
        const size_t o_mask = al(m), o_re = o_mask + al(m), o_ok = o_re + al(m), o_rhs = o_ok + 256,
                     by_total = o_rhs + 32 * (size_t)AG_GROUP_MAX;
        if (ctx->agm_in.reserve(in_total) || ctx->agm_bytes.reserve(by_total)) return SSA_ERR_HIP;
        u8 *gi = (u8 *)ctx->agm_in.p, *gb = (u8 *)ctx->agm_bytes.p;
        int rc = timed_launch(ctx, "ag_k_gather", [&] {
            hipLaunchKernelGGL(ag_k_gather_rs, dim3(grid_for(m * 81 / 4, 256)), dim3(256), 0, ctx->stream, d_aggs, d_first,
                               g.agg0, g.aggs, g.seg_lanes, gi);
            hipLaunchKernelGGL(ag_k_gather, dim3(grid_for(m, 256)), dim3(256), 0, ctx->stream, d_aggs, d_first, g.agg0, g.aggs,
                               g.seg_lanes, d_pks, d_pk_inf, (const u64 *)ctx->ws_h.p, (const u64 *)ctx->ag_coeffs.p,
                               gi + o_pks, gb, (u64 *)(gi + o_h), (u64 *)(gi + o_co), gb + o_mask, gb + o_rhs);
        });
        if (rc) return rc;
        const DevBatch padded{gi, gi + o_pks, gb, {}};
        if ((rc = ssa_internal_msm_agg_segments(ctx, padded, g.aggs, g.seg_lanes, gi + o_co, (const uint64_t *)(gi + o_h),
                                                gb + o_mask, gb + o_re, gb + o_rhs, gb + o_ok)))
            return rc;
        rc = timed_launch(ctx, "ag_k_finish", [&] {
            hipLaunchKernelGGL(ag_k_verdicts_seg, dim3(g.aggs), dim3(256), 0, ctx->stream, gb + o_ok, gb + o_re, gb + o_mask,
                               gb + o_rhs, g.seg_lanes, d_verdicts_out + g.agg0);
        });
        if (rc) return rc;
    }
    return 0;
}

extern "C" int ssa_verify_aggregates_many_device(ssa_ctx *ctx, const uint8_t *d_aggs, const uint64_t *counts, size_t k,
                                                 const uint8_t *d_pks, const uint8_t *d_pk_inf, const uint8_t *d_msgs,
                                                 const uint64_t *d_msg_off, size_t msg_stride, size_t msg_len,
                                                 uint32_t *d_verdicts_out) {
    const MsgView mv{d_msgs, d_msg_off, msg_stride, msg_len};
    AgPlan pl;
    size_t n = 0;
    if (int rc = agm_check_args(ctx, d_aggs, counts, k, d_pks, mv, d_verdicts_out, pl, &n)) return rc;
    if (k == 0) return SSA_OK;
    return agm_run(ctx, pl, d_aggs, k, d_pks, d_pk_inf, mv, n, d_verdicts_out);
}

extern "C" int ssa_verify_aggregates_many(ssa_ctx *ctx, const uint8_t *aggs, const uint64_t *counts, size_t k,
                                          const uint8_t *pks, const uint8_t *pk_inf, const uint8_t *msgs,
                                          const uint64_t *msg_off, size_t msg_stride, size_t msg_len, uint32_t *verdicts_out) {
    AgPlan pl;
    size_t n = 0;
    if (int rc = agm_check_args(ctx, aggs, counts, k, pks, {msgs, msg_off, msg_stride, msg_len}, verdicts_out, pl, &n)) return rc;
    if (int rc = check_host_offsets(msg_off, n)) return rc;
    if (k == 0) return SSA_OK;
    HostCall hc(ctx);
    const DevBatch b = hc.lanes({aggs, pks, pk_inf, msgs, msg_off, msg_stride, msg_len}, 49 * n + 32 * k, n);
    uint32_t *d_verdicts = (uint32_t *)hc.out(ctx->st_status, verdicts_out, k * sizeof(uint32_t), 16);
    return hc.finish([&] { return agm_run(ctx, pl, b.sigs, k, b.pks, b.pk_inf, b.msgs, n, d_verdicts); });
}

// ------------------------------------------------------------------ the producer of many aggregates
// ctx->agp_acc: two words per aggregate (failing lanes, 256 - the smallest nonzero status), zeroed before every fold, and
// behind them the results when the caller takes none
static int agp_run(ssa_ctx *ctx, const AgPlan &pl, const uint8_t *d_sigs, size_t k, const uint8_t *d_pks,
                   const uint8_t *d_pk_inf, const MsgView &mv, size_t n, uint32_t flags, uint8_t *d_aggs_out,
                   uint32_t *d_results_out, uint8_t *d_status_out, uint64_t *d_n_fail_out) {
    unsigned long long *d_fail;
    if (int rc = reset_fail_counter(ctx, d_n_fail_out, &d_fail)) return rc;
    const bool screened = (flags & SSA_AGG_CHECK) != 0;
    const size_t acc_bytes = (2 * k * sizeof(u32) + 15) & ~(size_t)15;
    if (ctx->agp_acc.reserve(acc_bytes + k * sizeof(u32)) || (n && !d_status_out && ctx->ag_status.reserve(n + 16)) ||
        ctx->ag_partials.reserve((size_t)pl.pfirst[k] * 32 + 32))
        return SSA_ERR_HIP;
    u32 *d_acc = (u32 *)ctx->agp_acc.p;
    u32 *d_results = d_results_out ? d_results_out : (u32 *)((u8 *)ctx->agp_acc.p + acc_bytes);
    u8 *d_status = d_status_out ? d_status_out : (u8 *)ctx->ag_status.p;
    // the screen counts the failing lanes of the call itself; its statuses do not depend on how the lanes are grouped
    if (screened && n)
        if (int rc = ssa_verify_batch_screened_device(ctx, d_sigs, d_pks, d_pk_inf, mv.msgs, mv.off, mv.stride, mv.len, n,
                                                      nullptr, 0, d_status, (uint64_t *)d_fail))
            return rc;
    std::vector<AgPass> passes;
    size_t pfirst_off = 0;
    if (int rc = agm_upload_plan(ctx, pl, passes, &pfirst_off)) return rc;
    const u32 *d_first = (const u32 *)ctx->agm_plan.p, *d_pfirst = (const u32 *)((const u8 *)ctx->agm_plan.p + pfirst_off);
    HIP_TRY(hipMemsetAsync(d_acc, 0, acc_bytes, ctx->stream));
    if (n) {
        if (int rc = ag_transcript(ctx, nullptr, d_sigs, d_pks, mv, n, false, d_first, k, passes)) return rc;
        const int rc = timed_launch(ctx, "ag_k_fold_seg", [&] {
            hipLaunchKernelGGL(ag_k_fold_seg, dim3(grid_for(n, 256)), dim3(256), 0, ctx->stream, d_sigs, d_pks, d_pk_inf,
                               (const u64 *)ctx->ag_coeffs.p, (const u32 *)ctx->agm_map.p, d_first, d_pfirst, n,
                               (u64 *)ctx->ag_partials.p, d_status, screened ? 1u : 0u, d_acc);
        });
        if (rc) return rc;
    }
    int rc = timed_launch(ctx, "ag_k_fold_finish_seg", [&] {
        hipLaunchKernelGGL(ag_k_fold_finish_seg, dim3((unsigned)k), dim3(64), 0, ctx->stream, (const u64 *)ctx->ag_partials.p,
                           d_first, d_pfirst, (const u32 *)d_acc, d_aggs_out, d_results,
                           screened ? (unsigned long long *)nullptr : d_fail);
    });
    if (rc || !n) return rc;
    return timed_launch(ctx, "ag_k_pack_many", [&] {
        hipLaunchKernelGGL(ag_k_pack_many, dim3(grid_for((n * 49 + 3) / 4, 256)), dim3(256), 0, ctx->stream, d_sigs,
                           (const u32 *)ctx->agm_map.p, (const u32 *)d_results, n, d_aggs_out);
    });
}

// arguments of both forms: those of ssa_verify_aggregates_many with aggs_out in the place of the wire form and of the
// verdicts, then the flags and the signatures
static int agp_check_args(const ssa_ctx *ctx, const void *sigs, const uint64_t *counts, size_t k, const void *pks,
                          const MsgView &mv, uint32_t flags, const void *aggs_out, AgPlan &pl, size_t *n_out) {
    *n_out = 0;
    if (!ctx || (flags & ~SSA_AGG_CHECK)) return SSA_ERR_ARG;
    if (int rc = agm_check_args(ctx, aggs_out, counts, k, pks, mv, aggs_out, pl, n_out)) return rc;
    return *n_out && !sigs ? SSA_ERR_ARG : 0;
}

// Only enqueues, but for what ssa_verify_batch_screened_device does under SSA_AGG_CHECK.
extern "C" int ssa_aggregates_many_device(ssa_ctx *ctx, const uint8_t *d_sigs, const uint64_t *counts, size_t k,
                                          const uint8_t *d_pks, const uint8_t *d_pk_inf, const uint8_t *d_msgs,
                                          const uint64_t *d_msg_off, size_t msg_stride, size_t msg_len, uint32_t flags,
                                          uint8_t *d_aggs_out, uint32_t *d_results_out, uint8_t *d_status_out,
                                          uint64_t *d_n_fail_out) {
    const MsgView mv{d_msgs, d_msg_off, msg_stride, msg_len};
    AgPlan pl;
    size_t n = 0;
    if (int rc = agp_check_args(ctx, d_sigs, counts, k, d_pks, mv, flags, d_aggs_out, pl, &n)) return rc;
    if (k == 0) {
        unsigned long long *d_fail;
        return reset_fail_counter(ctx, d_n_fail_out, &d_fail);
    }
    return agp_run(ctx, pl, d_sigs, k, d_pks, d_pk_inf, mv, n, flags, d_aggs_out, d_results_out, d_status_out, d_n_fail_out);
}

extern "C" int ssa_aggregates_many(ssa_ctx *ctx, const uint8_t *sigs, const uint64_t *counts, size_t k, const uint8_t *pks,
                                   const uint8_t *pk_inf, const uint8_t *msgs, const uint64_t *msg_off, size_t msg_stride,
                                   size_t msg_len, uint32_t flags, uint8_t *aggs_out, uint32_t *results_out,
                                   uint8_t *status_out, uint64_t *n_fail_out) {
    AgPlan pl;
    size_t n = 0;
    if (int rc = agp_check_args(ctx, sigs, counts, k, pks, {msgs, msg_off, msg_stride, msg_len}, flags, aggs_out, pl, &n))
        return rc;
    if (int rc = check_host_offsets(msg_off, n)) return rc;
    if (n_fail_out) *n_fail_out = 0;
    if (k == 0) return SSA_OK;
    HostCall hc(ctx);
    const DevBatch b = hc.lanes({sigs, pks, pk_inf, msgs, msg_off, msg_stride, msg_len}, n * 81, n);
    u8 *d_aggs = hc.out(ctx->st_aux, aggs_out, 49 * n + 32 * k, 16);
    uint32_t *d_results = (uint32_t *)hc.out(ctx->st_aux2, results_out, k * sizeof(uint32_t), 16);
    u8 *d_status = hc.out(ctx->st_status, status_out, n, 16);
    unsigned long long nf = 0;
    hc.copy_back(&nf, ctx->ws_fail.p, sizeof nf);
    const int rc = hc.finish([&] {
        return agp_run(ctx, pl, n ? b.sigs : nullptr, k, n ? b.pks : nullptr, b.pk_inf, b.msgs, n, flags, d_aggs, d_results,
                       d_status, nullptr);
    });
    if (rc) return rc;
    if (n_fail_out) *n_fail_out = nf;
    return SSA_OK;
}

// ------------------------------------------------------------------ aggregates through a key cache
// The cache in front of agm_run, and the fold of the key statuses behind it.  The N lanes go through the cache in slices
// of at most lane_slice lanes, in order, whatever the aggregate boundaries; a later slice may clear or compact the
// cache, so each slice leaves what the aggregate stages need of its rows in N-lane buffers of the context
// (agc_k_expand) before the next one starts.  Then agm_run as it is over U, then agc_k_key_verdicts.
// wire: d_keys = N dense 49-byte keys (a wire cache), else N affine keys with d_pk_inf (an affine cache).
// sv (or nullptr): words 0..4 of the statistics and the host's part of word 5; the device's part of word 5 and word 6
// are ctx->agc_cnt, read by the caller behind everything queued here.  One synchronisation per slice, the dedup's.
static int agc_check_cache(const ssa_ctx *ctx, const ssa_keycache *kc, bool wire) {
    return !ctx || !kc || kc->ctx != ctx || kc->wire_mode != wire ? SSA_ERR_ARG : 0;
}

// The cache in front of an aggregate call, in two steps, because the streaming verifier zeroes its object's statuses
// between them.  First: the context's device is selected, the n-lane buffers of wire keys reserved and the counters
// ctx->agc_cnt zeroed on the stream.  own_kst: the statuses go to ctx->agc_kst, reserved here too.
static int agc_begin(ssa_ctx *ctx, bool wire, size_t n, bool own_kst) {
    HIP_TRY(hipSetDevice(ctx->device));
    if (ctx->agc_cnt.reserve(64) || (own_kst && ctx->agc_kst.reserve(n + 16)) ||
        (wire && (ctx->agc_pks.reserve(n * 96 + 16) || ctx->agc_inf.reserve(n + 16))))
        return SSA_ERR_HIP;
    HIP_TRY(hipMemsetAsync(ctx->agc_cnt.p, 0, AGC_CNT_WORDS * sizeof(unsigned long long), ctx->stream));
    return 0;
}

// Then the slices: the lanes' key statuses go to kst[0, n) -- ctx->agc_kst for the many-aggregates call, the object's
// kst + held for the streaming verifier -- and *u names the keys and flags U that the following stage reads: the
// caller's, or for wire keys what agc_k_expand wrote into ctx->agc_pks and ctx->agc_inf.  sv (or nullptr) as above.
static int agc_slices(ssa_ctx *ctx, ssa_keycache *kc, const uint8_t *d_keys, const uint8_t *d_pk_inf, bool wire, size_t n,
                      u8 *kst, uint64_t *sv, DevBatch *u) {
    unsigned long long *d_cnt = (unsigned long long *)ctx->agc_cnt.p;
    u8 *u_inf = wire ? (u8 *)ctx->agc_inf.p : nullptr;
    u64 *u_pks = wire ? (u64 *)ctx->agc_pks.p : nullptr;
    const size_t slice = ctx->knobs.lane_slice;
    for (size_t lo = 0; lo < n; lo += slice) {
        const size_t cnt = n - lo < slice ? n - lo : slice;
        const KeySource src = wire ? KeySource{nullptr, nullptr, d_keys + 49 * lo, 49}
                                   : KeySource{d_keys + 96 * lo, d_pk_inf ? d_pk_inf + lo : nullptr, nullptr};
        KeyView kv{};
        KeyRows rows{};
        uint64_t u = 0, hits = 0, ks[4] = {0, 0, 0, 0};
        const unsigned long long *d_unpub = nullptr;
        if (int rc = keycache_slice(ctx, kc, src, cnt, nullptr, &kv, &u, &hits, ks, &d_unpub, &rows)) return rc;
        const int rc = timed_launch(ctx, "agc_expand", [&] {
            hipLaunchKernelGGL(agc_k_expand, dim3(grid_for(wire ? cnt * 12 : cnt, 256)), dim3(256), 0, ctx->stream, kv.lane_key,
                               kv.status, wire ? rows.pks : (const u64 *)nullptr, rows.inf, kv.n_keys, (u32)cnt, kst + lo,
                               wire ? u_pks + 12 * lo : (u64 *)nullptr, wire ? u_inf + lo : (u8 *)nullptr, d_unpub, d_cnt);
        });
        if (rc) return rc;
        if (sv) {
            sv[0] += u;
            for (int w = 0; w < 4; w++) sv[1 + w] += ks[w];
            sv[5] += hits;
        }
    }
    u->pks = wire ? (const u8 *)u_pks : d_keys;
    u->pk_inf = wire ? (const u8 *)u_inf : d_pk_inf;
    return 0;
}

static int agc_run(ssa_ctx *ctx, ssa_keycache *kc, const AgPlan &pl, const uint8_t *d_aggs, size_t k, const uint8_t *d_keys,
                   const uint8_t *d_pk_inf, bool wire, const MsgView &mv, size_t n, uint32_t *d_verdicts_out, uint64_t *sv) {
    if (int rc = agc_begin(ctx, wire, n, true)) return rc;
    u8 *kst = (u8 *)ctx->agc_kst.p;
    DevBatch u{};
    if (int rc = agc_slices(ctx, kc, d_keys, d_pk_inf, wire, n, kst, sv, &u)) return rc;
    if (int rc = agm_run(ctx, pl, d_aggs, k, u.pks, u.pk_inf, mv, n, d_verdicts_out)) return rc;
    if (n == 0) return 0;       // (no lane, no key: every verdict is V_j)
    return timed_launch(ctx, "agc_k_key_verdicts", [&] {
        hipLaunchKernelGGL(agc_k_key_verdicts, dim3(grid_for(k, AGC_WAVES)), dim3(AGC_BLOCK), 0, ctx->stream, (const u8 *)kst,
                           (const u32 *)ctx->agm_plan.p, (u32)k, d_verdicts_out, (unsigned long long *)ctx->agc_cnt.p);
    });
}

// The caller's eight statistics words (or nullptr): words 0..4 and the host's part of word 5 from sv, the device's part
// of word 5 from the counters the device kept, and word 6 from them too where the call has verdicts (a push of the
// streaming verifier has none before finish: its [6] and [7] stay 0).
static void agc_stats_out(uint64_t stats_out[8], const uint64_t sv[8], const unsigned long long cnt[AGC_CNT_WORDS],
                          bool verdicts) {
    if (!stats_out) return;
    for (int w = 0; w < 8; w++) stats_out[w] = w < 6 ? sv[w] : 0;
    stats_out[5] += cnt[AGC_CNT_UNPUB];
    if (verdicts) stats_out[6] = cnt[AGC_CNT_BAD];
}

// the device forms, behind everything queued: the counters are read back only for a caller that asks for statistics,
// and that is its one extra wait
static int agc_stats_dev(ssa_ctx *ctx, uint64_t stats_out[8], const uint64_t sv[8], bool verdicts) {
    if (!stats_out) return 0;
    unsigned long long cnt[AGC_CNT_WORDS] = {0, 0};
    HIP_TRY(hipMemcpyAsync(cnt, ctx->agc_cnt.p, sizeof cnt, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    agc_stats_out(stats_out, sv, cnt, verdicts);
    return 0;
}

static int agc_device(ssa_ctx *ctx, ssa_keycache *kc, const uint8_t *d_aggs, const uint64_t *counts, size_t k,
                      const uint8_t *d_keys, const uint8_t *d_pk_inf, bool wire, const MsgView &mv, uint32_t *d_verdicts_out,
                      uint64_t stats_out[8]) {
    AgPlan pl;
    size_t n = 0;
    if (int rc = agc_check_cache(ctx, kc, wire)) return rc;
    if (int rc = agm_check_args(ctx, d_aggs, counts, k, d_keys, mv, d_verdicts_out, pl, &n)) return rc;
    uint64_t sv[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    unsigned long long cnt[AGC_CNT_WORDS] = {0, 0};
    agc_stats_out(stats_out, sv, cnt, true);      // (still empty: the caller's words are zeroed)
    if (k == 0) return SSA_OK;
    if (int rc = agc_run(ctx, kc, pl, d_aggs, k, d_keys, d_pk_inf, wire, mv, n, d_verdicts_out, sv)) return rc;
    return agc_stats_dev(ctx, stats_out, sv, true);      // (the two words the device counted, behind the aggregate stages)
}

static int agc_host(ssa_ctx *ctx, ssa_keycache *kc, const uint8_t *aggs, const uint64_t *counts, size_t k,
                    const uint8_t *keys, const uint8_t *pk_inf, bool wire, const uint8_t *msgs, const uint64_t *msg_off,
                    size_t msg_stride, size_t msg_len, uint32_t *verdicts_out, uint64_t stats_out[8]) {
    AgPlan pl;
    size_t n = 0;
    if (int rc = agc_check_cache(ctx, kc, wire)) return rc;
    if (int rc = agm_check_args(ctx, aggs, counts, k, keys, {msgs, msg_off, msg_stride, msg_len}, verdicts_out, pl, &n)) return rc;
    if (int rc = check_host_offsets(msg_off, n)) return rc;
    uint64_t sv[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    unsigned long long cnt[AGC_CNT_WORDS] = {0, 0};
    agc_stats_out(stats_out, sv, cnt, true);      // (still empty: the caller's words are zeroed)
    if (k == 0) return SSA_OK;
    HostCall hc(ctx);
    const DevBatch b = hc.lanes({aggs, keys, pk_inf, msgs, msg_off, msg_stride, msg_len}, 49 * n + 32 * k, n, wire);
    uint32_t *d_verdicts = (uint32_t *)hc.out(ctx->st_status, verdicts_out, k * sizeof(uint32_t), 16);
    (void)hc.out(ctx->agc_cnt, cnt, sizeof cnt, 48);      // (copied back behind the verdicts)
    if (int rc = hc.finish([&] { return agc_run(ctx, kc, pl, b.sigs, k, b.pks, b.pk_inf, wire, b.msgs, n, d_verdicts, sv); }))
        return rc;
    agc_stats_out(stats_out, sv, cnt, true);
    return 0;
}

extern "C" int ssa_verify_aggregates_many_cached_device(ssa_ctx *ctx, ssa_keycache *kc, const uint8_t *d_aggs,
                                                        const uint64_t *counts, size_t k, const uint8_t *d_pks,
                                                        const uint8_t *d_pk_inf, const uint8_t *d_msgs,
                                                        const uint64_t *d_msg_off, size_t msg_stride, size_t msg_len,
                                                        uint32_t *d_verdicts_out, uint64_t stats_out[8]) {
    return agc_device(ctx, kc, d_aggs, counts, k, d_pks, d_pk_inf, false, {d_msgs, d_msg_off, msg_stride, msg_len},
                      d_verdicts_out, stats_out);
}

extern "C" int ssa_verify_aggregates_many_cached(ssa_ctx *ctx, ssa_keycache *kc, const uint8_t *aggs, const uint64_t *counts,
                                                 size_t k, const uint8_t *pks, const uint8_t *pk_inf, const uint8_t *msgs,
                                                 const uint64_t *msg_off, size_t msg_stride, size_t msg_len,
                                                 uint32_t *verdicts_out, uint64_t stats_out[8]) {
    return agc_host(ctx, kc, aggs, counts, k, pks, pk_inf, false, msgs, msg_off, msg_stride, msg_len, verdicts_out, stats_out);
}

extern "C" int ssa_verify_aggregates_many_cached_wire_device(ssa_ctx *ctx, ssa_keycache *kc, const uint8_t *d_aggs,
                                                             const uint64_t *counts, size_t k, const uint8_t *d_pks49,
                                                             const uint8_t *d_msgs, const uint64_t *d_msg_off,
                                                             size_t msg_stride, size_t msg_len, uint32_t *d_verdicts_out,
                                                             uint64_t stats_out[8]) {
    return agc_device(ctx, kc, d_aggs, counts, k, d_pks49, nullptr, true, {d_msgs, d_msg_off, msg_stride, msg_len},
                      d_verdicts_out, stats_out);
}

extern "C" int ssa_verify_aggregates_many_cached_wire(ssa_ctx *ctx, ssa_keycache *kc, const uint8_t *aggs,
                                                      const uint64_t *counts, size_t k, const uint8_t *pks49,
                                                      const uint8_t *msgs, const uint64_t *msg_off, size_t msg_stride,
                                                      size_t msg_len, uint32_t *verdicts_out, uint64_t stats_out[8]) {
    return agc_host(ctx, kc, aggs, counts, k, pks49, nullptr, true, msgs, msg_off, msg_stride, msg_len, verdicts_out,
                    stats_out);
}

// ------------------------------------------------------------------ the streaming verifier through a key cache
// The cache in front of the push of section 28, as agc_run puts it in front of agm_run: the n lanes go through the
// cache in slices of at most lane_slice lanes, and behind each slice, before the next one may clear or compact the
// cache, agc_k_expand writes the lanes' key statuses into the OBJECT (kst + held + lo) and, for wire keys, the keys and
// flags into the context's n-lane buffers.  Then the push body of section 28 unchanged over U.  The first cached push of
// an object turns `keyed` on behind a zeroing of kst[0, held) (the rule in ssa_aggverifier.hpp).  `held` moves in the
// body, behind the last launch: a push that fails on the way leaves the object's lanes as they were (the cache may have
// taken keys, as after a failed ssa_verify_many_cached).  sv: words 0..4 of the statistics and the host's part of word
// 5; the device's part is ctx->agc_cnt[AGC_CNT_UNPUB].  One synchronisation per slice, the dedup's.
static int agv_push_cached_run(ssa_ctx *ctx, ssa_aggverifier *av, ssa_keycache *kc, const u8 *d_rs49, const u8 *d_keys,
                               const u8 *d_pk_inf, bool wire, const MsgView &mv, size_t n, uint64_t *sv) {
    if (int rc = agc_begin(ctx, wire, n, false)) return rc;
    if (!av->keyed) {
        if (av->held) HIP_TRY(hipMemsetAsync(av->kst.p, 0, av->held, ctx->stream));
        av->keyed = true;
    }
    DevBatch u{};
    if (int rc = agc_slices(ctx, kc, d_keys, d_pk_inf, wire, n, (u8 *)av->kst.p + av->held, sv, &u)) return rc;
    return agv_push_body(ctx, av, d_rs49, u.pks, u.pk_inf, mv, n, true);
}

// what all four cached pushes refuse before anything is enqueued, counted or written
static int agv_push_cached_args(const ssa_ctx *ctx, const ssa_aggverifier *av, const ssa_keycache *kc, bool wire,
                                const MsgView &mv, size_t n, const void *rs49, const void *keys) {
    if (int rc = agc_check_cache(ctx, kc, wire)) return rc;
    return agv_push_args(ctx, av, mv, n, rs49, keys);
}

// The statistics of a cached push: words 0..5 of section 23's; [6] and [7] stay 0 (agc_stats_out without verdicts):
// nothing about verdicts is known before finish.
static int agv_push_cached_dev(ssa_ctx *ctx, ssa_aggverifier *av, ssa_keycache *kc, const u8 *d_rs49, const u8 *d_keys,
                               const u8 *d_pk_inf, bool wire, const MsgView &mv, size_t n, uint64_t stats_out[8]) {
    if (int rc = agv_push_cached_args(ctx, av, kc, wire, mv, n, d_rs49, d_keys)) return rc;
    uint64_t sv[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const unsigned long long none[AGC_CNT_WORDS] = {0, 0};
    agc_stats_out(stats_out, sv, none, false);
    if (n == 0) return agv_push_body(ctx, av, nullptr, nullptr, nullptr, mv, 0, false);
    if (int rc = agv_push_cached_run(ctx, av, kc, d_rs49, d_keys, d_pk_inf, wire, mv, n, sv)) return rc;
    return agc_stats_dev(ctx, stats_out, sv, false);      // (the one word the device counted, behind the push)
}

static int agv_push_cached_host(ssa_ctx *ctx, ssa_aggverifier *av, ssa_keycache *kc, const uint8_t *rs49,
                                const uint8_t *keys, const uint8_t *pk_inf, bool wire, const uint8_t *msgs,
                                const uint64_t *msg_off, size_t msg_stride, size_t msg_len, size_t n, uint64_t stats_out[8]) {
    if (int rc = agv_push_cached_args(ctx, av, kc, wire, {msgs, msg_off, msg_stride, msg_len}, n, rs49, keys)) return rc;
    if (int rc = check_host_offsets(msg_off, n)) return rc;
    if (n == 0)
        return agv_push_cached_dev(ctx, av, kc, nullptr, nullptr, nullptr, wire, {nullptr, nullptr, msg_stride, msg_len}, 0,
                                   stats_out);
    uint64_t sv[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    unsigned long long cnt[AGC_CNT_WORDS] = {0, 0};
    agc_stats_out(stats_out, sv, cnt, false);
    HostCall hc(ctx);
    const DevBatch b = hc.lanes({rs49, keys, pk_inf, msgs, msg_off, msg_stride, msg_len}, n * 49, n, wire);
    (void)hc.out(ctx->agc_cnt, cnt, sizeof cnt, 48);      // (copied back behind the push: finish() waits for it, and with
                                                          //  it for the kernels that read the staging buffers)
    if (int rc = hc.finish([&] { return agv_push_cached_run(ctx, av, kc, b.sigs, b.pks, b.pk_inf, wire, b.msgs, n, sv); }))
        return rc;
    agc_stats_out(stats_out, sv, cnt, false);
    return SSA_OK;
}

extern "C" int ssa_aggverifier_push_cached_device(ssa_ctx *ctx, ssa_aggverifier *av, ssa_keycache *kc, const uint8_t *d_rs49,
                                                  const uint8_t *d_pks, const uint8_t *d_pk_inf, const uint8_t *d_msgs,
                                                  const uint64_t *d_msg_off, size_t msg_stride, size_t msg_len, size_t n,
                                                  uint64_t stats_out[8]) {
    return agv_push_cached_dev(ctx, av, kc, d_rs49, d_pks, d_pk_inf, false, {d_msgs, d_msg_off, msg_stride, msg_len}, n,
                               stats_out);
}

extern "C" int ssa_aggverifier_push_cached(ssa_ctx *ctx, ssa_aggverifier *av, ssa_keycache *kc, const uint8_t *rs49,
                                           const uint8_t *pks, const uint8_t *pk_inf, const uint8_t *msgs,
                                           const uint64_t *msg_off, size_t msg_stride, size_t msg_len, size_t n,
                                           uint64_t stats_out[8]) {
    return agv_push_cached_host(ctx, av, kc, rs49, pks, pk_inf, false, msgs, msg_off, msg_stride, msg_len, n, stats_out);
}

extern "C" int ssa_aggverifier_push_cached_wire_device(ssa_ctx *ctx, ssa_aggverifier *av, ssa_keycache *kc,
                                                       const uint8_t *d_rs49, const uint8_t *d_pks49, const uint8_t *d_msgs,
                                                       const uint64_t *d_msg_off, size_t msg_stride, size_t msg_len, size_t n,
                                                       uint64_t stats_out[8]) {
    return agv_push_cached_dev(ctx, av, kc, d_rs49, d_pks49, nullptr, true, {d_msgs, d_msg_off, msg_stride, msg_len}, n,
                               stats_out);
}

extern "C" int ssa_aggverifier_push_cached_wire(ssa_ctx *ctx, ssa_aggverifier *av, ssa_keycache *kc, const uint8_t *rs49,
                                                const uint8_t *pks49, const uint8_t *msgs, const uint64_t *msg_off,
                                                size_t msg_stride, size_t msg_len, size_t n, uint64_t stats_out[8]) {
    return agv_push_cached_host(ctx, av, kc, rs49, pks49, nullptr, true, msgs, msg_off, msg_stride, msg_len, n, stats_out);
}

// ------------------------------------------------------------------ a block against the pool through the key cache
// The cache in front of the mixed push of section 34, as agv_push_cached_run puts it in front of the plain push: the u
// compact keys go through the cache in slices of at most lane_slice lanes; agc_k_expand leaves their statuses DENSE in
// ctx->agc_kst (a compact lane's place in the object is known only on the device) and, for wire keys, the keys and
// flags in the context's u-lane buffers; the body then scatters the statuses behind its append (agv_k_kst_at).  The
// first such push turns `keyed` on behind a zeroing of kst[0, held).  require > 0: the classification reads the pool's
// admission column.  One synchronisation per slice, the dedup's; none without an unknown lane.
// what all four forms refuse before anything is enqueued, counted or written
static int agv_mixed_cached_args(const ssa_ctx *ctx, const ssa_aggverifier *av, const ssa_aggregator *ag,
                                 const ssa_keycache *kc, bool wire, const uint32_t *places, size_t n, size_t u,
                                 const MsgView &mv, const void *rs49, const void *keys, uint32_t require, bool device) {
    if (int rc = agc_check_cache(ctx, kc, wire)) return rc;
    if (int rc = agv_mixed_args(ctx, av, ag, places, n, u, mv, rs49, keys, device)) return rc;
    return require > SSA_ADM_KEY_CHECKED || (require && !ag->hold_adm()) ? SSA_ERR_ARG : 0;
}

// n >= 1, the context's device selected
static int agv_push_mixed_cached_run(ssa_ctx *ctx, ssa_aggverifier *av, const ssa_aggregator *ag, ssa_keycache *kc,
                                     const u32 *d_places, size_t n, size_t u, const u8 *d_rs49, const u8 *d_keys,
                                     const u8 *d_pk_inf, bool wire, const MsgView &mv, u32 require, u32 *d_result_out,
                                     uint64_t *sv) {
    AgvMixedCached mc;
    mc.require = require;
    if (u)
        if (int rc = agc_begin(ctx, wire, u, true)) return rc;
    if (!av->keyed) {
        if (av->held) HIP_TRY(hipMemsetAsync(av->kst.p, 0, av->held, ctx->stream));
        av->keyed = true;
    }
    DevBatch U{};
    if (u) {
        if (int rc = agc_slices(ctx, kc, d_keys, d_pk_inf, wire, u, (u8 *)ctx->agc_kst.p, sv, &U)) return rc;
        mc.d_kst = (const u8 *)ctx->agc_kst.p;
    }
    return agv_push_mixed_body(ctx, av, ag, d_places, n, u, d_rs49, U.pks, U.pk_inf, mv, d_result_out, mc);
}

static int agv_push_mixed_cached_dev(ssa_ctx *ctx, ssa_aggverifier *av, ssa_aggregator *ag, ssa_keycache *kc,
                                     const uint32_t *d_places, size_t n, const u8 *d_rs49, const u8 *d_keys,
                                     const u8 *d_pk_inf, bool wire, const MsgView &mv, size_t u, uint32_t require,
                                     uint32_t *d_result_out, uint64_t stats_out[8]) {
    if (int rc = agv_mixed_cached_args(ctx, av, ag, kc, wire, d_places, n, u, mv, d_rs49, d_keys, require, true)) return rc;
    if (!d_result_out) return SSA_ERR_ARG;
    uint64_t sv[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const unsigned long long none[AGC_CNT_WORDS] = {0, 0};
    agc_stats_out(stats_out, sv, none, false);
    HIP_TRY(hipSetDevice(ctx->device));
    if (n == 0) return agv_push_mixed_body(ctx, av, ag, d_places, 0, 0, nullptr, nullptr, nullptr, mv, d_result_out);
    if (int rc = agv_push_mixed_cached_run(ctx, av, ag, kc, d_places, n, u, d_rs49, d_keys, d_pk_inf, wire, mv, require,
                                           d_result_out, sv))
        return rc;
    return u ? agc_stats_dev(ctx, stats_out, sv, false) : 0;      // (no unknown lane: the cache was not asked)
}

// The list is on the host, the classes are on the device: the host refuses what push_mixed refuses, and with
// require > 0 agv_k_require reads the classes of the uploaded places -- its word is read before the cache or the object
// is touched.
static int agv_push_mixed_cached_host(ssa_ctx *ctx, ssa_aggverifier *av, ssa_aggregator *ag, ssa_keycache *kc,
                                      const uint32_t *places, size_t n, const uint8_t *rs49, const uint8_t *keys,
                                      const uint8_t *pk_inf, bool wire, const uint8_t *msgs, const uint64_t *msg_off,
                                      size_t msg_stride, size_t msg_len, size_t u, uint32_t require, uint64_t stats_out[8]) {
    if (int rc = agv_mixed_cached_args(ctx, av, ag, kc, wire, places, n, u, {msgs, msg_off, msg_stride, msg_len}, rs49, keys,
                                       require, false))
        return rc;
    if (int rc = check_host_offsets(msg_off, u)) return rc;
    size_t sentinels = 0;
    for (size_t i = 0; i < n; i++) {
        if (places[i] == SSA_AGGV_UNKNOWN) sentinels++;
        else if (places[i] >= ag->held) return SSA_ERR_ARG;
    }
    if (sentinels != u) return SSA_ERR_ARG;
    uint64_t sv[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    unsigned long long cnt[AGC_CNT_WORDS] = {0, 0};
    agc_stats_out(stats_out, sv, cnt, false);
    if (n == 0) {
        av->pushes++;
        return SSA_OK;
    }
    HostCall hc(ctx);
    const u32 *d_places = hc.in<u32>(ctx->agv_places, places, n * sizeof(u32));
    // (reserved here at the size the body asks for: the words do not move under it)
    if (hc.ok() && ctx->agv_misc.reserve(AGV_MISC_BYTES)) hc.rc = SSA_ERR_HIP;
    if (!hc.ok()) return hc.rc;
    if (require) {
        u32 below = 0, *d_flag = (u32 *)agv_misc(ctx, AGV_PUSH_FLAG);
        hc.step([&]() -> int {
            HIP_TRY(hipMemsetAsync(d_flag, 0, sizeof(u32), ctx->stream));
            if (int rc = timed_launch(ctx, "agv_k_require", [&] {
                    hipLaunchKernelGGL(agv_k_require, dim3(grid_for(n, 256)), dim3(256), 0, ctx->stream, d_places, n, ag->held,
                                       (const u8 *)ag->adm.p, require, d_flag);
                }))
                return rc;
            HIP_TRY(hipMemcpyAsync(&below, d_flag, sizeof below, hipMemcpyDeviceToHost, ctx->stream));
            HIP_TRY(hipStreamSynchronize(ctx->stream));
            return 0;
        });
        if (!hc.ok()) return hc.rc;
        if (below) return SSA_ERR_ARG;       // object, cache and info untouched
    }
    DevBatch b{};
    if (u) b = hc.lanes({rs49, keys, pk_inf, msgs, msg_off, msg_stride, msg_len}, u * 49, u, wire);
    u32 refused = 0, *d_result = (u32 *)agv_misc(ctx, AGV_RESULT);
    hc.copy_back(&refused, d_result, sizeof refused);
    if (u) (void)hc.out(ctx->agc_cnt, cnt, sizeof cnt, 48);      // (copied back behind the push, as a cached push's)
    const int rc = hc.finish([&] {
        return agv_push_mixed_cached_run(ctx, av, ag, kc, d_places, n, u, b.sigs, b.pks, b.pk_inf, wire,
                                         {b.msgs.msgs, b.msgs.off, msg_stride, msg_len}, require, d_result, sv);
    });
    if (rc) return rc;
    agc_stats_out(stats_out, sv, cnt, false);
    return refused ? SSA_ERR_HIP : SSA_OK;      // (cannot be: the list and the classes were checked above)
}

extern "C" int ssa_aggverifier_push_mixed_cached_device(ssa_ctx *ctx, ssa_aggverifier *av, ssa_aggregator *ag,
                                                        ssa_keycache *kc, const uint32_t *d_places, size_t n,
                                                        const uint8_t *d_rs49, const uint8_t *d_pks, const uint8_t *d_pk_inf,
                                                        const uint8_t *d_msgs, const uint64_t *d_msg_off, size_t msg_stride,
                                                        size_t msg_len, size_t u, uint32_t require, uint32_t *d_result_out,
                                                        uint64_t stats_out[8]) {
    return agv_push_mixed_cached_dev(ctx, av, ag, kc, d_places, n, d_rs49, d_pks, d_pk_inf, false,
                                     {d_msgs, d_msg_off, msg_stride, msg_len}, u, require, d_result_out, stats_out);
}

extern "C" int ssa_aggverifier_push_mixed_cached(ssa_ctx *ctx, ssa_aggverifier *av, ssa_aggregator *ag, ssa_keycache *kc,
                                                 const uint32_t *places, size_t n, const uint8_t *rs49, const uint8_t *pks,
                                                 const uint8_t *pk_inf, const uint8_t *msgs, const uint64_t *msg_off,
                                                 size_t msg_stride, size_t msg_len, size_t u, uint32_t require,
                                                 uint64_t stats_out[8]) {
    return agv_push_mixed_cached_host(ctx, av, ag, kc, places, n, rs49, pks, pk_inf, false, msgs, msg_off, msg_stride, msg_len,
                                      u, require, stats_out);
}

extern "C" int ssa_aggverifier_push_mixed_cached_wire_device(ssa_ctx *ctx, ssa_aggverifier *av, ssa_aggregator *ag,
                                                             ssa_keycache *kc, const uint32_t *d_places, size_t n,
                                                             const uint8_t *d_rs49, const uint8_t *d_pks49,
                                                             const uint8_t *d_msgs, const uint64_t *d_msg_off,
                                                             size_t msg_stride, size_t msg_len, size_t u, uint32_t require,
                                                             uint32_t *d_result_out, uint64_t stats_out[8]) {
    return agv_push_mixed_cached_dev(ctx, av, ag, kc, d_places, n, d_rs49, d_pks49, nullptr, true,
                                     {d_msgs, d_msg_off, msg_stride, msg_len}, u, require, d_result_out, stats_out);
}

extern "C" int ssa_aggverifier_push_mixed_cached_wire(ssa_ctx *ctx, ssa_aggverifier *av, ssa_aggregator *ag,
                                                      ssa_keycache *kc, const uint32_t *places, size_t n,
                                                      const uint8_t *rs49, const uint8_t *pks49, const uint8_t *msgs,
                                                      const uint64_t *msg_off, size_t msg_stride, size_t msg_len, size_t u,
                                                      uint32_t require, uint64_t stats_out[8]) {
    return agv_push_mixed_cached_host(ctx, av, ag, kc, places, n, rs49, pks49, nullptr, true, msgs, msg_off, msg_stride,
                                      msg_len, u, require, stats_out);
}

// ------------------------------------------------------------------ filtering half-aggregation through a key cache
// ssa_aggregate_valid_many with the statuses of ssa_verify_many_cached (affine keys) or ssa_verify_keyed_many_cached
// (130-byte records: d_keyed, and b holds the messages alone) in place of the screen's, and the kept lanes' keys handed
// on.  Every message is hashed once: over all n lanes in front (affine), or slice by slice behind the slice's keys
// (records); either way the scalars of all n lanes stand in ctx->ws_h and the raw digests in ctx->ag_dig when the slices
// are through.  Nothing between the hash and the gathers writes either: with ready hashes neither msm_run_one nor the
// exact kernels hash, the cache slice works in the dd_*, kc_* and ky_* buffers, ssa_k_keyset_build writes rows of the
// cache or ctx->ws_tab, and the re-check gather copies scalars into ctx->scr_in.  Both are reserved for n lanes before
// the first slice, so no later reserve of a slice's size moves them.
// The synchronisations of the slices (ssa_verify_many_cached_device has the count) and one for |K|.
// The status half, which the cached pushes of the streaming aggregator share (section 31): the hash and the n statuses
// at *d_status_io (nullptr: a buffer of the context, handed back there).
static int avc_status(ssa_ctx *ctx, ssa_keycache *kc, const DevBatch &b, const u8 *d_keyed, size_t n, u8 **d_status_io,
                      uint64_t *stats_out) {
    HIP_TRY(hipSetDevice(ctx->device));
    u8 *d_status = *d_status_io = ag_status_buf(ctx, *d_status_io, n);
    if (!d_status) return SSA_ERR_HIP;
    if (d_keyed) {
        if (ctx->ws_h.reserve(n * 32) || ctx->ag_dig.reserve(n * 32)) return SSA_ERR_HIP;
        return ssa_internal_screen_keyed_hashed(ctx, kc, d_keyed, b.msgs, n, (uint64_t *)ctx->ws_h.p, (uint8_t *)ctx->ag_dig.p,
                                                d_status, stats_out);
    }
    const u8 *d_sigs = b.sigs;
    if (int rc = ag_transcript_front(ctx, nullptr, &d_sigs, b.pks, b.msgs, n, true, nullptr, 1)) return rc;
    return ssa_internal_screen_many_hashed(ctx, kc, b, n, (const uint64_t *)ctx->ws_h.p, d_status, stats_out);
}

static int avc_run(ssa_ctx *ctx, ssa_keycache *kc, const DevBatch &b, const u8 *d_keyed, size_t n, u8 *d_agg_out,
                   u32 *d_kept_out, uint64_t *n_kept_out, u8 *d_status_out, u8 *d_keys_out, u8 *d_inf_out,
                   uint64_t *stats_out) {
    u8 *d_status = d_status_out;
    if (int rc = avc_status(ctx, kc, b, d_keyed, n, &d_status, stats_out)) return rc;
    // the kept lanes' keys as the caller gave them, and zeros up to the capacity of n lanes (the kernel writes both)
    const auto gather_keys = [&](size_t m) {
        if (!d_keys_out && !d_inf_out) return 0;
        const u32 width = d_keyed ? 49u : 96u;
        return timed_launch(ctx, "av_k_gather_keys", [&] {
            if (d_keys_out)
                hipLaunchKernelGGL(av_k_gather_keys, dim3(grid_for((n * width + 3) / 4, 256)), dim3(256), 0, ctx->stream,
                                   d_keyed ? d_keyed : b.pks, d_keyed ? 130u : 96u, width, (const u32 *)d_kept_out, m, n,
                                   d_keys_out);
            if (d_inf_out)
                hipLaunchKernelGGL(av_k_gather_keys, dim3(grid_for((n + 3) / 4, 256)), dim3(256), 0, ctx->stream, b.pk_inf, 1u,
                                   1u, (const u32 *)d_kept_out, m, n, d_inf_out);
        });
    };
    return d_keyed ? av_finish_kept(ctx, d_status, n, d_keyed, 130, 49, d_agg_out, d_kept_out, n_kept_out, gather_keys)
                   : av_finish_kept(ctx, d_status, n, b.sigs, 81, 0, d_agg_out, d_kept_out, n_kept_out, gather_keys);
}

// arguments of all four forms, before anything is written: in0, in1 = the inputs that must not be null when n != 0
static int avc_check_args(const ssa_ctx *ctx, const ssa_keycache *kc, bool keyed, const void *in0, const void *in1,
                          const MsgView &mv, size_t n, const void *agg_out, const void *kept_out, uint64_t *n_kept_out,
                          uint64_t *stats_out) {
    if (int rc = agc_check_cache(ctx, kc, keyed)) return rc;
    if (!agg_out || !kept_out || !n_kept_out || (n && (!in0 || !in1))) return SSA_ERR_ARG;
    if (int rc = agg_check_args(ctx, mv, n)) return rc;
    *n_kept_out = 0;
    if (stats_out) std::memset(stats_out, 0, 12 * sizeof(uint64_t));
    return 0;
}

extern "C" int ssa_aggregate_valid_many_cached_device(ssa_ctx *ctx, ssa_keycache *kc, const uint8_t *d_sigs,
                                                      const uint8_t *d_pks, const uint8_t *d_pk_inf, const uint8_t *d_msgs,
                                                      const uint64_t *d_msg_off, size_t msg_stride, size_t msg_len, size_t n,
                                                      uint8_t *d_agg_out, uint32_t *d_kept_out, uint64_t *n_kept_out,
                                                      uint8_t *d_status_out, uint8_t *d_pks_out, uint8_t *d_pk_inf_out,
                                                      uint64_t stats_out[12]) {
    const DevBatch b{d_sigs, d_pks, d_pk_inf, {d_msgs, d_msg_off, msg_stride, msg_len}};
    if (int rc = avc_check_args(ctx, kc, false, d_sigs, d_pks, b.msgs, n, d_agg_out, d_kept_out, n_kept_out, stats_out)) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    if (n == 0) {
        HIP_TRY(hipMemsetAsync(d_agg_out, 0, 32, ctx->stream));
        return SSA_OK;
    }
    return avc_run(ctx, kc, b, nullptr, n, d_agg_out, d_kept_out, n_kept_out, d_status_out, d_pks_out, d_pk_inf_out, stats_out);
}

extern "C" int ssa_aggregate_valid_keyed_many_cached_device(ssa_ctx *ctx, ssa_keycache *kc, const uint8_t *d_keyed,
                                                            const uint8_t *d_msgs, const uint64_t *d_msg_off,
                                                            size_t msg_stride, size_t msg_len, size_t n, uint8_t *d_agg_out,
                                                            uint32_t *d_kept_out, uint64_t *n_kept_out, uint8_t *d_status_out,
                                                            uint8_t *d_keys49_out, uint64_t stats_out[12]) {
    const DevBatch b{nullptr, nullptr, nullptr, {d_msgs, d_msg_off, msg_stride, msg_len}};
    if (int rc = avc_check_args(ctx, kc, true, d_keyed, d_keyed, b.msgs, n, d_agg_out, d_kept_out, n_kept_out, stats_out)) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    if (n == 0) {
        HIP_TRY(hipMemsetAsync(d_agg_out, 0, 32, ctx->stream));
        return SSA_OK;
    }
    return avc_run(ctx, kc, b, d_keyed, n, d_agg_out, d_kept_out, n_kept_out, d_status_out, d_keys49_out, nullptr, stats_out);
}

extern "C" int ssa_aggregate_valid_many_cached(ssa_ctx *ctx, ssa_keycache *kc, const uint8_t *sigs, const uint8_t *pks,
                                               const uint8_t *pk_inf, const uint8_t *msgs, const uint64_t *msg_off,
                                               size_t msg_stride, size_t msg_len, size_t n, uint8_t *agg_out,
                                               uint32_t *kept_out, uint64_t *n_kept_out, uint8_t *status_out, uint8_t *pks_out,
                                               uint8_t *pk_inf_out, uint64_t stats_out[12]) {
    if (int rc = avc_check_args(ctx, kc, false, sigs, pks, {msgs, msg_off, msg_stride, msg_len}, n, agg_out, kept_out,
                                n_kept_out, nullptr))
        return rc;
    if (int rc = check_host_offsets(msg_off, n)) return rc;
    if (stats_out) std::memset(stats_out, 0, 12 * sizeof(uint64_t));
    if (n == 0) {
        std::memset(agg_out, 0, 32);
        return SSA_OK;
    }
    HostCall hc(ctx);
    const DevBatch b = hc.lanes({sigs, pks, pk_inf, msgs, msg_off, msg_stride, msg_len}, n * 81, n);
    u8 *d_agg = hc.out(ctx->st_aux, agg_out, SSA_AGGREGATE_LENGTH(n), 16);
    u32 *d_kept = (u32 *)hc.out(ctx->st_aux2, kept_out, n * sizeof(u32));
    u8 *d_status = hc.out(ctx->st_status, status_out, n, 16);
    u8 *d_pks_out = pks_out ? hc.out(ctx->avc_keys, pks_out, n * 96) : nullptr;
    u8 *d_inf_out = pk_inf_out ? hc.out(ctx->avc_inf, pk_inf_out, n, 16) : nullptr;
    return hc.finish([&] {
        return avc_run(ctx, kc, b, nullptr, n, d_agg, d_kept, n_kept_out, d_status, d_pks_out, d_inf_out, stats_out);
    });
}

extern "C" int ssa_aggregate_valid_keyed_many_cached(ssa_ctx *ctx, ssa_keycache *kc, const uint8_t *keyed, const uint8_t *msgs,
                                                     const uint64_t *msg_off, size_t msg_stride, size_t msg_len, size_t n,
                                                     uint8_t *agg_out, uint32_t *kept_out, uint64_t *n_kept_out,
                                                     uint8_t *status_out, uint8_t *keys49_out, uint64_t stats_out[12]) {
    if (int rc = avc_check_args(ctx, kc, true, keyed, keyed, {msgs, msg_off, msg_stride, msg_len}, n, agg_out, kept_out,
                                n_kept_out, nullptr))
        return rc;
    if (int rc = check_host_offsets(msg_off, n)) return rc;
    if (stats_out) std::memset(stats_out, 0, 12 * sizeof(uint64_t));
    if (n == 0) {
        std::memset(agg_out, 0, 32);
        return SSA_OK;
    }
    HostCall hc(ctx);
    const u8 *d_keyed = hc.in(ctx->st_keyed, keyed, n * 130);
    const MsgView mv = hc.msgs(msgs, msg_off, msg_stride, msg_len, n);
    u8 *d_agg = hc.out(ctx->st_aux, agg_out, SSA_AGGREGATE_LENGTH(n), 16);
    u32 *d_kept = (u32 *)hc.out(ctx->st_aux2, kept_out, n * sizeof(u32));
    u8 *d_status = hc.out(ctx->st_status, status_out, n, 16);
    u8 *d_keys_out = keys49_out ? hc.out(ctx->avc_keys, keys49_out, n * 49, 16) : nullptr;
    return hc.finish([&] {
        return avc_run(ctx, kc, {nullptr, nullptr, nullptr, mv}, d_keyed, n, d_agg, d_kept, n_kept_out, d_status, d_keys_out,
                       nullptr, stats_out);
    });
}

// ---- the streaming aggregator's admission through a key cache: the status half of avc_run, then
// the tail of every push (agx_admit) in place of the kept lanes' transcript, fold and key gather.
// arguments of all four forms, before anything is written, enqueued or counted
static int agx_push_cached_args(const ssa_ctx *ctx, const ssa_aggregator *ag, const ssa_keycache *kc, bool keyed,
                                const void *in0, const void *in1, const MsgView &mv, size_t n, uint64_t *n_kept_out,
                                uint64_t *stats_out) {
    if (int rc = agc_check_cache(ctx, kc, keyed)) return rc;
    if (int rc = agx_push_args(ctx, ag, mv, n, 0, in0, in1, n_kept_out, keyed)) return rc;
    *n_kept_out = 0;
    if (stats_out) std::memset(stats_out, 0, 12 * sizeof(uint64_t));
    return 0;
}

// d_keyed: the records (then b holds the messages alone), or nullptr and b the affine lanes.  n >= 1.
static int agx_push_cached_run(ssa_ctx *ctx, ssa_aggregator *ag, ssa_keycache *kc, const DevBatch &b, const u8 *d_keyed,
                               size_t n, u8 *d_status_out, uint64_t *n_kept_out, uint64_t *stats_out) {
    u8 *d_status = d_status_out;
    if (int rc = avc_status(ctx, kc, b, d_keyed, n, &d_status, stats_out)) return rc;
    return d_keyed ? agx_admit(ctx, ag, d_status, n, d_keyed, 130, 49, SSA_ADM_KEY_CHECKED, n_kept_out)
                   : agx_admit(ctx, ag, d_status, n, b.sigs, 81, 0, SSA_ADM_KEY_CHECKED, n_kept_out);
}

extern "C" int ssa_aggregator_push_cached_device(ssa_ctx *ctx, ssa_aggregator *ag, ssa_keycache *kc, const uint8_t *d_sigs,
                                                 const uint8_t *d_pks, const uint8_t *d_pk_inf, const uint8_t *d_msgs,
                                                 const uint64_t *d_msg_off, size_t msg_stride, size_t msg_len, size_t n,
                                                 uint8_t *d_status_out, uint64_t *n_kept_out, uint64_t stats_out[12]) {
    const DevBatch b{d_sigs, d_pks, d_pk_inf, {d_msgs, d_msg_off, msg_stride, msg_len}};
    if (int rc = agx_push_cached_args(ctx, ag, kc, false, d_sigs, d_pks, b.msgs, n, n_kept_out, stats_out)) return rc;
    if (n == 0) {
        ag->pushes++;
        return SSA_OK;
    }
    return agx_push_cached_run(ctx, ag, kc, b, nullptr, n, d_status_out, n_kept_out, stats_out);
}

extern "C" int ssa_aggregator_push_keyed_cached_device(ssa_ctx *ctx, ssa_aggregator *ag, ssa_keycache *kc,
                                                       const uint8_t *d_keyed, const uint8_t *d_msgs,
                                                       const uint64_t *d_msg_off, size_t msg_stride, size_t msg_len, size_t n,
                                                       uint8_t *d_status_out, uint64_t *n_kept_out, uint64_t stats_out[12]) {
    const DevBatch b{nullptr, nullptr, nullptr, {d_msgs, d_msg_off, msg_stride, msg_len}};
    if (int rc = agx_push_cached_args(ctx, ag, kc, true, d_keyed, d_keyed, b.msgs, n, n_kept_out, stats_out)) return rc;
    if (n == 0) {
        ag->pushes++;
        return SSA_OK;
    }
    return agx_push_cached_run(ctx, ag, kc, b, d_keyed, n, d_status_out, n_kept_out, stats_out);
}

extern "C" int ssa_aggregator_push_cached(ssa_ctx *ctx, ssa_aggregator *ag, ssa_keycache *kc, const uint8_t *sigs,
                                          const uint8_t *pks, const uint8_t *pk_inf, const uint8_t *msgs,
                                          const uint64_t *msg_off, size_t msg_stride, size_t msg_len, size_t n,
                                          uint8_t *status_out, uint64_t *n_kept_out, uint64_t stats_out[12]) {
    if (int rc = agx_push_cached_args(ctx, ag, kc, false, sigs, pks, {msgs, msg_off, msg_stride, msg_len}, n, n_kept_out,
                                      nullptr))
        return rc;
    if (int rc = check_host_offsets(msg_off, n)) return rc;
    if (stats_out) std::memset(stats_out, 0, 12 * sizeof(uint64_t));
    if (n == 0) {
        ag->pushes++;
        return SSA_OK;
    }
    HostCall hc(ctx);
    const DevBatch b = hc.lanes({sigs, pks, pk_inf, msgs, msg_off, msg_stride, msg_len}, n * 81, n);
    u8 *d_status = hc.out(ctx->st_status, status_out, n, 16);
    return hc.finish([&] { return agx_push_cached_run(ctx, ag, kc, b, nullptr, n, d_status, n_kept_out, stats_out); });
}

extern "C" int ssa_aggregator_push_keyed_cached(ssa_ctx *ctx, ssa_aggregator *ag, ssa_keycache *kc, const uint8_t *keyed,
                                                const uint8_t *msgs, const uint64_t *msg_off, size_t msg_stride,
                                                size_t msg_len, size_t n, uint8_t *status_out, uint64_t *n_kept_out,
                                                uint64_t stats_out[12]) {
    if (int rc = agx_push_cached_args(ctx, ag, kc, true, keyed, keyed, {msgs, msg_off, msg_stride, msg_len}, n, n_kept_out,
                                      nullptr))
        return rc;
    if (int rc = check_host_offsets(msg_off, n)) return rc;
    if (stats_out) std::memset(stats_out, 0, 12 * sizeof(uint64_t));
    if (n == 0) {
        ag->pushes++;
        return SSA_OK;
    }
    HostCall hc(ctx);
    const u8 *d_keyed = hc.in(ctx->st_keyed, keyed, n * 130);
    const MsgView mv = hc.msgs(msgs, msg_off, msg_stride, msg_len, n);
    u8 *d_status = hc.out(ctx->st_status, status_out, n, 16);
    return hc.finish([&] {
        return agx_push_cached_run(ctx, ag, kc, {nullptr, nullptr, nullptr, mv}, d_keyed, n, d_status, n_kept_out, stats_out);
    });
}

// tests: the plan of a call from its counts alone (no device): out[0..4) = lanes, tree passes, groups, descriptors in
// all; then six words per group (first aggregate, aggregates, first lane, lanes, padded segment, 1 = bucket path); then
// per pass its number of descriptors and four words each (first node, nodes, slot, n_j of a top workgroup or 0).
// Returns the words the plan takes (out receives them only if out_words is enough), or SSA_ERR_ARG.
extern "C" int64_t ssa_debug_aggregates_plan(const uint64_t *counts, size_t k, size_t msm_slice, size_t small_max,
                                             uint64_t *out, size_t out_words) {
    if ((k && !counts) || k > SSA_MAX_BATCH) return SSA_ERR_ARG;
    AgPlan pl;
    if (int rc = ag_plan(counts, k, msm_slice, small_max, pl)) return rc;
    std::vector<uint64_t> w{pl.first[k], pl.passes.size(), pl.groups.size(), 0};
    for (const AgGroup &g : pl.groups) w.insert(w.end(), {g.agg0, g.aggs, g.lane0, g.lanes, g.seg_lanes, g.bucket});
    for (const auto &pass : pl.passes) {
        w[3] += pass.size();
        w.push_back(pass.size());
        for (const AgTreeDesc &d : pass) w.insert(w.end(), {d.first, d.count, d.slot, d.top_n});
    }
    if (out && out_words >= w.size()) std::memcpy(out, w.data(), w.size() * sizeof(uint64_t));
    return (int64_t)w.size();
}

// tests: the partial offsets of the producer's fold (ssa_aggregates_many) from the counts alone: out[0] = the partials in
// all, out[1 .. k + 2) = pfirst.  Returns the k + 2 words it takes (out receives them only if out_words is enough).
extern "C" int64_t ssa_debug_aggregates_fold_plan(const uint64_t *counts, size_t k, uint64_t *out, size_t out_words) {
    if ((k && !counts) || k > SSA_MAX_BATCH) return SSA_ERR_ARG;
    AgPlan pl;
    if (int rc = ag_plan(counts, k, SSA_MAX_BATCH, 0, pl)) return rc;
    if (out && out_words >= k + 2) {
        out[0] = pl.pfirst[k];
        for (size_t j = 0; j <= k; j++) out[1 + j] = pl.pfirst[j];
    }
    return (int64_t)(k + 2);
}

// tests: the coefficients of all N lanes as ssa_verify_aggregates_many derives them -> N x 16 bytes
extern "C" int ssa_debug_aggregates_many_coeffs(ssa_ctx *ctx, const uint8_t *aggs, const uint64_t *counts, size_t k,
                                                const uint8_t *pks, const uint8_t *msgs, const uint64_t *msg_off,
                                                size_t msg_stride, size_t msg_len, uint8_t *coeffs16_out) {
    AgPlan pl;
    size_t n = 0;
    if (int rc = agm_check_args(ctx, aggs, counts, k, pks, {msgs, msg_off, msg_stride, msg_len}, coeffs16_out, pl, &n)) return rc;
    if (int rc = check_host_offsets(msg_off, n)) return rc;
    if (n == 0) return 0;
    HostCall hc(ctx);
    const u8 *d_aggs = hc.in(ctx->st_sigs, aggs, 49 * n + 32 * k), *d_pks = hc.in(ctx->st_pks, pks, n * 96);
    const MsgView mv = hc.msgs(msgs, msg_off, msg_stride, msg_len, n);
    (void)hc.out(ctx->ag_coeffs, coeffs16_out, n * 16);
    return hc.finish([&] { return agm_run(ctx, pl, d_aggs, k, d_pks, nullptr, mv, n, nullptr); });
}

// tests: the coefficients a_i of an aggregate's R's (n x 49 bytes), keys and messages -> n x 16 bytes
extern "C" int ssa_debug_aggregate_coeffs(ssa_ctx *ctx, const uint8_t *rs49, const uint8_t *pks, const uint8_t *pk_inf,
                                          const uint8_t *msgs, const uint64_t *msg_off, size_t msg_stride, size_t msg_len,
                                          size_t n, uint8_t *coeffs16_out) {
    (void)pk_inf;         // (the transcript reads the key bytes, not the flag)
    if (!ctx || (n && (!rs49 || !pks || !coeffs16_out))) return SSA_ERR_ARG;
    if (int rc = agg_check_args(ctx, {msgs, msg_off, msg_stride, msg_len}, n)) return rc;
    if (int rc = check_host_offsets(msg_off, n)) return rc;
    if (n == 0) return 0;
    HostCall hc(ctx);
    const u8 *d_rs = hc.in(ctx->st_sigs, rs49, n * 49), *d_pks = hc.in(ctx->st_pks, pks, n * 96);
    const MsgView mv = hc.msgs(msgs, msg_off, msg_stride, msg_len, n);
    (void)hc.out(ctx->ag_coeffs, coeffs16_out, n * 16);
    // (n R's side by side are the wire form of one aggregate, short of its scalar)
    return hc.finish([&] { return ag_transcript(ctx, d_rs, nullptr, d_pks, mv, n, false, nullptr, 1, ag_uniform_passes(n)); });
}

// ------------------------------------------------------------------ probes
extern "C" int ssa_debug_corrupt_table_builds(int n) {
    if (n < 0) return SSA_ERR_ARG;
    g_corrupt_builds.store(n);
    return 0;
}

extern "C" int ssa_debug_fault_after_chunk(ssa_ctx *ctx, int chunk) {
    if (!ctx) return SSA_ERR_ARG;
    ctx->fault_after_chunk = chunk;
    return 0;
}

// Tests of "a call's result does not depend on what its workspaces held before" ("What a call may assume
// about its workspaces"): every byte up to `cap` of every DevBuf of the context and of its twin becomes `byte`, on each
// one's own stream and behind whatever is queued there, and every HostBuf on the host.  The one listed buffer left out
// is ctab: it is no workspace but the constant-time signer's table, built once and trusted from then on (ctab_ready);
// filling it would make every later constant-time signature wrong by design.  No other listed buffer is read by a call
// that did not write it first (rng_seed, rng_scratch and dv_recs are wiped after each call, not kept).  What is not in
// the list -- the comb, d_params, key sets, key caches, signer sets, streaming aggregators and aggregate verifiers -- is not touched.
extern "C" int ssa_debug_poison_workspaces(ssa_ctx *ctx, int byte) {
    if (!ctx || byte < 0 || byte > 255) return SSA_ERR_ARG;
    HIP_TRY(hipSetDevice(ctx->device));
    for (ssa_ctx *c : {ctx, ctx->twin}) {
        if (!c) continue;
        // (every public call returns with its side streams joined to c->stream or drained; they are waited for all the
        //  same, so that the fill can never race a copy or a hash launch still reading a staging buffer)
        HIP_TRY(hipStreamSynchronize(c->copy_stream));
        for (auto &hs : c->hash_stream) HIP_TRY(hipStreamSynchronize(hs));
        HIP_TRY(hipStreamSynchronize(c->stream));
        hipError_t err = hipSuccess;
        for_each_devbuf(c, [&](DevBuf &b) {
            if (&b == &c->ctab || !b.p || !b.cap || err != hipSuccess) return;
            err = hipMemsetAsync(b.p, byte, b.cap, c->stream);
        });
        HIP_TRY(err);
        HIP_TRY(hipStreamSynchronize(c->stream));
        for_each_hostbuf(c, [&](HostBuf &b) {
            if (b.p && b.cap) std::memset(b.p, byte, b.cap);
        });
    }
    return 0;
}

extern "C" int ssa_debug_arith(ssa_ctx *ctx, int op, const uint64_t *a, const uint64_t *b, size_t n,
                               size_t a_stride, size_t b_stride, uint64_t *out, size_t out_stride) {
    if (!ctx || !a || !out || n == 0 || op < 0 || op > 18) return SSA_ERR_ARG;
    if ((op == 0 || op == 3 || op == 4 || op == 5 || (op >= 7 && op != 18)) && !b) return SSA_ERR_ARG;
    if (op == 18 && (a_stride < 2 || out_stride < 6)) return SSA_ERR_ARG;
    if (op >= 15 && op <= 17) {
        // the generated loops take their count from a[19] through v_readfirstlane (wave-uniform) and count DOWN to
        // zero: n == 0 would wrap to 2^32 iterations, rows that disagree would silently run lane 0's count
        if (a_stride < 20 || b_stride < 12 || out_stride < 19) return SSA_ERR_ARG;
        if (op != 16)
            for (size_t i = 0; i < n; i++)
                if (a[i * a_stride + 19] == 0 || a[i * a_stride + 19] > 64 || a[i * a_stride + 19] != a[19])
                    return SSA_ERR_ARG;
    }
    HostCall hc(ctx);
    const u64 *da = hc.in<u64>(ctx->st_aux, a, n * a_stride * 8), *db = b ? hc.in<u64>(ctx->st_aux2, b, n * b_stride * 8) : nullptr;
    u64 *d_out = (u64 *)hc.out(ctx->st_status, out, n * out_stride * 8);
    return hc.finish([&] {
        HIP_TRY(hipMemsetAsync(d_out, 0, n * out_stride * 8, ctx->stream));
        if (op == 7) {
            hipLaunchKernelGGL(ssa_k_debug_coop, dim3((unsigned)n), dim3(64), 0, ctx->stream, da, db, n, a_stride, b_stride,
                               d_out, out_stride);
        } else if (op == 4 || (op >= 15 && op <= 17)) {
            if (ctx->ws_tab.reserve(n * (size_t)(PTAB_ENTRIES * PTAB_ENTRY_U64) * sizeof(u64))) return SSA_ERR_HIP;
            hipLaunchKernelGGL(ssa_k_debug_mul, dim3(grid_for(n, 64)), dim3(64), 0, ctx->stream, op, da, db, n, a_stride,
                               b_stride, (u64 *)ctx->ws_tab.p, d_out, out_stride);
        } else {
            hipLaunchKernelGGL(ssa_k_debug, dim3(grid_for(n, 64)), dim3(64), 0, ctx->stream, op, da, db, n, a_stride,
                               b_stride, d_out, out_stride);
        }
        HIP_TRY(hipGetLastError());
        return 0;
    });
}

extern "C" int ssa_bench_fpmul(ssa_ctx *ctx, int variant, double *fpmul_per_s) {
    if (!ctx || !fpmul_per_s) return SSA_ERR_ARG;
    HIP_TRY(hipSetDevice(ctx->device));
    if (variant >= 10 && variant <= 13) {   // cooperative point-operation chain: result = operations per second
        if (ctx->st_aux.reserve(64)) return SSA_ERR_HIP;
        hipEvent_t c0, c1;
        HIP_TRY(hipEventCreate(&c0));
        HIP_TRY(hipEventCreate(&c1));
        const int n_ops = 2000;
        for (int rep = 0; rep < 2; rep++) {
            HIP_TRY(hipEventRecord(c0, ctx->stream));
            hipLaunchKernelGGL(ssa_k_coop_bench, dim3(1), dim3(64), 0, ctx->stream, variant - 10, n_ops,
                               (u64 *)ctx->st_aux.p);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipEventRecord(c1, ctx->stream));
            HIP_TRY(hipEventSynchronize(c1));
        }
        float cms = 0;
        HIP_TRY(hipEventElapsedTime(&cms, c0, c1));
        (void)hipEventDestroy(c0);
        (void)hipEventDestroy(c1);
        *fpmul_per_s = n_ops / (cms * 1e-3);
        return 0;
    }
    const unsigned blocks = 256 * 16, threads = 256;
    const int iters = 2000;
    if (ctx->st_aux.reserve((size_t)blocks * threads * 8)) return SSA_ERR_HIP;
    hipEvent_t e0, e1;
    HIP_TRY(hipEventCreate(&e0));
    HIP_TRY(hipEventCreate(&e1));
    double muls_per_thread = 0;
    for (int rep = 0; rep < 2; rep++) {  // first repetition warms up
        HIP_TRY(hipEventRecord(e0, ctx->stream));
        switch (variant) {
            case 0:
                hipLaunchKernelGGL(ssa_k_fpmul_bench<1>, dim3(blocks), dim3(threads), 0, ctx->stream,
                                   (u64 *)ctx->st_aux.p, 0x1234567ull, iters);
                muls_per_thread = 2.0 * 1 * iters;
                break;
            case 1:
                hipLaunchKernelGGL(ssa_k_fpmul_bench<4>, dim3(blocks), dim3(threads), 0, ctx->stream,
                                   (u64 *)ctx->st_aux.p, 0x1234567ull, iters);
                muls_per_thread = 2.0 * 4 * iters;
                break;
            case 2:
                hipLaunchKernelGGL(ssa_k_fpmul_bench<8>, dim3(blocks), dim3(threads), 0, ctx->stream,
                                   (u64 *)ctx->st_aux.p, 0x1234567ull, iters);
                muls_per_thread = 2.0 * 8 * iters;
                break;
            case 4:
                hipLaunchKernelGGL(ssa_k_fpsqr_bench<0>, dim3(blocks), dim3(threads), 0, ctx->stream,
                                   (u64 *)ctx->st_aux.p, 0x1234567ull, iters / 4);
                muls_per_thread = 16.0 * (iters / 4);
                break;
            case 5:
                hipLaunchKernelGGL(ssa_k_fpsqr_bench<1>, dim3(blocks), dim3(threads), 0, ctx->stream,
                                   (u64 *)ctx->st_aux.p, 0x1234567ull, iters / 4);
                muls_per_thread = 16.0 * (iters / 4);
                break;
            default:
                hipLaunchKernelGGL(ssa_k_f6mul_bench, dim3(blocks), dim3(threads), 0, ctx->stream,
                                   (u64 *)ctx->st_aux.p, 0x1234567ull, iters / 4);
                muls_per_thread = (36.0 + 21.0) * (iters / 4);
                break;
        }
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(e1, ctx->stream));
        HIP_TRY(hipEventSynchronize(e1));
    }
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    *fpmul_per_s = muls_per_thread * (double)blocks * threads / (ms * 1e-3);
    return 0;
}

#ifdef SSA_WAVE_TIMES
extern "C" int ssa_debug_phase_times(unsigned long long *out, size_t n_waves) {
    if (n_waves > ssa::SSA_WAVE_TIMES_MAX) n_waves = ssa::SSA_WAVE_TIMES_MAX;
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(ssa::g_phase_times), 4 * n_waves * sizeof(unsigned long long)) == hipSuccess ? 0 : -1;
}
// diagnostic build only: (start, end, hardware id) of every wave of the LAST ssa_k_verify launch, wall_clock64 ticks (100 MHz)
extern "C" int ssa_debug_wave_times(unsigned long long *out, size_t n_waves) {
    if (n_waves > ssa::SSA_WAVE_TIMES_MAX) n_waves = ssa::SSA_WAVE_TIMES_MAX;
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(ssa::g_wave_times), 3 * n_waves * sizeof(unsigned long long)) == hipSuccess ? 0 : -1;
}
#endif

