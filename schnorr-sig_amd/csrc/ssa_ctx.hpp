// Internal: context layout and helpers shared by the translation units of the library
// (ssa_api.hip: per-lane verification path; ssa_msm.hip: MSM-form batch verification).
#pragma once
#include "../../include/schnorr_sig_amd.h"
#include "ssa_kernels.hpp"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <mutex>
#include <string>
#include <thread>
#include <utility>
#include <vector>

using namespace ssa;

// a library does not write to stderr on its own: the failing call is reported only when SSA_DEBUG is set
static inline bool ssa_debug_enabled() {
    static const bool on = std::getenv("SSA_DEBUG") != nullptr;
    return on;
}
#define HIP_TRY(expr)                                                                    \
    do {                                                                                 \
        hipError_t err__ = (expr);                                                       \
        if (err__ != hipSuccess) {                                                       \
            if (ssa_debug_enabled())                                                     \
                std::fprintf(stderr, "[schnorr_sig_amd] %s failed: %s (%s:%d)\n", #expr, \
                             hipGetErrorString(err__), __FILE__, __LINE__);              \
            return SSA_ERR_HIP;                                                          \
        }                                                                                \
    } while (0)

struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    int reserve(size_t bytes) {
        if (bytes <= cap) return 0;
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
        size_t want = bytes + bytes / 8 + 256;
        if (hipMalloc(&p, want) != hipSuccess) return SSA_ERR_HIP;
        cap = want;
        return 0;
    }
    // exactly `bytes` (rounded up to 256), for a buffer whose final size is known when it is made: no room to grow into
    int reserve_exact(size_t bytes) {
        release();
        const size_t want = (bytes + 255) & ~(size_t)255;
        if (hipMalloc(&p, want) != hipSuccess) {
            p = nullptr;
            return SSA_ERR_HIP;
        }
        cap = want;
        return 0;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
};

// page-locked HOST memory owned by the library (hipHostMalloc): what the DMA engines read and write in the host-buffer entry
// points.  The caller's memory itself is never registered with the runtime (see pipelined_upload_hash).
struct HostBuf {
    void *p = nullptr;
    size_t cap = 0;
    int reserve(size_t bytes) {
        if (bytes <= cap) return 0;
        if (p) (void)hipHostFree(p);
        p = nullptr;
        cap = 0;
        const size_t want = bytes + bytes / 8 + 4096;
        if (hipHostMalloc(&p, want, hipHostMallocDefault) != hipSuccess) {
            (void)hipGetLastError();
            p = nullptr;
            return SSA_ERR_HIP;
        }
        cap = want;
        return 0;
    }
    void release() {
        if (p) (void)hipHostFree(p);
        p = nullptr;
        cap = 0;
    }
};

// one entry of a timing key.  A call split over the two streams records ONE entry for its two
// launches of a kernel: start2 / stop2 are the second launch's, and the entry runs from the earlier start to the later stop
struct TimedLaunch {
    hipEvent_t start, stop;
    hipEvent_t start2 = nullptr, stop2 = nullptr;
};

// key dedup defaults: keyed route when u < ratio * lanes, without / with the subgroup check
constexpr double DEDUP_RATIO_NO_CHECK = 0.0, DEDUP_RATIO_CHECK = 1.0;
constexpr unsigned DEDUP_PROBE_BOUND = 128;

// Everything that configures HOW calls run on a context, and that its second set of streams must share: filled from the
// environment once, at ssa_ctx_create (ctx_read_env in ssa_api.hip: one line per variable), changed afterwards by the
// debug setters alone, and handed to the twin whole (ssa_internal_twin).  State of ONE context -- streams, events,
// buffers, handle lists, one-shot hooks, the comb geometry -- stays in ssa_ctx.
struct CtxKnobs {
    size_t pipeline_min_n = 1 << 17;          // host-buffer batches from this size on are uploaded in chunks
    unsigned pipeline_chunks = 8;             // SSA_PIPELINE_CHUNKS overrides (1 = off)
    // batches up to these sizes take the cooperative (waves-per-signature) kernel: measured crossovers without /
    // with the subgroup check (tools/mode_crossover.py); SSA_COOP_MAX_N overrides both
    size_t coop_max_n = 7680, coop_max_n_torsion = 10496;   // lane kernels: 3.5 / 5.4 ms flat up to 2^15 (round 2, window asm)
    size_t msm_small_max = 3072;  // MSM-form batches up to this size: one cooperative block per signature (measured
                                  // crossover with the bucket method: tools/msm_small_crossover.py; SSA_MSM_SMALL_MAX)
    // Workspace bound: the per-lane kernels run over slices of at most lane_slice lanes (2 KB of table + 32 B of scalar
    // each: 2.1 GB at 2^20), the MSM-form pipeline over slices of at most msm_slice signatures whose records are
    // combined like the shards of a multi-GPU batch.  SSA_LANE_SLICE / SSA_MSM_SLICE override (tests force small ones).
    size_t lane_slice = (size_t)1 << 20, msm_slice = (size_t)1 << 23;
    size_t agg_block = 0;         // lanes per block of the sliced and sharded half-aggregation; 0: the
                                  // largest power of two not above msm_slice.  SSA_AGG_BLOCK (tests); rounded down to a power of two
    bool msm_overlap = true;      // the h-independent half of msm_k_prepare runs under ssa_k_hash (SSA_MSM_OVERLAP=0: off)
    unsigned msm_tree_group = 16; // chunk sums added per cooperating wave and tree level (SSA_MSM_TREE_GROUP: 2..64)
    unsigned verify_block = 256;  // threads per block of ssa_k_verify (SSA_VERIFY_BLOCK overrides: 64/128/256)
    // the end game of ssa_k_verify (ssa_kernels.hpp "The end game of a launch"): the last generation of lanes runs in
    // tail_pieces pieces per ladder pass, only the last of which stand at the end of the grid
    unsigned verify_waves = 0;    // waves of ssa_k_verify resident at once on this device (occupancy x CUs x 4)
    unsigned tail_pieces = 5;     // SSA_TAIL_PIECES (0 or 1: off); launches of less than one generation have none
    unsigned tail_gens = 1;       // SSA_TAIL_GENS: tail groups, in generations of resident waves
    bool tail_uniform = false;    // SSA_TAIL_UNIFORM=1: equal pieces instead of 1/2, 1/4, 1/8, ...
    bool tail_reversed = false;   // SSA_TAIL_REVERSED=1 (tests): the end game's roles dealt from the end of the grid
    unsigned tail_min_main = 0;   // SSA_TAIL_MIN_MAIN: generations of ordinary workgroups a launch must have beside its tail
    unsigned tail_waves_override = 0;   // SSA_TAIL_WAVES: the tests' small "generation" (the end game on batches of thousands)
    bool timing = false;          // ssa_ctx_enable_timing
    // A one-slice call of the lane kernels as two UNEQUAL parts on the context's two streams: the
    // short part B = split_frac sixteenths of the lanes runs on the twin's stream, its verifier under the end of the long
    // part's hash and its ladder under the long part's first table builds; the long part ends alone, with the end game.
    // Measured (profiles/r30/README.md): 2/16 gains 0.1-0.9 ms at every size tried from 2^19 to 2^20 lanes (-0.43 ms at
    // 2^20) and loses at 2^18 and below; an end game of B's own costs what the split brings.
    size_t split_min = (size_t)1 << 19;   // SSA_SPLIT_MIN: one-slice calls of fewer lanes are not split
    unsigned split_frac = 2;      // SSA_SPLIT_FRAC: the short part's share in 1/16ths, 1..8 (0: no call is split)
    bool split_tail_b = false;    // SSA_SPLIT_TAIL_B=1: the short part runs with an end game of its own when it is long enough
    bool split_alone = true;      // SSA_SPLIT_ALONE=0: split also while the process has other contexts on the device (two
                                  //   contexts that each split their half of a batch lose 1.0-1.5 ms per batch)
    unsigned screen_segs = 0;     // segments per slice of the screened forms forced by ssa_debug_screen_segments (0 = automatic)
    // a slice takes the keyed route when u < dedup_ratio[subgroup check on] * lanes: the measured thresholds of DESIGN.md
    // section 14 (without the check the keyed route never paid, with it always but for all-distinct keys);
    // ssa_debug_dedup_config overrides both.  A lane probes at most dedup_probe_bound slots.
    double dedup_ratio[2] = {DEDUP_RATIO_NO_CHECK, DEDUP_RATIO_CHECK};
    unsigned dedup_probe_bound = DEDUP_PROBE_BOUND;
};

// Every DevBuf of a context, declared HERE and nowhere else: the members of ssa_ctx and for_each_devbuf (what
// ssa_ctx_destroy releases and ssa_ctx_info sums) both expand from this list.
#define SSA_CTX_DEVBUFS(X) \
    X(ws_h) X(ws_tab) X(ws_fail) \
    /* staging for the host-buffer entry points */ \
    X(st_sigs) X(st_pks) X(st_inf) X(st_msgs) X(st_off) X(st_status) X(st_aux) X(st_aux2) X(st_coeffs) \
    /* MSM-form batch verification (ssa_msm.hip) */ \
    X(msm_points) X(msm_scalars) X(msm_keys) X(msm_vals) X(msm_keys2) X(msm_vals2) X(msm_sort_tmp) X(msm_bounds) \
    X(msm_buckets) X(msm_chunks) X(msm_windows) X(msm_partials) X(msm_flags) X(msm_cnt) X(msm_cnt2) X(msm_ids) \
    X(msm_ids2) X(msm_comb_pts) X(msm_comb_lins) \
    X(msm_slice_recs)   /* one 24-word record per MSM slice */ \
    X(msm_sbuf)         /* the coefficients s_i between the two halves of the preparation (32 B per signature) */ \
    /* screened batch verification (ssa_msm.hip): the segment verdicts, the gathered lanes of \
       failing segments (inputs and challenge scalars), their statuses, and a scratch rejection counter */ \
    X(scr_ok) X(scr_in) X(scr_status) X(scr_fail) \
    /* ssa_verify_many_screened: per lane "cannot be screened" (from its key) and "re-check" \
       bytes, the re-check list (lane numbers), per-workgroup counts and offsets of the list, and three counters */ \
    X(scr_mask) X(scr_mark) X(scr_list) X(scr_blk) X(scr_cnt) \
    /* key dedup (ssa_dedup.hpp): the slot table, each lane's representative, the \
       representatives' numbers and list, each lane's key index, per-workgroup counts and offsets, two counters (lanes \
       at the probe bound, u), and the compacted keys, flags and key statuses.  The 16-multiple tables of the u keys \
       live in ws_tab. */ \
    X(dd_slots) X(dd_rep) X(dd_num) X(dd_reps) X(dd_idx) X(dd_blk) X(dd_stats) X(dd_pks) X(dd_inf) X(dd_kstatus) \
    /* key cache (ssa_keycache.hpp): per distinct key of the slice its cache row or miss number, \
       the misses' representative lanes, per-workgroup counts and offsets of the misses, and a cache row per lane */ \
    X(kc_found) X(kc_missrep) X(kc_blk) X(kc_lane_row) \
    /* KeyedSignature wire records (ssa_keyed.hpp): one slice of 130-byte records staged by the \
       host forms, and per lane of a slice the 81 signature bytes, the 96 key bytes and the pk_inf boolean */ \
    X(st_keyed) X(ky_sigs) X(ky_pks) X(ky_inf) \
    /* signing (ssa_sign.hip): the 4-bit comb table of the constant-time signer (98 KB, built at the first use) and \
       the intermediates of the keyed (130-byte) output */ \
    X(ctab) X(sg_sigs) X(sg_pks) \
    X(tc_out)           /* table self-check (ssa_selfcheck.hpp): failing rows, first failing row */ \
    X(kck_ws)           /* key-table self-check (ssa_keycheck.hpp): a bad flag per key and two lists of key numbers */ \
    X(dv_recs)          /* key derivation (ssa_derive.hpp): one record per parent, wiped after each call */ \
    /* device-drawn scalars (ssa_rng.hpp): the call's 44-byte seed and one slice of drawn scalars (both zeroed on the \
       stream after each call) */ \
    X(rng_seed) X(rng_scratch) \
    /* half-aggregation (ssa_aggregate.hpp): the aggregate's R's at stride 81, the raw challenge \
       digests, the tree's nodes (two buffers, passes alternate), the coefficients a_i, the fold's partial sums, a status \
       byte per lane, and one small block: MSM record and e_agg of the single calls */ \
    X(ag_sigs) X(ag_dig) X(ag_nodes) X(ag_nodes2) X(ag_coeffs) X(ag_partials) X(ag_status) X(ag_misc) \
    /* many aggregates in one call: the plan (prefix sums, then the tree's descriptors), each \
       lane's aggregate, one root per aggregate (the single calls': slot 0), and a padded group of the bucket path: its \
       inputs (R's, keys, flags, challenge scalars, coefficients) and its bytes (mask, re-check marks, segment verdicts, \
       right-hand scalars) */ \
    X(agm_plan) X(agm_map) X(agm_roots) X(agm_in) X(agm_bytes) \
    /* the producer of many aggregates: per aggregate its failing lanes and 256 - their smallest \
       nonzero status, and the results when the caller takes none */ \
    X(agp_acc) \
    /* filtering half-aggregation: per-workgroup counts and offsets of the kept lanes (the \
       length of the list behind them), and the kept lanes' signatures and raw digests side by side */ \
    X(av_blk) X(av_sigs) X(av_dig) \
    /* filtering half-aggregation through a key cache: the kept keys (49 or 96 bytes each) and \
       their pk_inf bytes as the host forms stage them */ \
    X(avc_keys) X(avc_inf) \
    /* aggregates through a key cache (ssa_aggcache.hpp): per lane of the CALL (not of a slice) \
       its key's status byte and, for wire keys, its 96 key bytes and pk_inf boolean; and the call's two counters */ \
    X(agc_kst) X(agc_pks) X(agc_inf) X(agc_cnt) \
    /* sliced and sharded half-aggregation: one 32-byte top per block of lanes, and one partial \
       scalar and one MSM record per slice of a shard */ \
    X(ags_tops) X(ags_parts) X(ags_recs) \
    /* the streaming aggregator (ssa_aggregator.hpp): the kept lanes of one push.  What the object \
       holds between calls is its own and not listed here */ \
    X(agx_kept) \
    /* removing lanes from a streaming aggregator: the staging of one piece of the move -- its \
       leaves, its scalars, its R's -- and the first place a mask changes.  Nothing lives in them between calls */ \
    X(agx_stage) X(agx_first) \
    /* a selection of held lanes: the staging of the gathered lanes -- leaves, scalars, R's, \
       keys, laid out as a piece of the move -- the flag word, the result word of the host forms and the bitmap of the \
       lanes held (cleared by every call that uses them, never assumed clean), the list as the host forms upload it, \
       and the byte mask remove_indices hands to the move */ \
    X(agx_sel_stage) X(agx_sel_bits) X(agx_sel_order) X(agx_sel_mask) \
    /* known lanes in the streaming aggregate verifier: a keep byte per lane of a mixed push, the \
       list of unknown positions (of a push) or places (of a finish), the place list as the host forms upload it, and \
       one small block: the flag words, the result word of the host forms, S and e_agg - S.  Nothing lives in them \
       between calls */ \
    X(agv_keep) X(agv_pos) X(agv_places) X(agv_misc) \
    /* the end game of ssa_k_verify, per tail group: finished pieces; parked accumulators + status (152 B per lane) */ \
    X(tail_done) X(tail_park)

// The page-locked buffers of a context, in the same way: the bounce buffers of the host-buffer entry points (one slice of
// inputs, 257 B + message per lane; the caller's coefficients of the MSM form; one slice of statuses) and the host copy of
// the device RNG's seed (wiped before the call returns)
#define SSA_CTX_HOSTBUFS(X) X(pin_in) X(pin_coeffs) X(pin_out) X(pin_seed)

struct ssa_ctx {
    int device = 0;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    hipStream_t copy_stream = nullptr;        // uploads of the host-buffer entry points, overlapped with the kernels
    hipEvent_t copy_done[8] = {};             // one per upload chunk
    hipStream_t hash_stream[2] = {};          // the chunks' hash launches alternate between two streams, so that the
    hipEvent_t hash_done[8] = {};             //   tail of one launch (a lane hashes for ~4 ms) overlaps the next
    hipEvent_t pipe_start = nullptr;          // everything queued on `stream` before a pipelined upload began
    hipEvent_t order_ev = nullptr;            // ssa_ctx_stream_release / _acquire
    hipEvent_t agm_plan_ev = nullptr;         // the last upload of agm_plan_host has left the host (created at the first use)
    std::vector<uint32_t> agm_plan_host;      // ssa_verify_aggregates_many: the plan as it is uploaded
    CtxKnobs knobs;
    DevParams *d_params = nullptr;
    u64 *d_gtab = nullptr;                    // the comb table for G: owned by gtab_share (one per device, generator and
    struct SharedGtab *gtab_share = nullptr;  //   geometry); its first word carries the geometry (ssa_kernels.hpp)
    uint32_t gtab_bits = 0;                   // window width of that table (16 / 20 / 22 / 24)
    uint64_t hbm_budget = 0;                  // bytes the speed-for-memory tables may take (comb for G, per-key combs)
    DevParams h_params;                       // host copy of the blob the context was created from (derived flags set)
    ssa_ctx *twin = nullptr;                  // second set of streams and workspaces: calls of more than one slice
                                              //   alternate their slices between the two (created at the first such call)
    bool is_twin = false, two_streams = true; // SSA_TWO_STREAMS=0 turns the alternation off
    bool counted_live = false;                // counted among the live contexts of its device (ssa_api.hip: live_ctxs_on)
#define X(name) DevBuf name;
    SSA_CTX_DEVBUFS(X)
#undef X
#define X(name) HostBuf name;
    SSA_CTX_HOSTBUFS(X)
#undef X
    bool default_params = false;   // created from the built-in (unpinned) blob
    int fault_after_chunk = -1;   // ssa_debug_fault_after_chunk (tests)
    uint64_t dedup_key[2] = {0, 0};   // the key of the dedup's fingerprint (ssa_dedup.hpp): getrandom(2) at the first use
    bool dedup_key_set = false;
    bool ctab_ready = false;      // the constant-time signer's table (ctab) is built
    bool rng_pinned = false;      // the test pin of the device-drawn scalars (ssa_rng.hpp)
    uint8_t rng_pin[44] = {};
    std::map<std::string, std::vector<TimedLaunch>> timed;
    std::vector<struct ssa_keyset *> keysets;   // live key sets of this context (orphaned, not leaked, by ssa_ctx_destroy)
    std::vector<struct ssa_signer_set *> signer_sets;   // live signer sets (ssa_sign.hip), orphaned the same way
    std::vector<struct ssa_keycache *> keycaches;       // live key caches, orphaned the same way
    std::vector<struct ssa_aggregator *> aggregators;   // live streaming aggregators, the same way
    std::vector<struct ssa_aggverifier *> aggverifiers; // live streaming aggregate verifiers, the same way
};

template <class Ctx, class F>
static inline void for_each_devbuf(Ctx *c, F &&f) {
#define X(name) f(c->name);
    SSA_CTX_DEVBUFS(X)
#undef X
}
template <class Ctx, class F>
static inline void for_each_hostbuf(Ctx *c, F &&f) {
#define X(name) f(c->name);
    SSA_CTX_HOSTBUFS(X)
#undef X
}

// p out of a list of live handles (a context's key sets, signer sets or key caches; the comb registry), if it is there
template <class T>
static inline void forget_handle(std::vector<T *> &v, T *p) {
    const auto it = std::find(v.begin(), v.end(), p);
    if (it != v.end()) v.erase(it);
}

// keyed context (entry points in ssa_api.hip; ssa_ctx_destroy orphans the key sets that outlive their context)
struct ssa_keyset {
    ssa_ctx *ctx = nullptr;   // nullptr: the context is gone, the device memory went with it
    size_t m = 0;
    bool comb = false;      // per-key comb tables (16 x 65536 rows = 100 MB per key) instead of the ladder's 16 multiples
    DevBuf tab, status, pks, inf, ktab;     // inf: the pk_inf boolean of each key (zeros when the caller gave none)
    void release_all() {
        tab.release();
        status.release();
        pks.release();
        inf.release();
        ktab.release();
    }
};

// key cache (entry points in ssa_api.hip and ssa_msm.hip): a ladder-kind key set of `capacity` rows
// that fills itself (rows.tab, rows.status, rows.pks: rows [0, held) are complete), the pk_inf boolean of each row, and
// the slot table over the rows (ssa_keycache.hpp).  The host knows `held`: rows are handed out in order and never freed
// but by a clear of the whole cache or a compaction (below).  In wire mode (SSA_KEYCACHE_WIRE) the identity of a row is the
// 49 compressed bytes it was built from, kept in `wire` as seven words per row.
struct ssa_keycache {
    ssa_ctx *ctx = nullptr;   // nullptr: the context is gone, the device memory went with it
    size_t capacity = 0, held = 0, n_slots = 0;
    uint64_t clears = 0;
    bool wire_mode = false;
    ssa_keyset rows;          // never registered with the context: owned by the cache
    DevBuf inf, slots, wire;
    // eviction (ssa_keycache_set_eviction): the policy, the epoch (one per slice that looks keys up
    // under SSA_KEYCACHE_EVICT_RECENT), the rows' stamps and the compaction's scratch (both allocated at the first switch
    // to that policy and kept), and what ssa_keycache_eviction_info reports
    uint32_t policy = 0;
    uint64_t epoch = 0, compactions = 0, dropped = 0, last_kept = 0, last_moved = 0;
    DevBuf stamps, evict_ws;
    uint64_t device_bytes() const {
        return rows.tab.cap + rows.status.cap + rows.pks.cap + inf.cap + slots.cap + wire.cap + stamps.cap + evict_ws.cap;
    }
    void release_all() {
        rows.release_all();
        inf.release();
        slots.release();
        wire.release();
        stamps.release();
        evict_ws.release();
    }
};

// signer set (the signing twin of ssa_keyset; entry points in ssa_sign.hip): m key pairs resident on the device
struct ssa_signer_set {
    ssa_ctx *ctx = nullptr;   // nullptr: the context is gone, the device memory went with it
    size_t m = 0;
    DevBuf sks, pks, cpks, status;        // m x 32 secret keys, m x 96 affine keys, m x 49 compressed keys, m statuses
    std::vector<uint8_t> host_status;     // a copy of `status`: what the host form refuses without a device round trip
    SignerView view() const { return {(const u8 *)sks.p, (const u8 *)pks.p, (const u8 *)cpks.p, (const u8 *)status.p, (u32)m}; }
    // the secret keys are zeroed on the device before their memory goes back to the allocator
    void wipe_release() {
        if (sks.p) {
            (void)hipMemsetAsync(sks.p, 0, sks.cap, ctx->stream);
            (void)hipStreamSynchronize(ctx->stream);
        }
        sks.release();
        pks.release();
        cpks.release();
        status.release();
    }
};

static inline unsigned grid_for(size_t n, unsigned block) { return (unsigned)((n + block - 1) / block); }

template <class F>
static inline int timed_launch(ssa_ctx *ctx, const char *name, F &&launch) {
    if (!ctx->knobs.timing) {
        launch();
        HIP_TRY(hipGetLastError());
        return 0;
    }
    TimedLaunch t;
    HIP_TRY(hipEventCreate(&t.start));
    HIP_TRY(hipEventCreate(&t.stop));
    HIP_TRY(hipEventRecord(t.start, ctx->stream));
    launch();
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(t.stop, ctx->stream));
    ctx->timed[name].push_back(t);
    return 0;
}

// what an entry measured, in ms: stop - start, or for the two launches of a split call the span from the earlier start to
// the later stop -- the largest of the four differences (events of two streams of one device compare); false: not measurable
static inline bool timed_ms(const TimedLaunch &t, float *ms) {
    if (hipEventElapsedTime(ms, t.start, t.stop) != hipSuccess) return false;
    if (!t.start2) return true;
    for (hipEvent_t s : {t.start, t.start2})
        for (hipEvent_t e : {t.stop, t.stop2}) {
            float d = 0;
            if (hipEventElapsedTime(&d, s, e) != hipSuccess) return false;
            if (d > *ms) *ms = d;
        }
    return true;
}
static inline void timed_destroy(TimedLaunch &t) {
    for (hipEvent_t ev : {t.start, t.stop, t.start2, t.stop2})
        if (ev) (void)hipEventDestroy(ev);
}


// ---- argument checks and host->device staging shared by the entry points ----
static inline int check_msgs(const MsgView &mv, size_t n) {
    if (n == 0) return 0;
    if (n > SSA_MAX_BATCH) return SSA_ERR_ARG;   // grid sizes and workspace offsets are computed for n <= 2^30
    if (!mv.off && mv.len > 0 && !mv.msgs) return SSA_ERR_ARG;
    if (!mv.off && mv.stride < mv.len) return SSA_ERR_ARG;
    if (mv.len > 0xffffffffull) return SSA_ERR_ARG;
    return 0;
}

// the offset table of a host batch (read here, so once per host entry point and before anything is enqueued): offsets
// never decrease and no message is longer than 2^32 - 1 bytes.  check_msgs also runs on device pointers: it reads no offset.
static inline int check_host_offsets(const uint64_t *off, size_t n) {
    if (off)
        for (size_t i = 0; i < n; i++)
            if (off[i + 1] < off[i] || off[i + 1] - off[i] > 0xffffffffull) return SSA_ERR_ARG;
    return 0;
}

static inline size_t msgs_bytes(const uint64_t *off, size_t stride, size_t len, size_t n) {
    if (n == 0) return 0;
    if (off) return (size_t)off[n];
    return (n - 1) * stride + len;
}

// a batch in host memory as the verification entry points take it: 81-byte signatures, 96-byte keys, optional identity
// flags, and the messages by offset table or by stride
struct HostBatch {
    const uint8_t *sigs, *pks, *pk_inf, *msgs;
    const uint64_t *msg_off;
    size_t msg_stride, msg_len;
    // lanes [lo, lo + cnt) as a batch of their own (an offset table is rebased into `off`, which must outlive the result)
    HostBatch slice(size_t lo, size_t cnt, std::vector<uint64_t> &off) const {
        HostBatch s = *this;
        s.sigs = sigs ? sigs + 81 * lo : nullptr;
        s.pks = pks ? pks + 96 * lo : nullptr;
        s.pk_inf = pk_inf ? pk_inf + lo : nullptr;
        if (msg_off) {
            off.resize(cnt + 1);
            for (size_t k = 0; k <= cnt; k++) off[k] = msg_off[lo + k] - msg_off[lo];
            s.msgs = msgs ? msgs + msg_off[lo] : nullptr;
            s.msg_off = off.data();
        } else {
            s.msgs = msgs ? msgs + lo * msg_stride : nullptr;
        }
        return s;
    }
};

// a batch in device memory as the internal device paths take it (host code only: kernels take the pointers and the
// MsgView).  Message offsets are absolute into msgs.msgs.
struct DevBatch {
    const uint8_t *sigs, *pks, *pk_inf;
    MsgView msgs;
    // lanes from lo on: signatures, keys and flags move by lo, strided messages by lo * stride, an offset table by lo
    // (the message bytes stay put)
    DevBatch slice(size_t lo) const {
        DevBatch s = *this;
        s.sigs = sigs ? sigs + 81 * lo : nullptr;
        s.pks = pks ? pks + 96 * lo : nullptr;
        s.pk_inf = pk_inf ? pk_inf + lo : nullptr;
        if (msgs.off) s.msgs.off = msgs.off + lo;
        else if (msgs.msgs) s.msgs.msgs = msgs.msgs + lo * msgs.stride;
        return s;
    }
};

// fn(lo, cnt, lanes [lo, lo + cnt) of b) for every slice of at most `slice` lanes, in order; stops at the first error
template <class F>
static inline int for_dev_slices(const DevBatch &b, size_t n, size_t slice, F &&fn) {
    for (size_t lo = 0; lo < n; lo += slice)
        if (int rc = fn(lo, n - lo < slice ? n - lo : slice, b.slice(lo))) return rc;
    return 0;
}

// The argument checks of the entry points that return one status byte per signature, before anything is zeroed or
// enqueued: host forms (the offset table is read here) and device forms (d_coeffs: coefficients of coeff_bytes each)
static inline int check_host_batch(const ssa_ctx *ctx, const HostBatch &b, size_t n, const uint8_t *status_out) {
    if (!ctx || (n && (!b.sigs || !b.pks || !status_out))) return SSA_ERR_ARG;
    if (int rc = check_msgs({b.msgs, b.msg_off, b.msg_stride, b.msg_len}, n)) return rc;
    return check_host_offsets(b.msg_off, n);
}
static inline int check_dev_batch(const ssa_ctx *ctx, const DevBatch &b, size_t n, const uint8_t *d_status_out,
                                  const uint8_t *d_coeffs = nullptr, uint32_t coeff_bytes = 32) {
    if (!ctx || (n && (!b.sigs || !b.pks || !d_status_out))) return SSA_ERR_ARG;
    if (d_coeffs && (coeff_bytes == 0 || coeff_bytes > 32)) return SSA_ERR_ARG;
    return check_msgs(b.msgs, n);
}

// small batches take the cooperative kernel (one wave per signature: low latency), large ones the lane kernels (one lane
// per signature: throughput).  The host forms stage their inputs by this answer and the device forms launch by it.
static inline bool takes_coop_of(size_t coop_max_n, size_t coop_max_n_torsion, size_t n, uint32_t flags) {
    const size_t coop_lim = (flags & SSA_FLAG_CHECK_TORSION) ? coop_max_n_torsion : coop_max_n;
    return (flags & SSA_FLAG_FORCE_COOP) || (!(flags & SSA_FLAG_FORCE_LANE) && n <= coop_lim);
}
static inline bool takes_coop(const ssa_ctx *ctx, size_t n, uint32_t flags) {
    return takes_coop_of(ctx->knobs.coop_max_n, ctx->knobs.coop_max_n_torsion, n, flags);
}

// the statistics words an entry point reports (`width` of them: 4 for the dedup, 8 screened, 12 with a key cache), summed
// over its slices; the host forms' two threads add to it under the lock
struct CallStats {
    const int width;
    std::mutex mu;
    uint64_t v[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    explicit CallStats(int words) : width(words) {}
    void add(const uint64_t *d) {
        std::lock_guard<std::mutex> lock(mu);
        for (int k = 0; k < width; k++) v[k] += d[k];
    }
    void out(uint64_t *stats_out) const {
        if (stats_out)
            for (int k = 0; k < width; k++) stats_out[k] = v[k];
    }
};

// device copies of one slice of a batch; hashed: ctx->ws_h already holds the challenge scalars (pipelined_upload_hash)
struct StagedInputs {
    DevBatch batch{};
    const u8 *coeffs = nullptr;
    bool hashed = false;
};

// a counted device form begins: the context's device is selected, and the rejection counter (the caller's, or the
// context's own) is zeroed on ctx->stream
static inline int reset_fail_counter(ssa_ctx *ctx, uint64_t *d_n_fail_out, unsigned long long **d_fail) {
    HIP_TRY(hipSetDevice(ctx->device));
    *d_fail = (unsigned long long *)(d_n_fail_out ? (void *)d_n_fail_out : ctx->ws_fail.p);
    HIP_TRY(hipMemsetAsync(*d_fail, 0, sizeof(unsigned long long), ctx->stream));
    return 0;
}

// Device copies of secrets (keys, nonces, seeds, parent and master xprvs) do not outlive the call that made them,
// whichever way it returns: the named buffers are zeroed on the context's stream, each clamped to its capacity, when
// this goes out of scope.  Whoever owns it synchronises where the call must not return before the zeroing.
struct SecretWipe {
    ssa_ctx *ctx;
    std::vector<std::pair<DevBuf *, size_t>> bufs;     // buffer, bytes of secrets in it
    void add(DevBuf &b, size_t bytes) { bufs.emplace_back(&b, bytes); }
    bool zero() {             // true when something was zeroed
        bool any = false;
        for (auto &b : bufs)
            if (b.first->p && b.second) {
                (void)hipMemsetAsync(b.first->p, 0, std::min(b.second, b.first->cap), ctx->stream);
                any = true;
            }
        bufs.clear();
        return any;
    }
    ~SecretWipe() { zero(); }
};

constexpr bool SECRET = true;

// One call of a host-buffer entry point that stages its inputs, runs the device form and copies the results back.
// Built after the argument checks, it selects the device; in() stages an input into the named context buffer, out()
// reserves an output there and remembers where it goes (a null destination: no copy), msgs() stages a message batch.
// The first error sticks and every later step is skipped, so a call site needs no check per line.  finish() runs the
// device form, queues the copies back in order and synchronises once.  On destruction the secret buffers are zeroed on
// the stream, and the stream is drained if anything was zeroed or if an error return left work in flight: the caller
// may free or reuse its buffers as soon as the entry point returns.
struct HostCall {
    ssa_ctx *ctx;
    int rc = 0;
    bool enqueued = false, settled = false;
    SecretWipe wipe{ctx};
    struct Back { void *dst; const void *src; size_t bytes; };
    std::vector<Back> back;       // the copies of finish(), in order

    explicit HostCall(ssa_ctx *c) : ctx(c) { hip(hipSetDevice(ctx->device)); }
    ~HostCall() {
        const bool zeroed = wipe.zero();
        if (zeroed || (enqueued && !settled)) (void)hipStreamSynchronize(ctx->stream);
    }
    bool ok() const { return rc == 0; }
    void hip(hipError_t err) {
        if (err == hipSuccess || rc) return;
        if (ssa_debug_enabled()) std::fprintf(stderr, "[schnorr_sig_amd] host call: %s\n", hipGetErrorString(err));
        rc = SSA_ERR_HIP;
    }
    // one step on the stream (a launch, a device form), unless an earlier one failed
    template <class F>
    void step(F &&f) {
        if (rc) return;
        enqueued = true;
        rc = f();
    }
    // bytes of host memory into buf: its device copy (a non-null dummy for zero bytes), or nullptr for a null source
    template <class T = u8>
    const T *in(DevBuf &buf, const void *src, size_t bytes, bool secret = false) {
        if (rc) return nullptr;
        if (secret) wipe.add(buf, bytes);
        enqueued = true;
        if (buf.reserve(src && bytes ? bytes : 16)) rc = SSA_ERR_HIP;
        else if (src && bytes) hip(hipMemcpyAsync(buf.p, src, bytes, hipMemcpyHostToDevice, ctx->stream));
        return rc || !src ? nullptr : (const T *)buf.p;
    }
    // `bytes` of results in buf (reserved with `pad` bytes to spare), copied to dst by finish()
    u8 *out(DevBuf &buf, void *dst, size_t bytes, size_t pad = 0, bool secret = false) {
        if (rc) return nullptr;
        if (buf.reserve(bytes + pad)) {
            rc = SSA_ERR_HIP;
            return nullptr;
        }
        if (secret) wipe.add(buf, bytes);
        if (dst) copy_back(dst, buf.p, bytes);
        return (u8 *)buf.p;
    }
    void copy_back(void *dst, const void *src, size_t bytes) { back.push_back({dst, src, bytes}); }
    // the messages of n lanes into ctx->st_msgs (and the offset table into ctx->st_off)
    MsgView msgs(const uint8_t *msgs, const uint64_t *off, size_t stride, size_t len, size_t n) {
        MsgView mv{nullptr, nullptr, stride, len};
        if (off) mv.off = in<u64>(ctx->st_off, off, (n + 1) * sizeof(uint64_t));
        if (rc) return mv;
        const size_t mb = msgs_bytes(off, stride, len, n);
        if (mb && !msgs) rc = SSA_ERR_ARG;
        else if (ctx->st_msgs.reserve(mb + 16)) rc = SSA_ERR_HIP;
        else if (mb) hip(hipMemcpyAsync(ctx->st_msgs.p, msgs, mb, hipMemcpyHostToDevice, ctx->stream));
        mv.msgs = rc ? nullptr : (const u8 *)ctx->st_msgs.p;
        return mv;
    }
    // the n lanes of an aggregate call, staged in this order: the lead array (b.sigs: lead_bytes of signatures, R's or a
    // wire form) into ctx->st_sigs, the keys (96 bytes each into ctx->st_pks; wire_keys: 49 each into ctx->st_keyed),
    // the identity flags if there are any, the messages
    DevBatch lanes(const HostBatch &b, size_t lead_bytes, size_t n, bool wire_keys = false) {
        DevBatch d{};
        d.sigs = in(ctx->st_sigs, b.sigs, lead_bytes);
        d.pks = wire_keys ? in(ctx->st_keyed, b.pks, n * 49) : in(ctx->st_pks, b.pks, n * 96);
        d.pk_inf = b.pk_inf ? in(ctx->st_inf, b.pk_inf, n) : nullptr;
        d.msgs = msgs(b.msgs, b.msg_off, b.msg_stride, b.msg_len, n);
        return d;
    }
    template <class F>
    int finish(F &&device_form) {
        step(device_form);
        for (const Back &c : back)
            if (rc == 0) hip(hipMemcpyAsync(c.dst, c.src, c.bytes, hipMemcpyDeviceToHost, ctx->stream));
        if (rc == 0 && !back.empty()) hip(hipStreamSynchronize(ctx->stream));
        settled = rc == 0;
        return rc;
    }
};


// defined in ssa_api.hip
int ssa_internal_hash_chunk(ssa_ctx *ctx, hipStream_t hs, const DevBatch &b, size_t cnt, uint64_t *d_h);

// An error return after work was queued on the context's side streams (copies out of the bounce buffers, hash launches
// that write ctx->ws_h, msm_k_prepare): wait for all of it before the next call reuses the buffers it reads or writes.
struct SideStreamDrain {
    ssa_ctx *armed = nullptr;   // set with the first enqueue; done(): no error return from here on needs the wait
    void done() { armed = nullptr; }
    ~SideStreamDrain() {
        if (!armed) return;
        (void)hipStreamSynchronize(armed->copy_stream);
        for (auto &hs : armed->hash_stream) (void)hipStreamSynchronize(hs);
        (void)hipStreamSynchronize(armed->stream);
    }
};

// Host-buffer uploads go through page-locked memory of the LIBRARY's (ctx->pin_in): the caller's bytes are copied into it
// by host threads, chunk by chunk, and the DMA engines read it asynchronously, under the kernels of the chunk before.
// Rounds 3-5 registered the CALLER's memory with the runtime for the duration of a call instead (hipHostRegister: no host
// copy, 29 M verifications/s).  That is not safe: for buffers that live in the process heap -- where glibc puts even
// megabyte arrays once its mmap threshold has grown, and where a range shares its first and last page with its neighbours --
// a later ordinary copy out of such memory faulted on the GPU side (`Memory access fault` on a page-aligned heap address;
// tools/soak_large.py found it within ten iterations, never with the in-place registration off, never with the arrays in
// their own mappings).  Whatever the runtime keeps of a registration, a library has no business changing the mapping state
// of memory it does not own.
struct PipelinedInputs : SideStreamDrain {
    StagedInputs s;     // device copies (context staging buffers)
};

// caller memory -> page-locked memory on up to SSA_COPY_THREADS (default 8) host threads (one thread moves ~10 GB/s; a
// 2^20-signature slice is 270 MB and its upload must not take as long as its kernels)
static inline size_t host_copy_threads() {
    static const size_t t = [] {
        const char *e = std::getenv("SSA_COPY_THREADS");
        const long v = e ? std::atol(e) : 8;
        return (size_t)(v < 1 ? 1 : v > 32 ? 32 : v);
    }();
    return t;
}
static inline void host_copy(void *dst, const void *src, size_t bytes) {
    constexpr size_t PIECE = 4u << 20;
    if (bytes <= 2 * PIECE || host_copy_threads() == 1) {
        std::memcpy(dst, src, bytes);
        return;
    }
    const size_t parts = bytes / PIECE < host_copy_threads() ? bytes / PIECE : host_copy_threads();
    const size_t per = (bytes / parts + 63) & ~(size_t)63;
    std::vector<std::thread> th;
    for (size_t t = 1; t < parts; t++) {
        const size_t lo = t * per, hi = t + 1 == parts ? bytes : (t + 1) * per;
        th.emplace_back([=] { std::memcpy((char *)dst + lo, (const char *)src + lo, hi - lo); });
    }
    std::memcpy(dst, src, per < bytes ? per : bytes);
    for (auto &x : th) x.join();
}

// debug hook of the error-path tests (ssa_debug_fault_after_chunk): the next pipelined upload fails (SSA_ERR_HIP) after
// chunk k has been enqueued.  One shot, armed through the ABI on this context only: no environment is read per call.
static inline int pipeline_fault_chunk(ssa_ctx *ctx) {
    const int k = ctx->fault_after_chunk;
    ctx->fault_after_chunk = -1;
    return k;
}

// Uploads of a large host-buffer batch in chunks on the copy stream; the challenge hashes of chunk c start as soon as
// chunk c has arrived (they are 27 % of the per-signature work, 62 % of the MSM form), alternating between two
// streams -- a lane hashes for ~4 ms and a launch's tail would otherwise idle most of the chip once per chunk.
// Ordering: the side streams first wait for everything already queued on ctx->stream (an earlier asynchronous
// *_device call may still read ws_h or the staging buffers this call overwrites), and on return ctx->stream waits for
// all of it: whatever the caller enqueues next sees the inputs and ctx->ws_h.
// *used == false: the ranges could not be pinned (e.g. a read-only mapping) and nothing was enqueued.
static inline int pipelined_upload_hash(ssa_ctx *ctx, const HostBatch &b, size_t n, PipelinedInputs &pin, bool *used) {
    const uint8_t *sigs = b.sigs, *pks = b.pks, *pk_inf = b.pk_inf, *msgs = b.msgs;
    const uint64_t *msg_off = b.msg_off;
    const size_t msg_stride = b.msg_stride, msg_len = b.msg_len;
    *used = false;
    // arguments first: nothing is pinned or enqueued for a call that is going to be refused (the offset table was
    // checked by the entry point)
    const size_t mb = msgs_bytes(msg_off, msg_stride, msg_len, n);
    if (mb && !msgs) return SSA_ERR_ARG;
    auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t o_pks = al(n * 81), o_msgs = o_pks + al(n * 96), o_inf = o_msgs + al(mb),
                 o_off = o_inf + al(pk_inf ? n : 0), total = o_off + al(msg_off ? (n + 1) * sizeof(uint64_t) : 0);
    if (ctx->pin_in.reserve(total)) return 0;      // no page-locked memory to be had: the staged path
    u8 *h_sigs = (u8 *)ctx->pin_in.p, *h_pks = h_sigs + o_pks, *h_msgs = h_sigs + o_msgs, *h_inf = h_sigs + o_inf,
       *h_off = h_sigs + o_off;
    *used = true;
    if (ctx->st_sigs.reserve(n * 81) || ctx->st_pks.reserve(n * 96) || ctx->st_msgs.reserve(mb + 16) ||
        ctx->ws_h.reserve(n * 4 * sizeof(u64)) || (msg_off && ctx->st_off.reserve((n + 1) * sizeof(uint64_t))) ||
        (pk_inf && ctx->st_inf.reserve(n)))
        return SSA_ERR_HIP;
    HIP_TRY(hipEventRecord(ctx->pipe_start, ctx->stream));
    HIP_TRY(hipStreamWaitEvent(ctx->copy_stream, ctx->pipe_start, 0));
    for (auto &hs : ctx->hash_stream) HIP_TRY(hipStreamWaitEvent(hs, ctx->pipe_start, 0));
    pin.armed = ctx;
    const int fault_chunk = pipeline_fault_chunk(ctx);
    u8 *d_sigs = (u8 *)ctx->st_sigs.p, *d_pks = (u8 *)ctx->st_pks.p, *d_msgs = (u8 *)ctx->st_msgs.p;
    DevBatch &d = pin.s.batch;
    d = {d_sigs, d_pks, nullptr, {d_msgs, nullptr, msg_stride, msg_len}};
    if (msg_off) {
        host_copy(h_off, msg_off, (n + 1) * sizeof(uint64_t));
        HIP_TRY(hipMemcpyAsync(ctx->st_off.p, h_off, (n + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, ctx->copy_stream));
        d.msgs.off = (const u64 *)ctx->st_off.p;
    }
    if (pk_inf) {
        host_copy(h_inf, pk_inf, n);
        HIP_TRY(hipMemcpyAsync(ctx->st_inf.p, h_inf, n, hipMemcpyHostToDevice, ctx->copy_stream));
        d.pk_inf = (const u8 *)ctx->st_inf.p;
    }
    const unsigned chunks = ctx->knobs.pipeline_chunks;
    for (unsigned c = 0; c < chunks; c++) {
        const size_t lo = n * c / chunks, hi = n * (c + 1) / chunks, cnt = hi - lo;
        if (cnt == 0) continue;
        // (the host copies of chunk c run while the DMA engines and the hash kernels work on chunk c - 1)
        host_copy(h_sigs + 81 * lo, sigs + 81 * lo, cnt * 81);
        HIP_TRY(hipMemcpyAsync(d_sigs + 81 * lo, h_sigs + 81 * lo, cnt * 81, hipMemcpyHostToDevice, ctx->copy_stream));
        host_copy(h_pks + 96 * lo, pks + 96 * lo, cnt * 96);
        HIP_TRY(hipMemcpyAsync(d_pks + 96 * lo, h_pks + 96 * lo, cnt * 96, hipMemcpyHostToDevice, ctx->copy_stream));
        const size_t m_lo = msg_off ? (size_t)msg_off[lo] : lo * msg_stride;
        const size_t m_hi = msg_off ? (size_t)msg_off[hi] : (hi == n ? mb : hi * msg_stride);
        if (m_hi > m_lo) {
            host_copy(h_msgs + m_lo, msgs + m_lo, m_hi - m_lo);
            HIP_TRY(hipMemcpyAsync(d_msgs + m_lo, h_msgs + m_lo, m_hi - m_lo, hipMemcpyHostToDevice, ctx->copy_stream));
        }
        HIP_TRY(hipEventRecord(ctx->copy_done[c], ctx->copy_stream));
        hipStream_t hs = ctx->hash_stream[c & 1u];
        HIP_TRY(hipStreamWaitEvent(hs, ctx->copy_done[c], 0));
        if (int rc = ssa_internal_hash_chunk(ctx, hs, d.slice(lo), cnt, (uint64_t *)ctx->ws_h.p + 4 * lo)) return rc;
        HIP_TRY(hipEventRecord(ctx->hash_done[c], hs));
        HIP_TRY(hipStreamWaitEvent(ctx->stream, ctx->hash_done[c], 0));
        if ((int)c == fault_chunk) return SSA_ERR_HIP;   // injected (tests)
    }
    return 0;
}

// The inputs of ONE host slice on the device, for status_host_one and msm_host_one: a large slice
// (with `pipeline`, from ctx->knobs.pipeline_min_n lanes on) goes through pipelined_upload_hash, which leaves the challenge
// hashes in ctx->ws_h (hashed) and arms `pin`; any other slice, or one that finds no page-locked memory for its
// statuses (pin_out) or for the caller's 32-byte coefficients, is staged by `hc`.  Errors are left in hc.rc.
static inline StagedInputs slice_inputs(HostCall &hc, PipelinedInputs &pin, const HostBatch &b, size_t n,
                                        const uint8_t *coeffs, bool pipeline, bool pin_out) {
    ssa_ctx *ctx = hc.ctx;
    if (hc.ok() && pipeline && n >= ctx->knobs.pipeline_min_n && ctx->knobs.pipeline_chunks > 1 && !(pin_out && ctx->pin_out.reserve(n)) &&
        (!coeffs || ctx->pin_coeffs.reserve(n * 32) == 0)) {
        bool used = false;
        if (coeffs && ctx->st_coeffs.reserve(n * 32)) hc.rc = SSA_ERR_HIP;
        else hc.rc = pipelined_upload_hash(ctx, b, n, pin, &used);
        if (!hc.ok() || used) {
            StagedInputs s = pin.s;
            s.hashed = true;
            if (coeffs && hc.ok()) {
                // behind the chunk copies on the copy stream; ctx->stream waits for this copy explicitly
                host_copy(ctx->pin_coeffs.p, coeffs, n * 32);
                hc.step([&] {
                    HIP_TRY(hipMemcpyAsync(ctx->st_coeffs.p, ctx->pin_coeffs.p, n * 32, hipMemcpyHostToDevice, ctx->copy_stream));
                    HIP_TRY(hipEventRecord(ctx->pipe_start, ctx->copy_stream));
                    HIP_TRY(hipStreamWaitEvent(ctx->stream, ctx->pipe_start, 0));
                    return 0;
                });
                s.coeffs = (const u8 *)ctx->st_coeffs.p;
            }
            return s;
        }
    }
    StagedInputs s;
    s.batch.sigs = hc.in(ctx->st_sigs, b.sigs, n * 81);
    s.batch.pks = hc.in(ctx->st_pks, b.pks, n * 96);
    if (b.pk_inf) s.batch.pk_inf = hc.in(ctx->st_inf, b.pk_inf, n);
    s.batch.msgs = hc.msgs(b.msgs, b.msg_off, b.msg_stride, b.msg_len, n);
    if (coeffs) s.coeffs = hc.in(ctx->st_coeffs, coeffs, n * 32);
    return s;
}

// ONE slice from host buffers for the entry points that return one status byte per signature: the inputs staged or
// pipelined (slice_inputs: coeffs, pipeline and pin_out are its arguments), device_form(inputs, d_status, d_fail) run on
// ctx->stream -- it leaves the rejection count in *d_fail, zeroing or counting as its pipeline needs -- and statuses and
// count copied back.  With pin_out the statuses of a pipelined slice come back through page-locked memory.
template <class F>
static int status_host_one(ssa_ctx *ctx, const HostBatch &b, size_t n, const uint8_t *coeffs, bool pipeline, bool pin_out,
                           uint8_t *status_out, uint64_t *n_fail_out, F &&device_form) {
    HostCall hc(ctx);
    PipelinedInputs pin;      // its destructor drains the side streams on every error return
    const StagedInputs s = slice_inputs(hc, pin, b, n, coeffs, pipeline, pin_out);
    const bool through_pin = pin_out && s.hashed;
    u8 *d_status = hc.out(ctx->st_status, through_pin ? ctx->pin_out.p : status_out, n, 16);
    unsigned long long nf = 0, *d_fail = (unsigned long long *)ctx->ws_fail.p;
    hc.copy_back(&nf, d_fail, sizeof nf);
    if (int rc = hc.finish([&] { return device_form(s, d_status, d_fail); })) return rc;
    pin.done();
    if (through_pin) std::memcpy(status_out, ctx->pin_out.p, n);
    if (n_fail_out) *n_fail_out = nf;
    return 0;
}

// defined in ssa_api.hip: hash_message + Scalar::from_bits_vartime for n signatures into ctx->ws_h
int ssa_internal_hash_scalars(ssa_ctx *ctx, const DevBatch &b, size_t n);

// the same launch (timing key ssa_k_hash) with its outputs named: the scalars into d_h (n x 4 words) and the raw digests
// into d_dig (n x 32 bytes), both the caller's
int ssa_internal_hash_scalars_digests(ssa_ctx *ctx, const DevBatch &b, size_t n, uint64_t *d_h, uint8_t *d_dig);

// defined in ssa_msm.hip, for ssa_verify_aggregate (ssa_api.hip): ONE slice (n <= ctx->knobs.msm_slice) of the MSM form
// reduced to its 24-word record on ctx->stream -- the left-hand point in canonical form, sum s_i e_i, the malformed flag.
// d_h: the slice's challenge scalars if they exist (batches of at most ctx->knobs.msm_small_max lanes hash for themselves)
int ssa_internal_msm_record(ssa_ctx *ctx, const DevBatch &b, size_t n, const uint8_t *d_coeffs, uint32_t coeff_bytes,
                            const uint64_t *d_h, uint64_t *d_record_out);

// defined in ssa_msm.hip, for the streaming aggregate verifier (ssa_api.hip): ONE slice of the
// bucket pipeline -- never msm_k_small -- whose first stage is the caller's.  `fill` is called once, after the flags are
// zeroed, and enqueues on ctx->stream whatever writes what MsmFill names for the n lanes: the 2n point rows (R_i at i,
// -P_i at n + i, (0, 0) for the identity), the signed digits of the coefficients (coeff_bytes < 32 wide) over windows
// [0, wa) for point i and of a_i h_i mod q over all windows for point n + i, n_blocks partial sums of a_i e_i (32 bytes
// each), and flags[0] != 0 when a lane is malformed.  The record then comes out as ssa_internal_msm_record's.
struct MsmFill {
    MsmShape sh;
    u32 wa;
    size_t n;
    unsigned n_blocks;
    u64 *points;
    short *digits;
    u64 *partials;
    u32 *flags;
};
using MsmFillFn = std::function<int(const MsmFill &)>;
int ssa_internal_msm_record_prepared(ssa_ctx *ctx, size_t n, uint32_t coeff_bytes, const MsmFillFn &fill,
                                     uint64_t *d_record_out);

// defined in ssa_msm.hip, for the sharded half-aggregation (ssa_api.hip): k (1..4096) records added
// up into ONE record by one wave on ctx->stream -- points, scalars mod q, malformed words OR-ed.  checked: the records
// come from outside the call and are validated first (magic, malformed word, canonical limbs and scalar, point on the
// curve); one that fails makes the sum the malformed record.
int ssa_internal_msm_sum_records(ssa_ctx *ctx, const uint64_t *d_records, size_t k, bool checked, uint64_t *d_record_out);

// defined in ssa_msm.hip, for ssa_verify_aggregates_many (ssa_api.hip): the left-hand sides of one
// group of aggregates, by msm_k_small and one record sum per aggregate, or by the screened MSM over padded segments
int ssa_internal_msm_agg_small(ssa_ctx *ctx, const DevBatch &b, size_t n, const uint8_t *d_coeffs16, const uint32_t *d_first,
                               uint32_t agg0, uint32_t aggs, const uint64_t **d_recs_out);
int ssa_internal_msm_agg_segments(ssa_ctx *ctx, const DevBatch &b, uint32_t segs, uint32_t seg_lanes,
                                  const uint8_t *d_coeffs16, const uint64_t *d_h, const uint8_t *d_mask, uint8_t *d_recheck,
                                  const uint8_t *d_rhs, uint8_t *d_seg_ok);

// defined in ssa_msm.hip, for ssa_aggregate_valid_many (ssa_api.hip): the statuses of
// ssa_verify_batch_screened (library-drawn coefficients) for ONE slice whose challenge scalars are already in d_h, into
// d_status[0, n); d_fail != nullptr: *d_fail = the number of nonzero ones.  The messages of b are not read; d_h is only
// read.  At most one synchronisation (none at n <= ctx->knobs.msm_small_max).
int ssa_internal_screen_hashed(ssa_ctx *ctx, const DevBatch &b, size_t n, const uint64_t *d_h, uint8_t *d_status,
                               unsigned long long *d_fail);

// defined in ssa_msm.hip, for ssa_aggregate_valid_many_cached (ssa_api.hip): the statuses and the
// 12 statistics words of ssa_verify_many_cached_device / ssa_verify_keyed_many_cached_device (subgroup check and flag
// byte, library-drawn coefficients) for the n >= 1 lanes of a call, slice after slice through the cache as those calls
// take them, with ONE hash per lane.  Affine: the scalars are ready in d_h and only read.  Records: the keys exist only
// behind each slice's look-up, so one ssa_k_hash per slice writes that slice's scalars into d_h and raw digests into
// d_dig, and nothing else hashes.  stats_out: host memory, may be null.
int ssa_internal_screen_many_hashed(ssa_ctx *ctx, struct ssa_keycache *kc, const DevBatch &b, size_t n, const uint64_t *d_h,
                                    uint8_t *d_status, uint64_t stats_out[12]);
int ssa_internal_screen_keyed_hashed(ssa_ctx *ctx, struct ssa_keycache *kc, const uint8_t *d_keyed, const MsgView &mv,
                                     size_t n, uint64_t *d_h, uint8_t *d_dig, uint8_t *d_status, uint64_t stats_out[12]);

// defined in ssa_api.hip: ssa_k_verify over n lanes of b (its messages unused) whose challenge scalars are already in
// d_h (the per-lane workspace reserved for one slice of lanes); *d_fail is added to
int ssa_internal_verify_hashed(ssa_ctx *ctx, const DevBatch &b, const uint64_t *d_h, size_t n, uint32_t flags,
                               uint8_t *d_status_out, unsigned long long *d_fail);

// defined in ssa_api.hip: ssa_verify_many_device for the library's own use -- the same call, but a one-slice batch is
// never split over the two streams (only the exported entry point may)
int ssa_internal_verify_many_device(ssa_ctx *ctx, const uint8_t *d_sigs, const uint8_t *d_pks, const uint8_t *d_pk_inf,
                                    const uint8_t *d_msgs, const uint64_t *d_msg_off, size_t msg_stride, size_t msg_len,
                                    size_t n, uint32_t flags, uint8_t *d_status_out, uint64_t *d_n_fail_out);

// defined in ssa_api.hip, for ssa_verify_many_screened (ssa_msm.hip): the distinct keys of one slice of at most
// ctx->knobs.lane_slice lanes checked once each (ctx->dd_idx, ctx->dd_kstatus, tables in ctx->ws_tab; one synchronisation, for
// u), and ssa_k_verify_keyed over n lanes against those keys (*d_fail is added to)
int ssa_internal_dedup_keys(ssa_ctx *ctx, const uint8_t *d_pks, const uint8_t *d_pk_inf, size_t cnt, uint64_t *u_out,
                            uint64_t *bound_hits_out);
int ssa_internal_verify_keyed(ssa_ctx *ctx, const uint8_t *d_sigs, const uint32_t *d_key_idx, uint64_t u,
                              const uint64_t *d_h, size_t n, uint32_t flags, uint8_t *d_status_out,
                              unsigned long long *d_fail);

// where the checked keys of a slice are: a key number per lane, the keys' tables of sixteen multiples and status bytes,
// and the bound of the key numbers.  The context's own (ssa_internal_dedup_keys) or rows of a key cache.
struct KeyView {
    const uint32_t *lane_key;
    const uint64_t *tab;
    const uint8_t *status;
    uint32_t n_keys;
};
// the view ssa_internal_dedup_keys leaves: ctx->dd_idx, ctx->ws_tab, ctx->dd_kstatus
static inline KeyView ctx_key_view(const ssa_ctx *ctx, uint64_t u) {
    return {(const uint32_t *)ctx->dd_idx.p, (const uint64_t *)ctx->ws_tab.p, (const uint8_t *)ctx->dd_kstatus.p, (uint32_t)u};
}
// ssa_internal_verify_keyed with explicit pointers
int ssa_internal_verify_keyed_view(ssa_ctx *ctx, const uint8_t *d_sigs, const uint32_t *d_lane_key, const KeyView &kv,
                                   const uint64_t *d_h, size_t n, uint32_t flags, uint8_t *d_status_out,
                                   unsigned long long *d_fail);

// defined in ssa_api.hip, for ssa_verify_many_cached (ssa_msm.hip): the distinct keys of one slice looked up in the cache
// and the unseen ones checked and inserted (or the cache cleared, or bypassed: ssa_keycache.hpp).
// One synchronisation, the one of the dedup.  *kv is where the slice's keys are; ks[0] keys found, ks[1] keys inserted,
// ks[2] automatic clears, ks[3] 1 when the slice bypassed the cache; *d_unpublished (device, read it behind the slice's
// later launches) counts rows that found no slot, or is nullptr.
int ssa_internal_keycache_slice(ssa_ctx *ctx, struct ssa_keycache *kc, const uint8_t *d_pks, const uint8_t *d_pk_inf,
                                size_t cnt, KeyView *kv, uint64_t *u_out, uint64_t *bound_hits_out, uint64_t ks[4],
                                const unsigned long long **d_unpublished);

// defined in ssa_api.hip, for ssa_verify_keyed_many_cached (ssa_msm.hip): ONE slice of cnt 130-byte
// records through a key cache in wire mode.  The signatures are split into ctx->ky_sigs, the distinct 49-byte keys are
// found and looked up, the misses decompressed, checked and inserted (or the cache cleared, or bypassed), and every
// lane's key bytes and flag expanded into ctx->ky_pks / ctx->ky_inf: *b is the slice as the screen reads it (its
// messages are left alone).  The other results as ssa_internal_keycache_slice gives them; one synchronisation.
int ssa_internal_keyed_cache_slice(ssa_ctx *ctx, struct ssa_keycache *kc, const uint8_t *d_keyed, size_t cnt, DevBatch *b,
                                   KeyView *kv, uint64_t *u_out, uint64_t *bound_hits_out, uint64_t ks[4],
                                   const unsigned long long **d_unpublished);
// defined in ssa_api.hip: ssa_k_unpack_keyed over n records into ctx->ky_sigs / ky_pks / ky_inf (the exact keyed path)
int ssa_internal_unpack_keyed(ssa_ctx *ctx, const uint8_t *d_keyed, size_t n, DevBatch *b);

// defined in ssa_api.hip: ssa_k_keyset_build over m keys, queued on the context's stream (timing key ssa_k_keyset_build)
int ssa_internal_keyset_build(ssa_ctx *ctx, const uint8_t *d_pks, const uint8_t *d_pk_inf, size_t m, uint64_t *d_tab,
                              uint8_t *d_status);

// defined in ssa_sign.hip (ssa_selfcheck.hpp): the exact check of a comb table for G (res[0] failing rows, res[1] the
// first failing row or ~0) and of the context's constant-time table (out[0] rows checked, out[1], out[2] as res)
int ssa_internal_gtab_check(ssa_ctx *ctx, const uint64_t *d_gtab, uint32_t bits, uint64_t res[2]);
int ssa_internal_ctab_selfcheck(ssa_ctx *ctx, uint64_t out[3]);

// defined in ssa_api.hip: the context's second set of streams and workspaces (nullptr: none -- a twin itself, turned
// off, or no memory for it)
ssa_ctx *ssa_internal_twin(ssa_ctx *ctx);

// Host-buffer batches in bounded device memory (round 5): more than one slice of lanes runs slice after slice through
// staging buffers sized for ONE slice, pinning only the slice in flight, into the caller's one status array and one
// counter -- fn(c, lo, cnt) is the one-slice form of the entry point on context c.  With a twin (ssa_internal_twin) two host
// threads take alternate slices, one on the context and one on its twin: the upload of a slice runs under the kernels
// of the other, and the kernels' tails fill each other.
template <class F>
static int run_host_slices(ssa_ctx *ctx, size_t n, size_t slice, F &&fn) {
    const size_t k = (n + slice - 1) / slice;
    ssa_ctx *tw = k > 1 ? ssa_internal_twin(ctx) : nullptr;
    if (!tw) {
        for (size_t j = 0; j < k; j++) {
            const size_t lo = j * slice, cnt = n - lo < slice ? n - lo : slice;
            if (int rc = fn(ctx, lo, cnt)) return rc;
        }
        return 0;
    }
    int rcs[2] = {0, 0};
    auto worker = [&](size_t w) {
        if (hipSetDevice(ctx->device) != hipSuccess) {
            rcs[w] = SSA_ERR_HIP;
            return;
        }
        ssa_ctx *c = w ? tw : ctx;
        for (size_t j = w; j < k && rcs[w] == 0; j += 2) {
            const size_t lo = j * slice, cnt = n - lo < slice ? n - lo : slice;
            rcs[w] = fn(c, lo, cnt);
        }
    };
    std::thread second(worker, (size_t)1);
    worker(0);
    second.join();
    return rcs[0] ? rcs[0] : rcs[1];
}

// run_host_slices for the counted forms: fn(c, lo, cnt, slice, nf) is the one-slice form on context c for the lanes
// [lo, lo + cnt) of b (their own batch, slice), which writes its rejection count to *nf; the counts add up into
// *n_fail_out.  A batch of one slice is handed over whole.
template <class F>
static int run_host_slices_counted(ssa_ctx *ctx, const HostBatch &b, size_t n, size_t slice, uint64_t *n_fail_out, F &&fn) {
    if (n <= slice) return fn(ctx, (size_t)0, n, b, n_fail_out);
    std::mutex mu;
    uint64_t total = 0;
    const int rc = run_host_slices(ctx, n, slice, [&](ssa_ctx *c, size_t lo, size_t cnt) {
        std::vector<uint64_t> off;
        uint64_t nf = 0;
        const int r = fn(c, lo, cnt, b.slice(lo, cnt, off), &nf);
        std::lock_guard<std::mutex> lock(mu);
        total += nf;
        return r;
    });
    if (rc) return rc;
    if (n_fail_out) *n_fail_out = total;
    return 0;
}
