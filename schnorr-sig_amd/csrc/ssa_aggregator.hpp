// Internal: the streaming aggregator (ssa_aggregator_*).  A block producer receives signatures over
// a whole slot and needs the half-aggregate (ssa_aggregate.hpp) at block time.  Everything in front of the coefficients is
// independent of a lane's place in the aggregate -- the challenge hash, the admission check, the leaf, and every complete
// aligned block of B = 2^t leaves, which is a whole subtree of the level-by-level tree -- so it is
// done when the lanes arrive, and the object keeps the results on the device, in arrival order:
//
//   wire    49 bytes per lane: the R's, already in the aggregate's wire layout (and room for e_agg behind the last)
//   scal    four words per lane: e_i, canonical (every kept lane has e_i < q by either admission check)
//   leaves  four words per lane: leaf_i
//   tops    four words per COMPLETE block of B lanes: the top of its subtree
//   keys    49 bytes per lane, only in an object created with SSA_AGGR_HOLD_KEYS49: the wire key of
//           the lane's KeyedSignature record, verbatim -- the key column of the block body next to the aggregate
//   adm     one byte per lane, only in an object created with SSA_AGGR_HOLD_ADMISSION: the class of
//           the push that admitted the lane (SSA_ADM_*).  Written by agx_admit alone -- one hipMemsetAsync of
//           adm[held, held + m) behind agx_k_append, the kept count being on the host by then -- moved with its lane by
//           agx_k_move, read by ssa_aggregator_admission and by the mixed pushes of the streaming aggregate verifier
//           (agv_k_classify_adm, agv_k_require in ssa_aggverifier.hpp).  finish, finish_select and keys do not touch it.
//   index   8 bytes per slot, dd_slots_for(capacity) slots, and one counter, only in an object created with
//           SSA_AGGR_HOLD_INDEX: the open-addressing table of ssa_dedup.hpp over the leaf column,
//           which answers "which place holds this leaf?" (agi_k_insert, agi_k_lookup below).  LAZY: no push, finish or
//           removal touches it -- they keep `indexed` and `stale` on the host -- and all of its work is enqueued by
//           ssa_aggregator_index_sync and in front of a look-up.
//
//   push    status vector (the screen of ssa_verify_batch_screened, the checks of ag_k_fold, or -- the cached pushes,
//           section 31 -- the statuses of ssa_verify_many_cached / ssa_verify_keyed_many_cached) -> av_keep lists the kept
//           lanes -> agx_k_append stores leaf, scalar and R of each -> the blocks this push completed are reduced to
//           their tops: ag_k_tree over that range of the leaves for B = 512, log2 B launches of ag_k_level for smaller B
//   finish  for the first n held lanes: the stored tops of the n / B complete blocks are copied into a workspace of the
//           context, the ragged block [B (n / B), n) is reduced behind them by one workgroup of ag_k_tree (never into the
//           object: with n below the lanes held that slot is a complete block's top), ags_root gives the root,
//           agx_k_coeff_fold one partial sum of a_i e_i per workgroup, ag_k_fold_finish their sum, and two copies write
//           the R's and e_agg.  finish changes nothing in the object.
//   remove  (drop_front, remove) the kept lanes move to the front piece by piece through staging
//           workspaces of the context (agx_k_move, below), and agx_remove_plan says which tops stay, move or are reduced
//           again.  No message, key or signature is touched.
//   select  (finish_select, remove_indices) a list of distinct places, in the caller's order: the
//           named lanes are gathered into staging workspaces of the context (agx_k_select, below, which also decides
//           whether the list is valid), the tree runs over the gathered leaves from the bottom -- the stored tops say
//           nothing about another order -- and the coefficient fold is finish's.  The object is read, never written.
//
// The object's four (with the key column, the admission column and the leaf index: up to seven) arrays are its own allocations (released by destroy, or by the context's clean-up): they are not in
// the context's list of workspaces, and nothing the object needs between two calls lives in one.
#pragma once
#include "ssa_aggregate.hpp"
#include "ssa_ctx.hpp"
#include "ssa_dedup.hpp"

// What the streaming aggregator and the streaming aggregate verifier (ssa_aggverifier.hpp) both are: lanes in arrival
// order, their leaves, and the tops of the complete blocks of B.
struct AgxStore {
    ssa_ctx *ctx = nullptr;   // nullptr: the context is gone, the device memory went with it
    size_t capacity = 0, block = 0, held = 0;     // block: B, a power of two from 2 to AG_TREE_SPAN
    uint32_t flags = 0;                           // the create flags (each type says which it knows: kCreateFlags)
    uint64_t pushes = 0, finishes = 0;
    DevBuf leaves, tops;
    // a buffer of the object and the bytes it takes at the object's capacity and B
    struct Buf {
        DevBuf *buf;
        size_t bytes;
    };
    size_t n_tops() const { return block ? (capacity + block - 1) / block : 0; }
};

struct ssa_aggregator : AgxStore {
    static constexpr uint32_t kCreateFlags = SSA_AGGR_HOLD_KEYS49 | SSA_AGGR_HOLD_ADMISSION | SSA_AGGR_HOLD_INDEX;
    uint64_t offered = 0, dropped = 0;
    DevBuf wire, scal, keys, adm, index;
    // the leaf index (SSA_AGGR_HOLD_INDEX), host side: lanes [0, indexed) are in the table; stale:
    // the table says nothing (never cleared yet, or lanes moved since) and is cleared before the next insert
    size_t indexed = 0;
    bool stale = true;
    uint64_t rebuilds = 0, lookups = 0, looked_up = 0;
    bool hold_keys() const { return (flags & SSA_AGGR_HOLD_KEYS49) != 0; }
    bool hold_adm() const { return (flags & SSA_AGGR_HOLD_ADMISSION) != 0; }
    bool hold_index() const { return (flags & SSA_AGGR_HOLD_INDEX) != 0; }
    size_t index_slots() const { return ssa::dd_slots_for(capacity); }
    u64 *index_table() const { return (u64 *)index.p; }
    unsigned long long *index_over() const { return (unsigned long long *)index.p + index_slots(); }   // behind the slots
    // the lanes moved, or left: what the table says is void (every removal that changed the object, reset, a failed move)
    void index_void() {
        indexed = 0;
        stale = true;
    }
};
// everything the object will ever hold, in the order it is allocated and released (the key column: only with the flag,
// 49 bytes per lane and the rest of the last dword -- agx_k_move reads whole aligned dwords; the admission column: only
// with its flag, one byte per lane, read and written as bytes)
static inline std::vector<AgxStore::Buf> agx_bufs(ssa_aggregator &a) {
    std::vector<AgxStore::Buf> bufs{
        {&a.wire, 49 * a.capacity + 32}, {&a.scal, 32 * a.capacity}, {&a.leaves, 32 * a.capacity}, {&a.tops, 32 * a.n_tops()}};
    if (a.hold_keys()) bufs.push_back({&a.keys, 49 * a.capacity + 3});
    if (a.hold_adm()) bufs.push_back({&a.adm, a.capacity + 16});
    if (a.hold_index()) bufs.push_back({&a.index, 8 * a.index_slots() + 8});
    return bufs;
}
template <class T>
static inline void agx_release_all(T &obj) {
    for (const AgxStore::Buf &b : agx_bufs(obj)) b.buf->release();
}

namespace ssa {

// What a push of m kept lanes onto `held` lanes completes, with blocks of B lanes: blocks [first, first + count) get their
// tops, and the ragged tail is the `tail_len` lanes from `tail_first` on.  finish(n) reads the same plan with held = 0,
// m = n: `count` stored tops and the tail it reduces for itself.
struct AgxPlan {
    uint64_t first, count, tail_first, tail_len;
};
static inline AgxPlan agx_plan(uint64_t held, uint64_t m, uint64_t B) {
    const uint64_t b0 = held / B, b1 = (held + m) / B;
    return {b0, b1 - b0, B * b1, held + m - B * b1};
}

// What removing lanes does to the stored tops.  The object held `held` lanes, `m` are kept, and f
// is the first place whose content changes: the first removed lane (0 for a front drop; anything up to m when held == m,
// where nothing changes).  `front`: the removed lanes are exactly the first held - m.
//   blocks [0, unchanged)            keep their tops: every lane of theirs lies in front of f
//   blocks [0, moved)                front drop by a multiple of B only: new block b IS old block b + (held - m) / B, so
//                                    its top is moved, not computed again (then unchanged == 0 and count == 0)
//   blocks [first, first + count)    are reduced again from the moved leaves (agx_reduce_blocks)
// Every complete block of the new object, [0, m / B), is in exactly one of the three.
struct AgxRemovePlan {
    uint64_t unchanged, moved, first, count;
};
static inline AgxRemovePlan agx_remove_plan(uint64_t held, uint64_t f, uint64_t m, uint64_t B, bool front) {
    const uint64_t blocks = m / B;
    if (m == held) return {blocks, 0, blocks, 0};
    if (front && (held - m) % B == 0) return {0, blocks, blocks, 0};
    return {f / B, 0, f / B, blocks - f / B};
}

#ifndef SSA_NO_KERNELS
// status[i] = 0 or SSA_MALFORMED by the checks ssa_aggregate_many makes without SSA_AGG_CHECK (ag_k_fold with a status)
__global__ void __launch_bounds__(256)
agx_k_check(const u8 *__restrict__ sigs, const u8 *__restrict__ pks, const u8 *__restrict__ pk_inf, size_t n,
            u8 *__restrict__ status) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    sc256 e;
    status[i] = (u8)(ag_lane_ok(sigs, pks, pk_inf, i, true, e) ? ST_OK : ST_MALFORMED);
}

// The 49-byte columns (the R's in `wire`, the wire keys in `keys`) and the one rule by which they are written, here and
// in the staging of agx_k_move.  The lanes of a launch land on bytes [d0, d1) of `dst` -- a dword-aligned array; d0 and
// d1 are multiples of 49 and start and end anywhere mod 4 -- the lane at place p on [49 p, 49 (p + 1)).  A dword belongs
// to the lane its FIRST byte lies in, so a lane writes the aligned dwords that start in [49 p, 49 (p + 1)) -- the last of
// them may run into the next lane's bytes and takes those from `next`, the NEXT lane's source (read only where there is
// one: the dword ends within d1) -- as dwords while they end within d1.  The two edges are bytes: the first lane
// (49 p == d0) writes [d0, the first aligned address), the last lane what is left behind the last whole dword.  So no
// two threads write one dword, and no byte in front of d0 -- the lanes of earlier pushes -- or behind d1 is written.
// ANY: src lies in device memory at any alignment and the dwords inside the lane are read with ld_u32_any (agx_k_move);
// otherwise they are put together from bytes (agx_k_append, whose source is the caller's batch).
static __device__ __forceinline__ u32 ld_u32_any(const u8 *p) {
    const uintptr_t a = (uintptr_t)p;
    const u32 *q = reinterpret_cast<const u32 *>(a & ~(uintptr_t)3);
    const u32 sh = 8u * (u32)(a & 3u);
    const u32 lo = q[0];
    return sh ? (lo >> sh) | (q[1] << (32u - sh)) : lo;
}

template <bool ANY>
static __device__ __forceinline__ void agx_put49(u8 *__restrict__ dst, size_t d0, size_t d1, size_t place,
                                                 const u8 *__restrict__ src, const u8 *__restrict__ next) {
    const size_t lo = 49 * place, hi = lo + 49;
    size_t w = (lo + 3) & ~(size_t)3;
    if (lo == d0)
        for (size_t b = lo; b < w && b < d1; b++) dst[b] = src[b - lo];
    for (; w < hi; w += 4) {
        if (ANY && w + 4 <= hi) {
            *reinterpret_cast<u32 *>(dst + w) = ld_u32_any(src + (w - lo));
        } else if (w + 4 <= d1) {                     // (ANY: the dword shared with the next lane)
            u32 v = 0;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const size_t b = w + k;
                v |= (u32)(b < hi ? src[b - lo] : next[b - hi]) << (8 * k);
            }
            *reinterpret_cast<u32 *>(dst + w) = v;
        } else {                                      // (the last lane alone: for every other one d1 >= hi + 49)
            for (size_t b = w; b < d1; b++) dst[b] = src[b - lo];
        }
    }
}

// One lane per kept lane: rank c, source lane kept[c] of the push, place held + c of the aggregate.  The lanes are
// records of `stride` bytes with the signature at `off`: 81 / 0 for signatures, 130 / 49 for KeyedSignature records (the
// idiom of av_finish_kept).
//   leaves[held + c] = H(d || flag byte of R || 0xA1) from the lane's raw digest (the body of ag_k_leaf);
//   scal[held + c]   = e as four words;
//   wire[49 (held + c), + 49) = R;
//   keys[49 (held + c), + 49) = the first 49 bytes of the record, when the object has a key column (keys != nullptr;
//                               then the lanes are records).
// Both columns by agx_put49 on [49 held, 49 (held + m)).
__global__ void __launch_bounds__(256, 4)
agx_k_append(const DevParams *__restrict__ prm, const u8 *__restrict__ recs, u32 stride, u32 off,
             const u64 *__restrict__ dig, const u32 *__restrict__ kept, size_t m, size_t held, u64 *__restrict__ leaves,
             u64 *__restrict__ scal, u8 *__restrict__ wire, u8 *__restrict__ keys) {
    __shared__ u64 lds[RS_LDS_U64];
    u64 *A = lds + threadIdx.x;
    const size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= m) return;
    const size_t src = kept[c], dst = held + c;
    const u8 *rec = recs + (size_t)stride * src, *sig = rec + off;
    u64 d[4];
    ag_leaf_hash(A, prm, dig, src, sig[48], d);
    const sc256 e = ld_sc(sig + 49);
#pragma unroll
    for (int k = 0; k < 4; k++) {
        leaves[4 * dst + k] = d[k];
        scal[4 * dst + k] = e.w[k];
    }
    const u8 *next = c + 1 < m ? recs + (size_t)stride * kept[c + 1] : rec;     // (read only where c + 1 < m)
    agx_put49<false>(wire, 49 * held, 49 * (held + m), dst, sig, next + off);
    if (keys) agx_put49<false>(keys, 49 * held, 49 * (held + m), dst, rec, next);
}

// Removing lanes (ssa_aggregator_drop_front, _remove).  The kept lanes, ascending, take the places
// 0, 1, 2, ...: kept lane c comes from place src(c) = kept[c] (a mask; the list of av_keep) or c + shift (a front drop:
// kept == nullptr, no list exists), and src(c) >= c, src ascending.  What a lane stores does not depend on its place, so
// the lane is MOVED: four words of leaves, four of scal, 49 bytes of wire and, with a key column, 49 bytes of keys.
//
// The hazard.  The move is in place, and the threads of a launch run in no order: with one lane dropped at the front
// every thread's source is its neighbour's destination.  So no launch writes the object.  The host walks the kept
// lanes in ascending pieces [c0, c1) of at most the context's MSM slice, and for each piece
//   1. agx_k_move gathers the piece -- reads the object at src(c), writes STAGING (workspaces of the context) at c - c0;
//   2. three (with a key column: four) stream-ordered device-to-device copies put the staging back on places [c0, c1);
//   3. only then is the next piece enqueued, on the same stream.
// Why that is right: (a) a piece's own sources were all read by step 1 before step 2 began (stream order), so step 2
// may overwrite them; (b) every later piece reads places src(c) >= c >= c1, and step 2 wrote [c0, c1) alone, so no
// later source has been overwritten; (c) earlier pieces wrote places < c0 <= src(c) only.  Every lane is therefore read
// as it was before the call.  The walk starts at the first place whose content changes: nothing in front of it is
// written, not even with its own value.  The argument speaks of PLACES, not of arrays: the key column is a fourth array
// indexed by the same places, gathered by the same launch and copied back by a fourth copy behind the other three, so
// (a), (b) and (c) cover it unchanged.  So they do the admission column (adm: one byte per place, nullptr without it),
// gathered by the same launch -- thread t stores the one byte st_adm[t], so no two lanes write one staging byte and
// nothing outside [0, cnt) is written -- and copied back by one more copy behind the others.
//
// The 49-byte stride.  The staging of a piece starts dword-aligned (each 49-byte part of it does), so the piece is a
// column of agx_put49 with d0 = 0, d1 = 49 cnt and lane t at place t; the next lane's source is the column at
// src(c + 1).  The source 49 src(c) starts anywhere mod 4: ld_u32_any reads the one or two aligned dwords a misaligned
// one lies in (never past the dword that holds its last byte, so never outside the column).  The copy back lands at
// byte 49 c0 of the column, any alignment.
__global__ void __launch_bounds__(256)
agx_k_move(const u32 *__restrict__ kept, size_t shift, size_t c0, size_t cnt, const u64 *__restrict__ leaves,
           const u64 *__restrict__ scal, const u8 *__restrict__ wire, const u8 *__restrict__ keys,
           const u8 *__restrict__ adm, u64 *__restrict__ st_leaves, u64 *__restrict__ st_scal, u8 *__restrict__ st_wire,
           u8 *__restrict__ st_keys, u8 *__restrict__ st_adm) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= cnt) return;
    const size_t src = kept ? (size_t)kept[c0 + t] : c0 + t + shift;
    const ulonglong2 *l = reinterpret_cast<const ulonglong2 *>(leaves + 4 * src);
    const ulonglong2 *s = reinterpret_cast<const ulonglong2 *>(scal + 4 * src);
    const ulonglong2 l0 = l[0], l1 = l[1], s0 = s[0], s1 = s[1];
    ulonglong2 *dl = reinterpret_cast<ulonglong2 *>(st_leaves + 4 * t), *ds = reinterpret_cast<ulonglong2 *>(st_scal + 4 * t);
    dl[0] = l0;
    dl[1] = l1;
    ds[0] = s0;
    ds[1] = s1;
    // (the next lane's source is read only for the dword shared with it: then t + 1 < cnt)
    const size_t nsrc = t + 1 < cnt ? (kept ? (size_t)kept[c0 + t + 1] : src + 1) : src;
    agx_put49<true>(st_wire, 0, 49 * cnt, t, wire + 49 * src, wire + 49 * nsrc);
    if (keys) agx_put49<true>(st_keys, 0, 49 * cnt, t, keys + 49 * src, keys + 49 * nsrc);
    if (adm) st_adm[t] = adm[src];
}

// out[0] = the first place whose content a removal changes: the first c with kept[c] != c, or m when the m kept lanes
// are the first m (kept[c] - c never decreases, so exactly one c in [0, m] stands at that edge: one thread stores, no
// atomic).  *m_dev: the kept count behind av_k_keep_scan's offsets.  One thread per c in [0, n].
__global__ void __launch_bounds__(256)
agx_k_first_changed(const u32 *__restrict__ kept, const u32 *__restrict__ m_dev, size_t n, u32 *__restrict__ out) {
    const size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t m = *m_dev;
    if (c > n || c > m) return;
    const bool here = c == m || kept[c] != c, before = c > 0 && kept[c - 1] != c - 1;
    if (here && !before) out[0] = (u32)c;
}

// A selection (ssa_aggregator_finish_select, _remove_indices): order[0, m) names m DISTINCT places
// below `held`.  Whether it does is decided here, on the device, by every thread for its own index:
//   bits   one bit per held lane, cleared by the call in front of the launch; the thread of order[t] sets bit order[t]
//          with an atomic OR, and the value the OR returns says whether somebody set it before;
//   flag   one word, cleared with the bitmap, raised (atomic OR) for an index >= held or a bit that was already set.
// Of two threads that name the same place exactly one finds the bit set, whichever comes second: the flag ends up
// raised either way, and nothing else depends on which of them it was.
// -> the index is in range (a duplicate is: its lane may be read, the flag refuses the list as a whole).
static __device__ __forceinline__ bool agx_claim(u32 idx, size_t held, u32 *__restrict__ bits, u32 *__restrict__ flag) {
    if ((size_t)idx >= held) {
        atomicOr(flag, 1u);
        return false;
    }
    const u32 bit = 1u << (idx & 31u);
    if (atomicOr(bits + (idx >> 5), bit) & bit) atomicOr(flag, 1u);
    return true;
}

// The gather of a selection: one lane per selected position t.  The lane at place order[t] of the object is copied to
// place t of the STAGING (workspaces of the context: the selection reads the object and never writes it) -- leaf and
// scalar as in agx_k_move, the 49-byte columns by agx_put49 with d0 = 0, d1 = 49 m and lane t at place t.  The next
// lane's source is the column at order[t + 1]; the sources are in no order, which agx_put49 does not need: it reads
// `next` for the bytes of one shared dword only.
//
// Why no thread reads outside [0, held).  Every address into the object is formed from `src` or `nsrc`, and both have
// been compared with `held` first: a thread whose own index fails agx_claim returns before it forms any address (it
// reads nothing and writes nothing: the flag it raised makes the call zero its outputs), and a next index that is not
// below `held` is replaced by the thread's own, checked, index -- the bytes it then puts into the shared dword are wrong,
// in a list that is refused anyway.  ld_u32_any stays inside the column of the lane it is given (see agx_k_move), and the
// bitmap word idx >> 5 exists because idx < held.
__global__ void __launch_bounds__(256)
agx_k_select(const u32 *__restrict__ order, size_t m, size_t held, u32 *__restrict__ bits, u32 *__restrict__ flag,
             const u64 *__restrict__ leaves, const u64 *__restrict__ scal, const u8 *__restrict__ wire,
             const u8 *__restrict__ keys, u64 *__restrict__ st_leaves, u64 *__restrict__ st_scal, u8 *__restrict__ st_wire,
             u8 *__restrict__ st_keys) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= m) return;
    const u32 idx = order[t];
    if (!agx_claim(idx, held, bits, flag)) return;
    const size_t src = idx;
    const ulonglong2 *l = reinterpret_cast<const ulonglong2 *>(leaves + 4 * src);
    const ulonglong2 *s = reinterpret_cast<const ulonglong2 *>(scal + 4 * src);
    const ulonglong2 l0 = l[0], l1 = l[1], s0 = s[0], s1 = s[1];
    ulonglong2 *dl = reinterpret_cast<ulonglong2 *>(st_leaves + 4 * t), *ds = reinterpret_cast<ulonglong2 *>(st_scal + 4 * t);
    dl[0] = l0;
    dl[1] = l1;
    ds[0] = s0;
    ds[1] = s1;
    size_t nsrc = src;
    if (t + 1 < m) {
        const u32 nidx = order[t + 1];
        if ((size_t)nidx < held) nsrc = nidx;
    }
    agx_put49<true>(st_wire, 0, 49 * m, t, wire + 49 * src, wire + 49 * nsrc);
    if (st_keys) agx_put49<true>(st_keys, 0, 49 * m, t, keys + 49 * src, keys + 49 * nsrc);
}

// The same decision without a gather (ssa_aggregator_remove_indices): one thread per listed index.
__global__ void __launch_bounds__(256)
agx_k_mark(const u32 *__restrict__ order, size_t m, size_t held, u32 *__restrict__ bits, u32 *__restrict__ flag) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < m) (void)agx_claim(order[t], held, bits, flag);
}

// The bitmap as the byte mask ssa_aggregator_remove_device takes: mask[i] = 1 iff bit i is set.  One thread per held lane.
__global__ void __launch_bounds__(256)
agx_k_bits_to_mask(const u32 *__restrict__ bits, size_t held, u8 *__restrict__ mask) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < held) mask[i] = (u8)((bits[i >> 5] >> (i & 31u)) & 1u);
}

// Behind a selection's copies: *result = 0 for a valid list, 1 for a refused one, and a refused list's outputs -- n_agg
// bytes at agg, n_keys bytes at keys (nullptr: none), at any alignment -- are zeroed, the way ssa_aggregates_many refuses
// an aggregate.  A valid list costs every thread one read of the flag.  Grid-stride over bytes.
__global__ void __launch_bounds__(256)
agx_k_select_verdict(const u32 *__restrict__ flag, u8 *__restrict__ agg, size_t n_agg, u8 *__restrict__ keys, size_t n_keys,
                     u32 *__restrict__ result) {
    const u32 bad = *flag ? 1u : 0u;
    const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x, step = (size_t)gridDim.x * blockDim.x;
    if (g == 0) *result = bad;
    if (!bad) return;
    for (size_t b = g; b < n_agg; b += step) agg[b] = 0;
    if (keys)
        for (size_t b = g; b < n_keys; b += step) keys[b] = 0;
}

// The leaf column in the caller's order (ssa_aggregator_leaves_select): out[t] = the leaf at place
// order[t], four words into a dword-aligned workspace of the context.  The range check dominates the read: a thread
// whose index is not below `held` raises the flag (atomic OR, as agx_claim does) and returns before it forms an address;
// agx_k_select_verdict then zeroes the output.  A place named twice is copied twice: whether a list may repeat a place
// is finish_select's business.
__global__ void __launch_bounds__(256)
agx_k_leaves_select(const u32 *__restrict__ order, size_t m, size_t held, u32 *__restrict__ flag,
                    const u64 *__restrict__ leaves, u64 *__restrict__ out) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= m) return;
    const u32 idx = order[t];
    if ((size_t)idx >= held) {
        atomicOr(flag, 1u);
        return;
    }
    const ulonglong2 *l = reinterpret_cast<const ulonglong2 *>(leaves + 4 * (size_t)idx);
    const ulonglong2 l0 = l[0], l1 = l[1];
    ulonglong2 *d = reinterpret_cast<ulonglong2 *>(out + 4 * t);
    d[0] = l0;
    d[1] = l1;
}

// ---- the leaf index (SSA_AGGR_HOLD_INDEX): which place holds this leaf?
// The table of ssa_dedup.hpp over the leaf column: `slots` 64-bit words, a power of two and at least four per lane of
// the capacity, all ones = empty, otherwise (fingerprint's upper half << 32) | place.  The fingerprint is dd_fingerprint
// under the context's random key over the leaf's four words and one constant word (33 bytes: dd_fingerprint wants a
// partly filled last word); it only picks slots.  Whether a place holds an id is decided on the 32 bytes, always.
//
// A source of ssa_dedup.hpp over the leaf column (the rows of the index) and over the caller's ids (the lanes of a
// look-up: any byte alignment, read by u64 when the base is 8-aligned -- then every id is, at 32 bytes apart -- and byte
// by byte otherwise, as dd_key_word reads a key).
constexpr u64 AGI_TAG = 0xA4;
struct AgiLeafRows {
    static constexpr int WORDS = 5, BYTES = 33;
    const u64 *leaves;
    SSA_DEV u64 word(size_t p, int k) const { return k < 4 ? leaves[4 * p + k] : AGI_TAG; }
};
struct AgiIdLanes {
    static constexpr int WORDS = 5, BYTES = 33;
    const u8 *ids;
    bool aligned;
    SSA_DEV u64 word(size_t i, int k) const {
        const u8 *p = ids + 32 * i + 8 * k;
        return k < 4 ? (aligned ? *reinterpret_cast<const u64 *>(p) : ld_u64_le(p)) : AGI_TAG;
    }
};

// The insert: one thread per place p in [lo, hi).  The walk starts at fp & mask and takes at most `bound` slots:
//   an empty slot       is claimed by compare-and-swap with tag << 32 | p;
//   a slot of my tag whose owner o < hi holds my four words   is my leaf's slot: atomicMin of the 64-bit word with mine
//                       -- the upper halves are equal, so the lower PLACE wins -- and the walk ends;
//   anything else       moves on to the next slot.
// A lane that finds neither within the bound is counted in *over (one atomicAdd of the ballot's popcount per wave) and
// is in no slot: a look-up answers "unknown" for its leaf unless a lower place holds the same leaf.
//
// Memory model (the argument of ssa_dedup.hpp, with one more transition).  Between the workgroups of a launch nothing
// is exchanged but the slot words, through agent-scope atomics only.  The leaves read behind a slot word -- places below
// hi -- were written by an earlier launch on the same stream (agx_k_append, or the copies of a removal).  A slot word
// goes from empty to owned, and from there only to a LOWER owner of the SAME leaf (atomicMin between lanes that have
// compared all four words): whatever value a thread reads, now or stale, is the place of a lane that holds the leaf the
// slot stands for, so a comparison against it decides rightly, and a stale "empty" costs one failed swap.
//
// Why the result does not depend on the order in which the waves arrive.  Lanes with equal leaves have equal
// fingerprints and walk the same chain of slots from the same start under the same bound.  A slot never becomes empty
// again and never changes the leaf it stands for, so a chain only grows at its end: every slot a lane passed stays a
// slot another lane of the same leaf passes too.  Of the lanes of one leaf, whichever reaches the first slot that is
// empty or already theirs claims it, and every other one finds it there; atomicMin then leaves the lowest place among
// them, in any order.  Lanes [0, lo) were inserted by earlier launches and are below every p of this one, so an
// incremental insert never lowers an owner and leaves what a rebuild over [0, hi) would.  (WHICH leaves run into the
// probe bound may depend on the order -- it decides who stands where in a shared chain; with the default bound at load
// <= 1/4 none does.  Such a leaf is answered "unknown", never with a wrong place.)
__global__ void __launch_bounds__(256)
agi_k_insert(const u64 *__restrict__ leaves, u32 lo, u32 hi, u64 k0, u64 k1, u64 *__restrict__ slots, u32 mask, u32 bound,
             unsigned long long *__restrict__ over) {
    const u32 p = lo + blockIdx.x * DD_BLOCK + threadIdx.x;
    const AgiLeafRows rows{leaves};
    bool lost = false;
    if (p < hi) {
        const ulonglong2 *l = reinterpret_cast<const ulonglong2 *>(leaves + 4 * (size_t)p);
        const ulonglong2 l0 = l[0], l1 = l[1];
        const u64 w[AgiLeafRows::WORDS] = {l0.x, l0.y, l1.x, l1.y, AGI_TAG};
        const u64 fp = dd_fingerprint_of<AgiLeafRows>(w, k0, k1);
        const u64 tag = fp >> 32, mine = (tag << 32) | (u64)p;
        u32 s = (u32)fp & mask;
        lost = true;
#pragma unroll 1
        for (u32 t = 0; t < bound; t++) {
            u64 cur = __hip_atomic_load(slots + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (cur == DD_EMPTY) {
                cur = atomicCAS((unsigned long long *)(slots + s), (unsigned long long)DD_EMPTY, (unsigned long long)mine);
                if (cur == DD_EMPTY) {
                    lost = false;
                    break;
                }
            }
            const u32 o = (u32)cur;
            if ((cur >> 32) == tag && o < hi && dd_same_key(rows, o, w)) {       // my leaf's slot: the bytes decided
                atomicMin((unsigned long long *)(slots + s), (unsigned long long)mine);
                lost = false;
                break;
            }
            s = (s + 1u) & mask;
        }
    }
    const unsigned long long losts = __ballot(lost);
    if ((threadIdx.x & 63u) == 0 && losts) atomicAdd(over, (unsigned long long)__popcll(losts));
}

// The look-up: one thread per id, the same walk, read-only.  places[i] = the owner of the first slot of the id's tag
// whose owner holds the id's four words, or SSA_AGGV_UNKNOWN at an empty slot or at the bound.  An owner is used as an
// index only after it compared below `indexed` -- the lanes the table was built over, all written by earlier launches --
// so no thread reads outside the leaf column whatever a slot word holds.  No slot is written: the launch exchanges
// nothing between its threads but the count, *n_unknown += the ballot's popcount, once per wave (cleared by the call in
// front of the launch).  places and n_unknown are 4-byte aligned (the call checks).
__global__ void __launch_bounds__(256)
agi_k_lookup(const u8 *__restrict__ ids, u32 n, const u64 *__restrict__ leaves, u32 indexed, u64 k0, u64 k1,
             const u64 *__restrict__ slots, u32 mask, u32 bound, u32 *__restrict__ places, u32 *__restrict__ n_unknown) {
    const u32 i = blockIdx.x * DD_BLOCK + threadIdx.x;
    const AgiIdLanes lanes{ids, ((size_t)ids & 7u) == 0};
    const AgiLeafRows rows{leaves};
    bool unknown = false;
    if (i < n) {
        u64 w[AgiIdLanes::WORDS];
        dd_load(lanes, i, w);
        const u64 fp = dd_fingerprint_of<AgiIdLanes>(w, k0, k1);
        const u64 tag = fp >> 32;
        u32 s = (u32)fp & mask, place = SSA_AGGV_UNKNOWN;
#pragma unroll 1
        for (u32 t = 0; t < bound; t++) {
            const u64 cur = __hip_atomic_load(slots + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (cur == DD_EMPTY) break;
            const u32 o = (u32)cur;
            if ((cur >> 32) == tag && o < indexed && dd_same_key(rows, o, w)) {      // the bytes decide
                place = o;
                break;
            }
            s = (s + 1u) & mask;
        }
        places[i] = place;
        unknown = place == SSA_AGGV_UNKNOWN;
    }
    const unsigned long long unknowns = __ballot(unknown);
    if ((threadIdx.x & 63u) == 0 && unknowns) atomicAdd(n_unknown, (u32)__popcll(unknowns));
}

// The block-time hot path: one lane per held lane of a piece.  Lane i (place lane0 + i of the aggregate) derives its
// coefficient out of H(root || lane0 + i || 0xA3) (one permutation; ag_coeff_of_digest), multiplies the stored scalar by
// it and the workgroup sums: partials[b] = sum over workgroup b of a_i e_i mod q.  The coefficients never travel through
// memory.
// scal: the piece's scalars, four words per lane.
// (the lane's term, a_place e mod q with e the four words at `scal4`, is agx_coeff_term: the known fold of the streaming
// aggregate verifier, agv_k_known_fold in ssa_aggverifier.hpp, sums the same term over the lanes it took from a pool)
SSA_DEV sc256 agx_coeff_term(u64 *A, const DevParams *__restrict__ prm, const u64 *__restrict__ root, u64 place,
                             const u64 *__restrict__ scal4) {
    u64 in[8], d[4];
#pragma unroll
    for (int k = 0; k < 4; k++) in[k] = root[k];
    in[4] = place;
    in[5] = AG_TAG_COEFF;
    in[6] = in[7] = 0;
    ag_hash8(A, prm, in, 6u, d);
    sc256 a, e;
    ag_coeff_of_digest(d, a.w[0], a.w[1]);
    a.w[2] = a.w[3] = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) e.w[k] = scal4[k];
    return sc_mul_mod(a, e);
}

__global__ void __launch_bounds__(256, 4)
agx_k_coeff_fold(const DevParams *__restrict__ prm, const u64 *__restrict__ root, const u64 *__restrict__ scal, size_t n,
                 u64 lane0, u64 *__restrict__ partials) {
    __shared__ u64 lds[RS_LDS_U64];
    __shared__ u64 red[256 * 4];
    u64 *A = lds + threadIdx.x;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    sc256 ae;
#pragma unroll
    for (int k = 0; k < 4; k++) ae.w[k] = 0;
    if (i < n) ae = agx_coeff_term(A, prm, root, lane0 + (u64)i, scal + 4 * i);
    ag_block_sum(red, ae);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < 4; k++) partials[4 * (size_t)blockIdx.x + k] = red[k];
    }
}
#endif  // SSA_NO_KERNELS

}  // namespace ssa
