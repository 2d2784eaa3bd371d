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
//
//   push    status vector (the screen of ssa_verify_batch_screened, or the checks of ag_k_fold) -> av_keep lists the kept
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
//
// The object's four arrays are its own allocations (released by destroy, or by the context's clean-up): they are not in
// the context's list of workspaces, and nothing the object needs between two calls lives in one.
#pragma once
#include "ssa_aggregate.hpp"
#include "ssa_ctx.hpp"

// What the streaming aggregator and the streaming aggregate verifier (ssa_aggverifier.hpp) both are: lanes in arrival
// order, their leaves, and the tops of the complete blocks of B.
struct AgxStore {
    ssa_ctx *ctx = nullptr;   // nullptr: the context is gone, the device memory went with it
    size_t capacity = 0, block = 0, held = 0;     // block: B, a power of two from 2 to AG_TREE_SPAN
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
    uint64_t offered = 0, dropped = 0;
    DevBuf wire, scal;
};
// everything the object will ever hold, in the order it is allocated and released
static inline std::vector<AgxStore::Buf> agx_bufs(ssa_aggregator &a) {
    return {{&a.wire, 49 * a.capacity + 32}, {&a.scal, 32 * a.capacity}, {&a.leaves, 32 * a.capacity}, {&a.tops, 32 * a.n_tops()}};
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

// One lane per kept lane: rank c, source lane kept[c] of the push, place held + c of the aggregate.
//   leaves[held + c] = H(d || flag byte of R || 0xA1) from the lane's raw digest (the body of ag_k_leaf);
//   scal[held + c]   = e as four words;
//   wire[49 (held + c), + 49) = R.
// The R's of a push land on bytes [D0, D1) = [49 held, 49 (held + m)) of `wire` (the object's own allocation: wire itself
// is dword-aligned), which start and end anywhere mod 4.  A dword belongs to the lane its FIRST byte lies in, so lane c
// writes the aligned dwords that start in [49 (held + c), 49 (held + c + 1)) -- the last of them may run into lane c + 1's
// R and takes those bytes from kept[c + 1] -- as dwords while they end within D1.  The two edges are bytes: lane 0 writes
// [D0, the first aligned address), the last lane what is left behind the last whole dword.  So no two threads write one
// dword, and no byte in front of D0 -- the R's of earlier pushes -- is written.
__global__ void __launch_bounds__(256, 4)
agx_k_append(const DevParams *__restrict__ prm, const u8 *__restrict__ sigs, const u64 *__restrict__ dig,
             const u32 *__restrict__ kept, size_t m, size_t held, u64 *__restrict__ leaves, u64 *__restrict__ scal,
             u8 *__restrict__ wire) {
    __shared__ u64 lds[RS_LDS_U64];
    u64 *A = lds + threadIdx.x;
    const size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= m) return;
    const size_t src = kept[c], dst = held + c;
    const u8 *sig = sigs + 81 * src;
    u64 d[4];
    ag_leaf_hash(A, prm, dig, sigs, src, d);
    const sc256 e = ld_sc(sig + 49);
#pragma unroll
    for (int k = 0; k < 4; k++) {
        leaves[4 * dst + k] = d[k];
        scal[4 * dst + k] = e.w[k];
    }
    const size_t lo = 49 * dst, hi = lo + 49, end = 49 * (held + m);
    size_t w = (lo + 3) & ~(size_t)3;
    if (c == 0)
        for (size_t b = lo; b < w && b < end; b++) wire[b] = sig[b - lo];
    const u8 *next = c + 1 < m ? sigs + 81 * (size_t)kept[c + 1] : sig;     // (read only where c + 1 < m)
    for (; w < hi; w += 4) {
        if (w + 4 <= end) {
            u32 v = 0;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const size_t b = w + k;
                v |= (u32)(b < hi ? sig[b - lo] : next[b - hi]) << (8 * k);
            }
            *reinterpret_cast<u32 *>(wire + w) = v;
        } else {                                      // (the last lane alone: for every other one end >= hi + 49)
            for (size_t b = w; b < end; b++) wire[b] = sig[b - lo];
        }
    }
}

// Removing lanes (ssa_aggregator_drop_front, _remove).  The kept lanes, ascending, take the places
// 0, 1, 2, ...: kept lane c comes from place src(c) = kept[c] (a mask; the list of av_keep) or c + shift (a front drop:
// kept == nullptr, no list exists), and src(c) >= c, src ascending.  What a lane stores does not depend on its place, so
// the lane is MOVED: four words of leaves, four of scal, 49 bytes of wire.
//
// The hazard.  The move is in place, and the threads of a launch run in no order: with one lane dropped at the front
// every thread's source is its neighbour's destination.  So no launch writes the object.  The host walks the kept
// lanes in ascending pieces [c0, c1) of at most the context's MSM slice, and for each piece
//   1. agx_k_move gathers the piece -- reads the object at src(c), writes STAGING (workspaces of the context) at c - c0;
//   2. three stream-ordered device-to-device copies put the staging back on places [c0, c1);
//   3. only then is the next piece enqueued, on the same stream.
// Why that is right: (a) a piece's own sources were all read by step 1 before step 2 began (stream order), so step 2
// may overwrite them; (b) every later piece reads places src(c) >= c >= c1, and step 2 wrote [c0, c1) alone, so no
// later source has been overwritten; (c) earlier pieces wrote places < c0 <= src(c) only.  Every lane is therefore read
// as it was before the call.  The walk starts at the first place whose content changes: nothing in front of it is
// written, not even with its own value.
//
// The 49-byte stride.  The staging of a piece starts dword-aligned, so lane t owns the aligned dwords that START in
// [49 t, 49 (t + 1)) of it -- the rule of agx_k_append: the last of them may run into lane t + 1's R and takes those
// bytes from src(c + 1) -- written as dwords while they end within the piece's 49 cnt bytes; the last lane writes what
// is left behind the last whole dword as bytes.  No two threads write one dword.  The source 49 src(c) starts anywhere
// mod 4: ld_u32_any reads the one or two aligned dwords a misaligned one lies in (never past the dword that holds its
// last byte, so never outside `wire`).  The copy back lands at byte 49 c0 of wire, any alignment.
static __device__ __forceinline__ u32 ld_u32_any(const u8 *p) {
    const uintptr_t a = (uintptr_t)p;
    const u32 *q = reinterpret_cast<const u32 *>(a & ~(uintptr_t)3);
    const u32 sh = 8u * (u32)(a & 3u);
    const u32 lo = q[0];
    return sh ? (lo >> sh) | (q[1] << (32u - sh)) : lo;
}

__global__ void __launch_bounds__(256)
agx_k_move(const u32 *__restrict__ kept, size_t shift, size_t c0, size_t cnt, const u64 *__restrict__ leaves,
           const u64 *__restrict__ scal, const u8 *__restrict__ wire, u64 *__restrict__ st_leaves,
           u64 *__restrict__ st_scal, u8 *__restrict__ st_wire) {
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
    const size_t lo = 49 * t, hi = lo + 49, end = 49 * cnt;
    const u8 *r = wire + 49 * src;
    for (size_t w = (lo + 3) & ~(size_t)3; w < hi; w += 4) {
        if (w + 4 <= hi) {
            *reinterpret_cast<u32 *>(st_wire + w) = ld_u32_any(r + (w - lo));
        } else if (w + 4 <= end) {                    // the dword shared with lane t + 1 (then t + 1 < cnt)
            const u8 *next = wire + 49 * (kept ? (size_t)kept[c0 + t + 1] : src + 1);
            u32 v = 0;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const size_t b = w + k;
                v |= (u32)(b < hi ? r[b - lo] : next[b - hi]) << (8 * k);
            }
            *reinterpret_cast<u32 *>(st_wire + w) = v;
        } else {                                      // (the last lane alone: for every other one end >= hi + 49)
            for (size_t b = w; b < end; b++) st_wire[b] = r[b - lo];
        }
    }
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

// The block-time hot path: one lane per held lane of a piece.  Lane i (place lane0 + i of the aggregate) derives its
// coefficient out of H(root || lane0 + i || 0xA3) (one permutation; ag_coeff_of_digest), multiplies the stored scalar by
// it and the workgroup sums: partials[b] = sum over workgroup b of a_i e_i mod q.  The coefficients never travel through
// memory.
// scal: the piece's scalars, four words per lane.
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
    if (i < n) {
        u64 in[8], d[4];
#pragma unroll
        for (int k = 0; k < 4; k++) in[k] = root[k];
        in[4] = lane0 + (u64)i;
        in[5] = AG_TAG_COEFF;
        in[6] = in[7] = 0;
        ag_hash8(A, prm, in, 6u, d);
        sc256 a, e;
        ag_coeff_of_digest(d, a.w[0], a.w[1]);
        a.w[2] = a.w[3] = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) e.w[k] = scal[4 * i + k];
        ae = sc_mul_mod(a, e);
    }
    ag_block_sum(red, ae);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < 4; k++) partials[4 * (size_t)blockIdx.x + k] = red[k];
    }
}
#endif  // SSA_NO_KERNELS

}  // namespace ssa
