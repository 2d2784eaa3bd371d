// Internal: the streaming aggregate verifier (ssa_aggverifier_*), the validator's counterpart of the
// streaming aggregator (ssa_aggregator.hpp).  A validator receives a block body -- R's, keys, messages -- before it can
// verify the half-aggregate: the coefficients need the root, and the root needs the last R.  Everything in front of the
// coefficients is independent of a lane's place -- the challenge hash, the leaf, the checks and the Fp6 square root of
// msm_k_prepare, and every complete aligned block of B = 2^t leaves -- so it is done when the lanes arrive, and the object
// keeps the results on the device, in arrival order:
//
//   rpts    12 words per lane: R decompressed, the affine row msm_k_prepare would store ((0, 0): identity or failed lane)
//   ppts    12 words per lane: -P canonical, as msm_k_prepare stores it ((0, 0): pk_inf or failed lane)
//   h       four words per lane: the challenge scalar mod q
//   leaves  four words per lane: leaf_i
//   bad     one byte per lane: nonzero iff the lane failed one of msm_k_prepare's checks
//   tops    four words per COMPLETE block of B lanes: the top of its subtree
//   kst     one byte per lane: the status of the lane's key as the key cache gave it (0, SSA_INVALID_PUBLIC_KEY,
//           SSA_MALFORMED), 0 = "not checked" for a lane of a plain push.  RULE: kst is read only
//           while the host flag `keyed` is on, and then every byte of kst[0, held) has been written by the push that
//           brought its lane.  `keyed` turns on at the first push through a cache, which zeroes kst[0, held) on the
//           context's stream first; from then on the cached pushes write their lanes' bytes through agc_k_expand and
//           the plain push writes its n bytes with one hipMemsetAsync (a mixed push: zeros in its classification, and,
//           through a cache, the unknown lanes' statuses by agv_k_kst_at behind them); reset turns it off.  So bytes that a failed push
//           left behind `held`, or that an earlier life of the object left anywhere, are overwritten before they can be
//           read as a status, and an object that never sees a cached push enqueues exactly what it did without kst.
//
//   push    ag_transcript_front (expand to stride 81, ONE ssa_k_hash: raw digests and scalars mod q) -> agv_k_append
//           stores leaf, scalar, the two point rows and the bad byte of each lane -> the blocks this push completed are
//           reduced to their tops (agx_reduce_blocks, shared with the aggregator).  Every lane is appended: a validator
//           cannot drop one, place is part of the transcript.
//   finish  for the first n held lanes: stored tops, the ragged block and ags_root as the aggregator's finish; per piece of
//           at most one MSM slice agv_k_scalars derives a_i, writes the digits of a_i and a_i h_i and copies the stored
//           rows into the MSM's workspaces; sort, buckets and reduce run unchanged (ssa_internal_msm_record_prepared); the
//           pieces' records are added up and compared exactly with [e_agg]G (ag_k_finish_scalar).  finish changes nothing
//           in the object.  A keyed object then folds kst[0, n) into the verdict word (agv_k_key_verdict): the key
//           decides, as in ssa_verify_aggregates_many_cached.  The key status never enters the MSM: the record is the same.
//
//   known   one byte per lane: 1 iff the lane was taken from a streaming aggregator of the same context by a mixed push
//           (DESIGN.md section 34).  Such a lane holds the pool's leaf, the pool's scalar s_i IN ITS h SLOT, the (0, 0)
//           sentinels in both rows, bad = 0 (1: its place was refused on the device) and key status 0.  RULE: as kst's,
//           with the host flag `mixed`: it turns on at the first mixed push, which zeroes known[0, held) first; from then
//           on a mixed push writes its lanes' bytes (agv_k_classify) and every other push zeroes its n bytes; reset
//           turns it off.  An object that never sees a mixed push enqueues exactly what it did without the array.
//
//   push_mixed  agv_k_classify (a known lane: leaf and scalar gathered from the pool, sentinels, bytes; every lane: a
//           keep byte) -> av_keep lists the unknown positions -> ag_transcript_front over the u unknown lanes the call
//           brought -> agv_k_append_at, the body of agv_k_append with lane j at place held + pos[j] -> agv_k_mixed_close
//           (the result word; a sentinel count other than u marks every lane bad) -> agx_reduce_blocks.
//   finish  with a known lane in the prefix: the root as always; av_keep lists the prefix's unknown places from the known
//           bytes; agv_k_scalars_at fills the bucket pipeline through that list (u_cap rows, known on the host; rows
//           behind the device's count are sentinels with zero digits); agv_k_known_fold sums S = sum a_i s_i over the
//           known lanes (the term of agx_k_coeff_fold at the lane's true place); agv_k_known_close hands
//           e_agg - S mod q to ag_k_finish_scalar, or, with no unknown lane at all, writes the verdict itself.
//
//   push_mixed_cached   the u compact keys through the key cache first, slice by slice as a cached
//           push's (agc_begin, agc_slices: the dense statuses into ctx->agc_kst, wire keys expanded into the context's
//           buffers), then push_mixed over the expanded keys with two differences: the classification also reads the
//           pool's admission class of a known lane and refuses one below `require` as it refuses a place out of range
//           (agv_k_classify_adm; bit 1 of the flag word), and behind agv_k_append_at agv_k_kst_at scatters the dense
//           statuses to the lanes' true places, kst[held + pos[j]] = status[j] -- behind agv_k_classify_adm on the same
//           stream, which wrote zeros there.  The first such push turns `keyed` on by kst's rule.  The host forms
//           with require > 0 run agv_k_require over the uploaded places and read its word before anything is touched.
//
// The object's eight arrays are its own allocations (released by destroy, or by the context's clean-up): they are not in
// the context's list of workspaces, and nothing the object needs between two calls lives in one.
#pragma once
#include "ssa_aggcache.hpp"
#include "ssa_aggregator.hpp"

struct ssa_aggverifier : AgxStore {
    static constexpr uint32_t kCreateFlags = 0;
    uint64_t pushed = 0, cached = 0;              // cached: lanes pushed through a key cache
    bool keyed = false;                           // kst[0, held) is valid and finish folds it (the rule above)
    bool mixed = false;                           // known[0, held) is valid (the rule above)
    // a push that took lanes from a pool: places [first, first + lanes), `unknown` of them came with the call
    struct MixedPush {
        uint64_t first, lanes, unknown;
    };
    std::vector<MixedPush> mixed_pushes;
    DevBuf rpts, ppts, h, bad, kst, known;
    // the prefix [0, n) holds a lane of a mixed push
    bool prefix_mixed(size_t n) const {
        for (const MixedPush &m : mixed_pushes)
            if (m.first < n) return true;
        return false;
    }
    // u_cap: at least the unknown lanes of [0, n) -- every lane outside the mixed pushes, and of a mixed push that begins
    // below n as many as it brought (or as many of its lanes as the prefix takes, if those are fewer)
    size_t unknown_cap(size_t n) const {
        size_t cap = n;
        for (const MixedPush &m : mixed_pushes)
            if (m.first < n) {
                const size_t in = (size_t)std::min<uint64_t>(m.lanes, n - m.first);
                cap -= in - (size_t)std::min<uint64_t>(m.unknown, in);
            }
        return cap;
    }
};
// everything the object will ever hold, in the order it is allocated and released
static inline std::vector<AgxStore::Buf> agx_bufs(ssa_aggverifier &v) {
    return {{&v.rpts, 96 * v.capacity}, {&v.ppts, 96 * v.capacity}, {&v.h, 32 * v.capacity},  {&v.leaves, 32 * v.capacity},
            {&v.bad, v.capacity + 16},  {&v.tops, 32 * v.n_tops()}, {&v.kst, v.capacity + 16},
            {&v.known, v.capacity + 16}};
}

namespace ssa {

// lanes of kst one workgroup of agv_k_key_verdict folds: 256 threads x 16 bytes x 2 steps.  2^20 lanes are 128
// workgroups; a multiple of 4096, so that every span but the last is whole 16-byte steps of the whole workgroup.
constexpr u32 AGV_KST_SPAN = 8192;
static_assert(AGV_KST_SPAN % 4096 == 0, "whole steps of 256 threads x 16 bytes");

#ifndef SSA_NO_KERNELS
// One lane per pushed lane: lane i of the push (sigs: its R's at stride 81 with e = 0, as ag_k_expand lays them out),
// place held + i of the object.
//   leaves[held + i] = H(d || flag byte of R || 0xA1) from the lane's raw digest (the body of ag_k_leaf);
//   h[held + i]      = the challenge scalar mod q;
//   rpts / ppts      = the rows msm_k_prepare stores for the lane: its checks (msm_lane_key, msm_lane_decode), R's
//                      square root, the (0, 0) sentinels, -P canonical;
//   bad[held + i]    = 1 iff a check failed.
// (the lane's body, written once: lane i of the push goes to place dst of the object)
static __device__ __forceinline__ void
agv_append_lane(u64 *A, const DevParams *__restrict__ prm, const u8 *__restrict__ sigs, const u8 *__restrict__ pks,
                const u8 *__restrict__ pk_inf, const u64 *__restrict__ dig, const u64 *__restrict__ h_in, size_t i,
                size_t dst, u64 *__restrict__ leaves, u64 *__restrict__ h, u64 *__restrict__ rpts, u64 *__restrict__ ppts,
                u8 *__restrict__ bad) {
    u64 d[4];
    ag_leaf_hash(A, prm, dig, i, sigs[81 * i + 48], d);
#pragma unroll
    for (int k = 0; k < 4; k++) {
        leaves[4 * dst + k] = d[k];
        h[4 * dst + k] = h_in[4 * i + k];
    }
    // (msm_k_prepare also wants e < q between the two steps: here e is the 32 zero bytes ag_k_expand wrote)
    bool ok = true, r_inf;
    aff P, R;
    msm_lane_key(pks, i, P, ok);
    const bool p_inf = pk_inf && pk_inf[i];
    ok = msm_lane_decode(ok, p_inf, P, sigs + 81 * i, R, r_inf);
    if (!ok || r_inf) {       // a failed lane, or an identity R: the (0, 0) sentinel jac_madd skips
        R.x = f6_zero();
        R.y = f6_zero();
    }
    if (!ok || p_inf) {
        P.x = f6_zero();
        P.y = f6_zero();
    }
    P.y = f6_canon(f6_neg(P.y));
    st_aff_row(rpts + 12 * dst, R);
    st_aff_row(ppts + 12 * dst, P);
    bad[dst] = (u8)(ok ? 0u : 1u);
}

__global__ void __launch_bounds__(256)
agv_k_append(const DevParams *__restrict__ prm, const u8 *__restrict__ sigs, const u8 *__restrict__ pks,
             const u8 *__restrict__ pk_inf, const u64 *__restrict__ dig, const u64 *__restrict__ h_in, size_t n, size_t held,
             u64 *__restrict__ leaves, u64 *__restrict__ h, u64 *__restrict__ rpts, u64 *__restrict__ ppts,
             u8 *__restrict__ bad) {
    __shared__ u64 lds[RS_LDS_U64];
    u64 *A = lds + threadIdx.x;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    agv_append_lane(A, prm, sigs, pks, pk_inf, dig, h_in, i, held + i, leaves, h, rpts, ppts, bad);
}

// The append of a mixed push: the u lanes the call brought stand side by side, and lane j goes to
// place held + pos[j], pos the ascending list of the push's unknown positions (av_k_keep_list over agv_k_classify's keep
// bytes: every entry is below the n of the push, so below capacity - held) and *m_dev its length.  j >= *m_dev: the list
// names no place for the lane (the push is refused as a whole by agv_k_mixed_close) and nothing is read or written.
__global__ void __launch_bounds__(256)
agv_k_append_at(const DevParams *__restrict__ prm, const u8 *__restrict__ sigs, const u8 *__restrict__ pks,
                const u8 *__restrict__ pk_inf, const u64 *__restrict__ dig, const u64 *__restrict__ h_in, size_t u,
                const u32 *__restrict__ pos, const u32 *__restrict__ m_dev, size_t held, u64 *__restrict__ leaves,
                u64 *__restrict__ h, u64 *__restrict__ rpts, u64 *__restrict__ ppts, u8 *__restrict__ bad) {
    __shared__ u64 lds[RS_LDS_U64];
    u64 *A = lds + threadIdx.x;
    const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= u || j >= (size_t)*m_dev) return;
    agv_append_lane(A, prm, sigs, pks, pk_inf, dig, h_in, j, held + (size_t)pos[j], leaves, h, rpts, ppts, bad);
}

// The first launch of a mixed push: one thread per position i of the push, place held + i of the object.
//   places[i] == AGV_UNKNOWN      keep[i] = 0 (av_keep lists the zero bytes): the lane came with the call and
//                                 agv_k_append_at fills it.  Until then it is an empty lane: zero leaf, zero scalar,
//                                 sentinel rows -- so a refused push, whose list names no place for it, leaves nothing
//                                 undefined behind.
//   places[i] < ag_held           a known lane: leaf and scalar of the pool's lane places[i], two 16-byte words each (the
//                                 scalar into the h slot: with sentinel rows no digit of a_i h_i is ever formed from it),
//                                 the (0, 0) sentinels in both rows, bad = 0.
//   anything else                 refused: as a known lane, with zeros for leaf and scalar, bad = 1 and the flag raised.
// The range check dominates every read, as in agx_k_select: `src` is formed only from a place that compared below
// ag_held, and a thread whose place fails forms no address into the pool.  known[.] = 1 for every lane that is not
// unknown; kst (nullptr: the object is not keyed) = 0, "not checked", for every lane.
constexpr u32 AGV_UNKNOWN = 0xFFFFFFFFu;
// (the body, written once.  ADM: the push requires an admission class -- adm is the pool's admission column, one byte
// per place, and a known lane with adm[p] < require is refused as a place out of range is, raising bit 1 of *flag where
// that raises bit 0.  adm[p] is read only for a place that compared below ag_held: the rule above covers it.)
template <bool ADM>
static __device__ __forceinline__ void
agv_classify_lane(const u32 *__restrict__ places, size_t n, size_t held, size_t ag_held, const u64 *__restrict__ ag_leaves,
                  const u64 *__restrict__ ag_scal, const u8 *__restrict__ adm, u32 require, u64 *__restrict__ leaves,
                  u64 *__restrict__ h, u64 *__restrict__ rpts, u64 *__restrict__ ppts, u8 *__restrict__ bad,
                  u8 *__restrict__ kst, u8 *__restrict__ known, u8 *__restrict__ keep, u32 *__restrict__ flag) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const u32 p = places[i];
    const bool unknown = p == AGV_UNKNOWN, in_range = !unknown && (size_t)p < ag_held;
    bool below = false;
    if (ADM && in_range) below = (u32)adm[p] < require;
    const bool taken = in_range && !below;
    const ulonglong2 zero = make_ulonglong2(0, 0);
    ulonglong2 l0 = zero, l1 = zero, s0 = zero, s1 = zero;
    if (taken) {
        const size_t src = p;
        const ulonglong2 *l = reinterpret_cast<const ulonglong2 *>(ag_leaves + 4 * src);
        const ulonglong2 *s = reinterpret_cast<const ulonglong2 *>(ag_scal + 4 * src);
        l0 = l[0];
        l1 = l[1];
        s0 = s[0];
        s1 = s[1];
    }
    const size_t dst = held + i;
    ulonglong2 *dl = reinterpret_cast<ulonglong2 *>(leaves + 4 * dst), *dh = reinterpret_cast<ulonglong2 *>(h + 4 * dst);
    dl[0] = l0;
    dl[1] = l1;
    dh[0] = s0;
    dh[1] = s1;
    ulonglong2 *rd = reinterpret_cast<ulonglong2 *>(rpts + 12 * dst), *pd = reinterpret_cast<ulonglong2 *>(ppts + 12 * dst);
#pragma unroll
    for (int k = 0; k < 6; k++) {
        rd[k] = zero;
        pd[k] = zero;
    }
    const bool refused = !unknown && !taken;
    bad[dst] = (u8)(refused ? 1u : 0u);
    known[dst] = (u8)(unknown ? 0u : 1u);
    if (kst) kst[dst] = 0;
    keep[i] = (u8)(unknown ? 0u : 1u);
    if (refused) atomicOr(flag, below ? 2u : 1u);
}

__global__ void __launch_bounds__(256)
agv_k_classify(const u32 *__restrict__ places, size_t n, size_t held, size_t ag_held, const u64 *__restrict__ ag_leaves,
               const u64 *__restrict__ ag_scal, u64 *__restrict__ leaves, u64 *__restrict__ h, u64 *__restrict__ rpts,
               u64 *__restrict__ ppts, u8 *__restrict__ bad, u8 *__restrict__ kst, u8 *__restrict__ known,
               u8 *__restrict__ keep, u32 *__restrict__ flag) {
    agv_classify_lane<false>(places, n, held, ag_held, ag_leaves, ag_scal, nullptr, 0u, leaves, h, rpts, ppts, bad, kst, known,
                             keep, flag);
}

// The same launch for a push that requires an admission class (require is 1 or 2, adm the
// admission column of a pool created with SSA_AGGR_HOLD_ADMISSION, ag_held bytes of it written).
__global__ void __launch_bounds__(256)
agv_k_classify_adm(const u32 *__restrict__ places, size_t n, size_t held, size_t ag_held, const u64 *__restrict__ ag_leaves,
                   const u64 *__restrict__ ag_scal, const u8 *__restrict__ adm, u32 require, u64 *__restrict__ leaves,
                   u64 *__restrict__ h, u64 *__restrict__ rpts, u64 *__restrict__ ppts, u8 *__restrict__ bad,
                   u8 *__restrict__ kst, u8 *__restrict__ known, u8 *__restrict__ keep, u32 *__restrict__ flag) {
    agv_classify_lane<true>(places, n, held, ag_held, ag_leaves, ag_scal, adm, require, leaves, h, rpts, ppts, bad, kst, known,
                            keep, flag);
}

// The pre-check of the host forms with require > 0: one thread per position of the uploaded list, nothing but the word
// is written.  *flag (cleared in front) gets bit 1 for a known place whose class is below `require` and bit 0 for a
// place out of range (the host checked the range itself: cannot be).  adm[p] is read only for p < ag_held.
__global__ void __launch_bounds__(256)
agv_k_require(const u32 *__restrict__ places, size_t n, size_t ag_held, const u8 *__restrict__ adm, u32 require,
              u32 *__restrict__ flag) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const u32 p = places[i];
    if (p == AGV_UNKNOWN) return;
    if ((size_t)p >= ag_held) {
        atomicOr(flag, 1u);
        return;
    }
    if ((u32)adm[p] < require) atomicOr(flag, 2u);
}

// Behind agv_k_append_at in a mixed push through a key cache: the key status of compact lane j, status[j] as
// agc_k_expand wrote it, goes to the lane's true place, kst[pos[j]] (kst: the object's array from lane `held` on; pos
// and *m_dev as in agv_k_append_at: every entry below the n of the push).  j >= *m_dev: no place, nothing is written --
// the push is refused as a whole.  Distinct j have distinct pos[j]: no two threads write one byte.
__global__ void __launch_bounds__(256)
agv_k_kst_at(const u8 *__restrict__ status, size_t u, const u32 *__restrict__ pos, const u32 *__restrict__ m_dev,
             u8 *__restrict__ kst) {
    const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= u || j >= (size_t)*m_dev) return;
    kst[pos[j]] = status[j];
}

// The last launch of a mixed push before the tree: *result = 0 for a valid list; bit 0 for a refused one -- a place out
// of range raised bit 0 of *flag, or the list holds *m_dev sentinels where the caller announced u -- and bit 1 where a
// known lane was below the required class (bit 1 of *flag: agv_k_classify_adm alone raises it).  In the second case nobody knows
// which compact lane belongs where, so EVERY lane of the push is marked bad (behind agv_k_append_at on the stream, which
// writes the byte of the lanes it fills).  A valid list costs every thread two reads.  Grid-stride over the n lanes.
__global__ void __launch_bounds__(256)
agv_k_mixed_close(const u32 *__restrict__ m_dev, u32 u, const u32 *__restrict__ flag, size_t n, u8 *__restrict__ bad,
                  u32 *__restrict__ result) {
    const bool miscount = *m_dev != u;
    const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x, step = (size_t)gridDim.x * blockDim.x;
    if (g == 0) {
        const u32 f = *flag;
        *result = (miscount || (f & 1u) ? 1u : 0u) | (f & 2u);
    }
    if (!miscount) return;
    for (size_t i = g; i < n; i += step) bad[i] = 1;
}

// The block-time stage in front of the bucket pipeline: one lane per held lane of a piece of n lanes whose first stands at
// place lane0 of the aggregate (h, rpts, ppts, bad: the object's arrays from that lane on).  Lane i derives its coefficient
// out of H(root || lane0 + i || 0xA3) (one permutation; ag_coeff_of_digest) and writes what msm_k_prepare writes with a
// 16-byte coefficient and e = 0: the signed digits of a_i over the wa windows a coefficient reaches for point i, those of
// a_i h_i mod q over all windows for point n + i, and the two stored rows as points i and n + i.  A wave with a bad lane
// sets the malformed word: one ballot, one atomic.  The coefficients never travel through memory.
// (the lane's body, written once: row i of a piece of n rows is the held lane at `place` of the aggregate, whose scalar,
// rows and bad byte stand at h4, r12, p12 and *bad1.  Returns "the lane is bad".)
static __device__ __forceinline__ bool
agv_scalars_lane(u64 *A, const DevParams *__restrict__ prm, const u64 *__restrict__ root, u64 place,
                 const u64 *__restrict__ h4, const u64 *__restrict__ r12, const u64 *__restrict__ p12,
                 const u8 *__restrict__ bad1, size_t n, size_t i, MsmShape shp, u32 wa, u64 *__restrict__ points,
                 short *__restrict__ digits) {
    u64 in[8], d[4];
#pragma unroll
    for (int k = 0; k < 4; k++) in[k] = root[k];
    in[4] = place;
    in[5] = AG_TAG_COEFF;
    in[6] = in[7] = 0;
    ag_hash8(A, prm, in, 6u, d);
    sc256 a, hv;
    ag_coeff_of_digest(d, a.w[0], a.w[1]);
    a.w[2] = a.w[3] = 0;
    (void)write_signed_digits(a, shp.c, wa, digits, 2 * n, i);       // 126 bits: never carries out
#pragma unroll
    for (int k = 0; k < 4; k++) hv.w[k] = h4[k];
    (void)write_signed_digits(sc_mul_mod(a, hv), shp.c, shp.windows, digits, 2 * n, n + i);
    // a row is 96 bytes at a multiple of 96 from a device allocation: six 16-byte words
    const ulonglong2 *rs = reinterpret_cast<const ulonglong2 *>(r12);
    const ulonglong2 *ps = reinterpret_cast<const ulonglong2 *>(p12);
    ulonglong2 *rd = reinterpret_cast<ulonglong2 *>(points + 12 * i);
    ulonglong2 *pd = reinterpret_cast<ulonglong2 *>(points + 12 * (n + i));
#pragma unroll
    for (int k = 0; k < 6; k++) {
        rd[k] = rs[k];
        pd[k] = ps[k];
    }
    return *bad1 != 0;
}

__global__ void __launch_bounds__(256)
agv_k_scalars(const DevParams *__restrict__ prm, const u64 *__restrict__ root, const u64 *__restrict__ h,
              const u64 *__restrict__ rpts, const u64 *__restrict__ ppts, const u8 *__restrict__ bad, size_t n, u64 lane0,
              MsmShape shp, u32 wa, u64 *__restrict__ points, short *__restrict__ digits, u32 *__restrict__ malformed) {
    __shared__ u64 lds[RS_LDS_U64];
    u64 *A = lds + threadIdx.x;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool is_bad = false;
    if (i < n)
        is_bad = agv_scalars_lane(A, prm, root, lane0 + (u64)i, h + 4 * i, rpts + 12 * i, ppts + 12 * i, bad + i, n, i, shp,
                                  wa, points, digits);
    if (__ballot(is_bad) != 0 && (threadIdx.x & 63u) == 0) atomicOr(malformed, 1u);
}

// The same stage for a prefix that holds known lanes: the piece's n rows are rows
// [row0, row0 + n) of the list of the prefix's unknown places (av_k_keep_list over known[0, n_take): ascending, every
// entry below n_take) and *m_dev is the list's length.  Row row0 + i below *m_dev is the held lane at place
// p = list[row0 + i] -- h, rpts, ppts, bad are the object's arrays from lane 0 on -- with the coefficient of place p.  A
// row at or behind *m_dev (the host sized the launch by u_cap >= *m_dev) is an empty one: zero digits for both its
// points and the (0, 0) sentinels, which enter no bucket.
__global__ void __launch_bounds__(256)
agv_k_scalars_at(const DevParams *__restrict__ prm, const u64 *__restrict__ root, const u64 *__restrict__ h,
                 const u64 *__restrict__ rpts, const u64 *__restrict__ ppts, const u8 *__restrict__ bad,
                 const u32 *__restrict__ list, const u32 *__restrict__ m_dev, size_t row0, size_t n, MsmShape shp, u32 wa,
                 u64 *__restrict__ points, short *__restrict__ digits, u32 *__restrict__ malformed) {
    __shared__ u64 lds[RS_LDS_U64];
    u64 *A = lds + threadIdx.x;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool is_bad = false;
    if (i < n) {
        if (row0 + i < (size_t)*m_dev) {
            const size_t p = list[row0 + i];
            is_bad = agv_scalars_lane(A, prm, root, (u64)p, h + 4 * p, rpts + 12 * p, ppts + 12 * p, bad + p, n, i, shp, wa,
                                      points, digits);
        } else {
            sc256 z;
#pragma unroll
            for (int k = 0; k < 4; k++) z.w[k] = 0;
            (void)write_signed_digits(z, shp.c, wa, digits, 2 * n, i);
            (void)write_signed_digits(z, shp.c, shp.windows, digits, 2 * n, n + i);
            const ulonglong2 zero = make_ulonglong2(0, 0);
            ulonglong2 *rd = reinterpret_cast<ulonglong2 *>(points + 12 * i);
            ulonglong2 *pd = reinterpret_cast<ulonglong2 *>(points + 12 * (n + i));
#pragma unroll
            for (int k = 0; k < 6; k++) {
                rd[k] = zero;
                pd[k] = zero;
            }
        }
    }
    if (__ballot(is_bad) != 0 && (threadIdx.x & 63u) == 0) atomicOr(malformed, 1u);
}

// S = sum over the KNOWN lanes of the prefix of a_i s_i mod q, piece by piece as agx_k_coeff_fold: lane i of the piece
// is place lane0 + i; a lane whose known byte is zero adds nothing and pays no permutation; a known lane adds
// agx_coeff_term -- the term of agx_k_coeff_fold -- at its true place, with the pool's scalar from its h slot.  A wave
// with a known lane marked bad (a place refused on the device) raises *flag: one ballot, one atomic.  So does a list of
// unknown places longer than the u_cap rows the host sized the MSM by (*m_dev > u_cap: only a push whose sentinel count
// was refused can hold more unknown lanes than it announced): lanes the MSM will not see must not pass unseen.
// h, known, bad: the piece's, from its first lane on.
__global__ void __launch_bounds__(256, 4)
agv_k_known_fold(const DevParams *__restrict__ prm, const u64 *__restrict__ root, const u64 *__restrict__ h,
                 const u8 *__restrict__ known, const u8 *__restrict__ bad, size_t n, u64 lane0,
                 const u32 *__restrict__ m_dev, u32 u_cap, u64 *__restrict__ partials, u32 *__restrict__ flag) {
    __shared__ u64 lds[RS_LDS_U64];
    __shared__ u64 red[256 * 4];
    u64 *A = lds + threadIdx.x;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    sc256 ae;
#pragma unroll
    for (int k = 0; k < 4; k++) ae.w[k] = 0;
    bool is_bad = false;
    if (i < n && known[i] != 0) {
        ae = agx_coeff_term(A, prm, root, lane0 + (u64)i, h + 4 * i);
        is_bad = bad[i] != 0;
    }
    if (__ballot(is_bad) != 0 && (threadIdx.x & 63u) == 0) atomicOr(flag, 1u);
    if (blockIdx.x == 0 && threadIdx.x == 0 && *m_dev > u_cap) atomicOr(flag, 1u);
    ag_block_sum(red, ae);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < 4; k++) partials[4 * (size_t)blockIdx.x + k] = red[k];
    }
}

// ONE thread, between the known fold and the comparison.  e_agg, s32: 32 bytes each, little-endian (s32 canonical, from
// ag_k_fold_finish).
//   rec != nullptr   the unknown lanes' record exists: d32 = e_agg - S mod q for ag_k_finish_scalar, which compares the
//                    record with [d]G.  A non-canonical e_agg is handed on AS IT IS, so that the canonical check stays
//                    on e_agg itself; a raised *flag goes into the record's malformed word (rec[22]), where a bad
//                    unknown lane's already stands.
//   rec == nullptr   no unknown lane in the prefix, no MSM: the verdict is written here -- malformed for a raised flag
//                    or a non-canonical e_agg, else valid iff e_agg == S.
__global__ void __launch_bounds__(64)
agv_k_known_close(const u8 *__restrict__ e_agg, const u8 *__restrict__ s32, const u32 *__restrict__ flag,
                  u64 *__restrict__ rec, u8 *__restrict__ d32, u32 *__restrict__ verdict) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const sc256 e = ld_sc(e_agg), s = ld_sc(s32);
    const bool canonical = !sc_geq_q(e), raised = *flag != 0;
    const sc256 d = canonical ? sc_add_mod(e, sc_neg_mod(s)) : e;
    if (rec) {
        for (int b = 0; b < 32; b++) d32[b] = (u8)(d.w[b >> 3] >> (8 * (b & 7)));
        if (raised) rec[22] = 1;
    } else {
        const bool zero = (d.w[0] | d.w[1] | d.w[2] | d.w[3]) == 0;
        *verdict = raised || !canonical ? ST_MALFORMED : (zero ? ST_OK : ST_INVALID_SIG);
    }
}

// Behind ag_k_finish_scalar, for a keyed object and n >= 1: *verdict = SSA_INVALID_PUBLIC_KEY iff some byte of kst[0, n)
// says so; otherwise the word is left as the comparison wrote it.  One prefix of up to 2^30 bytes, where
// agc_k_key_verdicts would fold a long aggregate with one workgroup: workgroup b scans kst[b SPAN, min((b + 1) SPAN, n))
// with agc_scan (16-byte loads over the aligned middle -- a span starts at a multiple of 16, so only the tail of the
// last one is ragged), one __ballot per wave, and lane 0 of every wave that saw the status stores the value: several
// writers, one value, ordinary vector stores -- no atomic, no LDS, no barrier.  It reads kst alone, which no launch of a
// finish writes.
__global__ void __launch_bounds__(256)
agv_k_key_verdict(const u8 *__restrict__ kst, size_t n, u32 *__restrict__ verdict) {
    const size_t base = (size_t)blockIdx.x * AGV_KST_SPAN;
    if (base >= n) return;       // (never: the grid is ceil(n / SPAN); uniform for the workgroup)
    const u32 cnt = n - base < AGV_KST_SPAN ? (u32)(n - base) : AGV_KST_SPAN;
    const bool any = __ballot(agc_scan(kst + base, 0u, cnt, threadIdx.x, 256u)) != 0ull;
    if (any && (threadIdx.x & 63u) == 0) *verdict = AGC_BAD_KEY;
}
#endif  // SSA_NO_KERNELS

}  // namespace ssa
