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
//           the plain push writes its n bytes with one hipMemsetAsync; reset turns it off.  So bytes that a failed push
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
// The object's seven arrays are its own allocations (released by destroy, or by the context's clean-up): they are not in
// the context's list of workspaces, and nothing the object needs between two calls lives in one.
#pragma once
#include "ssa_aggcache.hpp"
#include "ssa_aggregator.hpp"

struct ssa_aggverifier : AgxStore {
    static constexpr uint32_t kCreateFlags = 0;
    uint64_t pushed = 0, cached = 0;              // cached: lanes pushed through a key cache
    bool keyed = false;                           // kst[0, held) is valid and finish folds it (the rule above)
    DevBuf rpts, ppts, h, bad, kst;
};
// everything the object will ever hold, in the order it is allocated and released
static inline std::vector<AgxStore::Buf> agx_bufs(ssa_aggverifier &v) {
    return {{&v.rpts, 96 * v.capacity}, {&v.ppts, 96 * v.capacity}, {&v.h, 32 * v.capacity},  {&v.leaves, 32 * v.capacity},
            {&v.bad, v.capacity + 16},  {&v.tops, 32 * v.n_tops()}, {&v.kst, v.capacity + 16}};
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
__global__ void __launch_bounds__(256)
agv_k_append(const DevParams *__restrict__ prm, const u8 *__restrict__ sigs, const u8 *__restrict__ pks,
             const u8 *__restrict__ pk_inf, const u64 *__restrict__ dig, const u64 *__restrict__ h_in, size_t n, size_t held,
             u64 *__restrict__ leaves, u64 *__restrict__ h, u64 *__restrict__ rpts, u64 *__restrict__ ppts,
             u8 *__restrict__ bad) {
    __shared__ u64 lds[RS_LDS_U64];
    u64 *A = lds + threadIdx.x;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const size_t dst = held + i;
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

// The block-time stage in front of the bucket pipeline: one lane per held lane of a piece of n lanes whose first stands at
// place lane0 of the aggregate (h, rpts, ppts, bad: the object's arrays from that lane on).  Lane i derives its coefficient
// out of H(root || lane0 + i || 0xA3) (one permutation; ag_coeff_of_digest) and writes what msm_k_prepare writes with a
// 16-byte coefficient and e = 0: the signed digits of a_i over the wa windows a coefficient reaches for point i, those of
// a_i h_i mod q over all windows for point n + i, and the two stored rows as points i and n + i.  A wave with a bad lane
// sets the malformed word: one ballot, one atomic.  The coefficients never travel through memory.
__global__ void __launch_bounds__(256)
agv_k_scalars(const DevParams *__restrict__ prm, const u64 *__restrict__ root, const u64 *__restrict__ h,
              const u64 *__restrict__ rpts, const u64 *__restrict__ ppts, const u8 *__restrict__ bad, size_t n, u64 lane0,
              MsmShape shp, u32 wa, u64 *__restrict__ points, short *__restrict__ digits, u32 *__restrict__ malformed) {
    __shared__ u64 lds[RS_LDS_U64];
    u64 *A = lds + threadIdx.x;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool is_bad = false;
    if (i < n) {
        u64 in[8], d[4];
#pragma unroll
        for (int k = 0; k < 4; k++) in[k] = root[k];
        in[4] = lane0 + (u64)i;
        in[5] = AG_TAG_COEFF;
        in[6] = in[7] = 0;
        ag_hash8(A, prm, in, 6u, d);
        sc256 a, hv;
        ag_coeff_of_digest(d, a.w[0], a.w[1]);
        a.w[2] = a.w[3] = 0;
        (void)write_signed_digits(a, shp.c, wa, digits, 2 * n, i);       // 126 bits: never carries out
#pragma unroll
        for (int k = 0; k < 4; k++) hv.w[k] = h[4 * i + k];
        (void)write_signed_digits(sc_mul_mod(a, hv), shp.c, shp.windows, digits, 2 * n, n + i);
        // a row is 96 bytes at a multiple of 96 from a device allocation: six 16-byte words
        const ulonglong2 *rs = reinterpret_cast<const ulonglong2 *>(rpts + 12 * i);
        const ulonglong2 *ps = reinterpret_cast<const ulonglong2 *>(ppts + 12 * i);
        ulonglong2 *rd = reinterpret_cast<ulonglong2 *>(points + 12 * i);
        ulonglong2 *pd = reinterpret_cast<ulonglong2 *>(points + 12 * (n + i));
#pragma unroll
        for (int k = 0; k < 6; k++) {
            rd[k] = rs[k];
            pd[k] = ps[k];
        }
        is_bad = bad[i] != 0;
    }
    if (__ballot(is_bad) != 0 && (threadIdx.x & 63u) == 0) atomicOr(malformed, 1u);
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
