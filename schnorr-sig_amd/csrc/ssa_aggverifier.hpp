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
//
//   push    ag_transcript_front (expand to stride 81, ONE ssa_k_hash: raw digests and scalars mod q) -> agv_k_append
//           stores leaf, scalar, the two point rows and the bad byte of each lane -> the blocks this push completed are
//           reduced to their tops (agx_reduce_blocks, shared with the aggregator).  Every lane is appended: a validator
//           cannot drop one, place is part of the transcript.
//   finish  for the first n held lanes: stored tops, the ragged block and ags_root as the aggregator's finish; per piece of
//           at most one MSM slice agv_k_scalars derives a_i, writes the digits of a_i and a_i h_i and copies the stored
//           rows into the MSM's workspaces; sort, buckets and reduce run unchanged (ssa_internal_msm_record_prepared); the
//           pieces' records are added up and compared exactly with [e_agg]G (ag_k_finish_scalar).  finish changes nothing
//           in the object.
//
// The object's six arrays are its own allocations (released by destroy, or by the context's clean-up): they are not in
// the context's list of workspaces, and nothing the object needs between two calls lives in one.
#pragma once
#include "ssa_aggregator.hpp"

struct ssa_aggverifier {
    ssa_ctx *ctx = nullptr;   // nullptr: the context is gone, the device memory went with it
    size_t capacity = 0, block = 0, held = 0;     // block: B, a power of two from 2 to AG_TREE_SPAN
    uint64_t pushes = 0, pushed = 0, finishes = 0;
    DevBuf rpts, ppts, h, leaves, bad, tops;
    void release_all() {
        rpts.release();
        ppts.release();
        h.release();
        leaves.release();
        bad.release();
        tops.release();
    }
};

namespace ssa {

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
    ag_leaf_hash(A, prm, dig, sigs, i, d);
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
#endif  // SSA_NO_KERNELS

}  // namespace ssa
