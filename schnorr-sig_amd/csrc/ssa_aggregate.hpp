// Internal: non-interactive half-aggregation of signatures (ssa_aggregate_many / ssa_verify_aggregate, DESIGN.md
// section 20; Chalkias, Garillot, Kondi, Nikolaenko, CT-RSA 2021).  n signatures (R_i, e_i) become the n R's and ONE
// scalar e_agg = sum a_i e_i mod q, where the coefficients a_i are hashed out of a transcript that binds every R_i,
// key, message and the order of the lanes.  The transcript is Rescue all the way down:
//
//   d_i    = the raw 4-felt digest of hash_message(R_i.x, P_i, m_i)        ssa_k_hash (digest_out), unchanged
//   leaf_i = H(d_i || flag byte of R_i || 0xA1)                            ag_k_leaf    one lane per signature
//   node   = H(left || right), an odd last node moves up unchanged         ag_k_tree    512 nodes per workgroup and pass:
//   root   = H(top || n || 0xA2)                                                        nine levels through LDS
//   a_i    = low 126 bits of Digest::to_bytes(H(root || i || 0xA3)), 0 -> 1   ag_k_coeff   n x 16 bytes
//
// ONE transcript with an optional plan.  The kernels run over all N lanes of a call at once and take the plan's device
// pointers: first (k + 1 prefix sums of the aggregates' sizes), map (lane -> aggregate, ag_k_lane_map) and the tree's
// descriptors (one per workgroup and pass, built on the host by ag_plan: no aggregate's nodes mix with another's).  A null
// plan is the single call: one aggregate of n lanes starting at lane 0, the uniform cut of the
// tree, root 0.  Many aggregates in one call (ssa_verify_aggregates_many) upload a plan; verdict j
// is then the single call's for aggregate j alone by construction, as far as the transcript goes.
//
//   ag_k_expand    the aggregates' R's back at stride 81 with e = 0: what ssa_k_hash and the MSM preparation read
//   ag_k_fold / ag_k_fold_finish   sum a_i e_i mod q: per-workgroup partial sums, then one finishing workgroup; the
//                                  first also makes the checks of msm_k_prepare (canonical limbs, e < q, key on the
//                                  curve, R decodable) when the caller did not screen the signatures
//   ag_k_pack      the first 49 bytes of every signature side by side: the aggregate's R's
//   ag_k_level     one level of the tree as one flat launch, a lane per output node: what a shard
//                  of a larger aggregate reduces its blocks of 2^t lanes with
//   ag_k_finish    one wave per aggregate: [e_agg]G from the comb and the EXACT comparison with the left-hand point of
//                  the MSM's record (affine x and y, or the identity) -- not the x-only one of msm_k_finish; the empty
//                  aggregate is valid iff its scalar is zero
//
// A workgroup of ag_k_tree takes at most 512 consecutive nodes: the tree over an aligned run of 2^9 leaves is the same
// subtree whether it is cut out of the level-by-level definition or reduced on its own, and the ragged last run follows
// the same odd-node rule, so passes of nine levels reproduce the definition for every n.  Everything is written with
// ordinary vector stores and read by a later launch on the same stream.
//
// After the transcript, every group of consecutive aggregates of a many-call takes the small path (msm_k_small over the
// group's lanes, one wave per aggregate adds its records, ag_k_finish) or the bucket path (ag_k_gather* pad the group to
// equal segments, the screened MSM gives one exact comparison per segment against [e_agg_j]G, ag_k_verdicts_seg turns it
// into the aggregate's verdict).
//
// ssa_aggregate_valid_many aggregates only the lanes that pass the screen: av_k_keep_count,
// av_k_keep_scan and av_k_keep_list turn the status vector into the ascending list of kept lanes (ballots and sums, no
// atomic), av_k_gather_sigs and av_k_gather_dig lay those lanes' signatures and raw digests side by side, and leaf, tree,
// coefficient, fold and pack run over them as over any batch: a lane's digest does not depend on its place.
//
// ssa_aggregate_valid_many_cached keeps the lanes that pass ssa_verify_many_cached instead -- the
// subgroup check of the key included -- and hands the kept lanes' keys on: av_k_gather_sigs also reads signatures out of
// 130-byte records, av_k_gather_keys lays the kept keys (49 or 96 bytes, and the pk_inf byte) side by side.
//
// ssa_aggregates_many produces k aggregates in one call: the transcript with a plan over the
// signatures themselves, then ag_k_fold_seg (one lane per signature over the dense lanes, a segmented sum per workgroup,
// one partial per workgroup and aggregate), ag_k_fold_finish_seg (one wave per aggregate: its scalar and its refusal,
// decided on the device) and ag_k_pack_many (the R's into the wire form ssa_verify_aggregates_many reads).
//
// The streaming aggregator (ssa_aggregator.hpp) does the work in front of the coefficients when the
// lanes arrive and shares the per-lane bodies here: ag_leaf_hash, ag_lane_ok, ag_coeff_of_digest, ag_block_sum.
#pragma once
#include <vector>
#include "ssa_kernels.hpp"

namespace ssa {

constexpr u64 AG_TAG_LEAF = 0xA1, AG_TAG_ROOT = 0xA2, AG_TAG_COEFF = 0xA3;
constexpr u32 AG_TREE_LEVELS = 9, AG_TREE_SPAN = 1u << AG_TREE_LEVELS;   // nodes a workgroup of 256 lanes reduces to one
constexpr u64 AG_COEFF_HI_MASK = (1ull << 62) - 1ull;                    // 126 bits: no window recoding ever carries out

// hash_field of the first n_felts (<= 8: one permutation) of `in`
SSA_DEV void ag_hash8(u64 *A, const DevParams *__restrict__ prm, const u64 (&in)[8], u32 n_felts, u64 (&d)[4]) {
    sponge_hash(A, A, prm, n_felts, [&](u32 idx) -> u64 {
        u64 v = in[0];
#pragma unroll
        for (int k = 1; k < 8; k++)
            if (idx == (u32)k) v = in[k];
        return v;
    }, d);
}

// ---- the plan of one ssa_verify_aggregates_many call: host code, from the caller's counts alone ----
// a workgroup of ag_k_tree: nodes [first, first + count) of this pass's input belong to one aggregate and reduce to
// one node, out[slot]; top_n != 0: the node is that aggregate's top, top_n its n_j, and roots[slot] receives the root
struct AgTreeDesc {
    u32 first, count, slot, top_n;
};
// consecutive aggregates [agg0, agg0 + aggs) with lanes [lane0, lane0 + lanes); seg_lanes: the largest n_j of the group
// rounded up to 256 (the padded segment of the bucket path); bucket: which path the group takes
struct AgGroup {
    u32 agg0, aggs, lane0, lanes, seg_lanes, bucket;
};
constexpr u32 AG_GROUP_MAX = 256;        // segments of one screened MSM (SCREEN_MAX_SEGS)
struct AgPlan {
    std::vector<u32> first;                          // k + 1 prefix sums of the counts
    std::vector<u32> pfirst;                         // k + 1 prefix sums of the 256-lane workgroups each aggregate touches
    std::vector<std::vector<AgTreeDesc>> passes;     // the passes per call are those of the largest aggregate
    std::vector<AgGroup> groups;
};

// Groups are formed greedily from consecutive aggregates: at most AG_GROUP_MAX of them, and padded lanes
// (aggregates x seg_lanes) within one MSM slice.  A group whose real lanes fit small_max takes the small path.
// SSA_ERR_ARG: an aggregate above the slice, or more than SSA_MAX_BATCH lanes in all.
static inline int ag_plan(const uint64_t *counts, size_t k, size_t slice, size_t small_max, AgPlan &pl) {
    pl.first.assign(k + 1, 0u);
    pl.passes.clear();
    pl.groups.clear();
    uint64_t total = 0;
    for (size_t j = 0; j < k; j++) {
        if (counts[j] > slice || counts[j] > SSA_MAX_BATCH) return SSA_ERR_ARG;
        total += counts[j];
        if (total > SSA_MAX_BATCH) return SSA_ERR_ARG;
        pl.first[j + 1] = (u32)total;
    }
    // the producer's fold (ag_k_fold_seg): over the dense lanes aggregate j shares lanes with the workgroups
    // first[j] >> 8 .. (first[j + 1] - 1) >> 8, and each of them writes one partial for it; an empty one has none
    pl.pfirst.assign(k + 1, 0u);
    for (size_t j = 0; j < k; j++)
        pl.pfirst[j + 1] = pl.pfirst[j] + (counts[j] ? ((pl.first[j + 1] - 1) >> 8) - (pl.first[j] >> 8) + 1 : 0u);
    // the tree: every aggregate advances in the same pass; (offset, count) of its nodes in the pass's input
    std::vector<u32> off(pl.first.begin(), pl.first.end() - 1), cnt(k);
    size_t live = 0;
    for (size_t j = 0; j < k; j++) live += (cnt[j] = (u32)counts[j]) != 0;
    while (live) {
        std::vector<AgTreeDesc> pass;
        u32 next = 0;
        for (size_t j = 0; j < k; j++) {
            if (!cnt[j]) continue;
            const u32 g = (cnt[j] + AG_TREE_SPAN - 1) / AG_TREE_SPAN;
            const bool top = g == 1;
            for (u32 b = 0; b < g; b++) {
                const u32 lo = b * AG_TREE_SPAN, c = cnt[j] - lo < AG_TREE_SPAN ? cnt[j] - lo : AG_TREE_SPAN;
                pass.push_back({off[j] + lo, c, top ? (u32)j : next + b, top ? (u32)counts[j] : 0u});
            }
            if (top) {
                cnt[j] = 0;
                live--;
            } else {
                off[j] = next;
                cnt[j] = g;
                next += g;
            }
        }
        pl.passes.push_back(std::move(pass));
    }
    auto pad = [](uint64_t n) { return (n + 255) & ~(uint64_t)255; };
    for (size_t j = 0; j < k;) {
        AgGroup g{(u32)j, 0u, pl.first[j], 0u, 0u, 0u};
        uint64_t seg = 256;
        while (j < k && g.aggs < AG_GROUP_MAX) {
            const uint64_t s2 = pad(counts[j]) > seg ? pad(counts[j]) : seg;
            if (g.aggs && s2 * (g.aggs + 1) > slice) break;     // (one aggregate always fits: n_j <= slice, checked by the caller's bound)
            seg = s2;
            g.aggs++;
            j++;
        }
        g.lanes = pl.first[g.agg0 + g.aggs] - g.lane0;
        g.seg_lanes = (u32)seg;
        g.bucket = g.lanes > small_max ? 1u : 0u;
        pl.groups.push_back(g);
    }
    return 0;
}

#ifndef SSA_NO_KERNELS
// The wire form of a call: aggregate j is its n_j R's (49 bytes each) and then e_agg_j (32 bytes), the aggregates end to
// end.  lane: the lane's number in the call (first_j + l); a single aggregate is j = 0.
SSA_DEV size_t ag_wire_r(size_t lane, u32 j) { return 49 * lane + 32 * (size_t)j; }
// e_agg_j stands behind the aggregate's last R; first == nullptr: the one aggregate of n lanes
SSA_DEV size_t ag_wire_e(const u32 *__restrict__ first, u32 j, size_t n) { return ag_wire_r(first ? first[j + 1] : n, j); }

// sigs_out (the library's own buffer: dword-aligned, n * 81 bytes) = R_i (49 bytes) || 32 zero bytes, over the n lanes of
// the wire form `aggs`; map[i]: the aggregate of lane i, nullptr: one aggregate.  One lane per dword.
__global__ void __launch_bounds__(256)
ag_k_expand(const u8 *__restrict__ aggs, const u32 *__restrict__ map, size_t n, u8 *__restrict__ sigs_out) {
    const size_t d = (size_t)blockIdx.x * 256 + threadIdx.x, total = n * 81, o = 4 * d;
    if (o >= total) return;
    u32 v = 0;
    const int cnt = total - o < 4 ? (int)(total - o) : 4;
    for (int k = 0; k < cnt; k++) {
        const size_t b = o + k, i = b / 81, r = b - 81 * i;
        if (r < 49) v |= (u32)aggs[ag_wire_r(i, map ? map[i] : 0u) + r] << (8 * k);
    }
    if (cnt == 4) {
        reinterpret_cast<u32 *>(sigs_out)[d] = v;
    } else {
        for (int k = 0; k < cnt; k++) sigs_out[o + k] = (u8)(v >> (8 * k));
    }
}

// agg_out[0, 49 n) = the first 49 bytes of every signature.  agg_out is the caller's: dwords only when it is aligned.
__global__ void __launch_bounds__(256)
ag_k_pack(const u8 *__restrict__ sigs, size_t n, u8 *__restrict__ agg_out) {
    const size_t d = (size_t)blockIdx.x * 256 + threadIdx.x, total = n * 49, o = 4 * d;
    if (o >= total) return;
    u32 v = 0;
    const int cnt = total - o < 4 ? (int)(total - o) : 4;
    for (int k = 0; k < cnt; k++) {
        const size_t b = o + k, i = b / 49;
        v |= (u32)sigs[81 * i + (b - 49 * i)] << (8 * k);
    }
    if (cnt == 4 && (reinterpret_cast<uintptr_t>(agg_out) & 3u) == 0) {
        reinterpret_cast<u32 *>(agg_out)[d] = v;
    } else {
        for (int k = 0; k < cnt; k++) agg_out[o + k] = (u8)(v >> (8 * k));
    }
}

// leaf_i = H(d_i || flag byte of R_i || 0xA1): dig the raw digests (four words per lane), flag the lane's byte 48
SSA_DEV void ag_leaf_hash(u64 *A, const DevParams *__restrict__ prm, const u64 *__restrict__ dig, size_t i, u8 flag,
                          u64 (&d)[4]) {
    u64 in[8];
#pragma unroll
    for (int k = 0; k < 4; k++) in[k] = dig[4 * i + k];
    in[4] = (u64)flag;
    in[5] = AG_TAG_LEAF;
    in[6] = in[7] = 0;
    ag_hash8(A, prm, in, 6u, d);
}

__global__ void __launch_bounds__(256, 4)
ag_k_leaf(const DevParams *__restrict__ prm, const u64 *__restrict__ dig, const u8 *__restrict__ sigs, size_t n,
          u64 *__restrict__ nodes) {
    __shared__ u64 lds[RS_LDS_U64];
    u64 *A = lds + threadIdx.x;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    u64 d[4];
    ag_leaf_hash(A, prm, dig, i, sigs[81 * i + 48], d);
#pragma unroll
    for (int k = 0; k < 4; k++) nodes[4 * i + k] = d[k];
}

// One level of the tree, flat: lane j of the launch writes node j of the next level,
// H(in[2j] || in[2j + 1]), or in[2j] unchanged when it is the odd last node of its level; count nodes come in,
// (count + 1) / 2 go out.  One permutation per lane at ag_k_leaf's shape; nodes travel through global memory alone (in and
// out are different buffers), so no lane waits for another.  Over the lanes of a shard that starts on a multiple of
// B = 2^t, pairs of the first t levels never cross a block of B leaves: t launches leave one top per block, the ragged
// last block's by the same odd-node rule.
__global__ void __launch_bounds__(256, 4)
ag_k_level(const DevParams *__restrict__ prm, const u64 *__restrict__ in, size_t count, u64 *__restrict__ out) {
    __shared__ u64 lds[RS_LDS_U64];
    u64 *A = lds + threadIdx.x;
    const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= (count + 1) / 2) return;
    u64 r[4];
    if (2 * j + 1 < count) {
        u64 v[8];
#pragma unroll
        for (int k = 0; k < 8; k++) v[k] = in[8 * j + k];
        ag_hash8(A, prm, v, 8u, r);
    } else {                                          // the odd last node moves up unchanged
#pragma unroll
        for (int k = 0; k < 4; k++) r[k] = in[8 * j + k];
    }
#pragma unroll
    for (int k = 0; k < 4; k++) out[4 * j + k] = r[k];
}

// cnt (>= 1) nodes at src reduced by one workgroup of 256 lanes to one node at out (four words); top != 0: the node left
// is a tree's top and out receives the root, H(top || n_total || 0xA2).  lds, node: the workgroup's shared arrays.
SSA_DEV void ag_tree_reduce(u64 *lds, u64 *node, const DevParams *__restrict__ prm, const u64 *__restrict__ src, u32 cnt,
                            u64 n_total, u32 top, u64 *__restrict__ out) {
    u64 *A = lds + threadIdx.x;
    const u32 t = threadIdx.x;
#pragma unroll 1
    for (u32 lvl = 0; lvl < AG_TREE_LEVELS && cnt > 1; lvl++) {
        const u32 outc = (cnt + 1) / 2;
        u64 r[4] = {0, 0, 0, 0};
        if (t < outc) {
            if (2 * t + 1 < cnt) {
                u64 v[8];
#pragma unroll
                for (int k = 0; k < 8; k++) v[k] = src[8 * t + k];
                ag_hash8(A, prm, v, 8u, r);
            } else {                                  // the odd last node moves up unchanged
#pragma unroll
                for (int k = 0; k < 4; k++) r[k] = src[8 * t + k];
            }
        }
        __syncthreads();                              // every read of this level before the first write of the next
        if (t < outc) {
#pragma unroll
            for (int k = 0; k < 4; k++) node[4 * t + k] = r[k];
        }
        __syncthreads();
        cnt = outc;
        src = node;
    }
    if (t != 0) return;
    u64 v[8], r[4];
#pragma unroll
    for (int k = 0; k < 4; k++) r[k] = v[k] = src[k];
    if (top) {
        v[4] = n_total;
        v[5] = AG_TAG_ROOT;
        v[6] = v[7] = 0;
        ag_hash8(A, prm, v, 6u, r);
    }
#pragma unroll
    for (int k = 0; k < 4; k++) out[k] = r[k];
}

// One pass of the tree.  Workgroup b follows desc[b] (ag_plan; count of them), so one aggregate's nodes never mix with
// another's.  desc == nullptr, one aggregate: it forms its own descriptor, nodes [512 b, 512 b + 512) of the count in all
// into slot b, and top_n (its n on the pass of ONE workgroup, else 0).  A top workgroup writes its aggregate's root,
// H(top || n || 0xA2), to roots[slot], any other its node to out[slot].
__global__ void __launch_bounds__(256, 4)
ag_k_tree(const DevParams *__restrict__ prm, const u64 *__restrict__ in, const AgTreeDesc *__restrict__ desc, u32 count,
          u32 top_n, u64 *__restrict__ out, u64 *__restrict__ roots) {
    __shared__ u64 lds[RS_LDS_U64];
    __shared__ u64 node[256 * 4];
    AgTreeDesc d;
    if (desc) {
        if (blockIdx.x >= count) return;              // (block-uniform)
        d = desc[blockIdx.x];
    } else {
        const u32 first = blockIdx.x * AG_TREE_SPAN;
        if (first >= count) return;                   // (block-uniform)
        d = {first, count - first < AG_TREE_SPAN ? count - first : AG_TREE_SPAN, blockIdx.x, top_n};
    }
    ag_tree_reduce(lds, node, prm, in + 4 * (size_t)d.first, d.count, (u64)d.top_n, d.top_n != 0u,
                   (d.top_n ? roots : out) + 4 * (size_t)d.slot);
}

// map[i] = the aggregate of lane i: the smallest j with first[j + 1] > i (empty aggregates own no lane)
__global__ void __launch_bounds__(256)
ag_k_lane_map(const u32 *__restrict__ first, u32 k, size_t n, u32 *__restrict__ map) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    u32 lo = 0, hi = k - 1;
    while (lo < hi) {
        const u32 mid = (lo + hi) / 2;
        if ((size_t)first[mid + 1] <= i) lo = mid + 1;
        else hi = mid;
    }
    map[i] = lo;
}

// (lo, hi) = the coefficient out of the digest d = H(root || index || 0xA3): the first 16 bytes of Digest::to_bytes,
// little-endian, masked to 126 bits; 0 becomes 1.  The one place where the mask and the 0 -> 1 rule stand: ag_k_coeff
// writes the pair out, agx_k_coeff_fold (ssa_aggregator.hpp) multiplies by it.
SSA_DEV void ag_coeff_of_digest(const u64 (&d)[4], u64 &lo, u64 &hi) {
    lo = d[0];
    hi = d[1] & AG_COEFF_HI_MASK;
    if ((lo | hi) == 0) lo = 1;
}

// a_i = H(root_j || i - first_j || 0xA3) with the root and the index of the lane's own aggregate j = map[i]; map and
// first == nullptr: one aggregate, root 0 and index lane0 + i -- lane0 is the place of the launch's first lane in its
// aggregate: 0 but for a shard of a larger aggregate
__global__ void __launch_bounds__(256, 4)
ag_k_coeff(const DevParams *__restrict__ prm, const u64 *__restrict__ roots, const u32 *__restrict__ map,
           const u32 *__restrict__ first, size_t n, u64 *__restrict__ coeffs, u64 lane0) {
    __shared__ u64 lds[RS_LDS_U64];
    u64 *A = lds + threadIdx.x;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const u32 j = map ? map[i] : 0u;
    u64 in[8], d[4];
#pragma unroll
    for (int k = 0; k < 4; k++) in[k] = roots[4 * (size_t)j + k];
    in[4] = lane0 + (u64)(i - (first ? first[j] : 0u));
    in[5] = AG_TAG_COEFF;
    in[6] = in[7] = 0;
    ag_hash8(A, prm, in, 6u, d);
    u64 lo, hi;
    ag_coeff_of_digest(d, lo, hi);
    reinterpret_cast<ulonglong2 *>(coeffs)[i] = make_ulonglong2(lo, hi);
}

// The sum mod q of one scalar per lane of a workgroup of 256, through red (256 x 4 words): red[0, 4) holds it once the
// call returns.
SSA_DEV void ag_block_sum(u64 *red, const sc256 &v) {
#pragma unroll
    for (int k = 0; k < 4; k++) red[threadIdx.x * 4 + k] = v.w[k];
    __syncthreads();
    for (u32 stride = 128; stride > 0; stride >>= 1) {
        if (threadIdx.x < stride) {
            sc256 a, b;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                a.w[k] = red[threadIdx.x * 4 + k];
                b.w[k] = red[(threadIdx.x + stride) * 4 + k];
            }
            a = sc_add_mod(a, b);
#pragma unroll
            for (int k = 0; k < 4; k++) red[threadIdx.x * 4 + k] = a.w[k];
        }
        __syncthreads();
    }
}

// The checks a fold makes of lane i, and its scalar e: e < q always; check: the other checks of msm_k_prepare too
// (canonical limbs, key on the curve, R decodable).  Returns "passed".
SSA_DEV bool ag_lane_ok(const u8 *__restrict__ sigs, const u8 *__restrict__ pks, const u8 *__restrict__ pk_inf, size_t i,
                        bool check, sc256 &e) {
    e = ld_sc(sigs + 81 * i + 49);
    bool ok = !sc_geq_q(e);
    if (check) {
        aff P;
        P.x = ld_fp6(pks + 96 * i, ok);
        P.y = ld_fp6(pks + 96 * i + 48, ok);
        if (ok && !(pk_inf && pk_inf[i])) ok = aff_on_curve(P);
        aff R;
        bool r_inf = false;
        if (ok) ok = decompress_lane(sigs + 81 * i, R, r_inf) == 0;
    }
    return ok;
}

// Lane i of a fold: ae = a_i e_i mod q when the lane passes, else it stays as it came (zero).  e < q is checked always;
// check: the other checks of msm_k_prepare too (canonical limbs, key on the curve, R decodable).  Returns "passed".
SSA_DEV bool ag_fold_lane(const u8 *__restrict__ sigs, const u8 *__restrict__ pks, const u8 *__restrict__ pk_inf,
                          const u64 *__restrict__ coeffs, size_t i, bool check, sc256 &ae) {
    sc256 e;
    const bool ok = ag_lane_ok(sigs, pks, pk_inf, i, check, e);
    if (ok) {
        sc256 a;
        a.w[0] = coeffs[2 * i];
        a.w[1] = coeffs[2 * i + 1];
        a.w[2] = a.w[3] = 0;
        ae = sc_mul_mod(a, e);
    }
    return ok;
}

// partials[b] = sum over the lanes of workgroup b of a_i e_i mod q.  status != nullptr: the checks of msm_k_prepare too --
// status[i] = SSA_MALFORMED on a lane that fails one (and it adds nothing), else 0; *n_bad counts them.
__global__ void __launch_bounds__(256)
ag_k_fold(const u8 *__restrict__ sigs, const u8 *__restrict__ pks, const u8 *__restrict__ pk_inf,
          const u64 *__restrict__ coeffs, size_t n, u64 *__restrict__ partials, u8 *__restrict__ status,
          unsigned long long *__restrict__ n_bad) {
    __shared__ u64 red[256 * 4];
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    sc256 ae;
#pragma unroll
    for (int k = 0; k < 4; k++) ae.w[k] = 0;
    if (i < n) {
        const bool ok = ag_fold_lane(sigs, pks, pk_inf, coeffs, i, status != nullptr, ae);
        if (status) {
            status[i] = (u8)(ok ? ST_OK : ST_MALFORMED);
            if (!ok) atomicAdd(n_bad, 1ull);
        }
    }
    ag_block_sum(red, ae);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < 4; k++) partials[4 * (size_t)blockIdx.x + k] = red[k];
    }
}

// ONE workgroup: e_out (32 bytes, little-endian, canonical) = the sum of the partial sums mod q
__global__ void __launch_bounds__(256)
ag_k_fold_finish(const u64 *__restrict__ partials, u32 n_partials, u8 *__restrict__ e_out) {
    __shared__ u64 red[256 * 4];
    sc256 acc;
#pragma unroll
    for (int k = 0; k < 4; k++) acc.w[k] = 0;
#pragma unroll 1
    for (u32 b = threadIdx.x; b < n_partials; b += 256u) {
        sc256 p;
#pragma unroll
        for (int k = 0; k < 4; k++) p.w[k] = partials[4 * (size_t)b + k];
        acc = sc_add_mod(acc, p);
    }
    ag_block_sum(red, acc);
    if (threadIdx.x < 32) e_out[threadIdx.x] = (u8)(red[threadIdx.x >> 3] >> (8 * (threadIdx.x & 7u)));
}

// ---- the producer of many aggregates (ssa_aggregates_many) ----
// The fold over all N lanes of the call, densely packed: a workgroup of 256 lanes may hold the end of one aggregate,
// several whole ones and the start of another.  map[i]: the aggregate of lane i (ag_k_lane_map: non-decreasing), so a
// workgroup's lanes fall into runs of equal map.  The workgroup sums every run with a segmented suffix scan through LDS:
// at step d lane t adds lane t + d's value iff both stand in the same run -- after eight steps the head of a run (lane
// 0 of the workgroup, or map[i] != map[i - 1]) holds the run's sum, and writes it as ONE partial.  The partials of
// aggregate j are contiguous: workgroup b's stands at pfirst[j] + b - (first[j] >> 8) (ag_plan).
// screened == 0: the checks of ag_k_fold, status[i] written as there.  screened != 0: status[i] is the screen's and is
// read.  Either way a lane with a nonzero status st adds 1 to acc[2 j] and raises acc[2 j + 1] to 256 - st (both zeroed
// before the launch): the failing lanes of aggregate j and, turned round, the smallest nonzero status among them.
__global__ void __launch_bounds__(256)
ag_k_fold_seg(const u8 *__restrict__ sigs, const u8 *__restrict__ pks, const u8 *__restrict__ pk_inf,
              const u64 *__restrict__ coeffs, const u32 *__restrict__ map, const u32 *__restrict__ first,
              const u32 *__restrict__ pfirst, size_t n, u64 *__restrict__ partials, u8 *__restrict__ status, u32 screened,
              u32 *__restrict__ acc) {
    __shared__ u64 red[256 * 4];
    __shared__ u32 key[256];
    const u32 t = threadIdx.x;
    const size_t i = (size_t)blockIdx.x * 256 + t;
    sc256 v;
#pragma unroll
    for (int k = 0; k < 4; k++) v.w[k] = 0;
    u32 j = 0xFFFFFFFFu;                              // (lanes behind the last one: a run of their own, never written)
    if (i < n) {
        j = map[i];
        const bool ok = ag_fold_lane(sigs, pks, pk_inf, coeffs, i, screened == 0u, v);
        u32 st;
        if (screened) {
            st = status[i];
        } else {
            st = ok ? ST_OK : ST_MALFORMED;
            status[i] = (u8)st;
        }
        if (st) {
            atomicAdd(acc + 2 * (size_t)j, 1u);
            atomicMax(acc + 2 * (size_t)j + 1, 256u - st);
        }
    }
    key[t] = j;
#pragma unroll 1
    for (u32 d = 1; d < 256u; d <<= 1) {
#pragma unroll
        for (int k = 0; k < 4; k++) red[t * 4 + k] = v.w[k];
        __syncthreads();                              // (the first one also publishes key)
        if (t + d < 256u && key[t + d] == j) {
            sc256 b;
#pragma unroll
            for (int k = 0; k < 4; k++) b.w[k] = red[(t + d) * 4 + k];
            v = sc_add_mod(v, b);
        }
        __syncthreads();                              // every read of this step before the next one's writes
    }
    if (i < n && (t == 0 || key[t - 1] != j)) {
        const size_t slot = (size_t)pfirst[j] + blockIdx.x - (first[j] >> 8);
#pragma unroll
        for (int k = 0; k < 4; k++) partials[4 * slot + k] = v.w[k];
    }
}

// One wave per aggregate j: e_agg_j = the sum of its partials [pfirst[j], pfirst[j + 1]) mod q (none for an empty
// aggregate: zero), and the refusal, decided here.  results[j] = 0, or the smallest nonzero status of the aggregate's
// lanes (256 - acc[2 j + 1]) when acc[2 j] of them failed; the 32 bytes at ag_wire_e are e_agg_j, canonical, or zero for
// a refused aggregate.  n_fail != nullptr: the failing lanes are added to the call's count.
__global__ void __launch_bounds__(64)
ag_k_fold_finish_seg(const u64 *__restrict__ partials, const u32 *__restrict__ first, const u32 *__restrict__ pfirst,
                     const u32 *__restrict__ acc, u8 *__restrict__ aggs_out, u32 *__restrict__ results,
                     unsigned long long *__restrict__ n_fail) {
    __shared__ u64 red[64 * 4];
    const u32 j = blockIdx.x, t = threadIdx.x;
    sc256 v;
#pragma unroll
    for (int k = 0; k < 4; k++) v.w[k] = 0;
#pragma unroll 1
    for (u32 b = pfirst[j] + t; b < pfirst[j + 1]; b += 64u) {
        sc256 p;
#pragma unroll
        for (int k = 0; k < 4; k++) p.w[k] = partials[4 * (size_t)b + k];
        v = sc_add_mod(v, p);
    }
#pragma unroll
    for (int k = 0; k < 4; k++) red[t * 4 + k] = v.w[k];
    __syncthreads();
    for (u32 stride = 32; stride > 0; stride >>= 1) {
        if (t < stride) {
            sc256 a, b;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                a.w[k] = red[t * 4 + k];
                b.w[k] = red[(t + stride) * 4 + k];
            }
            a = sc_add_mod(a, b);
#pragma unroll
            for (int k = 0; k < 4; k++) red[t * 4 + k] = a.w[k];
        }
        __syncthreads();
    }
    const u32 bad = acc[2 * (size_t)j], res = bad ? 256u - acc[2 * (size_t)j + 1] : (u32)ST_OK;
    if (t < 32) aggs_out[ag_wire_e(first, j, 0) + t] = res ? (u8)0 : (u8)(red[t >> 3] >> (8 * (t & 7u)));
    if (t == 0) {
        results[j] = res;
        if (n_fail && bad) atomicAdd(n_fail, (unsigned long long)bad);
    }
}

// The R's of the call's n signatures into the wire form of its aggregates: the inverse of ag_k_expand with the map.  Byte
// r < 49 of lane i goes to ag_wire_r(i, map[i]) + r, zero where the lane's aggregate is refused (results[map[i]] != 0).
// One thread per four bytes of the n x 49; aggs_out is the caller's: a dword only when it is aligned and the four bytes
// stand in one aggregate (they then keep their distance: the shift of aggregate j is 32 j bytes).
__global__ void __launch_bounds__(256)
ag_k_pack_many(const u8 *__restrict__ sigs, const u32 *__restrict__ map, const u32 *__restrict__ results, size_t n,
               u8 *__restrict__ aggs_out) {
    const size_t d = (size_t)blockIdx.x * 256 + threadIdx.x, total = n * 49, o = 4 * d;
    if (o >= total) return;
    const int cnt = total - o < 4 ? (int)(total - o) : 4;
    const size_t i0 = o / 49, i1 = (o + cnt - 1) / 49;
    const u32 j0 = map[i0], j1 = map[i1];
    const bool z0 = results[j0] != 0u, z1 = results[j1] != 0u;
    u32 v = 0;
    for (int k = 0; k < cnt; k++) {
        const size_t b = o + k, i = b / 49;
        if (!(i == i0 ? z0 : z1)) v |= (u32)sigs[81 * i + (b - 49 * i)] << (8 * k);
    }
    if (cnt == 4 && j0 == j1 && (reinterpret_cast<uintptr_t>(aggs_out) & 3u) == 0) {
        *reinterpret_cast<u32 *>(aggs_out + ag_wire_r(i0, j0) + (o - 49 * i0)) = v;
    } else {
        for (int k = 0; k < cnt; k++) {
            const size_t b = o + k, i = b / 49;
            aggs_out[ag_wire_r(i, i == i0 ? j0 : j1) + (b - 49 * i)] = (u8)(v >> (8 * k));
        }
    }
}

// ONE wave.  rec: the 24-word record of the MSM over the aggregate's R's with e = 0 -- the left-hand point
// sum a_i R_i - sum (a_i h_i) P_i in canonical form (affine (x, y, 1), or (0, 0, 0) for the identity), and the malformed
// flag.  right = [e_agg]G from the comb (coop_comb_add), then the exact comparison (coop_jac_equal): what
// msm_k_finish_seg does with a segment.
SSA_DEV void ag_finish_wave(CoopLds &L, const u64 *__restrict__ rec, const u8 *__restrict__ e_agg,
                            const u64 *__restrict__ gtab, u32 *__restrict__ verdict) {
    const u32 lane = threadIdx.x;
    const int ws = 0;
    const sc256 e = ld_sc(e_agg);
    if (rec[22] != 0 || rec[23] != SSA_MSM_RECORD_MAGIC || sc_geq_q(e)) {   // (wave-uniform)
        if (lane == 0) *verdict = ST_MALFORMED;
        return;
    }
    // slots as msm_k_finish_seg: left 0..2 (X, Y, Z); right accumulator 20..23, addend 24..25, scratch 26..34; comparison 7..10
    int t[9];
#pragma unroll
    for (int k = 0; k < 9; k++) t[k] = 26 + k;
    coop_load_jac(L, 0, rec, lane);
    coop_set_identity(L, 20, lane, ws);
    coop_comb_add(L, 20, 24, 25, e, gtab, t, lane, ws);
    const bool eq = coop_jac_equal(L, 0, 20, 7, lane, ws);
    if (lane == 0) *verdict = eq ? ST_OK : ST_INVALID_SIG;
}

// One wave per aggregate: block s compares recs[s], the record of aggregate j = agg0 + s (the small path: the sum of its
// lanes' records), with [e_agg_j]G for that aggregate's own scalar.  first == nullptr: one aggregate of n lanes.  The empty
// aggregate has no record: it is valid iff its 32 bytes are zero.
// the verdict of an aggregate without lanes
SSA_DEV u32 ag_empty_verdict(const u8 *__restrict__ e_agg) {
    const sc256 e = ld_sc(e_agg);
    const bool zero = (e.w[0] | e.w[1] | e.w[2] | e.w[3]) == 0;
    return zero ? ST_OK : (sc_geq_q(e) ? ST_MALFORMED : ST_INVALID_SIG);
}

__global__ void __launch_bounds__(64)
ag_k_finish(const u64 *__restrict__ recs, const u8 *__restrict__ aggs, const u32 *__restrict__ first, size_t n, u32 agg0,
            const u64 *__restrict__ gtab, u32 *__restrict__ verdicts) {
    __shared__ CoopLds L;
    const u32 j = agg0 + blockIdx.x;
    const u8 *e_agg = aggs + ag_wire_e(first, j, n);
    if (first ? first[j + 1] == first[j] : n == 0) {  // (block-uniform)
        if (threadIdx.x == 0) verdicts[j] = ag_empty_verdict(e_agg);
        return;
    }
    ag_finish_wave(L, recs + 24 * (size_t)blockIdx.x, e_agg, gtab, verdicts + j);
}

// ONE wave, one aggregate whose scalar stands on its own (ssa_verify_aggregate_combine_device): rec against [e_agg]G, or
// the rule of the empty aggregate when it has no lanes (rec is then not read)
__global__ void __launch_bounds__(64)
ag_k_finish_scalar(const u64 *__restrict__ rec, const u8 *__restrict__ e_agg, u32 empty, const u64 *__restrict__ gtab,
                   u32 *__restrict__ verdict) {
    __shared__ CoopLds L;
    if (empty) {                                      // (block-uniform)
        if (threadIdx.x == 0) *verdict = ag_empty_verdict(e_agg);
        return;
    }
    ag_finish_wave(L, rec, e_agg, gtab, verdict);
}

// ---- the bucket path: a group of `segs` consecutive aggregates padded to segments of seg_lanes lanes each ----
// Padded lane p = s * seg_lanes + l is lane first[agg0 + s] + l of the call when l < n_(agg0 + s), else padding:
// mask 1 (left out of the sums by msm_k_prepare), zero key, zero R, zero scalars.
// One thread per dword of the padded R's at stride 81 (e = 0), straight from the wire form.
__global__ void __launch_bounds__(256)
ag_k_gather_rs(const u8 *__restrict__ aggs, const u32 *__restrict__ first, u32 agg0, u32 segs, u32 seg_lanes,
               u8 *__restrict__ sigs_out) {
    const size_t d = (size_t)blockIdx.x * 256 + threadIdx.x, total = (size_t)segs * seg_lanes * 81, o = 4 * d;
    if (o >= total) return;                            // (total is a multiple of 4: seg_lanes is one of 256)
    u32 v = 0;
    for (int k = 0; k < 4; k++) {
        const size_t b = o + k, p = b / 81, r = b - 81 * p;
        if (r >= 49) continue;
        const u32 j = agg0 + (u32)(p / seg_lanes), l = (u32)(p % seg_lanes);
        if (l < first[j + 1] - first[j]) v |= (u32)aggs[ag_wire_r((size_t)first[j] + l, j) + r] << (8 * k);
    }
    reinterpret_cast<u32 *>(sigs_out)[d] = v;
}

// One thread per padded lane: key, pk_inf, challenge scalar, coefficient and mask; the first 32 * segs threads also copy
// the e_agg's of the group side by side (rhs: what msm_k_finish_seg multiplies G by).
__global__ void __launch_bounds__(256)
ag_k_gather(const u8 *__restrict__ aggs, const u32 *__restrict__ first, u32 agg0, u32 segs, u32 seg_lanes,
            const u8 *__restrict__ pks, const u8 *__restrict__ pk_inf, const u64 *__restrict__ h,
            const u64 *__restrict__ coeffs, u8 *__restrict__ g_pks, u8 *__restrict__ g_inf, u64 *__restrict__ g_h,
            u64 *__restrict__ g_coeffs, u8 *__restrict__ g_mask, u8 *__restrict__ g_rhs) {
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x, total = (size_t)segs * seg_lanes;
    if (p >= total) return;
    if (p < 32 * (size_t)segs) {
        const u32 j = agg0 + (u32)(p >> 5);
        g_rhs[p] = aggs[ag_wire_e(first, j, 0) + (p & 31u)];
    }
    const u32 j = agg0 + (u32)(p / seg_lanes), l = (u32)(p % seg_lanes);
    const bool real = l < first[j + 1] - first[j];
    const size_t i = (size_t)first[j] + l;
    u64 *kd = reinterpret_cast<u64 *>(g_pks + 96 * p);      // (the library's own buffer: aligned)
    if (real && (reinterpret_cast<uintptr_t>(pks) & 7u) == 0) {
        const u64 *ks = reinterpret_cast<const u64 *>(pks + 96 * i);
#pragma unroll
        for (int k = 0; k < 12; k++) kd[k] = ks[k];
    } else {
#pragma unroll 1
        for (int k = 0; k < 12; k++) kd[k] = real ? ld_u64_le(pks + 96 * i + 8 * k) : 0ull;
    }
    g_inf[p] = (u8)(real && pk_inf && pk_inf[i] ? 1u : 0u);
#pragma unroll
    for (int k = 0; k < 4; k++) g_h[4 * p + k] = real ? h[4 * i + k] : 0ull;
#pragma unroll
    for (int k = 0; k < 2; k++) g_coeffs[2 * p + k] = real ? coeffs[2 * i + k] : 0ull;
    g_mask[p] = (u8)(real ? 0u : 1u);
}

// Block s, after the screened MSM over the padded group: the verdict of aggregate agg0 + s.  recheck[p] != 0 on a real
// lane (mask[p] == 0) is a failed check of msm_k_prepare -- a non-canonical limb, a key off the curve, an R that does not
// decode --: SSA_MALFORMED, as is e_agg >= q; else seg_ok[s] is the exact comparison with [e_agg]G.
__global__ void __launch_bounds__(256)
ag_k_verdicts_seg(const u8 *__restrict__ seg_ok, const u8 *__restrict__ recheck, const u8 *__restrict__ mask,
                  const u8 *__restrict__ rhs, u32 seg_lanes, u32 *__restrict__ verdicts) {
    const u32 s = blockIdx.x;
    const size_t lo = (size_t)s * seg_lanes;
    int bad = 0;
    for (u32 l = threadIdx.x; l < seg_lanes; l += 256u) bad |= (recheck[lo + l] != 0 && mask[lo + l] == 0) ? 1 : 0;
    bad = __syncthreads_or(bad);
    if (threadIdx.x != 0) return;
    const sc256 e = ld_sc(rhs + 32 * (size_t)s);
    verdicts[s] = (bad || sc_geq_q(e)) ? ST_MALFORMED : (seg_ok[s] ? ST_OK : ST_INVALID_SIG);
}

// ---- ssa_aggregate_valid_many: the lanes that verify, as an ascending list, and their gathers ----
// A lane is kept iff its status byte is zero.  Its place in the list is a sum of counts and nothing else: the kept lanes
// of the workgroups in front of its own (av_k_keep_scan), of the waves in front of its own within the workgroup, and of
// the lanes below it in its wave's 64-bit ballot.  So the list is ascending and the same on every run: no atomic takes
// part.  Three launches; each reads what the one before wrote.
constexpr u32 AV_BLOCK = 256;

// blk_cnt[b] = kept lanes of workgroup b
__global__ void __launch_bounds__(256)
av_k_keep_count(const u8 *__restrict__ status, u32 n, u32 *__restrict__ blk_cnt) {
    __shared__ u32 wave_cnt[AV_BLOCK / 64];
    const u32 i = blockIdx.x * AV_BLOCK + threadIdx.x;
    const unsigned long long keeps = __ballot(i < n && status[i] == 0);
    if ((threadIdx.x & 63u) == 0) wave_cnt[threadIdx.x >> 6] = (u32)__popcll(keeps);
    __syncthreads();
    if (threadIdx.x == 0) blk_cnt[blockIdx.x] = wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
}

// ONE workgroup: blk_off[b] = kept lanes in front of workgroup b's, blk_off[nb] = the length of the list.  Thread t sums
// a strip of ceil(nb / 256) consecutive counts (128 of them for a full slice of 2^23 lanes), the 256 strip sums are
// scanned through LDS, and the thread walks its strip again from its exclusive sum.
__global__ void __launch_bounds__(256)
av_k_keep_scan(const u32 *__restrict__ blk_cnt, u32 nb, u32 *__restrict__ blk_off) {
    __shared__ u32 part[AV_BLOCK];
    const u32 t = threadIdx.x, per = (nb + AV_BLOCK - 1) / AV_BLOCK;
    const u32 lo = t * per < nb ? t * per : nb, hi = lo + per < nb ? lo + per : nb;
    u32 sum = 0;
    for (u32 b = lo; b < hi; b++) sum += blk_cnt[b];
    part[t] = sum;
    __syncthreads();
    for (u32 d = 1; d < AV_BLOCK; d <<= 1) {
        const u32 v = t >= d ? part[t - d] : 0u;
        __syncthreads();                              // every read of this step before its first write
        part[t] += v;
        __syncthreads();
    }
    u32 acc = part[t] - sum;
    if (t == AV_BLOCK - 1) blk_off[nb] = part[t];
    for (u32 b = lo; b < hi; b++) {
        blk_off[b] = acc;
        acc += blk_cnt[b];
    }
}

// kept[c] = the c-th kept lane, in lane order; kept[c] = 0 from the length of the list up to n
__global__ void __launch_bounds__(256)
av_k_keep_list(const u8 *__restrict__ status, u32 n, const u32 *__restrict__ blk_off, u32 nb, u32 *__restrict__ kept) {
    __shared__ u32 wave_cnt[AV_BLOCK / 64];
    const u32 i = blockIdx.x * AV_BLOCK + threadIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const bool keep = i < n && status[i] == 0;
    const unsigned long long keeps = __ballot(keep);
    if (lane == 0) wave_cnt[wave] = (u32)__popcll(keeps);
    __syncthreads();
    if (i < n && i >= blk_off[nb]) kept[i] = 0;       // (a list entry is below the length: no two threads write one word)
    if (!keep) return;
    u32 pos = blk_off[blockIdx.x] + (u32)__popcll(keeps & ((1ull << lane) - 1ull));
    for (u32 k = 0; k < wave; k++) pos += wave_cnt[k];
    kept[pos] = i;
}

// sigs_out (the library's own buffer: dword-aligned, m * 81 bytes) = the signatures of the m listed lanes side by side.
// The signature of lane i stands at sigs + stride * i + off: (81, 0) for an array of signatures, (130, 49) for
// KeyedSignature records.  One thread per dword, as ag_k_pack; the source lane of every byte is looked up in the list.
__global__ void __launch_bounds__(256)
av_k_gather_sigs(const u8 *__restrict__ sigs, u32 stride, u32 off, const u32 *__restrict__ kept, size_t m,
                 u8 *__restrict__ sigs_out) {
    const size_t d = (size_t)blockIdx.x * 256 + threadIdx.x, total = m * 81, o = 4 * d;
    if (o >= total) return;
    u32 v = 0;
    const int cnt = total - o < 4 ? (int)(total - o) : 4;
    for (int k = 0; k < cnt; k++) {
        const size_t b = o + k, c = b / 81;
        v |= (u32)sigs[(size_t)stride * kept[c] + off + (b - 81 * c)] << (8 * k);
    }
    if (cnt == 4) {
        reinterpret_cast<u32 *>(sigs_out)[d] = v;
    } else {
        for (int k = 0; k < cnt; k++) sigs_out[o + k] = (u8)(v >> (8 * k));
    }
}

// The keys of the m listed lanes side by side, and zeros behind them up to the capacity of `cap` lanes (DESIGN.md
// section 24): out[width * c + r] = src[stride * kept[c] + r] for c < m and r < width, out[width * m, width * cap) = 0.
// Three shapes: 49 bytes out of 130-byte records, 96-byte affine keys, and the pk_inf byte (width 1); src == nullptr (no
// pk_inf given) writes zeros only.  One thread per output dword, the source lane looked up in the list as above; a dword
// that lies within one key and whose source is aligned is one load.  out is the caller's: dwords only when it is aligned.
__global__ void __launch_bounds__(256)
av_k_gather_keys(const u8 *__restrict__ src, u32 stride, u32 width, const u32 *__restrict__ kept, size_t m, size_t cap,
                 u8 *__restrict__ out) {
    const size_t d = (size_t)blockIdx.x * 256 + threadIdx.x, total = cap * width, used = src ? m * width : 0, o = 4 * d;
    if (o >= total) return;
    const int cnt = total - o < 4 ? (int)(total - o) : 4;
    u32 v = 0;
    if (o < used) {
        const size_t c0 = o / width, r0 = o - c0 * width;
        const u8 *p = src + (size_t)stride * kept[c0] + r0;
        if (r0 + 4 <= width && (reinterpret_cast<uintptr_t>(p) & 3u) == 0) {      // (then cnt == 4: c0 < m <= cap)
            v = *reinterpret_cast<const u32 *>(p);
        } else {
            for (int k = 0; k < cnt && o + k < used; k++) {
                const size_t b = o + k, c = b / width;
                v |= (u32)src[(size_t)stride * kept[c] + (b - c * width)] << (8 * k);
            }
        }
    }
    if (cnt == 4 && (reinterpret_cast<uintptr_t>(out) & 3u) == 0) {
        reinterpret_cast<u32 *>(out)[d] = v;
    } else {
        for (int k = 0; k < cnt; k++) out[o + k] = (u8)(v >> (8 * k));
    }
}

// dig_out[c] = dig[kept[c]]: the raw digests (four words) of the m listed lanes, two threads of 16 bytes per lane.  Both
// buffers are the library's own.
__global__ void __launch_bounds__(256)
av_k_gather_dig(const u64 *__restrict__ dig, const u32 *__restrict__ kept, size_t m, u64 *__restrict__ dig_out) {
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= 2 * m) return;
    reinterpret_cast<ulonglong2 *>(dig_out)[t] =
        reinterpret_cast<const ulonglong2 *>(dig)[2 * (size_t)kept[t >> 1] + (t & 1u)];
}
#endif  // SSA_NO_KERNELS

}  // namespace ssa
