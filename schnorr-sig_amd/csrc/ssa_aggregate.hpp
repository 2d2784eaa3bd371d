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
//   ag_k_fold / ag_k_fold_finish   sum a_i e_i mod q: per-workgroup partial sums, then one finishing workgroup; the
//                                  first also makes the checks of msm_k_prepare (canonical limbs, e < q, key on the
//                                  curve, R decodable) when the caller did not screen the signatures
//   ag_k_pack      the first 49 bytes of every signature side by side: the aggregate's R's
//   ag_k_expand    the aggregate's R's back at stride 81 with e = 0: what ssa_k_hash and the MSM preparation read
//   ag_k_finish    one wave: [e_agg]G from the comb and the EXACT comparison with the left-hand point of the MSM's record
//                  (affine x and y, or the identity) -- not the x-only one of msm_k_finish
//
// A workgroup of ag_k_tree takes 512 consecutive nodes: the tree over an aligned run of 2^9 leaves is the same subtree
// whether it is cut out of the level-by-level definition or reduced on its own, and the ragged last run follows the same
// odd-node rule, so passes of nine levels reproduce the definition for every n.  Everything is written with ordinary
// vector stores and read by a later launch on the same stream.
#pragma once
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

#ifndef SSA_NO_KERNELS
// sigs_out (the library's own buffer: dword-aligned, n * 81 bytes) = R_i (49 bytes) || 32 zero bytes.  One lane per dword.
__global__ void __launch_bounds__(256)
ag_k_expand(const u8 *__restrict__ rs49, size_t n, u8 *__restrict__ sigs_out) {
    const size_t d = (size_t)blockIdx.x * 256 + threadIdx.x, total = n * 81, o = 4 * d;
    if (o >= total) return;
    u32 v = 0;
    const int cnt = total - o < 4 ? (int)(total - o) : 4;
    for (int k = 0; k < cnt; k++) {
        const size_t b = o + k, i = b / 81, r = b - 81 * i;
        if (r < 49) v |= (u32)rs49[49 * i + r] << (8 * k);
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

__global__ void __launch_bounds__(256, 4)
ag_k_leaf(const DevParams *__restrict__ prm, const u64 *__restrict__ dig, const u8 *__restrict__ sigs, size_t n,
          u64 *__restrict__ nodes) {
    __shared__ u64 lds[RS_LDS_U64];
    u64 *A = lds + threadIdx.x;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    u64 in[8], d[4];
#pragma unroll
    for (int k = 0; k < 4; k++) in[k] = dig[4 * i + k];
    in[4] = (u64)sigs[81 * i + 48];
    in[5] = AG_TAG_LEAF;
    in[6] = in[7] = 0;
    ag_hash8(A, prm, in, 6u, d);
#pragma unroll
    for (int k = 0; k < 4; k++) nodes[4 * i + k] = d[k];
}

// One pass of the tree: workgroup b reduces nodes [512 b, 512 b + 512) of `in` (count of them in all) to out[b].  top != 0
// (a launch of ONE workgroup): the node left is the tree's top and out[0] receives the root, H(top || n_total || 0xA2).
__global__ void __launch_bounds__(256, 4)
ag_k_tree(const DevParams *__restrict__ prm, const u64 *__restrict__ in, u32 count, u64 n_total, u32 top,
          u64 *__restrict__ out) {
    __shared__ u64 lds[RS_LDS_U64];
    __shared__ u64 node[256 * 4];
    u64 *A = lds + threadIdx.x;
    const u32 t = threadIdx.x, first = blockIdx.x * AG_TREE_SPAN;
    if (first >= count) return;                       // (block-uniform)
    u32 cnt = count - first < AG_TREE_SPAN ? count - first : AG_TREE_SPAN;
    const u64 *src = in + 4 * (size_t)first;          // this level's nodes: global for the first level, then LDS
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
    for (int k = 0; k < 4; k++) out[4 * (size_t)blockIdx.x + k] = r[k];
}

__global__ void __launch_bounds__(256, 4)
ag_k_coeff(const DevParams *__restrict__ prm, const u64 *__restrict__ root, size_t n, u64 *__restrict__ coeffs) {
    __shared__ u64 lds[RS_LDS_U64];
    u64 *A = lds + threadIdx.x;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    u64 in[8], d[4];
#pragma unroll
    for (int k = 0; k < 4; k++) in[k] = root[k];
    in[4] = (u64)i;
    in[5] = AG_TAG_COEFF;
    in[6] = in[7] = 0;
    ag_hash8(A, prm, in, 6u, d);
    // the first 16 bytes of Digest::to_bytes, little-endian, masked to 126 bits; 0 becomes 1
    u64 lo = d[0];
    const u64 hi = d[1] & AG_COEFF_HI_MASK;
    if ((lo | hi) == 0) lo = 1;
    reinterpret_cast<ulonglong2 *>(coeffs)[i] = make_ulonglong2(lo, hi);
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
        const sc256 e = ld_sc(sigs + 81 * i + 49);
        bool ok = !sc_geq_q(e);
        if (status) {
            aff P;
            P.x = ld_fp6(pks + 96 * i, ok);
            P.y = ld_fp6(pks + 96 * i + 48, ok);
            if (ok && !(pk_inf && pk_inf[i])) ok = aff_on_curve(P);
            aff R;
            bool r_inf = false;
            if (ok) ok = decompress_lane(sigs + 81 * i, R, r_inf) == 0;
            status[i] = (u8)(ok ? ST_OK : ST_MALFORMED);
            if (!ok) atomicAdd(n_bad, 1ull);
        }
        if (ok) {
            sc256 a;
            a.w[0] = coeffs[2 * i];
            a.w[1] = coeffs[2 * i + 1];
            a.w[2] = a.w[3] = 0;
            ae = sc_mul_mod(a, e);
        }
    }
#pragma unroll
    for (int k = 0; k < 4; k++) red[threadIdx.x * 4 + k] = ae.w[k];
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
#pragma unroll
    for (int k = 0; k < 4; k++) red[threadIdx.x * 4 + k] = acc.w[k];
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
    if (threadIdx.x < 32) e_out[threadIdx.x] = (u8)(red[threadIdx.x >> 3] >> (8 * (threadIdx.x & 7u)));
}

// the empty aggregate (n == 0): valid iff its 32 bytes are zero
__global__ void __launch_bounds__(64)
ag_k_empty(const u8 *__restrict__ e_agg, u32 *__restrict__ verdict) {
    if (threadIdx.x != 0) return;
    const sc256 e = ld_sc(e_agg);
    const bool zero = (e.w[0] | e.w[1] | e.w[2] | e.w[3]) == 0;
    *verdict = zero ? ST_OK : (sc_geq_q(e) ? ST_MALFORMED : ST_INVALID_SIG);
}

// ONE wave.  rec: the 24-word record of the MSM over the aggregate's R's with e = 0 -- the left-hand point
// sum a_i R_i - sum (a_i h_i) P_i in canonical form (affine (x, y, 1), or (0, 0, 0) for the identity), and the malformed
// flag.  right = [e_agg]G from the comb (the walk of msm_k_finish's second wave, same slots); then the comparison of
// msm_k_finish_seg: both coordinates, the identity equal to the identity only.
__global__ void __launch_bounds__(64)
ag_k_finish(const u64 *__restrict__ rec, const u8 *__restrict__ e_agg, const u64 *__restrict__ gtab,
            u32 *__restrict__ verdict) {
    __shared__ CoopLds L;
    const u32 lane = threadIdx.x;
    const int ws = 0;
    const sc256 e = ld_sc(e_agg);
    if (rec[22] != 0 || rec[23] != SSA_MSM_RECORD_MAGIC || sc_geq_q(e)) {   // (wave-uniform)
        if (lane == 0) *verdict = ST_MALFORMED;
        return;
    }
    // slots: left 0..2 (X, Y, Z); right accumulator 20..23, addend 24..25, scratch 26..34; comparison 7..10
    int t[9];
#pragma unroll
    for (int k = 0; k < 9; k++) t[k] = 26 + k;
    if (lane < 36) {
        const u32 v = lane / 12u, c = lane % 12u;
        const u64 w = rec[6u * v + c % 6u];
        L.slot[(int)v][c] = c < 6 ? w : fp_mul_small(w, 7u);
    }
    coop_sync();
    coop_set(L, 20, 1ull, lane, ws);
    coop_set(L, 21, 1ull, lane, ws);
    coop_set(L, 22, 0ull, lane, ws);
    coop_set(L, 23, 0ull, lane, ws);
    const GtabGeom gg = gtab_geom(gtab);
#pragma unroll 1
    for (u32 w = 0; w < gg.count; w++) {              // BASEPOINT_TABLE.multiply_vartime
        const u32 d = sc_bits(e, w * gg.bits, gg.bits);
        if (d != 0) {
            const u64 *rowp = gtab + (((size_t)w << gg.bits) + d) * 12;
            if (lane < 24) {
                const u32 half = lane / 12u, c = lane % 12u;
                const u64 v = rowp[6u * half + c % 6u];
                L.slot[half ? 25 : 24][c] = c < 6 ? v : fp_mul_small(v, 7u);
            }
            coop_sync();
            coop_jac_madd(L, 20, 24, 25, t, lane, ws);
        }
    }
    // X_l Z_r^2 == X_r Z_l^2 and Y_l Z_r^3 == Y_r Z_l^3 (X_r and Y_r only as first operands: their 7x halves may be stale)
    const bool li = coop_is_zero(L, 2, lane, ws), ri = coop_is_zero(L, 22, lane, ws);
    bool eq;
    if (li || ri) {
        eq = li && ri;
    } else {
        coop_mul(L, 7, 22, 22, lane, ws);      // Z_r^2
        coop_mul(L, 8, 0, 7, lane, ws);        // X_l Z_r^2
        coop_mul(L, 9, 2, 2, lane, ws);        // Z_l^2
        coop_mul(L, 10, 20, 9, lane, ws);      // X_r Z_l^2
        eq = coop_eq(L, 8, 10, lane, ws);
        coop_mul(L, 7, 7, 22, lane, ws);       // Z_r^3
        coop_mul(L, 8, 1, 7, lane, ws);        // Y_l Z_r^3
        coop_mul(L, 9, 9, 2, lane, ws);        // Z_l^3
        coop_mul(L, 10, 21, 9, lane, ws);      // Y_r Z_l^3
        eq = eq && coop_eq(L, 8, 10, lane, ws);
    }
    if (lane == 0) *verdict = eq ? ST_OK : ST_INVALID_SIG;
}
#endif  // SSA_NO_KERNELS

}  // namespace ssa
