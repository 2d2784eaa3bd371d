// Hierarchical deterministic key derivation (reference src/derivation.rs), batched: many children of few parents.
// Included at the end of ssa_sign.hip, whose constant-time base multiplication (ct_base_mul, ct_to_aff, the 4-bit
// table of ensure_ctab) and masked scalar arithmetic it uses; the variable-time comb on the context's wide table
// (add_base_mul on ctx->d_gtab) serves the public side.
//
//   ssa_k_derive_prep   one lane per PARENT: decode it (xpub: decompress_lane; xprv: canonical non-zero key, checked
//                       without a branch on the value, and compress([sk]G) by the constant-time product), HMAC's ipad
//                       and opad states of its chain code, and the first seven words of the 53-byte messages -- one
//                       DRV_REC_WORDS record per parent in context scratch (ctx->dv_recs)
//   ssa_k_xprv_derive   one lane per CHILD, constant-time in every secret: derive_private (src/derivation.rs:88-154),
//                       and with SSA_FLAG_DERIVE_PUBLIC derive_public (:160-174) -- two SHA-512 compressions per child
//   ssa_k_xpub_derive   one lane per CHILD, variable-time (everything is public): derive_normal_public (:235-260)
//   ssa_k_xprv_master   generate_master_key (:66-82), one lane per seed, constant-time
//   ssa_k_hmac_sha512   the debug probe: HMAC-SHA512 of public bytes, any key up to 256 bytes, messages up to 239
//
// parse(I_L) is Scalar::from_bytes_non_canonical of the left half of the MAC, read as the full reduction mod q of the
// 256-bit little-endian integer (q < 2^255: two masked subtractions, sc_reduce256_ct / sc_reduce256).  The cheetah crate
// that defines it is not vendored here, so this reading is stated, not pinned.
#pragma once
#include "sha512.hpp"

namespace ssa {

// per-parent record (u64 words)
constexpr int DRV_IPAD = 0, DRV_OPAD = 8, DRV_MSG_N = 16, DRV_MSG_H = 23, DRV_SK = 30, DRV_PX = 34, DRV_STATUS = 46;
constexpr int DRV_REC_WORDS = 48;                  // 384 B: P at word 34 (byte 272) keeps ld_aff's 16-byte alignment
constexpr u32 DRV_MSG_BITS = (128u + 53u) * 8u;    // both child messages are 53 bytes behind the 128-byte key block
constexpr u32 DRV_NONE = 1u;                       // status: the reference's CtOption is none

// the first 56 bytes of a 53-byte message (bytes 0..48 from `byte`, the index slot 49..52 zero, the 0x80 terminator at
// 53) as seven big-endian words
template <class B>
SSA_DDEV void drv_pack53(u64 (&w)[7], B byte) {
#pragma unroll
    for (int i = 0; i < 7; i++) {
        u64 v = 0;
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const int pos = 8 * i + k;
            v = (v << 8) | (pos < 49 ? (u64)byte(pos < 49 ? pos : 0) : pos == 53 ? 0x80ull : 0ull);
        }
        w[i] = v;
    }
}
// the index i (its little-endian bytes, the reference's &[u8; 4]) in bytes 49..52 of the message: word 6
SSA_DDEV u64 drv_index_bits(u32 idx) {
    return ((u64)(idx & 0xffu) << 48) | ((u64)((idx >> 8) & 0xffu) << 40) | ((u64)((idx >> 16) & 0xffu) << 32) |
           ((u64)(idx >> 24) << 24);
}
// the rest of the inner block
SSA_DDEV void drv_block_tail(u64 (&w)[16]) {
#pragma unroll
    for (int i = 7; i < 15; i++) w[i] = 0;
    w[15] = DRV_MSG_BITS;
}
// sort flag of the compressed form (CompressedPoint bit 6) of a finite public point
SSA_DDEV u32 drv_flag(const aff &p) { return f6_lex_largest(p.y) ? 0x40u : 0x00u; }

// a + b mod q for a, b < q by one masked subtraction (sc_fold_ct)
SSA_DEV sc256 sc_add_mod_ct(const sc256 &a, const sc256 &b) {
    u64 r[5];
    u64 carry = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const u64 s = a.w[i] + b.w[i];
        const u64 c1 = s < a.w[i];
        const u64 s2 = s + carry;
        const u64 c2 = s2 < s;
        r[i] = s2;
        carry = c1 | c2;
    }
    r[4] = carry;
    return sc_fold_ct(r);
}
SSA_DEV u64 sc_is_zero_mask(const sc256 &a) {     // all ones when a == 0, without a branch
    const u64 o = a.w[0] | a.w[1] | a.w[2] | a.w[3];
    return (u64)0 - (u64)(o == 0ull);
}

// ---- secret-touching code: out of line, so that tests/test_derive_ct_static.py can check the bodies ------------------
// HMAC's key states of a 32-byte chain code at cc (little-endian bytes) into pads[0..16)
SSA_FN void ct_hmac_pads(u64 *__restrict__ pads, const u8 *__restrict__ cc) {
    u64 k[4], ip[8], op[8];
#pragma unroll
    for (int i = 0; i < 4; i++) k[i] = ld_u64_le(cc + 8 * i);
    hmac_pads32(k, ip, op);
#pragma unroll
    for (int i = 0; i < 8; i++) {
        pads[DRV_IPAD + i] = ip[i];
        pads[DRV_OPAD + i] = op[i];
    }
}

// an xprv parent sk(32) || cc(32) -> its record's key, hardened-message words and status (MALFORMED for a key that is
// zero or >= q: ExtendedPrivateKey::from_bytes is none, src/derivation.rs:192-207), and the scalar the public key is
// computed from (the key, or 1 for a malformed one: the product never meets the exceptional inputs of k = 0)
SSA_FN void ct_xprv_prep(u64 *__restrict__ rec, sc256 *__restrict__ sk_use, const u8 *__restrict__ parent) {
    const sc256 sk = ld_sc(parent);
    u64 bw = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) {                  // sk - q: the final borrow says sk < q
        const u64 t = sk.w[i] - SC_Q(i);
        const u64 b1 = sk.w[i] < SC_Q(i);
        const u64 b2 = t < bw;
        bw = b1 | b2;
    }
    const u64 ok = (u64)0 - (bw & ~sc_is_zero_mask(sk) & 1ull);
    ct_hmac_pads(rec, parent + 32);
    u64 mh[7];
    drv_pack53(mh, [&](int pos) -> u64 {           // [0; 17] || sk (32 bytes, little-endian)
        const int b = pos - 17 < 0 ? 0 : pos - 17;
        return pos < 17 ? 0ull : (sk.w[b >> 3] >> (8 * (b & 7))) & 0xffull;
    });
#pragma unroll
    for (int i = 0; i < 7; i++) rec[DRV_MSG_H + i] = mh[i];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        rec[DRV_SK + i] = sk.w[i];
        sk_use->w[i] = (sk.w[i] & ok) | ((i == 0 ? 1ull : 0ull) & ~ok);
    }
    rec[DRV_STATUS] = ST_MALFORMED & ~ok;
}

// derive_private (src/derivation.rs:88-154) of one child: the hardened or normal message chosen by select (the
// reference's conditional_select), two compressions from the parent's key states, child = parse(I_L) + sk mod q by
// masked arithmetic.  out[0..4) child scalar, out[4..8) I_R (cc') as little-endian words, out[8] all ones when
// child == 0 (none), else 0.
SSA_FN void ct_xprv_child(u64 *__restrict__ out, const u64 *__restrict__ rec, u32 idx) {
    const bool hard = (idx >> 31) != 0u;
    u64 w[16];
#pragma unroll
    for (int i = 0; i < 7; i++) w[i] = ct_sel(hard, rec[DRV_MSG_N + i], rec[DRV_MSG_H + i]);
    w[6] |= drv_index_bits(idx);
    drv_block_tail(w);
    u64 st[8], op[8];
#pragma unroll
    for (int i = 0; i < 8; i++) {
        st[i] = rec[DRV_IPAD + i];
        op[i] = rec[DRV_OPAD + i];
    }
    sha512_compress(st, w);
    hmac_outer(st, op);
    sc256 t, sk;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        t.w[i] = __builtin_bswap64(st[i]);
        sk.w[i] = rec[DRV_SK + i];
    }
    const sc256 c = sc_add_mod_ct(sc_reduce256_ct(t), sk);
#pragma unroll
    for (int i = 0; i < 4; i++) {
        out[i] = c.w[i];
        out[4 + i] = __builtin_bswap64(st[4 + i]);
    }
    out[8] = sc_is_zero_mask(c);
}

// word i of the 128-byte HMAC key block of generate_master_key's public key b"Cheetah - Master extended key seed"
// (34 bytes, zero-padded): folded to constants
constexpr char DRV_MASTER_KEY[] = "Cheetah - Master extended key seed";
__host__ __device__ constexpr u64 drv_master_key_word(int i) {
    u64 v = 0;
    for (int k = 0; k < 8; k++) {
        const int pos = 8 * i + k;
        v = (v << 8) | (pos < (int)sizeof(DRV_MASTER_KEY) - 1 ? (u64)(u8)DRV_MASTER_KEY[pos] : 0ull);
    }
    return v;
}
static_assert(drv_master_key_word(0) == 0x4368656574616820ULL, "b\"Cheetah \"");

// generate_master_key (src/derivation.rs:66-82): HMAC-SHA512(b"Cheetah - Master extended key seed", seed).
// out as ct_xprv_child.
SSA_FN void ct_master(u64 *__restrict__ out, const u8 *__restrict__ seed) {
    u64 w[16], ip[8], op[8];
#pragma unroll
    for (int i = 0; i < 16; i++) w[i] = drv_master_key_word(i) ^ 0x3636363636363636ULL;
    sha512_iv(ip);
    sha512_compress(ip, w);
#pragma unroll
    for (int i = 0; i < 16; i++) w[i] = drv_master_key_word(i) ^ 0x5c5c5c5c5c5c5c5cULL;
    sha512_iv(op);
    sha512_compress(op, w);
#pragma unroll
    for (int i = 0; i < 4; i++) w[i] = __builtin_bswap64(ld_u64_le(seed + 8 * i));
    w[4] = 0x8000000000000000ULL;
#pragma unroll
    for (int i = 5; i < 15; i++) w[i] = 0;
    w[15] = (128 + 32) * 8;
    sha512_compress(ip, w);
    hmac_outer(ip, op);
    sc256 t;
#pragma unroll
    for (int i = 0; i < 4; i++) t.w[i] = __builtin_bswap64(ip[i]);
    const sc256 c = sc_reduce256_ct(t);
#pragma unroll
    for (int i = 0; i < 4; i++) {
        out[i] = c.w[i];
        out[4 + i] = __builtin_bswap64(ip[4 + i]);
    }
    out[8] = sc_is_zero_mask(c);
}

// ---- kernels -------------------------------------------------------------------------------------------------------
// the parent of child lane i: parent_idx[i], or (no table) 0 for one parent, i for one parent per child
SSA_DDEV size_t drv_parent(const u32 *__restrict__ pidx, size_t m, size_t i) {
    return pidx ? (size_t)pidx[i] : (m == 1 ? 0 : i);
}
SSA_DDEV void st_zero(u8 *__restrict__ p, int bytes) {
    for (int k = 0; k < bytes; k++) p[k] = 0;
}

__global__ void __launch_bounds__(256, 2)
ssa_k_derive_prep(const u64 *__restrict__ ctab, const u64 *__restrict__ gtab, const u8 *__restrict__ parents, size_t m,
                  int xpub, u64 *__restrict__ recs) {
    const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= m) return;
    u64 *rec = recs + (size_t)DRV_REC_WORDS * p;
    aff pk;
    if (xpub) {                                    // public: ExtendedPublicKey::from_bytes (src/derivation.rs:275-290)
        const u8 *par = parents + 81 * p;
        bool inf;
        const u32 st = decompress_lane(par, pk, inf);
        rec[DRV_STATUS] = (st != 0u || inf) ? ST_MALFORMED : ST_OK;
        ct_hmac_pads(rec, par + 49);
        st_aff(rec + DRV_PX, pk);
    } else {
        sc256 k;
        ct_xprv_prep(rec, &k, parents + 64 * p);
        jac pj;
        bool bad;
        ct_base_mul(&pj, &bad, ctab, &k);
        if (bad) pj = add_base_mul(jac_identity(), gtab, k);     // a ~2^-250 event (k != 0 here): the exact code
        ct_to_aff(&pk, &pj);
    }
    // compress(P) (PublicKey::to_bytes): the normal child's message -- P is public on both sides
    const u32 flag = drv_flag(pk);
    u64 mn[7];
    drv_pack53(mn, [&](int pos) -> u64 {
        return pos < 48 ? (fp_canon(pk.x.c[pos >> 3]) >> (8 * (pos & 7))) & 0xffull : (u64)flag;
    });
#pragma unroll
    for (int i = 0; i < 7; i++) rec[DRV_MSG_N + i] = mn[i];
}

// derive_private / derive_public of an xprv: out n x 64 (sk || cc'), or n x 81 (compress([sk]G) || cc') with
// derive_public.  status 0, DRV_NONE (child == 0), ST_MALFORMED (parent does not decode, parent index >= m).
__global__ void __launch_bounds__(256, 2)
ssa_k_xprv_derive(const u64 *__restrict__ recs, size_t m, const u32 *__restrict__ pidx, const u32 *__restrict__ indices,
                  size_t n, int derive_public, const u64 *__restrict__ ctab, const u64 *__restrict__ gtab,
                  u8 *__restrict__ out, u8 *__restrict__ status_out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int len = derive_public ? 81 : 64;
    u8 *o = out + (size_t)len * i;
    const size_t p = drv_parent(pidx, m, i);
    // (the parent index and the parent's validity are public: the caller learns both from the status)
    if (p >= m || recs[(size_t)DRV_REC_WORDS * p + DRV_STATUS] != ST_OK) {
        st_zero(o, len);
        status_out[i] = (u8)ST_MALFORMED;
        return;
    }
    const u64 *rec = recs + (size_t)DRV_REC_WORDS * p;
    u64 c[9];
    ct_xprv_child(c, rec, indices[i]);
    const u64 keep = ~c[8];                        // all ones unless child == 0
    if (derive_public) {
        sc256 k;
#pragma unroll
        for (int j = 0; j < 4; j++) k.w[j] = (c[j] & keep) | ((j == 0 ? 1ull : 0ull) & ~keep);
        jac pj;
        bool bad;
        ct_base_mul(&pj, &bad, ctab, &k);
        if (bad) pj = add_base_mul(jac_identity(), gtab, k);     // as ssa_k_pubkey_ct
        aff pk;
        ct_to_aff(&pk, &pj);
        // the child public key is public from here on
        const u32 flag = drv_flag(pk);
#pragma unroll
        for (int j = 0; j < 6; j++) st_u64_le(o + 8 * j, fp_canon(pk.x.c[j]) & keep);
        o[48] = (u8)(flag & (u32)keep);
#pragma unroll
        for (int j = 0; j < 4; j++) st_u64_le(o + 49 + 8 * j, c[4 + j] & keep);
    } else {
#pragma unroll
        for (int j = 0; j < 4; j++) {
            st_u64_le(o + 8 * j, c[j] & keep);
            st_u64_le(o + 32 + 8 * j, c[4 + j] & keep);
        }
    }
    status_out[i] = (u8)(DRV_NONE & (u32)c[8]);
}

// derive_normal_public of an xpub: children n x 81, pks_out n x 96 (optional, the affine child; zero for the identity),
// pk_inf_out (optional, 1 for the identity child -- a valid child, [0; 48] || 0x80).  status 0, DRV_NONE (hardened
// index, or T = [parse(I_L)]G is the identity), ST_MALFORMED.
__global__ void __launch_bounds__(256, 2)
ssa_k_xpub_derive(const u64 *__restrict__ recs, size_t m, const u32 *__restrict__ pidx, const u32 *__restrict__ indices,
                  size_t n, const u64 *__restrict__ gtab, u8 *__restrict__ children, u8 *__restrict__ pks_out,
                  u8 *__restrict__ inf_out, u8 *__restrict__ status_out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    u8 *o = children + 81 * i;
    const size_t p = drv_parent(pidx, m, i);
    const u32 idx = indices[i];
    u32 st = ST_OK;
    if (p >= m || recs[(size_t)DRV_REC_WORDS * p + DRV_STATUS] != ST_OK) st = ST_MALFORMED;
    else if (idx >> 31) st = DRV_NONE;
    aff c;
    bool inf = false;
    if (st == ST_OK) {
        const u64 *rec = recs + (size_t)DRV_REC_WORDS * p;
        u64 w[16], h[8], op[8];
#pragma unroll
        for (int j = 0; j < 7; j++) w[j] = rec[DRV_MSG_N + j];
        w[6] |= drv_index_bits(idx);
        drv_block_tail(w);
#pragma unroll
        for (int j = 0; j < 8; j++) {
            h[j] = rec[DRV_IPAD + j];
            op[j] = rec[DRV_OPAD + j];
        }
        sha512_compress(h, w);
        hmac_outer(h, op);
        sc256 t;
#pragma unroll
        for (int j = 0; j < 4; j++) t.w[j] = __builtin_bswap64(h[j]);
        const jac T = add_base_mul(jac_identity(), gtab, sc_reduce256(t));
        if (jac_is_identity(T)) {
            st = DRV_NONE;
        } else {
            const jac C = jac_madd(T, ld_aff(rec + DRV_PX));     // exact: T = +-P and the identity are handled
            inf = jac_is_identity(C);
            c = jac_to_aff(C);                                     // (0, 0) for the identity
            const u32 flag = inf ? 0x80u : drv_flag(c);
            st_fp6(o, c.x);
            o[48] = (u8)flag;
#pragma unroll
            for (int j = 0; j < 4; j++) st_u64_le(o + 49 + 8 * j, __builtin_bswap64(h[4 + j]));
        }
    }
    if (st != ST_OK) {
        st_zero(o, 81);
        c.x = f6_zero();
        c.y = f6_zero();
        inf = false;
    }
    if (pks_out) {
        st_fp6(pks_out + 96 * i, c.x);
        st_fp6(pks_out + 96 * i + 48, c.y);
    }
    if (inf_out) inf_out[i] = inf ? 1 : 0;
    status_out[i] = (u8)st;
}

// generate_master_key for n seeds: out n x 64 (sk || cc), status 0 or DRV_NONE (sk == 0)
__global__ void __launch_bounds__(256)
ssa_k_xprv_master(const u8 *__restrict__ seeds, size_t n, u8 *__restrict__ out, u8 *__restrict__ status_out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    u64 c[9];
    ct_master(c, seeds + 32 * i);
    const u64 keep = ~c[8];
    u8 *o = out + 64 * i;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        st_u64_le(o + 8 * j, c[j] & keep);
        st_u64_le(o + 32 + 8 * j, c[4 + j] & keep);
    }
    status_out[i] = (u8)(DRV_NONE & (u32)c[8]);
}

__global__ void __launch_bounds__(256)
ssa_k_hmac_sha512(const u8 *__restrict__ key, u32 klen, const u8 *__restrict__ msgs, u32 mlen, size_t n,
                  u8 *__restrict__ out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    u64 h[8];
    hmac_sha512_bytes(key, klen, msgs + (size_t)mlen * i, mlen, h);
#pragma unroll
    for (int j = 0; j < 8; j++) st_u64_le(out + 64 * i + 8 * j, __builtin_bswap64(h[j]));
}

}  // namespace ssa

// ------------------------------------------------------------------------------------------------------------------
// entry points (include/schnorr_sig_amd.h)
static int derive_args(size_t m, const void *parents, const void *indices, size_t n, const uint32_t *parent_idx,
                       const void *out, const void *status) {
    if (n > SSA_MAX_BATCH || m > SSA_MAX_BATCH) return SSA_ERR_ARG;
    if (n == 0) return 0;
    if (m == 0 || !parents || !indices || !out || !status) return SSA_ERR_ARG;
    if (!parent_idx && m != 1 && m != n) return SSA_ERR_ARG;
    return 0;
}

// the per-parent records into ctx->dv_recs; the caller wipes them (they hold secrets on the xprv side)
static int derive_prep(ssa_ctx *ctx, const uint8_t *d_parents, size_t m, bool xpub) {
    if (ctx->dv_recs.reserve(m * DRV_REC_WORDS * sizeof(u64))) return SSA_ERR_HIP;
    if (!xpub)
        if (int rc = ensure_ctab(ctx)) return rc;
    return timed_launch(ctx, "ssa_k_derive_prep", [&] {
        hipLaunchKernelGGL(ssa_k_derive_prep, dim3(grid_for(m, 256)), dim3(256), 0, ctx->stream, (const u64 *)ctx->ctab.p,
                           (const u64 *)ctx->d_gtab, d_parents, m, xpub ? 1 : 0, (u64 *)ctx->dv_recs.p);
    });
}

extern "C" int ssa_xprv_master_many_device(ssa_ctx *ctx, const uint8_t *d_seeds, size_t n, uint8_t *d_xprvs_out,
                                           uint8_t *d_status_out) {
    if (!ctx || n > SSA_MAX_BATCH || (n && (!d_seeds || !d_xprvs_out || !d_status_out))) return SSA_ERR_ARG;
    if (n == 0) return 0;
    HIP_TRY(hipSetDevice(ctx->device));
    return timed_launch(ctx, "ssa_k_xprv_master", [&] {
        hipLaunchKernelGGL(ssa_k_xprv_master, dim3(grid_for(n, 256)), dim3(256), 0, ctx->stream, d_seeds, n, d_xprvs_out,
                           d_status_out);
    });
}

extern "C" int ssa_xprv_master_many(ssa_ctx *ctx, const uint8_t *seeds, size_t n, uint8_t *xprvs_out,
                                    uint8_t *status_out) {
    if (!ctx || n > SSA_MAX_BATCH || (n && (!seeds || !xprvs_out || !status_out))) return SSA_ERR_ARG;
    if (n == 0) return 0;
    HostCall hc(ctx);
    const u8 *d_seeds = hc.in(ctx->st_sigs, seeds, n * 32, SECRET);
    u8 *d_xprvs = hc.out(ctx->st_aux, xprvs_out, n * 64, 0, SECRET), *d_status = hc.out(ctx->st_status, status_out, n, 16);
    return hc.finish([&] { return ssa_xprv_master_many_device(ctx, d_seeds, n, d_xprvs, d_status); });
}

extern "C" int ssa_xprv_derive_many_device(ssa_ctx *ctx, const uint8_t *d_parents, size_t m, const uint32_t *d_parent_idx,
                                           const uint32_t *d_indices, size_t n, uint32_t flags, uint8_t *d_children_out,
                                           uint8_t *d_status_out) {
    if (!ctx || (flags & ~SSA_FLAG_DERIVE_PUBLIC)) return SSA_ERR_ARG;
    if (int rc = derive_args(m, d_parents, d_indices, n, d_parent_idx, d_children_out, d_status_out)) return rc;
    if (n == 0) return 0;
    HIP_TRY(hipSetDevice(ctx->device));
    SecretWipe wipe{ctx, {{&ctx->dv_recs, m * DRV_REC_WORDS * sizeof(u64)}}};    // behind the launches that read them
    if (int rc = derive_prep(ctx, d_parents, m, false)) return rc;
    const int pub = (flags & SSA_FLAG_DERIVE_PUBLIC) ? 1 : 0;
    return timed_launch(ctx, "ssa_k_xprv_derive", [&] {
        hipLaunchKernelGGL(ssa_k_xprv_derive, dim3(grid_for(n, 256)), dim3(256), 0, ctx->stream, (const u64 *)ctx->dv_recs.p,
                           m, (const u32 *)d_parent_idx, (const u32 *)d_indices, n, pub, (const u64 *)ctx->ctab.p,
                           (const u64 *)ctx->d_gtab, d_children_out, d_status_out);
    });
}

extern "C" int ssa_xprv_derive_many(ssa_ctx *ctx, const uint8_t *parents, size_t m, const uint32_t *parent_idx,
                                    const uint32_t *indices, size_t n, uint32_t flags, uint8_t *children_out,
                                    uint8_t *status_out) {
    if (!ctx || (flags & ~SSA_FLAG_DERIVE_PUBLIC)) return SSA_ERR_ARG;
    if (int rc = derive_args(m, parents, indices, n, parent_idx, children_out, status_out)) return rc;
    if (n == 0) return 0;
    const size_t len = (flags & SSA_FLAG_DERIVE_PUBLIC) ? 81 : 64;
    HostCall hc(ctx);
    const u8 *d_par = hc.in(ctx->st_sigs, parents, m * 64, SECRET);
    const uint32_t *d_idx = hc.in<uint32_t>(ctx->st_off, indices, n * 4),
                   *d_pidx = parent_idx ? hc.in<uint32_t>(ctx->st_inf, parent_idx, n * 4) : nullptr;
    u8 *d_children = hc.out(ctx->st_aux, children_out, n * len, 0, SECRET), *d_status = hc.out(ctx->st_status, status_out, n, 16);
    return hc.finish([&] {
        return ssa_xprv_derive_many_device(ctx, d_par, m, d_pidx, d_idx, n, flags, d_children, d_status);
    });
}

extern "C" int ssa_xpub_derive_many_device(ssa_ctx *ctx, const uint8_t *d_parents, size_t m, const uint32_t *d_parent_idx,
                                           const uint32_t *d_indices, size_t n, uint8_t *d_children_out,
                                           uint8_t *d_pks_out, uint8_t *d_pk_inf_out, uint8_t *d_status_out) {
    if (!ctx) return SSA_ERR_ARG;
    if (int rc = derive_args(m, d_parents, d_indices, n, d_parent_idx, d_children_out, d_status_out)) return rc;
    if (n == 0) return 0;
    HIP_TRY(hipSetDevice(ctx->device));
    if (int rc = derive_prep(ctx, d_parents, m, true)) return rc;
    return timed_launch(ctx, "ssa_k_xpub_derive", [&] {
        hipLaunchKernelGGL(ssa_k_xpub_derive, dim3(grid_for(n, 256)), dim3(256), 0, ctx->stream, (const u64 *)ctx->dv_recs.p,
                           m, (const u32 *)d_parent_idx, (const u32 *)d_indices, n, (const u64 *)ctx->d_gtab,
                           d_children_out, d_pks_out, d_pk_inf_out, d_status_out);
    });
}

extern "C" int ssa_xpub_derive_many(ssa_ctx *ctx, const uint8_t *parents, size_t m, const uint32_t *parent_idx,
                                    const uint32_t *indices, size_t n, uint8_t *children_out, uint8_t *pks_out,
                                    uint8_t *pk_inf_out, uint8_t *status_out) {
    if (!ctx) return SSA_ERR_ARG;
    if (int rc = derive_args(m, parents, indices, n, parent_idx, children_out, status_out)) return rc;
    if (n == 0) return 0;
    HostCall hc(ctx);
    const u8 *d_par = hc.in(ctx->st_pks, parents, m * 81);
    const uint32_t *d_idx = hc.in<uint32_t>(ctx->st_off, indices, n * 4),
                   *d_pidx = parent_idx ? hc.in<uint32_t>(ctx->st_inf, parent_idx, n * 4) : nullptr;
    u8 *d_children = hc.out(ctx->st_aux, children_out, n * 81),
       *d_pks = pks_out ? hc.out(ctx->st_aux2, pks_out, n * 96) : nullptr,
       *d_inf = pk_inf_out ? hc.out(ctx->st_msgs, pk_inf_out, n, 16) : nullptr,
       *d_status = hc.out(ctx->st_status, status_out, n, 16);
    return hc.finish([&] {
        return ssa_xpub_derive_many_device(ctx, d_par, m, d_pidx, d_idx, n, d_children, d_pks, d_inf, d_status);
    });
}

extern "C" int ssa_debug_hmac_sha512(ssa_ctx *ctx, const uint8_t *key, size_t key_len, const uint8_t *msgs,
                                     size_t msg_len, size_t n, uint8_t *out) {
    if (!ctx || key_len > 256 || msg_len > 239 || n > SSA_MAX_BATCH) return SSA_ERR_ARG;
    if (n && (!out || (key_len && !key) || (msg_len && !msgs))) return SSA_ERR_ARG;
    if (n == 0) return 0;
    HostCall hc(ctx);
    const u8 *d_key = hc.in(ctx->st_pks, key_len ? key : nullptr, key_len),
             *d_msgs = hc.in(ctx->st_msgs, msg_len ? msgs : nullptr, n * msg_len);
    u8 *d_out = hc.out(ctx->st_aux, out, n * 64);
    return hc.finish([&] {
        return timed_launch(ctx, "ssa_k_hmac_sha512", [&] {
            hipLaunchKernelGGL(ssa_k_hmac_sha512, dim3(grid_for(n, 256)), dim3(256), 0, ctx->stream, d_key, (u32)key_len,
                               d_msgs, (u32)msg_len, n, d_out);
        });
    });
}
