// Scalar::random(rng) on the device: the nonces of sign(message, rng) and
// sign_and_bind_pkey(message, rng) (reference src/signature.rs:65-156) and the keys of KeyPair::new(rng)
// (src/keypair.rs:57-65, src/private.rs:49-57), drawn where they are used, so that no nonce exists on the host.
//
// Layout (pinned: tests/device_rng_model.py models it):
//   * per call a 44-byte seed S from getrandom(2): ChaCha20 key K = S[0:32], 96-bit nonce N = S[32:44], RFC 8439 blocks
//     with a 32-bit block counter (the block function of msm_k_chacha20, ssa_msm.hip);
//   * lane i -- the index of the scalar in the whole call, across slices -- takes B0 = block(K, 2i, N) and
//     B1 = block(K, 2i + 1, N);
//   * r_i = from_bytes_wide(B0) (the 64 bytes little-endian, mod q: Scalar::from_bytes_wide, as PrivateKey::from_seed),
//     or from_bytes_wide(B1) where that is 0 (probability ~2^-254).  Both blocks are always computed and reduced and the
//     choice is a select.  Both being 0 (probability ~2^-509) is unreachable in practice; the lane would then hold 0,
//     which the signers compute correctly but through their variable-time fallback -- never a fixed, known nonce.
//
// The secret work -- the ChaCha20 rounds on the secret key, the 512-bit reduction and the select -- lives in the
// out-of-line ct_draw_scalar / ct_draw_wide, which tests/test_device_rng_ct_static.py checks with the rules of the
// signer's secret functions.  The seed reaches the kernel through device memory only (kernel arguments are never wiped).
#pragma once

#include <sys/random.h>

namespace ssa {

constexpr size_t RNG_SEED_BYTES = 44;

SSA_DEV u32 rng_rotl32(u32 x, int n) { return (x << n) | (x >> (32 - n)); }
#define SSA_RNG_QR(a, b, c, d)             \
    a += b; d ^= a; d = rng_rotl32(d, 16); \
    c += d; b ^= c; b = rng_rotl32(b, 12); \
    a += b; d ^= a; d = rng_rotl32(d, 8);  \
    c += d; b ^= c; b = rng_rotl32(b, 7)

// one RFC 8439 block: kn = key words 0..7, nonce words 8..10; out = the 16 keystream words (little-endian bytes)
SSA_DEV void rng_chacha_block(u32 (&out)[16], const u32 (&kn)[11], u32 counter) {
    const u32 st[16] = {0x61707865u, 0x3320646eu, 0x79622d32u, 0x6b206574u, kn[0], kn[1], kn[2], kn[3],
                        kn[4], kn[5], kn[6], kn[7], counter, kn[8], kn[9], kn[10]};
#pragma unroll
    for (int i = 0; i < 16; i++) out[i] = st[i];
#pragma unroll 1
    for (int r = 0; r < 10; r++) {          // (r is the loop counter: uniform and public)
        SSA_RNG_QR(out[0], out[4], out[8], out[12]);
        SSA_RNG_QR(out[1], out[5], out[9], out[13]);
        SSA_RNG_QR(out[2], out[6], out[10], out[14]);
        SSA_RNG_QR(out[3], out[7], out[11], out[15]);
        SSA_RNG_QR(out[0], out[5], out[10], out[15]);
        SSA_RNG_QR(out[1], out[6], out[11], out[12]);
        SSA_RNG_QR(out[2], out[7], out[8], out[13]);
        SSA_RNG_QR(out[3], out[4], out[9], out[14]);
    }
#pragma unroll
    for (int i = 0; i < 16; i++) out[i] += st[i];
}

// Scalar::from_bytes_wide of 64 bytes given as 16 little-endian words: lo + hi 2^256 = (lo mod q) + (hi mod q)(2^256 mod q),
// every step masked (sc_reduce256_ct, sc_mul_mod_ct, sc_add_mod_ct)
SSA_DEV sc256 sc_from_wide_ct(const u32 (&b)[16]) {
    sc256 lo, hi;
    const sc256 R2 = {{0x57793b82a256a662ULL, 0x9b0ab1b99fd511baULL, 0x538081e0cdeb9095ULL, 0x0a1b4cc98981ba5fULL}};
#pragma unroll
    for (int k = 0; k < 4; k++) {
        lo.w[k] = mk64(b[2 * k], b[2 * k + 1]);
        hi.w[k] = mk64(b[8 + 2 * k], b[8 + 2 * k + 1]);
    }
    return sc_add_mod_ct(sc_reduce256_ct(lo), sc_mul_mod_ct(sc_reduce256_ct(hi), R2));
}

// the draw rule: from_bytes_wide(B0), or from_bytes_wide(B1) where the first is 0 -- both reduced, a masked select
SSA_DEV void rng_wide_select(u8 *__restrict__ out, const u32 (&b0)[16], const u32 (&b1)[16]) {
    const sc256 r0 = sc_from_wide_ct(b0), r1 = sc_from_wide_ct(b1);
    const u64 z = sc_is_zero_mask(r0);
#pragma unroll
    for (int k = 0; k < 4; k++) st_u64_le(out + 8 * k, (r0.w[k] & ~z) | (r1.w[k] & z));
}

// the scalar of lane `lane` under the seed at `seed` (11 words: K, N) -> 32 bytes at out
SSA_FN void ct_draw_scalar(u8 *__restrict__ out, const u32 *__restrict__ seed, u32 lane) {
    u32 kn[11];
#pragma unroll
    for (int k = 0; k < 11; k++) kn[k] = seed[k];
    const u32 ctr = 2u * lane;
    u32 b0[16], b1[16];
    rng_chacha_block(b0, kn, ctr);
    rng_chacha_block(b1, kn, ctr + 1u);
    rng_wide_select(out, b0, b1);
}

// the same rule on caller-supplied blocks (B0 || B1, 128 bytes): ssa_debug_draw_scalars
SSA_FN void ct_draw_wide(u8 *__restrict__ out, const u8 *__restrict__ blocks) {
    u32 b0[16], b1[16];
#pragma unroll
    for (int k = 0; k < 16; k++) {
        b0[k] = (u32)blocks[4 * k] | (u32)blocks[4 * k + 1] << 8 | (u32)blocks[4 * k + 2] << 16 | (u32)blocks[4 * k + 3] << 24;
        b1[k] = (u32)blocks[64 + 4 * k] | (u32)blocks[65 + 4 * k] << 8 | (u32)blocks[66 + 4 * k] << 16 |
                (u32)blocks[67 + 4 * k] << 24;
    }
    rng_wide_select(out, b0, b1);
}

// lanes lane0 .. lane0 + n - 1 of the call -> n x 32 bytes at out (the pre-pass of the _rng signers and of
// ssa_signer_set_generate; the signing kernels then read `out` as their nonces, unchanged)
__global__ void __launch_bounds__(256)
ssa_k_draw_scalars_ct(const u32 *__restrict__ seed, size_t lane0, size_t n, u8 *__restrict__ out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const u32 lane = (u32)(lane0 + i);      // < SSA_MAX_BATCH = 2^30: the counters 2i, 2i + 1 fit 32 bits
    ct_draw_scalar(out + 32 * i, seed, lane);
}

__global__ void __launch_bounds__(256)
ssa_k_draw_wide(const u8 *__restrict__ blocks, size_t n, u8 *__restrict__ out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    ct_draw_wide(out + 32 * i, blocks + 128 * i);
}

}  // namespace ssa

// ---- host side ---------------------------------------------------------------------------------------------------
static void rng_wipe_host(void *p, size_t bytes) {      // a wipe the compiler may not drop
    volatile uint8_t *v = (volatile uint8_t *)p;
    for (size_t i = 0; i < bytes; i++) v[i] = 0;
}

// the call's seed into ctx->rng_seed (device) through the library's page-locked ctx->pin_seed, which is wiped before
// this returns.  The copy is complete when it returns (so it waits for the work queued before it on the stream): the
// host copy can then be wiped, and a later call cannot overwrite a seed an earlier one has yet to read.
static int rng_stage_seed(ssa_ctx *ctx) {
    if (ctx->rng_seed.reserve(64) || ctx->pin_seed.reserve(64)) return SSA_ERR_HIP;
    uint8_t *h = (uint8_t *)ctx->pin_seed.p;
    struct HostWipe {
        uint8_t *p;
        ~HostWipe() { rng_wipe_host(p, RNG_SEED_BYTES); }
    } host_wipe{h};
    if (ctx->rng_pinned) {
        std::memcpy(h, ctx->rng_pin, RNG_SEED_BYTES);
    } else {
        size_t got = 0;
        while (got < RNG_SEED_BYTES) {
            const ssize_t r = getrandom(h + got, RNG_SEED_BYTES - got, 0);
            if (r <= 0) return SSA_ERR_HIP;
            got += (size_t)r;
        }
    }
    HIP_TRY(hipMemcpyAsync(ctx->rng_seed.p, h, RNG_SEED_BYTES, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return 0;
}

// n scalars drawn slice by slice (at most ctx->knobs.lane_slice lanes of scratch, 32 B each), each slice handed to
// consume(lo, cnt, d_scalars) on the context's stream.  The device seed and the scratch are zeroed on the stream
// after the last consumer, whichever way this returns.
template <class F>
static int rng_draw_slices(ssa_ctx *ctx, size_t n, F &&consume) {
    const size_t slice = ctx->knobs.lane_slice < n ? ctx->knobs.lane_slice : n;
    if (ctx->rng_scratch.reserve(slice * 32)) return SSA_ERR_HIP;
    SecretWipe wipe{ctx, {{&ctx->rng_scratch, slice * 32}, {&ctx->rng_seed, 64}}};
    if (int rc = rng_stage_seed(ctx)) return rc;
    for (size_t lo = 0; lo < n; lo += slice) {
        const size_t cnt = n - lo < slice ? n - lo : slice;
        if (int rc = timed_launch(ctx, "ssa_k_draw_scalars_ct", [&] {
                hipLaunchKernelGGL(ssa_k_draw_scalars_ct, dim3(grid_for(cnt, 256)), dim3(256), 0, ctx->stream,
                                   (const u32 *)ctx->rng_seed.p, lo, cnt, (u8 *)ctx->rng_scratch.p);
            }))
            return rc;
        if (int rc = consume(lo, cnt, (const u8 *)ctx->rng_scratch.p)) return rc;
    }
    return 0;
}

extern "C" int ssa_keygen_sign_many_rng_device(ssa_ctx *ctx, const uint8_t *d_sks, const uint8_t *d_msgs,
                                               const uint64_t *d_msg_off, size_t msg_stride, size_t msg_len, size_t n,
                                               uint32_t flags, uint8_t *d_pks_out, uint8_t *d_sigs_out) {
    if (!ctx || (flags & ~(SSA_FLAG_SIGN_CT | SSA_FLAG_SIGN_KEYED))) return SSA_ERR_ARG;
    const bool keyed = (flags & SSA_FLAG_SIGN_KEYED) != 0;
    if (n && (!d_sks || !d_sigs_out || (!keyed && !d_pks_out))) return SSA_ERR_ARG;
    const DevBatch b{nullptr, nullptr, nullptr, {d_msgs, d_msg_off, msg_stride, msg_len}};     // (the messages only)
    if (int rc = check_msgs(b.msgs, n)) return rc;
    if (n == 0) return 0;
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t rec = keyed ? 130 : 81;
    return rng_draw_slices(ctx, n, [&](size_t lo, size_t cnt, const u8 *d_nonces) {
        const MsgView mv = b.slice(lo).msgs;
        return ssa_keygen_sign_many_ex_device(ctx, d_sks + 32 * lo, d_nonces, mv.msgs, mv.off, mv.stride, mv.len, cnt, flags,
                                              d_pks_out ? d_pks_out + 96 * lo : nullptr, d_sigs_out + rec * lo);
    });
}

extern "C" int ssa_keygen_sign_many_rng(ssa_ctx *ctx, const uint8_t *sks, const uint8_t *msgs, const uint64_t *msg_off,
                                        size_t msg_stride, size_t msg_len, size_t n, uint32_t flags, uint8_t *pks_out,
                                        uint8_t *sigs_out) {
    if (!ctx || (flags & ~(SSA_FLAG_SIGN_CT | SSA_FLAG_SIGN_KEYED))) return SSA_ERR_ARG;
    const bool keyed = (flags & SSA_FLAG_SIGN_KEYED) != 0;
    if (n && (!sks || !sigs_out || (!keyed && !pks_out))) return SSA_ERR_ARG;
    if (int rc = check_msgs({msgs, msg_off, msg_stride, msg_len}, n)) return rc;
    if (int rc = check_host_offsets(msg_off, n)) return rc;
    if (n == 0) return 0;
    if (!scalars_canonical_nonzero(sks, n)) return SSA_ERR_ARG;
    HostCall hc(ctx);
    const u8 *d_sks = hc.in(ctx->st_sigs, sks, n * 32, SECRET);
    const MsgView mv = hc.msgs(msgs, msg_off, msg_stride, msg_len, n);
    u8 *d_pks = hc.out(ctx->st_aux, pks_out, n * 96), *d_sigs = hc.out(ctx->st_aux2, sigs_out, n * (keyed ? 130 : 81));
    return hc.finish([&] {
        return ssa_keygen_sign_many_rng_device(ctx, d_sks, mv.msgs, mv.off, msg_stride, msg_len, n, flags, d_pks, d_sigs);
    });
}

extern "C" int ssa_sign_many_indexed_rng_device(ssa_ctx *ctx, ssa_signer_set *ss, const uint32_t *d_key_idx,
                                                const uint8_t *d_msgs, const uint64_t *d_msg_off, size_t msg_stride,
                                                size_t msg_len, size_t n, uint32_t flags, uint8_t *d_sigs_out,
                                                uint8_t *d_status_out) {
    if (!ctx || !ss || ss->ctx != ctx || (flags & ~(SSA_FLAG_SIGN_CT | SSA_FLAG_SIGN_KEYED))) return SSA_ERR_ARG;
    if (n && (!d_key_idx || !d_sigs_out)) return SSA_ERR_ARG;
    const DevBatch b{nullptr, nullptr, nullptr, {d_msgs, d_msg_off, msg_stride, msg_len}};     // (the messages only)
    if (int rc = check_msgs(b.msgs, n)) return rc;
    if (n == 0) return 0;
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t rec = (flags & SSA_FLAG_SIGN_KEYED) ? 130 : 81;
    return rng_draw_slices(ctx, n, [&](size_t lo, size_t cnt, const u8 *d_nonces) {
        const MsgView mv = b.slice(lo).msgs;
        return ssa_sign_many_indexed_device(ctx, ss, d_key_idx + lo, d_nonces, mv.msgs, mv.off, mv.stride, mv.len, cnt, flags,
                                            d_sigs_out + rec * lo, d_status_out ? d_status_out + lo : nullptr);
    });
}

extern "C" int ssa_sign_many_indexed_rng(ssa_ctx *ctx, ssa_signer_set *ss, const uint32_t *key_idx, const uint8_t *msgs,
                                         const uint64_t *msg_off, size_t msg_stride, size_t msg_len, size_t n,
                                         uint32_t flags, uint8_t *sigs_out) {
    if (!ctx || !ss || ss->ctx != ctx || (flags & ~(SSA_FLAG_SIGN_CT | SSA_FLAG_SIGN_KEYED))) return SSA_ERR_ARG;
    if (n && (!key_idx || !sigs_out)) return SSA_ERR_ARG;
    if (int rc = check_msgs({msgs, msg_off, msg_stride, msg_len}, n)) return rc;
    if (int rc = check_host_offsets(msg_off, n)) return rc;
    if (n == 0) return 0;
    for (size_t i = 0; i < n; i++)                 // (indices are public)
        if (key_idx[i] >= ss->m || ss->host_status[key_idx[i]] != ST_OK) return SSA_ERR_ARG;
    HostCall hc(ctx);
    const uint32_t *d_idx = hc.in<uint32_t>(ctx->st_inf, key_idx, n * sizeof(uint32_t));
    const MsgView mv = hc.msgs(msgs, msg_off, msg_stride, msg_len, n);
    u8 *d_sigs = hc.out(ctx->st_aux2, sigs_out, n * ((flags & SSA_FLAG_SIGN_KEYED) ? 130 : 81));
    return hc.finish([&] {
        return ssa_sign_many_indexed_rng_device(ctx, ss, d_idx, mv.msgs, mv.off, msg_stride, msg_len, n, flags, d_sigs,
                                                nullptr);
    });
}

// KeyPair::new(rng) for m key pairs: the keys are drawn straight into the set (slice by slice through the scratch),
// checked by ssa_k_signer_keys and published by the path of ssa_signer_set_create_device
extern "C" int ssa_signer_set_generate(ssa_ctx *ctx, size_t m, ssa_signer_set **out) {
    if (!ctx || !out || m == 0 || m > SSA_MAX_BATCH) return SSA_ERR_ARG;
    *out = nullptr;
    HIP_TRY(hipSetDevice(ctx->device));
    ssa_signer_set *ss = new ssa_signer_set();
    ss->ctx = ctx;
    ss->m = m;
    int rc = signer_set_reserve(ss);
    if (!rc)
        rc = rng_draw_slices(ctx, m, [&](size_t lo, size_t cnt, const u8 *d_sks) {
            return signer_set_keys(ctx, ss, d_sks, 32, lo, cnt);
        });
    if (!rc) rc = signer_set_publish(ctx, ss);
    if (rc) {
        ssa_signer_set_destroy(ss);
        return rc;
    }
    ctx->signer_sets.push_back(ss);
    *out = ss;
    return 0;
}

extern "C" int ssa_signer_set_secret_keys(ssa_signer_set *ss, uint8_t *sks_out) {
    if (!ss || !ss->ctx || !sks_out) return SSA_ERR_ARG;
    HostCall hc(ss->ctx);
    hc.copy_back(sks_out, ss->sks.p, ss->m * 32);
    return hc.finish([] { return 0; });
}

extern "C" int ssa_debug_pin_rng(ssa_ctx *ctx, const uint8_t *seed) {
    if (!ctx) return SSA_ERR_ARG;
    if (seed) std::memcpy(ctx->rng_pin, seed, RNG_SEED_BYTES);
    else rng_wipe_host(ctx->rng_pin, RNG_SEED_BYTES);
    ctx->rng_pinned = seed != nullptr;
    return 0;
}

extern "C" int ssa_debug_draw_scalars(ssa_ctx *ctx, const uint8_t *blocks, size_t n, uint8_t *out) {
    if (!ctx || (n && (!blocks || !out)) || n > SSA_MAX_BATCH) return SSA_ERR_ARG;
    if (n == 0) return 0;
    HostCall hc(ctx);
    const u8 *d_blocks = hc.in(ctx->st_aux, blocks, n * 128);
    u8 *d_out = hc.out(ctx->st_aux2, out, n * 32);
    return hc.finish([&] {
        return timed_launch(ctx, "ssa_k_draw_wide", [&] {
            hipLaunchKernelGGL(ssa_k_draw_wide, dim3(grid_for(n, 256)), dim3(256), 0, ctx->stream, d_blocks, n, d_out);
        });
    });
}
