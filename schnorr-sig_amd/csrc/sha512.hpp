// SHA-512 (FIPS 180-4) and HMAC-SHA512 (RFC 2104) on the GPU, one message per lane: what hierarchical key derivation
// hashes (reference src/derivation.rs:66-82, :100-110, :129-137, :238-244; ssa_derive.hpp).
//
//   * the 8-word state and a rolling 16-word message schedule stay in VGPRs (the 80 rounds run as five fully unrolled
//     blocks of 16, so every schedule index is a compile-time constant);
//   * the 80 round constants are wave-uniform scalar loads from a __constant__ table, indexed by the round counter only;
//   * 64-bit rotates are v_alignbit_b32 pairs, Ch and Maj are written in the shape the compiler maps to v_bfi_b32;
//   * no branch on data and no table indexed by data: the same code serves the secret inputs of the xprv side.
// Message words are big-endian (byte 0 of a block is the top byte of w[0]).
#pragma once
#include "fp.hpp"

namespace ssa {

#define SSA_DDEV __device__ __forceinline__

__constant__ u64 SHA512_K[80] = {
    0x428a2f98d728ae22ULL, 0x7137449123ef65cdULL, 0xb5c0fbcfec4d3b2fULL, 0xe9b5dba58189dbbcULL, 0x3956c25bf348b538ULL,
    0x59f111f1b605d019ULL, 0x923f82a4af194f9bULL, 0xab1c5ed5da6d8118ULL, 0xd807aa98a3030242ULL, 0x12835b0145706fbeULL,
    0x243185be4ee4b28cULL, 0x550c7dc3d5ffb4e2ULL, 0x72be5d74f27b896fULL, 0x80deb1fe3b1696b1ULL, 0x9bdc06a725c71235ULL,
    0xc19bf174cf692694ULL, 0xe49b69c19ef14ad2ULL, 0xefbe4786384f25e3ULL, 0x0fc19dc68b8cd5b5ULL, 0x240ca1cc77ac9c65ULL,
    0x2de92c6f592b0275ULL, 0x4a7484aa6ea6e483ULL, 0x5cb0a9dcbd41fbd4ULL, 0x76f988da831153b5ULL, 0x983e5152ee66dfabULL,
    0xa831c66d2db43210ULL, 0xb00327c898fb213fULL, 0xbf597fc7beef0ee4ULL, 0xc6e00bf33da88fc2ULL, 0xd5a79147930aa725ULL,
    0x06ca6351e003826fULL, 0x142929670a0e6e70ULL, 0x27b70a8546d22ffcULL, 0x2e1b21385c26c926ULL, 0x4d2c6dfc5ac42aedULL,
    0x53380d139d95b3dfULL, 0x650a73548baf63deULL, 0x766a0abb3c77b2a8ULL, 0x81c2c92e47edaee6ULL, 0x92722c851482353bULL,
    0xa2bfe8a14cf10364ULL, 0xa81a664bbc423001ULL, 0xc24b8b70d0f89791ULL, 0xc76c51a30654be30ULL, 0xd192e819d6ef5218ULL,
    0xd69906245565a910ULL, 0xf40e35855771202aULL, 0x106aa07032bbd1b8ULL, 0x19a4c116b8d2d0c8ULL, 0x1e376c085141ab53ULL,
    0x2748774cdf8eeb99ULL, 0x34b0bcb5e19b48a8ULL, 0x391c0cb3c5c95a63ULL, 0x4ed8aa4ae3418acbULL, 0x5b9cca4f7763e373ULL,
    0x682e6ff3d6b2b8a3ULL, 0x748f82ee5defb2fcULL, 0x78a5636f43172f60ULL, 0x84c87814a1f0ab72ULL, 0x8cc702081a6439ecULL,
    0x90befffa23631e28ULL, 0xa4506cebde82bde9ULL, 0xbef9a3f7b2c67915ULL, 0xc67178f2e372532bULL, 0xca273eceea26619cULL,
    0xd186b8c721c0c207ULL, 0xeada7dd6cde0eb1eULL, 0xf57d4f7fee6ed178ULL, 0x06f067aa72176fbaULL, 0x0a637dc5a2c898a6ULL,
    0x113f9804bef90daeULL, 0x1b710b35131c471bULL, 0x28db77f523047d84ULL, 0x32caab7b40c72493ULL, 0x3c9ebe0a15c9bebcULL,
    0x431d67c49c100d4cULL, 0x4cc5d4becb3e42b6ULL, 0x597f299cfc657e2aULL, 0x5fcb6fab3ad6faecULL, 0x6c44198c4a475817ULL};

SSA_DDEV void sha512_iv(u64 (&st)[8]) {
    st[0] = 0x6a09e667f3bcc908ULL;
    st[1] = 0xbb67ae8584caa73bULL;
    st[2] = 0x3c6ef372fe94f82bULL;
    st[3] = 0xa54ff53a5f1d36f1ULL;
    st[4] = 0x510e527fade682d1ULL;
    st[5] = 0x9b05688c2b3e6c1fULL;
    st[6] = 0x1f83d9abfb41bd6bULL;
    st[7] = 0x5be0cd19137e2179ULL;
}

// x >>> n for a constant n: two v_alignbit_b32 (each half is a funnel shift of the two halves)
SSA_DDEV u64 sha_rotr(u64 x, int n) {
    const u32 lo = (u32)x, hi = (u32)(x >> 32);
    if (n < 32) return mk64(__builtin_amdgcn_alignbit(hi, lo, n), __builtin_amdgcn_alignbit(lo, hi, n));
    return mk64(__builtin_amdgcn_alignbit(lo, hi, n - 32), __builtin_amdgcn_alignbit(hi, lo, n - 32));
}

// one round; j is a compile-time constant, k the round constant (a scalar register)
SSA_DDEV void sha512_round(u64 &a, u64 &b, u64 &c, u64 &d, u64 &e, u64 &f, u64 &g, u64 &h, u64 k, u64 wj) {
    const u64 S1 = sha_rotr(e, 14) ^ sha_rotr(e, 18) ^ sha_rotr(e, 41);
    const u64 ch = (e & f) | (~e & g);                         // v_bfi_b32
    const u64 t1 = h + S1 + ch + k + wj;
    const u64 S0 = sha_rotr(a, 28) ^ sha_rotr(a, 34) ^ sha_rotr(a, 39);
    const u64 ab = a ^ b;
    const u64 maj = (ab & c) | (~ab & b);                      // v_bfi_b32: a != b -> c, else b
    h = g;
    g = f;
    f = e;
    e = d + t1;
    d = c;
    c = b;
    b = a;
    a = t1 + S0 + maj;
}

// one compression: st <- st + F(st, w).  w is consumed (it holds the rolling schedule afterwards).
SSA_DDEV void sha512_compress(u64 (&st)[8], u64 (&w)[16]) {
    u64 a = st[0], b = st[1], c = st[2], d = st[3], e = st[4], f = st[5], g = st[6], h = st[7];
#pragma unroll
    for (int j = 0; j < 16; j++) sha512_round(a, b, c, d, e, f, g, h, SHA512_K[j], w[j]);
#pragma unroll 1
    for (int r = 16; r < 80; r += 16) {        // r: the round counter, uniform (scalar compare + scalar branch)
#pragma unroll
        for (int j = 0; j < 16; j++) {
            const u64 w2 = w[(j + 14) & 15], w15 = w[(j + 1) & 15];
            const u64 s1 = sha_rotr(w2, 19) ^ sha_rotr(w2, 61) ^ (w2 >> 6);
            const u64 s0 = sha_rotr(w15, 1) ^ sha_rotr(w15, 8) ^ (w15 >> 7);
            w[j] += s1 + w[(j + 9) & 15] + s0;
            sha512_round(a, b, c, d, e, f, g, h, SHA512_K[r + j], w[j]);
        }
    }
    st[0] += a;
    st[1] += b;
    st[2] += c;
    st[3] += d;
    st[4] += e;
    st[5] += f;
    st[6] += g;
    st[7] += h;
}

// HMAC's two intermediate states for a key of 32 bytes given as four little-endian words (k[0] = bytes 0..7, the
// layout of ld_u64_le): ipad = F(IV, K ^ 0x36..), opad = F(IV, K ^ 0x5c..) -- computed once per key.
SSA_DDEV void hmac_pads32(const u64 (&k)[4], u64 (&ipad)[8], u64 (&opad)[8]) {
    u64 w[16];
#pragma unroll
    for (int i = 0; i < 16; i++) w[i] = (i < 4 ? __builtin_bswap64(k[i < 4 ? i : 0]) : 0ull) ^ 0x3636363636363636ULL;
    sha512_iv(ipad);
    sha512_compress(ipad, w);
#pragma unroll
    for (int i = 0; i < 16; i++) w[i] = (i < 4 ? __builtin_bswap64(k[i < 4 ? i : 0]) : 0ull) ^ 0x5c5c5c5c5c5c5c5cULL;
    sha512_iv(opad);
    sha512_compress(opad, w);
}

// the outer hash of HMAC: st <- F(opad, inner digest || padding), total length 128 + 64 bytes
SSA_DDEV void hmac_outer(u64 (&st)[8], const u64 (&opad)[8]) {
    u64 w[16];
#pragma unroll
    for (int i = 0; i < 8; i++) w[i] = st[i];
    w[8] = 0x8000000000000000ULL;
#pragma unroll
    for (int i = 9; i < 15; i++) w[i] = 0;
    w[15] = (128 + 64) * 8;
#pragma unroll
    for (int i = 0; i < 8; i++) st[i] = opad[i];
    sha512_compress(st, w);
}

// ---- byte-oriented forms (public data only: the loops run over public lengths) ------------------------------------
// the blocks of `len` bytes at p, padded, after `prefix` bytes already absorbed into st
SSA_DDEV void sha512_absorb_tail(u64 (&st)[8], const u8 *__restrict__ p, u32 len, u32 prefix) {
    const u32 nblk = (len + 17u + 127u) / 128u;
    const u64 bits = (u64)(prefix + len) * 8u;
    for (u32 b = 0; b < nblk; b++) {
        u64 w[16];
#pragma unroll
        for (int i = 0; i < 16; i++) {
            u64 v = 0;
            for (int k = 0; k < 8; k++) {
                const u32 pos = b * 128u + 8u * (u32)i + (u32)k;
                u32 byte = 0;
                if (pos < len) byte = p[pos];
                else if (pos == len) byte = 0x80u;
                v = (v << 8) | byte;
            }
            w[i] = v;
        }
        if (b + 1 == nblk) w[15] = bits;     // (len + 17 <= 128 nblk: the length field never overlaps data)
        sha512_compress(st, w);
    }
}

// HMAC-SHA512(key, msg) for any key length (keys longer than the 128-byte block are hashed first, RFC 2104) -> the
// 64-byte MAC as eight big-endian words
SSA_DDEV void hmac_sha512_bytes(const u8 *__restrict__ key, u32 klen, const u8 *__restrict__ msg, u32 mlen,
                                u64 (&out)[8]) {
    u64 kw[16];
    if (klen > 128u) {
        u64 kh[8];
        sha512_iv(kh);
        sha512_absorb_tail(kh, key, klen, 0);
#pragma unroll
        for (int i = 0; i < 16; i++) kw[i] = i < 8 ? kh[i < 8 ? i : 0] : 0ull;
    } else {
#pragma unroll
        for (int i = 0; i < 16; i++) {
            u64 v = 0;
            for (int k = 0; k < 8; k++) {
                const u32 pos = 8u * (u32)i + (u32)k;
                v = (v << 8) | (pos < klen ? (u64)key[pos] : 0ull);
            }
            kw[i] = v;
        }
    }
    u64 w[16], opad[8];
#pragma unroll
    for (int i = 0; i < 16; i++) w[i] = kw[i] ^ 0x5c5c5c5c5c5c5c5cULL;
    sha512_iv(opad);
    sha512_compress(opad, w);
#pragma unroll
    for (int i = 0; i < 16; i++) w[i] = kw[i] ^ 0x3636363636363636ULL;
    sha512_iv(out);
    sha512_compress(out, w);
    sha512_absorb_tail(out, msg, mlen, 128);
    hmac_outer(out, opad);
}

}  // namespace ssa
