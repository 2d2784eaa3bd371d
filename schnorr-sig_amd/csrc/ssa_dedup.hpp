// Internal: the distinct public keys of one slice of lanes, found on the device (ssa_verify_many_dedup, DESIGN.md
// section 14), and with them the ONE notion of what identifies a key, for the dedup and for the key caches built on it
// (ssa_keycache.hpp, ssa_keyed.hpp).
//
// A key is WORDS 64-bit words.  An AFFINE key is the 12 words of its 96 bytes and its pk_inf flag as 0 / 1 (97 bytes); a
// WIRE key is the 49 compressed bytes in front of a 130-byte record as received: six words of x and the flag byte.  A
// "source" is a small struct of pointers that gives the words of the key at an index: of a lane of wire records
// (DdWireLanes) or of a row of a key cache (DdAffineRows, DdWireRows); an affine lane is read by dd_key_word and
// dd_key_flag.  Two keys are the same key exactly when all their words are equal (dd_same_key), and the fingerprint
// (dd_fingerprint: ONE SipHash-2-4, under the context's random 128-bit key) is taken over the same words, so every
// kernel below and in the two cache headers agrees on both.
// The fingerprint is keyed because public keys are chosen by the sender: without the key a sender could build long
// probe chains.  It only picks slots: equality is never decided on the fingerprint.
//
// Input: cnt <= lane_slice lanes.  Output: u, the u representative lanes reps[0..u), and key_idx[i] < u for every lane,
// with key_idx[i] == key_idx[j] ONLY IF the two lanes hold the same key.  (The converse holds too unless a lane ran
// into the probe bound: such a lane becomes a key of its own, which is always correct and only costs time.)
//
//   dd_k_insert   (affine lanes; dd_insert_body is the same loop over a lane source, the body of ky_k_insert)  the
//                 fingerprint picks the first slot of an open-addressing table of 64-bit words (fingerprint's upper half << 32 | owner lane;
//                 all ones = empty; at least four slots per lane).  An empty slot is claimed by compare-and-swap: the
//                 claimant is the key's representative.  A taken slot with the same upper half is a CANDIDATE: the lane
//                 compares its words with the owner's, in the caller's input, and joins it only when they are equal;
//                 anything else moves on to the next slot (linear probing), at most `bound` slots in all.
//   dd_k_scan / dd_k_number / dd_k_index   number the representatives by a prefix sum over the lanes (per-workgroup
//                 counts from the insert, one workgroup scans them) and give every lane its representative's number.
//   dd_k_gather   the representatives' affine keys and flags, compacted (what ssa_k_keyset_build reads).
//
// Memory model, for this file and the two cache headers.  Between workgroups of ONE launch nothing is exchanged but the
// slot words, and those only through agent-scope atomics (a compare-and-swap decides every claim; the load in front of
// it only saves the swap when the slot is taken, and a slot changes once, from empty to owned: a stale read costs one
// failed swap, never a wrong answer).  What a lane reads behind a slot word was written before the launch: the caller's
// input, or cache rows completed by an earlier launch.  Everything a kernel writes with ordinary stores is read by a
// LATER launch on the same stream.  Which lane represents a key depends on the order in which the waves arrive; the
// classes, u and therefore every status do not (a lane that hits the probe bound may or may not do so in another run:
// it then verifies against its own copy of the same key, with the same result).
#pragma once
#include "ssa_kernels.hpp"

namespace ssa {

constexpr u64 DD_EMPTY = ~0ull;
constexpr u32 DD_BLOCK = 256;

// slots of the table for cnt lanes: a power of two, at least four per lane (load <= 1/4: 1.2 probes on average)
__host__ __device__ inline size_t dd_slots_for(size_t cnt) {
    size_t cap = 1024;
    while (cap < 4 * cnt) cap <<= 1;
    return cap;
}

#define DD_SIPROUND(v0, v1, v2, v3)                              \
    do {                                                         \
        v0 += v1; v1 = (v1 << 13) | (v1 >> 51); v1 ^= v0;        \
        v0 = (v0 << 32) | (v0 >> 32);                            \
        v2 += v3; v3 = (v3 << 16) | (v3 >> 48); v3 ^= v2;        \
        v0 += v3; v3 = (v3 << 21) | (v3 >> 43); v3 ^= v0;        \
        v2 += v1; v1 = (v1 << 17) | (v1 >> 47); v1 ^= v2;        \
        v2 = (v2 << 32) | (v2 >> 32);                            \
    } while (0)

// SipHash-2-4 (Aumasson, Bernstein 2012) of a key of L bytes given as W little-endian words, the last one partly
// filled (8 * (W - 1) < L < 8 * W, its unused bytes zero): the last word absorbed carries the length in its top byte
template <int W, int L>
SSA_DEV u64 dd_fingerprint(const u64 w[W], u64 k0, u64 k1) {
    static_assert(8 * (W - 1) < L && L < 8 * W && L < 256, "the length byte shares the last word");
    u64 v0 = k0 ^ 0x736f6d6570736575ull, v1 = k1 ^ 0x646f72616e646f6dull, v2 = k0 ^ 0x6c7967656e657261ull,
        v3 = k1 ^ 0x7465646279746573ull;
#pragma unroll
    for (int k = 0; k < W; k++) {
        const u64 m = k < W - 1 ? w[k] : (w[W - 1] | ((u64)L << 56));
        v3 ^= m;
        DD_SIPROUND(v0, v1, v2, v3);
        DD_SIPROUND(v0, v1, v2, v3);
        v0 ^= m;
    }
    v2 ^= 0xffull;
#pragma unroll
    for (int k = 0; k < 4; k++) DD_SIPROUND(v0, v1, v2, v3);
    return v0 ^ v1 ^ v2 ^ v3;
}

// word k of lane i's key (the caller's buffer need not be aligned: then byte by byte)
SSA_DEV u64 dd_key_word(const u8 *__restrict__ pks, size_t i, int k, bool aligned) {
    const u8 *p = pks + 96 * i + 8 * k;
    return aligned ? *reinterpret_cast<const u64 *>(p) : ld_u64_le(p);
}
SSA_DEV u32 dd_key_flag(const u8 *__restrict__ pk_inf, size_t i) { return pk_inf && pk_inf[i] ? 1u : 0u; }

constexpr int KY_WIRE_WORDS = 7;      // a wire key's 49 bytes: six words of x, one word holding the flag byte

// word k < 6 of x, or (k == 6) the flag byte, of wire key i; the keys are `stride` bytes apart: 130 in front of wire
// records, 49 side by side (never aligned either way)
SSA_DEV u64 ky_wire_word(const u8 *__restrict__ keyed, size_t i, int k, u32 stride) {
    const u8 *p = keyed + (size_t)stride * i;
    return k < 6 ? ld_u64_le(p + 8 * k) : (u64)p[48];
}

// the affine key's fingerprint from its 12 words and its flag (0 / 1): the 97 bytes
SSA_DEV u64 dd_fingerprint(const u64 w[12], u32 flag, u64 k0, u64 k1) {
    u64 v[13];
#pragma unroll
    for (int k = 0; k < 12; k++) v[k] = w[k];
    v[12] = flag;
    return dd_fingerprint<13, 97>(v, k0, k1);
}

// ---- the sources (see the head of this file): a key has WORDS words in BYTES bytes; word(index, k) is word k of the
// key at an index (k is a constant after unrolling).  For affine keys "all words equal" is "the 96 bytes equal and the
// flags agree as booleans".
struct DdWireLanes {
    static constexpr int WORDS = KY_WIRE_WORDS, BYTES = 49;
    const u8 *keyed;
    u32 stride = 130;       // bytes from one lane's key to the next: wire records by default, 49 for dense keys
    SSA_DEV u64 word(size_t i, int k) const { return ky_wire_word(keyed, i, k, stride); }
};
struct DdAffineRows {
    static constexpr int WORDS = 13, BYTES = 97;
    const u64 *c_pks;
    const u8 *c_inf;
    SSA_DEV u64 word(size_t r, int k) const { return k < 12 ? c_pks[r * 12 + k] : (c_inf[r] ? 1u : 0u); }
};
struct DdWireRows {
    static constexpr int WORDS = KY_WIRE_WORDS, BYTES = 49;
    const u64 *c_wire;
    SSA_DEV u64 word(size_t r, int k) const { return c_wire[r * WORDS + k]; }
};

// all the words of the key at `index` of src
template <class Src>
SSA_DEV void dd_load(const Src src, size_t index, u64 w[Src::WORDS]) {
#pragma unroll
    for (int k = 0; k < Src::WORDS; k++) w[k] = src.word(index, k);
}
template <class Src>
SSA_DEV u64 dd_fingerprint_of(const u64 w[Src::WORDS], u64 k0, u64 k1) {
    return dd_fingerprint<Src::WORDS, Src::BYTES>(w, k0, k1);
}
// the key at `index` of src is the key w: the words decide, never the fingerprint (a word is only read while all the
// words in front of it agree)
template <class Src>
SSA_DEV bool dd_same_key(const Src src, size_t index, const u64 w[Src::WORDS]) {
    bool eq = true;
#pragma unroll
    for (int k = 0; k < Src::WORDS; k++) eq = eq && src.word(index, k) == w[k];
    return eq;
}

#ifndef SSA_NO_KERNELS
// The insert over a lane source (the body of ky_k_insert): one lane per lane of the slice.  stats[0] += lanes that hit the probe bound;
// blk_cnt[b] = representatives among the lanes of workgroup b
template <class Lanes>
SSA_DEV void dd_insert_body(const Lanes lanes, u32 n, u64 k0, u64 k1, u64 *__restrict__ slots, u32 mask, u32 bound,
                            u32 *__restrict__ rep, u32 *__restrict__ blk_cnt, unsigned long long *__restrict__ stats) {
    __shared__ u32 wave_cnt[DD_BLOCK / 64];
    const u32 i = blockIdx.x * DD_BLOCK + threadIdx.x;
    bool is_rep = false, over = false;
    if (i < n) {
        u64 w[Lanes::WORDS];
        dd_load(lanes, i, w);
        const u64 fp = dd_fingerprint_of<Lanes>(w, k0, k1);
        const u64 tag = fp >> 32, mine = (tag << 32) | (u64)i;
        u32 s = (u32)fp & mask, r = i;
        bool found = false;
#pragma unroll 1
        for (u32 p = 0; p < bound && !found; p++) {
            u64 cur = __hip_atomic_load(slots + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (cur == DD_EMPTY) {
                cur = atomicCAS((unsigned long long *)(slots + s), (unsigned long long)DD_EMPTY, (unsigned long long)mine);
                if (cur == DD_EMPTY) {
                    found = is_rep = true;
                    break;
                }
            }
            const u32 o = (u32)cur;
            if ((cur >> 32) == tag && o < n && dd_same_key(lanes, o, w)) {        // a candidate: the bytes decide
                r = o;
                found = true;
                break;
            }
            s = (s + 1u) & mask;
        }
        if (!found) over = is_rep = true;             // the probe bound: a key of its own
        rep[i] = r;
    }
    const unsigned long long reps = __ballot(is_rep), overs = __ballot(over);
    if ((threadIdx.x & 63u) == 0) {
        wave_cnt[threadIdx.x >> 6] = (u32)__popcll(reps);
        if (overs) atomicAdd(stats, (unsigned long long)__popcll(overs));
    }
    __syncthreads();
    if (threadIdx.x == 0) blk_cnt[blockIdx.x] = wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
}

// dd_k_insert keeps a body of its own: written over a lane source the compiler merges the aligned and the byte-wise
// load of a key word, and the kernel then runs slower where most lanes hold one key (profiles/r15).  It is the loop of
// dd_insert_body over the 12 words and the flag of an affine lane, the flag compared first.
// stats[0] += lanes that hit the probe bound; blk_cnt[b] = representatives among the lanes of workgroup b
__global__ void __launch_bounds__(256)
dd_k_insert(const u8 *__restrict__ pks, const u8 *__restrict__ pk_inf, u32 n, u64 k0, u64 k1, u64 *__restrict__ slots,
            u32 mask, u32 bound, u32 *__restrict__ rep, u32 *__restrict__ blk_cnt, unsigned long long *__restrict__ stats) {
    __shared__ u32 wave_cnt[DD_BLOCK / 64];
    const u32 i = blockIdx.x * DD_BLOCK + threadIdx.x;
    const bool aligned = ((size_t)pks & 7u) == 0;
    bool is_rep = false, over = false;
    if (i < n) {
        u64 w[12];
#pragma unroll
        for (int k = 0; k < 12; k++) w[k] = dd_key_word(pks, i, k, aligned);
        const u32 flag = dd_key_flag(pk_inf, i);
        const u64 fp = dd_fingerprint(w, flag, k0, k1);
        const u64 tag = fp >> 32, mine = (tag << 32) | (u64)i;
        u32 s = (u32)fp & mask, r = i;
        bool found = false;
#pragma unroll 1
        for (u32 p = 0; p < bound && !found; p++) {
            u64 cur = __hip_atomic_load(slots + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (cur == DD_EMPTY) {
                cur = atomicCAS((unsigned long long *)(slots + s), (unsigned long long)DD_EMPTY, (unsigned long long)mine);
                if (cur == DD_EMPTY) {
                    found = is_rep = true;
                    break;
                }
            }
            const u32 o = (u32)cur;
            if ((cur >> 32) == tag && o < n) {        // a candidate: the bytes decide
                bool eq = dd_key_flag(pk_inf, o) == flag;
#pragma unroll
                for (int k = 0; k < 12; k++) eq = eq && dd_key_word(pks, o, k, aligned) == w[k];
                if (eq) {
                    r = o;
                    found = true;
                    break;
                }
            }
            s = (s + 1u) & mask;
        }
        if (!found) over = is_rep = true;             // the probe bound: a key of its own
        rep[i] = r;
    }
    const unsigned long long reps = __ballot(is_rep), overs = __ballot(over);
    if ((threadIdx.x & 63u) == 0) {
        wave_cnt[threadIdx.x >> 6] = (u32)__popcll(reps);
        if (overs) atomicAdd(stats, (unsigned long long)__popcll(overs));
    }
    __syncthreads();
    if (threadIdx.x == 0) blk_cnt[blockIdx.x] = wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
}

// ONE workgroup: blk_off[b] = representatives in front of workgroup b's lanes; stats[1] = u
__global__ void __launch_bounds__(256)
dd_k_scan(const u32 *__restrict__ blk_cnt, u32 nb, u32 *__restrict__ blk_off, unsigned long long *__restrict__ stats) {
    __shared__ u32 part[DD_BLOCK];
    const u32 t = threadIdx.x, per = (nb + DD_BLOCK - 1) / DD_BLOCK;
    const u32 lo = t * per < nb ? t * per : nb, hi = lo + per < nb ? lo + per : nb;
    u32 sum = 0;
    for (u32 b = lo; b < hi; b++) sum += blk_cnt[b];
    part[t] = sum;
    __syncthreads();
    if (t == 0) {
        u32 acc = 0;
        for (u32 k = 0; k < DD_BLOCK; k++) {
            const u32 v = part[k];
            part[k] = acc;
            acc += v;
        }
        stats[1] = acc;
    }
    __syncthreads();
    u32 acc = part[t];
    for (u32 b = lo; b < hi; b++) {
        blk_off[b] = acc;
        acc += blk_cnt[b];
    }
}

// num[i] = the number of representative i (lane order), reps[num[i]] = i
__global__ void __launch_bounds__(256)
dd_k_number(const u32 *__restrict__ rep, u32 n, const u32 *__restrict__ blk_off, u32 *__restrict__ num,
            u32 *__restrict__ reps) {
    __shared__ u32 wave_cnt[DD_BLOCK / 64];
    const u32 i = blockIdx.x * DD_BLOCK + threadIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const bool is_rep = i < n && rep[i] == i;
    const unsigned long long m = __ballot(is_rep);
    if (lane == 0) wave_cnt[wave] = (u32)__popcll(m);
    __syncthreads();
    if (!is_rep) return;
    u32 idx = blk_off[blockIdx.x] + (u32)__popcll(m & ((1ull << lane) - 1ull));
    for (u32 k = 0; k < wave; k++) idx += wave_cnt[k];
    num[i] = idx;
    reps[idx] = i;
}

__global__ void __launch_bounds__(256)
dd_k_index(const u32 *__restrict__ rep, const u32 *__restrict__ num, u32 n, u32 *__restrict__ key_idx) {
    const u32 i = blockIdx.x * DD_BLOCK + threadIdx.x;
    if (i < n) key_idx[i] = num[rep[i]];
}

// thread t copies word t % 12 of representative t / 12's key; out_pks is the library's own (aligned) buffer
__global__ void __launch_bounds__(256)
dd_k_gather(const u8 *__restrict__ pks, const u8 *__restrict__ pk_inf, const u32 *__restrict__ reps, u32 u,
            u64 *__restrict__ out_pks, u8 *__restrict__ out_inf) {
    const size_t t = (size_t)blockIdx.x * DD_BLOCK + threadIdx.x;
    if (t >= (size_t)u * 12) return;
    const u32 j = (u32)(t / 12), k = (u32)(t % 12), i = reps[j];
    out_pks[t] = dd_key_word(pks, i, (int)k, ((size_t)pks & 7u) == 0);
    if (k == 0) out_inf[j] = (u8)dd_key_flag(pk_inf, i);
}
#endif  // SSA_NO_KERNELS

}  // namespace ssa
