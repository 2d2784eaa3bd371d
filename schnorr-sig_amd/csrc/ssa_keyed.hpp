// Internal: KeyedSignature wire records through a key cache in wire mode (ssa_verify_keyed_many_cached, DESIGN.md
// section 18).  A record is pk (49 compressed bytes) || signature (81 bytes); the identity of a key is its 49 bytes AS
// RECEIVED, so the square root of the decompression runs once per key, with [q]P and the table of sixteen multiples, and
// a warm call computes none.  A wire row of the cache holds what an affine row holds (ssa_keycache.hpp) and the 49
// bytes it was built from, as seven words: the six words of x and the flag byte.  A key that does not decode is a key
// like any other: its row holds the affine bytes (0, 0), which ssa_k_keyset_build reports as SSA_MALFORMED.
//
//   ky_k_split       the 81 signature bytes of every record into a dense array (what the verify kernels read at stride
//                    81).  One lane per output dword: the stores of a wave are one contiguous 256 bytes, its byte loads
//                    fall into the three or four records behind them.  Keys are never copied: they are read in place.
//   ky_k_insert      dd_k_insert on 49 bytes: the fingerprint is SipHash-2-4 under the context's key over the six x
//                    words and a last word of flag byte | 49 << 56.  It only picks candidates; the 49 bytes decide.
//   ky_k_lookup      kc_k_lookup against the stored 49 bytes of the rows (dd_k_scan and kc_k_number follow as they are).
//   ky_k_decompress  one lane per miss: decompress_lane into rows base .. base + m -- the 96 bytes, the flag and the 49
//                    bytes.  ssa_k_keyset_build then runs as it is over those rows.
//   ky_k_publish     kc_k_publish with the fingerprint of the row's 49 bytes, launched after the build.
//   ky_k_expand      each lane's 96 key bytes and flag out of its row into a per-lane workspace: a gather, no arithmetic
//                    (one lane per word, so a wave stores 512 contiguous bytes and loads five or six whole keys).  It is
//                    what the MSM preparation and the challenge hash read as the batch's keys.
//
// Memory model: that of ssa_keycache.hpp.  Workgroups of one launch exchange only slot words, through agent-scope
// atomics (ky_k_insert on the slice's table, ky_k_publish on the cache's); everything else is written with ordinary
// vector stores and read by a later launch on the same stream.
#pragma once
#include "ssa_keycache.hpp"

namespace ssa {

constexpr int KY_WIRE_WORDS = 7;      // a row's 49 bytes: six words of x, one word holding the flag byte

// word k < 6 of x, or (k == 6) the flag byte, of record i (records are 130 bytes apart: never aligned)
SSA_DEV u64 ky_wire_word(const u8 *__restrict__ keyed, size_t i, int k) {
    const u8 *p = keyed + 130 * i;
    return k < 6 ? ld_u64_le(p + 8 * k) : (u64)p[48];
}

// SipHash-2-4 of the 49 bytes: six words and the flag byte with the length in the top byte of the last word
SSA_DEV u64 ky_fingerprint(const u64 w[KY_WIRE_WORDS], u64 k0, u64 k1) {
    u64 v0 = k0 ^ 0x736f6d6570736575ull, v1 = k1 ^ 0x646f72616e646f6dull, v2 = k0 ^ 0x6c7967656e657261ull,
        v3 = k1 ^ 0x7465646279746573ull;
#pragma unroll
    for (int k = 0; k < KY_WIRE_WORDS; k++) {
        const u64 m = k < 6 ? w[k] : (w[6] | (49ull << 56));
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

#ifndef SSA_NO_KERNELS
// sigs_out (the library's own buffer: dword-aligned) = the 81 signature bytes of records [0, n), side by side
__global__ void __launch_bounds__(256)
ky_k_split(const u8 *__restrict__ keyed, size_t n, u8 *__restrict__ sigs_out) {
    const size_t d = (size_t)blockIdx.x * 256 + threadIdx.x, total = n * 81, o = 4 * d;
    if (o >= total) return;
    u32 v = 0;
    const int cnt = total - o < 4 ? (int)(total - o) : 4;
    for (int k = 0; k < cnt; k++) {
        const size_t b = o + k, i = b / 81;
        v |= (u32)keyed[130 * i + 49 + (b - 81 * i)] << (8 * k);
    }
    if (cnt == 4) {
        reinterpret_cast<u32 *>(sigs_out)[d] = v;
    } else {
        for (int k = 0; k < cnt; k++) sigs_out[o + k] = (u8)(v >> (8 * k));
    }
}

// dd_k_insert over the 49 key bytes of n records: stats[0] += lanes that hit the probe bound; blk_cnt[b] =
// representatives among the lanes of workgroup b
__global__ void __launch_bounds__(256)
ky_k_insert(const u8 *__restrict__ keyed, u32 n, u64 k0, u64 k1, u64 *__restrict__ slots, u32 mask, u32 bound,
            u32 *__restrict__ rep, u32 *__restrict__ blk_cnt, unsigned long long *__restrict__ stats) {
    __shared__ u32 wave_cnt[DD_BLOCK / 64];
    const u32 i = blockIdx.x * DD_BLOCK + threadIdx.x;
    bool is_rep = false, over = false;
    if (i < n) {
        u64 w[KY_WIRE_WORDS];
#pragma unroll
        for (int k = 0; k < KY_WIRE_WORDS; k++) w[k] = ky_wire_word(keyed, i, k);
        const u64 fp = ky_fingerprint(w, k0, k1);
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
                bool eq = true;
#pragma unroll
                for (int k = 0; k < KY_WIRE_WORDS; k++) eq = eq && ky_wire_word(keyed, o, k) == w[k];
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

// kc_k_lookup for a wire cache: c_wire = the rows' seven words; stats[1] = u; n = the lanes of the slice
__global__ void __launch_bounds__(256)
ky_k_lookup(const u8 *__restrict__ keyed, const u32 *__restrict__ reps, u32 n, const unsigned long long *__restrict__ stats,
            u64 k0, u64 k1, const u64 *__restrict__ slots, u32 mask, u32 bound, const u64 *__restrict__ c_wire, u32 held,
            u32 *__restrict__ found, u32 *__restrict__ blk_cnt, u32 *__restrict__ stamps, u32 epoch) {
    __shared__ u32 wave_cnt[DD_BLOCK / 64];
    const u32 j = blockIdx.x * DD_BLOCK + threadIdx.x;
    const u32 u = (u32)stats[1];
    bool miss = false;
    if (j < u && j < n) {
        const u32 i = reps[j];
        u64 w[KY_WIRE_WORDS];
#pragma unroll
        for (int k = 0; k < KY_WIRE_WORDS; k++) w[k] = i < n ? ky_wire_word(keyed, i, k) : 0;
        const u64 fp = ky_fingerprint(w, k0, k1);
        const u64 tag = fp >> 32;
        u32 s = (u32)fp & mask, row = KC_MISS;
#pragma unroll 1
        for (u32 p = 0; p < bound; p++) {
            const u64 cur = __hip_atomic_load(slots + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (cur == DD_EMPTY) break;
            const u32 r = (u32)cur;
            if ((cur >> 32) == tag && r < held) {         // a candidate: the bytes decide
                bool eq = true;
#pragma unroll
                for (int k = 0; k < KY_WIRE_WORDS; k++) eq = eq && c_wire[(size_t)r * KY_WIRE_WORDS + k] == w[k];
                if (eq) {
                    row = r;
                    break;
                }
            }
            s = (s + 1u) & mask;
        }
        found[j] = row;
        miss = row == KC_MISS;
        if (stamps && !miss) stamps[row] = epoch;     // (SSA_KEYCACHE_EVICT_RECENT: the row's last use)
    }
    const unsigned long long misses = __ballot(miss);
    if ((threadIdx.x & 63u) == 0) wave_cnt[threadIdx.x >> 6] = (u32)__popcll(misses);
    __syncthreads();
    if (threadIdx.x == 0) blk_cnt[blockIdx.x] = wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
}

// the keys of lanes reps[0, m) decompressed into rows [0, m) of out_pks / out_inf (the caller offsets them to the rows
// it fills); out_wire (or nullptr: the context's own workspaces, which keep no wire bytes) gets the 49 bytes.  A key
// that does not decode leaves (0, 0) and no flag.
__global__ void __launch_bounds__(256)
ky_k_decompress(const u8 *__restrict__ keyed, const u32 *__restrict__ reps, u32 m, u32 n, u64 *__restrict__ out_pks,
                u8 *__restrict__ out_inf, u64 *__restrict__ out_wire) {
    const u32 t = blockIdx.x * 256 + threadIdx.x;
    if (t >= m) return;
    const u32 i = reps[t];
    if (i >= n) return;       // (never: a representative is a lane of the slice)
    const u8 *rec = keyed + 130 * (size_t)i;
    aff p;
    bool inf;
    (void)decompress_lane(rec, p, inf);
#pragma unroll
    for (int k = 0; k < 6; k++) {
        out_pks[12 * (size_t)t + k] = p.x.c[k];
        out_pks[12 * (size_t)t + 6 + k] = p.y.c[k];
    }
    out_inf[t] = inf ? 1 : 0;
    if (out_wire) {
#pragma unroll
        for (int k = 0; k < KY_WIRE_WORDS; k++) out_wire[(size_t)t * KY_WIRE_WORDS + k] = ky_wire_word(keyed, i, k);
    }
}

// kc_k_publish for wire rows base .. base + m (complete: an earlier launch built them)
__global__ void __launch_bounds__(256)
ky_k_publish(const u64 *__restrict__ c_wire, u32 base, u32 m, u64 k0, u64 k1, u64 *__restrict__ slots, u32 mask,
             u32 bound, unsigned long long *__restrict__ unpublished) {
    const u32 t = blockIdx.x * DD_BLOCK + threadIdx.x;
    bool lost = false;
    if (t < m) {
        const u32 r = base + t;
        u64 w[KY_WIRE_WORDS];
#pragma unroll
        for (int k = 0; k < KY_WIRE_WORDS; k++) w[k] = c_wire[(size_t)r * KY_WIRE_WORDS + k];
        const u64 fp = ky_fingerprint(w, k0, k1);
        const u64 mine = ((fp >> 32) << 32) | (u64)r;
        u32 s = (u32)fp & mask;
        lost = true;
#pragma unroll 1
        for (u32 p = 0; p < bound; p++) {
            u64 cur = __hip_atomic_load(slots + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (cur == DD_EMPTY) {
                cur = atomicCAS((unsigned long long *)(slots + s), (unsigned long long)DD_EMPTY, (unsigned long long)mine);
                if (cur == DD_EMPTY) {
                    lost = false;
                    break;
                }
            }
            s = (s + 1u) & mask;
        }
    }
    const unsigned long long losts = __ballot(lost);
    if ((threadIdx.x & 63u) == 0 && losts) atomicAdd(unpublished, (unsigned long long)__popcll(losts));
}

// thread t copies word t % 12 of the key of lane t / 12 (row lane_row[lane] < n_rows of row_pks / row_inf)
__global__ void __launch_bounds__(256)
ky_k_expand(const u32 *__restrict__ lane_row, const u64 *__restrict__ row_pks, const u8 *__restrict__ row_inf, u32 n_rows,
            u32 n, u64 *__restrict__ out_pks, u8 *__restrict__ out_inf) {
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (size_t)n * 12) return;
    const u32 i = (u32)(t / 12), k = (u32)(t % 12), r = lane_row[i];
    const bool in = r < n_rows;       // (always)
    out_pks[t] = in ? row_pks[(size_t)r * 12 + k] : 0;
    if (k == 0) out_inf[i] = in && row_inf[r] ? 1 : 0;
}
#endif  // SSA_NO_KERNELS

}  // namespace ssa
