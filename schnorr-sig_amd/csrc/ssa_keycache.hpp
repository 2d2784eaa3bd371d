// Internal: the device key cache (ssa_verify_many_cached).  A key cache is a ladder-kind key set
// that fills itself: rows of checked keys (the 96 key bytes, the pk_inf boolean, the status byte, the table of sixteen
// multiples) and an open-addressing table of 64-bit slot words over them (fingerprint's upper half << 32 | cache row;
// all ones = empty; at least four slots per row; linear probing; the context's probe bound).  The fingerprint is
// dd_fingerprint (ssa_dedup.hpp) under the context's key, and as there it only picks slots: a slot with a matching
// upper half is a CANDIDATE and the 97 bytes stored in the row decide.  Equality is never decided on the fingerprint.
//
//   kc_k_lookup   one lane per DISTINCT key of the slice (u is read from the device: the launch is queued behind
//                 dd_k_index and in front of the read-back of dedup_slice).  found[j] = the cache row of key j, or
//                 KC_MISS; blk_cnt[b] = misses among the keys of workgroup b.  An empty slot ends a probe chain (the
//                 cache never deletes an entry: eviction is a clear of the whole table); the probe bound ends it too.
//   dd_k_scan     (as it is) the per-workgroup offsets and m, the number of misses.
//   kc_k_number   miss t of the slice, in key order: found[j] = KC_MISS_BIT | t, miss_rep[t] = the key's representative
//                 lane (what dd_k_gather reads: it copies the misses' bytes into cache rows held .. held + m).
//   kc_k_publish  after ssa_k_keyset_build has filled rows base .. base + m: one lane per new row claims the first empty
//                 slot of the row's probe sequence by compare-and-swap.  A row that finds none within the probe bound
//                 stays unpublished: used by this call, not found by the next (counted).
//   kc_k_map      a cache row per lane from dd_idx and found[] (what ssa_k_verify_keyed and msm_k_screen_keymask index
//                 the cache's tables and statuses with).
//
// Memory model (the rules of ssa_dedup.hpp): workgroups of ONE launch exchange nothing but slot words, and those only
// through agent-scope atomics (kc_k_publish is the only writer; a compare-and-swap decides every claim and the load in
// front of it only saves the swap when the slot is taken).  A slot changes once between clears, from empty to owned.
// Everything written with ordinary stores (key bytes, flags, statuses, tables, found[], the row map) is read by a LATER
// launch on the same stream: kc_k_publish is launched after the build, so a row is complete before any later launch
// can find it.  All device writes are vector stores and vector atomics.
#pragma once
#include "ssa_dedup.hpp"

namespace ssa {

constexpr u32 KC_MISS = 0xffffffffu, KC_MISS_BIT = 0x80000000u;
constexpr size_t KC_MAX_CAPACITY = (size_t)1 << 24;

// what the host does with a slice of u distinct keys of which m missed, in a cache of `capacity` rows holding `held`
enum : int { KC_PLAN_INSERT = 0, KC_PLAN_CLEAR = 1, KC_PLAN_BYPASS = 2 };
__host__ inline int kc_plan(uint64_t capacity, uint64_t held, uint64_t u, uint64_t m) {
    if (held + m <= capacity) return KC_PLAN_INSERT;
    return u <= capacity ? KC_PLAN_CLEAR : KC_PLAN_BYPASS;
}

#ifndef SSA_NO_KERNELS
// the 12 key words and the flag of cache row r
SSA_DEV u64 kc_row_fingerprint(const u64 *__restrict__ c_pks, const u8 *__restrict__ c_inf, u32 r, u64 k0, u64 k1) {
    u64 w[12];
#pragma unroll
    for (int k = 0; k < 12; k++) w[k] = c_pks[(size_t)r * 12 + k];
    return dd_fingerprint(w, c_inf[r] ? 1u : 0u, k0, k1);
}

// stats[1] = u (dd_k_scan's); n = the lanes of the slice (the grid covers them: u <= n)
__global__ void __launch_bounds__(256)
kc_k_lookup(const u8 *__restrict__ pks, const u8 *__restrict__ pk_inf, const u32 *__restrict__ reps, u32 n,
            const unsigned long long *__restrict__ stats, u64 k0, u64 k1, const u64 *__restrict__ slots, u32 mask,
            u32 bound, const u64 *__restrict__ c_pks, const u8 *__restrict__ c_inf, u32 held, u32 *__restrict__ found,
            u32 *__restrict__ blk_cnt) {
    __shared__ u32 wave_cnt[DD_BLOCK / 64];
    const u32 j = blockIdx.x * DD_BLOCK + threadIdx.x;
    const u32 u = (u32)stats[1];
    bool miss = false;
    if (j < u && j < n) {
        const u32 i = reps[j];
        const bool aligned = ((size_t)pks & 7u) == 0;
        u64 w[12];
#pragma unroll
        for (int k = 0; k < 12; k++) w[k] = dd_key_word(pks, i, k, aligned);
        const u32 flag = dd_key_flag(pk_inf, i);
        const u64 fp = dd_fingerprint(w, flag, k0, k1);
        const u64 tag = fp >> 32;
        u32 s = (u32)fp & mask, row = KC_MISS;
#pragma unroll 1
        for (u32 p = 0; p < bound; p++) {
            const u64 cur = __hip_atomic_load(slots + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (cur == DD_EMPTY) break;
            const u32 r = (u32)cur;
            if ((cur >> 32) == tag && r < held) {         // a candidate: the bytes decide
                bool eq = (c_inf[r] ? 1u : 0u) == flag;
#pragma unroll
                for (int k = 0; k < 12; k++) eq = eq && c_pks[(size_t)r * 12 + k] == w[k];
                if (eq) {
                    row = r;
                    break;
                }
            }
            s = (s + 1u) & mask;
        }
        found[j] = row;
        miss = row == KC_MISS;
    }
    const unsigned long long misses = __ballot(miss);
    if ((threadIdx.x & 63u) == 0) wave_cnt[threadIdx.x >> 6] = (u32)__popcll(misses);
    __syncthreads();
    if (threadIdx.x == 0) blk_cnt[blockIdx.x] = wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
}

__global__ void __launch_bounds__(256)
kc_k_number(const u32 *__restrict__ reps, u32 n, const unsigned long long *__restrict__ stats,
            const u32 *__restrict__ blk_off, u32 *__restrict__ found, u32 *__restrict__ miss_rep) {
    __shared__ u32 wave_cnt[DD_BLOCK / 64];
    const u32 j = blockIdx.x * DD_BLOCK + threadIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const u32 u = (u32)stats[1];
    const bool miss = j < u && j < n && found[j] == KC_MISS;
    const unsigned long long m = __ballot(miss);
    if (lane == 0) wave_cnt[wave] = (u32)__popcll(m);
    __syncthreads();
    if (!miss) return;
    u32 t = blk_off[blockIdx.x] + (u32)__popcll(m & ((1ull << lane) - 1ull));
    for (u32 k = 0; k < wave; k++) t += wave_cnt[k];
    found[j] = KC_MISS_BIT | t;
    miss_rep[t] = reps[j];
}

// rows base .. base + m are complete (an earlier launch built them): claim a slot for each; *unpublished += rows that
// found no empty slot within the probe bound
__global__ void __launch_bounds__(256)
kc_k_publish(const u64 *__restrict__ c_pks, const u8 *__restrict__ c_inf, u32 base, u32 m, u64 k0, u64 k1,
             u64 *__restrict__ slots, u32 mask, u32 bound, unsigned long long *__restrict__ unpublished) {
    const u32 t = blockIdx.x * DD_BLOCK + threadIdx.x;
    bool lost = false;
    if (t < m) {
        const u32 r = base + t;
        const u64 fp = kc_row_fingerprint(c_pks, c_inf, r, k0, k1);
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

// lane_row[i] = the cache row of lane i's key: a hit's row, base + t for miss t; all_new (the cache was cleared for this
// slice): key j took row j
__global__ void __launch_bounds__(256)
kc_k_map(const u32 *__restrict__ key_idx, const u32 *__restrict__ found, u32 n, u32 base, u32 all_new,
         u32 *__restrict__ lane_row) {
    const u32 i = blockIdx.x * DD_BLOCK + threadIdx.x;
    if (i >= n) return;
    const u32 j = key_idx[i];
    if (all_new) {
        lane_row[i] = j;
        return;
    }
    const u32 f = found[j];
    lane_row[i] = (f & KC_MISS_BIT) ? base + (f & ~KC_MISS_BIT) : f;
}
#endif  // SSA_NO_KERNELS

}  // namespace ssa
