// Internal: the device key cache (ssa_verify_many_cached).  A key cache is a ladder-kind key set
// that fills itself: rows of checked keys (the 96 key bytes, the pk_inf boolean, the status byte, the table of sixteen
// multiples; in wire mode also the 49 bytes the row was built from, ssa_keyed.hpp) and an open-addressing table of
// 64-bit slot words over them (fingerprint's upper half << 32 | cache row; all ones = empty; at least four slots per
// row; linear probing; the context's probe bound).  What identifies a key, its fingerprint and the rule that the words
// stored in the row decide, never the fingerprint, are those of ssa_dedup.hpp.  The publishing loop is written once
// over a row source (kc_publish_body); the look-up loop over a lane source and a row source (kc_lookup_body) serves the
// wire cache, and kc_k_lookup keeps the same loop written out for affine lanes (see there).
//
//   kc_k_lookup   (and kc_lookup_body, the body of ky_k_lookup)  one lane per DISTINCT key of the slice (u is
//                 read from the device: the launch is queued behind dd_k_index and in front of the read-back of
//                 dedup_slice).  found[j] = the cache row of key j, or KC_MISS; blk_cnt[b] = misses among the keys of
//                 workgroup b.  An empty slot ends a probe chain (the cache never deletes an entry: eviction empties
//                 the whole table); the probe bound ends it too.  It writes no slot.
//   dd_k_scan     (as it is) the per-workgroup offsets and m, the number of misses.
//   kc_k_number   miss t of the slice, in key order: found[j] = KC_MISS_BIT | t, miss_rep[t] = the key's representative
//                 lane (whose key goes into cache row held + t).
//   kc_publish_body  (the body of kc_k_publish and ky_k_publish)  after ssa_k_keyset_build has filled rows base .. base +
//                 m: one lane per new row claims the first empty slot of the row's probe sequence by compare-and-swap.
//                 A row that finds none within the probe bound stays unpublished: used by this call, not found by the
//                 next (counted).
//   kc_k_map      a cache row per lane from dd_idx and found[] (what ssa_k_verify_keyed and msm_k_screen_keymask index
//                 the cache's tables and statuses with).
//
// Memory model (the rules of ssa_dedup.hpp): workgroups of ONE launch exchange nothing but slot words, and those only
// through agent-scope atomics (the publishing kernels are the only writers; a compare-and-swap decides every claim and
// the load in front of it only saves the swap when the slot is taken).  A slot changes once between clears, from empty
// to owned.  Everything written with ordinary stores (key bytes, flags, wire words, statuses, tables, found[], the row
// map) is read by a LATER launch on the same stream: the publishing kernel is launched after the build, so a row is
// complete before any later launch can find it.  All device writes are vector stores and vector atomics.
//
// Eviction.  A cache keeps the clear-only policy above until ssa_keycache_set_eviction makes it
// SSA_KEYCACHE_EVICT_RECENT.  Then every row has a 32-bit stamp, the cache's epoch (one per slice that looks keys up) at
// its last use: the look-up kernels store it on a hit (one lane per distinct key, so one writer per row; a plain store,
// read by a later launch), inserted rows get the current epoch.  Where the clear-only policy clears, the cache COMPACTS:
//   kc_k_age_hist      rows of each age (epoch - stamp, 0..62, 63 = older) over rows [0, held): counts per workgroup
//                      in LDS, then vector atomics on 64 words the call has zeroed.  The host reads them and kc_keep
//                      picks the largest age a* whose rows fit the budget: K rows survive.
//   kc_k_evict_count   per workgroup: non-survivors below row K (holes), survivors at rows >= K (movers).  There are
//                      equally many of each.  dd_k_scan (as it is, twice) turns the counts into offsets.
//   kc_k_evict_assign  hole t and mover t, in row order, into two lists; remap[r] = r for a survivor below K, KC_MISS
//                      for every dropped row.
//   kc_k_evict_move    one wave per mover: the whole row (4 KB table at 16 bytes per lane per load, key words, pk_inf,
//                      status, stamp, wire words) from mover t to hole t, and remap[mover] = hole.  Rows read are all
//                      >= K, rows written all < K and no survivor: the two sets are disjoint, so one launch moves every
//                      row with no order between workgroups.
//   kc_k_remap         the slice's found[] through remap[] (its hits have age 0: they always survive).
// The slot words are then emptied and rows [0, K) published again by kc_k_publish / ky_k_publish, still the only
// writers of slot words.  Everything else is ordinary vector stores read by a later launch.
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

// Which rows a compaction keeps: hist[a] = rows of age a (a < 63; hist[63] = all older rows, never kept), u distinct keys
// in the slice of which m missed, m <= u <= capacity.  budget = max(u - m, (capacity - m) / 2); *age_out = the largest a
// in 0..62 with hist[0] + .. + hist[a] <= budget, *kept_out = that sum.  The rows the slice hit have age 0 and there
// are at most u - m of them, so an age exists; false only when hist[0] says otherwise (stamps that alias after 2^32
// slices: the caller then clears).  kept + m <= capacity, and at most half of the room left beside the misses is kept,
// so the next compaction is at least (capacity - m) / 2 insertions away.
constexpr int KC_AGE_BINS = 64;
__host__ inline bool kc_keep(uint64_t capacity, uint64_t u, uint64_t m, const uint64_t hist[KC_AGE_BINS], uint64_t *age_out,
                             uint64_t *kept_out) {
    const uint64_t half = (capacity - m) / 2, budget = u - m > half ? u - m : half;
    uint64_t sum = 0;
    bool any = false;
    for (int a = 0; a < KC_AGE_BINS - 1; a++) {
        if (hist[a] > budget - sum) break;
        sum += hist[a];
        *age_out = (uint64_t)a;
        *kept_out = sum;
        any = true;
    }
    return any;
}

#ifndef SSA_NO_KERNELS
// The look-up over a lane source and a row source (the body of ky_k_lookup): one lane per distinct key of the slice.  stats[1] = u (dd_k_scan's); n = the
// lanes of the slice (the grid covers them: u <= n); stamps (or nullptr): the rows' stamps, which get `epoch` on a hit
template <class Lanes, class Rows>
SSA_DEV void kc_lookup_body(const Lanes lanes, const Rows rows, const u32 *__restrict__ reps, u32 n,
                            const unsigned long long *__restrict__ stats, u64 k0, u64 k1, const u64 *__restrict__ slots,
                            u32 mask, u32 bound, u32 held, u32 *__restrict__ found, u32 *__restrict__ blk_cnt,
                            u32 *__restrict__ stamps, u32 epoch) {
    static_assert(Lanes::WORDS == Rows::WORDS && Lanes::BYTES == Rows::BYTES, "lanes and rows of one kind of key");
    __shared__ u32 wave_cnt[DD_BLOCK / 64];
    const u32 j = blockIdx.x * DD_BLOCK + threadIdx.x;
    const u32 u = (u32)stats[1];
    bool miss = false;
    if (j < u && j < n) {
        const u32 i = reps[j];
        u64 w[Lanes::WORDS] = {};
        if (i < n) dd_load(lanes, i, w);                  // (always: a representative is a lane of the slice)
        const u64 fp = dd_fingerprint_of<Lanes>(w, k0, k1);
        const u64 tag = fp >> 32;
        u32 s = (u32)fp & mask, row = KC_MISS;
#pragma unroll 1
        for (u32 p = 0; p < bound; p++) {
            const u64 cur = __hip_atomic_load(slots + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (cur == DD_EMPTY) break;
            const u32 r = (u32)cur;
            if ((cur >> 32) == tag && r < held && dd_same_key(rows, r, w)) {      // a candidate: the bytes decide
                row = r;
                break;
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

// kc_k_lookup keeps a body of its own, for the reason given at dd_k_insert (ssa_dedup.hpp): the loop of kc_lookup_body
// over an affine lane and the 12 words and the flag of an affine row, the flag compared first.
// stats[1] = u (dd_k_scan's); n = the lanes of the slice (the grid covers them: u <= n); stamps (or nullptr): the rows'
// stamps, which get `epoch` on a hit
__global__ void __launch_bounds__(256)
kc_k_lookup(const u8 *__restrict__ pks, const u8 *__restrict__ pk_inf, const u32 *__restrict__ reps, u32 n,
            const unsigned long long *__restrict__ stats, u64 k0, u64 k1, const u64 *__restrict__ slots, u32 mask,
            u32 bound, const u64 *__restrict__ c_pks, const u8 *__restrict__ c_inf, u32 held, u32 *__restrict__ found,
            u32 *__restrict__ blk_cnt, u32 *__restrict__ stamps, u32 epoch) {
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
        if (stamps && !miss) stamps[row] = epoch;     // (SSA_KEYCACHE_EVICT_RECENT: the row's last use)
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

// The body of kc_k_publish / ky_k_publish, the only writers of slot words: rows base .. base + m are complete (an
// earlier launch built them): claim a slot for each; *unpublished += rows that found no empty slot within the probe bound
template <class Rows>
SSA_DEV void kc_publish_body(const Rows rows, u32 base, u32 m, u64 k0, u64 k1, u64 *__restrict__ slots, u32 mask,
                             u32 bound, unsigned long long *__restrict__ unpublished) {
    const u32 t = blockIdx.x * DD_BLOCK + threadIdx.x;
    bool lost = false;
    if (t < m) {
        const u32 r = base + t;
        u64 w[Rows::WORDS];
        dd_load(rows, r, w);
        const u64 fp = dd_fingerprint_of<Rows>(w, k0, k1);
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

__global__ void __launch_bounds__(256)
kc_k_publish(const u64 *__restrict__ c_pks, const u8 *__restrict__ c_inf, u32 base, u32 m, u64 k0, u64 k1,
             u64 *__restrict__ slots, u32 mask, u32 bound, unsigned long long *__restrict__ unpublished) {
    kc_publish_body(DdAffineRows{c_pks, c_inf}, base, m, k0, k1, slots, mask, bound, unpublished);
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
// ---- compaction (SSA_KEYCACHE_EVICT_RECENT): see the head of this file

// hist[a] += rows of [0, held) whose age is a (63: any older); hist is zeroed by the caller on the same stream
__global__ void __launch_bounds__(256)
kc_k_age_hist(const u32 *__restrict__ stamps, u32 held, u32 epoch, u32 *__restrict__ hist) {
    __shared__ u32 h[KC_AGE_BINS];
    if (threadIdx.x < KC_AGE_BINS) h[threadIdx.x] = 0;
    __syncthreads();
    const u32 r = blockIdx.x * DD_BLOCK + threadIdx.x;
    if (r < held) {
        const u32 age = epoch - stamps[r];
        atomicAdd(&h[age < KC_AGE_BINS - 1 ? age : KC_AGE_BINS - 1], 1u);
    }
    __syncthreads();
    if (threadIdx.x < KC_AGE_BINS && h[threadIdx.x]) atomicAdd(hist + threadIdx.x, h[threadIdx.x]);
}

// row r < held survives a compaction that keeps the ages 0..max_age
SSA_DEV bool kc_survives(const u32 *__restrict__ stamps, u32 r, u32 epoch, u32 max_age) { return epoch - stamps[r] <= max_age; }

// hole_cnt[b] = rows of workgroup b below `kept` that do not survive; mover_cnt[b] = its rows at or above `kept` that do
__global__ void __launch_bounds__(256)
kc_k_evict_count(const u32 *__restrict__ stamps, u32 held, u32 epoch, u32 max_age, u32 kept, u32 *__restrict__ hole_cnt,
                 u32 *__restrict__ mover_cnt) {
    __shared__ u32 wave_cnt[2][DD_BLOCK / 64];
    const u32 r = blockIdx.x * DD_BLOCK + threadIdx.x;
    const bool surv = r < held && kc_survives(stamps, r, epoch, max_age);
    const unsigned long long holes = __ballot(r < kept && r < held && !surv), movers = __ballot(r >= kept && surv);
    if ((threadIdx.x & 63u) == 0) {
        wave_cnt[0][threadIdx.x >> 6] = (u32)__popcll(holes);
        wave_cnt[1][threadIdx.x >> 6] = (u32)__popcll(movers);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        hole_cnt[blockIdx.x] = wave_cnt[0][0] + wave_cnt[0][1] + wave_cnt[0][2] + wave_cnt[0][3];
        mover_cnt[blockIdx.x] = wave_cnt[1][0] + wave_cnt[1][1] + wave_cnt[1][2] + wave_cnt[1][3];
    }
}

// holes[t] = the t-th hole, movers[t] = the t-th mover, in row order (cap = the length of both lists); remap[r] for every
// row that is no mover: itself for a survivor below `kept`, KC_MISS for a dropped row
__global__ void __launch_bounds__(256)
kc_k_evict_assign(const u32 *__restrict__ stamps, u32 held, u32 epoch, u32 max_age, u32 kept,
                  const u32 *__restrict__ hole_off, const u32 *__restrict__ mover_off, u32 cap, u32 *__restrict__ holes,
                  u32 *__restrict__ movers, u32 *__restrict__ remap) {
    __shared__ u32 wave_cnt[2][DD_BLOCK / 64];
    const u32 r = blockIdx.x * DD_BLOCK + threadIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const bool in = r < held, surv = in && kc_survives(stamps, r, epoch, max_age);
    const bool hole = in && r < kept && !surv, mover = r >= kept && surv;
    const unsigned long long hm = __ballot(hole), mm = __ballot(mover);
    if (lane == 0) {
        wave_cnt[0][wave] = (u32)__popcll(hm);
        wave_cnt[1][wave] = (u32)__popcll(mm);
    }
    __syncthreads();
    if (!in) return;
    if (hole || mover) {
        const int w = hole ? 0 : 1;
        u32 t = (hole ? hole_off : mover_off)[blockIdx.x] + (u32)__popcll((hole ? hm : mm) & ((1ull << lane) - 1ull));
        for (u32 k = 0; k < wave; k++) t += wave_cnt[w][k];
        if (t < cap) (hole ? holes : movers)[t] = r;
    }
    if (!mover) remap[r] = surv ? r : KC_MISS;
}

// one wave per mover t < n_move: row movers[t] (>= kept) into row holes[t] (< kept), whole; remap[movers[t]] = holes[t].
// tab_words = the u64 words of a row's table (even: the table moves as 16-byte words); wire_words = the words of a wire
// row (at most 16; 0 for an affine cache, whose c_wire is not read)
__global__ void __launch_bounds__(256)
kc_k_evict_move(const u32 *__restrict__ movers, const u32 *__restrict__ holes, u32 n_move, u32 held, u32 kept,
                u32 tab_words, u64 *__restrict__ c_tab, u64 *__restrict__ c_pks, u8 *__restrict__ c_inf,
                u8 *__restrict__ c_status, u32 *__restrict__ stamps, u64 *__restrict__ c_wire, u32 wire_words, u32 *__restrict__ remap) {
    const u32 t = blockIdx.x * (DD_BLOCK / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (t >= n_move) return;
    const u32 src = movers[t], dst = holes[t];
    if (src >= held || src < kept || dst >= kept) return;      // (never)
    const uint4 *from = reinterpret_cast<const uint4 *>(c_tab + (size_t)src * tab_words);
    uint4 *to = reinterpret_cast<uint4 *>(c_tab + (size_t)dst * tab_words);
    for (u32 k = lane; k < tab_words / 2; k += 64) to[k] = from[k];
    if (lane < 12) c_pks[(size_t)dst * 12 + lane] = c_pks[(size_t)src * 12 + lane];
    if (lane >= 16 && lane - 16 < wire_words)
        c_wire[(size_t)dst * wire_words + (lane - 16)] = c_wire[(size_t)src * wire_words + (lane - 16)];
    if (lane == 32) c_inf[dst] = c_inf[src];
    if (lane == 33) c_status[dst] = c_status[src];
    if (lane == 34) stamps[dst] = stamps[src];
    if (lane == 35) remap[src] = dst;
}

// found[j] of the slice's u distinct keys through remap[]: a hit's row after the compaction (misses keep their numbers)
__global__ void __launch_bounds__(256)
kc_k_remap(u32 *__restrict__ found, u32 u, const u32 *__restrict__ remap, u32 held) {
    const u32 j = blockIdx.x * DD_BLOCK + threadIdx.x;
    if (j >= u) return;
    const u32 f = found[j];
    if (!(f & KC_MISS_BIT) && f < held) found[j] = remap[f];
}
#endif  // SSA_NO_KERNELS

}  // namespace ssa
