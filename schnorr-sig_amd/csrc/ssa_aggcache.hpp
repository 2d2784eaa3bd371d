// Internal: half-aggregates verified through a key cache (ssa_verify_aggregates_many_cached).
// The cache of sections 16, 18 and 19 answers per LANE and per SLICE (a row number that the next slice may clear or
// compact away); the aggregate verifier of section 21 wants the keys of all N lanes at once and answers per AGGREGATE.
// Two kernels stand between the two:
//
//   agc_k_expand        behind each slice of the cache, before the next one starts: what the aggregate stages need of a
//                       lane's row, written where it outlives the slice -- the key's status byte into kst[lane], and
//                       for wire keys the 96 key bytes and the flag.  The key gather is ky_k_expand's: one thread per
//                       8-byte word, so a wave stores 512 contiguous bytes and loads five or six whole rows; the thread
//                       of a lane's word 0 also moves its two bytes.  Without keys to move (affine keys: the caller's
//                       arrays are the keys) it is one thread per lane.  Thread 0 adds the slice's count of
//                       unpublished rows to the call's, since the next slice zeroes that word.
//   agc_k_key_verdicts  behind agm_run: verdicts[j] = SSA_INVALID_PUBLIC_KEY for every aggregate j that holds a lane
//                       with that key status; every other verdict word is left as the aggregate stages wrote it.
//
// Memory model: no two workgroups of a launch touch the same byte but the one counter of agc_k_key_verdicts, an
// agent-scope atomic add; everything is written with ordinary vector stores and read by a later launch on the same stream.
#pragma once
#include "ssa_keyed.hpp"

namespace ssa {

constexpr u32 AGC_BLOCK = 256, AGC_WAVES = AGC_BLOCK / 64;
constexpr u32 AGC_WAVE_MAX = 4096;      // lanes up to which ONE wave folds an aggregate (four 16-byte loads per lane)
constexpr u32 AGC_BAD_KEY = 1;          // SSA_INVALID_PUBLIC_KEY as ssa_k_keyset_build stores it
// the call's two counters (ctx->agc_cnt): aggregates answered SSA_INVALID_PUBLIC_KEY, rows that could not be published
enum : int { AGC_CNT_BAD = 0, AGC_CNT_UNPUB = 1, AGC_CNT_WORDS = 2 };

#ifndef SSA_NO_KERNELS
// lanes [0, n) of a slice: lane_row[i] < n_rows is lane i's row of row_status / row_pks / row_inf (rows of the cache, or
// under a bypass of the context's own workspaces).  out_pks == nullptr: the status bytes alone, one thread per lane.
__global__ void __launch_bounds__(256)
agc_k_expand(const u32 *__restrict__ lane_row, const u8 *__restrict__ row_status, const u64 *__restrict__ row_pks,
             const u8 *__restrict__ row_inf, u32 n_rows, u32 n, u8 *__restrict__ out_kst, u64 *__restrict__ out_pks,
             u8 *__restrict__ out_inf, const unsigned long long *__restrict__ unpublished,
             unsigned long long *__restrict__ cnt) {
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t == 0 && unpublished) cnt[AGC_CNT_UNPUB] += *unpublished;       // (one writer per launch, launches in order)
    if (!out_pks) {
        if (t >= n) return;
        const u32 r = lane_row[t];
        out_kst[t] = r < n_rows ? row_status[r] : (u8)3;       // (never out of range; if ever, SSA_MALFORMED)
        return;
    }
    if (t >= (size_t)n * 12) return;
    const u32 i = (u32)(t / 12), k = (u32)(t % 12), r = lane_row[i];
    const bool in = r < n_rows;       // (always)
    out_pks[t] = in ? row_pks[(size_t)r * 12 + k] : 0;
    if (k == 0) {
        out_inf[i] = in && row_inf[r] ? 1 : 0;
        out_kst[i] = in ? row_status[r] : (u8)3;
    }
}

// some byte of w equals AGC_BAD_KEY (exact: the classic zero-byte test on w ^ 0x01010101)
SSA_DEV bool agc_word_has_bad(u32 w) {
    const u32 x = w ^ (AGC_BAD_KEY * 0x01010101u);
    return ((x - 0x01010101u) & ~x & 0x80808080u) != 0;
}

// this thread's share (thread t of nt) of "some byte of kst[lo, hi) equals AGC_BAD_KEY": the 16-byte aligned middle of
// the range by 16-byte loads (kst is a device allocation: 256-byte aligned), the up to 15 bytes on either side singly
SSA_DEV bool agc_scan(const u8 *__restrict__ kst, u32 lo, u32 hi, u32 t, u32 nt) {
    bool bad = false;
    const u32 a = (lo + 15u) & ~15u, b = hi & ~15u;
    if (a >= b) {
        for (u32 i = lo + t; i < hi; i += nt) bad |= kst[i] == AGC_BAD_KEY;
        return bad;
    }
    for (u32 i = lo + t; i < a; i += nt) bad |= kst[i] == AGC_BAD_KEY;
    for (u32 i = b + t; i < hi; i += nt) bad |= kst[i] == AGC_BAD_KEY;
    const uint4 *p = reinterpret_cast<const uint4 *>(kst + a);
    const u32 chunks = (b - a) >> 4;
    for (u32 c = t; c < chunks; c += nt) {
        const uint4 v = p[c];
        bad |= agc_word_has_bad(v.x) | agc_word_has_bad(v.y) | agc_word_has_bad(v.z) | agc_word_has_bad(v.w);
    }
    return bad;
}

// verdicts[j] = SSA_INVALID_PUBLIC_KEY where kst[first[j], first[j + 1]) holds that status; cnt[AGC_CNT_BAD] += their
// number.  The mapping has to serve one aggregate of 2^20 lanes and 2^17 aggregates of a few lanes alike, with one writer
// per verdict word and no atomic on it: a workgroup of four waves owns FOUR consecutive aggregates.
//   - An aggregate of at most AGC_WAVE_MAX lanes is folded by the one wave of its number: 16-byte loads, __ballot, lane 0
//     stores.  2^17 small aggregates are 2^15 workgroups with every wave at work, and no barrier is reached by them.
//   - A longer aggregate is folded by the whole workgroup, one after the other (the counts are the same for every
//     thread, so the branch and its barriers are uniform): 256 threads x 16 bytes per step, __ballot per wave, one LDS
//     word per wave, thread 0 stores.  2^20 lanes come to 256 such steps per thread (computed, not timed).
// An empty aggregate has no byte to read and keeps its verdict.
__global__ void __launch_bounds__(AGC_BLOCK)
agc_k_key_verdicts(const u8 *__restrict__ kst, const u32 *__restrict__ first, u32 k, u32 *__restrict__ verdicts,
                   unsigned long long *__restrict__ cnt) {
    __shared__ u32 s_any[AGC_WAVES];
    const u32 tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u, j0 = blockIdx.x * AGC_WAVES;
    {
        const u32 j = j0 + wave;
        if (j < k) {
            const u32 lo = first[j], hi = first[j + 1];
            if (hi - lo <= AGC_WAVE_MAX) {
                const bool any = __ballot(agc_scan(kst, lo, hi, lane, 64u)) != 0ull;
                if (any && lane == 0) {
                    verdicts[j] = AGC_BAD_KEY;
                    atomicAdd(&cnt[AGC_CNT_BAD], 1ull);
                }
            }
        }
    }
    for (u32 q = 0; q < AGC_WAVES; q++) {
        const u32 j = j0 + q;
        if (j >= k) break;
        const u32 lo = first[j], hi = first[j + 1];
        if (hi - lo <= AGC_WAVE_MAX) continue;
        const bool any = __ballot(agc_scan(kst, lo, hi, tid, AGC_BLOCK)) != 0ull;
        if (lane == 0) s_any[wave] = any ? 1u : 0u;
        __syncthreads();
        if (tid == 0) {
            u32 all = 0;
            for (u32 w = 0; w < AGC_WAVES; w++) all |= s_any[w];
            if (all) {
                verdicts[j] = AGC_BAD_KEY;
                atomicAdd(&cnt[AGC_CNT_BAD], 1ull);
            }
        }
        __syncthreads();
    }
}
#endif  // SSA_NO_KERNELS

}  // namespace ssa
