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
//   ky_k_insert, ky_k_lookup, ky_k_publish   the dedup's insert and the cache's look-up and publish (dd_insert_body,
//                    kc_lookup_body, kc_publish_body) over wire sources: the 49 bytes of the records (DdWireLanes) and the
//                    seven words of the rows (DdWireRows).  dd_k_scan and kc_k_number follow the look-up as they are.
//   ky_k_decompress  one lane per miss: decompress_lane into rows base .. base + m -- the 96 bytes, the flag and the 49
//                    bytes.  ssa_k_keyset_build then runs as it is over those rows.
//   ky_k_expand      each lane's 96 key bytes and flag out of its row into a per-lane workspace: a gather, no arithmetic
//                    (one lane per word, so a wave stores 512 contiguous bytes and loads five or six whole keys).  It is
//                    what the MSM preparation and the challenge hash read as the batch's keys.
//
// Memory model: that of ssa_dedup.hpp and ssa_keycache.hpp, whose bodies these kernels run.  Workgroups of one launch
// exchange only slot words, through agent-scope atomics (ky_k_insert on the slice's table, ky_k_publish on the
// cache's); everything else is written with ordinary vector stores and read by a later launch on the same stream.
#pragma once
#include "ssa_keycache.hpp"

namespace ssa {

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

// dd_k_insert, kc_k_lookup and kc_k_publish for wire keys: the shared bodies over the 49 bytes of the records and the
// seven words of the rows (c_wire).  stride: the bytes from one lane's key to the next, 130 for records, 49 for dense
// keys (ssa_verify_aggregates_many_cached_wire)
__global__ void __launch_bounds__(256)
ky_k_insert(const u8 *__restrict__ keyed, u32 stride, u32 n, u64 k0, u64 k1, u64 *__restrict__ slots, u32 mask, u32 bound,
            u32 *__restrict__ rep, u32 *__restrict__ blk_cnt, unsigned long long *__restrict__ stats) {
    dd_insert_body(DdWireLanes{keyed, stride}, n, k0, k1, slots, mask, bound, rep, blk_cnt, stats);
}
__global__ void __launch_bounds__(256)
ky_k_lookup(const u8 *__restrict__ keyed, u32 stride, const u32 *__restrict__ reps, u32 n,
            const unsigned long long *__restrict__ stats, u64 k0, u64 k1, const u64 *__restrict__ slots, u32 mask,
            u32 bound, const u64 *__restrict__ c_wire, u32 held, u32 *__restrict__ found, u32 *__restrict__ blk_cnt,
            u32 *__restrict__ stamps, u32 epoch) {
    kc_lookup_body(DdWireLanes{keyed, stride}, DdWireRows{c_wire}, reps, n, stats, k0, k1, slots, mask, bound, held, found,
                   blk_cnt, stamps, epoch);
}
__global__ void __launch_bounds__(256)
ky_k_publish(const u64 *__restrict__ c_wire, u32 base, u32 m, u64 k0, u64 k1, u64 *__restrict__ slots, u32 mask,
             u32 bound, unsigned long long *__restrict__ unpublished) {
    kc_publish_body(DdWireRows{c_wire}, base, m, k0, k1, slots, mask, bound, unpublished);
}

// the keys of lanes reps[0, m) decompressed into rows [0, m) of out_pks / out_inf (the caller offsets them to the rows
// it fills); out_wire (or nullptr: the context's own workspaces, which keep no wire bytes) gets the 49 bytes.  A key
// that does not decode leaves (0, 0) and no flag.
__global__ void __launch_bounds__(256)
ky_k_decompress(const u8 *__restrict__ keyed, u32 stride, const u32 *__restrict__ reps, u32 m, u32 n,
                u64 *__restrict__ out_pks, u8 *__restrict__ out_inf, u64 *__restrict__ out_wire) {
    const u32 t = blockIdx.x * 256 + threadIdx.x;
    if (t >= m) return;
    const u32 i = reps[t];
    if (i >= n) return;       // (never: a representative is a lane of the slice)
    const u8 *rec = keyed + (size_t)stride * i;
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
        for (int k = 0; k < KY_WIRE_WORDS; k++) out_wire[(size_t)t * KY_WIRE_WORDS + k] = ky_wire_word(keyed, i, k, stride);
    }
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
