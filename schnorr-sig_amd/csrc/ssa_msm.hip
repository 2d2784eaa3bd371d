// MSM-form batch verification on the GPU: the algorithm the reference's verify_batch actually runs
// (src/batch.rs:31-130).
//
//     sum_i s_i R_i  -  sum_i (s_i h_i) P_i   ?=   [ sum_i s_i e_i ] G        (x-only comparison)
//
// with R_i decompressed from sig.x (src/batch.rs:104), h_i = hash_message scalars (:64-73), s_i the
// random coefficients (:75-78).  The 2n-point multi-scalar multiplication is a bucket method laid out
// for the GPU:
//   1. msm_k_prepare   per signature: decompress R, form the points R_i, -P_i and the scalars a_i = s_i,
//                      b_i = s_i h_i mod q -- written as SIGNED c-bit digits (|d| <= 2^(c-1): half the buckets
//                      of the unsigned form, a negative digit adds the negated point) --, block-reduce s_i e_i
//   2. grouping the (point, window) items by bucket -- the library's own two-level counting sort (round 4; hipCUB's
//      radix sort and its ~40 small launches are gone): the items of one window are consecutive, so a tile of 4096
//      items belongs to ONE window:
//        msm_k_hist     per tile (16384 items): LDS histogram of the HIGH 8 bits of the bucket number
//        msm_k_rowsum / msm_k_rowscan   exclusive scan of the (bin, tile) counts -> every tile's write positions
//        msm_k_scatter  per tile: items -> their (window, high-bits) group, ranks by LDS atomics (order inside a
//                       bucket means nothing to a sum: no stable pass is needed)
//        msm_k_group    per group (~4096 items, 128 buckets): LDS counting sort by the low 7 bits; the buckets'
//                       extents fall out of it (no keys are stored, no bounds pass, no global atomic anywhere)
//        msm_k_sizes / msm_k_size_ranks / msm_k_order   the buckets in global order of size, largest first: the 64
//                       buckets of a wave hold the same number of points (sizes are Poisson-distributed and a wave
//                       waits for its largest) and the launch ends on its shortest waves
//   3. msm_k_buckets   ONE BUCKET PER LANE: a lane adds up the points of its bucket with mixed
//                      additions (every exceptional case handled: equal public keys land in one bucket)
//   4. msm_k_chunks    running-sum trick on chunks of 8 buckets (short chains, 2^16 lanes);
//                      msm_k_tree sums the chunk sums of a window 16 at a time, one cooperating wave per sum
//                      (three launches); msm_k_finish is ONE cooperative
//                      block: wave 0 combines the windows by Horner's rule (the only long sequential chain
//                      of the method, ~240 doublings, wave-cooperative Fp6 arithmetic), wave 1 computes
//                      [lin]G from the comb table meanwhile; then the x coordinates are compared
// Panics of the reference (undecodable x, x not on the curve: src/batch.rs:67,104) give SSA_MALFORMED.
#define SSA_NO_KERNELS 1
#include "ssa_ctx.hpp"

#include <sys/random.h>

namespace ssa {

constexpr int MSM_CHUNK = 8;   // buckets per lane in the running-sum pass (short chains, many lanes)
// (the tree: one cooperating wave sums ctx->knobs.msm_tree_group = 16 chunk sums -- 15 additions of ~2.2 us --: 4096 -> 256 -> 16 -> 1)

constexpr u32 MSM_TILE = 16384;         // items per tile of the grouping passes (256 threads x 64): a tile writes runs of
                                        // ~64 items (256 B) per group
constexpr u32 MSM_HI_BINS = 256;        // groups per window: the bucket number's bits above the low 7
constexpr u32 MSM_LO_BITS = 7, MSM_LO_BINS = 1u << MSM_LO_BITS;
constexpr u32 MSM_MAX_WINDOWS = 32;

// the (point, window) items in window-major order: window j holds the P points (n .. 2n-1) always and the R points
// (0 .. n-1) while j < wa (a coefficient of `coeff_bytes` bytes reaches only its lowest wa windows)
struct MsmItems {
    u32 n, wa, windows;
    u32 seg_blocks, cm1;                // screened form: 256-lane blocks per segment, c - 1
    u32 tile0[MSM_MAX_WINDOWS + 1];     // first tile of window j (tiles never straddle two windows)
    u32 base[MSM_MAX_WINDOWS + 1];      // first position of window j's region in the item arrays
};
SSA_DEV u32 items_of_window(const MsmItems &it, u32 j) { return j < it.wa ? 2u * it.n : it.n; }
// item k of window j -> point index
SSA_DEV u32 item_point(const MsmItems &it, u32 j, u32 k) { return j < it.wa ? k : it.n + k; }

// (MsmShape, sc_window, write_signed_digits, st_aff_row and the per-lane checks msm_lane_key / msm_lane_decode: ssa_kernels.hpp)

// ---- 1. points and scalars ---------------------------------------------------------------------
__global__ void __launch_bounds__(256)
msm_k_prepare(const u8 *__restrict__ sigs, const u8 *__restrict__ pks, const u8 *__restrict__ pk_inf,
              const u64 *__restrict__ h_in,
              const u8 *__restrict__ coeffs, u32 coeff_bytes, size_t n, MsmShape shp, u32 wa, u64 *__restrict__ points,
              short *__restrict__ digits, u64 *__restrict__ partials, u32 *__restrict__ malformed,
              u64 *__restrict__ s_out, u8 *__restrict__ status, const u8 *__restrict__ lane_mask,
              u8 *__restrict__ recheck) {
    // recheck != nullptr (ssa_verify_many_screened): a lane whose key could not be screened
    // (lane_mask[i] != 0) or that fails a check here enters the sums as the identity, like a malformed lane, but gets NO
    // status from this kernel: recheck[i] = 1 sends it to the exact kernel, the only authority for a nonzero status.
    // h_in == nullptr (round 5): everything that does not need the challenge scalars -- the checks, R's square root,
    // the coefficient's digits, s_i e_i -- so that this kernel can run on a second stream UNDER ssa_k_hash (it fills the
    // hash kernel's tail and its own); the coefficient s_i is left in s_out for msm_k_prepare_h, which writes the digits
    // of s_i h_i once the hashes exist.
    __shared__ u64 red[256 * 4];
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    sc256 se;
#pragma unroll
    for (int k = 0; k < 4; k++) se.w[k] = 0;
    if (i < n) {
        bool ok = true;
        aff P;
        msm_lane_key(pks, i, P, ok);
        const sc256 e = ld_sc(sigs + 81 * i + 49);
        ok = ok && !sc_geq_q(e);
        // an identity key is a valid PublicKey (src/public.rs:95-101); negated and fed to the MSM it adds nothing
        // (src/batch.rs:106): the (0, 0) sentinel jac_madd skips
        const bool p_inf = pk_inf && pk_inf[i];
        aff R;
        bool r_inf;
        ok = msm_lane_decode(ok, p_inf, P, sigs + 81 * i, R, r_inf);
        if (recheck) {
            ok = ok && lane_mask[i] == 0;
            recheck[i] = (u8)(ok ? 0u : 1u);
        }
        if (!ok) {
            atomicOr(malformed, 1u);
            R.x = f6_zero(); R.y = f6_zero();
            P.x = f6_zero(); P.y = f6_zero();
        }
        // the screened form's per-lane status: 3 exactly where the per-lane check with the flag byte says 3 (the same
        // limb, range, curve and decompression checks); 0 stands until the lane's segment fails
        if (status) status[i] = (u8)(ok || recheck ? ST_OK : ST_MALFORMED);
        if (r_inf) {  // identity R: the (0, 0) sentinel jac_madd skips
            R.x = f6_zero();
            R.y = f6_zero();
        }
        if (p_inf) {
            P.x = f6_zero();
            P.y = f6_zero();
        }
        sc256 s;
#pragma unroll
        for (int k = 0; k < 4; k++) s.w[k] = 0;
        const u8 *cp = coeffs + (size_t)coeff_bytes * i;
        for (u32 b = 0; b < coeff_bytes; b++) s.w[b >> 3] |= (u64)cp[b] << (8 * (b & 7u));
        // R_i carries the coefficient itself.  A 32-byte coefficient is taken mod q (Scalar::random, :75-78) and recoded
        // over all the windows.  A narrower one is recoded over ITS OWN wa windows only -- a carry window on top would
        // hold the digit 1 for half of the points: one enormous bucket -- so when its signed digits carry out of the
        // last window (a coefficient that fills its windows to the top bit, about half of the 128-bit ones) they
        // represent  raw - 2^(wa c), and THAT value is the coefficient: it multiplies R_i (through the digits), h_i and
        // e_i (through s below) alike, so the equation is the reference's with another, equally random, coefficient.
        if (coeff_bytes >= 32u) {
            s = sc_reduce256(s);
            (void)write_signed_digits(s, shp.c, wa, digits, 2 * n, i);
        } else if (write_signed_digits(s, shp.c, wa, digits, 2 * n, i)) {      // -(2^(wa c) - raw) mod q
            const u32 bits = wa * shp.c;        // (< 256: a narrow coefficient has fewer windows than a scalar)
            sc256 s_abs;
            u64 borrow = 0;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const u32 lo_bit = 64u * (u32)k;
                const u64 pw = (bits >= lo_bit && bits < lo_bit + 64u) ? 1ull << (bits - lo_bit) : 0ull;
                const u64 d = pw - s.w[k];
                const u64 b1 = pw < s.w[k];
                const u64 d2 = d - borrow;
                const u64 b2 = d < borrow;
                s_abs.w[k] = d2;
                borrow = b1 | b2;
            }
            s = sc_neg_mod(s_abs);
        }
        if (ok) se = sc_mul_mod(s, e);                                 // s * e, :92-97
        P.y = f6_canon(f6_neg(P.y));                                   // k.0.neg(), :106
        st_aff_row(points + 12 * i, R);
        st_aff_row(points + 12 * (n + i), P);
        if (h_in) {
            sc256 h;
#pragma unroll
            for (int k = 0; k < 4; k++) h.w[k] = h_in[4 * i + k];
            const sc256 sh = sc_mul_mod(s, h);                         // hashes[i] *= scalars[i], :109-111
            (void)write_signed_digits(sh, shp.c, shp.windows, digits, 2 * n, n + i);
        } else {
#pragma unroll
            for (int k = 0; k < 4; k++) s_out[4 * i + k] = s.w[k];
        }
    }
    // block reduction of s_i e_i mod q
#pragma unroll
    for (int k = 0; k < 4; k++) red[threadIdx.x * 4 + k] = se.w[k];
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
        for (int k = 0; k < 4; k++) partials[4 * blockIdx.x + k] = red[k];
    }
}

// the half of msm_k_prepare that needs the challenge scalars: the digits of s_i h_i for the point -P_i
__global__ void __launch_bounds__(256)
msm_k_prepare_h(const u64 *__restrict__ h_in, const u64 *__restrict__ s_in, size_t n, MsmShape shp,
                short *__restrict__ digits) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    sc256 s, h;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        s.w[k] = s_in[4 * i + k];
        h.w[k] = h_in[4 * i + k];
    }
    (void)write_signed_digits(sc_mul_mod(s, h), shp.c, shp.windows, digits, 2 * n, n + i);   // hashes[i] *= scalars[i], :109-111
}

// ---- 2. grouping the items by bucket ------------------------------------------------------------------
// bucket number of a digit: |d| - 1 in [0, 2^(c-1)); hi = its bits above the low 7 (the group), lo = the low 7
SSA_DEV bool tile_of_block(const MsmItems &it, u32 blk, u32 &j, u32 &k0, u32 &cnt) {
    j = 0;
#pragma unroll 1
    while (j + 1 < it.windows && blk >= it.tile0[j + 1]) j++;
    const u32 items = items_of_window(it, j);
    k0 = (blk - it.tile0[j]) * MSM_TILE;
    if (k0 >= items) return false;
    cnt = items - k0 < MSM_TILE ? items - k0 : MSM_TILE;
    return true;
}

// Bucket number of a nonzero digit of point `pt`: |d| - 1 in [0, 2^(c-1)); the screened form (SEG) keys the buckets by
// (window, segment, digit) instead: b = segment << (c - 1) | (|d| - 1), where the segment is that of the point's lane
// for R_i and -P_i alike.  hi = the bits above the low 7 (the group), lo = the low 7.
template <bool SEG>
SSA_DEV u32 bucket_of(const MsmItems &it, u32 pt, int d) {
    const u32 b = (u32)((d < 0 ? -d : d) - 1);
    if (!SEG) return b;
    const u32 lane = pt < it.n ? pt : pt - it.n;
    return (((lane >> 8) / it.seg_blocks) << it.cm1) | b;
}

// tile_hist[(j * 256 + bin) * tmax + tile] = items of this tile whose bucket lies in group `bin`
template <bool SEG>
SSA_DEV void hist_tile(const short *__restrict__ digits, const MsmItems &it, u32 tmax, u32 *__restrict__ tile_hist) {
    __shared__ u32 h[MSM_HI_BINS];
    h[threadIdx.x] = 0u;
    __syncthreads();
    u32 j, k0, cnt;
    if (!tile_of_block(it, blockIdx.x, j, k0, cnt)) return;        // (block-uniform)
    const short *dj = digits + (size_t)j * (2u * (size_t)it.n);
    for (u32 k = threadIdx.x; k < cnt; k += 256u) {
        const u32 pt = item_point(it, j, k0 + k);
        const int d = dj[pt];
        if (d != 0) atomicAdd(&h[bucket_of<SEG>(it, pt, d) >> MSM_LO_BITS], 1u);
    }
    __syncthreads();
    tile_hist[((size_t)j * MSM_HI_BINS + threadIdx.x) * tmax + (blockIdx.x - it.tile0[j])] = h[threadIdx.x];
}
__global__ void __launch_bounds__(256)
msm_k_hist(const short *__restrict__ digits, MsmItems it, u32 tmax, u32 *__restrict__ tile_hist) {
    hist_tile<false>(digits, it, tmax, tile_hist);
}
__global__ void __launch_bounds__(256)
msm_k_hist_seg(const short *__restrict__ digits, MsmItems it, u32 tmax, u32 *__restrict__ tile_hist) {
    hist_tile<true>(digits, it, tmax, tile_hist);
}

// Exclusive scan of a window's (bin, tile) counts in bin-major order, in place, in two steps:
//   msm_k_rowsum  one wave per (window, bin) row: the row's total
//   msm_k_rowscan one block per row: base = the window's region + the totals of the bins before it, then the row's
//                 exclusive scan in place -> the position at which tile `tile` writes its first item of group `bin`;
//                 gstart[j * 257 + bin] = first position of the group, gstart[j * 257 + 256] = one past the window's last
__global__ void __launch_bounds__(64)
msm_k_rowsum(MsmItems it, u32 tmax, const u32 *__restrict__ tile_hist, u32 *__restrict__ rowsum) {
    const u32 row = blockIdx.x, j = row / MSM_HI_BINS;
    const u32 tiles = it.tile0[j + 1] - it.tile0[j];
    const u32 *th = tile_hist + (size_t)row * tmax;
    u32 sum = 0;
    for (u32 t = threadIdx.x; t < tiles; t += 64u) sum += th[t];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) sum += __shfl_down(sum, off, 64);
    if (threadIdx.x == 0) rowsum[row] = sum;
}

__global__ void __launch_bounds__(256)
msm_k_rowscan(MsmItems it, u32 tmax, const u32 *__restrict__ rowsum, u32 *__restrict__ tile_hist,
              u32 *__restrict__ gstart) {
    __shared__ u32 sh[256];
    const u32 row = blockIdx.x, j = row / MSM_HI_BINS, bin = row % MSM_HI_BINS;
    const u32 tiles = it.tile0[j + 1] - it.tile0[j];
    // totals of the bins before this one (and of all of them, for the sentinel)
    const u32 mine = rowsum[j * MSM_HI_BINS + threadIdx.x];
    sh[threadIdx.x] = mine;
    __syncthreads();
    for (u32 off = 1; off < 256u; off <<= 1) {
        const u32 v = threadIdx.x >= off ? sh[threadIdx.x - off] : 0u;
        __syncthreads();
        sh[threadIdx.x] += v;
        __syncthreads();
    }
    const u32 before = bin ? sh[bin - 1] : 0u, all = sh[255];
    __syncthreads();
    u32 run = it.base[j] + before;
    if (threadIdx.x == 0) {
        gstart[j * (MSM_HI_BINS + 1) + bin] = run;
        if (bin == MSM_HI_BINS - 1) gstart[j * (MSM_HI_BINS + 1) + MSM_HI_BINS] = it.base[j] + all;
    }
    u32 *th = tile_hist + (size_t)row * tmax;
    for (u32 t0 = 0; t0 < tiles; t0 += 256u) {           // the row in pieces of 256 tiles, the running total carried
        const u32 t = t0 + threadIdx.x;
        const u32 c = t < tiles ? th[t] : 0u;
        sh[threadIdx.x] = c;
        __syncthreads();
        for (u32 off = 1; off < 256u; off <<= 1) {
            const u32 v = threadIdx.x >= off ? sh[threadIdx.x - off] : 0u;
            __syncthreads();
            sh[threadIdx.x] += v;
            __syncthreads();
        }
        if (t < tiles) th[t] = run + sh[threadIdx.x] - c;
        const u32 piece = sh[255];
        __syncthreads();
        run += piece;
    }
}

// items -> their group, ONE word per item: v1[pos] = point index (24 bits: 2n <= 2^24 per slice) | low 7 bits of the
// bucket number << 24 | sign << 31
template <bool SEG>
SSA_DEV void scatter_tile(const short *__restrict__ digits, const MsmItems &it, u32 tmax, const u32 *__restrict__ tile_hist,
                          u32 *__restrict__ v1) {
    __shared__ u32 cur[MSM_HI_BINS];
    u32 j, k0, cnt;
    if (!tile_of_block(it, blockIdx.x, j, k0, cnt)) return;
    cur[threadIdx.x] = tile_hist[((size_t)j * MSM_HI_BINS + threadIdx.x) * tmax + (blockIdx.x - it.tile0[j])];
    __syncthreads();
    const short *dj = digits + (size_t)j * (2u * (size_t)it.n);
    for (u32 k = threadIdx.x; k < cnt; k += 256u) {
        const u32 pt = item_point(it, j, k0 + k);
        const int d = dj[pt];
        if (d != 0) {
            const u32 b = bucket_of<SEG>(it, pt, d);
            const u32 pos = atomicAdd(&cur[b >> MSM_LO_BITS], 1u);
            v1[pos] = pt | ((b & (MSM_LO_BINS - 1u)) << 24) | (d < 0 ? 0x80000000u : 0u);
        }
    }
}
__global__ void __launch_bounds__(256)
msm_k_scatter(const short *__restrict__ digits, MsmItems it, u32 tmax, const u32 *__restrict__ tile_hist,
              u32 *__restrict__ v1) {
    scatter_tile<false>(digits, it, tmax, tile_hist, v1);
}
__global__ void __launch_bounds__(256)
msm_k_scatter_seg(const short *__restrict__ digits, MsmItems it, u32 tmax, const u32 *__restrict__ tile_hist,
                  u32 *__restrict__ v1) {
    scatter_tile<true>(digits, it, tmax, tile_hist, v1);
}

// one block per (window, group): counting sort of the group's items by the low 7 bits of their bucket number; the
// 128 buckets' extents are the by-product: bstart[t], cnt[t] for t = j * buckets + group * 128 + lo
__global__ void __launch_bounds__(256)
msm_k_group(const u32 *__restrict__ gstart, const u32 *__restrict__ v1, MsmShape sh, u32 *__restrict__ v2,
            u32 *__restrict__ bstart, u32 *__restrict__ cnt) {
    __shared__ u32 h[MSM_LO_BINS], pre[MSM_LO_BINS];
    const u32 j = blockIdx.x / MSM_HI_BINS, bin = blockIdx.x % MSM_HI_BINS;
    if (bin * MSM_LO_BINS >= sh.buckets) return;                    // (narrow windows have fewer groups)
    const u32 gs = gstart[j * (MSM_HI_BINS + 1) + bin], ge = gstart[j * (MSM_HI_BINS + 1) + bin + 1];
    if (threadIdx.x < MSM_LO_BINS) h[threadIdx.x] = 0u;
    __syncthreads();
    for (u32 p = gs + threadIdx.x; p < ge; p += 256u) atomicAdd(&h[(v1[p] >> 24) & (MSM_LO_BINS - 1u)], 1u);
    __syncthreads();
    if (threadIdx.x < 64u) {          // exclusive scan of the 128 counts on one wave: two per lane
        const u32 a = h[2u * threadIdx.x], b = h[2u * threadIdx.x + 1u];
        u32 incl = a + b;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const u32 v = __shfl_up(incl, off, 64);
            if ((int)threadIdx.x >= off) incl += v;
        }
        pre[2u * threadIdx.x] = incl - a - b;
        pre[2u * threadIdx.x + 1u] = incl - b;
    }
    __syncthreads();
    if (threadIdx.x < MSM_LO_BINS && bin * MSM_LO_BINS + threadIdx.x < sh.buckets) {
        const size_t t = (size_t)j * sh.buckets + bin * MSM_LO_BINS + threadIdx.x;
        bstart[t] = gs + pre[threadIdx.x];
        cnt[t] = h[threadIdx.x];
    }
    __syncthreads();
    for (u32 p = gs + threadIdx.x; p < ge; p += 256u) {
        const u32 v = v1[p];
        v2[gs + atomicAdd(&pre[(v >> 24) & (MSM_LO_BINS - 1u)], 1u)] = v & 0x80ffffffu;
    }
}

// Bucket sizes are Poisson-distributed (mean ~48 at n = 2^20) and a wave waits for its largest bucket: the lanes take
// the buckets in GLOBAL order of size, largest first (sizes clamped at 1023) -- the 64 buckets of a wave hold the same
// number of points, and the long waves start first, so the launch ends on its shortest ones (with four waves per
// slot at 2^20 signatures a long wave started late would idle most of the chip: measured 3.5 ms against 3.0 for the
// same additions when the order was only local).  Counting sort in three small launches; the only global atomics are
// one per (block, size class present in the block): ~60 per block.
__global__ void __launch_bounds__(1024)
msm_k_sizes(const u32 *__restrict__ cnt, u32 nb, u32 *__restrict__ ghist) {
    __shared__ u32 h[1024];
    const u32 t = blockIdx.x * 1024u + threadIdx.x;
    h[threadIdx.x] = 0u;
    __syncthreads();
    if (t < nb) atomicAdd(&h[cnt[t] < 1023u ? cnt[t] : 1023u], 1u);
    __syncthreads();
    if (h[threadIdx.x]) atomicAdd(&ghist[threadIdx.x], h[threadIdx.x]);
}
// gcur[c] = first rank of size class c when the classes are laid out from 1023 down to 0
__global__ void __launch_bounds__(1024)
msm_k_size_ranks(const u32 *__restrict__ ghist, u32 *__restrict__ gcur) {
    __shared__ u32 h[1024];
    const u32 mine = ghist[1023u - threadIdx.x];
    h[threadIdx.x] = mine;
    __syncthreads();
    for (u32 off = 1; off < 1024u; off <<= 1) {
        const u32 v = threadIdx.x >= off ? h[threadIdx.x - off] : 0u;
        __syncthreads();
        h[threadIdx.x] += v;
        __syncthreads();
    }
    gcur[1023u - threadIdx.x] = h[threadIdx.x] - mine;
}
__global__ void __launch_bounds__(1024)
msm_k_order(const u32 *__restrict__ cnt, u32 nb, u32 *__restrict__ gcur, u32 *__restrict__ order) {
    __shared__ u32 h[1024], base[1024];
    const u32 t = blockIdx.x * 1024u + threadIdx.x;
    h[threadIdx.x] = 0u;
    __syncthreads();
    const u32 c = t < nb ? (cnt[t] < 1023u ? cnt[t] : 1023u) : 0u;
    if (t < nb) atomicAdd(&h[c], 1u);
    __syncthreads();
    if (h[threadIdx.x]) base[threadIdx.x] = atomicAdd(&gcur[threadIdx.x], h[threadIdx.x]);   // this block's run of the class
    __syncthreads();
    h[threadIdx.x] = 0u;
    __syncthreads();
    if (t < nb) order[base[c] + atomicAdd(&h[c], 1u)] = t;
}

// ---- 3. one bucket per lane ---------------------------------------------------------------------
__global__ void __launch_bounds__(256, 2)
msm_k_buckets(const u64 *__restrict__ points, const u32 *__restrict__ vals, const u32 *__restrict__ bstart,
              const u32 *__restrict__ cnt, const u32 *__restrict__ order, size_t nb, u64 *__restrict__ bsum) {
    const size_t lane_id = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (lane_id >= nb) return;
    const size_t t = order[lane_id];
    jac acc = jac_identity();
    const u32 lo = bstart[t], hi = lo + cnt[t];
#pragma unroll 1
    for (u32 p = lo; p < hi; p++) {
        const u32 item = vals[p];
        aff q = ld_aff(points + 12 * (size_t)(item & 0x7fffffffu));
        if (item >> 31) q.y = f6_neg(q.y);                // a negative digit adds the negated point ((0, 0) stays (0, 0))
        acc = jac_madd_fast(acc, q);      // asm block; identity / equal points fall back to the exact addition
    }
    st_jac(bsum + 18 * t, acc);
}

// ---- 4. bucket reduction ------------------------------------------------------------------------
// chunk of MSM_CHUNK buckets [k0, k0 + L) of a window, bucket k weighing k + 1 (|digit|):
//   sum_k (k + 1) B_k = sum_k (k - k0 + 1) B_k + k0 sum_k B_k
// (2^16 lanes are one wave per SIMD anyway: with one wave per SIMD allowed the general addition keeps its values in
//  registers -- 256 VGPRs + 384 B of scratch before)
// (SEG: a window holds one run of 2^(c-1) buckets per segment, and a chunk's weights count from its segment's first
//  bucket: k0 mod 2^(c-1))
template <bool SEG>
SSA_DEV void chunk_sum(const u64 *__restrict__ bsum, const MsmShape &sh, u64 *__restrict__ chunk_out) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (size_t)sh.windows * sh.chunks) return;
    const u32 j = (u32)(t / sh.chunks), ch = (u32)(t % sh.chunks);
    const u32 len = sh.buckets < (u32)MSM_CHUNK ? sh.buckets : (u32)MSM_CHUNK;
    const u32 k0 = ch * len;
    // the top bucket opens both sums (two additions to the identity saved per chunk)
    jac running = ld_jac(bsum + 18 * ((size_t)j * sh.buckets + (k0 + len - 1))), total = running;
#pragma unroll 1
    for (int k = (int)(k0 + len) - 2; k >= (int)k0; k--) {
        const jac b = ld_jac(bsum + 18 * ((size_t)j * sh.buckets + (u32)k));
        running = jac_add(running, b);
        total = jac_add(total, running);
    }
    // + [k0] running: double-and-add from the top set bit of the weight, the doublings through the ladder's
    // generated statement
    const u32 m = SEG ? k0 & ((1u << (sh.c - 1)) - 1u) : k0;
    if (m > 0) {
        jac acc = running;
#pragma unroll 1
        for (int bit = 30 - __builtin_clz(m); bit >= 0; bit--) {
            acc = jac_dbl_n(acc, 1u);
            if ((m >> bit) & 1u) acc = jac_add(acc, running);
        }
        total = jac_add(total, acc);
    }
    st_jac(chunk_out + 18 * t, total);
}
__global__ void __launch_bounds__(256, 1)
msm_k_chunks(const u64 *__restrict__ bsum, MsmShape sh, u64 *__restrict__ chunk_out) {
    chunk_sum<false>(bsum, sh, chunk_out);
}
__global__ void __launch_bounds__(256, 1)
msm_k_chunks_seg(const u64 *__restrict__ bsum, MsmShape sh, u64 *__restrict__ chunk_out) {
    chunk_sum<true>(bsum, sh, chunk_out);
}

// tree step: out[j][g] = sum of `group` consecutive points of window j's `count` inputs.  ONE WAVE per output, the
// general additions on the wave-cooperative arithmetic (ssa_coop.hpp: ~2.2 us per addition, where a lone lane takes ~15):
// three launches of 16-way sums replace round 3's twelve pairwise ones (0.20 -> 0.1 ms).
__global__ void __launch_bounds__(64)
msm_k_tree(const u64 *__restrict__ in, u32 windows, u32 count, u32 group, u64 *__restrict__ out) {
    __shared__ CoopLds L;
    const u32 lane = threadIdx.x;
    const u32 groups = (count + group - 1) / group;
    const u32 t = blockIdx.x;
    if (t >= windows * groups) return;
    const u32 j = t / groups, g = t % groups;
    const u32 lo = g * group, hi = (lo + group < count) ? lo + group : count;    // (lo < hi: groups = ceil(count / group))
    int tt[9];
#pragma unroll
    for (int k = 0; k < 9; k++) tt[k] = 7 + k;
    // accumulator 0..3 (X, Y, Z, W = Z^4), addend 4..6
    coop_sum_points(L, 0, 4, tt, lane, 0, hi - lo, 0u, [&](u32 k) { return in + 18 * ((size_t)j * count + lo + k); });
    if (lane < 18) out[18 * (size_t)t + lane] = fp_canon(L.slot[(int)(lane / 6u)][lane % 6u]);
}

// ---- coefficients ---------------------------------------------------------------------------------
// Scalar::random(rng) (src/batch.rs:75-78) when the caller supplies none: 128-bit coefficients from a
// ChaCha20 keystream (RFC 8439 block function, 32-bit block counter) keyed per call with 44 bytes of
// getrandom(2).  One 64-byte block = four coefficients per lane; drawing 16 MB on the host took ~20 ms.
struct ChaChaKey {
    u32 key[8];
    u32 nonce[3];
};
SSA_DEV u32 rotl32(u32 x, int n) { return (x << n) | (x >> (32 - n)); }
#define SSA_QR(a, b, c, d)          \
    a += b; d ^= a; d = rotl32(d, 16); \
    c += d; b ^= c; b = rotl32(b, 12); \
    a += b; d ^= a; d = rotl32(d, 8);  \
    c += d; b ^= c; b = rotl32(b, 7)
__global__ void __launch_bounds__(256)
msm_k_chacha20(ChaChaKey kn, u32 counter0, size_t n_blocks, u32 *__restrict__ out) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_blocks) return;
    u32 st[16] = {0x61707865u, 0x3320646eu, 0x79622d32u, 0x6b206574u, kn.key[0], kn.key[1], kn.key[2], kn.key[3],
                  kn.key[4], kn.key[5], kn.key[6], kn.key[7], counter0 + (u32)t, kn.nonce[0], kn.nonce[1], kn.nonce[2]};
    u32 x[16];
#pragma unroll
    for (int i = 0; i < 16; i++) x[i] = st[i];
#pragma unroll 1
    for (int r = 0; r < 10; r++) {
        SSA_QR(x[0], x[4], x[8], x[12]);
        SSA_QR(x[1], x[5], x[9], x[13]);
        SSA_QR(x[2], x[6], x[10], x[14]);
        SSA_QR(x[3], x[7], x[11], x[15]);
        SSA_QR(x[0], x[5], x[10], x[15]);
        SSA_QR(x[1], x[6], x[11], x[12]);
        SSA_QR(x[2], x[7], x[8], x[13]);
        SSA_QR(x[3], x[4], x[9], x[14]);
    }
#pragma unroll
    for (int i = 0; i < 16; i++) out[16 * t + i] = x[i] + st[i];   // little-endian words = the keystream bytes
}

// A record that carries no point (include/schnorr_sig_amd.h, "shard records"): 24 words, all zero but the malformed flag
// at word 22 and SSA_MSM_RECORD_MAGIC at word 23.  malformed = false is the record of an empty shard: the identity (Z = 0),
// sum s_i e_i = 0 -- and the magic word: a buffer that nobody wrote (all zero) is NOT a record.  Called by whole blocks.
SSA_DEV void msm_record_flag(u64 *__restrict__ rec, bool malformed) {
    if (threadIdx.x < 24) rec[threadIdx.x] = threadIdx.x == 22 ? (u64)malformed : threadIdx.x == 23 ? SSA_MSM_RECORD_MAGIC : 0ull;
}

// ---- the one sequential chain of the reduction ---------------------------------------------------
// left = sum_j 2^(c j) W_j by Horner's rule: (windows - 1) x (c doublings + one addition), a chain of ~240
// dependent doublings.  A lone lane ran it at ~80 us per doubling; here wave 0 of the block works on the
// one point (wave-cooperative Fp6 arithmetic, ssa_coop.hpp: ~2.5 us per doubling) while wave 1 adds up
// lin = sum of the blocks' partial sums and computes right = [lin] G from the comb table.
// Verdict: x-only comparison, left.get_x() == right.get_x() (src/batch.rs:98-100, :125-129).
__global__ void __launch_bounds__(128)
msm_k_finish(const u64 *__restrict__ win_in, MsmShape sh, const u64 *__restrict__ partials, u32 n_partials,
             const u64 *__restrict__ gtab, const u32 *__restrict__ malformed, u32 *__restrict__ verdict,
             u64 *__restrict__ partial_out) {
    // partial_out != nullptr: this device holds one shard of the batch (ssa_multi_verify_batch_msm): emit the
    // shard's left-hand point (X, Y, Z: words 0..17), its sum s_i e_i (18..21) and the malformed flag (22) instead
    // of a verdict; device 0 adds the shards up with this same kernel (sh.c = 0: no doublings between the "windows")
    __shared__ CoopLds L;
    __shared__ u64 lin_sh[64][4];
    const u32 lane = threadIdx.x & 63u;
    const int ws = (int)(threadIdx.x >> 6);
    if (*malformed) {   // block-uniform
        if (partial_out) msm_record_flag(partial_out, true);
        else if (threadIdx.x == 0) *verdict = ST_MALFORMED;
        return;
    }
    // slots: wave 0 accumulator 0..3 (X, Y, Z, W), addend 4..6, scratch 7..15; wave 1 accumulator 20..23,
    // addend 24..25, scratch 26..34
    int t[9];
#pragma unroll
    for (int k = 0; k < 9; k++) t[k] = (ws ? 26 : 7) + k;
    if (ws == 0) {   // Horner from the top window down
        coop_sum_points(L, 0, 4, t, lane, ws, sh.windows, sh.c,
                        [&](u32 k) { return win_in + 18 * (size_t)(sh.windows - 1 - k); });
    } else {
        const sc256 lin = wave_sum_mod_q(lin_sh, partials, 0, n_partials, lane);
        if (partial_out) {   // the record carries lin itself, not [lin]G
            if (lane < 4) partial_out[18 + lane] = lin.w[lane];
        } else {
            coop_set_identity(L, 20, lane, ws);
            coop_comb_add(L, 20, 24, 25, lin, gtab, t, lane, ws);
        }
    }
    __syncthreads();
    if (partial_out) {
        // The record carries the point in its CANONICAL form: affine (x, y, 1), or (0, 0, 0) for the identity.  The
        // grouping passes rank the items of a bucket by LDS atomics, so the order of the additions -- and with it
        // the Jacobian representative -- differs from run to run; the point does not, and equal shards give equal
        // bytes (records are compared, committed as fixtures and cross process boundaries).
        if (ws == 0) {
            const bool inf = coop_is_zero(L, 2, lane, ws);
            if (!inf) {
                coop_inv(L, 7, 2, 8, 9, 10, lane, ws);     // 1 / Z
                coop_mul(L, 8, 7, 7, lane, ws);            // 1 / Z^2
                coop_mul(L, 0, 0, 8, lane, ws);            // x
                coop_mul(L, 8, 8, 7, lane, ws);            // 1 / Z^3
                coop_mul(L, 1, 1, 8, lane, ws);            // y
            }
            if (lane < 18) {
                const u32 v = lane / 6u, c = lane % 6u;
                u64 w = v == 2 ? (c == 0 ? 1ull : 0ull) : fp_canon(L.slot[(int)v][c]);
                partial_out[lane] = inf ? 0ull : w;
            }
        }
        if (threadIdx.x == 0) {
            partial_out[22] = 0;
            partial_out[23] = SSA_MSM_RECORD_MAGIC;
        }
        return;
    }
    if (ws == 0) {
        // X_l Z_r^2 == X_r Z_l^2; the identity's x is taken as 0
        const bool li = coop_is_zero(L, 2, lane, ws), ri = coop_is_zero(L, 22, lane, ws);
        bool eq;
        if (li || ri) {
            eq = (li && ri) || (li && coop_is_zero(L, 20, lane, ws)) || (ri && coop_is_zero(L, 0, lane, ws));
        } else {
            coop_mul(L, 7, 22, 22, lane, ws);
            coop_mul(L, 7, 0, 7, lane, ws);
            coop_mul(L, 8, 2, 2, lane, ws);
            coop_mul(L, 8, 20, 8, lane, ws);
            eq = coop_eq(L, 7, 8, lane, ws);
        }
        if (lane == 0) *verdict = eq ? ST_OK : ST_INVALID_SIG;
    }
}

// ---- the screened form: one verdict per segment ---------------------------
// Block s per segment s (the same split as msm_k_finish): wave 0 runs Horner over the segment's window sums
// win_in[j * segs + s], wave 1 adds up the segment's block partials of s_i e_i (segments are whole 256-lane blocks,
// the last one ragged) and computes [lin_s] G from the comb table.  Then the EXACT point comparison
//     sum s_i R_i - sum s_i h_i P_i  ==  [sum s_i e_i] G       (identity = Z 0 on both sides)
// -- not x-only: a segment whose equation holds only up to the sign of both sides fails.  Malformed lanes entered
// the sums as the identity with s_i e_i = 0 (msm_k_prepare); the global flag is not read.
__global__ void __launch_bounds__(128)
msm_k_finish_seg(const u64 *__restrict__ win_in, MsmShape sh, u32 segs, u32 seg_blocks, const u64 *__restrict__ partials,
                 u32 n_partials, const u64 *__restrict__ gtab, u8 *__restrict__ seg_ok, const u8 *__restrict__ rhs) {
    __shared__ CoopLds L;
    __shared__ u64 lin_sh[64][4];
    const u32 lane = threadIdx.x & 63u, s = blockIdx.x;
    const int ws = (int)(threadIdx.x >> 6);
    // slots as msm_k_finish: wave 0 accumulator 0..3, addend 4..6, scratch 7..15; wave 1 accumulator 20..23,
    // addend 24..25, scratch 26..34
    int t[9];
#pragma unroll
    for (int k = 0; k < 9; k++) t[k] = (ws ? 26 : 7) + k;
    if (ws == 0) {   // Horner over this segment's window sums
        coop_sum_points(L, 0, 4, t, lane, ws, sh.windows, sh.c,
                        [&](u32 k) { return win_in + 18 * ((size_t)(sh.windows - 1 - k) * segs + s); });
    } else {
        const u32 b_lo = s * seg_blocks, b_hi = b_lo + seg_blocks < n_partials ? b_lo + seg_blocks : n_partials;
        sc256 lin = wave_sum_mod_q(lin_sh, partials, b_lo, b_hi, lane);
        // rhs != nullptr (ssa_verify_aggregates_many): the segment's right-hand scalar is given --
        // 32 bytes per segment, the aggregate's e_agg -- instead of the sum of the block partials (zero there: e = 0)
        if (rhs) lin = ld_sc(rhs + 32 * (size_t)s);
        coop_set_identity(L, 20, lane, ws);
        coop_comb_add(L, 20, 24, 25, lin, gtab, t, lane, ws);
    }
    __syncthreads();
    if (ws == 0) {
        const bool eq = coop_jac_equal(L, 0, 20, 7, lane, ws);
        if (lane == 0) seg_ok[s] = eq ? 1u : 0u;
    }
}

// the failing segments of a slice (ascending; only the last segment of a slice can be ragged, so failing segment f
// lands at compact lane f * seg_lanes)
struct ScreenList {
    u32 count, seg_lanes, n;
    uint16_t id[256];
};

SSA_DEV void copy_run(u8 *__restrict__ dst, const u8 *__restrict__ src, size_t bytes, size_t tid, size_t nth) {
    if (((reinterpret_cast<uintptr_t>(dst) | reinterpret_cast<uintptr_t>(src)) & 15u) == 0) {
        const size_t v = bytes / 16;
        for (size_t k = tid; k < v; k += nth) reinterpret_cast<uint4 *>(dst)[k] = reinterpret_cast<const uint4 *>(src)[k];
        for (size_t k = v * 16 + tid; k < bytes; k += nth) dst[k] = src[k];
    } else {
        for (size_t k = tid; k < bytes; k += nth) dst[k] = src[k];
    }
}

// the lanes of the failing segments -> compact buffers (signature 81 B, key 96 B, pk_inf 1 B, challenge scalar 32 B):
// blockIdx.y = failing segment, the x blocks share its bytes
__global__ void __launch_bounds__(256)
msm_k_screen_gather(ScreenList sl, const u8 *__restrict__ sigs, const u8 *__restrict__ pks, const u8 *__restrict__ pk_inf,
                    const u64 *__restrict__ h, u8 *__restrict__ g_sigs, u8 *__restrict__ g_pks, u8 *__restrict__ g_inf,
                    u64 *__restrict__ g_h) {
    const u32 f = blockIdx.y;
    if (f >= sl.count) return;
    const size_t lo = (size_t)sl.id[f] * sl.seg_lanes, dlo = (size_t)f * sl.seg_lanes;
    if (lo >= sl.n) return;
    const size_t cnt = sl.n - lo < sl.seg_lanes ? sl.n - lo : sl.seg_lanes;
    const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, nth = (size_t)gridDim.x * blockDim.x;
    copy_run(g_sigs + 81 * dlo, sigs + 81 * lo, 81 * cnt, tid, nth);
    copy_run(g_pks + 96 * dlo, pks + 96 * lo, 96 * cnt, tid, nth);
    copy_run(reinterpret_cast<u8 *>(g_h + 4 * dlo), reinterpret_cast<const u8 *>(h + 4 * lo), 32 * cnt, tid, nth);
    if (pk_inf) copy_run(g_inf + dlo, pk_inf + lo, cnt, tid, nth);
}

// compact statuses -> their lanes
__global__ void __launch_bounds__(256)
msm_k_screen_scatter(ScreenList sl, size_t m, const u8 *__restrict__ g_status, u8 *__restrict__ status) {
    const size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= m) return;
    const u32 f = (u32)(c / sl.seg_lanes);
    status[(size_t)sl.id[f] * sl.seg_lanes + c % sl.seg_lanes] = g_status[c];
}

// *n_fail += number of nonzero statuses (one ballot and one atomic per wave)
__global__ void __launch_bounds__(256)
msm_k_screen_count(const u8 *__restrict__ status, size_t n, unsigned long long *__restrict__ n_fail) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const unsigned long long bad = __ballot(i < n && status[i] != 0);
    if ((threadIdx.x & 63u) == 0 && bad) atomicAdd(n_fail, (unsigned long long)__popcll(bad));
}

// ---- ssa_verify_many_screened: the lanes to re-check as an index list ------------------------
// Everything these kernels write is read by a LATER launch on the same stream (or by the host after the stream has been
// synchronised); the only values that workgroups of one launch combine are counters, by agent-scope atomic adds.
constexpr u32 SCR_BLOCK = 256;

// lane_mask[i] = lane i cannot be screened because of its key: the per-key check found it malformed or outside the
// prime-order subgroup.  Such a lane stays out of every sum, WHATEVER the flags: the per-key check computes [q]P == O
// anyway, and a key outside the subgroup is the one way an error of pure small order gets into a sum on the key side.
// Without SSA_FLAG_CHECK_TORSION the exact kernel then verifies the lane against that key as ssa_verify_many does.
__global__ void __launch_bounds__(256)
msm_k_screen_keymask(const u32 *__restrict__ key_idx, const u8 *__restrict__ key_status, u32 n_keys, u32 n,
                     u8 *__restrict__ lane_mask) {
    const u32 i = blockIdx.x * SCR_BLOCK + threadIdx.x;
    if (i >= n) return;
    const u32 k = key_idx[i];
    lane_mask[i] = (u8)((k < n_keys && key_status[k] == ST_OK) ? 0u : 1u);
}

// mark[i] (in: msm_k_prepare's "could not be screened"; out: "re-check") |= the lane's segment failed;
// blk_cnt[b] = marked lanes of workgroup b; cnt[0] += lanes that could not be screened
__global__ void __launch_bounds__(256)
msm_k_screen_mark(const u8 *__restrict__ seg_ok, u32 seg_lanes, u32 n, u8 *__restrict__ mark, u32 *__restrict__ blk_cnt,
                  unsigned long long *__restrict__ cnt) {
    __shared__ u32 wave_cnt[SCR_BLOCK / 64];
    const u32 i = blockIdx.x * SCR_BLOCK + threadIdx.x;
    const bool unscreened = i < n && mark[i] != 0;
    const bool m = i < n && (unscreened || seg_ok[i / seg_lanes] == 0);
    if (i < n) mark[i] = (u8)(m ? 1u : 0u);
    const unsigned long long ms = __ballot(m), us = __ballot(unscreened);
    if ((threadIdx.x & 63u) == 0) {
        wave_cnt[threadIdx.x >> 6] = (u32)__popcll(ms);
        if (us) atomicAdd(cnt, (unsigned long long)__popcll(us));
    }
    __syncthreads();
    if (threadIdx.x == 0) blk_cnt[blockIdx.x] = wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
}

// ONE workgroup: blk_off[b] = marked lanes in front of workgroup b's; cnt[1] = the length of the list
__global__ void __launch_bounds__(256)
msm_k_screen_scan(const u32 *__restrict__ blk_cnt, u32 nb, u32 *__restrict__ blk_off, unsigned long long *__restrict__ cnt) {
    __shared__ u32 part[SCR_BLOCK];
    const u32 t = threadIdx.x, per = (nb + SCR_BLOCK - 1) / SCR_BLOCK;
    const u32 lo = t * per < nb ? t * per : nb, hi = lo + per < nb ? lo + per : nb;
    u32 sum = 0;
    for (u32 b = lo; b < hi; b++) sum += blk_cnt[b];
    part[t] = sum;
    __syncthreads();
    if (t == 0) {
        u32 acc = 0;
        for (u32 k = 0; k < SCR_BLOCK; k++) {
            const u32 v = part[k];
            part[k] = acc;
            acc += v;
        }
        cnt[1] = acc;
    }
    __syncthreads();
    u32 acc = part[t];
    for (u32 b = lo; b < hi; b++) {
        blk_off[b] = acc;
        acc += blk_cnt[b];
    }
}

// list[c] = the c-th marked lane, in lane order
__global__ void __launch_bounds__(256)
msm_k_screen_list(const u8 *__restrict__ mark, u32 n, const u32 *__restrict__ blk_off, u32 *__restrict__ list) {
    __shared__ u32 wave_cnt[SCR_BLOCK / 64];
    const u32 i = blockIdx.x * SCR_BLOCK + threadIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const bool m = i < n && mark[i] != 0;
    const unsigned long long ms = __ballot(m);
    if (lane == 0) wave_cnt[wave] = (u32)__popcll(ms);
    __syncthreads();
    if (!m) return;
    u32 pos = blk_off[blockIdx.x] + (u32)__popcll(ms & ((1ull << lane) - 1ull));
    for (u32 k = 0; k < wave; k++) pos += wave_cnt[k];
    list[pos] = i;
}

// the listed lanes -> compact buffers: signature (81 B, thread t copies byte t % 81 of list entry t / 81), challenge
// scalar (32 B) and key index
__global__ void __launch_bounds__(256)
msm_k_screen_gather_list(const u32 *__restrict__ list, u32 m, const u8 *__restrict__ sigs, const u64 *__restrict__ h,
                         const u32 *__restrict__ key_idx, u8 *__restrict__ g_sigs, u64 *__restrict__ g_h,
                         u32 *__restrict__ g_idx) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (size_t)m * 81) return;
    const u32 c = (u32)(t / 81), k = (u32)(t % 81);
    const size_t src = list[c];
    g_sigs[t] = sigs[81 * src + k];
    if (k < 4) g_h[4 * (size_t)c + k] = h[4 * src + k];
    else if (k == 4) g_idx[c] = key_idx[src];
}

// compact statuses -> the listed lanes
__global__ void __launch_bounds__(256)
msm_k_screen_scatter_list(const u32 *__restrict__ list, u32 m, const u8 *__restrict__ g_status, u8 *__restrict__ status) {
    const u32 c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c < m) status[list[c]] = g_status[c];
}

// ---- small batches: Straus on cooperating waves ---------------------------------------------------
// The bucket method pays ~20 launches of lone, latency-bound waves however small the batch is (2.5 ms at the
// reference's own bench sizes, benches/schnorr.rs:78-96: 4..128 signatures).  Below MSM_SMALL_MAX signatures the
// same equation is evaluated term by term instead: ONE two-wave block per signature computes
//     T_i = [s_i] R_i - [s_i h_i] P_i      and      s_i e_i mod q
// with the wave-cooperative arithmetic of ssa_coop.hpp (table of eight multiples + signed 4-bit windows for each
// of the two points, the same code as the low-latency verification kernel), and writes them as one 24-word record
// -- the very record a shard of a multi-process batch produces (include/schnorr_sig_amd.h), so the records are summed
// by the same combination kernel.
//   wave 0: stage, P on the curve, table of P      ||  wave 1: hash_message -> h, s h mod q, s e mod q
//   wave 0: decompress R, table of R, [s] R        ||  wave 1: [s h] P from P's table, negate
//   wave 0: T = [s]R + (-[s h]P), record
struct MsmSmallShared {
    u32 ok, r_ok, r_inf;
    u64 s[4], b[4], se[4];
};

__global__ void __launch_bounds__(128)
msm_k_small(const DevParams *__restrict__ prm, const u8 *__restrict__ sigs, const u8 *__restrict__ pks,
            const u8 *__restrict__ pk_inf, MsgView mv, const u8 *__restrict__ coeffs, u32 coeff_bytes, size_t n,
            u64 *__restrict__ records) {
    __shared__ CoopLds L;
    __shared__ MsmSmallShared sh;
    using namespace coop_slots;
    const size_t i = blockIdx.x;
    if (i >= n) return;
    const u32 lane = threadIdx.x & 63u;
    const int ws = (int)(threadIdx.x >> 6);
    COOP_WORKING_SET(ws);
    int t[9];
#pragma unroll
    for (int k = 0; k < 9; k++) t[k] = T0 + k;
    const u8 *sig = sigs + 81 * i, *pk = pks + 96 * i;
    const bool inf = pk_inf && pk_inf[i];
    u64 *rec = records + 24 * i;
    u32 len;
    const u8 *m = msg_ptr(mv, i, len);
    const sc256 e = ld_sc(sig + 49);
    if (ws == 0) {   // stage the inputs, canonical-limb checks (the reference panics on these: src/batch.rs:67,104)
        bool ok = true;
        if (lane < 12) {
            const u32 c = lane % 6u;
            const u64 xs = ld_u64_le(sig + 8 * c), px = ld_u64_le(pk + 8 * c), py = ld_u64_le(pk + 48 + 8 * c);
            coop_store7(L, SX, xs, lane);
            coop_store7(L, PX, px, lane);
            coop_store7(L, PY, py, lane);
            ok = px < FP_P && py < FP_P && xs < FP_P;
        }
        ok = __all(ok) && !sc_geq_q(e);
        if (lane == 0) {
            sh.ok = ok;
            sh.r_ok = 0;
            sh.r_inf = 0;
        }
    }
    __syncthreads();
    // wave 0's share of R: decompression (one lane: the Fp6 square root is a long serial chain either way) and the
    // table of its multiples.  With 128-bit coefficients [s]R is half a ladder and all of this fits beside wave 1's
    // [s h]P; with full-width coefficients (a shim passing Scalar::random) both ladders are equally long and R's table
    // is built BEFORE the first barrier instead, beside wave 1's hash.
    const bool wide = coeff_bytes > 16;
    auto r_tables = [&]() {
        if (lane == 0) {   // R = from_compressed(sig.x).unwrap() (:104)
            aff R;
            bool r_inf = false;
            const u32 st = decompress_lane(sig, R, r_inf);
            sh.r_ok = st == 0;
            sh.r_inf = r_inf;
#pragma unroll
            for (int c = 0; c < 6; c++) {
                L.slot[RX][c] = R.x.c[c];
                L.slot[RX][6 + c] = fp_mul_small(R.x.c[c], 7u);
                L.slot[RY][c] = R.y.c[c];
                L.slot[RY][6 + c] = fp_mul_small(R.y.c[c], 7u);
            }
        }
        coop_sync();
        if (sh.r_ok) coop_build_table(L, sh.r_inf != 0, lane, ws, TAB2, RX, RY);   // (lane 0 wrote it before the fence)
    };
    if (ws == 0) {
        bool ok = sh.ok != 0;
        if (ok && !inf) {   // y^2 == x^3 + x + (u + 395)
            coop_mul(L, T0, PX, PX, lane, ws);
            coop_mul(L, T0, T0, PX, lane, ws);
            coop_add(L, T0, T0, PX, lane, ws);
            if (lane < 2) L.slot[T0][lane] = fp_add(L.slot[T0][lane], lane == 0 ? 395ull : 1ull);   // compared only
            coop_sync();
            coop_mul(L, T0 + 1, PY, PY, lane, ws);
            ok = coop_eq(L, T0, T0 + 1, lane, ws);
        }
        if (lane == 0) sh.ok = ok;
        if (ok) {
            coop_build_table(L, inf, lane, ws);
            if (wide) r_tables();
        }
    } else {
        const sc256 h = coop_hash_message(L, prm, m, len, lane, ws);   // reads SX, PX, PY only; h_i, src/batch.rs:64-73
        if (lane == 0) {
            sc256 s;
#pragma unroll
            for (int k = 0; k < 4; k++) s.w[k] = 0;
            const u8 *cp = coeffs + (size_t)coeff_bytes * i;
            for (u32 b = 0; b < coeff_bytes; b++) s.w[b >> 3] |= (u64)cp[b] << (8 * (b & 7u));
            s = sc_reduce256(s);                                       // Scalar::random, :75-78
            const sc256 sb = sc_mul_mod(s, h), se = sc_mul_mod(s, e);  // :109-111, :92-97
#pragma unroll
            for (int k = 0; k < 4; k++) {
                sh.s[k] = s.w[k];
                sh.b[k] = sb.w[k];
                sh.se[k] = se.w[k];
            }
        }
    }
    __syncthreads();
    if (!sh.ok) {   // block-uniform
        msm_record_flag(rec, true);
        return;
    }
    if (ws == 0) {
        if (!wide) r_tables();
        if (sh.r_ok) {
            sc256 s;
#pragma unroll
            for (int k = 0; k < 4; k++) s.w[k] = sh.s[k];
            coop_mul_table(L, s, lane, ws, TAB2);                           // [s_i] R_i
        }
    } else {
        sc256 b;
#pragma unroll
        for (int k = 0; k < 4; k++) b.w[k] = sh.b[k];
        coop_mul_table(L, b, lane, ws);                                     // [s_i h_i] P_i  (the identity for an identity key)
        coop_neg(L, AY, AY, lane, ws);                                      // k.0.neg(), :106
    }
    __syncthreads();
    if (!sh.r_ok) {
        msm_record_flag(rec, true);
        return;
    }
    if (ws == 0) {
        // wave 1's accumulator as the second operand (X, Y, Z with their 7x halves) in this wave's I0..I2
        if (lane < 18) {
            const u32 v = lane / 6u, c = lane % 6u;
            const u64 w = L.slot[WS_SLOTS + (int)v][c];
            L.slot[I0 + (int)v][c] = w;
            L.slot[I0 + (int)v][6 + c] = fp_mul_small(w, 7u);
        }
        coop_sync();
        coop_jac_add(L, AX, I0, t, lane, ws);
        if (lane < 18) rec[lane] = fp_canon(L.slot[AX + (int)(lane / 6u)][lane % 6u]);
        else if (lane < 22) rec[lane] = sh.se[lane - 18u];
        else if (lane == 22) rec[lane] = 0ull;
        else if (lane == 23) rec[lane] = SSA_MSM_RECORD_MAGIC;
    }
}

// records [lo, hi) of `in` (lo < hi) -> one record at rec, by ONE wave: the points by cooperative general additions, the
// scalars mod q, the malformed flags OR-ed
SSA_DEV void sum_records_range(CoopLds &L, const u64 *__restrict__ in, u32 lo, u32 hi, u64 *__restrict__ rec) {
    const u32 lane = threadIdx.x;
    int t[9];
#pragma unroll
    for (int k = 0; k < 9; k++) t[k] = 7 + k;
    bool bad = false;
    sc256 lin;
#pragma unroll
    for (int k = 0; k < 4; k++) lin.w[k] = 0;
    // accumulator 0..3 (X, Y, Z, W = Z^4), addend 4..6.  The loop of coop_sum_points with dbl = 0, spelled out: it also
    // folds each record's scalar and flag, and through the helper the kernels were 1 % slower (profiles/r17/README.md)
    coop_load_jac(L, 0, in + 24 * (size_t)lo, lane);
    coop_mul(L, 3, 2, 2, lane, 0);
    coop_mul(L, 3, 3, 3, lane, 0);
#pragma unroll 1
    for (u32 j = lo; j < hi; j++) {
        bad = bad || in[24 * (size_t)j + 22] != 0;
        sc256 p;
#pragma unroll
        for (int k = 0; k < 4; k++) p.w[k] = in[24 * (size_t)j + 18 + k];
        lin = sc_add_mod(lin, p);
        if (j > lo) {
            coop_load_jac(L, 4, in + 24 * (size_t)j, lane);
            coop_jac_add(L, 0, 4, t, lane, 0);
        }
    }
    if (lane < 18) rec[lane] = bad ? 0ull : fp_canon(L.slot[(int)(lane / 6u)][lane % 6u]);
    else if (lane < 22) rec[lane] = lin.w[lane - 18u];
    else if (lane == 22) rec[lane] = bad ? 1ull : 0ull;
    else if (lane == 23) rec[lane] = SSA_MSM_RECORD_MAGIC;
}

// records [g * group, (g + 1) * group) -> one record (one wave per group)
__global__ void __launch_bounds__(64)
msm_k_sum_records(const u64 *__restrict__ in, u32 count, u32 group, u64 *__restrict__ out) {
    __shared__ CoopLds L;
    const u32 g = blockIdx.x;
    const u32 lo = g * group, hi = lo + group < count ? lo + group : count;
    if (lo >= hi) return;
    sum_records_range(L, in, lo, hi, out + 24 * (size_t)g);
}

// The segmented form (ssa_verify_aggregates_many's small path): wave s adds the contiguous records of aggregate
// agg0 + s -- lanes [first[agg0 + s], first[agg0 + s + 1]) of the call, `in` starting at lane first[agg0] -- into out[s];
// an aggregate without lanes gets the record of an empty shard.
__global__ void __launch_bounds__(64)
msm_k_sum_records_seg(const u64 *__restrict__ in, const u32 *__restrict__ first, u32 agg0, u64 *__restrict__ out) {
    __shared__ CoopLds L;
    const u32 j = agg0 + blockIdx.x, lo = first[j] - first[agg0], hi = first[j + 1] - first[agg0];
    u64 *rec = out + 24 * (size_t)blockIdx.x;
    if (lo >= hi) {                                   // (block-uniform)
        msm_record_flag(rec, false);
        return;
    }
    sum_records_range(L, in, lo, hi, rec);
}

// the record of an empty shard
__global__ void msm_k_empty_record(u64 *__restrict__ rec) { msm_record_flag(rec, false); }

}  // namespace ssa

// ------------------------------------------------------------------------------------------------
static MsmShape msm_shape(size_t n) {
    // Window width: 16 bits, or 8 for small batches.  Both divide 128 (library-drawn coefficients) and
    // leave a wide top window for 255-bit scalars (255 mod 16 = 15, 255 mod 8 = 7): a narrow partial
    // window would have a handful of digits and therefore a handful of enormous buckets (measured:
    // c = 14 put n/4 points into single lanes and took 0.9 s at n = 2^18).  Signed digits (round 4): 2^(c-1)
    // buckets per window, and the top window's c - 1 bits absorb the last carry.
    MsmShape sh;
    sh.c = n >= 4096 ? 16u : 8u;
    sh.windows = (255 + sh.c - 1) / sh.c;
    sh.buckets = 1u << (sh.c - 1);
    sh.chunks = sh.buckets <= (u32)MSM_CHUNK ? 1u : sh.buckets / (u32)MSM_CHUNK;
    return sh;
}

// n_blocks 64-byte ChaCha20 blocks into d_out (device), on the context's stream
static int msm_chacha20(ssa_ctx *ctx, const uint8_t key[32], const uint8_t nonce[12], uint32_t counter0,
                        size_t n_blocks, void *d_out) {
    ChaChaKey kn;
    memcpy(kn.key, key, 32);
    memcpy(kn.nonce, nonce, 12);
    if (n_blocks == 0) return 0;
    hipLaunchKernelGGL(msm_k_chacha20, dim3(grid_for(n_blocks, 256)), dim3(256), 0, ctx->stream, kn, counter0, n_blocks,
                       (u32 *)d_out);
    HIP_TRY(hipGetLastError());
    return 0;
}

// fresh 128-bit coefficients for n signatures in ctx->st_coeffs (device)
static int msm_draw_coefficients(ssa_ctx *ctx, size_t n, const void **d_out) {
    uint8_t seed[44];
    size_t got = 0;
    while (got < sizeof seed) {
        ssize_t r = getrandom(seed + got, sizeof seed - got, 0);
        if (r <= 0) return SSA_ERR_ARG;
        got += (size_t)r;
    }
    const size_t n_blocks = (n * 16 + 63) / 64;
    if (ctx->st_coeffs.reserve(n_blocks * 64)) return SSA_ERR_HIP;
    if (int rc = msm_chacha20(ctx, seed, seed + 32, 0u, n_blocks, ctx->st_coeffs.p)) return rc;
    *d_out = ctx->st_coeffs.p;
    return 0;
}

extern "C" int ssa_debug_chacha20(ssa_ctx *ctx, const uint8_t key[32], const uint8_t nonce[12], uint32_t counter0,
                                  size_t n_blocks, uint8_t *out) {
    if (!ctx || !key || !nonce || (n_blocks && !out)) return SSA_ERR_ARG;
    HostCall hc(ctx);
    u8 *d_out = hc.out(ctx->st_coeffs, out, n_blocks * 64, 64);
    return hc.finish([&] { return msm_chacha20(ctx, key, nonce, counter0, n_blocks, d_out); });
}

namespace ssa {
// k partial records (24-word stride) -> the layout msm_k_finish reads: k points of 18 words, k scalars of 4 words, and
// the OR of the malformed flags
__global__ void msm_k_unpack_parts(const u64 *__restrict__ parts, u32 k, u64 *__restrict__ pts, u64 *__restrict__ lins,
                                   u32 *__restrict__ malformed) {
    const u32 t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= k * 24u) return;
    const u32 j = t / 24u, w = t % 24u;
    const u64 v = parts[t];
    if (w < 18) {
        pts[18u * j + w] = v;
        if (v >= FP_P) atomicOr(malformed, 1u);                 // limbs of a record are canonical
    } else if (w < 22) {
        lins[4u * j + (w - 18u)] = v;
    } else if (w == 22) {
        if (v != 0) atomicOr(malformed, 1u);
    } else if (v != SSA_MSM_RECORD_MAGIC) {
        atomicOr(malformed, 1u);   // not a record of this format: never written (all zero), foreign version, garbled
    }
}

// One lane per record: the scalar is canonical (< q) and the point is the identity (Z = 0) or satisfies the Jacobian
// curve equation Y^2 = X^3 + X Z^4 + (u + 395) Z^6.  Records cross process boundaries (all-gather): a corrupted or
// foreign one gives SSA_MALFORMED, never an arbitrary verdict.  k <= 4096: the cost is one short launch.
SSA_DEV bool msm_record_valid(const u64 *__restrict__ r) {
    bool ok = true;
    fp6 X, Y, Z;
#pragma unroll
    for (int c = 0; c < 6; c++) {
        X.c[c] = r[c];
        Y.c[c] = r[6 + c];
        Z.c[c] = r[12 + c];
        ok = ok && X.c[c] < FP_P && Y.c[c] < FP_P && Z.c[c] < FP_P;
    }
    sc256 lin;
#pragma unroll
    for (int c = 0; c < 4; c++) lin.w[c] = r[18 + c];
    ok = ok && !sc_geq_q(lin);
    if (ok && !f6_is_zero(Z)) {
        const fp6 z2 = f6_sqr(Z), z4 = f6_sqr(z2), z6 = f6_mul(z4, z2);
        fp6 b = f6_zero();
        b.c[0] = 395ull;
        b.c[1] = 1ull;
        const fp6 rhs = f6_add(f6_add(f6_mul(f6_sqr(X), X), f6_mul(X, z4)), f6_mul(b, z6));
        ok = f6_eq(f6_sqr(Y), rhs);
    }
    return ok;
}
__global__ void __launch_bounds__(64)
msm_k_check_parts(const u64 *__restrict__ parts, u32 k, u32 *__restrict__ malformed) {
    const u32 j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= k) return;
    if (!msm_record_valid(parts + 24u * (size_t)j)) atomicOr(malformed, 1u);
}

// ONE wave: k records that crossed a process or device boundary -> their sum as one record (the shards of a
// half-aggregate, DESIGN.md section 25: the sum is compared exactly by ag_k_finish, not x-only by msm_k_finish).  Fails
// closed as msm_k_unpack_parts and msm_k_check_parts do together: a record without the magic word, with a set malformed
// word, a non-canonical limb or scalar or a point off the curve leaves the malformed record.
__global__ void __launch_bounds__(64)
msm_k_sum_records_checked(const u64 *__restrict__ in, u32 k, u64 *__restrict__ rec) {
    __shared__ CoopLds L;
    bool ok = true;
    for (u32 j = threadIdx.x; j < k; j += 64u) {
        const u64 *r = in + 24u * (size_t)j;
        ok = ok && r[22] == 0 && r[23] == SSA_MSM_RECORD_MAGIC && msm_record_valid(r);
    }
    if (__ballot(!ok) != 0ull) {                      // (wave-uniform)
        msm_record_flag(rec, true);
        return;
    }
    sum_records_range(L, in, 0u, k, rec);
}
}  // namespace ssa

// The shards added up on one device: one Jacobian addition per shard, the scalars mod q, [lin]G from the comb table and
// the x-only comparison (src/batch.rs:98-100,123-129) -- msm_k_finish with no doublings between its "windows".
// check_points: the records come from outside this call (ssa_msm_combine*): scalars and points are validated too
static int msm_combine_records(ssa_ctx *ctx, const u64 *d_records, size_t k, uint32_t *d_verdict_out, u64 *d_partial_out,
                               bool check_points = false) {
    if (ctx->msm_comb_pts.reserve(18 * k * sizeof(u64)) || ctx->msm_comb_lins.reserve(4 * k * sizeof(u64)) ||
        ctx->msm_flags.reserve(64))
        return SSA_ERR_HIP;
    HIP_TRY(hipMemsetAsync(ctx->msm_flags.p, 0, 64, ctx->stream));
    hipLaunchKernelGGL(msm_k_unpack_parts, dim3(grid_for(k * 24, 256)), dim3(256), 0, ctx->stream, d_records, (u32)k,
                       (u64 *)ctx->msm_comb_pts.p, (u64 *)ctx->msm_comb_lins.p, (u32 *)ctx->msm_flags.p);
    HIP_TRY(hipGetLastError());
    if (check_points) {
        hipLaunchKernelGGL(msm_k_check_parts, dim3(grid_for(k, 64)), dim3(64), 0, ctx->stream, d_records, (u32)k,
                           (u32 *)ctx->msm_flags.p);
        HIP_TRY(hipGetLastError());
    }
    MsmShape sh;
    sh.c = 0;
    sh.windows = (u32)k;
    sh.buckets = 1;
    sh.chunks = 1;
    return timed_launch(ctx, "msm_combine", [&] {
        hipLaunchKernelGGL(msm_k_finish, dim3(1), dim3(128), 0, ctx->stream, (const u64 *)ctx->msm_comb_pts.p, sh,
                           (const u64 *)ctx->msm_comb_lins.p, (u32)k, (const u64 *)ctx->d_gtab,
                           (const u32 *)ctx->msm_flags.p, d_verdict_out, d_partial_out);
    });
}

extern "C" int ssa_msm_combine_device(ssa_ctx *ctx, const uint64_t *d_parts24, size_t k, uint32_t *d_verdict_out) {
    if (!ctx || !d_parts24 || !d_verdict_out || k == 0 || k > 4096) return SSA_ERR_ARG;
    HIP_TRY(hipSetDevice(ctx->device));
    return msm_combine_records(ctx, (const u64 *)d_parts24, k, d_verdict_out, nullptr, true);
}

extern "C" int ssa_msm_combine(ssa_ctx *ctx, const uint64_t *parts24, size_t k) {
    if (!ctx || !parts24 || k == 0 || k > 4096) return SSA_ERR_ARG;
    HostCall hc(ctx);
    const uint64_t *d_parts = hc.in<uint64_t>(ctx->st_aux, parts24, k * SSA_MSM_PARTIAL_WORDS * sizeof(uint64_t));
    uint32_t v = SSA_MALFORMED, *d_verdict = (uint32_t *)((char *)ctx->ws_fail.p + 32);
    hc.copy_back(&v, d_verdict, sizeof v);
    const int rc = hc.finish([&] { return ssa_msm_combine_device(ctx, d_parts, k, d_verdict); });
    return rc ? rc : (int)v;
}

// the screened form: segments of the slice, per-lane status out, one verdict byte per segment
struct ScreenArgs {
    u32 segs, seg_blocks;
    u8 *status, *seg_ok;
    // ssa_verify_many_screened only (null in ssa_verify_batch_screened): lanes to leave out of the sums, and where
    // msm_k_prepare marks them and its own decode failures for the exact re-check instead of writing a status
    const u8 *lane_mask = nullptr;
    u8 *recheck = nullptr;
    // ssa_verify_aggregates_many only: 32 bytes per segment, the right-hand scalar of its comparison
    const u8 *rhs = nullptr;
};
constexpr u32 SCREEN_C = 8;                 // window bits: K * 2^(c-1) <= 256 * 128 stays within the grouping grid
static MsmShape screen_shape(u32 segs) {
    MsmShape sh;
    sh.c = SCREEN_C;
    sh.windows = (255 + sh.c - 1) / sh.c;
    sh.buckets = segs << (sh.c - 1);
    sh.chunks = sh.buckets / (u32)MSM_CHUNK;
    return sh;
}

// Small batch (n <= ctx->knobs.msm_small_max): one cooperative block per signature, then the records are summed -- in
// groups of 16 by one wave each while there are more than 16 of them, the rest by the combination kernel, which also
// computes [sum s_i e_i] G and compares (or emits the shard's record).
static int msm_run_small(ssa_ctx *ctx, const DevBatch &b, size_t n, const uint8_t *d_coeffs, uint32_t coeff_bytes,
                         uint32_t *d_verdict_out, u64 *d_partial_out) {
    const size_t groups = (n + 15) / 16;
    if (ctx->msm_buckets.reserve(n * 24 * sizeof(u64)) || ctx->msm_chunks.reserve(groups * 24 * sizeof(u64)) ||
        ctx->msm_windows.reserve(groups * 24 * sizeof(u64)))
        return SSA_ERR_HIP;
    int rc = timed_launch(ctx, "msm_k_small", [&] {
        hipLaunchKernelGGL(msm_k_small, dim3((unsigned)n), dim3(128), 0, ctx->stream, ctx->d_params, b.sigs, b.pks, b.pk_inf,
                           b.msgs, d_coeffs, coeff_bytes, n, (u64 *)ctx->msm_buckets.p);
    });
    if (rc) return rc;
    const u64 *recs = (const u64 *)ctx->msm_buckets.p;
    size_t count = n;
    u64 *ping = (u64 *)ctx->msm_chunks.p, *pong = (u64 *)ctx->msm_windows.p;
    while (count > 16) {     // the combination kernel adds its records one after the other: hand it at most 16
        const size_t g = (count + 15) / 16;
        hipLaunchKernelGGL(msm_k_sum_records, dim3((unsigned)g), dim3(64), 0, ctx->stream, recs, (u32)count, 16u, ping);
        HIP_TRY(hipGetLastError());
        recs = ping;
        u64 *tmp = ping;
        ping = pong;
        pong = tmp;
        count = g;
    }
    return msm_combine_records(ctx, recs, count, d_verdict_out, d_partial_out);
}

// One slice of the bucket pipeline on ctx->stream, with the stage that fills it handed in: `fill` enqueues whatever writes
// the 2n point rows (R_i at i, -P_i at n + i), the signed digits (window-major; the R's over their lowest wa windows, the
// keys over all), the per-workgroup partial sums of s_i e_i and the malformed word of the flags (zeroed here, in front of
// it); then sort, buckets and reduce run over them.  msm_run_one's preparation is one such stage, the streaming aggregate
// verifier's agv_k_scalars (ssa_api.hip) the other.
static int msm_run_prepared(ssa_ctx *ctx, size_t n, const MsmShape &sh, u32 wa, uint32_t *d_verdict_out, u64 *d_partial_out,
                            const ScreenArgs *scr, const MsmFillFn &fill) {
    MsmItems it;
    it.n = (u32)n;
    it.wa = wa;
    it.windows = sh.windows;
    it.seg_blocks = scr ? scr->seg_blocks : 0u;
    it.cm1 = sh.c - 1;
    it.tile0[0] = it.base[0] = 0;
    for (u32 j = 0; j < sh.windows; j++) {
        const size_t items = j < wa ? 2 * n : n;
        it.tile0[j + 1] = it.tile0[j] + (u32)((items + MSM_TILE - 1) / MSM_TILE);
        it.base[j + 1] = it.base[j] + (u32)items;
    }
    const u32 n_tiles = it.tile0[sh.windows], tmax = (u32)((2 * n + MSM_TILE - 1) / MSM_TILE);
    const size_t npts = 2 * n, total = it.base[sh.windows], nb = (size_t)sh.windows * sh.buckets;
    const unsigned n_blocks = grid_for(n, 256);
    if (ctx->msm_points.reserve(npts * 96) ||
        ctx->msm_scalars.reserve(npts * sh.windows * sizeof(short)) ||                 // signed digits, window-major
        ctx->msm_keys.reserve((size_t)sh.windows * MSM_HI_BINS * tmax * 4) ||          // per-tile group counts / positions
        ctx->msm_vals.reserve(total * 4) ||                                            // items by group: point | low bits | sign
        ctx->msm_keys2.reserve((size_t)sh.windows * MSM_HI_BINS * 4) ||                // row totals of the scan
        ctx->msm_ids.reserve(2048 * 4) ||                                              // size classes: counts, first ranks
        ctx->msm_vals2.reserve(total * 4) ||                                           // items by bucket
        ctx->msm_bounds.reserve(nb * 4) || ctx->msm_cnt.reserve(nb * 4) ||             // bucket extents
        ctx->msm_ids2.reserve((nb + 1024) * 4) ||                                      // buckets in order of size
        ctx->msm_cnt2.reserve((size_t)sh.windows * (MSM_HI_BINS + 1) * 4) ||           // group extents
        ctx->msm_buckets.reserve(nb * 144) ||
        ctx->msm_chunks.reserve((size_t)sh.windows * sh.chunks * 144) ||
        ctx->msm_windows.reserve((size_t)sh.windows * sh.chunks * 144) ||
        ctx->msm_partials.reserve((size_t)n_blocks * 32) || ctx->msm_flags.reserve(64))
        return SSA_ERR_HIP;
    HIP_TRY(hipMemsetAsync(ctx->msm_flags.p, 0, 64, ctx->stream));
    int rc = fill({sh, wa, n, n_blocks, (u64 *)ctx->msm_points.p, (short *)ctx->msm_scalars.p, (u64 *)ctx->msm_partials.p,
                   (u32 *)ctx->msm_flags.p});
    if (rc) return rc;
    rc = timed_launch(ctx, "msm_sort", [&] {
        hipLaunchKernelGGL(scr ? msm_k_hist_seg : msm_k_hist, dim3(n_tiles), dim3(256), 0, ctx->stream,
                           (const short *)ctx->msm_scalars.p, it, tmax, (u32 *)ctx->msm_keys.p);
        hipLaunchKernelGGL(msm_k_rowsum, dim3(sh.windows * MSM_HI_BINS), dim3(64), 0, ctx->stream, it, tmax,
                           (const u32 *)ctx->msm_keys.p, (u32 *)ctx->msm_keys2.p);
        hipLaunchKernelGGL(msm_k_rowscan, dim3(sh.windows * MSM_HI_BINS), dim3(256), 0, ctx->stream, it, tmax,
                           (const u32 *)ctx->msm_keys2.p, (u32 *)ctx->msm_keys.p, (u32 *)ctx->msm_cnt2.p);
        hipLaunchKernelGGL(scr ? msm_k_scatter_seg : msm_k_scatter, dim3(n_tiles), dim3(256), 0, ctx->stream,
                           (const short *)ctx->msm_scalars.p, it, tmax, (const u32 *)ctx->msm_keys.p, (u32 *)ctx->msm_vals.p);
        hipLaunchKernelGGL(msm_k_group, dim3(sh.windows * MSM_HI_BINS), dim3(256), 0, ctx->stream,
                           (const u32 *)ctx->msm_cnt2.p, (const u32 *)ctx->msm_vals.p, sh, (u32 *)ctx->msm_vals2.p,
                           (u32 *)ctx->msm_bounds.p, (u32 *)ctx->msm_cnt.p);
    });
    if (rc) return rc;
    rc = timed_launch(ctx, "msm_k_buckets", [&] {
        u32 *ghist = (u32 *)ctx->msm_ids.p, *gcur = ghist + 1024;
        (void)hipMemsetAsync(ghist, 0, 1024 * 4, ctx->stream);
        hipLaunchKernelGGL(msm_k_sizes, dim3(grid_for(nb, 1024)), dim3(1024), 0, ctx->stream, (const u32 *)ctx->msm_cnt.p,
                           (u32)nb, ghist);
        hipLaunchKernelGGL(msm_k_size_ranks, dim3(1), dim3(1024), 0, ctx->stream, (const u32 *)ghist, gcur);
        hipLaunchKernelGGL(msm_k_order, dim3(grid_for(nb, 1024)), dim3(1024), 0, ctx->stream, (const u32 *)ctx->msm_cnt.p,
                           (u32)nb, gcur, (u32 *)ctx->msm_ids2.p);
        hipLaunchKernelGGL(msm_k_buckets, dim3(grid_for(nb, 256)), dim3(256), 0, ctx->stream,
                           (const u64 *)ctx->msm_points.p, (const u32 *)ctx->msm_vals2.p,
                           (const u32 *)ctx->msm_bounds.p, (const u32 *)ctx->msm_cnt.p, (const u32 *)ctx->msm_ids2.p, nb,
                           (u64 *)ctx->msm_buckets.p);
    });
    if (rc) return rc;
    // per window (and segment): running sums on chunks of MSM_CHUNK buckets, a tree over the chunk sums, then one
    // cooperative block (per segment): Horner over the windows || [lin]G, and the comparison
    // (screened: a window's chunks are `segs` runs of 2^(c-1) / MSM_CHUNK, the tree reduces each run on its own)
    const u32 runs = scr ? scr->segs : 1u;
    u64 *ping = (u64 *)ctx->msm_chunks.p, *pong = (u64 *)ctx->msm_windows.p;
    rc = timed_launch(ctx, "msm_reduce", [&] {
        hipLaunchKernelGGL(scr ? msm_k_chunks_seg : msm_k_chunks, dim3(grid_for((size_t)sh.windows * sh.chunks, 256)),
                           dim3(256), 0, ctx->stream, (const u64 *)ctx->msm_buckets.p, sh, (u64 *)ctx->msm_chunks.p);
        u32 count = sh.chunks / runs;
        while (count > 1) {
            const u32 groups = (count + ctx->knobs.msm_tree_group - 1) / ctx->knobs.msm_tree_group;
            hipLaunchKernelGGL(msm_k_tree, dim3(sh.windows * runs * groups), dim3(64), 0, ctx->stream,
                               (const u64 *)ping, sh.windows * runs, count, ctx->knobs.msm_tree_group, pong);
            u64 *tmp = ping;
            ping = pong;
            pong = tmp;
            count = groups;
        }
        if (!scr)
            hipLaunchKernelGGL(msm_k_finish, dim3(1), dim3(128), 0, ctx->stream, (const u64 *)ping, sh,
                               (const u64 *)ctx->msm_partials.p, n_blocks, (const u64 *)ctx->d_gtab,
                               (const u32 *)ctx->msm_flags.p, d_verdict_out, d_partial_out);
    });
    if (rc || !scr) return rc;
    return timed_launch(ctx, "msm_k_finish_seg", [&] {
        hipLaunchKernelGGL(msm_k_finish_seg, dim3(scr->segs), dim3(128), 0, ctx->stream, (const u64 *)ping, sh, scr->segs,
                           scr->seg_blocks, (const u64 *)ctx->msm_partials.p, n_blocks, (const u64 *)ctx->d_gtab,
                           scr->seg_ok, scr->rhs);
    });
}

// the kernels of one MSM-form slice on ctx->stream: a verdict (d_partial_out == nullptr) or the slice's / shard's record
// d_h: the challenge scalars if they exist already, else nullptr (they are computed into ctx->ws_h)
// scr != nullptr: the screened form -- (window, segment, digit) buckets, a per-lane status, one verdict per segment in
// scr->seg_ok (no verdict, no record)
static int msm_run_one(ssa_ctx *ctx, const DevBatch &b, size_t n, const uint8_t *d_coeffs, uint32_t coeff_bytes,
                       uint32_t *d_verdict_out, u64 *d_partial_out, const u64 *d_h, const ScreenArgs *scr = nullptr) {
    if (n > (1ull << 23)) return SSA_ERR_ARG;   // an item carries its point index in 24 bits: 2n <= 2^24 (msm_run slices)
    if (n == 0) {   // empty batch: Ok (src/batch.rs); an empty shard adds the identity and 0
        if (d_partial_out) {
            hipLaunchKernelGGL(msm_k_empty_record, dim3(1), dim3(64), 0, ctx->stream, d_partial_out);
            HIP_TRY(hipGetLastError());
            return 0;
        }
        HIP_TRY(hipMemsetAsync(d_verdict_out, 0, sizeof(uint32_t), ctx->stream));
        return 0;
    }
    if (!d_coeffs) {   // Scalar::random(rng): the library draws 128-bit coefficients
        const void *p;
        if (int rc = msm_draw_coefficients(ctx, n, &p)) return rc;
        d_coeffs = (const uint8_t *)p;
        coeff_bytes = 16;
    }
    if (!scr && n <= ctx->knobs.msm_small_max)
        return msm_run_small(ctx, b, n, d_coeffs, coeff_bytes, d_verdict_out, d_partial_out);
    const MsmShape sh = scr ? screen_shape(scr->segs) : msm_shape(n);
    // windows the coefficients themselves can reach (32-byte ones are reduced mod q: all of them).  A narrower coefficient
    // whose width is a whole number of windows is read as a TWO'S-COMPLEMENT integer (msm_k_prepare): its signed digits
    // then need no carry window -- which would hold the digit 1 for half of the points, one enormous bucket -- and a
    // random coefficient is as good signed as unsigned (the same value multiplies R_i, h_i and e_i).
    const u32 wa = coeff_bytes >= 32 ? sh.windows : (8u * coeff_bytes + sh.c - 1) / sh.c;
    if (!d_h && ctx->ws_h.reserve(n * 32)) return SSA_ERR_HIP;
    const unsigned n_blocks = grid_for(n, 256);
    return msm_run_prepared(ctx, n, sh, wa, d_verdict_out, d_partial_out, scr, [&](const MsmFill &) -> int {
        int rc = 0;
        if (!d_h && ctx->knobs.msm_overlap) {
            // The challenge hashes are 62 % of this form and nothing but the digits of s_i h_i needs them: the rest of the
            // preparation (R's square roots above all) runs on a second stream UNDER ssa_k_hash -- its waves fill the hash
            // kernel's tail (the last wave of every SIMD alone, 0.35 ms) and the hash fills theirs --, ctx->stream joins it
            // after the hash and writes the digits that were missing.
            // Until msm_k_prepare_h is queued behind it, an error return waits for msm_k_prepare: it writes msm_points,
            // msm_scalars, msm_sbuf and msm_flags.
            if (ctx->msm_sbuf.reserve(n * 32)) return SSA_ERR_HIP;
            hipStream_t side = ctx->hash_stream[0];
            HIP_TRY(hipEventRecord(ctx->pipe_start, ctx->stream));
            HIP_TRY(hipStreamWaitEvent(side, ctx->pipe_start, 0));
            SideStreamDrain drain{ctx};
            hipLaunchKernelGGL(msm_k_prepare, dim3(n_blocks), dim3(256), 0, side, b.sigs, b.pks, b.pk_inf,
                               (const u64 *)nullptr, d_coeffs, coeff_bytes, n, sh, wa, (u64 *)ctx->msm_points.p,
                               (short *)ctx->msm_scalars.p, (u64 *)ctx->msm_partials.p, (u32 *)ctx->msm_flags.p,
                               (u64 *)ctx->msm_sbuf.p, scr ? scr->status : (u8 *)nullptr,
                               scr ? scr->lane_mask : (const u8 *)nullptr, scr ? scr->recheck : (u8 *)nullptr);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipEventRecord(ctx->hash_done[0], side));
            if (int hrc = ssa_internal_hash_scalars(ctx, b, n)) return hrc;
            d_h = (const u64 *)ctx->ws_h.p;
            HIP_TRY(hipStreamWaitEvent(ctx->stream, ctx->hash_done[0], 0));
            rc = timed_launch(ctx, "msm_k_prepare", [&] {
                hipLaunchKernelGGL(msm_k_prepare_h, dim3(n_blocks), dim3(256), 0, ctx->stream, d_h, (const u64 *)ctx->msm_sbuf.p,
                                   n, sh, (short *)ctx->msm_scalars.p);
            });
            if (rc) return rc;
            drain.done();
        } else {
            // challenge scalars h_i with the kernel of the per-lane path
            if (!d_h) {
                if (int hrc = ssa_internal_hash_scalars(ctx, b, n)) return hrc;
                d_h = (const u64 *)ctx->ws_h.p;
            }
            rc = timed_launch(ctx, "msm_k_prepare", [&] {
                hipLaunchKernelGGL(msm_k_prepare, dim3(n_blocks), dim3(256), 0, ctx->stream, b.sigs, b.pks, b.pk_inf,
                                   d_h, d_coeffs, coeff_bytes, n, sh, wa, (u64 *)ctx->msm_points.p,
                                   (short *)ctx->msm_scalars.p, (u64 *)ctx->msm_partials.p, (u32 *)ctx->msm_flags.p,
                                   (u64 *)nullptr, scr ? scr->status : (u8 *)nullptr,
                                   scr ? scr->lane_mask : (const u8 *)nullptr, scr ? scr->recheck : (u8 *)nullptr);
            });
            if (rc) return rc;
        }
        return 0;
    });
}

int ssa_internal_msm_record(ssa_ctx *ctx, const DevBatch &b, size_t n, const uint8_t *d_coeffs, uint32_t coeff_bytes,
                            const uint64_t *d_h, uint64_t *d_record_out) {
    if (!d_coeffs || !d_record_out || n > ctx->knobs.msm_slice) return SSA_ERR_ARG;
    return msm_run_one(ctx, b, n, d_coeffs, coeff_bytes, nullptr, (u64 *)d_record_out, (const u64 *)d_h);
}

// Always the bucket pipeline, whatever n is: msm_k_small hashes and decompresses for itself, which is what the caller of
// this entry has done already.  msm_shape gives 8-bit windows below 4096 lanes, and the grouping passes take any n >= 1
// (contexts with SSA_MSM_SMALL_MAX=0 drive them at n = 1): no floor is needed.
int ssa_internal_msm_record_prepared(ssa_ctx *ctx, size_t n, uint32_t coeff_bytes, const MsmFillFn &fill,
                                     uint64_t *d_record_out) {
    if (!fill || !d_record_out || n == 0 || n > ctx->knobs.msm_slice || n > (1ull << 23) || coeff_bytes == 0 ||
        coeff_bytes >= 32)
        return SSA_ERR_ARG;
    const MsmShape sh = msm_shape(n);
    return msm_run_prepared(ctx, n, sh, (8u * coeff_bytes + sh.c - 1) / sh.c, nullptr, (u64 *)d_record_out, nullptr, fill);
}

int ssa_internal_msm_sum_records(ssa_ctx *ctx, const uint64_t *d_records, size_t k, bool checked, uint64_t *d_record_out) {
    if (!d_records || !d_record_out || k == 0 || k > 4096) return SSA_ERR_ARG;
    return timed_launch(ctx, "msm_k_sum_records", [&] {
        if (checked)
            hipLaunchKernelGGL(msm_k_sum_records_checked, dim3(1), dim3(64), 0, ctx->stream, (const u64 *)d_records, (u32)k,
                               (u64 *)d_record_out);
        else
            hipLaunchKernelGGL(msm_k_sum_records, dim3(1), dim3(64), 0, ctx->stream, (const u64 *)d_records, (u32)k, (u32)k,
                               (u64 *)d_record_out);
    });
}

// The left-hand sides of ssa_verify_aggregates_many (ssa_api.hip), one group of aggregates each.
// Small path: msm_k_small over the n lanes of b (the group's, the transcript's coefficients), then one wave per aggregate
// adds its records: *d_recs_out = `aggs` records, 24 words each.  d_first: the call's prefix sums on the device.
int ssa_internal_msm_agg_small(ssa_ctx *ctx, const DevBatch &b, size_t n, const uint8_t *d_coeffs16, const uint32_t *d_first,
                               uint32_t agg0, uint32_t aggs, const uint64_t **d_recs_out) {
    if (!d_coeffs16 || !d_first || !d_recs_out || aggs == 0) return SSA_ERR_ARG;
    if (ctx->msm_buckets.reserve((n ? n : 1) * 24 * sizeof(u64)) || ctx->msm_chunks.reserve((size_t)aggs * 24 * sizeof(u64)))
        return SSA_ERR_HIP;
    if (n) {
        const int rc = timed_launch(ctx, "msm_k_small", [&] {
            hipLaunchKernelGGL(msm_k_small, dim3((unsigned)n), dim3(128), 0, ctx->stream, ctx->d_params, b.sigs, b.pks,
                               b.pk_inf, b.msgs, d_coeffs16, 16u, n, (u64 *)ctx->msm_buckets.p);
        });
        if (rc) return rc;
    }
    *d_recs_out = (const uint64_t *)ctx->msm_chunks.p;
    return timed_launch(ctx, "msm_k_sum_records_seg", [&] {
        hipLaunchKernelGGL(msm_k_sum_records_seg, dim3(aggs), dim3(64), 0, ctx->stream, (const u64 *)ctx->msm_buckets.p,
                           d_first, agg0, (u64 *)ctx->msm_chunks.p);
    });
}

// Bucket path: b holds segs x seg_lanes padded lanes (seg_lanes a multiple of 256; padding lanes have d_mask 1 and enter
// no sum), d_h and d_coeffs16 their challenge scalars and coefficients.  The screened pipeline keyed by (window, segment,
// digit) leaves in d_seg_ok[s] the exact comparison of segment s with [d_rhs[s]]G, and in d_recheck the lanes that
// msm_k_prepare left out: the padding and every lane that failed one of its checks.
int ssa_internal_msm_agg_segments(ssa_ctx *ctx, const DevBatch &b, uint32_t segs, uint32_t seg_lanes,
                                  const uint8_t *d_coeffs16, const uint64_t *d_h, const uint8_t *d_mask, uint8_t *d_recheck,
                                  const uint8_t *d_rhs, uint8_t *d_seg_ok) {
    if (!d_coeffs16 || !d_h || !d_mask || !d_recheck || !d_rhs || !d_seg_ok) return SSA_ERR_ARG;
    if (segs == 0 || segs > 256u || seg_lanes == 0 || (seg_lanes & 255u)) return SSA_ERR_ARG;
    ScreenArgs sa{segs, seg_lanes / 256u, nullptr, d_seg_ok};
    sa.lane_mask = d_mask;
    sa.recheck = d_recheck;
    sa.rhs = d_rhs;
    return msm_run_one(ctx, b, (size_t)segs * seg_lanes, d_coeffs16, 16, nullptr, nullptr, (const u64 *)d_h, &sa);
}

// A batch of any size (n <= SSA_MAX_BATCH) in bounded memory: more than ctx->knobs.msm_slice signatures run slice after slice,
// every slice reduced to its 24-word record exactly as a shard of a multi-GPU batch is (src/batch.rs:98-129: one point
// and one scalar per part), and the records are added up by the combination kernel -- one point addition per slice.
// hashed: ctx->ws_h already holds the challenge scalars of the WHOLE batch (the host-buffer pipeline computed them).
static int msm_run(ssa_ctx *ctx, const DevBatch &b, size_t n, const uint8_t *d_coeffs, uint32_t coeff_bytes,
                   uint32_t *d_verdict_out, u64 *d_partial_out, bool hashed = false) {
    if (!ctx || (!d_verdict_out && !d_partial_out)) return SSA_ERR_ARG;
    if (n && (!b.sigs || !b.pks)) return SSA_ERR_ARG;
    if (d_coeffs && (coeff_bytes == 0 || coeff_bytes > 32)) return SSA_ERR_ARG;
    if (int rc = check_msgs(b.msgs, n)) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    const u64 *d_h = hashed ? (const u64 *)ctx->ws_h.p : nullptr;
    if (n <= ctx->knobs.msm_slice) return msm_run_one(ctx, b, n, d_coeffs, coeff_bytes, d_verdict_out, d_partial_out, d_h);
    const size_t slice = ctx->knobs.msm_slice, k = (n + slice - 1) / slice;
    if (ctx->msm_slice_recs.reserve(k * 24 * sizeof(u64))) return SSA_ERR_HIP;
    u64 *recs = (u64 *)ctx->msm_slice_recs.p;
    if (int rc = for_dev_slices(b, n, slice, [&](size_t lo, size_t cnt, const DevBatch &s) {
            return msm_run_one(ctx, s, cnt, d_coeffs ? d_coeffs + (size_t)coeff_bytes * lo : nullptr, coeff_bytes, nullptr,
                               recs + 24 * (lo / slice), d_h ? d_h + 4 * lo : nullptr);
        }))
        return rc;
    return msm_combine_records(ctx, recs, k, d_verdict_out, d_partial_out);
}

extern "C" int ssa_verify_batch_msm_device(ssa_ctx *ctx, const uint8_t *d_sigs, const uint8_t *d_pks,
                                           const uint8_t *d_pk_inf, const uint8_t *d_msgs,
                                           const uint64_t *d_msg_off, size_t msg_stride,
                                           size_t msg_len, size_t n, const uint8_t *d_coeffs, uint32_t coeff_bytes,
                                           uint32_t *d_verdict_out) {
    if (!d_verdict_out) return SSA_ERR_ARG;
    return msm_run(ctx, {d_sigs, d_pks, d_pk_inf, {d_msgs, d_msg_off, msg_stride, msg_len}}, n, d_coeffs, coeff_bytes,
                   d_verdict_out, nullptr);
}

// the device-buffer form: what one rank of a process-per-GPU job calls on its shard (the records then travel by
// all-gather, 24 words per rank)
extern "C" int ssa_verify_batch_msm_partial_device(ssa_ctx *ctx, const uint8_t *d_sigs, const uint8_t *d_pks,
                                                   const uint8_t *d_pk_inf, const uint8_t *d_msgs,
                                                   const uint64_t *d_msg_off, size_t msg_stride, size_t msg_len, size_t n,
                                                   const uint8_t *d_coeffs, uint32_t coeff_bytes,
                                                   uint64_t *d_partial_out) {
    if (!d_partial_out) return SSA_ERR_ARG;
    return msm_run(ctx, {d_sigs, d_pks, d_pk_inf, {d_msgs, d_msg_off, msg_stride, msg_len}}, n, d_coeffs, coeff_bytes,
                   nullptr, (u64 *)d_partial_out);
}

// ONE slice (n <= ctx->knobs.msm_slice) from host buffers: the verdict (out24 == nullptr) or the slice's 24-word record
static int msm_host_one(ssa_ctx *ctx, const HostBatch &b, size_t n, const uint8_t *coeffs, int *verdict_out,
                        uint64_t *out24) {
    HostCall hc(ctx);
    uint32_t v = SSA_MALFORMED, *d_verdict = out24 ? nullptr : (uint32_t *)((char *)ctx->ws_fail.p + 32);
    u64 *d_rec = out24 ? (u64 *)hc.out(ctx->st_aux2, nullptr, SSA_MSM_PARTIAL_WORDS * sizeof(u64)) : nullptr;
    // Scalar::random(rng) (src/batch.rs:75-78): caller-supplied 32-byte scalars, or (coeffs == NULL) 128-bit
    // coefficients drawn on the device from a ChaCha20 stream keyed with getrandom(2).  A large batch: uploads in
    // chunks, the hashes (62 % of this form) behind them.
    PipelinedInputs pin;      // its destructor drains the side streams on every error return
    const StagedInputs s = slice_inputs(hc, pin, b, n, coeffs, true, false);
    if (out24) hc.copy_back(out24, d_rec, SSA_MSM_PARTIAL_WORDS * sizeof(u64));
    else hc.copy_back(&v, d_verdict, sizeof v);
    if (int rc = hc.finish([&] { return msm_run(ctx, s.batch, n, s.coeffs, 32, d_verdict, d_rec, s.hashed); })) return rc;
    pin.done();
    if (verdict_out) *verdict_out = (int)v;
    return 0;
}

// A host batch of more than one MSM slice in bounded device memory (round 5): slice after slice through the one-slice
// form -- staging sized for a slice, only the slice in flight pinned, on the context and its twin alternately -- each
// reduced to its 24-word record in HOST memory, and the records combined like the shards of a multi-GPU batch
// (src/batch.rs:98-129: one point and one scalar per part): a verdict, or the whole batch's own record.
static int msm_host_sliced(ssa_ctx *ctx, const HostBatch &b, size_t n, const uint8_t *coeffs, int *verdict_out,
                           uint64_t *out24) {
    const size_t slice = ctx->knobs.msm_slice, k = (n + slice - 1) / slice;
    if (k > 4096) return SSA_ERR_ARG;
    std::vector<uint64_t> recs(k * SSA_MSM_PARTIAL_WORDS, 0);
    int rc = run_host_slices(ctx, n, slice, [&](ssa_ctx *c, size_t lo, size_t cnt) {
        std::vector<uint64_t> off;
        return msm_host_one(c, b.slice(lo, cnt, off), cnt, coeffs ? coeffs + 32 * lo : nullptr, nullptr,
                            recs.data() + (lo / slice) * SSA_MSM_PARTIAL_WORDS);
    });
    if (rc) return rc;
    HostCall hc(ctx);
    const u64 *d_parts = hc.in<u64>(ctx->st_aux, recs.data(), recs.size() * sizeof(uint64_t));
    uint32_t v = SSA_MALFORMED, *d_verdict = (uint32_t *)((char *)ctx->ws_fail.p + 32);
    u64 *d_rec = out24 ? (u64 *)hc.out(ctx->st_aux2, out24, SSA_MSM_PARTIAL_WORDS * sizeof(u64)) : nullptr;
    if (!out24) hc.copy_back(&v, d_verdict, sizeof v);
    if (int r = hc.finish([&] { return msm_combine_records(ctx, d_parts, k, out24 ? nullptr : d_verdict, d_rec, true); }))
        return r;
    if (verdict_out) *verdict_out = (int)v;
    return 0;
}

// One shard of a batch that spans several devices: stage the host buffers, run the MSM pipeline, return the shard's
// 24-word partial record (left-hand point, sum s_i e_i, malformed flag) in host memory.
extern "C" int ssa_verify_batch_msm_partial(ssa_ctx *ctx, const uint8_t *sigs, const uint8_t *pks, const uint8_t *pk_inf,
                                            const uint8_t *msgs, const uint64_t *msg_off, size_t msg_stride,
                                            size_t msg_len, size_t n, const uint8_t *coeffs,
                                            uint64_t out24[SSA_MSM_PARTIAL_WORDS]) {
    if (!ctx || !out24 || (n && (!sigs || !pks))) return SSA_ERR_ARG;
    if (int rc = check_msgs({msgs, msg_off, msg_stride, msg_len}, n)) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    std::memset(out24, 0, SSA_MSM_PARTIAL_WORDS * sizeof(uint64_t));
    if (n == 0) {
        out24[23] = SSA_MSM_RECORD_MAGIC;    // the empty shard's record: identity, 0
        return 0;
    }
    if (int rc = check_host_offsets(msg_off, n)) return rc;
    const HostBatch b{sigs, pks, pk_inf, msgs, msg_off, msg_stride, msg_len};
    return n > ctx->knobs.msm_slice ? msm_host_sliced(ctx, b, n, coeffs, nullptr, out24)
                              : msm_host_one(ctx, b, n, coeffs, nullptr, out24);
}

extern "C" int ssa_verify_batch_msm(ssa_ctx *ctx, const uint8_t *sigs, const uint8_t *pks, const uint8_t *pk_inf,
                                    const uint8_t *msgs, const uint64_t *msg_off, size_t msg_stride, size_t msg_len,
                                    size_t n, const uint8_t *coeffs) {
    if (!ctx || (n && (!sigs || !pks))) return SSA_ERR_ARG;
    if (int rc = check_msgs({msgs, msg_off, msg_stride, msg_len}, n)) return rc;
    if (int rc = check_host_offsets(msg_off, n)) return rc;
    if (n == 0) return SSA_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    const HostBatch b{sigs, pks, pk_inf, msgs, msg_off, msg_stride, msg_len};
    int verdict = SSA_MALFORMED;
    const int rc = n > ctx->knobs.msm_slice ? msm_host_sliced(ctx, b, n, coeffs, &verdict, nullptr)
                                      : msm_host_one(ctx, b, n, coeffs, &verdict, nullptr);
    return rc ? rc : verdict;
}

// ------------------------------------------------------------------------------------------------
// Screened batch verification: the MSM above with its buckets keyed by (window, segment, digit)
// gives one sum per contiguous segment of the slice in one pass; a segment whose equation holds exactly is accepted as a
// whole, and only the lanes of failing segments run the exact per-lane kernel, on the challenge scalars the MSM hashed.
constexpr u32 SCREEN_MAX_SEGS = 256;
constexpr u32 SCREEN_MIN_SEG_LANES = 1024;  // automatic K: the largest power of two <= 256 whose segments hold this many

struct ScreenPlan {
    u32 segs, seg_lanes;
};
// segments of a slice of n lanes: k requested (0 = automatic), segment size rounded up to whole 256-lane blocks, so the
// per-block partial sums of s_i e_i add up per segment; only the last segment can be ragged
static ScreenPlan screen_plan(size_t n, unsigned forced) {
    size_t k = forced;
    if (k == 0) {
        k = SCREEN_MAX_SEGS;
        while (k > 1 && n / k < SCREEN_MIN_SEG_LANES) k >>= 1;
    }
    size_t per = (n + k - 1) / k;
    per = (per + 255) & ~(size_t)255;
    return {(u32)((n + per - 1) / per), (u32)per};
}

extern "C" int ssa_debug_screen_plan(size_t n, uint32_t coeff_bytes, uint64_t out[8]) {
    if (!out || n == 0 || n > SSA_MAX_BATCH || coeff_bytes > 32) return SSA_ERR_ARG;
    const size_t slice = (size_t)1 << 23;           // the default SSA_MSM_SLICE
    const size_t first = n < slice ? n : slice, slices = (n + slice - 1) / slice, last = n - (slices - 1) * slice;
    const ScreenPlan pl = screen_plan(first, 0);
    const MsmShape sh = screen_shape(pl.segs);
    const u32 cb = coeff_bytes ? coeff_bytes : 16u;   // 0: the library draws 128-bit coefficients
    out[0] = pl.segs;
    out[1] = pl.seg_lanes;
    out[2] = sh.c;
    out[3] = sh.windows;
    out[4] = cb >= 32 ? sh.windows : (8u * cb + sh.c - 1) / sh.c;
    out[5] = sh.buckets;
    out[6] = slices;
    out[7] = (uint64_t)(slices - 1) * pl.segs + screen_plan(last, 0).segs;
    return 0;
}

extern "C" int ssa_debug_screen_segments(ssa_ctx *ctx, uint32_t k) {
    if (!ctx || k > SCREEN_MAX_SEGS) return SSA_ERR_ARG;
    ctx->knobs.screen_segs = k;
    return 0;
}

// ONE slice (n <= ctx->knobs.msm_slice) on ctx->stream into d_status[0, n): d_h = the slice's challenge scalars if they exist
// (else they are computed into ctx->ws_h).  Synchronises the stream once, to read the segment verdicts.
static int screen_slice(ssa_ctx *ctx, const DevBatch &b, size_t n, const uint8_t *d_coeffs, uint32_t coeff_bytes,
                        const u64 *d_h, uint8_t *d_status) {
    if (ctx->scr_fail.reserve(16)) return SSA_ERR_HIP;
    unsigned long long *scratch_fail = (unsigned long long *)ctx->scr_fail.p;    // (the caller counts the statuses)
    if (n <= ctx->knobs.msm_small_max) {      // the exact per-lane path
        if (d_h) return ssa_internal_verify_hashed(ctx, b, d_h, n, SSA_FLAG_SIG_FLAG_BYTE, d_status, scratch_fail);
        return ssa_internal_verify_many_device(ctx, b.sigs, b.pks, b.pk_inf, b.msgs.msgs, b.msgs.off, b.msgs.stride, b.msgs.len, n,
                                               SSA_FLAG_SIG_FLAG_BYTE, d_status, (uint64_t *)scratch_fail);
    }
    const ScreenPlan pl = screen_plan(n, ctx->knobs.screen_segs);
    if (ctx->scr_ok.reserve(SCREEN_MAX_SEGS)) return SSA_ERR_HIP;
    const ScreenArgs sa{pl.segs, pl.seg_lanes / 256u, d_status, (u8 *)ctx->scr_ok.p};
    if (int rc = msm_run_one(ctx, b, n, d_coeffs, coeff_bytes, nullptr, nullptr, d_h, &sa)) return rc;
    const u64 *h = d_h ? d_h : (const u64 *)ctx->ws_h.p;     // (msm_run_one hashed into ws_h)
    uint8_t ok[SCREEN_MAX_SEGS];
    HIP_TRY(hipMemcpyAsync(ok, ctx->scr_ok.p, pl.segs, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    ScreenList sl{};
    sl.seg_lanes = pl.seg_lanes;
    sl.n = (u32)n;
    size_t m = 0;
    for (u32 s = 0; s < pl.segs; s++) {
        if (ok[s]) continue;
        sl.id[sl.count++] = (uint16_t)s;
        const size_t lo = (size_t)s * pl.seg_lanes;
        m += n - lo < pl.seg_lanes ? n - lo : pl.seg_lanes;
    }
    if (m == 0) return 0;
    // Most of the slice fails (e.g. one bad lane in every segment): no gather, the per-lane kernel over all of it.
    if (2 * m > n)
        return ssa_internal_verify_hashed(ctx, b, h, n, SSA_FLAG_SIG_FLAG_BYTE, d_status, scratch_fail);
    auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t o_pks = al(m * 81), o_h = o_pks + al(m * 96), o_inf = o_h + al(m * 32), total = o_inf + al(m);
    if (ctx->scr_in.reserve(total) || ctx->scr_status.reserve(m + 16)) return SSA_ERR_HIP;
    u8 *g = (u8 *)ctx->scr_in.p;
    int rc = timed_launch(ctx, "screen_gather", [&] {
        const unsigned gx = grid_for((size_t)pl.seg_lanes * 210u / 16u, 256u * 4u);   // ~4 vectors per thread
        hipLaunchKernelGGL(msm_k_screen_gather, dim3(gx, sl.count), dim3(256), 0, ctx->stream, sl, b.sigs, b.pks, b.pk_inf,
                           h, g, g + o_pks, g + o_inf, (u64 *)(g + o_h));
    });
    if (rc) return rc;
    const DevBatch gathered{g, g + o_pks, b.pk_inf ? g + o_inf : nullptr, {}};
    if ((rc = ssa_internal_verify_hashed(ctx, gathered, (const u64 *)(g + o_h), m, SSA_FLAG_SIG_FLAG_BYTE,
                                         (u8 *)ctx->scr_status.p, scratch_fail)))
        return rc;
    return timed_launch(ctx, "screen_scatter", [&] {
        hipLaunchKernelGGL(msm_k_screen_scatter, dim3(grid_for(m, 256)), dim3(256), 0, ctx->stream, sl, m,
                           (const u8 *)ctx->scr_status.p, d_status);
    });
}

static int screen_count(ssa_ctx *ctx, const uint8_t *d_status, size_t n, unsigned long long *d_fail) {
    HIP_TRY(hipMemsetAsync(d_fail, 0, sizeof(unsigned long long), ctx->stream));
    hipLaunchKernelGGL(msm_k_screen_count, dim3(grid_for(n, 256)), dim3(256), 0, ctx->stream, d_status, n, d_fail);
    HIP_TRY(hipGetLastError());
    return 0;
}

int ssa_internal_screen_hashed(ssa_ctx *ctx, const DevBatch &b, size_t n, const uint64_t *d_h, uint8_t *d_status,
                               unsigned long long *d_fail) {
    if (!d_h || !d_status || n == 0 || n > ctx->knobs.msm_slice) return SSA_ERR_ARG;
    if (int rc = screen_slice(ctx, b, n, nullptr, 0, (const u64 *)d_h, d_status)) return rc;
    return d_fail ? screen_count(ctx, d_status, n, d_fail) : 0;
}

extern "C" int ssa_verify_batch_screened_device(ssa_ctx *ctx, const uint8_t *d_sigs, const uint8_t *d_pks,
                                                const uint8_t *d_pk_inf, const uint8_t *d_msgs, const uint64_t *d_msg_off,
                                                size_t msg_stride, size_t msg_len, size_t n, const uint8_t *d_coeffs,
                                                uint32_t coeff_bytes, uint8_t *d_status_out, uint64_t *d_n_fail_out) {
    const DevBatch b{d_sigs, d_pks, d_pk_inf, {d_msgs, d_msg_off, msg_stride, msg_len}};
    if (int rc = check_dev_batch(ctx, b, n, d_status_out, d_coeffs, coeff_bytes)) return rc;
    unsigned long long *d_fail;
    if (int rc = reset_fail_counter(ctx, d_n_fail_out, &d_fail)) return rc;
    if (n == 0) return 0;
    if (n <= ctx->knobs.msm_small_max)
        return ssa_internal_verify_many_device(ctx, d_sigs, d_pks, d_pk_inf, d_msgs, d_msg_off, msg_stride, msg_len, n,
                                               SSA_FLAG_SIG_FLAG_BYTE, d_status_out, (uint64_t *)d_fail);
    // (segments never straddle two slices)
    if (int rc = for_dev_slices(b, n, ctx->knobs.msm_slice, [&](size_t lo, size_t cnt, const DevBatch &s) {
            return screen_slice(ctx, s, cnt, d_coeffs ? d_coeffs + (size_t)coeff_bytes * lo : nullptr, coeff_bytes, nullptr,
                                d_status_out + lo);
        }))
        return rc;
    return screen_count(ctx, d_status_out, n, d_fail);
}

// ONE slice from host buffers (the staging of msm_host_one): statuses into status_out[0, n), *nf the count
static int screen_host_one(ssa_ctx *ctx, const HostBatch &b, size_t n, const uint8_t *coeffs, uint8_t *status_out,
                           uint64_t *nf) {
    return status_host_one(ctx, b, n, coeffs, true, false, status_out, nf,
                           [&](const StagedInputs &s, u8 *d_status, unsigned long long *d_fail) {
        if (int r = screen_slice(ctx, s.batch, n, s.coeffs, 32, s.hashed ? (const u64 *)ctx->ws_h.p : nullptr, d_status))
            return r;
        return screen_count(ctx, d_status, n, d_fail);
    });
}

extern "C" int ssa_verify_batch_screened(ssa_ctx *ctx, const uint8_t *sigs, const uint8_t *pks, const uint8_t *pk_inf,
                                         const uint8_t *msgs, const uint64_t *msg_off, size_t msg_stride, size_t msg_len,
                                         size_t n, const uint8_t *coeffs, uint8_t *status_out, uint64_t *n_fail_out) {
    const HostBatch b{sigs, pks, pk_inf, msgs, msg_off, msg_stride, msg_len};
    if (int rc = check_host_batch(ctx, b, n, status_out)) return rc;
    if (n_fail_out) *n_fail_out = 0;
    if (n == 0) return 0;
    HIP_TRY(hipSetDevice(ctx->device));
    if (n <= ctx->knobs.msm_small_max)
        return ssa_verify_many(ctx, sigs, pks, pk_inf, msgs, msg_off, msg_stride, msg_len, n, SSA_FLAG_SIG_FLAG_BYTE,
                               status_out, n_fail_out);
    return run_host_slices_counted(ctx, b, n, ctx->knobs.msm_slice, n_fail_out,
                                   [&](ssa_ctx *c, size_t lo, size_t cnt, const HostBatch &s, uint64_t *nf) {
                                       return screen_host_one(c, s, cnt, coeffs ? coeffs + 32 * lo : nullptr,
                                                              status_out + lo, nf);
                                   });
}

// ------------------------------------------------------------------------------------------------
// ssa_verify_many_screened: the screen above under the semantics of ssa_verify_many, for any
// combination of SSA_FLAG_CHECK_TORSION and SSA_FLAG_SIG_FLAG_BYTE.  Per slice of at most SSA_LANE_SLICE lanes: the
// distinct keys are found and checked once each (ssa_internal_dedup_keys), a lane whose key failed that check -- or whose
// signature gives msm_k_prepare no R -- is left out of the sums and marked, the segments are screened, and the marked
// lanes together with the lanes of failing segments run ssa_k_verify_keyed on the keys' tables and the hashes of the
// screen.  The screen only ever accepts: every nonzero status comes from the exact kernel.
constexpr uint32_t MANY_SCREEN_FLAGS = SSA_FLAG_CHECK_TORSION | SSA_FLAG_SIG_FLAG_BYTE;

// ONE slice (n <= ctx->knobs.lane_slice) on ctx->stream into d_status[0, n): d_h = the slice's challenge scalars if they exist
// (else they are computed into ctx->ws_h).  Synchronises the stream twice: for u, and for the segment verdicts together
// with the length of the re-check list.  With a key cache (ssa_verify_many_cached) the keys are
// looked up there and only the unseen ones are checked; everything behind the key check is the same code.
// stats: what the entry points report, a CallStats of 8 words, or of 12 with a key cache (words 8..11 are the cache's).
static int screen_slice_after_keys(ssa_ctx *ctx, const DevBatch &b, size_t n, const uint8_t *d_coeffs, uint32_t coeff_bytes,
                                   uint32_t flags, const u64 *d_h, uint8_t *d_status, CallStats *stats, const KeyView &kv,
                                   uint64_t u, uint64_t hits, const unsigned long long *d_unpublished, uint64_t sv[12]);

static int screen_many_slice(ssa_ctx *ctx, const DevBatch &b, size_t n, const uint8_t *d_coeffs, uint32_t coeff_bytes,
                             uint32_t flags, const u64 *d_h, uint8_t *d_status, CallStats *stats, ssa_keycache *kc) {
    uint64_t sv[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (ctx->scr_fail.reserve(16)) return SSA_ERR_HIP;
    unsigned long long *scratch_fail = (unsigned long long *)ctx->scr_fail.p;    // (the caller counts the statuses)
    if (n <= ctx->knobs.msm_small_max) {      // the exact per-lane path, the caller's flags
        sv[6] = 1;
        const int rc = d_h ? ssa_internal_verify_hashed(ctx, b, d_h, n, flags, d_status, scratch_fail)
                           : ssa_internal_verify_many_device(ctx, b.sigs, b.pks, b.pk_inf, b.msgs.msgs, b.msgs.off, b.msgs.stride,
                                                             b.msgs.len, n, flags, d_status, (uint64_t *)scratch_fail);
        if (rc == 0 && stats) stats->add(sv);
        return rc;
    }
    uint64_t u = 0, hits = 0;
    KeyView kv{};
    const unsigned long long *d_unpublished = nullptr;     // rows of the cache that found no slot (read with the verdicts)
    if (kc) {
        if (int rc = ssa_internal_keycache_slice(ctx, kc, b.pks, b.pk_inf, n, &kv, &u, &hits, sv + 8, &d_unpublished)) return rc;
    } else {
        if (int rc = ssa_internal_dedup_keys(ctx, b.pks, b.pk_inf, n, &u, &hits)) return rc;
        kv = ctx_key_view(ctx, u);
    }
    return screen_slice_after_keys(ctx, b, n, d_coeffs, coeff_bytes, flags, d_h, d_status, stats, kv, u, hits, d_unpublished,
                                   sv);
}

// The slice from its checked keys on: kv = where they are (the context's own, or rows of a key cache), u of them, `hits`
// lanes at the dedup's probe bound, sv[8..11] the cache's statistics.  Shared by the affine forms above and the wire form
// (ssa_verify_keyed_many_cached), whose b holds the split signatures and the expanded keys.
static int screen_slice_after_keys(ssa_ctx *ctx, const DevBatch &b, size_t n, const uint8_t *d_coeffs, uint32_t coeff_bytes,
                                   uint32_t flags, const u64 *d_h, uint8_t *d_status, CallStats *stats, const KeyView &kv,
                                   uint64_t u, uint64_t hits, const unsigned long long *d_unpublished, uint64_t sv[12]) {
    unsigned long long *scratch_fail = (unsigned long long *)ctx->scr_fail.p;    // (the caller counts the statuses)
    const unsigned nb = grid_for(n, SCR_BLOCK);
    if (ctx->scr_mask.reserve(n + 16) || ctx->scr_mark.reserve(n + 16) || ctx->scr_list.reserve(n * sizeof(u32)) ||
        ctx->scr_blk.reserve(2 * (size_t)nb * sizeof(u32)) || ctx->scr_cnt.reserve(64) || ctx->scr_ok.reserve(SCREEN_MAX_SEGS))
        return SSA_ERR_HIP;
    const u32 *key_idx = kv.lane_key;
    u8 *mark = (u8 *)ctx->scr_mark.p;
    u32 *blk_cnt = (u32 *)ctx->scr_blk.p, *blk_off = blk_cnt + nb, *list = (u32 *)ctx->scr_list.p;
    unsigned long long *d_cnt = (unsigned long long *)ctx->scr_cnt.p;
    int rc = timed_launch(ctx, "screen_keymask", [&] {
        hipLaunchKernelGGL(msm_k_screen_keymask, dim3(nb), dim3(SCR_BLOCK), 0, ctx->stream, key_idx,
                           kv.status, kv.n_keys, (u32)n, (u8 *)ctx->scr_mask.p);
    });
    if (rc) return rc;
    // (the side stream of msm_run_one waits for everything queued on ctx->stream so far: the key check and the mask are
    //  ordered before the half of msm_k_prepare that reads the mask, and that half still runs under the hash)
    const ScreenPlan pl = screen_plan(n, ctx->knobs.screen_segs);
    ScreenArgs sa{pl.segs, pl.seg_lanes / 256u, d_status, (u8 *)ctx->scr_ok.p};
    sa.lane_mask = (const u8 *)ctx->scr_mask.p;
    sa.recheck = mark;
    if ((rc = msm_run_one(ctx, b, n, d_coeffs, coeff_bytes, nullptr, nullptr, d_h, &sa))) return rc;
    const u64 *h = d_h ? d_h : (const u64 *)ctx->ws_h.p;     // (msm_run_one hashed into ws_h)
    HIP_TRY(hipMemsetAsync(d_cnt, 0, 2 * sizeof(unsigned long long), ctx->stream));
    rc = timed_launch(ctx, "screen_mark", [&] {
        hipLaunchKernelGGL(msm_k_screen_mark, dim3(nb), dim3(SCR_BLOCK), 0, ctx->stream, (const u8 *)ctx->scr_ok.p,
                           pl.seg_lanes, (u32)n, mark, blk_cnt, d_cnt);
        hipLaunchKernelGGL(msm_k_screen_scan, dim3(1), dim3(SCR_BLOCK), 0, ctx->stream, (const u32 *)blk_cnt, (u32)nb,
                           blk_off, d_cnt);
    });
    if (rc) return rc;
    uint8_t ok[SCREEN_MAX_SEGS];
    unsigned long long cnt[2] = {0, 0}, unpublished = 0;
    HIP_TRY(hipMemcpyAsync(ok, ctx->scr_ok.p, pl.segs, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(cnt, d_cnt, sizeof cnt, hipMemcpyDeviceToHost, ctx->stream));
    if (d_unpublished)
        HIP_TRY(hipMemcpyAsync(&unpublished, d_unpublished, sizeof unpublished, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    const size_t m = (size_t)cnt[1];
    if (m > n || cnt[0] > m) return SSA_ERR_HIP;     // (never)
    sv[0] = u;
    sv[1] = pl.segs;
    for (u32 s = 0; s < pl.segs; s++) sv[2] += ok[s] ? 0 : 1;
    sv[3] = m;
    sv[4] = cnt[0];
    sv[5] = 1;
    sv[7] = hits + unpublished;
    if (m == 0) {
        if (stats) stats->add(sv);
        return 0;
    }
    if (2 * m > n) {     // most of the slice: no list, the keyed kernel over all of it in place
        sv[6] = 1;
        rc = ssa_internal_verify_keyed_view(ctx, b.sigs, key_idx, kv, h, n, flags, d_status, scratch_fail);
        if (rc == 0 && stats) stats->add(sv);
        return rc;
    }
    auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t o_h = al(m * 81), o_idx = o_h + al(m * 32), total = o_idx + al(m * sizeof(u32));
    if (ctx->scr_in.reserve(total) || ctx->scr_status.reserve(m + 16)) return SSA_ERR_HIP;
    u8 *g = (u8 *)ctx->scr_in.p;
    rc = timed_launch(ctx, "screen_list_gather", [&] {
        hipLaunchKernelGGL(msm_k_screen_list, dim3(nb), dim3(SCR_BLOCK), 0, ctx->stream, (const u8 *)mark, (u32)n,
                           (const u32 *)blk_off, list);
        hipLaunchKernelGGL(msm_k_screen_gather_list, dim3(grid_for(m * 81, 256)), dim3(256), 0, ctx->stream,
                           (const u32 *)list, (u32)m, b.sigs, h, key_idx, g, (u64 *)(g + o_h), (u32 *)(g + o_idx));
    });
    if (rc) return rc;
    if ((rc = ssa_internal_verify_keyed_view(ctx, g, (const u32 *)(g + o_idx), kv, (const u64 *)(g + o_h), m, flags,
                                             (u8 *)ctx->scr_status.p, scratch_fail)))
        return rc;
    rc = timed_launch(ctx, "screen_list_scatter", [&] {
        hipLaunchKernelGGL(msm_k_screen_scatter_list, dim3(grid_for(m, 256)), dim3(256), 0, ctx->stream, (const u32 *)list,
                           (u32)m, (const u8 *)ctx->scr_status.p, d_status);
    });
    if (rc == 0 && stats) stats->add(sv);
    return rc;
}

// slices of this call: SSA_LANE_SLICE lanes (the dedup table, the per-key tables and the screen share one slice)
static size_t many_screen_slice_lanes(const ssa_ctx *ctx) {
    const size_t cap = (size_t)1 << 23;      // (msm_run_one: an item carries its point index in 24 bits)
    return ctx->knobs.lane_slice < cap ? ctx->knobs.lane_slice : cap;
}

// The device form of ssa_verify_many_screened (kc == nullptr, 8 statistics words) and of ssa_verify_many_cached (its key
// cache, 12 words): slice after slice on the context's stream.
static int many_screened_device(ssa_ctx *ctx, ssa_keycache *kc, const DevBatch &b, size_t n, uint32_t flags,
                                const uint8_t *d_coeffs, uint32_t coeff_bytes, uint8_t *d_status_out, uint64_t *d_n_fail_out,
                                uint64_t *stats_out, int stats_words) {
    if (flags & ~MANY_SCREEN_FLAGS) return SSA_ERR_ARG;
    if (int rc = check_dev_batch(ctx, b, n, d_status_out, d_coeffs, coeff_bytes)) return rc;
    if (kc && (kc->ctx != ctx || kc->wire_mode)) return SSA_ERR_ARG;      // (a wire cache takes wire records: section 18)
    CallStats st(stats_words);
    st.out(stats_out);      // (still empty: the caller's words are zeroed)
    if (flags == SSA_FLAG_SIG_FLAG_BYTE)      // verify_batch semantics: no key check to add or to cache, the screened form as it is
        return ssa_verify_batch_screened_device(ctx, b.sigs, b.pks, b.pk_inf, b.msgs.msgs, b.msgs.off, b.msgs.stride,
                                                b.msgs.len, n, d_coeffs, coeff_bytes, d_status_out, d_n_fail_out);
    unsigned long long *d_fail;
    if (int rc = reset_fail_counter(ctx, d_n_fail_out, &d_fail)) return rc;
    if (n == 0) return 0;
    if (n <= ctx->knobs.msm_small_max) {
        const int rc = ssa_internal_verify_many_device(ctx, b.sigs, b.pks, b.pk_inf, b.msgs.msgs, b.msgs.off, b.msgs.stride,
                                                       b.msgs.len, n, flags, d_status_out, (uint64_t *)d_fail);
        if (rc == 0 && stats_out) stats_out[6] = 1;
        return rc;
    }
    // (segments never straddle two slices)
    if (int rc = for_dev_slices(b, n, many_screen_slice_lanes(ctx), [&](size_t lo, size_t cnt, const DevBatch &s) {
            return screen_many_slice(ctx, s, cnt, d_coeffs ? d_coeffs + (size_t)coeff_bytes * lo : nullptr, coeff_bytes,
                                     flags, nullptr, d_status_out + lo, stats_out ? &st : nullptr, kc);
        }))
        return rc;
    if (int rc = screen_count(ctx, d_status_out, n, d_fail)) return rc;
    st.out(stats_out);
    return 0;
}

extern "C" int ssa_verify_many_screened_device(ssa_ctx *ctx, const uint8_t *d_sigs, const uint8_t *d_pks,
                                               const uint8_t *d_pk_inf, const uint8_t *d_msgs, const uint64_t *d_msg_off,
                                               size_t msg_stride, size_t msg_len, size_t n, uint32_t flags,
                                               const uint8_t *d_coeffs, uint32_t coeff_bytes, uint8_t *d_status_out,
                                               uint64_t *d_n_fail_out, uint64_t stats_out[8]) {
    return many_screened_device(ctx, nullptr, {d_sigs, d_pks, d_pk_inf, {d_msgs, d_msg_off, msg_stride, msg_len}}, n, flags,
                                d_coeffs, coeff_bytes, d_status_out, d_n_fail_out, stats_out, 8);
}

// ONE slice from host buffers (the staging of screen_host_one): statuses into status_out[0, n), *nf the count
static int screen_many_host_one(ssa_ctx *ctx, const HostBatch &b, size_t n, uint32_t flags, const uint8_t *coeffs,
                                uint8_t *status_out, uint64_t *nf, CallStats *stats, ssa_keycache *kc) {
    return status_host_one(ctx, b, n, coeffs, true, false, status_out, nf,
                           [&](const StagedInputs &s, u8 *d_status, unsigned long long *d_fail) {
        if (int r = screen_many_slice(ctx, s.batch, n, s.coeffs, 32, flags, s.hashed ? (const u64 *)ctx->ws_h.p : nullptr,
                                      d_status, stats, kc))
            return r;
        return screen_count(ctx, d_status, n, d_fail);
    });
}

// The slices of a host batch one after the other on the context itself, for a call whose slices share state (the key
// cache): fn as run_host_slices_counted takes it, the counts added up into *n_fail_out.  No second set of streams.
template <class F>
static int host_slices_in_order(ssa_ctx *ctx, const HostBatch &b, size_t n, size_t slice, uint64_t *n_fail_out, F &&fn) {
    uint64_t total = 0;
    for (size_t lo = 0; lo < n; lo += slice) {
        const size_t cnt = n - lo < slice ? n - lo : slice;
        std::vector<uint64_t> off;
        uint64_t nf = 0;
        if (int rc = fn(ctx, lo, cnt, b.slice(lo, cnt, off), &nf)) return rc;
        total += nf;
    }
    if (n_fail_out) *n_fail_out = total;
    return 0;
}

// The host form of ssa_verify_many_screened (kc == nullptr, 8 statistics words) and of ssa_verify_many_cached (DESIGN.md
// section 16: ssa_verify_many_screened with its per-key check behind a key cache, 12 words).
static int many_screened_host(ssa_ctx *ctx, ssa_keycache *kc, const HostBatch &b, size_t n, uint32_t flags,
                              const uint8_t *coeffs, uint8_t *status_out, uint64_t *n_fail_out, uint64_t *stats_out,
                              int stats_words) {
    if (flags & ~MANY_SCREEN_FLAGS) return SSA_ERR_ARG;
    if (int rc = check_host_batch(ctx, b, n, status_out)) return rc;
    if (kc && (kc->ctx != ctx || kc->wire_mode)) return SSA_ERR_ARG;      // (a wire cache takes wire records: section 18)
    CallStats st(stats_words);
    st.out(stats_out);      // (still empty: the caller's words are zeroed)
    if (flags == SSA_FLAG_SIG_FLAG_BYTE)      // verify_batch semantics: no key check to add or to cache
        return ssa_verify_batch_screened(ctx, b.sigs, b.pks, b.pk_inf, b.msgs, b.msg_off, b.msg_stride, b.msg_len, n, coeffs,
                                         status_out, n_fail_out);
    if (n_fail_out) *n_fail_out = 0;
    if (n == 0) return 0;
    HIP_TRY(hipSetDevice(ctx->device));
    if (n <= ctx->knobs.msm_small_max) {
        const int rc = ssa_verify_many(ctx, b.sigs, b.pks, b.pk_inf, b.msgs, b.msg_off, b.msg_stride, b.msg_len, n, flags,
                                       status_out, n_fail_out);
        if (rc == 0 && stats_out) stats_out[6] = 1;
        return rc;
    }
    auto one = [&](ssa_ctx *c, size_t lo, size_t cnt, const HostBatch &s, uint64_t *nf) {
        return screen_many_host_one(c, s, cnt, flags, coeffs ? coeffs + 32 * lo : nullptr, status_out + lo, nf,
                                    stats_out ? &st : nullptr, kc);
    };
    // The one difference between the two host forms.  Every slice reads and may extend the one cache, and two streams
    // would mutate it at once: with a cache the slices run in order on this context alone; without one they alternate
    // between the context and its second set of streams.
    const size_t slice = many_screen_slice_lanes(ctx);
    const int rc = kc ? host_slices_in_order(ctx, b, n, slice, n_fail_out, one)
                      : run_host_slices_counted(ctx, b, n, slice, n_fail_out, one);
    if (rc) return rc;
    st.out(stats_out);
    return 0;
}

extern "C" int ssa_verify_many_screened(ssa_ctx *ctx, const uint8_t *sigs, const uint8_t *pks, const uint8_t *pk_inf,
                                        const uint8_t *msgs, const uint64_t *msg_off, size_t msg_stride, size_t msg_len,
                                        size_t n, uint32_t flags, const uint8_t *coeffs, uint8_t *status_out,
                                        uint64_t *n_fail_out, uint64_t stats_out[8]) {
    return many_screened_host(ctx, nullptr, {sigs, pks, pk_inf, msgs, msg_off, msg_stride, msg_len}, n, flags, coeffs,
                              status_out, n_fail_out, stats_out, 8);
}

// ------------------------------------------------------------------------------------------------
// ssa_verify_many_cached: ssa_verify_many_screened with its per-key check behind a key cache.
// The slices of one call run in order on the context's stream in BOTH forms (many_screened_host has the reason).
extern "C" int ssa_verify_many_cached_device(ssa_ctx *ctx, ssa_keycache *kc, const uint8_t *d_sigs, const uint8_t *d_pks,
                                             const uint8_t *d_pk_inf, const uint8_t *d_msgs, const uint64_t *d_msg_off,
                                             size_t msg_stride, size_t msg_len, size_t n, uint32_t flags,
                                             const uint8_t *d_coeffs, uint32_t coeff_bytes, uint8_t *d_status_out,
                                             uint64_t *d_n_fail_out, uint64_t stats_out[12]) {
    if (!kc) return SSA_ERR_ARG;
    return many_screened_device(ctx, kc, {d_sigs, d_pks, d_pk_inf, {d_msgs, d_msg_off, msg_stride, msg_len}}, n, flags,
                                d_coeffs, coeff_bytes, d_status_out, d_n_fail_out, stats_out, 12);
}

extern "C" int ssa_verify_many_cached(ssa_ctx *ctx, ssa_keycache *kc, const uint8_t *sigs, const uint8_t *pks,
                                      const uint8_t *pk_inf, const uint8_t *msgs, const uint64_t *msg_off, size_t msg_stride,
                                      size_t msg_len, size_t n, uint32_t flags, const uint8_t *coeffs, uint8_t *status_out,
                                      uint64_t *n_fail_out, uint64_t stats_out[12]) {
    if (!kc) return SSA_ERR_ARG;
    return many_screened_host(ctx, kc, {sigs, pks, pk_inf, msgs, msg_off, msg_stride, msg_len}, n, flags, coeffs, status_out,
                              n_fail_out, stats_out, 12);
}

// ------------------------------------------------------------------------------------------------
// KeyedSignature wire records.  ssa_verify_keyed_many_device: the exact call on device buffers.
// ssa_verify_keyed_many_cached: ssa_verify_many_cached on 130-byte records through a cache in wire mode -- the key's 49
// bytes are its identity, so a warm call decompresses nothing.  Kernels: ssa_keyed.hpp; the slice: ssa_api.hip.

// Where ONE launch of ssa_k_hash over a slice of records leaves the challenge scalars mod q (h, four words per lane) and
// the raw digests (dig, 32 bytes per lane): the slice's keys exist only after its unpack or cache look-up, so a caller
// that needs both (ssa_aggregate_valid_keyed_many_cached) has the slice hash in between and the
// verification behind it then takes h as ready hashes.
struct SliceHash {
    u64 *h;
    u8 *dig;
};
static int keyed_hash_slice(ssa_ctx *ctx, const DevBatch &b, size_t n, const SliceHash &sh) {
    return ssa_internal_hash_scalars_digests(ctx, b, n, sh.h, sh.dig);
}

// ONE slice of at most lane_slice records on the exact path: unpacked into the context's per-lane workspaces, then
// ssa_verify_many_device with the caller's flags (*d_fail is zeroed by it); sh != nullptr: the hash as SliceHash says,
// then ssa_k_verify on those scalars (*d_fail is added to)
static int keyed_exact_slice(ssa_ctx *ctx, const uint8_t *d_keyed, const MsgView &mv, size_t n, uint32_t flags,
                             uint8_t *d_status, unsigned long long *d_fail, const SliceHash *sh = nullptr) {
    DevBatch b{nullptr, nullptr, nullptr, mv};
    if (int rc = ssa_internal_unpack_keyed(ctx, d_keyed, n, &b)) return rc;
    if (sh) {
        if (int rc = keyed_hash_slice(ctx, b, n, *sh)) return rc;
        return ssa_internal_verify_hashed(ctx, b, sh->h, n, flags, d_status, d_fail);
    }
    return ssa_internal_verify_many_device(ctx, b.sigs, b.pks, b.pk_inf, mv.msgs, mv.off, mv.stride, mv.len, n, flags, d_status,
                                           (uint64_t *)d_fail);
}

// check_dev_batch for records: the argument checks of the device forms, before anything is zeroed or enqueued
static int check_keyed_dev(const ssa_ctx *ctx, const uint8_t *d_keyed, const MsgView &mv, size_t n,
                           const uint8_t *d_status_out, const uint8_t *d_coeffs, uint32_t coeff_bytes) {
    if (!ctx || (n && (!d_keyed || !d_status_out))) return SSA_ERR_ARG;
    if (d_coeffs && (coeff_bytes == 0 || coeff_bytes > 32)) return SSA_ERR_ARG;
    return check_msgs(mv, n);
}

extern "C" int ssa_verify_keyed_many_device(ssa_ctx *ctx, const uint8_t *d_keyed, const uint8_t *d_msgs,
                                            const uint64_t *d_msg_off, size_t msg_stride, size_t msg_len, size_t n,
                                            uint32_t flags, uint8_t *d_status_out, uint64_t *d_n_fail_out) {
    const MsgView mv{d_msgs, d_msg_off, msg_stride, msg_len};
    if (int rc = check_keyed_dev(ctx, d_keyed, mv, n, d_status_out, nullptr, 32)) return rc;
    unsigned long long *d_fail;
    if (int rc = reset_fail_counter(ctx, d_n_fail_out, &d_fail)) return rc;
    if (n == 0) return 0;
    if (n <= ctx->knobs.lane_slice) return keyed_exact_slice(ctx, d_keyed, mv, n, flags, d_status_out, d_fail);
    if (ctx->scr_fail.reserve(16)) return SSA_ERR_HIP;
    const DevBatch b{nullptr, nullptr, nullptr, mv};
    if (int rc = for_dev_slices(b, n, ctx->knobs.lane_slice, [&](size_t lo, size_t cnt, const DevBatch &s) {
            return keyed_exact_slice(ctx, d_keyed + 130 * lo, s.msgs, cnt, flags, d_status_out + lo,
                                     (unsigned long long *)ctx->scr_fail.p);
        }))
        return rc;
    return screen_count(ctx, d_status_out, n, d_fail);
}

// ONE slice (n <= SSA_LANE_SLICE records) of the wire form on ctx->stream into d_status[0, n): screen_many_slice with
// the keys looked up by their 49 bytes.  A slice of at most msm_small_max lanes takes the exact keyed path.
// sh != nullptr: one hash launch between the keys and the screen (SliceHash), and no other.
static int keyed_cached_slice(ssa_ctx *ctx, ssa_keycache *kc, const uint8_t *d_keyed, const MsgView &mv, size_t n,
                              const uint8_t *d_coeffs, uint32_t coeff_bytes, uint32_t flags, uint8_t *d_status,
                              CallStats *stats, const SliceHash *sh = nullptr) {
    uint64_t sv[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (ctx->scr_fail.reserve(16)) return SSA_ERR_HIP;
    if (n <= ctx->knobs.msm_small_max) {
        sv[6] = 1;
        const int rc = keyed_exact_slice(ctx, d_keyed, mv, n, flags, d_status, (unsigned long long *)ctx->scr_fail.p, sh);
        if (rc == 0 && stats) stats->add(sv);
        return rc;
    }
    uint64_t u = 0, hits = 0;
    KeyView kv{};
    DevBatch b{nullptr, nullptr, nullptr, mv};
    const unsigned long long *d_unpublished = nullptr;
    if (int rc = ssa_internal_keyed_cache_slice(ctx, kc, d_keyed, n, &b, &kv, &u, &hits, sv + 8, &d_unpublished)) return rc;
    if (sh) {
        if (int rc = keyed_hash_slice(ctx, b, n, *sh)) return rc;
        return screen_slice_after_keys(ctx, b, n, d_coeffs, coeff_bytes, flags, sh->h, d_status, stats, kv, u, hits,
                                       d_unpublished, sv);
    }
    return screen_slice_after_keys(ctx, b, n, d_coeffs, coeff_bytes, flags, nullptr, d_status, stats, kv, u, hits,
                                   d_unpublished, sv);
}

// flags == SSA_FLAG_SIG_FLAG_BYTE alone (verify_batch semantics: no key check to cache): the records unpacked, slice by
// slice of the MSM form, and ssa_verify_batch_screened_device as it is; the cache is not touched
static int keyed_batch_screened_device(ssa_ctx *ctx, const uint8_t *d_keyed, const MsgView &mv, size_t n,
                                       const uint8_t *d_coeffs, uint32_t coeff_bytes, uint8_t *d_status_out,
                                       uint64_t *d_n_fail_out) {
    unsigned long long *d_fail;
    if (int rc = reset_fail_counter(ctx, d_n_fail_out, &d_fail)) return rc;
    if (n == 0) return 0;
    if (ctx->scr_fail.reserve(16)) return SSA_ERR_HIP;
    const DevBatch whole{nullptr, nullptr, nullptr, mv};
    if (int rc = for_dev_slices(whole, n, ctx->knobs.msm_slice, [&](size_t lo, size_t cnt, const DevBatch &s) {
            DevBatch b = s;
            if (int r = ssa_internal_unpack_keyed(ctx, d_keyed + 130 * lo, cnt, &b)) return r;
            return ssa_verify_batch_screened_device(ctx, b.sigs, b.pks, b.pk_inf, b.msgs.msgs, b.msgs.off, b.msgs.stride,
                                                    b.msgs.len, cnt, d_coeffs ? d_coeffs + (size_t)coeff_bytes * lo : nullptr,
                                                    coeff_bytes, d_status_out + lo, (uint64_t *)ctx->scr_fail.p);
        }))
        return rc;
    return screen_count(ctx, d_status_out, n, d_fail);
}

extern "C" int ssa_verify_keyed_many_cached_device(ssa_ctx *ctx, ssa_keycache *kc, const uint8_t *d_keyed,
                                                   const uint8_t *d_msgs, const uint64_t *d_msg_off, size_t msg_stride,
                                                   size_t msg_len, size_t n, uint32_t flags, const uint8_t *d_coeffs,
                                                   uint32_t coeff_bytes, uint8_t *d_status_out, uint64_t *d_n_fail_out,
                                                   uint64_t stats_out[12]) {
    if (flags & ~MANY_SCREEN_FLAGS) return SSA_ERR_ARG;
    if (!kc) return SSA_ERR_ARG;
    const MsgView mv{d_msgs, d_msg_off, msg_stride, msg_len};
    if (int rc = check_keyed_dev(ctx, d_keyed, mv, n, d_status_out, d_coeffs, coeff_bytes)) return rc;
    if (kc->ctx != ctx || !kc->wire_mode) return SSA_ERR_ARG;      // (an affine cache takes affine keys: section 16)
    CallStats st(12);
    st.out(stats_out);      // (still empty: the caller's words are zeroed)
    if (flags == SSA_FLAG_SIG_FLAG_BYTE)
        return keyed_batch_screened_device(ctx, d_keyed, mv, n, d_coeffs, coeff_bytes, d_status_out, d_n_fail_out);
    unsigned long long *d_fail;
    if (int rc = reset_fail_counter(ctx, d_n_fail_out, &d_fail)) return rc;
    if (n == 0) return 0;
    if (n <= ctx->knobs.msm_small_max) {
        const int rc = keyed_exact_slice(ctx, d_keyed, mv, n, flags, d_status_out, d_fail);
        if (rc == 0 && stats_out) stats_out[6] = 1;
        return rc;
    }
    const DevBatch whole{nullptr, nullptr, nullptr, mv};
    if (int rc = for_dev_slices(whole, n, many_screen_slice_lanes(ctx), [&](size_t lo, size_t cnt, const DevBatch &s) {
            return keyed_cached_slice(ctx, kc, d_keyed + 130 * lo, s.msgs, cnt,
                                      d_coeffs ? d_coeffs + (size_t)coeff_bytes * lo : nullptr, coeff_bytes, flags,
                                      d_status_out + lo, stats_out ? &st : nullptr);
        }))
        return rc;
    if (int rc = screen_count(ctx, d_status_out, n, d_fail)) return rc;
    st.out(stats_out);
    return 0;
}

// ONE slice of the wire form from host buffers (b: the messages only): the 130-byte records, the messages and the
// coefficients are staged on the context's stream -- no pipelined upload-and-hash: the hash needs y, which exists only
// after the look-up -- and device_form(d_keyed, messages, d_coeffs, d_status, d_fail) leaves the statuses and their count
template <class F>
static int keyed_host_one(ssa_ctx *ctx, const uint8_t *keyed, const HostBatch &b, size_t n, const uint8_t *coeffs,
                          uint8_t *status_out, uint64_t *nf_out, F &&device_form) {
    HostCall hc(ctx);
    const u8 *d_keyed = hc.in(ctx->st_keyed, keyed, n * 130);
    const MsgView mv = hc.msgs(b.msgs, b.msg_off, b.msg_stride, b.msg_len, n);
    const u8 *d_coeffs = coeffs ? hc.in(ctx->st_coeffs, coeffs, n * 32) : nullptr;
    u8 *d_status = hc.out(ctx->st_status, status_out, n, 16);
    unsigned long long nf = 0, *d_fail = (unsigned long long *)ctx->ws_fail.p;
    hc.copy_back(&nf, d_fail, sizeof nf);
    if (int rc = hc.finish([&] { return device_form(d_keyed, mv, d_coeffs, d_status, d_fail); })) return rc;
    if (nf_out) *nf_out = nf;
    return 0;
}

extern "C" int ssa_verify_keyed_many_cached(ssa_ctx *ctx, ssa_keycache *kc, const uint8_t *keyed, const uint8_t *msgs,
                                            const uint64_t *msg_off, size_t msg_stride, size_t msg_len, size_t n,
                                            uint32_t flags, const uint8_t *coeffs, uint8_t *status_out,
                                            uint64_t *n_fail_out, uint64_t stats_out[12]) {
    if (flags & ~MANY_SCREEN_FLAGS) return SSA_ERR_ARG;
    if (!ctx || !kc || (n && (!keyed || !status_out))) return SSA_ERR_ARG;
    if (int rc = check_msgs({msgs, msg_off, msg_stride, msg_len}, n)) return rc;
    if (int rc = check_host_offsets(msg_off, n)) return rc;
    if (kc->ctx != ctx || !kc->wire_mode) return SSA_ERR_ARG;      // (an affine cache takes affine keys: section 16)
    CallStats st(12);
    st.out(stats_out);      // (still empty: the caller's words are zeroed)
    if (n_fail_out) *n_fail_out = 0;
    if (n == 0) return 0;
    HIP_TRY(hipSetDevice(ctx->device));
    const HostBatch b{nullptr, nullptr, nullptr, msgs, msg_off, msg_stride, msg_len};
    const bool batch_form = flags == SSA_FLAG_SIG_FLAG_BYTE, small = !batch_form && n <= ctx->knobs.msm_small_max;
    // every slice reads and may extend the one cache: in order, on this context alone (host_slices_in_order)
    const size_t slice = batch_form ? ctx->knobs.msm_slice : many_screen_slice_lanes(ctx);
    const int rc = host_slices_in_order(ctx, b, n, slice, n_fail_out,
                                        [&](ssa_ctx *c, size_t lo, size_t cnt, const HostBatch &s, uint64_t *nf) {
        return keyed_host_one(c, keyed + 130 * lo, s, cnt, coeffs ? coeffs + 32 * lo : nullptr, status_out + lo, nf,
                              [&](const u8 *d_keyed, const MsgView &mv, const u8 *d_coeffs, u8 *d_status,
                                  unsigned long long *d_fail) {
            if (batch_form) return keyed_batch_screened_device(c, d_keyed, mv, cnt, d_coeffs, 32, d_status, (uint64_t *)d_fail);
            if (small) return keyed_exact_slice(c, d_keyed, mv, cnt, flags, d_status, d_fail);
            if (int r = keyed_cached_slice(c, kc, d_keyed, mv, cnt, d_coeffs, 32, flags, d_status, stats_out ? &st : nullptr))
                return r;
            return screen_count(c, d_status, cnt, d_fail);
        });
    });
    if (rc) return rc;
    if (small && stats_out) stats_out[6] = 1;
    if (!small && !batch_form) st.out(stats_out);
    return 0;
}

// ------------------------------------------------------------------------------------------------
// For ssa_aggregate_valid_many_cached (ssa_api.hip): the device forms of ssa_verify_many_cached and
// ssa_verify_keyed_many_cached with SSA_FLAG_CHECK_TORSION | SSA_FLAG_SIG_FLAG_BYTE and library-drawn coefficients, slice
// after slice as those calls take them, on challenge scalars that are hashed once for the caller and the screen alike.
// The arguments are the caller's to check (n >= 1, the cache of the right mode and of this context).
int ssa_internal_screen_many_hashed(ssa_ctx *ctx, ssa_keycache *kc, const DevBatch &b, size_t n, const uint64_t *d_h,
                                    uint8_t *d_status, uint64_t stats_out[12]) {
    if (!kc || !d_h || !d_status || n == 0) return SSA_ERR_ARG;
    CallStats st(12);
    st.out(stats_out);
    if (ctx->scr_fail.reserve(16)) return SSA_ERR_HIP;
    if (n <= ctx->knobs.msm_small_max) {      // (the whole call on the exact path: the cache is not used)
        const int rc = ssa_internal_verify_hashed(ctx, b, d_h, n, MANY_SCREEN_FLAGS, d_status,
                                                  (unsigned long long *)ctx->scr_fail.p);
        if (rc == 0 && stats_out) stats_out[6] = 1;
        return rc;
    }
    if (int rc = for_dev_slices(b, n, many_screen_slice_lanes(ctx), [&](size_t lo, size_t cnt, const DevBatch &s) {
            return screen_many_slice(ctx, s, cnt, nullptr, 0, MANY_SCREEN_FLAGS, (const u64 *)d_h + 4 * lo, d_status + lo,
                                     stats_out ? &st : nullptr, kc);
        }))
        return rc;
    st.out(stats_out);
    return 0;
}

// The same for 130-byte records through a wire cache.  d_h (n x 4 words) and d_dig (n x 32 bytes) are WRITTEN: one launch
// of ssa_k_hash per slice, behind the slice's keys, leaves lanes [lo, lo + cnt) of both.
int ssa_internal_screen_keyed_hashed(ssa_ctx *ctx, ssa_keycache *kc, const uint8_t *d_keyed, const MsgView &mv, size_t n,
                                     uint64_t *d_h, uint8_t *d_dig, uint8_t *d_status, uint64_t stats_out[12]) {
    if (!kc || !d_keyed || !d_h || !d_dig || !d_status || n == 0) return SSA_ERR_ARG;
    CallStats st(12);
    st.out(stats_out);
    if (ctx->scr_fail.reserve(16)) return SSA_ERR_HIP;
    if (n <= ctx->knobs.msm_small_max) {
        const SliceHash sh{(u64 *)d_h, d_dig};
        const int rc = keyed_exact_slice(ctx, d_keyed, mv, n, MANY_SCREEN_FLAGS, d_status, (unsigned long long *)ctx->scr_fail.p,
                                         &sh);
        if (rc == 0 && stats_out) stats_out[6] = 1;
        return rc;
    }
    const DevBatch whole{nullptr, nullptr, nullptr, mv};
    if (int rc = for_dev_slices(whole, n, many_screen_slice_lanes(ctx), [&](size_t lo, size_t cnt, const DevBatch &s) {
            const SliceHash sh{(u64 *)d_h + 4 * lo, d_dig + 32 * lo};
            return keyed_cached_slice(ctx, kc, d_keyed + 130 * lo, s.msgs, cnt, nullptr, 0, MANY_SCREEN_FLAGS, d_status + lo,
                                      stats_out ? &st : nullptr, &sh);
        }))
        return rc;
    st.out(stats_out);
    return 0;
}
