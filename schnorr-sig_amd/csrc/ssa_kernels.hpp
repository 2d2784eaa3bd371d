// HIP kernels of the verification path, one signature per lane (wave64, gfx950).
//
//   ssa_k_hash     hash_message (src/signature.rs:274-306) -> challenge scalar h mod q
//   ssa_k_verify   [h]P + [e]G, x-only compare, optional [q]P == O (src/signature.rs:181-205)
//   ssa_k_gtable   fixed-base comb table for G (BASEPOINT_TABLE, src/signature.rs:20,116)
//   ssa_k_sign     keygen + sign (src/public.rs:26-32, src/signature.rs:114-129)
//   ssa_k_rescue   RescueHash::hash_field on raw felt rows (src/signature.rs:303)
//   ssa_k_decompress  AffinePoint::from_compressed (src/public.rs:54-56, src/batch.rs:104)
//
// HBM layout: inputs stay in the caller's AoS byte records (81-B signatures, 96-B keys,
// message bytes); per-lane intermediates live in the context workspace:
//   ws_h    n x 4 u64       challenge scalars
//   ws_tab  n x 16 x 32 u64 per-lane affine multiples 1P..16P (256-B rows: x, y in the first 128-B line; the second
//                           line is scratch of the batch normalisation and holds the NEGATIVE entry (x, -y) once the
//                           table is finished), lane-contiguous so that a lane's gather of one entry -- of either
//                           sign -- is six 16-byte loads from ONE cache line
//   gtab    count x 2^bits x 12 u64 affine multiples d*2^(bits*w)*G -- 11 x 2^24 rows (17.7 GB) where HBM allows, down to
//           16 x 2^16 (100 MB); the geometry is a property of the table (its first row), chosen per context
#pragma once
#include "curve.hpp"
#include "fp3.hpp"
#include "rescue.hpp"

namespace ssa {

// Fixed-base comb for G: gtab[w][d] = affine [d 2^(bits w)] G, `count` windows of `bits` bits -- [e]G is `count` mixed
// additions and no doubling.  The geometry is a property of the TABLE, not of the build (round 5; a compile-time 24 / 11
// in round 4): 24 bits x 11 windows = 17.7 GB (ssa_k_verify 26.57 ms), 22 x 12 = 4.8 GB (26.70), 20 x 13 = 1.3 GB,
// 16 x 16 = 100 MB (27.08): ssa_ctx_create takes the widest that fits its HBM budget and falls back when the allocation
// fails.  ONE table per device, generator and geometry, shared by the contexts of a process: sized for the 288 GB of the
// part, not for a cache -- a lane gathers 11 rows in 13 ms of ladder, the second wave of the SIMD covers the misses.
// The table describes itself: row 0 of window 0 is the identity row that no digit ever selects (a zero digit skips the
// addition), and its first word carries bits | count << 8 -- every kernel that walks the comb reads the geometry
// from the table it was handed, so a table and its geometry cannot be mixed up.
struct GtabGeom {
    u32 bits, count;
};
constexpr int GW_BITS_MAX = 24, GW_BITS_MIN = 16;
__host__ __device__ inline u32 gtab_windows(u32 bits) { return (255u + bits) / bits; }           // bits * count >= 256
__host__ __device__ inline size_t gtab_entries(u32 bits) { return (size_t)gtab_windows(bits) << bits; }
__host__ __device__ inline size_t gbase_entries(u32 bits) { return ((size_t)gtab_windows(bits) * 2) << (bits / 2); }
__host__ __device__ inline u64 gtab_header(u32 bits) { return (u64)bits | ((u64)gtab_windows(bits) << 8); }
SSA_DEV GtabGeom gtab_geom(const u64 *__restrict__ gtab) {
    // (the same word for every lane: read once into scalar registers, so that the geometry costs no vector register and
    // the window arithmetic of the comb loops runs on the scalar unit)
    const u32 v = (u32)__builtin_amdgcn_readfirstlane((int)(u32)gtab[0]);
    GtabGeom g;
    g.bits = v & 0xffu;
    g.count = (v >> 8) & 0xffu;
    return g;
}
constexpr int PTAB_ENTRIES = 16;    // 1P..16P: signed 5-bit windows (round 4; 1P..8P and 4-bit windows before)
// a table row is 256 B = two 128-B lines: X, Y (affine x, y after the build) in the first -- a gather of the
// ladder touches exactly one line -- and Z, prefix product of the build in the second
constexpr int PTAB_ENTRY_U64 = 32, PTAB_Z = 16, PTAB_C = 22;
// finished table: the second 128-B line of a row holds the NEGATIVE of the entry, (x, -y): the ladder reads one line
// per window whatever the digit's sign and never negates (round 2 kept only -y there: a negative digit touched both lines)
constexpr int PTAB_NEG = 16, PTAB_NY = PTAB_NEG + 6;

constexpr u32 ST_OK = 0, ST_INVALID_PK = 1, ST_INVALID_SIG = 2, ST_MALFORMED = 3;

typedef uint8_t u8;

SSA_DEV u64 ld_u64_le(const u8 *p) {
    u64 v = 0;
#pragma unroll
    for (int k = 7; k >= 0; k--) v = (v << 8) | p[k];
    return v;
}
SSA_DEV void st_u64_le(u8 *p, u64 v) {
#pragma unroll
    for (int k = 0; k < 8; k++) p[k] = (u8)(v >> (8 * k));
}
// six limbs; ok &= all canonical
SSA_DEV fp6 ld_fp6(const u8 *p, bool &ok) {
    fp6 r;
#pragma unroll
    for (int i = 0; i < 6; i++) {
        r.c[i] = ld_u64_le(p + 8 * i);
        ok = ok && (r.c[i] < FP_P);
    }
    return r;
}
SSA_DEV void st_fp6(u8 *p, const fp6 &a) {
#pragma unroll
    for (int i = 0; i < 6; i++) st_u64_le(p + 8 * i, fp_canon(a.c[i]));
}
SSA_DEV sc256 ld_sc(const u8 *p) {
    sc256 r;
#pragma unroll
    for (int i = 0; i < 4; i++) r.w[i] = ld_u64_le(p + 8 * i);
    return r;
}

struct MsgView {
    const u8 *msgs;
    const u64 *off;  // n+1 offsets or nullptr
    size_t stride, len;
};
SSA_DEV const u8 *msg_ptr(const MsgView &mv, size_t i, u32 &len) {
    if (mv.off) {
        u64 b = mv.off[i];
        len = (u32)(mv.off[i + 1] - b);
        return mv.msgs + b;
    }
    len = (u32)mv.len;
    return mv.msgs + i * mv.stride;
}

// message felt c (src/signature.rs:285-301): 7 bytes LE; the final partial chunk gets a 0x01
// terminator at index chunk_len; no terminator felt when len % 7 == 0.
SSA_DEV u64 msg_felt(const u8 *m, u32 len, u32 c) {
    const u32 off = 7u * c;
    const u32 rem = len - off;
    u64 v = 0;
#pragma unroll
    for (int k = 0; k < 7; k++) {
        u64 b = 0;
        if ((u32)k < rem) b = m[off + k];
        else if ((u32)k == rem) b = 1;
        v |= b << (8 * k);
    }
    return v;
}

// hash_message for lane data already in registers -> 4 canonical digest felts
SSA_DEV void hash_message_lane(u64 *A, u64 *B, const DevParams *__restrict__ prm, const fp6 &rx,
                               const fp6 &px, u64 py0, const u8 *m, u32 len, u64 (&digest)[4]) {
    const u32 nmsg = (len + 6u) / 7u;
    const u32 n_felts = 13u + nmsg;
    auto src = [&](u32 idx) -> u64 {
        u64 v;
        if (idx < 13u) {
            v = py0;
#pragma unroll
            for (int i = 0; i < 6; i++) {
                if (idx == (u32)i) v = rx.c[i];
                if (idx == (u32)(6 + i)) v = px.c[i];
            }
        } else {
            v = msg_felt(m, len, idx - 13u);
        }
        return v;
    };
    sponge_hash(A, B, prm, n_felts, src, digest);
}

// signer sets (ssa_sign_many_indexed): the key pairs of a set, as the signing kernels read them
struct SignerView {
    const u8 *sks, *pks, *cpks, *status;   // m x 32 secret keys, m x 96 affine keys, m x 49 compressed keys, m statuses
    u32 m;
};
// the key row of signing lane i, or -1 when key_idx[i] >= m or the key is unusable: the lane's record (81 bytes, 130
// keyed) is zeroed and its status is SSA_MALFORMED.  (the index and the key's status are public: the status says both)
SSA_DEV long signer_row(const SignerView &sv, const u32 *__restrict__ key_idx, size_t i, u32 keyed, u8 *__restrict__ rec,
                        u8 *__restrict__ lane_status) {
    const u32 k = key_idx[i];
    const bool usable = k < sv.m && sv.status[k] == ST_OK;
    if (lane_status) lane_status[i] = (u8)(usable ? ST_OK : ST_MALFORMED);
    if (usable) return (long)k;
    const int len = keyed ? 130 : 81;
    for (int j = 0; j < len; j++) rec[j] = 0;
    return -1;
}
// KeyedSignature::to_bytes: the stored compressed key in front of the signature
SSA_DEV u8 *signer_record(const SignerView &sv, long k, u32 keyed, u8 *__restrict__ rec) {
    if (!keyed) return rec;
#pragma unroll
    for (int j = 0; j < 49; j++) rec[j] = sv.cpks[49 * k + j];
    return rec + 49;
}

// ------------------------------------------------------------------------------------------
#ifndef SSA_NO_KERNELS
__global__ void __launch_bounds__(256, 4)    // four waves per SIMD: 128 VGPRs (the S-box blocks own v72..v127)
ssa_k_hash(const DevParams *__restrict__ prm, const u8 *__restrict__ sigs,
           const u8 *__restrict__ pks, MsgView mv, size_t n, u64 *__restrict__ h_out,
           u8 *__restrict__ digest_out, const u32 *__restrict__ key_idx, u32 n_keys) {
    __shared__ u64 lds[RS_LDS_U64];
    u64 *A = lds + threadIdx.x, *B = A;   // the MDS layer works in place (rescue.hpp)
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    bool ok = true;
    // keyed context: the signer's key is row key_idx[i] of the key set (an index out of range hashes row 0; the
    // verification kernel reports it)
    const size_t prow = key_idx ? (size_t)(key_idx[i] < n_keys ? key_idx[i] : 0u) : i;
    const fp6 rx = ld_fp6(sigs + 81 * i, ok);
    const fp6 px = ld_fp6(pks + 96 * prow, ok);
    const u64 py0 = ld_u64_le(pks + 96 * prow + 48);
    u32 len;
    const u8 *m = msg_ptr(mv, i, len);
    u64 d[4];
    hash_message_lane(A, B, prm, rx, px, py0, m, len, d);
    if (digest_out) {  // Digest::to_bytes, src/signature.rs:305
#pragma unroll
        for (int k = 0; k < 4; k++) st_u64_le(digest_out + 32 * i + 8 * k, d[k]);
    }
    if (h_out) {       // Scalar::from_bits_vartime, src/signature.rs:189-192
        sc256 h;
#pragma unroll
        for (int k = 0; k < 4; k++) h.w[k] = d[k];
        h = sc_reduce256(h);
#pragma unroll
        for (int k = 0; k < 4; k++) h_out[4 * i + k] = h.w[k];
    }
}
#endif  // SSA_NO_KERNELS

#ifndef SSA_NO_KERNELS
__global__ void __launch_bounds__(256, 4)
ssa_k_rescue(const DevParams *__restrict__ prm, const u64 *__restrict__ felts, u32 per_row,
             size_t n, u64 *__restrict__ out) {
    __shared__ u64 lds[RS_LDS_U64];
    u64 *A = lds + threadIdx.x, *B = A;   // the MDS layer works in place (rescue.hpp)
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const u64 *row = felts + (size_t)per_row * i;
    u64 d[4];
    sponge_hash(A, B, prm, per_row, [&](u32 idx) -> u64 { return row[idx]; }, d);
#pragma unroll
    for (int k = 0; k < 4; k++) out[4 * i + k] = d[k];
}
#endif  // SSA_NO_KERNELS

// ------------------------------------------------------------------------------------------
// per-lane table rows
SSA_DEV void st_jac(u64 *__restrict__ row, const jac &p) {
    ulonglong2 *q = reinterpret_cast<ulonglong2 *>(row);
#pragma unroll
    for (int i = 0; i < 3; i++) {
        q[i] = make_ulonglong2(p.X.c[2 * i], p.X.c[2 * i + 1]);
        q[3 + i] = make_ulonglong2(p.Y.c[2 * i], p.Y.c[2 * i + 1]);
        q[6 + i] = make_ulonglong2(p.Z.c[2 * i], p.Z.c[2 * i + 1]);
    }
}
SSA_DEV jac ld_jac(const u64 *__restrict__ row) {
    const ulonglong2 *q = reinterpret_cast<const ulonglong2 *>(row);
    jac p;
#pragma unroll
    for (int i = 0; i < 3; i++) {
        ulonglong2 a = q[i], b = q[3 + i], c = q[6 + i];
        p.X.c[2 * i] = a.x; p.X.c[2 * i + 1] = a.y;
        p.Y.c[2 * i] = b.x; p.Y.c[2 * i + 1] = b.y;
        p.Z.c[2 * i] = c.x; p.Z.c[2 * i + 1] = c.y;
    }
    return p;
}
SSA_DEV aff ld_aff(const u64 *__restrict__ row) {
    const ulonglong2 *q = reinterpret_cast<const ulonglong2 *>(row);
    aff p;
#pragma unroll
    for (int i = 0; i < 3; i++) {
        ulonglong2 a = q[i], b = q[3 + i];
        p.x.c[2 * i] = a.x; p.x.c[2 * i + 1] = a.y;
        p.y.c[2 * i] = b.x; p.y.c[2 * i + 1] = b.y;
    }
    return p;
}

SSA_DEV void st_f6(u64 *__restrict__ p, const fp6 &a) {
    ulonglong2 *q = reinterpret_cast<ulonglong2 *>(p);
#pragma unroll
    for (int i = 0; i < 3; i++) q[i] = make_ulonglong2(a.c[2 * i], a.c[2 * i + 1]);
}
SSA_DEV fp6 ld_f6(const u64 *__restrict__ p) {
    const ulonglong2 *q = reinterpret_cast<const ulonglong2 *>(p);
    fp6 a;
#pragma unroll
    for (int i = 0; i < 3; i++) {
        ulonglong2 v = q[i];
        a.c[2 * i] = v.x;
        a.c[2 * i + 1] = v.y;
    }
    return a;
}
SSA_DEV void st_aff(u64 *__restrict__ row, const aff &p) {
    st_f6(row, p.x);
    st_f6(row + 6, p.y);
}

// a Jacobian point in a table row (X, Y in the first line, Z in the second); st_jac / ld_jac are the dense
// 18-word records of the MSM buffers
SSA_DEV void st_row(u64 *__restrict__ row, const jac &p) {
    st_f6(row, p.X);
    st_f6(row + 6, p.Y);
    st_f6(row + PTAB_Z, p.Z);
}
SSA_DEV jac ld_row(const u64 *__restrict__ row) {
    jac p;
    p.X = ld_f6(row);
    p.Y = ld_f6(row + 6);
    p.Z = ld_f6(row + PTAB_Z);
    return p;
}

// row-to-row point operations used only while building the table (cold code, kept out of line)
SSA_FN void tab_dbl(u64 *__restrict__ dst, const u64 *__restrict__ src) { st_row(dst, jac_dbl(ld_row(src))); }
SSA_FN void tab_madd(u64 *__restrict__ dst, const u64 *__restrict__ src, const u64 *__restrict__ paff) {
    st_row(dst, jac_madd(ld_row(src), ld_aff(paff)));
}

// The table of a GENERIC key without the Jacobian detour: affine doublings / additions whose denominators are inverted
// together -- 2P alone, then {3P = 2P + P, 4P = 2(2P)}, then {5P = 4P + P, 6P = 2(3P), 7P = 4P + 3P, 8P = 2(4P)}:
// three Fp6 inversions + 26 products + 11 squarings (~27 k instructions) instead of four Jacobian doublings, three
// mixed additions, one inversion and seven normalisations (~52 k).  A zero denominator (keys of order 2 or 5: some
// multiple is the identity or two operands coincide) makes it return false before anything is relied upon, and the
// caller builds the table the exact, slower way.
SSA_DEV fp6 aff_dbl_num(const fp6 &x) {          // 3 x^2 + a, a = 1
    const fp6 xx = f6_sqr(x);
    fp6 n = f6_add(f6_dbl(xx), xx);
    n.c[0] = fp_add(n.c[0], 1ull);
    return n;
}
SSA_DEV aff aff_from_slope(const fp6 &l, const fp6 &x1, const fp6 &y1, const fp6 &x2) {   // x3 = l^2 - x1 - x2
    aff r;
    r.x = f6_sub(f6_sub(f6_sqr(l), x1), x2);
    r.y = f6_sub(f6_mul(l, f6_sub(x1, r.x)), y1);
    return r;
}
SSA_DEV void st_tab_entry(u64 *__restrict__ row, const aff &a) {
    st_aff(row, a);
    st_f6(row + PTAB_NEG, a.x);
    st_f6(row + PTAB_NY, f6_neg(a.y));
}
// 9P .. 16P from the finished rows 1P .. 8P with ONE more shared inversion: mP = 8P + (m - 8)P for odd m, mP = 2 (m/2)P
// for even m -- eight denominators x8 - x_(m-8) / 2 y_(m/2), their prefix products parked in the rows' second lines
// (scratch until st_tab_entry writes the negative entry there), Montgomery's trick backwards.  Rolled loops: this runs
// once per lane and must not cost registers or code.  A zero denominator (keys of small order) returns false before any
// row of the upper half is final, and the caller builds the table the exact way.
SSA_DEV bool build_ptab_affine_upper(u64 *__restrict__ tab) {
    constexpr int R = PTAB_ENTRY_U64;
    const aff p8 = ld_aff(tab + 7 * R);
    fp6 c = f6_one();
#pragma unroll 1
    for (int m = 9; m <= 16; m++) {
        const aff b = ld_aff(tab + (((m & 1) ? m - 8 : m / 2) - 1) * R);
        const fp6 d = (m & 1) ? f6_sub(p8.x, b.x) : f6_dbl(b.y);
        st_f6(tab + (m - 1) * R + PTAB_Z, d);
        c = f6_mul(c, d);
        st_f6(tab + (m - 1) * R + PTAB_C, c);
    }
    if (f6_is_zero(c)) return false;
    fp6 inv = f6_inv(c);
#pragma unroll 1
    for (int m = 16; m >= 9; m--) {
        fp6 di = inv;                                                      // 1 / d_m = inv * prefix_(m-1)
        if (m > 9) di = f6_mul(inv, ld_f6(tab + (m - 2) * R + PTAB_C));
        inv = f6_mul(inv, ld_f6(tab + (m - 1) * R + PTAB_Z));
        const aff b = ld_aff(tab + (((m & 1) ? m - 8 : m / 2) - 1) * R);
        aff r;
        if (m & 1) r = aff_from_slope(f6_mul(f6_sub(p8.y, b.y), di), b.x, b.y, p8.x);
        else r = aff_from_slope(f6_mul(aff_dbl_num(b.x), di), b.x, b.y, b.x);
        // the row's own scratch (its denominator; its prefix product served row m + 1, done before) is dead now: the
        // finished entry and its negative go straight in (operands of the rows still to come are rows 1..8 only)
        st_tab_entry(tab + (m - 1) * R, r);
    }
    return true;
}

SSA_DEV bool build_ptab_affine(u64 *__restrict__ tab, const aff &p) {
    constexpr int R = PTAB_ENTRY_U64;
    // 2P
    const fp6 d2 = f6_dbl(p.y);
    if (f6_is_zero(d2)) return false;
    const aff p2 = aff_from_slope(f6_mul(aff_dbl_num(p.x), f6_inv(d2)), p.x, p.y, p.x);
    // 3P = 2P + P, 4P = 2(2P)
    const fp6 a3 = f6_sub(p2.x, p.x), a4 = f6_dbl(p2.y);
    const fp6 t34 = f6_mul(a3, a4);
    if (f6_is_zero(t34)) return false;
    const fp6 i34 = f6_inv(t34);
    const aff p3 = aff_from_slope(f6_mul(f6_sub(p2.y, p.y), f6_mul(i34, a4)), p.x, p.y, p2.x);
    const aff p4 = aff_from_slope(f6_mul(aff_dbl_num(p2.x), f6_mul(i34, a3)), p2.x, p2.y, p2.x);
    // 5P = 4P + P, 6P = 2(3P), 7P = 4P + 3P, 8P = 2(4P)
    const fp6 a5 = f6_sub(p4.x, p.x), a6 = f6_dbl(p3.y), a7 = f6_sub(p4.x, p3.x), a8 = f6_dbl(p4.y);
    const fp6 t56 = f6_mul(a5, a6), t567 = f6_mul(t56, a7), t5678 = f6_mul(t567, a8);
    if (f6_is_zero(t5678)) return false;
    fp6 inv = f6_inv(t5678);
    const fp6 i8 = f6_mul(inv, t567);
    inv = f6_mul(inv, a8);
    const fp6 i7 = f6_mul(inv, t56);
    inv = f6_mul(inv, a7);
    const fp6 i6 = f6_mul(inv, a5), i5 = f6_mul(inv, a6);
    st_tab_entry(tab, p);
    st_tab_entry(tab + 1 * R, p2);
    st_tab_entry(tab + 2 * R, p3);
    st_tab_entry(tab + 3 * R, p4);
    st_tab_entry(tab + 4 * R, aff_from_slope(f6_mul(f6_sub(p4.y, p.y), i5), p.x, p.y, p4.x));
    st_tab_entry(tab + 5 * R, aff_from_slope(f6_mul(aff_dbl_num(p3.x), i6), p3.x, p3.y, p3.x));
    st_tab_entry(tab + 6 * R, aff_from_slope(f6_mul(f6_sub(p4.y, p3.y), i7), p3.x, p3.y, p4.x));
    st_tab_entry(tab + 7 * R, aff_from_slope(f6_mul(aff_dbl_num(p4.x), i8), p4.x, p4.y, p4.x));
    return build_ptab_affine_upper(tab);
}

// Affine multiples 1P..16P of a lane's point into its table rows the EXACT way (keys the affine builder gives up on):
// 8 doublings + 7 mixed additions in Jacobian form, then one shared inversion (Montgomery's trick) to make every entry
// affine.  Multiples that are the identity (P of order <= 16: E(Fp6) has cofactor 2*5*29*...) are stored as
// the (0, 0) sentinel jac_madd understands.
SSA_DEV void build_ptab(u64 *__restrict__ tab, const aff &p, bool p_inf) {
    constexpr int R = PTAB_ENTRY_U64;
    if (p_inf) {
        aff z;
        z.x = f6_zero();
        z.y = f6_zero();
#pragma unroll 1
        for (int e = 0; e < PTAB_ENTRIES; e++) st_tab_entry(tab + e * R, z);
        return;
    }
#ifndef SSA_PTAB_JACOBIAN_ONLY
    if (build_ptab_affine(tab, p)) return;        // every key outside the few of order 2 or 5
#endif
    st_row(tab, jac_from_aff(p));                 // row 0 doubles as affine P: (x, y, Z = 1)
    tab_dbl(tab + 1 * R, tab);                    // 2P
    tab_madd(tab + 2 * R, tab + 1 * R, tab);      // 3P = 2P + P
    tab_dbl(tab + 3 * R, tab + 1 * R);            // 4P
    tab_madd(tab + 4 * R, tab + 3 * R, tab);      // 5P = 4P + P
    tab_dbl(tab + 5 * R, tab + 2 * R);            // 6P
    tab_madd(tab + 6 * R, tab + 5 * R, tab);      // 7P = 6P + P
    tab_dbl(tab + 7 * R, tab + 3 * R);            // 8P
#pragma unroll 1
    for (int m = 9; m <= 16; m++) {               // 9P = 8P + P, 10P = 2 (5P), 11P = 10P + P, ...
        if (m & 1) tab_madd(tab + (m - 1) * R, tab + (m - 2) * R, tab);
        else tab_dbl(tab + (m - 1) * R, tab + (m / 2 - 1) * R);
    }
    // forward pass: prefix products of the (non-zero) Z's, kept in the rows' fourth slot
    fp6 c = f6_one();
#pragma unroll 1
    for (int e = 1; e < PTAB_ENTRIES; e++) {
        fp6 z = ld_f6(tab + e * R + PTAB_Z);
        if (f6_is_zero(z)) z = f6_one();
        c = f6_mul(c, z);
        st_f6(tab + e * R + PTAB_C, c);
    }
    fp6 inv = f6_inv(c);
    // backward pass: 1/Z_e = inv * prefix_{e-1};  inv *= Z_e
#pragma unroll 1
    for (int e = PTAB_ENTRIES - 1; e >= 1; e--) {
        fp6 z = ld_f6(tab + e * R + PTAB_Z);
        const bool zero = f6_is_zero(z);
        if (zero) z = f6_one();
        fp6 zinv = inv;
        if (e > 1) zinv = f6_mul(inv, ld_f6(tab + (e - 1) * R + PTAB_C));
        inv = f6_mul(inv, z);
        const fp6 zi2 = f6_sqr(zinv);
        aff a;
        a.x = f6_mul(ld_f6(tab + e * R), zi2);
        a.y = f6_mul(ld_f6(tab + e * R + 6), f6_mul(zi2, zinv));
        if (zero) {
            a.x = f6_zero();
            a.y = f6_zero();
        }
        st_tab_entry(tab + e * R, a);
    }
    st_tab_entry(tab, p);
}

#include "qnaf.inc"

// [k]P, k < 2^255, from the lane's affine table 1P..16P with signed 5-bit windows (offset recoding): the top digit
// (<= 32) selects its table entry -- two entries above 16 --, then 50 x (5 doublings + 1 mixed addition) with
// every lane in lock-step: 250 doublings + 51 additions (round 3, 4-bit windows over 1P..8P: 252 + 63).
// order_q: [q]P for the subgroup check (is_torsion_free, src/signature.rs:182) -- the scalar is a constant, so its
// schedule is chosen offline: the width-5 NAF of q (qnaf.inc, tools/gen_qnaf.py), 43 additions and 255 doublings with a
// variable number of doublings per window (kr is ignored).  Same loop, same window statement: the
// ladder body exists once in the code.
// The ladder comes in two functions so that the pieces of ssa_k_verify's end game can stop after any window and park the
// accumulator: ladder_init picks the top digit, ladder_steps runs the windows [lo, hi).
constexpr int LADDER_STEPS = 50, LADDER_STEPS_Q = QNAF_LEN - 1;
SSA_DEV jac ladder_init(const u64 *__restrict__ tab, const sc256 &kr, bool order_q) {
    jac acc = jac_identity();
    const u32 top = order_q ? (u32)QNAF_DIGIT[0] : sc_top5(kr);   // in [0, 32]
    if (top != 0) {
        const aff p = ld_aff(tab + ((top > 16u ? 16u : top) - 1u) * PTAB_ENTRY_U64);
        if (!(f6_is_zero(p.x) && f6_is_zero(p.y))) acc = jac_from_aff(p);
        if (top > 16u) acc = jac_madd_fast(acc, ld_aff(tab + (top - 17u) * PTAB_ENTRY_U64));   // 16P + (top - 16)P
    }
    return acc;
}
// (tab by reference: the window statement hands the pointer through and so keeps it in a register, jac_asm.inc; the
// caller goes on with the statement's copy, so that no second copy of it stays live -- in scratch -- across the loop)
SSA_DEV jac ladder_steps(jac acc, const u64 *&tab, const sc256 &kr, bool order_q, int lo, int hi) {
#pragma unroll 1
    for (int it = lo; it < hi; it++) {
        int digit;
        u32 gap;
        if (order_q) {
            digit = (int)QNAF_DIGIT[it + 1];
            gap = (u32)QNAF_GAP[it + 1];
        } else {
            digit = (int)sc_win5(kr, (u32)(49 - it)) - 16;
            gap = 5u;
        }
        const int mag = digit < 0 ? -digit : digit;
#ifdef SSA_JAC_ASM
        // one asm statement per window: `gap` doublings + the addition on the lanes with a non-zero digit; -y comes from
        // the table and the statement gathers its entry itself (six loads issued in front of the doublings, awaited behind
        // them): the loop body outside the statement is the digit and one address
#ifdef SSA_GATHER_HOT    // timing only (wrong results): every window adds entry 0 -- what the gather's HBM latency costs
        const u64 *row = tab;
#else
        const u64 *row = tab + (size_t)((mag ? mag : 1) - 1) * PTAB_ENTRY_U64 + (digit < 0 ? PTAB_NEG : 0);
#endif
        if (__builtin_expect(!jac_window_asm(acc.X.c, acc.Y.c, acc.Z.c, row, (u32)mag, gap, tab), 0)) {
            if (digit != 0) {                            // exceptional inputs: the exact compiled addition
                aff q;
                q.x = ld_f6(row);
                q.y = ld_f6(row + 6);
                acc = jac_madd(acc, q);
            }
        }
#else
        acc = jac_dbl_n(acc, gap);
        if (digit != 0) {
            aff q = ld_aff(tab + (mag - 1) * PTAB_ENTRY_U64);
            q.y = f6_select(digit < 0, q.y, f6_neg(q.y));
            acc = jac_madd_fast(acc, q);
        }
#endif
    }
    return acc;
}
SSA_DEV jac mul_ptab(const u64 *__restrict__ tab_in, const sc256 &k, bool order_q = false) {
    const sc256 kr = sc_recode_offset5(k);
    const u64 *tab = tab_in;
    return ladder_steps(ladder_init(tab, kr, order_q), tab, kr, order_q, 0, order_q ? LADDER_STEPS_Q : LADDER_STEPS);
}

// The mixed addition on a comb table's entry: the statement gathers the entry itself and touches the one the NEXT
// addition will want (jac_asm.inc: jac_madd_gather_asm) -- comb entries lie at random places of tables far larger than
// the caches, and an addition that waits for its operand in front of the statement waits for the whole HBM latency.
// (base by reference: the statement hands the table's base through in a register, as the ladder's window does)
SSA_DEV jac jac_madd_gather(const jac &p, const u64 *row, const u64 *next, const u64 *&base) {
#ifdef SSA_JAC_ASM
    jac r = p;
    if (__builtin_expect(jac_madd_gather_asm(r.X.c, r.Y.c, r.Z.c, row, next, base) != 0, 1)) return r;
    return jac_madd(r, ld_aff(row));      // r is untouched: identity, (0, 0) entries, P == +-Q
#else
    (void)next;
    (void)base;
    return jac_madd(p, ld_aff(row));
#endif
}

// acc += sum over the windows of k of table[w][window w of k]: one mixed addition per non-zero window (`count` windows of
// `bits` bits, entry d of window w at base + ((w << bits) + d) * 12)
SSA_DEV jac comb_add(jac acc, const u64 *__restrict__ base_in, const sc256 &k, u32 bits, u32 count, bool hot = false) {
    const u64 *base = base_in;
#pragma unroll 1
    for (u32 w = 0; w < count; w++) {
        const u32 d = sc_bits(k, w * bits, bits);
        if (d != 0) {
            const u32 w1 = w + 1 < count ? w + 1 : w;      // (the last addition touches its own entry again)
            const u64 *next = base + (((size_t)w1 << bits) + sc_bits(k, w1 * bits, bits)) * 12;
#ifdef SSA_COMB_HOT       // timing only (wrong results): every window adds the same entry -- what the comb gathers' latency costs
            const u64 *row = base + (hot ? (size_t)12 : (((size_t)w << bits) + d) * 12);
#else
            const u64 *row = base + (((size_t)w << bits) + d) * 12;
#endif
            acc = jac_madd_gather(acc, row, next, base);
        }
    }
    return acc;
}

// acc += [e]G from the comb table of the generator (the table's own geometry)
SSA_DEV jac add_base_mul(jac acc, const u64 *__restrict__ gtab, const sc256 &e, bool hot = false) {
    const GtabGeom gg = gtab_geom(gtab);
    return comb_add(acc, gtab, e, gg.bits, gg.count, hot);
}

// CompressedPoint flag byte of a signature's x under verify_batch semantics (SSA_FLAG_SIG_FLAG_BYTE): the
// reference decompresses R with it (AffinePoint::from_compressed(&sig.x).unwrap(), src/batch.rs:104), so the batch
// equation only holds for the R the flag selects.  0 = well-formed, 3 = from_compressed is None (the reference panics).
SSA_DEV u32 sig_flag_precheck(u32 flag, bool x_is_zero) {
    if (flag & 0x3fu) return ST_MALFORMED;
    if ((flag & 0x80u) && (!x_is_zero || (flag & 0x40u))) return ST_MALFORMED;
    return ST_OK;
}
// sort bit of the affine y of a finite Jacobian point (cold: one Fp6 inversion)
SSA_FN bool jac_y_lex_largest(const jac &p) {
    const fp6 zi = f6_inv(p.Z);
    const fp6 y = f6_mul(p.Y, f6_mul(zi, f6_sqr(zi)));
    return f6_lex_largest(y);
}

// x is the abscissa of a curve point: x^3 + x + (u + 395) is a square (cold: rejected lanes of the flag-byte mode)
SSA_FN bool x_on_curve(const fp6 &x) {
    fp6 rhs = f6_add(f6_mul(f6_sqr(x), x), x);
    rhs.c[0] = fp_add(rhs.c[0], 395ull);
    rhs.c[1] = fp_add(rhs.c[1], 1ull);
    return f6_is_square(rhs);
}

constexpr u32 VF_CHECK_TORSION = 1u, VF_SIG_FLAG_BYTE = 8u;
#ifdef SSA_WAVE_TIMES
constexpr size_t SSA_WAVE_TIMES_MAX = 1u << 16;
__device__ unsigned long long g_wave_times[3 * SSA_WAVE_TIMES_MAX];
// ... and where an ORDINARY wave's time goes (tools/wave_times.py --phases): start, table built, ladder done, end
__device__ unsigned long long g_phase_times[4 * SSA_WAVE_TIMES_MAX];
#define SSA_PHASE_MARK(k) do { if (!in_piece && lane == 0 && (size_t)blockIdx.x * 4u + (threadIdx.x >> 6) < SSA_WAVE_TIMES_MAX) \
    g_phase_times[4 * ((size_t)blockIdx.x * 4u + (threadIdx.x >> 6)) + (k)] = wall_clock64(); } while (0)
#else
#define SSA_PHASE_MARK(k) do { } while (0)
#endif

// ------------------------------------------------------------------------------------------
// The end game of a launch (round 5).  A launch of one workgroup per 256 lanes ends with every SIMD finishing its last
// wave alone -- the sequencer serves the older wave of a SIMD first (76 % of the issue slots), so the younger one has
// most of its 3.2 ms ahead of it when its neighbour leaves, and a lone wave issues every 6.2 cycles instead of 4: 0.65 ms
// of a 26.6 ms launch (profiles/r05/job_sched_ab.txt).  What the scheduler experiment of this round showed is that SHORT
// last jobs cure it and that persistent waves and jobs in pieces everywhere cost more than they bring.  So, statically:
// the LAST generation of lanes (the tail groups: as many 64-lane groups as there are resident waves) is cut into pieces at
// window boundaries of the ladder -- the first half of the work, then a quarter, an eighth, ... -- ; the workgroups of the
// first pieces open the grid, where they are ordinary waves among ordinary waves, and all the other pieces close it,
// piece-major: the kernel ends with half a generation of work in waves that get shorter and shorter, which is what it takes
// to fill the staircase the SIMDs' slots free up in (they end a generation 2 ms apart).  Between two pieces a lane's
// accumulator and status are parked in HBM, lane-interleaved; the lanes' tables stay where they are.  Everything else is
// the launch it always was: no counter, no persistent wave.
//   grid: [piece 0][ordinary workgroups][piece 1][piece 2] ... [piece P-1]; a piece workgroup runs four tail groups.
// done[g] counts the finished pieces of tail group g (release after the parked state and, for piece 0, the tables are
// written; acquire before they are read: the XCDs' L2s are not coherent with each other), and a wave whose predecessor has
// not finished sleeps on the flag.  Workgroups are dispatched in grid order, so the predecessor started long before;
// liveness does not rest on that: pieces are CLAIMED (done[K + g] = first unclaimed piece of group g), a wave takes any
// earlier piece nobody has claimed along with its own, and therefore only ever waits for a piece a running wave holds.
constexpr int VP_MAX = 8;
struct TailPlan {
    u32 n_pieces;            // 0: no end game (every workgroup is an ordinary one)
    u32 tail_groups;         // K: 64-lane groups at the end of the batch that run in pieces (a multiple of 4)
    u32 main_blocks;         // ordinary workgroups (256 lanes each): lanes [0, 256 * main_blocks)
    u32 ph[VP_MAX];          // piece p: pass | first-of-pass << 1 | last-of-pass << 2 | it_lo << 8 | it_hi << 16
    u32 whole[2];            // the same descriptor for a whole pass 0 / pass 1 (ordinary workgroups)
    u32 reversed;            // test hook (SSA_TAIL_REVERSED=1): roles dealt from the END of the grid, the worst dispatch order
};
__host__ __device__ inline u32 tail_grid_blocks(const TailPlan &tp) { return tp.main_blocks + tp.n_pieces * (tp.tail_groups / 4u); }
struct BlockRole {
    u32 piece;               // piece index, or 0xffffffff for an ordinary workgroup
    u32 index;               // ordinary: its number among the ordinary workgroups; piece: its number among the piece's
};
SSA_DEV BlockRole tail_role(const TailPlan &tp, u32 blk) {
    // grid: [piece 0 of the tail groups][the ordinary workgroups][piece 1][piece 2] ... [piece P-1]
    BlockRole r;
    r.piece = 0xffffffffu;
    r.index = blk;
    if (tp.n_pieces == 0) return r;
    const u32 pb = tp.tail_groups / 4u;
    if (blk < pb) {
        r.piece = 0;
        return r;
    }
    if (blk < pb + tp.main_blocks) {
        r.index = blk - pb;
        return r;
    }
    const u32 q = blk - pb - tp.main_blocks;
    r.piece = 1u + q / pb;
    r.index = q - (r.piece - 1u) * pb;
    return r;
}
constexpr int PARK_WORDS = 19;   // X, Y, Z of a lane's accumulator and its status word; word w of lane l of tail group e
                                 // at park[(e * PARK_WORDS + w) * 64 + l]
// the parked state is written with agent-scope stores (write-through past the XCD's L2)
SSA_DEV void st_shared(u64 *__restrict__ p, u64 v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
SSA_DEV void park_store(u64 *__restrict__ pk, const jac &r) {
#pragma unroll
    for (int k = 0; k < 6; k++) {
        st_shared(pk + k * 64, r.X.c[k]);
        st_shared(pk + (6 + k) * 64, r.Y.c[k]);
        st_shared(pk + (12 + k) * 64, r.Z.c[k]);
    }
}
SSA_DEV jac park_load(const u64 *__restrict__ pk) {
    jac r;
#pragma unroll
    for (int k = 0; k < 6; k++) {
        r.X.c[k] = pk[k * 64];
        r.Y.c[k] = pk[(6 + k) * 64];
        r.Z.c[k] = pk[(12 + k) * 64];
    }
    return r;
}

#ifndef SSA_NO_KERNELS
__global__ void __launch_bounds__(256, 2)
ssa_k_verify(const u8 *__restrict__ sigs, const u8 *__restrict__ pks,
             const u8 *__restrict__ pk_inf, const u64 *__restrict__ h_in,
             const u64 *__restrict__ gtab, u64 *__restrict__ ws_tab, size_t n, u32 flags,
             u8 *__restrict__ status_out, unsigned long long *__restrict__ n_fail,
             TailPlan tp, u32 *__restrict__ done, u64 *__restrict__ park) {
#ifdef SSA_WAVE_TIMES       // diagnostic build only (tools/wave_times.py): when and where every wave of the kernel ran
    const unsigned long long wt0 = wall_clock64();
#endif
    // which lanes, which pieces: an ordinary workgroup runs its 256 lanes from start to end; a piece workgroup runs one
    // piece of four tail groups (wave w: tail group 4 * index + w).  (Measured and dropped: the closing waves pulling
    // their (piece, group) jobs from a counter until it runs dry, so that the faster XCDs take more -- the XCDs then do
    // finish together, 0.4 ms LATER: profiles/r05/end_game_ab.txt.)
    const BlockRole role = tail_role(tp, tp.reversed ? gridDim.x - 1u - blockIdx.x : blockIdx.x);
    const u32 lane = threadIdx.x & 63u;
    const bool in_piece = role.piece != 0xffffffffu;
    const u32 p_lo = in_piece ? role.piece : 0u;
    const u32 eg = in_piece ? 4u * role.index + (threadIdx.x >> 6) : 0u;                  // tail group (pieces only)
    const size_t i = in_piece ? ((size_t)tp.main_blocks * 256u + (size_t)eg * 64u + lane)
                              : ((size_t)role.index * blockDim.x + threadIdx.x);
    const bool runs_last = !in_piece || p_lo + 1u == tp.n_pieces;                         // this wave delivers the status
    const bool in = i < n;
    u64 *pk = park + ((size_t)eg * PARK_WORDS) * 64 + lane;
    u64 *tab = ws_tab + i * (size_t)(PTAB_ENTRIES * PTAB_ENTRY_U64);
    u32 status = ST_OK;
    bool ok_sig = true;
    jac r = jac_identity();
    // Which pieces this wave runs: its own -- and any earlier piece of the group that nobody has CLAIMED yet.  Every piece
    // wave claims at its start (next[g] = first unclaimed piece of tail group g, one compare-and-swap per wave).  In grid
    // order the predecessor has claimed piece p_lo - 1 long ago and this wave claims exactly p_lo; if a dispatcher ever
    // started this workgroup BEFORE its predecessor's, the wave takes the unclaimed pieces too and the late-comer, finding
    // its piece claimed, leaves at once.  So a wave only ever waits for pieces that a RUNNING wave has claimed: every wave of
    // the grid reaches its end whatever the dispatch order, and no piece is run twice.
    u32 run_lo = p_lo;
    if (in_piece) {
        u32 *next = done + tp.tail_groups + eg;
        u32 cur = 0;
        if (lane == 0) {
            cur = __hip_atomic_load(next, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            while (cur <= p_lo) {
                const u32 seen = atomicCAS(next, cur, p_lo + 1u);
                if (seen == cur) break;
                cur = seen;
            }
        }
        cur = (u32)__builtin_amdgcn_readfirstlane((int)cur);
        if (cur > p_lo) return;                       // another wave runs this piece
        run_lo = cur;
    }
    if (in_piece && run_lo > 0) {
        // (the wait itself relaxed, ONE acquire behind it: an acquiring load invalidates the XCD's L2 every time it is issued)
        while (__hip_atomic_load(done + eg, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < run_lo) __builtin_amdgcn_s_sleep(64);
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // (the invalidate completes asynchronously: MI355X_MICROARCH.md)
        const u64 sw = pk[18 * 64];
        status = (u32)(sw & 0xffu);
        ok_sig = ((sw >> 8) & 1u) != 0;
        if (in && status == ST_OK && !(tp.ph[run_lo] & 2u)) r = park_load(pk);            // (a pass's first piece starts afresh)
    } else if (in) {
        // check order of the reference (src/signature.rs:181-205): the key first (subgroup check, :182),
        // then the signature's x (Fp6::from_bytes(..).unwrap() panics at :186 -> SSA_MALFORMED)
        bool ok = true;
        const fp6 xs = ld_fp6(sigs + 81 * i, ok_sig);
        const sc256 e = ld_sc(sigs + 81 * i + 49);
        ok_sig = ok_sig && !sc_geq_q(e);
        const u32 fbyte = sigs[81 * i + 48];
        if ((flags & VF_SIG_FLAG_BYTE) && ok_sig) ok_sig = sig_flag_precheck(fbyte, f6_is_zero(xs)) == ST_OK;
        aff P;
        P.x = ld_fp6(pks + 96 * i, ok);
        P.y = ld_fp6(pks + 96 * i + 48, ok);
        const bool inf = pk_inf && pk_inf[i];
        if (ok && !inf) ok = aff_on_curve(P);
        if (!ok) status = ST_MALFORMED;
        else build_ptab(tab, P, inf);
    }
    SSA_PHASE_MARK(1);
    // pass 0 (only with SSA_FLAG_CHECK_TORSION): [q]P == O, is_torsion_free, :182-184 -- the offline schedule of the
    // constant q; pass 1: [h]P.  One rolled loop (ladder_steps) so that the ladder body exists once in the code.
    if (in && status == ST_OK) {
        sc256 h;
#pragma unroll
        for (int k = 0; k < 4; k++) h.w[k] = h_in[4 * i + k];
        const sc256 kr = sc_recode_offset5(h);
        // the descriptors this wave runs: one piece, or the whole passes (pass 0 only with the subgroup check)
        const u32 d_lo = in_piece ? run_lo : ((flags & VF_CHECK_TORSION) ? 0u : 1u);
        const u32 d_hi = in_piece ? p_lo + 1u : 2u;
        const u64 *ltab = tab;                              // (the ladder's copy: ladder_steps)
#pragma unroll 1
        for (u32 k = d_lo; k < d_hi; k++) {
            const u32 d = in_piece ? tp.ph[k] : tp.whole[k];
            const bool pass_q = (d & 1u) == 0, first = (d & 2u) != 0, last = (d & 4u) != 0;
            if (first) {
                if (!pass_q && !ok_sig) {
                    status = ST_MALFORMED;
                    break;
                }
                r = ladder_init(ltab, kr, pass_q);
            }
            r = ladder_steps(r, ltab, kr, pass_q, (int)((d >> 8) & 0xffu), (int)((d >> 16) & 0xffu));
            if (last && pass_q && !jac_is_identity(r)) {
                status = ST_INVALID_PK;
                break;
            }
        }
    }
    SSA_PHASE_MARK(2);
    if (runs_last) {
        if (in) {
            if (status == ST_OK) {
                bool okx = true;
                const fp6 xs = ld_fp6(sigs + 81 * i, okx);
                const sc256 e = ld_sc(sigs + 81 * i + 49);
                const u32 fbyte = sigs[81 * i + 48];
#ifdef SSA_COMB_HOT
                r = add_base_mul(r, gtab, e, true);
#else
                r = add_base_mul(r, gtab, e);               // + [e]G, :196-198
#endif
                // r.get_x() == x_felt (:200): X == x * Z^2; the identity's x is taken as 0
                bool eq;
                if (flags & VF_SIG_FLAG_BYTE) {
                    // verify_batch semantics: R is the point sig.x's flag byte selects (src/batch.rs:104)
                    if (fbyte & 0x80u) {
                        eq = jac_is_identity(r);
                    } else {
                        eq = !jac_is_identity(r) && f6_eq(r.X, f6_mul(xs, f6_sqr(r.Z)));
                        if (eq) eq = jac_y_lex_largest(r) == ((fbyte & 0x40u) != 0);
                        // an x with no curve point: from_compressed is None, the reference panics
#ifndef SSA_COMB_HOT
                        else if (!x_on_curve(xs)) ok_sig = false;
#endif
                    }
                } else if (jac_is_identity(r)) {
                    eq = f6_is_zero(xs);
                } else {
                    eq = f6_eq(r.X, f6_mul(xs, f6_sqr(r.Z)));
                }
                status = eq ? ST_OK : (ok_sig ? ST_INVALID_SIG : ST_MALFORMED);
            }
            status_out[i] = (u8)status;
        }
        // aggregate verdict: one ballot + one atomic per wave
        const unsigned long long bad = __ballot(status != ST_OK);
        if (lane == 0 && bad) atomicAdd(n_fail, (unsigned long long)__popcll(bad));
    } else {
        // park the lane and publish the piece: the first piece has written the lanes' tables with ordinary stores and
        // needs the XCD's L2 written back (release at agent scope); later pieces wrote only the parked words, which are
        // agent-scope (write-through) stores already, and the flag just has to follow their completion
        if (in && status == ST_OK) park_store(pk, r);
        st_shared(pk + 18 * 64, (u64)status | ((u64)(ok_sig ? 1u : 0u) << 8));
        // the hand-off in the form the platform guide gives as valid (MI355X_MICROARCH.md "Valid forms"): this wave's stores
        // drained, then -- where ordinary stores (the tables) are handed over -- the agent-scope release and ITS drain,
        // then the flag as a relaxed agent-scope store.  The waits are written out: the compiler may drop the one behind a
        // release when its own scoreboard is empty, and it knows nothing of the loads and stores of the asm statements.
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (run_lo == 0) {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        __hip_atomic_store(done + eg, p_lo + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
#ifdef SSA_WAVE_TIMES
    SSA_PHASE_MARK(3);
    if (lane == 0) {
        const size_t w = (size_t)blockIdx.x * (blockDim.x / 64u) + (threadIdx.x >> 6);
        if (w < SSA_WAVE_TIMES_MAX) {
            if (!in_piece) g_phase_times[4 * w] = wt0;
            g_wave_times[3 * w] = wt0;
            g_wave_times[3 * w + 1] = wall_clock64();
            g_wave_times[3 * w + 2] = ((unsigned long long)__builtin_amdgcn_s_getreg((20 << 0) | (0 << 6) | (31 << 11)) << 32) |
                                      (unsigned long long)__builtin_amdgcn_s_getreg((4 << 0) | (0 << 6) | (31 << 11));   // XCC_ID, HW_ID
        }
    }
#endif
}
#endif  // SSA_NO_KERNELS

// ------------------------------------------------------------------------------------------
// Keyed context (repeated public keys: validator sets; the reference's own batch test reuses keys,
// src/batch.rs:152-175).  ssa_k_keyset_build runs ONCE per key what ssa_k_verify runs per signature: limb and
// curve checks, the subgroup check [q]P == O (src/signature.rs:182-184) and the affine table 1P..8P.
// ssa_k_verify_keyed then starts at the ladder: no table build, no [q]P pass.
//   key_status: 0 usable, 1 not in the prime subgroup (InvalidPublicKey), 3 malformed
#ifndef SSA_NO_KERNELS
__global__ void __launch_bounds__(256, 2)
ssa_k_keyset_build(const u8 *__restrict__ pks, const u8 *__restrict__ pk_inf, size_t m, u64 *__restrict__ key_tab,
                   u8 *__restrict__ key_status) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    bool ok = true;
    aff P;
    P.x = ld_fp6(pks + 96 * i, ok);
    P.y = ld_fp6(pks + 96 * i + 48, ok);
    const bool inf = pk_inf && pk_inf[i];
    if (ok && !inf) ok = aff_on_curve(P);
    u32 st = ST_MALFORMED;
    if (ok) {
        u64 *tab = key_tab + i * (size_t)(PTAB_ENTRIES * PTAB_ENTRY_U64);
        build_ptab(tab, P, inf);
        sc256 q;
#pragma unroll
        for (int j = 0; j < 4; j++) q.w[j] = SC_Q(j);
        st = jac_is_identity(mul_ptab(tab, q, true)) ? ST_OK : ST_INVALID_PK;
    }
    key_status[i] = (u8)st;
}

__global__ void __launch_bounds__(256, 2)
ssa_k_verify_keyed(const u8 *__restrict__ sigs, const u32 *__restrict__ key_idx, const u64 *__restrict__ key_tab,
                   const u8 *__restrict__ key_status, u32 n_keys, const u64 *__restrict__ h_in,
                   const u64 *__restrict__ gtab, size_t n, u32 flags, u8 *__restrict__ status_out,
                   unsigned long long *__restrict__ n_fail) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    u32 status = ST_OK;
    if (i < n) {
        bool ok_sig = true;
        const fp6 xs = ld_fp6(sigs + 81 * i, ok_sig);
        const sc256 e = ld_sc(sigs + 81 * i + 49);
        ok_sig = ok_sig && !sc_geq_q(e);
        const u32 fbyte = sigs[81 * i + 48];
        if ((flags & VF_SIG_FLAG_BYTE) && ok_sig) ok_sig = sig_flag_precheck(fbyte, f6_is_zero(xs)) == ST_OK;
        const u32 k = key_idx[i];
        const u32 ks = k < n_keys ? (u32)key_status[k] : ST_MALFORMED;
        // the order of Signature::verify: the key first (src/signature.rs:182), then the signature's x (:186)
        if (ks == ST_MALFORMED) status = ST_MALFORMED;
        else if (ks == ST_INVALID_PK && (flags & VF_CHECK_TORSION)) status = ST_INVALID_PK;
        else if (!ok_sig) status = ST_MALFORMED;
        if (status == ST_OK) {
            const u64 *tab = key_tab + (size_t)k * (size_t)(PTAB_ENTRIES * PTAB_ENTRY_U64);
            sc256 h;
#pragma unroll
            for (int j = 0; j < 4; j++) h.w[j] = h_in[4 * i + j];
            jac r = mul_ptab(tab, h);
            r = add_base_mul(r, gtab, e);
            bool eq;
            if (flags & VF_SIG_FLAG_BYTE) {
                if (fbyte & 0x80u) {
                    eq = jac_is_identity(r);
                } else {
                    eq = !jac_is_identity(r) && f6_eq(r.X, f6_mul(xs, f6_sqr(r.Z)));
                    if (eq) eq = jac_y_lex_largest(r) == ((fbyte & 0x40u) != 0);
                    else if (!x_on_curve(xs)) ok_sig = false;
                }
            } else if (jac_is_identity(r)) {
                eq = f6_is_zero(xs);
            } else {
                eq = f6_eq(r.X, f6_mul(xs, f6_sqr(r.Z)));
            }
            status = eq ? ST_OK : (ok_sig ? ST_INVALID_SIG : ST_MALFORMED);
        }
        status_out[i] = (u8)status;
    }
    const unsigned long long bad = __ballot(status != ST_OK);
    if ((threadIdx.x & 63u) == 0 && bad) atomicAdd(n_fail, (unsigned long long)__popcll(bad));
}
#endif  // SSA_NO_KERNELS

// Per-key comb (keyed context, few keys): ktab[key][w][d] = affine [d * 2^(16 w)] P_key, w < 16, d < 65536 (100 MB per
// key -- round 4; 32 windows of 8 bits, 768 KB per key, before --; identity entries -- d = 0, identity keys, multiples of
// small-order keys that vanish -- are the (0, 0) sentinel).  [h]P is then 16 mixed additions and NO doublings: a
// signature costs 27 additions instead of 250 doublings + 62 additions.  Built like the comb for G: a base table
// kbase[key][w'][d] = [d 2^(8 w')] P_key (w' < 32, d < 256: round 3's whole table) by double-and-add, then one affine
// addition per entry -- exact for ANY key: a lane whose eight denominators include a zero (keys of small order: the two
// parts can coincide or cancel) adds its entries with the complete Jacobian formulas instead.
constexpr int KB_BITS = 8, KB_COUNT = 32;
constexpr size_t KBASE_ENTRIES_PER_KEY = (size_t)KB_COUNT << KB_BITS;
constexpr int KW_BITS = 16, KW_COUNT = 16;
constexpr size_t KTAB_ENTRIES_PER_KEY = (size_t)KW_COUNT << KW_BITS;

#ifndef SSA_NO_KERNELS
__global__ void __launch_bounds__(256)
ssa_k_keycomb_base(const u8 *__restrict__ pks, const u8 *__restrict__ pk_inf, const u8 *__restrict__ key_status,
                    size_t m, u64 *__restrict__ kbase) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= m * KBASE_ENTRIES_PER_KEY) return;
    const size_t key = t / KBASE_ENTRIES_PER_KEY;
    const u32 w = (u32)((t >> KB_BITS) % KB_COUNT), d = (u32)(t & ((1u << KB_BITS) - 1u));
    aff a;
    a.x = f6_zero();
    a.y = f6_zero();
    const bool inf = pk_inf && pk_inf[key];
    if (key_status[key] != ST_MALFORMED && !inf && d != 0) {
        bool ok = true;
        aff P;
        P.x = ld_fp6(pks + 96 * key, ok);
        P.y = ld_fp6(pks + 96 * key + 48, ok);
        jac acc = jac_identity();
#pragma unroll 1
        for (int b = KB_BITS - 1; b >= 0; b--) {
            acc = jac_dbl(acc);
            if ((d >> b) & 1u) acc = jac_madd(acc, P);
        }
#pragma unroll 1
        for (u32 k = 0; k < w * KB_BITS; k++) acc = jac_dbl(acc);
        a = jac_to_aff(acc);
    }
    ulonglong2 *q = reinterpret_cast<ulonglong2 *>(kbase + t * 12);
#pragma unroll
    for (int i = 0; i < 3; i++) {
        q[i] = make_ulonglong2(a.x.c[2 * i], a.x.c[2 * i + 1]);
        q[3 + i] = make_ulonglong2(a.y.c[2 * i], a.y.c[2 * i + 1]);
    }
}

// ktab[key][w][d] = kbase[key][2 w + 1][d >> 8] + kbase[key][2 w][d & 255]; a lane takes 8 consecutive entries
__global__ void __launch_bounds__(256)
ssa_k_keycomb_build(const u64 *__restrict__ kbase, size_t m, u64 *__restrict__ ktab) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= m * (KTAB_ENTRIES_PER_KEY / 8)) return;
    const size_t key = t / (KTAB_ENTRIES_PER_KEY / 8), e0 = (t % (KTAB_ENTRIES_PER_KEY / 8)) * 8;
    const u32 w = (u32)(e0 >> KW_BITS), d0 = (u32)(e0 & ((1u << KW_BITS) - 1u));
    const u32 dhi = d0 >> KB_BITS, dlo0 = d0 & ((1u << KB_BITS) - 1u);
    const u64 *kb = kbase + key * KBASE_ENTRIES_PER_KEY * 12;
    const u64 *slo = kb + ((size_t)(2 * w) << KB_BITS) * 12, *shi = kb + ((size_t)(2 * w + 1) << KB_BITS) * 12;
    u64 *out = ktab + (key * KTAB_ENTRIES_PER_KEY + e0) * 12;
    const aff p1 = ld_aff(shi + (size_t)dhi * 12);
    const bool p1_inf = f6_is_zero(p1.x) && f6_is_zero(p1.y);
    if (p1_inf) {                                     // no high part (d_hi = 0, an identity key, a vanished multiple): copies
#pragma unroll 1
        for (int k = 0; k < 8; k++) st_aff(out + 12 * k, ld_aff(slo + (size_t)(dlo0 + k) * 12));
        return;
    }
    // forward: prefix products of the denominators x2 - x1 (1 for an identity low part), parked in the output rows
    fp6 c = f6_one();
    bool degenerate = false;
#pragma unroll 1
    for (int k = 0; k < 8; k++) {
        const aff p2 = ld_aff(slo + (size_t)(dlo0 + k) * 12);
        const bool p2_inf = f6_is_zero(p2.x) && f6_is_zero(p2.y);
        const fp6 a = p2_inf ? f6_one() : f6_sub(p2.x, p1.x);
        degenerate = degenerate || f6_is_zero(a);
        c = f6_mul(c, a);
        st_f6(out + 12 * k, c);
    }
    if (degenerate) {                                 // P1 = +-P2 for some entry: the complete formulas for all eight
#pragma unroll 1
        for (int k = 0; k < 8; k++)
            st_aff(out + 12 * k, jac_to_aff(jac_madd(jac_from_aff(p1), ld_aff(slo + (size_t)(dlo0 + k) * 12))));
        return;
    }
    fp6 inv = f6_inv(c);
#pragma unroll 1
    for (int k = 7; k >= 0; k--) {
        const aff p2 = ld_aff(slo + (size_t)(dlo0 + k) * 12);
        const bool p2_inf = f6_is_zero(p2.x) && f6_is_zero(p2.y);
        const fp6 a = p2_inf ? f6_one() : f6_sub(p2.x, p1.x);
        fp6 ai = inv;
        if (k > 0) ai = f6_mul(inv, ld_f6(out + 12 * (k - 1)));
        inv = f6_mul(inv, a);
        aff r = p1;
        if (!p2_inf) r = aff_from_slope(f6_mul(f6_sub(p2.y, p1.y), ai), p1.x, p1.y, p2.x);
        aff rc;
        rc.x = f6_canon(r.x);
        rc.y = f6_canon(r.y);
        st_aff(out + 12 * k, rc);
    }
}

__global__ void __launch_bounds__(256, 2)
ssa_k_verify_keyed_comb(const u8 *__restrict__ sigs, const u32 *__restrict__ key_idx, const u64 *__restrict__ ktab,
                        const u8 *__restrict__ key_status, u32 n_keys, const u64 *__restrict__ h_in,
                        const u64 *__restrict__ gtab, size_t n, u32 flags, u8 *__restrict__ status_out,
                        unsigned long long *__restrict__ n_fail) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    u32 status = ST_OK;
    if (i < n) {
        bool ok_sig = true;
        const fp6 xs = ld_fp6(sigs + 81 * i, ok_sig);
        const sc256 e = ld_sc(sigs + 81 * i + 49);
        ok_sig = ok_sig && !sc_geq_q(e);
        const u32 fbyte = sigs[81 * i + 48];
        if ((flags & VF_SIG_FLAG_BYTE) && ok_sig) ok_sig = sig_flag_precheck(fbyte, f6_is_zero(xs)) == ST_OK;
        const u32 k = key_idx[i];
        const u32 ks = k < n_keys ? (u32)key_status[k] : ST_MALFORMED;
        if (ks == ST_MALFORMED) status = ST_MALFORMED;
        else if (ks == ST_INVALID_PK && (flags & VF_CHECK_TORSION)) status = ST_INVALID_PK;
        else if (!ok_sig) status = ST_MALFORMED;
        if (status == ST_OK) {
            const u64 *tab = ktab + (size_t)k * KTAB_ENTRIES_PER_KEY * 12;
            sc256 h;
#pragma unroll
            for (int j = 0; j < 4; j++) h.w[j] = h_in[4 * i + j];
            // [h]P: one mixed addition per non-zero 16-bit window of h, from the key's comb
            jac r = comb_add(jac_identity(), tab, h, (u32)KW_BITS, (u32)KW_COUNT);
            r = add_base_mul(r, gtab, ld_sc(sigs + 81 * i + 49));     // (e read again: not held -- in scratch -- across [h]P)
            bool eq;
            if (flags & VF_SIG_FLAG_BYTE) {
                if (fbyte & 0x80u) {
                    eq = jac_is_identity(r);
                } else {
                    eq = !jac_is_identity(r) && f6_eq(r.X, f6_mul(xs, f6_sqr(r.Z)));
                    if (eq) eq = jac_y_lex_largest(r) == ((fbyte & 0x40u) != 0);
                    else if (!x_on_curve(xs)) ok_sig = false;
                }
            } else if (jac_is_identity(r)) {
                eq = f6_is_zero(xs);
            } else {
                eq = f6_eq(r.X, f6_mul(xs, f6_sqr(r.Z)));
            }
            status = eq ? ST_OK : (ok_sig ? ST_INVALID_SIG : ST_MALFORMED);
        }
        status_out[i] = (u8)status;
    }
    const unsigned long long bad = __ballot(status != ST_OK);
    if ((threadIdx.x & 63u) == 0 && bad) atomicAdd(n_fail, (unsigned long long)__popcll(bad));
}
#endif  // SSA_NO_KERNELS

// ------------------------------------------------------------------------------------------
// The comb table in two steps (round 4; one double-and-add chain of ~250 doublings PER ENTRY before: 13.5 ms for 2^20
// entries, which would be 2.5 s for the 1.8 * 10^8 of the 24-bit table), for a geometry of `bits` (even) x count windows:
//   ssa_k_gbase   gbase[w][h][d] = affine [d 2^(bits w + bits/2 h)] G for d < 2^(bits/2): the slow way (90 112 entries
//                 and 1.3 ms for 24 bits)
//   ssa_k_gtable  gtab[w][d] = gbase[w][1][d >> bits/2] + gbase[w][0][d & (2^(bits/2) - 1)]: ONE affine addition per
//                 entry, a lane takes 8 consecutive entries (same high part) and inverts their 8 denominators together
//                 (23 ms in all for 24 bits); no exceptional case can occur between the two parts (d_hi 2^(bits/2) =
//                 +-d_lo (mod q) has no solution below 2^bits), only zero parts, which copy the other one.  d = 0 rows
//                 are (0, 0) and are never read as points; row 0 of window 0 carries the geometry (gtab_header).
#ifndef SSA_NO_KERNELS
__global__ void __launch_bounds__(256)
ssa_k_gbase(const DevParams *__restrict__ prm, u64 *__restrict__ gbase, u32 bits) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= gbase_entries(bits)) return;
    const u32 hb = bits / 2;
    const u32 d = (u32)(t & ((1u << hb) - 1u)), wh = (u32)(t >> hb);   // wh = 2 w + h
    aff g;
#pragma unroll
    for (int i = 0; i < 6; i++) {
        g.x.c[i] = prm->gen_x[i];
        g.y.c[i] = prm->gen_y[i];
    }
    jac acc = jac_identity();
#pragma unroll 1
    for (int b = (int)hb - 1; b >= 0; b--) {
        acc = jac_dbl(acc);
        if ((d >> b) & 1u) acc = jac_madd(acc, g);
    }
#pragma unroll 1
    for (u32 s = 0; s < wh * hb; s++) acc = jac_dbl(acc);
    st_aff(gbase + t * 12, jac_to_aff(acc));          // the identity (d = 0) as (0, 0)
}

__global__ void __launch_bounds__(256)
ssa_k_gtable(const u64 *__restrict__ gbase, u64 *__restrict__ gtab, u32 bits) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= gtab_entries(bits) / 8) return;
    const u32 hb = bits / 2;
    const u32 w = (u32)((t * 8) >> bits), d0 = (u32)((t * 8) & ((1u << bits) - 1u));
    const u32 dhi = d0 >> hb, dlo0 = d0 & ((1u << hb) - 1u);
    const u64 *slo = gbase + ((size_t)(2 * w) << hb) * 12, *shi = gbase + ((size_t)(2 * w + 1) << hb) * 12;
    u64 *out = gtab + (((size_t)w << bits) + d0) * 12;
    if (dhi == 0) {                                   // only the low part: copies (row 0 of gbase is (0, 0))
#pragma unroll 1
        for (int k = 0; k < 8; k++) st_aff(out + 12 * k, ld_aff(slo + (size_t)(dlo0 + k) * 12));
        if (t == 0) out[0] = gtab_header(bits);       // the identity row of window 0 describes the table
        return;
    }
    const aff p1 = ld_aff(shi + (size_t)dhi * 12);
    const int first = dlo0 == 0 ? 1 : 0;              // d_lo = 0 (only ever the first of the eight): the high part itself
    if (first) st_aff(out, p1);
    // forward: prefix products of the denominators x2 - x1, parked in the output rows
    fp6 c = f6_one();
#pragma unroll 1
    for (int k = first; k < 8; k++) {
        const fp6 x2 = ld_f6(slo + (size_t)(dlo0 + k) * 12);
        c = f6_mul(c, f6_sub(x2, p1.x));
        st_f6(out + 12 * k, c);
    }
    fp6 inv = f6_inv(c);
#pragma unroll 1
    for (int k = 7; k >= first; k--) {
        const aff p2 = ld_aff(slo + (size_t)(dlo0 + k) * 12);
        const fp6 a = f6_sub(p2.x, p1.x);
        fp6 ai = inv;                                  // 1 / a_k = inv * prefix_(k-1)
        if (k > first) ai = f6_mul(inv, ld_f6(out + 12 * (k - 1)));
        inv = f6_mul(inv, a);
        const aff r = aff_from_slope(f6_mul(f6_sub(p2.y, p1.y), ai), p1.x, p1.y, p2.x);
        aff rc;
        rc.x = f6_canon(r.x);
        rc.y = f6_canon(r.y);
        st_aff(out + 12 * k, rc);
    }
}
#endif  // SSA_NO_KERNELS

// out[0] = 1 when the blob's generator is a point of the prime-order subgroup: on the curve (which also rules out
// (0, 0)) and [q]G == O, computed from the freshly built comb table; 0 otherwise.  One lane.
#ifndef SSA_NO_KERNELS
__global__ void __launch_bounds__(64)
ssa_k_check_generator(const DevParams *__restrict__ prm, const u64 *__restrict__ gtab, unsigned *__restrict__ out) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    aff g;
#pragma unroll
    for (int i = 0; i < 6; i++) {
        g.x.c[i] = prm->gen_x[i];
        g.y.c[i] = prm->gen_y[i];
    }
    bool ok = aff_on_curve(g);
    if (ok) {
        sc256 q;
#pragma unroll
        for (int j = 0; j < 4; j++) q.w[j] = SC_Q(j);
        ok = jac_is_identity(add_base_mul(jac_identity(), gtab, q));
        // the table's first row must be G itself (the table was built from this blob)
        const aff g1 = ld_aff(gtab + 12);
        ok = ok && f6_eq(g1.x, g.x) && f6_eq(g1.y, g.y);
    }
    out[0] = ok ? 1u : 0u;
}
#endif  // SSA_NO_KERNELS

// ------------------------------------------------------------------------------------------
// scalar arithmetic mod q: signing (e = r - sk*h, src/signature.rs:124) and the batch coefficients (src/batch.rs:92-111)
SSA_DEV sc256 sc_dbl_mod(const sc256 &a) {  // 2a mod q, a < q < 2^255
    sc256 r;
    r.w[3] = (a.w[3] << 1) | (a.w[2] >> 63);
    r.w[2] = (a.w[2] << 1) | (a.w[1] >> 63);
    r.w[1] = (a.w[1] << 1) | (a.w[0] >> 63);
    r.w[0] = a.w[0] << 1;
    if (sc_geq_q(r)) r = sc_sub_q(r);
    return r;
}
SSA_DEV sc256 sc_add_mod(const sc256 &a, const sc256 &b) {
    sc256 r;
    u64 carry = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        u64 s = a.w[i] + b.w[i];
        u64 c1 = s < a.w[i];
        u64 s2 = s + carry;
        u64 c2 = s2 < s;
        r.w[i] = s2;
        carry = c1 | c2;
    }
    if (sc_geq_q(r)) r = sc_sub_q(r);
    return r;
}
SSA_DEV sc256 sc_neg_mod(const sc256 &a) {  // q - a (a < q), 0 stays 0
    sc256 r;
    u64 borrow = 0;
    bool zero = true;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        u64 d = SC_Q(i) - a.w[i];
        u64 b1 = SC_Q(i) < a.w[i];
        u64 d2 = d - borrow;
        u64 b2 = d < borrow;
        r.w[i] = d2;
        borrow = b1 | b2;
        zero = zero && a.w[i] == 0;
    }
    if (zero) r = a;
    return r;
}
// 4 x 4 limbs -> 8 limbs (schoolbook; mul64x64 = four v_mad_u64_u32)
SSA_DEV void sc_mul_4x4(const u64 (&a)[4], const u64 (&b)[4], u64 (&r)[8]) {
#pragma unroll
    for (int i = 0; i < 8; i++) r[i] = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        u64 carry = 0;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            u64 lo, hi;
            mul64x64(a[i], b[j], lo, hi);
            const u64 s = r[i + j] + lo;
            const u64 c1 = s < lo;
            const u64 s2 = s + carry;
            const u64 c2 = s2 < s;
            r[i + j] = s2;
            carry = hi + c1 + c2;   // a*b + r + carry < 2^128: no overflow
        }
        r[i + 4] = carry;
    }
}

// a*b mod q for a, b < q: 256 x 256 schoolbook product and one Barrett reduction with
// mu = floor(2^510 / q):  q3 = ((x >> 254) * mu) >> 256 is floor(x / q) or up to 2 less, so x - q3*q < 3q.
// (was a 256-step double-and-add; hashes[i] *= scalars[i] and s_i e_i of src/batch.rs:92-111 run it twice per
// signature in msm_k_prepare, signing (src/signature.rs:124) once.)
SSA_DEV sc256 sc_mul_mod(const sc256 &a, const sc256 &b) {
    const u64 MU[4] = {0xdfd9f45eab999731ULL, 0x3314f7c7edb24b7dULL, 0x8c4072a8b88f9d66ULL, 0x8542d23b3c0cc598ULL};
    const u64 QL[4] = {SC_Q(0), SC_Q(1), SC_Q(2), SC_Q(3)};
    u64 x[8];
    sc_mul_4x4(a.w, b.w, x);
    u64 q1[4];
#pragma unroll
    for (int i = 0; i < 4; i++) q1[i] = (x[3 + i] >> 62) | (x[4 + i] << 2);   // x >> 254 (x < 2^510: four limbs)
    u64 q2[8];
    sc_mul_4x4(q1, MU, q2);
    const u64 q3[4] = {q2[4], q2[5], q2[6], q2[7]};
    u64 t[8];
    sc_mul_4x4(q3, QL, t);
    // r = x - q3*q on five limbs (r < 3q < 2^257)
    u64 r[5];
    u64 borrow = 0;
#pragma unroll
    for (int i = 0; i < 5; i++) {
        const u64 d = x[i] - t[i];
        const u64 b1 = x[i] < t[i];
        const u64 d2 = d - borrow;
        const u64 b2 = d < borrow;
        r[i] = d2;
        borrow = b1 | b2;
    }
#pragma unroll
    for (int pass = 0; pass < 2; pass++) {
        sc256 lo;
#pragma unroll
        for (int i = 0; i < 4; i++) lo.w[i] = r[i];
        if (r[4] != 0 || sc_geq_q(lo)) {
            u64 bw = 0;
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const u64 d = r[i] - SC_Q(i);
                const u64 b1 = r[i] < SC_Q(i);
                const u64 d2 = d - bw;
                const u64 b2 = d < bw;
                r[i] = d2;
                bw = b1 | b2;
            }
            r[4] -= bw;
        }
    }
    sc256 out;
#pragma unroll
    for (int i = 0; i < 4; i++) out.w[i] = r[i];
    return out;
}

#ifndef SSA_NO_KERNELS
__global__ void __launch_bounds__(256, 2)
ssa_k_sign(const DevParams *__restrict__ prm, const u64 *__restrict__ gtab,
           const u8 *__restrict__ sks, const u8 *__restrict__ nonces, MsgView mv, size_t n,
           u8 *__restrict__ pks_out, u8 *__restrict__ sigs_out) {
    __shared__ u64 lds[RS_LDS_U64];
    u64 *A = lds + threadIdx.x, *B = A;   // the MDS layer works in place (rescue.hpp)
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const sc256 sk = sc_reduce256(ld_sc(sks + 32 * i));
    const sc256 r = sc_reduce256(ld_sc(nonces + 32 * i));
    const aff pk = jac_to_aff(add_base_mul(jac_identity(), gtab, sk));   // src/public.rs:29
    const jac rj = add_base_mul(jac_identity(), gtab, r);                // src/signature.rs:116
    const aff rp = jac_to_aff(rj);
    st_fp6(pks_out + 96 * i, pk.x);
    st_fp6(pks_out + 96 * i + 48, pk.y);
    u32 len;
    const u8 *m = msg_ptr(mv, i, len);
    u64 d[4];
    hash_message_lane(A, B, prm, rp.x, pk.x, pk.y.c[0], m, len, d);            // :118
    sc256 h;
#pragma unroll
    for (int k = 0; k < 4; k++) h.w[k] = d[k];
    h = sc_reduce256(h);                                                 // :122
    const sc256 e = sc_add_mod(r, sc_neg_mod(sc_mul_mod(sk, h)));        // :124
    u8 *sig = sigs_out + 81 * i;
    st_fp6(sig, rp.x);
    // CompressedPoint flag byte: bit 7 = infinity (src/public.rs:95-101); bit 6 = sort flag
    // (lexicographically largest y; unpinned; ignored by Signature::verify)
    sig[48] = jac_is_identity(rj) ? 0x80 : (f6_lex_largest(rp.y) ? 0x40 : 0x00);
#pragma unroll
    for (int k = 0; k < 4; k++) st_u64_le(sig + 49 + 8 * k, e.w[k]);
}

// KeyPair::sign / sign_and_bind_pkey (src/signature.rs:114-156) for a signer set: the key pair is row key_idx[i] of the
// set, so its public key is read, not computed -- ONE comb walk per signature, [r]G.  Same bytes as ssa_k_sign on the
// gathered rows (the set's keys are canonical and non-zero, sc_reduce256 leaves them as they are).
__global__ void __launch_bounds__(256, 2)
ssa_k_sign_indexed(const DevParams *__restrict__ prm, const u64 *__restrict__ gtab, SignerView sv,
                   const u32 *__restrict__ key_idx, const u8 *__restrict__ nonces, MsgView mv, size_t n, u32 keyed,
                   u8 *__restrict__ out, u8 *__restrict__ lane_status) {
    __shared__ u64 lds[RS_LDS_U64];
    u64 *A = lds + threadIdx.x, *B = A;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    u8 *rec = out + (size_t)(keyed ? 130 : 81) * i;
    const long k = signer_row(sv, key_idx, i, keyed, rec, lane_status);
    if (k < 0) return;
    const sc256 r = sc_reduce256(ld_sc(nonces + 32 * i));
    const jac rj = add_base_mul(jac_identity(), gtab, r);                // src/signature.rs:116
    const aff rp = jac_to_aff(rj);
    bool ok = true;
    const fp6 px = ld_fp6(sv.pks + 96 * k, ok);
    const u64 py0 = ld_u64_le(sv.pks + 96 * k + 48);
    u32 len;
    const u8 *m = msg_ptr(mv, i, len);
    u64 d[4];
    hash_message_lane(A, B, prm, rp.x, px, py0, m, len, d);              // :118
    sc256 h;
#pragma unroll
    for (int j = 0; j < 4; j++) h.w[j] = d[j];
    h = sc_reduce256(h);                                                 // :122
    const sc256 sk = sc_reduce256(ld_sc(sv.sks + 32 * k));
    const sc256 e = sc_add_mod(r, sc_neg_mod(sc_mul_mod(sk, h)));        // :124
    u8 *sig = signer_record(sv, k, keyed, rec);
    st_fp6(sig, rp.x);
    sig[48] = jac_is_identity(rj) ? 0x80 : (f6_lex_largest(rp.y) ? 0x40 : 0x00);
#pragma unroll
    for (int j = 0; j < 4; j++) st_u64_le(sig + 49 + 8 * j, e.w[j]);
}
#endif  // SSA_NO_KERNELS

// ------------------------------------------------------------------------------------------
// AffinePoint::from_compressed: 48 bytes of x || flag byte (bit 7 infinity, bit 6 sort flag, other
// bits must be clear) -> affine (x, y).  status 0 = ok, 1 = "decompression failed".
SSA_DEV u32 decompress_lane(const u8 *__restrict__ c, aff &out, bool &is_inf) {
    const u32 flag = c[48];
    is_inf = false;
    out.x = f6_zero();
    out.y = f6_zero();
    if (flag & 0x3fu) return 1;
    const bool inf = (flag & 0x80u) != 0, sort = (flag & 0x40u) != 0;
    bool ok = true;
    const fp6 x = ld_fp6(c, ok);
    if (!ok) return 1;
    if (inf) {
        if (!f6_is_zero(x) || sort) return 1;
        is_inf = true;
        return 0;
    }
    fp6 rhs = f6_add(f6_mul(f6_sqr(x), x), x);   // x^3 + x + (u + 395)
    rhs.c[0] = fp_add(rhs.c[0], 395ull);
    rhs.c[1] = fp_add(rhs.c[1], 1ull);
    fp6 y;
    if (!f6_sqrt(rhs, y)) return 1;
    y = f6_canon(y);
    if (f6_lex_largest(y) != sort) y = f6_canon(f6_neg(y));
    out.x = x;
    out.y = y;
    return 0;
}

// ------------------------------------------------------------------------------------------
// Per-lane pieces of the MSM preparation, shared by msm_k_prepare (ssa_msm.hip) and the streaming aggregate verifier
// (ssa_aggverifier.hpp), which does the position-independent part of that work when a lane arrives
// and the rest at block time.
struct MsmShape {
    u32 c;        // window bits
    u32 windows;  // ceil(255 / c) (+ 0: the top window of a 255-bit scalar has c - 1 bits, the last carry fits)
    u32 buckets;  // per window: 2^(c-1), for |digit| = 1 .. 2^(c-1) (signed digits; digit 0 contributes nothing)
    u32 chunks;   // per window
};

SSA_DEV u32 sc_window(const u64 *__restrict__ k, u32 bit, u32 c) {
    const u32 wi = bit >> 6, sh = bit & 63u;
    if (wi > 3) return 0u;
    u64 v = k[wi] >> sh;
    if (sh + c > 64 && wi < 3) v |= k[wi + 1] << (64 - sh);
    return (u32)(v & ((1ull << c) - 1ull));
}

// Signed c-bit digits, window-major: digits[j * npts + pt] in [-2^(c-1), 2^(c-1) - 1] -- every window read as a
// two's-complement number with the carry of the window below:
//   raw = window_j(k) + carry;  raw >= 2^(c-1): digit = raw - 2^c, carry 1.
// Returns the carry out of the LAST window: the digits represent  k - carry_out * 2^(windows * c).  A scalar mod q
// (< 2^255: its top window has c - 1 bits and a value below 2^(c-1) - 1) never carries out; a narrow coefficient that
// fills its windows to the last bit may (see msm_k_prepare: the coefficient then IS the value its digits represent).
SSA_DEV u32 write_signed_digits(const sc256 &k, u32 c, u32 windows, short *__restrict__ digits, size_t npts, size_t pt) {
    const int half = 1 << (c - 1);
    int carry = 0;
#pragma unroll 1
    for (u32 j = 0; j < windows; j++) {
        int raw = (int)sc_window(k.w, j * c, c) + carry;
        carry = 0;
        if (raw >= half) {
            raw -= 2 * half;
            carry = 1;
        }
        digits[(size_t)j * npts + pt] = (short)raw;
    }
    return (u32)carry;
}

SSA_DEV void st_aff_row(u64 *__restrict__ row, const aff &p) {
    st_f6(row, p.x);
    st_f6(row + 6, p.y);
}

// The checks msm_k_prepare makes of a lane, and what they decode, in two steps (the kernel reads e between them).
// First the key as it was loaded; ok is cleared on a non-canonical limb.
SSA_DEV void msm_lane_key(const u8 *__restrict__ pks, size_t i, aff &P, bool &ok) {
    P.x = ld_fp6(pks + 96 * i, ok);
    P.y = ld_fp6(pks + 96 * i + 48, ok);
}
// Then, for a lane that passed so far, the key on the curve (an identity key, p_inf, is a valid PublicKey:
// src/public.rs:95-101) and R = from_compressed(sig).unwrap() (src/batch.rs:104).  Returns "passed"; R is defined only
// where the lane got as far as the decompression, r_inf: it decoded to the identity.
SSA_DEV bool msm_lane_decode(bool ok, bool p_inf, const aff &P, const u8 *__restrict__ sig, aff &R, bool &r_inf) {
    if (ok && !p_inf) ok = aff_on_curve(P);
    r_inf = false;
    if (ok) ok = decompress_lane(sig, R, r_inf) == 0;
    return ok;
}

#ifndef SSA_NO_KERNELS
__global__ void __launch_bounds__(256)
ssa_k_decompress(const u8 *__restrict__ comp, size_t n, u8 *__restrict__ pks_out, u8 *__restrict__ inf_out,
                 u8 *__restrict__ status_out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    aff p;
    bool inf;
    const u32 st = decompress_lane(comp + 49 * i, p, inf);
    st_fp6(pks_out + 96 * i, p.x);
    st_fp6(pks_out + 96 * i + 48, p.y);
    if (inf_out) inf_out[i] = inf ? 1 : 0;
    status_out[i] = (u8)st;
}
#endif  // SSA_NO_KERNELS

// KeyedSignature wire form (src/signature.rs:236-271): pk (49 B compressed) || signature (81 B).
// Splits n records into the affine keys / signatures the verification kernels consume; a key that
// does not decompress becomes (0, 0), which ssa_k_verify reports as SSA_MALFORMED
// (KeyedSignature::from_bytes is_none).
#ifndef SSA_NO_KERNELS
__global__ void __launch_bounds__(256)
ssa_k_unpack_keyed(const u8 *__restrict__ keyed, size_t n, u8 *__restrict__ pks_out, u8 *__restrict__ inf_out,
                   u8 *__restrict__ sigs_out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const u8 *rec = keyed + 130 * i;
    aff p;
    bool inf;
    (void)decompress_lane(rec, p, inf);
    st_fp6(pks_out + 96 * i, p.x);
    st_fp6(pks_out + 96 * i + 48, p.y);
    inf_out[i] = inf ? 1 : 0;
    for (int k = 0; k < 81; k++) sigs_out[81 * i + k] = rec[49 + k];
}
#endif  // SSA_NO_KERNELS

// ------------------------------------------------------------------------------------------
// arithmetic probes (ssa_debug_arith)
#ifndef SSA_NO_KERNELS
__global__ void ssa_k_debug(int op, const u64 *__restrict__ a, const u64 *__restrict__ b, size_t n,
                            size_t as, size_t bs, u64 *__restrict__ out, size_t os) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const u64 *pa = a + i * as, *pb = b ? b + i * bs : nullptr;
    u64 *po = out + i * os;
    if (op == 5) {
        po[0] = fp_canon(fp_mul(pa[0], pb[0]));
        return;
    }
    if (op == 6) {
        po[0] = fp_canon(fp_inv(pa[0]));
        return;
    }
    if (op == 18) {   // the Rescue S-boxes on RAW loose values: a = (x, y) -> x^7, y^7, x^(1/7), y^(1/7), asm flags
        // the product's block wrapper (asm block, then the compiled exact chain for a lane the block flagged) on the values
        // (x, y, x); po[4], po[5]: this lane's bit of the mask the forward / inverse asm block returned
        u64 t[3] = {pa[0], pa[1], pa[0]};
        u64 *p[SSA_FP_CHAINS];
#pragma unroll
        for (int k = 0; k < SSA_FP_CHAINS; k++) p[k] = t + k;
        u64 st = sbox_block<false>(p);
        po[0] = fp_canon(t[0]);
        po[1] = fp_canon(t[1]);
        po[4] = 0;
#ifdef SSA_FP_CHAIN_ASM
        po[4] = lane_bit(st) ? 1u : 0u;
#endif
        t[0] = t[2] = pa[0];
        t[1] = pa[1];
        st = sbox_block<true>(p);
        po[2] = fp_canon(t[0]);
        po[3] = fp_canon(t[1]);
        po[5] = 0;
#ifdef SSA_FP_CHAIN_ASM
        po[5] = lane_bit(st) ? 1u : 0u;
#endif
        return;
    }
    if (op <= 2) {
        fp6 x, y, r;
#pragma unroll
        for (int k = 0; k < 6; k++) {
            x.c[k] = pa[k];
            y.c[k] = pb ? pb[k] : 0;
        }
        if (op == 0) r = f6_mul(x, y);
        else if (op == 1) r = f6_sqr(x);
        else r = f6_inv(x);
        r = f6_canon(r);
#pragma unroll
        for (int k = 0; k < 6; k++) po[k] = r.c[k];
        return;
    }
    if (op >= 8 && op <= 14) {   // fused product + linear terms: a = (a, b), b = (x, y)
        fp6 u, v, x, y, r;
#pragma unroll
        for (int k = 0; k < 6; k++) {
            u.c[k] = pa[k];
            v.c[k] = pa[6 + k];
            x.c[k] = pb[k];
            y.c[k] = pb[6 + k];
        }
        if (op == 8) r = f6_sqr_sub2(u, x, y);
        else if (op == 9) r = f6_sqr_add3x(u, x);
        else if (op == 10) r = f6_sqr_sub4x(u, x);
        else if (op == 11) r = f6_mul_sub8x(u, v, x);
        else if (op == 12) r = f6_mul_subx(u, v, x);
        else if (op == 13) r = f6_sqr_subx_sub2y(u, x, y);
        else r = f6_mul2_add(u, v, x, y);
        r = f6_canon(r);
#pragma unroll
        for (int k = 0; k < 6; k++) po[k] = r.c[k];
        return;
    }
    if (op == 3) {  // affine + affine (a[12] = inf flag, b[12] = inf flag) -> 12 felts + inf
        aff p, q;
#pragma unroll
        for (int k = 0; k < 6; k++) {
            p.x.c[k] = pa[k]; p.y.c[k] = pa[6 + k];
            q.x.c[k] = pb[k]; q.y.c[k] = pb[6 + k];
        }
        jac pj = pa[12] ? jac_identity() : jac_from_aff(p);
        jac r;
        if (pb[12]) r = pj;
        else if (pa[13]) r = jac_add(pj, jac_from_aff(q));  // a[13] selects the general add
        else r = jac_madd(pj, q);
        const aff o = jac_to_aff(r);
#pragma unroll
        for (int k = 0; k < 6; k++) {
            po[k] = o.x.c[k];
            po[6 + k] = o.y.c[k];
        }
        po[12] = jac_is_identity(r) ? 1 : 0;
        return;
    }
}
#endif  // SSA_NO_KERNELS

// [k]P with the production table code path (op 4): a = k (4 u64), b = P (12 u64 + inf)
#ifndef SSA_NO_KERNELS
__global__ void __launch_bounds__(256, 2)      // the asm doubling owns VGPRs up to v255: two waves per SIMD at most
ssa_k_debug_mul(int op, const u64 *__restrict__ a, const u64 *__restrict__ b, size_t n,
                                size_t as, size_t bs, u64 *__restrict__ ws_tab,
                                u64 *__restrict__ out, size_t os) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const u64 *pa = a + i * as, *pb = b + i * bs;
    u64 *po = out + i * os;
    if (op >= 15) {
        // the generated point operations on RAW loose limbs (any 64-bit values): a = X, Y, Z (18 u64), a[18] = act,
        // a[19] = n; b = x2, y2 (12 u64) -> X, Y, Z as they come out (not canonicalised) + out[18] = the statement's flag
        //   15: one ladder window (n doublings, then the addition where act != 0)   16: jac_madd_fast   17: jac_dbl_n
        jac p;
        aff q;
#pragma unroll
        for (int j = 0; j < 6; j++) {
            p.X.c[j] = pa[j]; p.Y.c[j] = pa[6 + j]; p.Z.c[j] = pa[12 + j];
            q.x.c[j] = pb[j]; q.y.c[j] = pb[6 + j];
        }
        u32 flag = 1;
#ifdef SSA_JAC_ASM
        const u64 *keep = pb;
        if (op == 15) flag = jac_window_asm(p.X.c, p.Y.c, p.Z.c, pb, (u32)pa[18], (u32)pa[19], keep);    // (gathers x2, y2 itself)
        else
#endif
        if (op == 16) p = jac_madd_fast(p, q);
        else p = jac_dbl_n(p, (u32)pa[19]);
#pragma unroll
        for (int j = 0; j < 6; j++) {
            po[j] = p.X.c[j]; po[6 + j] = p.Y.c[j]; po[12 + j] = p.Z.c[j];
        }
        po[18] = flag;
        return;
    }
    sc256 k;
#pragma unroll
    for (int j = 0; j < 4; j++) k.w[j] = pa[j];
    aff p;
#pragma unroll
    for (int j = 0; j < 6; j++) {
        p.x.c[j] = pb[j];
        p.y.c[j] = pb[6 + j];
    }
    u64 *tab = ws_tab + i * (size_t)(PTAB_ENTRIES * PTAB_ENTRY_U64);
    build_ptab(tab, p, pb[12] != 0);
    const jac r = mul_ptab(tab, k);
    const aff o = jac_to_aff(r);
#pragma unroll
    for (int j = 0; j < 6; j++) {
        po[j] = o.x.c[j];
        po[6 + j] = o.y.c[j];
    }
    po[12] = jac_is_identity(r) ? 1 : 0;
}
#endif  // SSA_NO_KERNELS

// register-resident Fp-mul throughput probe: each lane runs ILP independent multiply chains
#ifndef SSA_NO_KERNELS
template <int ILP>
__global__ void __launch_bounds__(256) ssa_k_fpmul_bench(u64 *out, u64 seed, int iters) {
    u64 x[ILP], y[ILP];
    const u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x;
#pragma unroll
    for (int j = 0; j < ILP; j++) {
        x[j] = seed * (t + 1) + 0x9e3779b97f4a7c15ULL * (j + 1);
        y[j] = seed ^ (t * 0xbf58476d1ce4e5b9ULL + j);
    }
#pragma unroll 1
    for (int it = 0; it < iters; it++) {
#pragma unroll
        for (int j = 0; j < ILP; j++) x[j] = fp_mul(x[j], y[j]);
#pragma unroll
        for (int j = 0; j < ILP; j++) y[j] = fp_mul(y[j], x[j]);
    }
    u64 acc = 0;
#pragma unroll
    for (int j = 0; j < ILP; j++) acc ^= x[j] ^ y[j];
    out[t] = acc;
}
#endif  // SSA_NO_KERNELS

// squaring chains (the shape of the Rescue S-boxes): MODE 0 = fp_mul(x, x) (four mads), 1 = fp_sqr3 (three mads)
#ifndef SSA_NO_KERNELS
template <int MODE>
__global__ void __launch_bounds__(256) ssa_k_fpsqr_bench(u64 *out, u64 seed, int iters) {
    u64 x[2];
    const u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x;
#pragma unroll
    for (int j = 0; j < 2; j++) x[j] = seed * (t + 1) + 0x9e3779b97f4a7c15ULL * (j + 1);
#pragma unroll 1
    for (int it = 0; it < iters; it++) {
#pragma unroll
        for (int r = 0; r < 8; r++) {
#pragma unroll
            for (int j = 0; j < 2; j++) x[j] = MODE == 0 ? fp_mul(x[j], x[j]) : fp_sqr3(x[j]);
        }
    }
    out[t] = x[0] ^ x[1];
}
#endif  // SSA_NO_KERNELS

// same probe through the lazy Fp6 product (36 products + 6 reductions per f6_mul)
#ifndef SSA_NO_KERNELS
__global__ void __launch_bounds__(256) ssa_k_f6mul_bench(u64 *out, u64 seed, int iters) {
    fp6 x, y;
    const u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x;
#pragma unroll
    for (int j = 0; j < 6; j++) {
        x.c[j] = seed * (t + 1) + 0x9e3779b97f4a7c15ULL * (j + 1);
        y.c[j] = seed ^ (t * 0xbf58476d1ce4e5b9ULL + j);
    }
#pragma unroll 1
    for (int it = 0; it < iters; it++) {
        x = f6_mul(x, y);
        y = f6_sqr(x);
    }
    u64 acc = 0;
#pragma unroll
    for (int j = 0; j < 6; j++) acc ^= x.c[j] ^ y.c[j];
    out[t] = acc;
}
#endif  // SSA_NO_KERNELS

}  // namespace ssa

// wave-cooperative path (device code only; the host-compiled unit tests leave it out)
#ifndef SSA_NO_COOP
#include "ssa_coop.hpp"

#ifndef SSA_NO_KERNELS
namespace ssa {
// Low-latency verification: two cooperating waves (one 128-thread block) per signature.
__global__ void __launch_bounds__(128)
ssa_k_verify_coop(const DevParams *__restrict__ prm, const u8 *__restrict__ sigs, const u8 *__restrict__ pks,
                  const u8 *__restrict__ pk_inf, MsgView mv, const u64 *__restrict__ gtab, size_t n, u32 flags,
                  u8 *__restrict__ status_out, unsigned long long *__restrict__ n_fail) {
    __shared__ CoopLds L;
    __shared__ CoopShared sh;
    const size_t i = blockIdx.x;
    if (i >= n) return;
    u32 len;
    const u8 *m = msg_ptr(mv, i, len);
    const u32 st = coop_verify_two_waves(L, sh, prm, sigs + 81 * i, pks + 96 * i, pk_inf && pk_inf[i], m, len, gtab,
                                         flags, threadIdx.x & 63u, (int)(threadIdx.x >> 6));
    if (threadIdx.x == 0) {
        status_out[i] = (u8)st;
        if (st != ST_OK) atomicAdd(n_fail, 1ull);
    }
}
// unit probe of the cooperative point operations, one wave per row: a = (x, y, inf, mode), b = (x, y, inf);
// mode 0: mixed addition a + b (a as a scaled Jacobian point, b affine), 1: general addition of two scaled
// Jacobian points, 2: doubling of a.  out = affine (x, y, inf).
__global__ void __launch_bounds__(64)
ssa_k_debug_coop(const u64 *__restrict__ a, const u64 *__restrict__ b, size_t n, size_t as, size_t bs,
                 u64 *__restrict__ out, size_t os) {
    __shared__ CoopLds L;
    const u32 lane = threadIdx.x;
    const size_t i = blockIdx.x;
    if (i >= n) return;
    const u64 *pa = a + i * as, *pb = b + i * bs;
    const int mode = (int)pa[13];
    enum { X1 = 0, Y1, Z1, W1, X2, Y2, Z2, LAM, T0, T1, T2, TS = 12 };
    int t[9];
#pragma unroll
    for (int k = 0; k < 9; k++) t[k] = TS + k;
    // modified Jacobian (lam^2 x, lam^3 y, lam, lam^4) of an affine point, (1, 1, 0, 0) for the identity
    auto lift = [&](const u64 *p, int X, const u64 (&lam)[6], bool with_w) {
        const int Y = X + 1, Z = X + 2, W = X + 3;
        if (p[12]) {
            coop_set(L, X, 1ull, lane);
            coop_set(L, Y, 1ull, lane);
            coop_set(L, Z, 0ull, lane);
            if (with_w) coop_set(L, W, 0ull, lane);
            return;
        }
        coop_store7(L, X, p[lane % 6u], lane);
        coop_store7(L, Y, p[6 + lane % 6u], lane);
        coop_store7(L, LAM, lam[lane % 6u], lane);
        coop_sync();
        coop_copy(L, Z, LAM, lane);
        coop_mul(L, T0, LAM, LAM, lane);
        coop_mul(L, X, X, T0, lane);
        if (with_w) coop_mul(L, W, T0, T0, lane);
        coop_mul(L, T0, T0, LAM, lane);
        coop_mul(L, Y, Y, T0, lane);
    };
    const u64 lam1[6] = {3, 1, 4, 1, 5, 9}, lam2[6] = {2, 7, 1, 8, 2, 8};
    lift(pa, X1, lam1, true);
    if (mode == 1) {
        lift(pb, X2, lam2, false);
        coop_jac_add(L, X1, X2, t, lane);
    } else if (mode == 0) {
        if (pb[12]) {
            coop_set(L, X2, 0ull, lane);
            coop_set(L, Y2, 0ull, lane);
        } else {
            coop_store7(L, X2, pb[lane % 6u], lane);
            coop_store7(L, Y2, pb[6 + lane % 6u], lane);
            coop_sync();
        }
        coop_jac_madd(L, X1, X2, Y2, t, lane);
    } else {
        coop_jac_dbl(L, X1, t, lane);
    }
    // W must still be Z^4 (the next operation would rely on it)
    coop_mul(L, T0, Z1, Z1, lane);
    coop_mul(L, T0, T0, T0, lane);
    const bool w_ok = coop_eq(L, T0, W1, lane);
    u64 *po = out + i * os;
    if (coop_is_zero(L, Z1, lane)) {
        if (lane == 0) po[12] = w_ok ? 1 : 99;
        return;
    }
    coop_inv(L, T0, Z1, T1, T2, LAM, lane);
    coop_mul(L, T1, T0, T0, lane);
    coop_mul(L, X1, X1, T1, lane);
    coop_mul(L, T1, T1, T0, lane);
    coop_mul(L, Y1, Y1, T1, lane);
    if (lane < 6) {
        po[lane] = fp_canon(L.slot[X1][lane]);
        po[6 + lane] = fp_canon(L.slot[Y1][lane]);
    }
    if (lane == 0) po[12] = w_ok ? 0 : 99;
}

// probe: a chain of dependent cooperative point operations on ONE wave (op 0: doubling, 1: mixed addition,
// 2: general addition, 3: one ladder window); the latency the low-latency kernel and the MSM tail are made of
__global__ void __launch_bounds__(64) ssa_k_coop_bench(int op, int iters, u64 *out) {
    __shared__ CoopLds L;
    const u32 lane = threadIdx.x;
    int t[9];
#pragma unroll
    for (int k = 0; k < 9; k++) t[k] = 8 + k;
    for (int s0 = 0; s0 < 8; s0++) {
        coop_store7(L, s0, 0x9e3779b97f4a7c15ULL * (u64)(7 * s0 + (int)(lane % 6u) + 1), lane);
    }
    coop_sync();
#pragma unroll 1
    for (int i = 0; i < iters; i++) {
        if (op == 0) coop_jac_dbl(L, 0, t, lane);
        else if (op == 1) coop_jac_madd(L, 0, 4, 5, t, lane);
        else if (op == 2) coop_jac_add(L, 0, 4, t, lane);
        else {   // one window of the ladder: 4 doublings + 1 mixed addition, first addition round fused
            for (int d = 0; d < 3; d++) coop_jac_dbl(L, 0, t, lane);
            coop_jac_dbl(L, 0, t, lane, 0, 5, t[4], t[5]);
            coop_jac_madd(L, 0, 4, 5, t, lane, 0, true);
        }
    }
    if (lane < 6) out[lane] = L.slot[0][lane] ^ L.slot[1][lane] ^ L.slot[2][lane];
}
}  // namespace ssa
#endif  // SSA_NO_KERNELS
#endif  // SSA_NO_COOP
