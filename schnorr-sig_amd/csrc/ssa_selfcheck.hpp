// Exact self-check of the fixed-base tables, included by ssa_sign.hip after the constant-time
// signer's table (ct_offset_scalar, CTAB_*) is defined.
//
//   ssa_k_gtab_check   every row of a comb table of `bits`-bit windows, [d 2^(bits w)]G, checked against the rows before
//                      it: (w, 0) is zero (row (0, 0) carries the header word), (0, 1) is G, (w, 1) = (w-1, 2^bits-1) +
//                      B_{w-1}, (w, 2) = 2 B_w, (w, d) = (w, d-1) + B_w, with B_w = row (w, 1); every limb < p.  The same
//                      kernel checks the 64 x 16 rows of the constant-time table (bits = 4, no header word).  The walk
//                      itself is comb_rows_check, which the per-key combs of key sets share (ssa_keycheck.hpp).
//   ssa_k_ctab_check_b the two offset rows of the constant-time table: B = [b]G by one walk of the (checked) comb, -B
//
// A relation R = P + Q (chord) or R = 2P (tangent) is checked without an inversion: with the slope num / den,
//   (x_R + x_P + x_Q) den^2 == num^2   and   (y_R + y_P) den == num (x_P - x_R),   den != 0
// (chord: num = y_Q - y_P, den = x_Q - x_P; tangent: num = 3 x_P^2 + a, a = 1, den = 2 y_P, x_Q = x_P).  With den != 0
// these two equations have exactly one solution R, so a clean pass proves every row exact, in chain order.  The kernels
// only read the tables, take the geometry from the host (never from the header word they check) and are variable-time:
// every input is public.
//
// Work layout (that of ssa_k_gtable): a lane takes 8 consecutive rows of one window and first loads the row before them
// (for the first lane of a window: the last row of the window before -- the hop).  A wave's 512 rows lie in one window
// of the comb, so B_w is the same address for the whole wave.  Per wave: ballots, then one atomicAdd of the failing
// rows and one atomicMin of the first failing row (rows grow with the lane, so the lowest lane with a failure holds it).
namespace ssa {

constexpr u64 TC_NONE = ~0ull;     // "no failing row"

SSA_DEV bool row_canonical(const aff &r) {
    bool ok = true;
#pragma unroll
    for (int i = 0; i < 6; i++) ok = ok && r.x.c[i] < FP_P && r.y.c[i] < FP_P;
    return ok;
}

SSA_DEV bool chain_rel(const aff &R, const aff &P, const aff &Q, bool tangent) {
    fp6 num, den, xs;
    if (tangent) {
        const fp6 x2 = f6_sqr(P.x);
        num = f6_add(f6_dbl(x2), x2);
        num.c[0] = fp_add(num.c[0], 1ull);
        den = f6_dbl(P.y);
        xs = f6_dbl(P.x);
    } else {
        num = f6_sub(Q.y, P.y);
        den = f6_sub(Q.x, P.x);
        xs = f6_add(P.x, Q.x);
    }
    if (f6_is_zero(den)) return false;
    const bool ex = f6_eq(f6_mul(f6_add(R.x, xs), f6_sqr(den)), f6_sqr(num));
    const bool ey = f6_eq(f6_mul(f6_add(R.y, P.y), den), f6_mul(num, f6_sub(P.x, R.x)));
    return ex && ey;
}

#ifndef SSA_CHECK_FUNCTIONS_ONLY      // (tests/csrc/keycheck_host.cpp compiles the relations alone, for the CPU)
// The 8 rows lane `t` takes of a comb of `bits`-bit windows at `tab` (see "Work layout"): nbad = how many fail, first =
// the first of them (TC_NONE: none).  `head` is word 0 of row (0, 0) (0: none); base_eq(R) says whether R is the point
// the comb is a table of -- row (0, 1), the one row that no relation ties to the rows before it.
template <class BaseEq>
SSA_DEV void comb_rows_check(const u64 *__restrict__ tab, u32 bits, size_t t, u64 head, BaseEq base_eq, u32 &nbad,
                             u64 &first) {
    const u32 mask = (1u << bits) - 1u;
    const u32 w = (u32)((t * 8) >> bits), d0 = (u32)((t * 8) & mask);
    const u64 *win = tab + ((size_t)w << bits) * 12;
    const aff B = ld_aff(win + 12);
    aff prev;
    prev.x = f6_zero();
    prev.y = f6_zero();
    if (d0 > 0) prev = ld_aff(win + 12 * (size_t)(d0 - 1));
    else if (w > 0) prev = ld_aff(win - 12);                 // (w - 1, 2^bits - 1)
#pragma unroll 1
    for (u32 k = 0; k < 8; k++) {
        const u32 d = d0 + k;
        const aff R = ld_aff(win + 12 * (size_t)d);
        bool ok = row_canonical(R);
        if (d == 0) {
            u64 z = R.x.c[0] ^ (w == 0 ? head : 0ull);
#pragma unroll
            for (int i = 1; i < 6; i++) z |= R.x.c[i];
#pragma unroll
            for (int i = 0; i < 6; i++) z |= R.y.c[i];
            ok = ok && z == 0ull;
        } else if (d == 1 && w == 0) {
            ok = ok && base_eq(R);
        } else {
            aff Q = B;
            if (d == 1) Q = ld_aff(win - 12 * (size_t)mask);    // B_{w-1} = (w - 1, 1)
            ok = ok && chain_rel(R, d == 2 ? B : prev, Q, d == 2);
            prev = R;
        }
        if (!ok) {
            nbad++;
            if (first == TC_NONE) first = ((size_t)w << bits) + d;
        }
    }
}

// out[0] += failing rows, out[1] = min(out[1], first failing row); `head` is word 0 of row (0, 0) (0: none)
__global__ void __launch_bounds__(256)
ssa_k_gtab_check(const DevParams *__restrict__ prm, const u64 *__restrict__ tab, u32 bits, u32 windows, u64 head,
                 unsigned long long *__restrict__ out) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    u32 nbad = 0;
    u64 first = TC_NONE;
    if (t < ((size_t)windows << bits) / 8)       // (no early return: every lane takes part in the ballots below)
        comb_rows_check(tab, bits, t, head, [&](const aff &R) {
            bool eq = true;
#pragma unroll
            for (int i = 0; i < 6; i++) eq = eq && fp_eq(R.x.c[i], prm->gen_x[i]) && fp_eq(R.y.c[i], prm->gen_y[i]);
            return eq;
        }, nbad, first);
    unsigned long long wave_bad = 0;
#pragma unroll
    for (int b = 0; b < 4; b++) wave_bad += (unsigned long long)__popcll(__ballot((nbad >> b) & 1u)) << b;
    const unsigned long long firsts = __ballot(first != TC_NONE);
    const u32 lane = threadIdx.x & 63u;
    if (lane == 0 && wave_bad) atomicAdd(out, wave_bad);
    if (firsts && lane == (u32)(__ffsll((long long)firsts) - 1)) atomicMin(out + 1, (unsigned long long)first);
}

// rows CTAB_B and CTAB_NEG_B of the constant-time table: [b]G recomputed through the comb, and its negative
__global__ void __launch_bounds__(64)
ssa_k_ctab_check_b(const u64 *__restrict__ gtab, const u64 *__restrict__ ctab, unsigned long long *__restrict__ out) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const aff b = jac_to_aff(add_base_mul(jac_identity(), gtab, ct_offset_scalar()));
#pragma unroll 1
    for (u32 s = 0; s < 2; s++) {
        const aff r = ld_aff(ctab + 12 * (CTAB_B + s));
        const fp6 y = s ? f6_neg(b.y) : b.y;
        if (!(row_canonical(r) && f6_eq(r.x, b.x) && f6_eq(r.y, y))) {
            atomicAdd(out, 1ull);
            atomicMin(out + 1, (unsigned long long)(CTAB_B + s));
        }
    }
}

#endif  // SSA_CHECK_FUNCTIONS_ONLY
}  // namespace ssa

#ifndef SSA_CHECK_FUNCTIONS_ONLY
// res[0] failing rows, res[1] first failing row (TC_NONE: none) of the table `tab` of `windows` x 2^bits rows, checked
// on the context's stream; with `ctab`, also the two offset rows of the constant-time table.  Synchronous.
static int table_check(ssa_ctx *ctx, const char *name, const u64 *tab, u32 bits, u32 windows, u64 head, bool ctab,
                       uint64_t res[2]) {
    if (ctx->tc_out.reserve(2 * sizeof(u64))) return SSA_ERR_HIP;
    unsigned long long *d = (unsigned long long *)ctx->tc_out.p;
    HIP_TRY(hipMemsetAsync(d, 0, sizeof(u64), ctx->stream));
    HIP_TRY(hipMemsetAsync(d + 1, 0xff, sizeof(u64), ctx->stream));
    const size_t lanes = ((size_t)windows << bits) / 8;
    if (int rc = timed_launch(ctx, name, [&] {
            hipLaunchKernelGGL(ssa_k_gtab_check, dim3(grid_for(lanes, 256)), dim3(256), 0, ctx->stream, ctx->d_params, tab,
                               bits, windows, head, d);
            if (ctab)
                hipLaunchKernelGGL(ssa_k_ctab_check_b, dim3(1), dim3(64), 0, ctx->stream, (const u64 *)ctx->d_gtab, tab, d);
        }))
        return rc;
    HIP_TRY(hipMemcpyAsync(res, d, 2 * sizeof(u64), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return 0;
}

int ssa_internal_gtab_check(ssa_ctx *ctx, const uint64_t *d_gtab, uint32_t bits, uint64_t res[2]) {
    return table_check(ctx, "ssa_k_gtab_check", d_gtab, bits, gtab_windows(bits), gtab_header(bits), false, res);
}

static int ctab_check(ssa_ctx *ctx, uint64_t res[2]) {
    return table_check(ctx, "ssa_k_ctab_check", (const u64 *)ctx->ctab.p, 4, CT_WINDOWS, 0ull, true, res);
}

// the on-demand check of the constant-time table: out[0] rows checked (0 before it is built), out[1] failing rows,
// out[2] first failing row.  A table that fails is no longer used: the next constant-time call rebuilds and checks it.
int ssa_internal_ctab_selfcheck(ssa_ctx *ctx, uint64_t out[3]) {
    out[0] = 0;
    out[1] = 0;
    out[2] = TC_NONE;
    if (!ctx->ctab_ready) return 0;
    uint64_t res[2];
    if (int rc = ctab_check(ctx, res)) return rc;
    out[0] = CTAB_ROWS;
    out[1] = res[0];
    out[2] = res[1];
    if (res[0]) ctx->ctab_ready = false;
    return 0;
}

// the rows of a table as the tests see them (which: 0 the comb for G, 1 the constant-time table once built)
static int debug_table_span(ssa_ctx *ctx, int which, u64 **base, uint64_t *rows) {
    if (which == 0) {
        *base = ctx->d_gtab;
        *rows = gtab_entries(ctx->gtab_bits);
        return 0;
    }
    if (which == 1 && ctx->ctab_ready) {
        *base = (u64 *)ctx->ctab.p;
        *rows = CTAB_ROWS;
        return 0;
    }
    return SSA_ERR_ARG;
}

extern "C" int ssa_debug_table_read(ssa_ctx *ctx, int which, uint64_t first_row, uint64_t n, uint64_t *rows_out) {
    if (!ctx || (n && !rows_out)) return SSA_ERR_ARG;
    u64 *base;
    uint64_t rows;
    if (int rc = debug_table_span(ctx, which, &base, &rows)) return rc;
    if (first_row > rows || n > rows - first_row) return SSA_ERR_ARG;
    if (n == 0) return 0;
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipMemcpyAsync(rows_out, base + 12 * first_row, n * 12 * sizeof(u64), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return 0;
}

extern "C" int ssa_debug_table_xor(ssa_ctx *ctx, int which, uint64_t row, uint32_t word, uint64_t mask) {
    if (!ctx || word >= 12) return SSA_ERR_ARG;
    u64 *base;
    uint64_t rows;
    if (int rc = debug_table_span(ctx, which, &base, &rows)) return rc;
    if (row >= rows) return SSA_ERR_ARG;
    HIP_TRY(hipSetDevice(ctx->device));
    u64 *p = base + 12 * row + word, v = 0;
    HIP_TRY(hipMemcpyAsync(&v, p, sizeof v, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    v ^= mask;
    HIP_TRY(hipMemcpyAsync(p, &v, sizeof v, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return 0;
}
#endif  // SSA_CHECK_FUNCTIONS_ONLY
