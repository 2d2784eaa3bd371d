// Exact self-check of the per-key tables of key sets and key caches, included by ssa_sign.hip
// behind ssa_selfcheck.hpp: the relations (chain_rel), row_canonical and the comb walk (comb_rows_check) are shared.
//
// The root of trust of a row is what it was built from: its 96 key bytes and its pk_inf boolean.  By stored status:
//   0, a finite key   the bytes are canonical and on the curve; entry 1P is the key, bit for bit; 2P is the tangent of
//                     1P and mP (3 <= m <= 16) the chord (m-1)P + P (section 11's two equations, den != 0); the second
//                     line of every entry is (x, -y).  P has prime order q and m <= 16, so no denominator vanishes on a
//                     true table and each entry is fixed by the ones before it.
//   0, the identity   all sixteen entries are the (0, 0) sentinel in both lines.
//   1                 denominators may vanish and entries may be sentinels: the relations are not sound.  The table is
//                     built again with build_ptab into scratch and the words the kernels read are compared.
//   3                 no kernel reads the table; the status itself is checked: the bytes must fail the limb or the
//                     curve test.
//   anything else     fails.
// build_ptab stores LOOSE limbs (fp.hpp: any u64 stands for its residue, and every kernel reads a table word as such), so
// table words are compared as residues; only the key bytes, and entry 1P against them, are compared bit for bit.  Words
// 12-15 and 28-31 of an entry are read by no kernel and are not checked.
//
//   kck_k_tables    one lane per key walks its sixteen entries (two 128-byte lines each, so a lane's loads are
//                   line-aligned), writes bad[i] and appends the key to the rebuild list (status 1) or, under DEEP, to
//                   the deep list (status 0, table clean).
//   kck_k_rebuild   one lane per key of a chunk of the rebuild list: build_ptab into scratch, compare; clean keys join
//                   the deep list under DEEP.
//   kck_k_deep      one lane per key of the deep list: jac_is_identity(mul_ptab(tab, q, true)) -- what
//                   ssa_k_keyset_build computes -- must agree with the stored status byte.
//   kck_k_comb      the per-key combs of a key set (16 windows of 16 bits, no header word, row (0, 1) = the key): the
//                   walk of ssa_k_gtab_check, 512 workgroups per key, so a wave's rows stay inside one key's comb.  An
//                   identity key's comb is all sentinels; combs of keys of status != 0 are counted and not checked.
//   kck_k_count     bad[] -> failing keys (ballots, one atomicAdd per wave) and the first of them (atomicMin).
//   kck_k_list / kck_k_gather / kck_k_scatter   repair: the failing rows' numbers, their stored bytes gathered for
//                   ssa_k_keyset_build (run as it is over the gathered rows), tables and statuses copied back.
// Lists are filled wave by wave: a ballot, one atomicAdd of the wave's count, plain stores of the row numbers (their
// order does not matter: every verdict is per key).  All device writes are vector stores and vector atomics, and
// every kernel only reads the object but for bad[], the lists and, in repair, the rows being rebuilt.
//
// A key cache in WIRE mode also keeps the 49 compressed bytes each row was built from, and those
// are the root of trust: the row's 96 bytes and pk_inf must be what the 49 bytes stand for.
//   kck_k_wire          one lane per row, after kck_k_tables: a string that cannot decode by its form (flag bits, a limb
//                       >= p, a bad infinity encoding) or that claims "not a square" must hold (0, 0) and no flag; the
//                       identity encoding (0, 0) and the flag; any other row x bit for bit and the sort bit of its y
//                       (f6_lex_largest).  With kck_k_tables' curve relation that fixes y: no square root is computed.
//                       Under DEEP a row of status 3 is decompressed after all, and fails if it decodes.
//   kck_k_wire_rebuild  repair: the listed rows' 96 bytes and flag again from their 49 bytes (decompress_lane), in front
//                       of the gather / build / scatter above.
namespace ssa {

constexpr int KCK_TAB_WORDS = PTAB_ENTRIES * PTAB_ENTRY_U64;        // 512 words per key
constexpr size_t KCK_CHUNK = (size_t)1 << 16;                       // keys rebuilt per launch (256 MB of scratch tables)
// the counters of one check, in ctx->tc_out
enum : int { KCK_BAD = 0, KCK_FIRST = 1, KCK_ST0 = 2, KCK_REBUILD = 3, KCK_DEEP = 4, KCK_COMB_SKIPPED = 5, KCK_LISTED = 6,
             KCK_WORDS = 8 };

// key i's bytes as a point; canon: every limb < p
SSA_DEV aff kck_ld_key(const u64 *__restrict__ pks, size_t i, bool &canon) {
    aff P;
    canon = true;
#pragma unroll
    for (int k = 0; k < 6; k++) {
        P.x.c[k] = pks[12 * i + k];
        P.y.c[k] = pks[12 * i + 6 + k];
        canon = canon && P.x.c[k] < FP_P && P.y.c[k] < FP_P;
    }
    return P;
}

// the words of an entry that the kernels read: (x, y) in the first line, (x, -y) in the second
SSA_DEV bool kck_entry_sentinel(const u64 *__restrict__ row) {
    const aff R = ld_aff(row), N = ld_aff(row + PTAB_NEG);
    return f6_is_zero(R.x) && f6_is_zero(R.y) && f6_is_zero(N.x) && f6_is_zero(N.y);
}

SSA_DEV bool kck_chain_ok(const u64 *__restrict__ tab, const aff &P) {
    bool ok = true;
    aff prev = P;
#pragma unroll 1
    for (int e = 0; e < PTAB_ENTRIES; e++) {
        const u64 *row = tab + e * PTAB_ENTRY_U64;
        const aff R = ld_aff(row), N = ld_aff(row + PTAB_NEG);
        bool eok = f6_eq(N.x, R.x) && f6_is_zero(f6_add(N.y, R.y));
        if (e == 0) {
#pragma unroll
            for (int k = 0; k < 6; k++) eok = eok && R.x.c[k] == P.x.c[k] && R.y.c[k] == P.y.c[k];
        } else {
            eok = eok && chain_rel(R, e == 1 ? P : prev, P, e == 1);
        }
        ok = ok && eok;
        prev = R;
    }
    return ok;
}

#ifndef SSA_CHECK_FUNCTIONS_ONLY      // (tests/csrc/keycheck_host.cpp compiles the per-key checks alone, for the CPU)
// the lanes of the wave with `take` append v to list (the wave's lanes get consecutive places, in lane order)
SSA_DEV void kck_append(bool take, u32 v, u32 *__restrict__ list, unsigned long long *__restrict__ count) {
    const unsigned long long takes = __ballot(take);
    if (!takes) return;
    const u32 lane = threadIdx.x & 63u, leader = (u32)(__ffsll((long long)takes) - 1);
    unsigned long long base = 0;
    if (lane == leader) base = atomicAdd(count, (unsigned long long)__popcll(takes));
    base = (unsigned long long)__shfl((long long)base, (int)leader);
    if (take) list[base + (u32)__popcll(takes & ((1ull << lane) - 1ull))] = v;
}

__global__ void __launch_bounds__(256)
kck_k_tables(const u64 *__restrict__ pks, const u8 *__restrict__ pk_inf, const u8 *__restrict__ status,
             const u64 *__restrict__ tab, u32 m, u32 deep, u8 *__restrict__ bad, u32 *__restrict__ rebuild_list,
             u32 *__restrict__ deep_list, unsigned long long *__restrict__ cnt) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    bool st0 = false, rebuild = false, want_deep = false;
    if (i < m) {                                  // (no early return: every lane takes part in the ballots below)
        bool canon;
        const aff P = kck_ld_key(pks, i, canon);
        const bool inf = pk_inf[i] != 0;
        const u32 st = status[i];
        const bool wellformed = canon && (inf || aff_on_curve(P));
        bool fail;
        if (st == ST_MALFORMED) {
            fail = wellformed;
        } else if (st > ST_INVALID_PK || !wellformed) {
            fail = true;
        } else if (st == ST_INVALID_PK) {
            fail = false;
            rebuild = true;
        } else {
            st0 = true;
            const u64 *t = tab + (size_t)i * KCK_TAB_WORDS;
            if (inf) {
                fail = false;
#pragma unroll 1
                for (int e = 0; e < PTAB_ENTRIES; e++) fail = fail || !kck_entry_sentinel(t + e * PTAB_ENTRY_U64);
            } else {
                fail = !kck_chain_ok(t, P);
            }
            want_deep = deep && !fail;
        }
        bad[i] = fail ? 1 : 0;
    }
    const unsigned long long st0s = __ballot(st0);
    if ((threadIdx.x & 63u) == 0 && st0s) atomicAdd(cnt + KCK_ST0, (unsigned long long)__popcll(st0s));
    kck_append(rebuild, i, rebuild_list, cnt + KCK_REBUILD);
    kck_append(want_deep, i, deep_list, cnt + KCK_DEEP);
}

// keys rebuild_list[lo, lo + n): the table built again at scratch + 512 t and compared with the stored one.  (One wave
// per SIMD: build_ptab's temporaries then live in the accumulation registers and not in scratch; these keys are rare.)
__global__ void __launch_bounds__(256)
kck_k_rebuild(const u64 *__restrict__ pks, const u8 *__restrict__ pk_inf, const u64 *__restrict__ tab,
              const u32 *__restrict__ rebuild_list, u32 lo, u32 n, u64 *__restrict__ scratch, u32 deep,
              u8 *__restrict__ bad, u32 *__restrict__ deep_list, unsigned long long *__restrict__ cnt) {
    const u32 t = blockIdx.x * blockDim.x + threadIdx.x;
    bool want_deep = false;
    u32 i = 0;
    if (t < n) {
        i = rebuild_list[lo + t];
        bool canon;
        const aff P = kck_ld_key(pks, i, canon);
        u64 *mine = scratch + (size_t)t * KCK_TAB_WORDS;
        build_ptab(mine, P, pk_inf[i] != 0);
        const u64 *theirs = tab + (size_t)i * KCK_TAB_WORDS;
        bool ok = true;
#pragma unroll 1
        for (int e = 0; e < PTAB_ENTRIES; e++) {
#pragma unroll 1
            for (int h = 0; h < 2; h++) {
                const aff a = ld_aff(mine + e * PTAB_ENTRY_U64 + h * PTAB_NEG);
                const aff b = ld_aff(theirs + e * PTAB_ENTRY_U64 + h * PTAB_NEG);
                ok = ok && f6_eq(a.x, b.x) && f6_eq(a.y, b.y);
            }
        }
        if (!ok) bad[i] = 1;
        want_deep = deep && ok;
    }
    kck_append(want_deep, i, deep_list, cnt + KCK_DEEP);
}

// the grid covers the keys that can be listed; cnt[KCK_DEEP] says how many are
__global__ void __launch_bounds__(256, 2)
kck_k_deep(const u64 *__restrict__ tab, const u8 *__restrict__ status, const u32 *__restrict__ deep_list,
           const unsigned long long *__restrict__ cnt, u8 *__restrict__ bad) {
    const u32 t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= cnt[KCK_DEEP]) return;
    const u32 i = deep_list[t];
    sc256 q;
#pragma unroll
    for (int j = 0; j < 4; j++) q.w[j] = SC_Q(j);
    const u32 st = jac_is_identity(mul_ptab(tab + (size_t)i * KCK_TAB_WORDS, q, true)) ? ST_OK : ST_INVALID_PK;
    if (st != (u32)status[i]) bad[i] = 1;
}

// 512 workgroups of 256 lanes per key, 8 rows per lane
constexpr u32 KCK_COMB_BLOCKS = (u32)(KTAB_ENTRIES_PER_KEY / 8 / 256);
__global__ void __launch_bounds__(256)
kck_k_comb(const u64 *__restrict__ pks, const u8 *__restrict__ pk_inf, const u8 *__restrict__ status,
           const u64 *__restrict__ ktab, u32 m, u8 *__restrict__ bad, unsigned long long *__restrict__ cnt) {
    const u32 key = blockIdx.x / KCK_COMB_BLOCKS;
    if (key >= m) return;
    const size_t t = (size_t)(blockIdx.x % KCK_COMB_BLOCKS) * 256 + threadIdx.x;
    if (status[key] != ST_OK) {
        if (t == 0) atomicAdd(cnt + KCK_COMB_SKIPPED, 1ull);
        return;
    }
    const u64 *comb = ktab + (size_t)key * KTAB_ENTRIES_PER_KEY * 12;
    u32 nbad = 0;
    if (pk_inf[key]) {
#pragma unroll 1
        for (u32 k = 0; k < 8; k++) {
            const aff R = ld_aff(comb + (t * 8 + k) * 12);
            u64 z = 0;
#pragma unroll
            for (int j = 0; j < 6; j++) z |= R.x.c[j] | R.y.c[j];
            nbad += z != 0ull;
        }
    } else {
        u64 first = TC_NONE;
        comb_rows_check(comb, (u32)KW_BITS, t, 0ull, [&](const aff &R) {
            bool eq = true;
#pragma unroll
            for (int j = 0; j < 6; j++) eq = eq && R.x.c[j] == pks[12 * (size_t)key + j] && R.y.c[j] == pks[12 * (size_t)key + 6 + j];
            return eq;
        }, nbad, first);
    }
    if (nbad) bad[key] = 1;
}

__global__ void __launch_bounds__(256)
kck_k_count(const u8 *__restrict__ bad, u32 m, unsigned long long *__restrict__ cnt) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    const unsigned long long bads = __ballot(i < m && bad[i] != 0);
    if (!bads) return;
    const u32 lane = threadIdx.x & 63u;
    if (lane == 0) atomicAdd(cnt + KCK_BAD, (unsigned long long)__popcll(bads));
    if (lane == (u32)(__ffsll((long long)bads) - 1)) atomicMin(cnt + KCK_FIRST, (unsigned long long)i);
}

__global__ void __launch_bounds__(256)
kck_k_list(const u8 *__restrict__ bad, u32 m, u32 *__restrict__ list, unsigned long long *__restrict__ cnt) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    kck_append(i < m && bad[i] != 0, i, list, cnt + KCK_LISTED);
}

// rows list[lo, lo + n): their 12 key words and flags, side by side (one lane per word)
__global__ void __launch_bounds__(256)
kck_k_gather(const u64 *__restrict__ pks, const u8 *__restrict__ pk_inf, const u32 *__restrict__ list, u32 lo, u32 n,
             u64 *__restrict__ g_pks, u8 *__restrict__ g_inf) {
    const u32 t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n * 12u) return;
    const u32 r = t / 12u, k = t % 12u, i = list[lo + r];
    g_pks[t] = pks[12 * (size_t)i + k];
    if (k == 0) g_inf[r] = pk_inf[i];
}

// the rebuilt tables and statuses back into rows list[lo, lo + n) (one lane per 16 bytes of table)
__global__ void __launch_bounds__(256)
kck_k_scatter(const u64 *__restrict__ g_tab, const u8 *__restrict__ g_status, const u32 *__restrict__ list, u32 lo, u32 n,
              u64 *__restrict__ tab, u8 *__restrict__ status) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (size_t)n * (KCK_TAB_WORDS / 2)) return;
    const u32 r = (u32)(t / (KCK_TAB_WORDS / 2)), k = (u32)(t % (KCK_TAB_WORDS / 2)), i = list[lo + r];
    reinterpret_cast<ulonglong2 *>(tab + (size_t)i * KCK_TAB_WORDS)[k] =
        reinterpret_cast<const ulonglong2 *>(g_tab + (size_t)r * KCK_TAB_WORDS)[k];
    if (k == 0) status[i] = g_status[r];
}

// a row's seven wire words as the 49 bytes decompress_lane reads (little-endian words: the bytes as they arrived)
SSA_DEV u32 kck_wire_decompress(const u64 *__restrict__ w, aff &P, bool &inf) {
    u64 buf[KY_WIRE_WORDS];
#pragma unroll
    for (int k = 0; k < KY_WIRE_WORDS; k++) buf[k] = w[k];
    return decompress_lane(reinterpret_cast<const u8 *>(buf), P, inf);
}

// bad[i] = 1 for a row whose stored key is not what its 49 bytes stand for (kck_k_tables wrote bad[] before)
__global__ void __launch_bounds__(256)
kck_k_wire(const u64 *__restrict__ wire, const u64 *__restrict__ pks, const u8 *__restrict__ pk_inf,
           const u8 *__restrict__ status, u32 m, u32 deep, u8 *__restrict__ bad) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const u64 *w = wire + (size_t)i * KY_WIRE_WORDS;
    const u64 flag = w[6];
    bool canon;
    const aff P = kck_ld_key(pks, i, canon);
    const bool zero = f6_is_zero(P.x) && f6_is_zero(P.y), inf = pk_inf[i] != 0;
    bool x_canon = true, x_zero = true, x_eq = true;
#pragma unroll
    for (int k = 0; k < 6; k++) {
        x_canon = x_canon && w[k] < FP_P;
        x_zero = x_zero && w[k] == 0;
        x_eq = x_eq && w[k] == P.x.c[k];
    }
    const bool f_inf = (flag & 0x80u) != 0, f_sort = (flag & 0x40u) != 0;
    bool fail;
    if (flag > 0xffull) {
        fail = true;                                           // (the word holds one byte)
    } else if ((flag & 0x3fu) || !x_canon || (f_inf && (!x_zero || f_sort))) {
        fail = !zero || inf;                                   // cannot decode: (0, 0), no flag
    } else if (f_inf) {
        fail = !zero || !inf;                                  // the identity
    } else if (zero && !inf) {
        fail = false;                                          // "not a square": DEEP looks below
    } else {
        fail = inf || !canon || !x_eq || f6_lex_largest(P.y) != f_sort;
    }
    if (!fail && deep && status[i] == ST_MALFORMED) {
        aff Q;
        bool q_inf;
        fail = kck_wire_decompress(w, Q, q_inf) == 0;          // it decodes after all
    }
    if (fail) bad[i] = 1;
}

// rows list[0, n): the 96 bytes and the flag again from the 49 bytes (a flag word with more than its byte set is cut)
__global__ void __launch_bounds__(256)
kck_k_wire_rebuild(u64 *__restrict__ wire, const u32 *__restrict__ list, u32 n, u32 m, u64 *__restrict__ pks,
                   u8 *__restrict__ pk_inf) {
    const u32 t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const u32 i = list[t];
    if (i >= m) return;       // (never)
    u64 *w = wire + (size_t)i * KY_WIRE_WORDS;
    if (w[6] > 0xffull) w[6] &= 0xffull;
    aff P;
    bool inf;
    (void)kck_wire_decompress(w, P, inf);
#pragma unroll
    for (int k = 0; k < 6; k++) {
        pks[12 * (size_t)i + k] = P.x.c[k];
        pks[12 * (size_t)i + 6 + k] = P.y.c[k];
    }
    pk_inf[i] = inf ? 1 : 0;
}

#endif  // SSA_CHECK_FUNCTIONS_ONLY
}  // namespace ssa

#ifndef SSA_CHECK_FUNCTIONS_ONLY
// the rows of a key set or a key cache as the check sees them
struct KeyRows {
    ssa_ctx *ctx;
    const u64 *pks;
    const u8 *inf;
    u8 *status;
    u64 *tab;
    const u64 *ktab;      // per-key combs (key sets in comb mode), or nullptr
    size_t m;
    u64 *wire = nullptr;  // the rows' 49 compressed bytes, seven words each (key caches in wire mode), or nullptr
};

static inline size_t kck_pad(size_t m) { return (m + 15) & ~(size_t)15; }

// One pass over the rows: res[] = the KCK_* counters.  ctx->kck_ws holds bad[m] (padded to 16 bytes), the rebuild list
// and the deep / repair list (m words each); ctx->ws_tab the scratch tables of a chunk of status-1 keys.
static int keycheck_pass(const KeyRows &r, bool deep, uint64_t res[KCK_WORDS]) {
    ssa_ctx *ctx = r.ctx;
    const size_t m = r.m;
    if (ctx->tc_out.reserve(KCK_WORDS * sizeof(u64)) || ctx->kck_ws.reserve(kck_pad(m) + 2 * m * sizeof(u32)))
        return SSA_ERR_HIP;
    unsigned long long *d = (unsigned long long *)ctx->tc_out.p;
    u8 *bad = (u8 *)ctx->kck_ws.p;
    u32 *rebuild_list = (u32 *)(bad + kck_pad(m)), *deep_list = rebuild_list + m;
    HIP_TRY(hipMemsetAsync(d, 0, KCK_WORDS * sizeof(u64), ctx->stream));
    HIP_TRY(hipMemsetAsync(d + KCK_FIRST, 0xff, sizeof(u64), ctx->stream));
    if (int rc = timed_launch(ctx, "ssa_k_keytab_check", [&] {
            hipLaunchKernelGGL(kck_k_tables, dim3(grid_for(m, 256)), dim3(256), 0, ctx->stream, r.pks, r.inf,
                               (const u8 *)r.status, (const u64 *)r.tab, (u32)m, deep ? 1u : 0u, bad, rebuild_list,
                               deep_list, d);
        }))
        return rc;
    HIP_TRY(hipMemcpyAsync(res, d, KCK_WORDS * sizeof(u64), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    const size_t n_rebuild = (size_t)res[KCK_REBUILD], n_st0 = (size_t)res[KCK_ST0];
    if (n_rebuild > m || n_st0 > m) return SSA_ERR_HIP;      // (never)
    for (size_t lo = 0; lo < n_rebuild; lo += KCK_CHUNK) {
        const size_t n = n_rebuild - lo < KCK_CHUNK ? n_rebuild - lo : KCK_CHUNK;
        if (ctx->ws_tab.reserve(n * KCK_TAB_WORDS * sizeof(u64))) return SSA_ERR_HIP;
        if (int rc = timed_launch(ctx, "ssa_k_keytab_rebuild", [&] {
                hipLaunchKernelGGL(kck_k_rebuild, dim3(grid_for(n, 256)), dim3(256), 0, ctx->stream, r.pks, r.inf,
                                   (const u64 *)r.tab, (const u32 *)rebuild_list, (u32)lo, (u32)n, (u64 *)ctx->ws_tab.p,
                                   deep ? 1u : 0u, bad, deep_list, d);
            }))
            return rc;
    }
    if (deep && n_st0 + n_rebuild)
        if (int rc = timed_launch(ctx, "ssa_k_keytab_deep", [&] {
                hipLaunchKernelGGL(kck_k_deep, dim3(grid_for(n_st0 + n_rebuild, 256)), dim3(256), 0, ctx->stream,
                                   (const u64 *)r.tab, (const u8 *)r.status, (const u32 *)deep_list,
                                   (const unsigned long long *)d, bad);
            }))
            return rc;
    if (r.wire)
        if (int rc = timed_launch(ctx, "ssa_k_keytab_check", [&] {
                hipLaunchKernelGGL(kck_k_wire, dim3(grid_for(m, 256)), dim3(256), 0, ctx->stream, (const u64 *)r.wire, r.pks,
                                   r.inf, (const u8 *)r.status, (u32)m, deep ? 1u : 0u, bad);
            }))
            return rc;
    if (r.ktab)
        if (int rc = timed_launch(ctx, "ssa_k_keycomb_check", [&] {
                hipLaunchKernelGGL(kck_k_comb, dim3((unsigned)(m * KCK_COMB_BLOCKS)), dim3(256), 0, ctx->stream, r.pks,
                                   r.inf, (const u8 *)r.status, r.ktab, (u32)m, bad, d);
            }))
            return rc;
    if (int rc = timed_launch(ctx, "ssa_k_keytab_check", [&] {
            hipLaunchKernelGGL(kck_k_count, dim3(grid_for(m, 256)), dim3(256), 0, ctx->stream, (const u8 *)bad, (u32)m, d);
        }))
        return rc;
    HIP_TRY(hipMemcpyAsync(res, d, KCK_WORDS * sizeof(u64), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return 0;
}

// the failing rows of the last pass (bad[] in ctx->kck_ws) rebuilt in place from their stored bytes
static int keycheck_repair(const KeyRows &r, uint64_t *rebuilt) {
    ssa_ctx *ctx = r.ctx;
    const size_t m = r.m;
    unsigned long long *d = (unsigned long long *)ctx->tc_out.p;
    u8 *bad = (u8 *)ctx->kck_ws.p;
    u32 *list = (u32 *)(bad + kck_pad(m)) + m;
    uint64_t n_bad = 0;
    if (int rc = timed_launch(ctx, "keycheck_repair", [&] {
            hipLaunchKernelGGL(kck_k_list, dim3(grid_for(m, 256)), dim3(256), 0, ctx->stream, (const u8 *)bad, (u32)m, list, d);
        }))
        return rc;
    HIP_TRY(hipMemcpyAsync(&n_bad, d + KCK_LISTED, sizeof n_bad, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (n_bad > m) return SSA_ERR_HIP;      // (never)
    if (r.wire && n_bad)        // a wire row is rebuilt from its 49 bytes: first the 96 bytes and the flag they stand for
        if (int rc = timed_launch(ctx, "keycheck_repair", [&] {
                hipLaunchKernelGGL(kck_k_wire_rebuild, dim3(grid_for(n_bad, 256)), dim3(256), 0, ctx->stream, r.wire,
                                   (const u32 *)list, (u32)n_bad, (u32)m, (u64 *)r.pks, (u8 *)r.inf);
            }))
            return rc;
    // a chunk's scratch in ws_tab: the tables, then the gathered key words, flags and statuses
    constexpr size_t TAB_BYTES = KCK_TAB_WORDS * sizeof(u64);
    for (size_t lo = 0; lo < n_bad; lo += KCK_CHUNK) {
        const size_t n = n_bad - lo < KCK_CHUNK ? n_bad - lo : KCK_CHUNK;
        if (ctx->ws_tab.reserve(n * (TAB_BYTES + 96) + 2 * kck_pad(n))) return SSA_ERR_HIP;
        u64 *g_tab = (u64 *)ctx->ws_tab.p, *g_pks = g_tab + n * KCK_TAB_WORDS;
        u8 *g_inf = (u8 *)(g_pks + 12 * n), *g_status = g_inf + kck_pad(n);
        if (int rc = timed_launch(ctx, "keycheck_repair", [&] {
                hipLaunchKernelGGL(kck_k_gather, dim3(grid_for(n * 12, 256)), dim3(256), 0, ctx->stream, r.pks, r.inf,
                                   (const u32 *)list, (u32)lo, (u32)n, g_pks, g_inf);
            }))
            return rc;
        if (int rc = ssa_internal_keyset_build(ctx, (const uint8_t *)g_pks, g_inf, n, g_tab, g_status)) return rc;
        if (int rc = timed_launch(ctx, "keycheck_repair", [&] {
                hipLaunchKernelGGL(kck_k_scatter, dim3(grid_for(n * (KCK_TAB_WORDS / 2), 256)), dim3(256), 0, ctx->stream,
                                   (const u64 *)g_tab, (const u8 *)g_status, (const u32 *)list, (u32)lo, (u32)n, r.tab,
                                   r.status);
            }))
            return rc;
    }
    *rebuilt = n_bad;
    return 0;
}

static int keycheck_run(const KeyRows &r, uint32_t flags, uint8_t *bad_out, uint64_t out[8]) {
    for (int k = 0; k < 8; k++) out[k] = 0;
    out[2] = TC_NONE;
    if (r.m == 0) return 0;
    HIP_TRY(hipSetDevice(r.ctx->device));
    const bool deep = (flags & SSA_KEYCHECK_DEEP) != 0;
    uint64_t res[KCK_WORDS];
    if (int rc = keycheck_pass(r, deep, res)) return rc;
    out[0] = r.m;
    out[1] = res[KCK_BAD];
    out[2] = res[KCK_FIRST];
    out[3] = (uint64_t)PTAB_ENTRIES * res[KCK_ST0];
    out[4] = r.ktab ? (r.m - res[KCK_COMB_SKIPPED]) * (uint64_t)KTAB_ENTRIES_PER_KEY : 0;
    out[5] = res[KCK_REBUILD];
    out[6] = r.ktab ? res[KCK_COMB_SKIPPED] : 0;
    if (bad_out) {
        HIP_TRY(hipMemcpyAsync(bad_out, r.ctx->kck_ws.p, r.m, hipMemcpyDeviceToHost, r.ctx->stream));
        HIP_TRY(hipStreamSynchronize(r.ctx->stream));
    }
    if (res[KCK_BAD] == 0) return 0;
    if (!(flags & SSA_KEYCHECK_REPAIR)) return SSA_ERR_TABLE;
    if (int rc = keycheck_repair(r, &out[7])) return rc;
    if (int rc = keycheck_pass(r, deep, res)) return rc;       // the rebuilt rows, and every other, once more
    return res[KCK_BAD] ? SSA_ERR_TABLE : 0;
}

static KeyRows keyset_rows(ssa_keyset *ks) {
    return {ks->ctx, (const u64 *)ks->pks.p, (const u8 *)ks->inf.p, (u8 *)ks->status.p, (u64 *)ks->tab.p,
            ks->comb ? (const u64 *)ks->ktab.p : nullptr, ks->m};
}
static KeyRows keycache_rows(ssa_keycache *kc) {
    return {kc->ctx, (const u64 *)kc->rows.pks.p, (const u8 *)kc->inf.p, (u8 *)kc->rows.status.p, (u64 *)kc->rows.tab.p,
            nullptr, kc->held, kc->wire_mode ? (u64 *)kc->wire.p : nullptr};
}

extern "C" int ssa_keyset_selfcheck(ssa_keyset *ks, uint32_t flags, uint8_t *bad_out, uint64_t out[8]) {
    if (!ks || !ks->ctx || !out || (flags & ~SSA_KEYCHECK_DEEP)) return SSA_ERR_ARG;
    return keycheck_run(keyset_rows(ks), flags, bad_out, out);
}

extern "C" int ssa_keycache_selfcheck(ssa_keycache *kc, uint32_t flags, uint64_t out[8]) {
    if (!kc || !kc->ctx || !out || (flags & ~(SSA_KEYCHECK_DEEP | SSA_KEYCHECK_REPAIR))) return SSA_ERR_ARG;
    return keycheck_run(keycache_rows(kc), flags, nullptr, out);
}

// where `what` of key `key` lives on the device: *p, its size in words (or 1 byte: *bytes) -- SSA_ERR_ARG outside the object
static int debug_keytab_span(ssa_keyset *ks, ssa_keycache *kc, int what, uint64_t key, ssa_ctx **ctx, u8 **p,
                             uint64_t *words, bool *bytes) {
    if ((ks == nullptr) == (kc == nullptr)) return SSA_ERR_ARG;
    if (ks ? !ks->ctx : !kc->ctx) return SSA_ERR_ARG;
    const KeyRows r = ks ? keyset_rows(ks) : keycache_rows(kc);
    if (key >= r.m) return SSA_ERR_ARG;
    *ctx = r.ctx;
    *bytes = what == 1 || what == 3;
    switch (what) {
    case 0: *p = (u8 *)(r.tab + key * KCK_TAB_WORDS); *words = KCK_TAB_WORDS; return 0;
    case 1: *p = r.status + key; *words = 1; return 0;
    case 2: *p = (u8 *)(r.pks + 12 * key); *words = 12; return 0;
    case 3: *p = (u8 *)r.inf + key; *words = 1; return 0;
    case 4:
        if (!r.ktab) return SSA_ERR_ARG;
        *p = (u8 *)(r.ktab + key * KTAB_ENTRIES_PER_KEY * 12);
        *words = KTAB_ENTRIES_PER_KEY * 12;
        return 0;
    case 5:
        if (!r.wire) return SSA_ERR_ARG;
        *p = (u8 *)(r.wire + key * KY_WIRE_WORDS);
        *words = KY_WIRE_WORDS;
        return 0;
    default: return SSA_ERR_ARG;
    }
}

extern "C" int ssa_debug_keytab_xor(ssa_keyset *ks, ssa_keycache *kc, int what, uint64_t key, uint32_t word, uint64_t mask) {
    ssa_ctx *ctx;
    u8 *p;
    uint64_t words;
    bool bytes;
    if (int rc = debug_keytab_span(ks, kc, what, key, &ctx, &p, &words, &bytes)) return rc;
    if (word >= words || (bytes && mask > 0xffull)) return SSA_ERR_ARG;
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t sz = bytes ? 1 : sizeof(u64);
    u64 v = 0;
    p += (size_t)word * sz;
    HIP_TRY(hipMemcpyAsync(&v, p, sz, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    v ^= mask;
    HIP_TRY(hipMemcpyAsync(p, &v, sz, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return 0;
}

extern "C" int ssa_debug_keytab_read(ssa_keyset *ks, ssa_keycache *kc, int what, uint64_t key, uint64_t *words_out) {
    ssa_ctx *ctx;
    u8 *p;
    uint64_t words;
    bool bytes;
    if (!words_out) return SSA_ERR_ARG;
    if (int rc = debug_keytab_span(ks, kc, what, key, &ctx, &p, &words, &bytes)) return rc;
    if (what == 4) words = 2 * 12;          // rows (0, 0) and (0, 1) of the key's comb
    HIP_TRY(hipSetDevice(ctx->device));
    if (bytes) words_out[0] = 0;
    HIP_TRY(hipMemcpyAsync(words_out, p, bytes ? 1 : words * sizeof(u64), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return 0;
}
#endif  // SSA_CHECK_FUNCTIONS_ONLY
