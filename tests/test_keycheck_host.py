"""Self-check of key-set and key-cache tables (ssa_keyset_selfcheck, ssa_keycache_selfcheck), host
side (no GPU): the C ABI it adds, the refusals that need no device, a big-integer model of the ladder-table check
(oracle/pymodel.py arithmetic, raw 64-bit words compared as the kernel compares them), and a static check of the new
kernels' instructions."""
import ctypes as C
import hashlib
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import pymodel as m
import schnorr_sig_amd as ssa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "schnorr-sig_amd", "csrc")
CACHE = os.path.join(ROOT, "build", "keycheck_static")
HDR = os.path.join(ROOT, "include", "schnorr_sig_amd.h")
NEW_SYMBOLS = ["ssa_keyset_selfcheck", "ssa_keycache_selfcheck", "ssa_debug_keytab_xor", "ssa_debug_keytab_read"]
# kernels that run over every key (or every comb row) of the object, and the one that runs over the rare status-1 keys
EVERY_KEY_KERNELS = ["kck_k_tables", "kck_k_deep", "kck_k_comb", "kck_k_count", "kck_k_list", "kck_k_gather", "kck_k_scatter"]
RARE_KEY_KERNELS = ["kck_k_rebuild"]
DEEP, REPAIR = 1, 2


def test_header_declares_the_calls_the_hooks_and_the_flags():
    hdr = open(HDR).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint %s\s*\(" % name, hdr), name
    assert re.search(r"#define SSA_KEYCHECK_DEEP\s+1u\b", hdr)
    assert re.search(r"#define SSA_KEYCHECK_REPAIR\s+2u\b", hdr)
    assert re.search(r"#define SSA_ABI_VERSION 5\b", hdr)
    assert re.search(r"int ssa_keyset_selfcheck\(ssa_keyset \*ks, uint32_t flags, uint8_t \*bad_out, uint64_t out\[8\]\);", hdr)
    assert re.search(r"int ssa_keycache_selfcheck\(ssa_keycache \*kc, uint32_t flags, uint64_t out\[8\]\);", hdr)
    # what a light check does not see is said where the caller reads it
    assert "WITHOUT SSA_KEYCHECK_DEEP A STATUS BYTE FLIPPED BETWEEN 0 AND 1 IS NOT DETECTED" in hdr
    assert "COMBS OF KEYS OF STATUS 1 OR 3 ARE NOT" in hdr


def test_library_exports_them_and_the_abi_version_stays():
    lib = C.CDLL(ssa.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in ssa.ABI_SYMBOLS, name
    assert ssa._lib.ssa_abi_version() == 5
    assert (ssa.KEYCHECK_DEEP, ssa.KEYCHECK_REPAIR) == (DEEP, REPAIR)
    for cls in (ssa.KeySet, ssa.KeyCache):
        for name in ("selfcheck", "debug_keytab_xor", "debug_keytab_read"):
            assert hasattr(cls, name), (cls, name)
    assert len(ssa.KEYCHECK_FIELDS) == 8


def test_refusals_that_need_no_device():
    lib = ssa._lib
    out = (C.c_uint64 * 8)(*([9] * 8))
    bad = (C.c_uint8 * 16)(*([7] * 16))
    orphan = (C.c_uint8 * 65536)()            # an object whose context pointer is NULL: orphaned, nothing behind it
    for flags in (0, DEEP):
        assert lib.ssa_keyset_selfcheck(None, flags, bad, out) == ssa.ERR_ARG
        assert lib.ssa_keyset_selfcheck(None, flags, None, out) == ssa.ERR_ARG
        assert lib.ssa_keyset_selfcheck(orphan, flags, bad, out) == ssa.ERR_ARG
        assert lib.ssa_keyset_selfcheck(orphan, flags, bad, None) == ssa.ERR_ARG
    for flags in (0, DEEP, REPAIR, DEEP | REPAIR):
        assert lib.ssa_keycache_selfcheck(None, flags, out) == ssa.ERR_ARG
        assert lib.ssa_keycache_selfcheck(orphan, flags, out) == ssa.ERR_ARG
        assert lib.ssa_keycache_selfcheck(orphan, flags, None) == ssa.ERR_ARG
    for flags in (4, 8, 1 << 31, DEEP | 4):
        assert lib.ssa_keyset_selfcheck(orphan, flags, bad, out) == ssa.ERR_ARG, flags
        assert lib.ssa_keycache_selfcheck(orphan, flags, out) == ssa.ERR_ARG, flags
    for flags in (REPAIR, DEEP | REPAIR):     # a key set has no repair
        assert lib.ssa_keyset_selfcheck(orphan, flags, bad, out) == ssa.ERR_ARG, flags
    assert list(out) == [9] * 8 and list(bad) == [7] * 16        # a refused call writes nothing
    words = (C.c_uint64 * 512)()
    for what in range(5):
        assert lib.ssa_debug_keytab_xor(None, None, what, 0, 0, 1) == ssa.ERR_ARG
        assert lib.ssa_debug_keytab_xor(orphan, orphan, what, 0, 0, 1) == ssa.ERR_ARG      # exactly one
        assert lib.ssa_debug_keytab_xor(orphan, None, what, 0, 0, 1) == ssa.ERR_ARG
        assert lib.ssa_debug_keytab_xor(None, orphan, what, 0, 0, 1) == ssa.ERR_ARG
        assert lib.ssa_debug_keytab_read(None, None, what, 0, words) == ssa.ERR_ARG
        assert lib.ssa_debug_keytab_read(orphan, None, what, 0, words) == ssa.ERR_ARG
        assert lib.ssa_debug_keytab_read(None, orphan, what, 0, None) == ssa.ERR_ARG


def test_cxx_mirror_declares_the_selfchecks(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    src = tmp_path / "t.cpp"
    src.write_text('#include "%s/schnorr-sig_amd/host/schnorr_sig.hpp"\n'
                   "using namespace schnorr_sig;\n"
                   "bool f(Context &cx, const std::vector<PublicKey> &p) {\n"
                   "  KeyCache cache(cx, 1024);\n"
                   "  KeySet ks(cx, p);\n"
                   "  KeyCheck a = cache.selfcheck(), b = cache.selfcheck(true, true), c = ks.selfcheck(), d = ks.selfcheck(true);\n"
                   "  return a.ok && b.rows_repaired == 0 && c.bad.size() == p.size() && d.keys_bad == 0 &&\n"
                   "         d.first_bad_key == UINT64_MAX && a.keys_checked + a.ladder_entries_checked + a.comb_rows_checked +\n"
                   "         a.keys_rebuilt_and_compared + a.combs_skipped == 0;\n"
                   "}\n" % ROOT)
    subprocess.check_call([cxx, "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", str(src)])


# ---- the model: a key's row as the device holds it (raw 64-bit words) and the check of kck_k_tables ----------------
ENTRIES, ENTRY_WORDS, NEG = 16, 32, 16
CHECKED = list(range(0, 12)) + list(range(16, 28))           # the words of an entry that kernels read
PADDING = [12, 13, 14, 15, 28, 29, 30, 31]


def chain_rel(R, P, Q, tangent):
    """section 11's two equations; False on den == 0"""
    (xr, yr), (xp, yp) = R, P
    if tangent:
        num = m.f6_add(m.f6_scale(m.f6_sqr(xp), 3), m.F6_ONE)
        den = m.f6_scale(yp, 2)
        xs = m.f6_scale(xp, 2)
    else:
        xq, yq = Q
        num, den, xs = m.f6_sub(yq, yp), m.f6_sub(xq, xp), m.f6_add(xp, xq)
    if den == m.F6_ZERO:
        return False
    ex = m.f6_mul(m.f6_add(xr, xs), m.f6_sqr(den)) == m.f6_sqr(num)
    ey = m.f6_mul(m.f6_add(yr, yp), den) == m.f6_mul(num, m.f6_sub(xp, xr))
    return ex and ey


def res(words):
    """six raw words as an Fp6 element: the table holds loose limbs, each standing for its residue"""
    return tuple(int(w) % m.P for w in words)


def table_words(points):
    """the 512 words of a ladder table whose entries are `points` (None: the (0, 0) sentinel), padding words zero"""
    t = [0] * (ENTRIES * ENTRY_WORDS)
    for e, pt in enumerate(points):
        x, y = pt if pt is not None else (m.F6_ZERO, m.F6_ZERO)
        ny = m.f6_neg(y)
        t[e * ENTRY_WORDS:e * ENTRY_WORDS + 12] = list(x) + list(y)
        t[e * ENTRY_WORDS + NEG:e * ENTRY_WORDS + NEG + 12] = list(x) + list(ny)
    return t


def key_words(pt):
    return list(pt[0]) + list(pt[1])


def check_status0(tab, key, inf):
    """the check of a key of stored status 0 -> (passes, first failing entry or None; -1: the key bytes themselves)"""
    if any(w >= m.P for w in key):
        return False, -1
    P = (tuple(key[:6]), tuple(key[6:]))
    if inf:
        for e in range(ENTRIES):
            if any(tab[e * ENTRY_WORDS + w] % m.P for w in CHECKED):
                return False, e
        return True, None
    if not m.on_curve(P):
        return False, -1
    prev = P
    for e in range(ENTRIES):
        row = tab[e * ENTRY_WORDS:(e + 1) * ENTRY_WORDS]
        R = (res(row[0:6]), res(row[6:12]))
        N = (res(row[16:22]), res(row[22:28]))
        ok = N[0] == R[0] and m.f6_add(N[1], R[1]) == m.F6_ZERO
        if e == 0:
            ok = ok and list(row[0:12]) == list(key)                  # bit for bit
        else:
            ok = ok and chain_rel(R, P if e == 1 else prev, P, e == 1)
        if not ok:
            return False, e
        prev = R
    return True, None


def multiples(P):
    out, acc = [], None
    for _ in range(ENTRIES):
        acc = m.pt_add(acc, P)
        out.append(acc)
    return out


@pytest.fixture(scope="module")
def subgroup_key():
    rng = np.random.default_rng(17001)
    k = int.from_bytes(rng.integers(0, 256, 32, dtype=np.uint8).tobytes(), "little") % m.Q
    P = m.pt_mul(k, m.default_params().generator())
    assert m.on_curve(P) and m.is_torsion_free(P)
    return P


def test_true_table_of_a_subgroup_key_passes(subgroup_key):
    tab = table_words(multiples(subgroup_key))
    assert check_status0(tab, key_words(subgroup_key), False) == (True, None)
    # a loose limb (the residue + p still fits 64 bits) is the same table: the builder stores such limbs
    for e, w in ((3, 2), (9, 23), (15, 7)):
        v = tab[e * ENTRY_WORDS + w]
        if v + m.P < 2 ** 64:
            loose = list(tab)
            loose[e * ENTRY_WORDS + w] = v + m.P
            assert check_status0(loose, key_words(subgroup_key), False) == (True, None)


def test_every_single_word_flip_is_found_at_its_entry(subgroup_key):
    rng = np.random.default_rng(17002)
    tab = table_words(multiples(subgroup_key))
    key = key_words(subgroup_key)
    for e in range(ENTRIES):
        for w in CHECKED:                                            # both halves: words 16..27 are (x, -y)
            bad = list(tab)
            bad[e * ENTRY_WORDS + w] ^= 1 << int(rng.integers(0, 64))
            assert check_status0(bad, key, False) == (False, e), (e, w)


def test_a_flip_in_a_padding_word_is_not_reported(subgroup_key):
    tab = table_words(multiples(subgroup_key))
    key = key_words(subgroup_key)
    for e in range(ENTRIES):
        for w in PADDING:
            bad = list(tab)
            bad[e * ENTRY_WORDS + w] ^= 0xDEADBEEF00000001
            assert check_status0(bad, key, False) == (True, None), (e, w)


def test_key_byte_flips_are_found(subgroup_key):
    tab = table_words(multiples(subgroup_key))
    for w in range(12):
        key = key_words(subgroup_key)
        key[w] ^= 1 << (5 * w)
        ok, where = check_status0(tab, key, False)
        assert not ok and where in (-1, 0), (w, where)


def test_identity_key_all_sentinel_table_passes_and_a_real_table_under_the_flag_fails(subgroup_key):
    sentinel = table_words([None] * ENTRIES)
    assert check_status0(sentinel, [0] * 12, True) == (True, None)
    bad = list(sentinel)
    bad[5 * ENTRY_WORDS + 22] = 1
    assert check_status0(bad, [0] * 12, True) == (False, 5)
    assert check_status0(table_words(multiples(subgroup_key)), key_words(subgroup_key), True) == (False, 0)
    # ... and the flag flipped the other way: (0, 0) is not on the curve
    assert check_status0(sentinel, [0] * 12, False) == (False, -1)


def test_a_valid_chain_on_another_curve_constant_is_refused():
    """chords and tangents use only a = 1: the multiples of a point of y^2 = x^3 + x + b', b' != b, satisfy every relation"""
    rng = np.random.default_rng(17003)
    P = (tuple(int(v) % m.P for v in rng.integers(0, 2 ** 63, 6)), tuple(int(v) % m.P for v in rng.integers(0, 2 ** 63, 6)))
    assert not m.on_curve(P)
    pts = multiples(P)
    for e in range(1, ENTRIES):
        assert chain_rel(pts[e], P if e == 1 else pts[e - 1], P, e == 1)
    assert check_status0(table_words(pts), key_words(P), False) == (False, -1)


# ---- the library's own per-key check, compiled for the CPU, on the tables its own builder makes ---------------------
HOST_SRC = os.path.join(ROOT, "tests", "csrc", "keycheck_host.cpp")
HOST_LIB = os.path.join(ROOT, "tests", "csrc", "libkeycheck_host.so")
PASS, FAIL, REBUILD = 0, 1, 2


@pytest.fixture(scope="module")
def host_twin():
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not available")
    deps = [HOST_SRC] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".hpp", ".inc"))]
    if not os.path.exists(HOST_LIB) or os.path.getmtime(HOST_LIB) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["hipcc", "--cuda-host-only", "-x", "hip", "-O2", "-shared", "-fPIC", HOST_SRC, "-o", HOST_LIB])
    return C.CDLL(HOST_LIB)


def _arr(words):
    return (C.c_uint64 * len(words))(*[int(w) for w in words])


def _build(lib, key, inf=False):
    tab = (C.c_uint64 * (ENTRIES * ENTRY_WORDS))()
    status = lib.kh_build(_arr(key), int(inf), tab)
    return list(tab), status


def test_builder_and_check_agree_on_a_subgroup_key(host_twin, subgroup_key):
    """build_ptab's table is the model's (as residues), passes kck_chain_ok, and the Python model passes it too"""
    key = key_words(subgroup_key)
    tab, status = _build(host_twin, key)
    assert status == 0
    model = table_words(multiples(subgroup_key))
    for e in range(ENTRIES):
        for w in CHECKED:
            assert tab[e * ENTRY_WORDS + w] % m.P == model[e * ENTRY_WORDS + w], (e, w)
    assert tab[:12] == key                                           # entry 1P: the key, bit for bit
    assert host_twin.kh_light(_arr(key), 0, 0, _arr(tab)) == PASS
    assert check_status0(tab, key, False) == (True, None)


def test_the_compiled_check_finds_every_single_word_flip_and_ignores_padding(host_twin, subgroup_key):
    rng = np.random.default_rng(17004)
    key = key_words(subgroup_key)
    tab, _ = _build(host_twin, key)
    for e in range(ENTRIES):
        for w in CHECKED:
            bad = list(tab)
            bad[e * ENTRY_WORDS + w] ^= 1 << int(rng.integers(0, 64))
            assert host_twin.kh_light(_arr(key), 0, 0, _arr(bad)) == FAIL, (e, w)
        for w in PADDING:
            bad = list(tab)
            bad[e * ENTRY_WORDS + w] ^= 0xDEADBEEF00000001
            assert host_twin.kh_light(_arr(key), 0, 0, _arr(bad)) == PASS, (e, w)
    for w in range(12):                                              # the key bytes themselves
        k2 = list(key)
        k2[w] ^= 1 << (5 * w)
        assert host_twin.kh_light(_arr(k2), 0, 0, _arr(tab)) == FAIL, w
    loose = [(e, w) for e in range(ENTRIES) for w in CHECKED if w >= 12 or e > 0
             if tab[e * ENTRY_WORDS + w] % m.P + m.P < 2 ** 64][:4]
    for e, w in loose:                                               # x and x + p are one residue: the same table
        same = list(tab)
        same[e * ENTRY_WORDS + w] = tab[e * ENTRY_WORDS + w] % m.P + m.P
        assert host_twin.kh_light(_arr(key), 0, 0, _arr(same)) == PASS, (e, w)


def test_the_compiled_check_on_the_special_keys(host_twin, subgroup_key):
    key = key_words(subgroup_key)
    tab, _ = _build(host_twin, key)
    zero = [0] * 12
    sentinel, status = _build(host_twin, zero, inf=True)
    assert status == 0 and not any(sentinel[e * ENTRY_WORDS + w] % m.P for e in range(ENTRIES) for w in CHECKED)
    assert host_twin.kh_light(_arr(zero), 1, 0, _arr(sentinel)) == PASS
    assert host_twin.kh_light(_arr(zero), 0, 0, _arr(sentinel)) == FAIL      # pk_inf 1 -> 0: (0, 0) is off the curve
    assert host_twin.kh_light(_arr(key), 1, 0, _arr(tab)) == FAIL            # pk_inf 0 -> 1: a real table, no sentinels
    t2 = m.SMALL_ORDER_POINTS[2]
    for pt, light_if_status_0 in ((t2, FAIL), (m.pt_add(subgroup_key, t2), PASS)):
        k2 = key_words(pt)
        t, status = _build(host_twin, k2)
        assert status == 1
        assert host_twin.kh_light(_arr(k2), 0, 1, _arr(t)) == REBUILD
        # a status flipped 1 -> 0: the table of P + T2 is a true chain (only DEEP sees it), the point of order 2 has a
        # sentinel as its 2P
        assert host_twin.kh_light(_arr(k2), 0, 0, _arr(t)) == light_if_status_0
        assert host_twin.kh_light(_arr(k2), 0, 3, _arr(t)) == FAIL           # well-formed bytes under status 3
    off = list(key)
    off[7] ^= 1
    noncanon = list(key)
    noncanon[0] = 2 ** 64 - 1
    for k2 in (off, noncanon):
        assert host_twin.kh_light(_arr(k2), 0, 3, _arr(tab)) == PASS         # the status really is 3
        for st in (0, 1, 2, 4, 255):
            assert host_twin.kh_light(_arr(k2), 0, st, _arr(tab)) == FAIL, st
    for st in (2, 4, 255):
        assert host_twin.kh_light(_arr(key), 0, st, _arr(tab)) == FAIL, st


# ---- static check of the new kernels' instructions --------------------------------------------------------------
def _asm():
    """gfx950 assembly of the translation unit that holds the new kernels (cached by the content of its sources)"""
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not available")
    deps = [os.path.join(CSRC, f) for f in sorted(os.listdir(CSRC)) if f.endswith((".hip", ".hpp", ".inc"))]
    deps.append(HDR)
    h = hashlib.sha256()
    for p in deps:
        h.update(os.path.basename(p).encode() + b"\0" + open(p, "rb").read() + b"\0")
    os.makedirs(CACHE, exist_ok=True)
    out, stamp = os.path.join(CACHE, "ssa_sign.s"), os.path.join(CACHE, "ssa_sign.s.srchash")
    if not (os.path.exists(out) and os.path.exists(stamp) and open(stamp).read().strip() == h.hexdigest()):
        subprocess.check_call(["hipcc", "-O3", "--offload-arch=gfx950", "-std=c++17", "--cuda-device-only", "-S", "-o", out,
                               os.path.join(CSRC, "ssa_sign.hip")], stderr=subprocess.DEVNULL)
        open(stamp, "w").write(h.hexdigest() + "\n")
    return open(out).read()


def _kernel_bodies(text):
    out = {}
    for ch in re.split(r"^(?=_ZN3ssa\w+:)", text, flags=re.M):
        mm = re.match(r"_ZN3ssa(\d+)(\w+):", ch)
        if mm:
            out[mm.group(2)[:int(mm.group(1))]] = ch.split(".Lfunc_end")[0]
    return out


def _private_segment_bytes(text):
    """kernel name -> the fixed private segment (scratch) of its kernel descriptor"""
    out = {}
    for mm in re.finditer(r"\.amdhsa_kernel _ZN3ssa(\d+)(\w+)\n(.*?)\.end_amdhsa_kernel", text, re.S):
        size = re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", mm.group(3))
        out[mm.group(2)[:int(mm.group(1))]] = int(size.group(1))
    return out


def test_keycheck_kernels_use_vector_memory_instructions_only_and_no_scratch():
    """The static check of tests/test_keycache_host.py on the new kernels and their translation unit: no scalar store, no
    scalar atomic, no scalar cache write-back or discard (the mnemonics are put together from parts).  No kernel has a
    scratch instruction in its body, and the kernels that run over every key have no private segment at all.  The
    rebuild-and-compare kernel of the rare status-1 keys calls build_ptab, whose out-of-line helpers (the ones
    ssa_k_keyset_build calls) keep a call frame: its private segment is theirs and is bounded here."""
    s = "s_"
    forbidden = [s + stem + r"\w*" for stem in ("store_", "buffer_" + "store_", "scratch_" + "store_", "atomic_",
                                                "buffer_" + "atomic_", "dcache_" + "wb", "dcache_" + "discard")]
    pat = re.compile(r"^\s*(" + "|".join(forbidden) + r")\b", re.M)
    text = _asm()
    bodies = _kernel_bodies(text)
    private = _private_segment_bytes(text)
    for k in EVERY_KEY_KERNELS + RARE_KEY_KERNELS + ["ssa_k_gtab_check"]:
        assert k in bodies, "kernel %s is not in the code object" % k
        body = bodies[k]
        assert len(body.splitlines()) > 10, k
        assert not pat.search(body), (k, pat.search(body).group(0))
        assert not re.search(r"^\s*scratch_", body, re.M), k
    for k in EVERY_KEY_KERNELS + ["ssa_k_gtab_check"]:
        assert private[k] == 0, (k, private[k])
    assert private["kck_k_rebuild"] <= 512, private["kck_k_rebuild"]
    # counts and the first failing key go through vector atomics, bad flags through plain byte stores
    assert re.search(r"^\s*global_atomic_(add|umin)_x2\b", bodies["kck_k_count"], re.M)
    assert re.search(r"^\s*global_atomic_umin_x2\b", bodies["kck_k_count"], re.M)
    assert re.search(r"^\s*global_store_byte\b", bodies["kck_k_tables"], re.M)
    for k in ("kck_k_deep", "kck_k_comb", "kck_k_gather", "kck_k_scatter"):
        assert not re.search(r"^\s*global_atomic_(?!add_x2)", bodies[k], re.M), k
    assert not pat.search(text), pat.search(text).group(0)
    src_pat = re.compile("|".join(f[:-3] for f in forbidden), re.I)
    for f in ("ssa_keycheck.hpp", "ssa_selfcheck.hpp", "ssa_sign.hip"):
        assert not src_pat.search(open(os.path.join(CSRC, f)).read()), f
