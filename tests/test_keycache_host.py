"""Key cache (ssa_keycache_create, ssa_verify_many_cached), host side (no GPU): the C ABI, the
argument checks, the policy ssa_debug_keycache_plan, the mirrors, and a static check of the new kernels' instructions."""
import ctypes as C
import hashlib
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import schnorr_sig_amd as ssa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "schnorr-sig_amd", "csrc")
CACHE = os.path.join(ROOT, "build", "keycache_static")
NEW_SYMBOLS = ["ssa_keycache_create", "ssa_keycache_destroy", "ssa_keycache_clear", "ssa_keycache_info",
               "ssa_verify_many_cached", "ssa_verify_many_cached_device", "ssa_debug_keycache_plan"]
NEW_KERNELS = ["kc_k_lookup", "kc_k_number", "kc_k_publish", "kc_k_map"]
INSERT, CLEAR, BYPASS = 0, 1, 2
MAX_CAPACITY = 1 << 24


def test_new_symbols_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "schnorr_sig_amd.h")).read()
    lib = C.CDLL(ssa.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name + "(" in hdr, name
        assert hasattr(lib, name), name
        assert name in ssa.ABI_SYMBOLS, name
    assert "typedef struct ssa_keycache ssa_keycache;" in hdr
    assert ssa._lib.ssa_abi_version() == 5           # additive: the ABI version does not move
    for name in ("keycache_create", "verify_many_cached", "verify_many_cached_device"):
        assert hasattr(ssa.Engine, name), name
    for name in ("info", "clear", "close", "__enter__", "__exit__"):
        assert hasattr(ssa.KeyCache, name), name
    assert callable(ssa.verify_many_cached)


def _host(lib, ctx, kc, *a):
    return lib.ssa_verify_many_cached(ctx, kc, *a[:9], None, *a[9:])


def _devf(lib, ctx, kc, *a):
    return lib.ssa_verify_many_cached_device(ctx, kc, *a[:9], None, 0, *a[9:])


def test_flag_bits_outside_the_two_are_refused_before_anything_else():
    lib = ssa._lib
    buf = (C.c_uint8 * 256)()
    nf = C.c_uint64(7)
    stats = (C.c_uint64 * 12)(*([9] * 12))
    fake = (C.c_uint8 * 65536)()                      # never dereferenced: the flags are looked at first
    for bad in (2, 4, 16, 32, 64, 1 | 2, 8 | 4, 1 << 31):
        assert lib.ssa_verify_many_cached(fake, fake, buf, buf, None, buf, None, 1, 1, 1, bad, None, buf, C.byref(nf),
                                          stats) == ssa.ERR_ARG, bad
        assert lib.ssa_verify_many_cached_device(fake, fake, buf, buf, None, buf, None, 1, 1, 1, bad, None, 0, buf, None,
                                                 stats) == ssa.ERR_ARG, bad
        # ... even with no context and no cache at all
        assert lib.ssa_verify_many_cached(None, None, buf, buf, None, buf, None, 1, 1, 1, bad, None, buf, C.byref(nf),
                                          stats) == ssa.ERR_ARG, bad
    assert list(stats) == [9] * 12 and nf.value == 7   # a refused call writes nothing


def test_null_context_and_null_cache_are_refused_without_a_device():
    lib = ssa._lib
    buf = (C.c_uint8 * 256)()
    nf = C.c_uint64(7)
    stats = (C.c_uint64 * 12)(*([9] * 12))
    fake = (C.c_uint8 * 65536)()
    for flags in (0, 1, 8, 9):
        for fn in (_host, _devf):
            assert fn(lib, None, fake, buf, buf, None, buf, None, 1, 1, 1, flags, buf, None, stats) == ssa.ERR_ARG
            assert fn(lib, fake, None, buf, buf, None, buf, None, 1, 1, 1, flags, buf, None, stats) == ssa.ERR_ARG
            assert fn(lib, None, None, buf, buf, None, buf, None, 1, 1, 1, flags, buf, None, stats) == ssa.ERR_ARG
        assert lib.ssa_verify_many_cached(fake, None, buf, buf, None, buf, None, 1, 1, 1, flags, None, buf, C.byref(nf),
                                          stats) == ssa.ERR_ARG
    assert list(stats) == [9] * 12 and nf.value == 7
    out = (C.c_uint64 * 4)(*([5] * 4))
    assert lib.ssa_keycache_clear(None) == ssa.ERR_ARG
    assert lib.ssa_keycache_info(None, out) == ssa.ERR_ARG
    assert list(out) == [5] * 4


def test_create_refuses_bad_capacities_and_destroy_takes_null():
    lib = ssa._lib
    fake = (C.c_uint8 * 65536)()
    for ctx, cap in ((None, 16), (fake, 0), (fake, MAX_CAPACITY + 1), (fake, 1 << 40), (None, 0)):
        h = C.c_void_p(0x1234)
        assert lib.ssa_keycache_create(ctx, cap, C.byref(h)) == ssa.ERR_ARG, (ctx is None, cap)
        assert not h.value, "a refused create leaves *out == NULL"
    assert lib.ssa_keycache_create(fake, 16, None) == ssa.ERR_ARG
    lib.ssa_keycache_destroy(None)                    # a no-op


def _plan(capacity, held, u, m):
    out = C.c_uint32(77)
    rc = ssa._lib.ssa_debug_keycache_plan(capacity, held, u, m, C.byref(out))
    return rc, out.value


def _plan_py(capacity, held, u, m):
    """the policy of the issue, restated"""
    if held + m <= capacity:
        return INSERT
    return CLEAR if u <= capacity else BYPASS


def test_plan_outcomes_and_boundaries():
    cap = 64
    assert _plan(cap, 10, 20, 20) == (0, INSERT)
    assert _plan(cap, 50, 50, 50) == (0, CLEAR)
    assert _plan(16, 0, 50, 50) == (0, BYPASS)
    # held + m == capacity / capacity + 1
    assert _plan(cap, 40, 30, 24) == (0, INSERT)
    assert _plan(cap, 40, 30, 25) == (0, CLEAR)
    # u == capacity / capacity + 1 (the cache is too full for the misses)
    assert _plan(cap, 64, 64, 1) == (0, CLEAR)
    assert _plan(cap, 64, 65, 1) == (0, BYPASS)
    assert _plan(cap, 0, 64, 64) == (0, INSERT)
    assert _plan(cap, 0, 65, 65) == (0, BYPASS)
    # m == 0: nothing to insert, whatever u is (a full cache and more keys than rows included)
    assert _plan(cap, 64, 64, 0) == (0, INSERT)
    assert _plan(cap, 64, 1000, 0) == (0, INSERT)
    assert _plan(cap, 0, 1, 0) == (0, INSERT)
    assert _plan(1, 1, 1, 1) == (0, CLEAR)
    assert _plan(MAX_CAPACITY, MAX_CAPACITY, 1 << 20, 1) == (0, CLEAR)
    assert ssa.keycache_plan(cap, 50, 50, 50) == CLEAR
    # arguments
    assert _plan(0, 0, 1, 1)[0] == ssa.ERR_ARG
    assert _plan(MAX_CAPACITY + 1, 0, 1, 1)[0] == ssa.ERR_ARG
    assert _plan(cap, 65, 1, 1)[0] == ssa.ERR_ARG           # held > capacity
    assert _plan(cap, 0, 5, 6)[0] == ssa.ERR_ARG            # m > u
    assert _plan(cap, 0, (1 << 30) + 1, 0)[0] == ssa.ERR_ARG
    assert ssa._lib.ssa_debug_keycache_plan(cap, 0, 1, 1, None) == ssa.ERR_ARG
    assert _plan(cap, 65, 1, 1)[1] == 77                    # a refused call writes nothing


def test_plan_matches_the_restatement_on_random_cases():
    rng = np.random.default_rng(16001)
    seen = set()
    for _ in range(20000):
        cap = int(rng.integers(1, 1 << int(rng.integers(1, 25))))
        cap = min(cap, MAX_CAPACITY)
        held = int(rng.integers(0, cap + 1))
        u = int(rng.integers(1, 2 * cap + 2))
        m = int(rng.integers(0, u + 1))
        rc, got = _plan(cap, held, u, m)
        assert rc == 0 and got == _plan_py(cap, held, u, m), (cap, held, u, m, got)
        seen.add(got)
    assert seen == {INSERT, CLEAR, BYPASS}


def test_module_level_call_checks_lengths_without_a_device():
    with pytest.raises(ssa.MalformedInput):
        ssa.verify_many_cached([ssa.Signature(bytes(81))], [], [b""], None)
    with pytest.raises(ssa.MalformedInput):
        ssa.verify_many_cached([], [], [b""], None)
    assert ssa.verify_many_cached([], [], [], None) == []


def test_cxx_mirror_declares_keycache_and_verify_many_cached_statuses(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    src = tmp_path / "t.cpp"
    src.write_text('#include "%s/schnorr-sig_amd/host/schnorr_sig.hpp"\n'
                   "using namespace schnorr_sig;\n"
                   "std::vector<uint8_t> f(Context &cx, const std::vector<Signature> &s, const std::vector<PublicKey> &p,\n"
                   "                       const std::vector<std::pair<const uint8_t *, size_t>> &m, Rng rng, uint64_t *stats) {\n"
                   "  KeyCache cache(cx, 1024);\n"
                   "  cache.clear();\n"
                   "  KeyCache::Info i = cache.info();\n"
                   "  (void)i.capacity; (void)i.held; (void)i.clears; (void)i.device_bytes;\n"
                   "  return verify_many_cached_statuses(cx, cache, s, p, m, rng, stats);\n"
                   "}\n" % ROOT)
    subprocess.check_call([cxx, "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", str(src)])


def _function_body(text, signature):
    """the text of the function whose definition starts with `signature`, braces balanced"""
    a = text.index(signature)
    i = text.index("{", text.index(")", a))
    depth, j = 0, i
    while True:
        depth += {"{": 1, "}": -1}.get(text[j], 0)
        j += 1
        if depth == 0:
            return text[a:j]


def test_the_host_form_stays_on_the_context_and_its_stream():
    """Two streams would mutate one cache: with a cache the host form runs its slices in order on the context, and no
    function on that path asks for the context's second set of streams (directly, or through the helpers that alternate
    slices).  The one place that chooses between the two ways to run the slices sends a cache to the in-order loop."""
    msm = open(os.path.join(CSRC, "ssa_msm.hip")).read()
    ctx_hpp = open(os.path.join(CSRC, "ssa_ctx.hpp")).read()
    names = ("ssa_internal_twin", "run_host_slices", "std::thread", "->twin")
    entry = _function_body(msm, 'extern "C" int ssa_verify_many_cached(')
    assert "many_screened_host(ctx, kc," in entry
    # every function the cached host form runs through, the shared one-slice shell included
    for text, signature in ((msm, 'extern "C" int ssa_verify_many_cached('), (msm, "static int host_slices_in_order("),
                            (msm, "static int screen_many_host_one("), (ctx_hpp, "static int status_host_one(")):
        body = _function_body(text, signature)
        for name in names:
            assert name not in body, (signature, name)
    assert "screen_many_host_one(c," in _function_body(msm, "static int many_screened_host(")
    assert "status_host_one(ctx," in _function_body(msm, "static int screen_many_host_one(")
    # the choice: the alternating helper is named once, in the arm WITHOUT a cache, and nothing else of the second set of
    # streams is; the in-order loop and the alternating helper are two functions
    choice = _function_body(msm, "static int many_screened_host(")
    assert re.search(r"=\s*kc\s*\?\s*host_slices_in_order\(ctx,[^;?:]*\)\s*:\s*run_host_slices_counted\(ctx,[^;?:]*\);", choice)
    assert choice.count("run_host_slices") == 1 and choice.count("host_slices_in_order(") == 1
    for name in ("ssa_internal_twin", "std::thread", "->twin"):
        assert name not in choice, name
    assert msm.count("static int host_slices_in_order(") == 1
    # the slice function is shared with ssa_verify_many_screened, not copied, and the device path with a cache reaches it
    assert msm.count("static int screen_many_slice(") == 1
    dev = _function_body(msm, 'extern "C" int ssa_verify_many_cached_device(')
    assert "many_screened_device(ctx, kc," in dev
    assert re.search(r"screen_many_slice\(ctx,[^;]*\bkc\)", _function_body(msm, "static int many_screened_device("))


def _asm():
    """gfx950 assembly of the translation unit that holds the new kernels (cached by the content of its sources)"""
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not available")
    deps = [os.path.join(CSRC, f) for f in sorted(os.listdir(CSRC)) if f.endswith((".hip", ".hpp", ".inc"))]
    deps.append(os.path.join(ROOT, "include", "schnorr_sig_amd.h"))
    h = hashlib.sha256()
    for p in deps:
        h.update(os.path.basename(p).encode() + b"\0" + open(p, "rb").read() + b"\0")
    os.makedirs(CACHE, exist_ok=True)
    out, stamp = os.path.join(CACHE, "ssa_api.s"), os.path.join(CACHE, "ssa_api.s.srchash")
    if not (os.path.exists(out) and os.path.exists(stamp) and open(stamp).read().strip() == h.hexdigest()):
        subprocess.check_call(["hipcc", "-O3", "--offload-arch=gfx950", "-std=c++17", "--cuda-device-only", "-S", "-o", out,
                               os.path.join(CSRC, "ssa_api.hip")], stderr=subprocess.DEVNULL)
        open(stamp, "w").write(h.hexdigest() + "\n")
    return open(out).read()


def _kernel_bodies(text):
    out = {}
    for ch in re.split(r"^(?=_ZN3ssa\w+:)", text, flags=re.M):
        m = re.match(r"_ZN3ssa(\d+)(\w+):", ch)
        if m:
            out[m.group(2)[:int(m.group(1))]] = ch.split(".Lfunc_end")[0]
    return out


def test_keycache_kernels_use_vector_memory_instructions_only():
    """The static check of tests/test_dedup_host.py on the cache's kernels and on the whole translation unit: no scalar
    store, no scalar atomic, no scalar cache write-back or discard.  (The mnemonics are put together from parts.)"""
    s = "s_"
    forbidden = [s + stem + r"\w*" for stem in ("store_", "buffer_" + "store_", "scratch_" + "store_", "atomic_",
                                                "buffer_" + "atomic_", "dcache_" + "wb", "dcache_" + "discard")]
    pat = re.compile(r"^\s*(" + "|".join(forbidden) + r")\b", re.M)
    text = _asm()
    bodies = _kernel_bodies(text)
    for k in NEW_KERNELS + ["dd_k_scan", "dd_k_gather", "ssa_k_keyset_build"]:
        assert k in bodies, "kernel %s is not in the code object" % k
        body = bodies[k]
        assert len(body.splitlines()) > 10, k
        assert not pat.search(body), (k, pat.search(body).group(0))
    # a slot is claimed by a vector compare-and-swap on 64 bits, and only the publishing kernel writes slots
    assert re.search(r"^\s*global_atomic_cmpswap_x2\b", bodies["kc_k_publish"], re.M)
    for k in ("kc_k_lookup", "kc_k_number", "kc_k_map"):
        assert not re.search(r"^\s*global_atomic_cmpswap", bodies[k], re.M), k
    assert not pat.search(text), pat.search(text).group(0)
    # the sources do not spell those mnemonics either, comments included
    src_pat = re.compile("|".join(f[:-3] for f in forbidden), re.I)
    for f in ("ssa_keycache.hpp", "ssa_api.hip", "ssa_msm.hip", "ssa_ctx.hpp"):
        assert not src_pat.search(open(os.path.join(CSRC, f)).read()), f
