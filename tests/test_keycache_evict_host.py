"""Key cache eviction (ssa_keycache_set_eviction), host side (no GPU): the C ABI, the mirrors, the
argument checks that need no device, and the keep rule ssa_debug_keycache_keep against a restatement in Python -- on the
cases worked out by hand in the issue and on random histograms, with the invariants the design states."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import schnorr_sig_amd as ssa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["ssa_keycache_set_eviction", "ssa_keycache_eviction_info", "ssa_debug_keycache_keep"]
MAX_CAPACITY = 1 << 24
CLEAR, RECENT = 0, 1


def test_new_symbols_are_declared_exported_and_mirrored():
    hdr = open(os.path.join(ROOT, "include", "schnorr_sig_amd.h")).read()
    lib = C.CDLL(ssa.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name + "(" in hdr, name
        assert hasattr(lib, name), name
        assert name in ssa.ABI_SYMBOLS, name
    assert "#define SSA_KEYCACHE_EVICT_CLEAR  0u" in hdr and "#define SSA_KEYCACHE_EVICT_RECENT 1u" in hdr
    assert ssa._lib.ssa_abi_version() == 5           # additive: the ABI version does not move
    assert ssa.KEYCACHE_EVICT == {"clear": CLEAR, "recent": RECENT}
    for name in ("set_eviction", "eviction_info"):
        assert hasattr(ssa.KeyCache, name), name
    import inspect
    assert inspect.signature(ssa.Engine.keycache_create).parameters["evict"].default == "clear"
    assert callable(ssa.keycache_keep)


def test_null_cache_and_unknown_policy_are_refused_without_a_device():
    lib = ssa._lib
    out = (C.c_uint64 * 8)(*([5] * 8))
    for policy in (CLEAR, RECENT, 2, 7, 1 << 31):
        assert lib.ssa_keycache_set_eviction(None, policy) == ssa.ERR_ARG
    assert lib.ssa_keycache_eviction_info(None, out) == ssa.ERR_ARG
    assert list(out) == [5] * 8                       # a refused call writes nothing
    with pytest.raises(ValueError):
        ssa.KeyCache(None, C.c_void_p()).set_eviction("lru")


def _keep(capacity, u, m, hist):
    h = (C.c_uint64 * 64)(*[int(v) for v in hist])
    out = (C.c_uint64 * 2)(77, 77)
    rc = ssa._lib.ssa_debug_keycache_keep(capacity, u, m, h, out)
    return rc, (int(out[0]), int(out[1]))


def _keep_py(capacity, u, m, hist):
    """the keep rule of the issue, restated: -> (a*, K), or None when no a* exists"""
    budget = max(u - m, (capacity - m) // 2)
    best = None
    for a in range(63):
        k = sum(int(v) for v in hist[:a + 1])
        if k <= budget:
            best = (a, k)
    return best


def _hist(d):
    h = [0] * 64
    for a, v in d.items():
        h[a] = v
    return h


def test_the_hand_cases_of_the_issue():
    # capacity 64; A (30 keys), B (20 others), then B + 20 new: budget 22, only B's rows fit
    assert _keep(64, 40, 20, _hist({0: 20, 2: 30})) == (0, (1, 20))
    # ... B again, then A again (30 misses): budget 17, nothing fits
    assert _keep(64, 30, 30, _hist({1: 20, 2: 20})) == (0, (0, 0))
    # A (30), B (30 others), A + 10 new: budget 30
    assert _keep(64, 40, 10, _hist({0: 30, 1: 30})) == (0, (0, 30))
    # the flood: 30 validators hit, 30 of the last call's fresh keys: budget 30
    assert _keep(64, 60, 30, _hist({0: 30, 1: 30})) == (0, (0, 30))
    # capacity 1024: 900 keys, then every third of them and 200 new ones: budget 412
    assert _keep(1024, 500, 200, _hist({0: 300, 1: 600})) == (0, (0, 300))
    # rows older than 62 slices are never kept, however much room there is
    assert _keep(1024, 10, 5, _hist({0: 5, 62: 7, 63: 100})) == (0, (62, 12))
    assert _keep(1024, 10, 5, _hist({0: 5, 63: 100})) == (0, (62, 5))
    # the sum may equal the budget; one more row and the age is out
    assert _keep(100, 20, 10, _hist({0: 10, 1: 35, 2: 1})) == (0, (1, 45))
    assert _keep(100, 20, 10, _hist({0: 10, 1: 36, 2: 1})) == (0, (0, 10))
    # empty ages beyond the last one that fits change nothing but a*: the largest such age is reported
    assert _keep(100, 20, 10, _hist({0: 10, 1: 35})) == (0, (62, 45))
    # u - m above half of the room: the slice's own hits always stay
    assert _keep(64, 64, 4, _hist({0: 60, 1: 4})) == (0, (0, 60))
    assert ssa.keycache_keep(64, 40, 20, _hist({0: 20, 2: 30})) == (1, 20)


def test_keep_refuses_bad_arguments_and_writes_nothing():
    h = _hist({0: 1})
    for cap, u, m in ((0, 1, 1), (MAX_CAPACITY + 1, 1, 1), (64, 5, 6), (64, 65, 1)):
        rc, out = _keep(cap, u, m, h)
        assert rc == ssa.ERR_ARG and out == (77, 77), (cap, u, m)
    assert _keep(64, 10, 5, _hist({0: 5, 3: 60}))[0] == ssa.ERR_ARG          # 65 rows in a cache of 64
    assert _keep(64, 10, 5, _hist({0: 30}))[0] == ssa.ERR_ARG                # 30 rows of age 0, budget 29: no a*
    assert _keep(64, 10, 5, _hist({0: 29}))[0] == 0
    out = (C.c_uint64 * 2)()
    assert ssa._lib.ssa_debug_keycache_keep(64, 10, 5, None, out) == ssa.ERR_ARG
    assert ssa._lib.ssa_debug_keycache_keep(64, 10, 5, (C.c_uint64 * 64)(), None) == ssa.ERR_ARG


def test_keep_matches_the_restatement_and_keeps_its_promises_on_random_histograms():
    """What a compaction meets: held + m > capacity (the plan), u <= capacity, hist[0] = u - m (the rows this slice hit),
    the other held rows spread over the ages.  a* exists; K + m <= capacity; K < held; at most max(u - m, half of the room
    beside the misses) is kept, so the next compaction is at least (capacity - m) / 2 insertions away unless the slice's
    own hits alone take more."""
    rng = np.random.default_rng(19001)
    ages_seen = set()
    for _ in range(20000):
        cap = min(int(rng.integers(1, 1 << int(rng.integers(1, 25)))), MAX_CAPACITY)
        held = int(rng.integers(1, cap + 1))
        m = int(rng.integers(cap - held + 1, cap + 1))           # held + m > capacity, m <= capacity
        hits = int(rng.integers(0, min(held, cap - m) + 1))       # u = hits + m <= capacity
        u = hits + m
        hist = [0] * 64
        hist[0] = hits
        rest = held - hits
        k = int(rng.integers(1, 8))
        ages = rng.integers(1, 64, size=k) if rng.integers(0, 2) else rng.integers(1, 5, size=k)
        cuts = np.sort(rng.integers(0, rest + 1, size=k - 1)) if k > 1 else np.zeros(0, dtype=np.int64)
        parts = np.diff(np.concatenate([[0], cuts, [rest]]))
        for a, v in zip(ages, parts):
            hist[int(a)] += int(v)
        assert sum(hist) == held
        assert ssa.keycache_plan(cap, held, u, m) == 1            # where the default policy clears
        rc, (a_star, kept) = _keep(cap, u, m, hist)
        want = _keep_py(cap, u, m, hist)
        assert rc == 0 and want is not None and (a_star, kept) == want, (cap, held, u, m, hist, a_star, kept, want)
        assert 0 <= a_star <= 62 and kept == sum(hist[:a_star + 1])
        assert kept >= hits                                       # the rows this slice hit always survive
        assert kept + m <= cap
        assert kept < held                                        # every compaction drops at least one row
        assert kept <= max(hits, (cap - m) // 2)
        if a_star < 62:
            assert kept + hist[a_star + 1] > max(hits, (cap - m) // 2)      # the next age does not fit
        ages_seen.add(a_star)
    assert {0, 1, 62} <= ages_seen


def test_the_plan_is_untouched():
    for args, want in (((64, 10, 20, 20), 0), ((64, 50, 50, 50), 1), ((16, 0, 50, 50), 2), ((64, 40, 30, 24), 0),
                       ((64, 40, 30, 25), 1), ((64, 64, 65, 1), 2), ((64, 64, 1000, 0), 0)):
        assert ssa.keycache_plan(*args) == want, args


def test_cxx_mirror_declares_the_eviction_methods(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    src = tmp_path / "t.cpp"
    src.write_text('#include "%s/schnorr-sig_amd/host/schnorr_sig.hpp"\n'
                   "using namespace schnorr_sig;\n"
                   "uint64_t f(Context &cx) {\n"
                   "  KeyCache cache(cx, 1024), wire(cx, 1024, KeyCache::Wire);\n"
                   "  cache.set_eviction(KeyCache::Recent);\n"
                   "  wire.set_eviction(KeyCache::Recent);\n"
                   "  cache.set_eviction(KeyCache::Clear);\n"
                   "  KeyCache::EvictionInfo i = cache.eviction_info();\n"
                   "  return i.policy + i.compactions + i.dropped + i.last_kept + i.last_moved + i.epoch;\n"
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


def test_one_function_handles_a_full_cache_for_both_kinds_of_cache():
    """the overflow handling is written once: ONE slice function serves both kinds of cache, it calls keycache_place
    once, only keycache_place clears or compacts, and the two entry points only hand their keys to the slice function"""
    api = open(os.path.join(ROOT, "schnorr-sig_amd", "csrc", "ssa_api.hip")).read()
    assert api.count("static int keycache_place(") == 1 and api.count("static int keycache_compact(") == 1
    assert api.count("static int keycache_slice(") == 1
    assert api.count("keycache_place(ctx, kc, plan,") == 1
    shared = _function_body(api, "static int keycache_slice(")
    wrappers = [_function_body(api, "int ssa_internal_keycache_slice("),
                _function_body(api, "int ssa_internal_keyed_cache_slice(")]
    assert shared.count("keycache_place(ctx, kc, plan,") == 1
    for body in [shared] + wrappers:
        assert "keycache_reset(" not in body and "keycache_compact(" not in body
    for body in wrappers:
        assert body.count("keycache_slice(ctx, kc,") == 1
        for name in ("keycache_place(", "hipLaunchKernelGGL", "dedup_slice("):
            assert name not in body, name
