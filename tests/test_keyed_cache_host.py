"""KeyedSignature wire records through a key cache in wire mode (ssa_keycache_create_ex, ssa_verify_keyed_many_cached,
ssa_verify_keyed_many_device), host side (no GPU): the C ABI, the argument checks that need no
device, the mirrors, and the shape of the host form's source."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

import schnorr_sig_amd as ssa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "schnorr-sig_amd", "csrc")
NEW_SYMBOLS = ["ssa_keycache_create_ex", "ssa_verify_keyed_many_cached", "ssa_verify_keyed_many_cached_device",
               "ssa_verify_keyed_many_device"]
MAX_BATCH = 1 << 30
MAX_CAPACITY = 1 << 24


def test_new_symbols_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "schnorr_sig_amd.h")).read()
    lib = C.CDLL(ssa.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name + "(" in hdr, name
        assert hasattr(lib, name), name
        assert name in ssa.ABI_SYMBOLS, name
    assert re.search(r"#define\s+SSA_KEYCACHE_WIRE\s+1u", hdr) and ssa.KEYCACHE_WIRE == 1
    assert ssa._lib.ssa_abi_version() == 5           # additive: the ABI version does not move
    for name in ("keycache_create", "verify_keyed_many_cached", "verify_keyed_many_cached_device",
                 "verify_keyed_many_device"):
        assert hasattr(ssa.Engine, name), name
    assert callable(ssa.verify_keyed_many_cached)
    assert ssa.KEYTAB_WIRE == 5
    import inspect
    assert "wire" in inspect.signature(ssa.Engine.keycache_create).parameters
    assert inspect.signature(ssa.Engine.keycache_create).parameters["wire"].default is False
    kc = ssa.KeyCache(None, C.c_void_p(), wire=True)
    assert kc.wire is True and ssa.KeyCache(None, C.c_void_p()).wire is False


def _host(lib, ctx, kc, n, flags, buf, nf, stats):
    return lib.ssa_verify_keyed_many_cached(ctx, kc, buf, buf, None, 1, 1, n, flags, None, buf, nf, stats)


def _devf(lib, ctx, kc, n, flags, buf, nf, stats):
    return lib.ssa_verify_keyed_many_cached_device(ctx, kc, buf, buf, None, 1, 1, n, flags, None, 0, buf, None, stats)


def test_flag_bits_outside_the_two_are_refused_before_anything_else():
    lib = ssa._lib
    buf = (C.c_uint8 * 256)()
    nf = C.c_uint64(7)
    stats = (C.c_uint64 * 12)(*([9] * 12))
    fake = (C.c_uint8 * 65536)()                      # never dereferenced: the flags are looked at first
    for bad in (2, 4, 16, 32, 64, 1 | 2, 8 | 4, 1 << 31):
        for fn in (_host, _devf):
            assert fn(lib, fake, fake, 1, bad, buf, C.byref(nf), stats) == ssa.ERR_ARG, bad
            # ... even with no context and no cache at all
            assert fn(lib, None, None, 1, bad, buf, C.byref(nf), stats) == ssa.ERR_ARG, bad
    assert list(stats) == [9] * 12 and nf.value == 7   # a refused call writes nothing


def test_null_context_null_cache_and_oversized_batches_are_refused_without_a_device():
    lib = ssa._lib
    buf = (C.c_uint8 * 256)()
    nf = C.c_uint64(7)
    stats = (C.c_uint64 * 12)(*([9] * 12))
    fake = (C.c_uint8 * 65536)()
    for flags in (0, 1, 8, 9):
        for fn in (_host, _devf):
            assert fn(lib, None, fake, 1, flags, buf, C.byref(nf), stats) == ssa.ERR_ARG
            assert fn(lib, fake, None, 1, flags, buf, C.byref(nf), stats) == ssa.ERR_ARG
            assert fn(lib, None, None, 1, flags, buf, C.byref(nf), stats) == ssa.ERR_ARG
            # n > SSA_MAX_BATCH is refused before the context or the cache is looked into
            assert fn(lib, fake, fake, MAX_BATCH + 1, flags, buf, C.byref(nf), stats) == ssa.ERR_ARG
        # null records or a null status array with n > 0
        assert lib.ssa_verify_keyed_many_cached(fake, fake, None, buf, None, 1, 1, 1, flags, None, buf, C.byref(nf),
                                                stats) == ssa.ERR_ARG
        assert lib.ssa_verify_keyed_many_cached(fake, fake, buf, buf, None, 1, 1, 1, flags, None, None, C.byref(nf),
                                                stats) == ssa.ERR_ARG
        # the device form of the exact call
        assert lib.ssa_verify_keyed_many_device(None, buf, buf, None, 1, 1, 1, flags & 1, buf, None) == ssa.ERR_ARG
        assert lib.ssa_verify_keyed_many_device(fake, None, buf, None, 1, 1, 1, flags & 1, buf, None) == ssa.ERR_ARG
        assert lib.ssa_verify_keyed_many_device(fake, buf, buf, None, 1, 1, 1, flags & 1, None, None) == ssa.ERR_ARG
        assert lib.ssa_verify_keyed_many_device(fake, buf, buf, None, 1, 1, MAX_BATCH + 1, flags & 1, buf,
                                                None) == ssa.ERR_ARG
    assert list(stats) == [9] * 12 and nf.value == 7


def test_create_ex_refuses_unknown_flags_before_anything_else_and_bad_capacities():
    lib = ssa._lib
    fake = (C.c_uint8 * 65536)()
    for flags in (2, 4, 3, 1 << 31, 0xFFFFFFFE):
        for ctx, cap in ((fake, 16), (None, 16), (fake, 0), (None, 0)):
            h = C.c_void_p(0x1234)
            assert lib.ssa_keycache_create_ex(ctx, cap, flags, C.byref(h)) == ssa.ERR_ARG, (flags, cap)
            assert not h.value, "a refused create leaves *out == NULL"
        assert lib.ssa_keycache_create_ex(None, 16, flags, None) == ssa.ERR_ARG
    for flags in (0, ssa.KEYCACHE_WIRE):
        for ctx, cap in ((None, 16), (fake, 0), (fake, MAX_CAPACITY + 1), (fake, 1 << 40)):
            h = C.c_void_p(0x1234)
            assert lib.ssa_keycache_create_ex(ctx, cap, flags, C.byref(h)) == ssa.ERR_ARG, (flags, cap)
            assert not h.value
        assert lib.ssa_keycache_create_ex(fake, 16, flags, None) == ssa.ERR_ARG


def test_cxx_mirror_declares_the_wire_cache_and_its_calls(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    src = tmp_path / "t.cpp"
    src.write_text('#include "%s/schnorr-sig_amd/host/schnorr_sig.hpp"\n'
                   "using namespace schnorr_sig;\n"
                   "std::vector<uint8_t> f(Context &cx, const std::vector<uint8_t> &keyed130,\n"
                   "                       const std::vector<std::pair<const uint8_t *, size_t>> &m, Rng rng, uint64_t *stats) {\n"
                   "  KeyCache cache(cx, 1024, KeyCache::Wire);\n"
                   "  bool w = cache.wire();\n"
                   "  (void)w;\n"
                   "  KeyCache::Info i = cache.info();\n"
                   "  (void)i.device_bytes;\n"
                   "  return verify_keyed_many_cached_statuses(cx, cache, keyed130, m, rng, stats);\n"
                   "}\n"
                   "int g(Context &cx, KeyCache &cache, const uint8_t *d_keyed, const uint8_t *d_msgs, size_t n, uint8_t *d_st,\n"
                   "      uint64_t *stats) {\n"
                   "  int a = verify_keyed_many_cached_device(cx, cache, d_keyed, d_msgs, 80, n, SSA_FLAG_CHECK_TORSION, nullptr, 32,\n"
                   "                                          d_st, nullptr, stats);\n"
                   "  int b = verify_keyed_many_device(cx, d_keyed, d_msgs, 80, n, SSA_FLAG_CHECK_TORSION, d_st, nullptr);\n"
                   "  return a | b;\n"
                   "}\n" % ROOT)
    subprocess.check_call([cxx, "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", str(src)])


def test_module_level_call_checks_lengths_without_a_device():
    k = ssa.KeyedSignature(ssa.PublicKey(bytes(96)), ssa.Signature(bytes(81)))
    with pytest.raises(ssa.MalformedInput):
        ssa.verify_keyed_many_cached([k], [], None)
    with pytest.raises(ssa.MalformedInput):
        ssa.verify_keyed_many_cached([], [b""], None)
    with pytest.raises(ssa.MalformedInput):
        ssa.verify_keyed_many_cached([k, k], [b"", b"", b""], None)
    assert ssa.verify_keyed_many_cached([], [], None) == []


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
    """Every slice reads and may extend the one cache: the host form of the wire call runs its slices in order on the
    context, and no function on that path asks for the context's second set of streams or for the pipelined
    upload-and-hash (the hash needs y, which exists only after the look-up).  The records have a staging buffer of their
    own, and the slice behind the keys is the shared one, not a copy."""
    msm = open(os.path.join(CSRC, "ssa_msm.hip")).read()
    api = open(os.path.join(CSRC, "ssa_api.hip")).read()
    ctx_hpp = open(os.path.join(CSRC, "ssa_ctx.hpp")).read()
    names = ("ssa_internal_twin", "run_host_slices", "std::thread", "->twin", "pipelined_upload_hash", "slice_inputs(",
             "status_host_one(", "copy_stream", "hash_stream")
    entry = _function_body(msm, 'extern "C" int ssa_verify_keyed_many_cached(')
    assert "host_slices_in_order(ctx," in entry and "keyed_host_one(c," in entry
    for text, signature in ((msm, 'extern "C" int ssa_verify_keyed_many_cached('), (msm, "static int keyed_host_one("),
                            (msm, "static int keyed_cached_slice("), (msm, "static int keyed_exact_slice("),
                            (msm, "static int keyed_batch_screened_device("), (msm, "static int host_slices_in_order("),
                            (api, "int ssa_internal_keyed_cache_slice("), (api, "static int keycache_slice("),
                            (api, "int ssa_internal_unpack_keyed(")):
        body = _function_body(text, signature)
        for name in names:
            assert name not in body, (signature, name)
    one = _function_body(msm, "static int keyed_host_one(")
    assert "hc.in(ctx->st_keyed, keyed, n * 130)" in one and "hc.in(ctx->st_coeffs, coeffs, n * 32)" in one
    assert re.search(r"X\(st_keyed\)", ctx_hpp)
    # the exact host call stages its records there too: st_coeffs holds coefficients only
    assert "hc.in(ctx->st_keyed, keyed, n * 130)" in _function_body(api, "static int verify_keyed_host_one(")
    # the slice: the wire look-up, then the code every screened form shares, with no challenge scalars handed in
    sl = _function_body(msm, "static int keyed_cached_slice(")
    assert "ssa_internal_keyed_cache_slice(ctx, kc, d_keyed," in sl
    assert re.search(r"screen_slice_after_keys\(ctx, b, n, d_coeffs, coeff_bytes, flags, nullptr,", sl)
    assert msm.count("static int screen_slice_after_keys(") == 2          # a declaration and the one definition
    assert "screen_slice_after_keys(ctx, b, n," in _function_body(msm, "static int screen_many_slice(")
    # ... whose keys go through the one slice function of both kinds of cache
    assert "keycache_slice(ctx, kc," in _function_body(api, "int ssa_internal_keyed_cache_slice(")
    dev = _function_body(msm, 'extern "C" int ssa_verify_keyed_many_cached_device(')
    assert "keyed_cached_slice(ctx, kc," in dev and "run_host_slices" not in dev
    # both directions of the mode check
    assert "!kc->wire_mode" in entry and "!kc->wire_mode" in dev
    for sig in ("static int many_screened_device(", "static int many_screened_host("):
        assert "kc->wire_mode" in _function_body(msm, sig), sig
