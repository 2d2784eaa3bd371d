"""Screened Signature::verify (ssa_verify_many_screened), host side (no GPU): the C ABI, the
argument checks, the mirrors, and a static check of the new kernels' instructions."""
import ctypes as C
import hashlib
import os
import re
import shutil
import subprocess

import pytest

import schnorr_sig_amd as ssa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "schnorr-sig_amd", "csrc")
CACHE = os.path.join(ROOT, "build", "screened_torsion_static")
NEW_SYMBOLS = ["ssa_verify_many_screened", "ssa_verify_many_screened_device"]
NEW_KERNELS = ["msm_k_screen_keymask", "msm_k_screen_mark", "msm_k_screen_scan", "msm_k_screen_list",
               "msm_k_screen_gather_list", "msm_k_screen_scatter_list"]


def test_new_symbols_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "schnorr_sig_amd.h")).read()
    lib = C.CDLL(ssa.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name + "(" in hdr, name
        assert hasattr(lib, name), name
        assert name in ssa.ABI_SYMBOLS, name
    assert ssa._lib.ssa_abi_version() == 5           # additive: the ABI version does not move
    for name in ("verify_many_screened", "verify_many_screened_device"):
        assert hasattr(ssa.Engine, name), name
    assert callable(ssa.verify_many_screened)


def test_flag_bits_outside_the_two_are_refused_before_anything_else():
    lib = ssa._lib
    buf = (C.c_uint8 * 256)()
    nf = C.c_uint64(7)
    stats = (C.c_uint64 * 8)(*([9] * 8))
    fake = (C.c_uint8 * 65536)()                      # never dereferenced: the flags are looked at first
    for bad in (2, 4, 16, 32, 64, 1 | 2, 8 | 4, 1 << 31):
        assert lib.ssa_verify_many_screened(fake, buf, buf, None, buf, None, 1, 1, 1, bad, None, buf, C.byref(nf),
                                            stats) == ssa.ERR_ARG, bad
        assert lib.ssa_verify_many_screened_device(fake, buf, buf, None, buf, None, 1, 1, 1, bad, None, 0, buf, None,
                                                   stats) == ssa.ERR_ARG, bad
    assert list(stats) == [9] * 8 and nf.value == 7   # a refused call writes nothing


def test_null_and_size_arguments_are_refused_without_a_device():
    lib = ssa._lib
    buf = (C.c_uint8 * 256)()
    stats = (C.c_uint64 * 8)()
    fake = (C.c_uint8 * 65536)()
    for flags in (0, 1, 8, 9):
        assert lib.ssa_verify_many_screened(None, buf, buf, None, buf, None, 1, 1, 1, flags, None, buf, None, stats) == ssa.ERR_ARG
        assert lib.ssa_verify_many_screened_device(None, buf, buf, None, buf, None, 1, 1, 1, flags, None, 0, buf, None,
                                                   stats) == ssa.ERR_ARG
        host = lambda *a: lib.ssa_verify_many_screened(*a[:10], None, *a[10:])              # noqa: E731
        devf = lambda *a: lib.ssa_verify_many_screened_device(*a[:10], None, 0, *a[10:])    # noqa: E731
        for fn in (host, devf):
            assert fn(fake, None, buf, None, buf, None, 1, 1, 1, flags, buf, None, stats) == ssa.ERR_ARG
            assert fn(fake, buf, None, None, buf, None, 1, 1, 1, flags, buf, None, stats) == ssa.ERR_ARG
            assert fn(fake, buf, buf, None, buf, None, 1, 1, 1, flags, None, None, stats) == ssa.ERR_ARG
            assert fn(fake, buf, buf, None, None, None, 1, 1, 1, flags, buf, None, stats) == ssa.ERR_ARG   # messages missing
            assert fn(fake, buf, buf, None, buf, None, 1, 1, (1 << 30) + 1, flags, buf, None, stats) == ssa.ERR_ARG
        # device coefficients of a width outside 1..32
        for width in (0, 33):
            assert lib.ssa_verify_many_screened_device(fake, buf, buf, None, buf, None, 1, 1, 1, flags, buf, width, buf, None,
                                                       stats) == ssa.ERR_ARG


def test_module_level_call_checks_lengths_without_a_device():
    with pytest.raises(ssa.MalformedInput):
        ssa.verify_many_screened([ssa.Signature(bytes(81))], [], [b""])
    with pytest.raises(ssa.MalformedInput):
        ssa.verify_many_screened([], [], [b""])
    assert ssa.verify_many_screened([], [], []) == []


def test_cxx_mirror_declares_verify_many_screened_statuses(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    src = tmp_path / "t.cpp"
    src.write_text('#include "%s/schnorr-sig_amd/host/schnorr_sig.hpp"\n'
                   "using namespace schnorr_sig;\n"
                   "std::vector<uint8_t> f(Context &cx, const std::vector<Signature> &s, const std::vector<PublicKey> &p,\n"
                   "                       const std::vector<std::pair<const uint8_t *, size_t>> &m, Rng rng, uint64_t *stats) {\n"
                   "  return verify_many_screened_statuses(cx, s, p, m, rng, stats);\n"
                   "}\n" % ROOT)
    subprocess.check_call([cxx, "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", str(src)])


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
    out, stamp = os.path.join(CACHE, "ssa_msm.s"), os.path.join(CACHE, "ssa_msm.s.srchash")
    if not (os.path.exists(out) and os.path.exists(stamp) and open(stamp).read().strip() == h.hexdigest()):
        subprocess.check_call(["hipcc", "-O3", "--offload-arch=gfx950", "-std=c++17", "--cuda-device-only", "-S", "-o", out,
                               os.path.join(CSRC, "ssa_msm.hip")], stderr=subprocess.DEVNULL)
        open(stamp, "w").write(h.hexdigest() + "\n")
    return open(out).read()


def _kernel_bodies(text):
    out = {}
    for ch in re.split(r"^(?=_ZN3ssa\w+:)", text, flags=re.M):
        m = re.match(r"_ZN3ssa(\d+)(\w+):", ch)
        if m:
            out[m.group(2)[:int(m.group(1))]] = ch.split(".Lfunc_end")[0]
    return out


def test_new_kernels_use_vector_memory_instructions_only():
    """The static check of tests/test_dedup_host.py on the new kernels, on msm_k_prepare (which now writes the re-check
    marks) and on the whole translation unit: no scalar store, no scalar atomic, no scalar cache write-back or discard.
    (The mnemonics are put together from parts.)"""
    s = "s_"
    forbidden = [s + stem + r"\w*" for stem in ("store_", "buffer_" + "store_", "scratch_" + "store_", "atomic_",
                                                "buffer_" + "atomic_", "dcache_" + "wb", "dcache_" + "discard")]
    pat = re.compile(r"^\s*(" + "|".join(forbidden) + r")\b", re.M)
    text = _asm()
    bodies = _kernel_bodies(text)
    for k in NEW_KERNELS + ["msm_k_prepare"]:
        assert k in bodies, "kernel %s is not in the code object" % k
        body = bodies[k]
        assert len(body.splitlines()) > 10, k
        assert not pat.search(body), (k, pat.search(body).group(0))
    # the counters that workgroups of one launch share are vector atomics
    assert re.search(r"^\s*global_atomic_add_x2\b", bodies["msm_k_screen_mark"], re.M)
    assert not pat.search(text), pat.search(text).group(0)
