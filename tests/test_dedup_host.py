"""Key dedup (ssa_verify_many_dedup), host side (no GPU): the C ABI, the argument checks, the C++
mirror, and a static check of the new kernels' instructions."""
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
CACHE = os.path.join(ROOT, "build", "dedup_static")
NEW_SYMBOLS = ["ssa_verify_many_dedup", "ssa_verify_many_dedup_device", "ssa_debug_dedup_device", "ssa_debug_dedup_config"]
NEW_KERNELS = ["dd_k_insert", "dd_k_scan", "dd_k_number", "dd_k_index", "dd_k_gather"]


def test_new_symbols_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "schnorr_sig_amd.h")).read()
    lib = C.CDLL(ssa.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name + "(" in hdr, name
        assert hasattr(lib, name), name
        assert name in ssa.ABI_SYMBOLS, name
    assert ssa._lib.ssa_abi_version() == 5           # additive: the ABI version does not move
    for name in ("verify_many_dedup", "verify_many_dedup_device", "debug_dedup_device", "debug_dedup_config"):
        assert hasattr(ssa.Engine, name), name
    assert callable(ssa.verify_many)


def test_null_and_size_arguments_are_refused_without_a_device():
    lib = ssa._lib
    buf = (C.c_uint8 * 256)()
    nf = C.c_uint64(7)
    stats = (C.c_uint64 * 4)()
    out = (C.c_uint64 * 2)()
    # a null context
    assert lib.ssa_verify_many_dedup(None, buf, buf, None, buf, None, 1, 1, 1, 0, buf, C.byref(nf), stats) == ssa.ERR_ARG
    assert lib.ssa_verify_many_dedup_device(None, buf, buf, None, buf, None, 1, 1, 1, 0, buf, None, stats) == ssa.ERR_ARG
    assert lib.ssa_debug_dedup_device(None, buf, None, 1, None, out) == ssa.ERR_ARG
    assert lib.ssa_debug_dedup_config(None, 0.5, 0) == ssa.ERR_ARG
    # null buffers and oversized batches are refused before the context is looked at: any non-null pointer will do
    fake = (C.c_uint8 * 65536)()
    for fn in (lib.ssa_verify_many_dedup, lib.ssa_verify_many_dedup_device):
        assert fn(fake, None, buf, None, buf, None, 1, 1, 1, 0, buf, None, stats) == ssa.ERR_ARG
        assert fn(fake, buf, None, None, buf, None, 1, 1, 1, 0, buf, None, stats) == ssa.ERR_ARG
        assert fn(fake, buf, buf, None, buf, None, 1, 1, 1, 0, None, None, stats) == ssa.ERR_ARG
        assert fn(fake, buf, buf, None, None, None, 1, 1, 1, 0, buf, None, stats) == ssa.ERR_ARG      # messages missing
        assert fn(fake, buf, buf, None, buf, None, 1, 1, (1 << 30) + 1, 0, buf, None, stats) == ssa.ERR_ARG
    assert lib.ssa_debug_dedup_device(fake, None, None, 1, None, out) == ssa.ERR_ARG
    assert lib.ssa_debug_dedup_device(fake, buf, None, 1, None, None) == ssa.ERR_ARG
    assert lib.ssa_debug_dedup_device(fake, buf, None, 0, None, out) == ssa.ERR_ARG
    assert lib.ssa_debug_dedup_device(fake, buf, None, (1 << 30) + 1, None, out) == ssa.ERR_ARG


def test_module_level_verify_many_checks_lengths_without_a_device():
    with pytest.raises(ssa.MalformedInput):
        ssa.verify_many([ssa.Signature(bytes(81))], [], [b""])
    with pytest.raises(ssa.MalformedInput):
        ssa.verify_many([], [], [b""])
    assert ssa.verify_many([], [], []) == []


def test_cxx_mirror_declares_verify_many_statuses(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    src = tmp_path / "t.cpp"
    src.write_text('#include "%s/schnorr-sig_amd/host/schnorr_sig.hpp"\n'
                   "using namespace schnorr_sig;\n"
                   "std::vector<uint8_t> f(Context &cx, const std::vector<Signature> &s, const std::vector<PublicKey> &p,\n"
                   "                       const std::vector<std::pair<const uint8_t *, size_t>> &m, uint64_t *stats) {\n"
                   "  return verify_many_statuses(cx, s, p, m, stats);\n"
                   "}\n" % ROOT)
    subprocess.check_call([cxx, "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", str(src)])


def _asm():
    """gfx950 assembly of the translation unit that holds the dedup kernels (cached by the content of its sources)"""
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


def test_dedup_kernels_use_vector_memory_instructions_only():
    """No scalar store, no scalar atomic, no scalar cache write-back or discard: the slot table is written by vector
    compare-and-swap, everything else by vector stores.  (The mnemonics are put together from parts.)"""
    s = "s_"
    forbidden = [s + stem + r"\w*" for stem in ("store_", "buffer_" + "store_", "scratch_" + "store_", "atomic_",
                                                "buffer_" + "atomic_", "dcache_" + "wb", "dcache_" + "discard")]
    pat = re.compile(r"^\s*(" + "|".join(forbidden) + r")\b", re.M)
    text = _asm()
    bodies = _kernel_bodies(text)
    for k in NEW_KERNELS:
        assert k in bodies, "kernel %s is not in the code object" % k
        body = bodies[k]
        assert len(body.splitlines()) > 10, k
        assert not pat.search(body), (k, pat.search(body).group(0))
    # the claim of a slot is a vector compare-and-swap on 64 bits; the slot is looked at with a vector load first
    ins = bodies["dd_k_insert"]
    assert re.search(r"^\s*global_atomic_cmpswap_x2\b", ins, re.M)
    # and nowhere else in the translation unit either
    assert not pat.search(text), pat.search(text).group(0)
