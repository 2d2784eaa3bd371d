"""Screened batch verification, host side (no GPU): the C ABI, argument checks and the segment plan
(ssa_debug_screen_plan)."""
import ctypes as C
import os
import subprocess
import shutil

import pytest

import schnorr_sig_amd as ssa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["ssa_verify_batch_screened", "ssa_verify_batch_screened_device", "ssa_debug_screen_plan",
               "ssa_debug_screen_segments"]
SLICE = 1 << 23          # the default SSA_MSM_SLICE


def test_new_symbols_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "schnorr_sig_amd.h")).read()
    lib = C.CDLL(ssa.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name + "(" in hdr, name
        assert hasattr(lib, name), name
        assert name in ssa.ABI_SYMBOLS, name
    assert ssa._lib.ssa_abi_version() == 5
    assert hasattr(ssa, "verify_batch_statuses") and hasattr(ssa.Engine, "verify_batch_screened")
    assert hasattr(ssa.Engine, "verify_batch_screened_device")


def test_null_and_size_arguments_are_refused_without_a_device():
    lib = ssa._lib
    buf = (C.c_uint8 * 256)()
    nf = C.c_uint64(7)
    assert lib.ssa_verify_batch_screened(None, buf, buf, None, buf, None, 1, 1, 1, None, buf, C.byref(nf)) == ssa.ERR_ARG
    assert lib.ssa_verify_batch_screened_device(None, buf, buf, None, buf, None, 1, 1, 1, None, 0, buf, None) == ssa.ERR_ARG
    assert lib.ssa_debug_screen_segments(None, 4) == ssa.ERR_ARG
    out = (C.c_uint64 * 8)()
    assert lib.ssa_debug_screen_plan(1000, 0, None) == ssa.ERR_ARG
    assert lib.ssa_debug_screen_plan(0, 0, out) == ssa.ERR_ARG
    assert lib.ssa_debug_screen_plan((1 << 30) + 1, 0, out) == ssa.ERR_ARG
    assert lib.ssa_debug_screen_plan(5000, 33, out) == ssa.ERR_ARG


def _ns():
    ns = set(range(3073, 3073 + 600, 37)) | {4095, 4096, 4097, 5000, 20000, 65535, 65536, 1 << 20, (1 << 20) + 1,
                                              SLICE - 1, SLICE, SLICE + 1, SLICE + 255, 3 * SLICE + 4097, 1 << 30}
    for k in range(12, 31):
        ns |= {(1 << k) - 1, 1 << k, (1 << k) + 257}
    return sorted(n for n in ns if 3073 <= n <= 1 << 30)


@pytest.mark.parametrize("coeff_bytes", [0, 16, 32])
def test_plan_invariants(coeff_bytes):
    for n in _ns():
        p = ssa.debug_screen_plan(n, coeff_bytes)
        first = min(n, SLICE)
        k, seg = p["segments"], p["segment_lanes"]
        c = p["window_bits"]
        # segments are whole 256-lane blocks, only the last one is ragged, and they cover the slice exactly
        assert seg % 256 == 0 and 1 <= k <= 256, (n, p)
        assert (k - 1) * seg < first <= k * seg, (n, p)
        # automatic K: the largest power of two <= 256 whose segments hold at least 1024 lanes
        want_k = 256
        while want_k > 1 and first // want_k < 1024:
            want_k //= 2
        assert k <= want_k, (n, p)
        # K 2^(c-1) within the 256 x 128 grouping grid
        assert p["buckets_per_window"] == k << (c - 1) <= 1 << 15, (n, p)
        assert c == 8 and p["windows"] * c >= 255 and (p["windows"] - 1) * c < 255
        # 128-bit coefficients fill whole windows; 32-byte ones reach every window
        if coeff_bytes in (0, 16):
            assert 128 % c == 0 and p["r_windows"] * c == 128
        else:
            assert p["r_windows"] == p["windows"]
        # segments never straddle a slice: every slice has its own plan, the whole batch is covered
        slices = (n + SLICE - 1) // SLICE
        assert p["slices"] == slices
        last = n - (slices - 1) * SLICE
        lp = ssa.debug_screen_plan(last, coeff_bytes)
        assert (lp["segments"] - 1) * lp["segment_lanes"] < last <= lp["segments"] * lp["segment_lanes"]
        assert p["total_segments"] == (slices - 1) * k + lp["segments"]
        assert SLICE % 256 == 0


def test_plan_examples():
    p = ssa.debug_screen_plan(1 << 20)
    assert (p["segments"], p["segment_lanes"], p["windows"], p["r_windows"]) == (256, 4096, 32, 16)
    p = ssa.debug_screen_plan(5000)
    assert (p["segments"], p["segment_lanes"]) == (4, 1280)
    p = ssa.debug_screen_plan(20000)
    assert (p["segments"], p["segment_lanes"]) == (16, 1280)


def test_cxx_mirror_declares_verify_batch_statuses(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    src = tmp_path / "t.cpp"
    src.write_text('#include "%s/schnorr-sig_amd/host/schnorr_sig.hpp"\n'
                   "using namespace schnorr_sig;\n"
                   "std::vector<uint8_t> f(Context &cx, const std::vector<Signature> &s, const std::vector<PublicKey> &p,\n"
                   "                       const std::vector<std::pair<const uint8_t *, size_t>> &m, Rng rng) {\n"
                   "  return verify_batch_statuses(cx, s, p, m, rng);\n"
                   "}\n" % ROOT)
    subprocess.check_call([cxx, "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", str(src)])
