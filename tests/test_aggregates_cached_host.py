"""Aggregates through a key cache (ssa_verify_aggregates_many_cached), host side (no GPU): the C
ABI, the argument checks that need no device, and the shape checks of the Python mirror."""
import ctypes as C
import os

import numpy as np
import pytest

import schnorr_sig_amd as ssa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["ssa_verify_aggregates_many_cached", "ssa_verify_aggregates_many_cached_device",
               "ssa_verify_aggregates_many_cached_wire", "ssa_verify_aggregates_many_cached_wire_device"]


def test_new_symbols_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "schnorr_sig_amd.h")).read()
    lib = C.CDLL(ssa.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert "int " + name + "(" in hdr, name
        assert hasattr(lib, name), name
        assert name in ssa.ABI_SYMBOLS, name
    assert "#define SSA_ABI_VERSION 5" in hdr and ssa._lib.ssa_abi_version() == 5     # additive
    for name in ("verify_aggregates_cached", "verify_aggregates_cached_device"):
        assert hasattr(ssa.Engine, name), name
    assert hasattr(ssa.AggregateSignature, "verify_many")
    mirror = open(os.path.join(ROOT, "schnorr-sig_amd", "host", "schnorr_sig.hpp")).read()
    assert "ssa_verify_aggregates_many_cached(" in mirror and "ssa_verify_aggregates_many_cached_wire(" in mirror


def _call(fn, wire, ctx, kc, buf, counts, k, verdicts, stats):
    keys = (buf,) if wire else (buf, None)
    return fn(ctx, kc, buf, counts, k, *keys, buf, None, 80, 80, verdicts, stats)


def test_null_context_and_null_cache_are_refused_without_a_device():
    lib = ssa._lib
    buf = (C.c_uint8 * 4096)()
    fake = (C.c_uint8 * 65536)()                      # never dereferenced: the null pointer is looked at first
    counts = (C.c_uint64 * 2)(3, 2)
    verdicts = (C.c_uint32 * 2)(77, 77)
    stats = (C.c_uint64 * 8)(*([9] * 8))
    for name in NEW_SYMBOLS:
        fn, wire = getattr(lib, name), "_wire" in name
        for k in (2, 0):
            assert _call(fn, wire, None, fake, buf, counts, k, verdicts, stats) == ssa.ERR_ARG, (name, k)
            assert _call(fn, wire, fake, None, buf, counts, k, verdicts, stats) == ssa.ERR_ARG, (name, k)
            assert _call(fn, wire, None, None, buf, counts, k, verdicts, stats) == ssa.ERR_ARG, (name, k)
    assert list(stats) == [9] * 8 and list(verdicts) == [77, 77]      # a refused call writes nothing


class _Cache:
    """what the mirror reads of a KeyCache before it calls the library"""
    handle = None

    def __init__(self, wire):
        self.wire = wire


def test_the_python_mirror_checks_shapes_before_it_calls_the_library():
    eng = object.__new__(ssa.Engine)                  # no context: every check below raises before one is needed
    agg = np.zeros(49 * 2 + 32, np.uint8)
    msgs = np.zeros((2, 80), np.uint8)
    with pytest.raises(ValueError, match="affine key cache takes"):
        eng.verify_aggregates_cached(_Cache(False), [agg], np.zeros((2, 49), np.uint8), msgs)
    with pytest.raises(ValueError, match="wire key cache takes"):
        eng.verify_aggregates_cached(_Cache(True), [agg], np.zeros((2, 96), np.uint8), msgs)
    with pytest.raises(ValueError, match="pk_inf does not go with wire keys"):
        eng.verify_aggregates_cached(_Cache(True), [agg], np.zeros((2, 49), np.uint8), msgs, pk_inf=np.zeros(2, np.uint8))
    with pytest.raises(ssa.MalformedInput):           # three keys for two lanes
        eng.verify_aggregates_cached(_Cache(False), [agg], np.zeros((3, 96), np.uint8), msgs)
    with pytest.raises(ValueError, match="one byte per key"):
        eng.verify_aggregates_cached(_Cache(False), [agg], np.zeros((2, 96), np.uint8), msgs, pk_inf=np.zeros(3, np.uint8))
    with pytest.raises(ssa.MalformedInput):           # not 49 n + 32 bytes
        eng.verify_aggregates_cached(_Cache(False), [agg[:-1]], np.zeros((2, 96), np.uint8), msgs)


def test_the_device_mirror_checks_the_key_bytes_before_it_calls_the_library():
    """a tensor of the other mode's width, or too few keys or flags, would be read past its end on the device"""
    import torch
    eng = object.__new__(ssa.Engine)
    aggs = torch.zeros(49 * 2 + 32, dtype=torch.uint8)
    msgs = torch.zeros((2, 80), dtype=torch.uint8)
    v = torch.zeros(1, dtype=torch.int32)
    k96, k49 = torch.zeros((2, 96), dtype=torch.uint8), torch.zeros((2, 49), dtype=torch.uint8)
    with pytest.raises(ValueError, match="affine key cache takes 192 key bytes"):
        eng.verify_aggregates_cached_device(_Cache(False), aggs, [2], k49, msgs, d_verdicts=v)
    with pytest.raises(ValueError, match="wire key cache takes 98 key bytes"):
        eng.verify_aggregates_cached_device(_Cache(True), aggs, [2], k96, msgs, d_verdicts=v)
    with pytest.raises(ValueError, match="affine key cache takes 192 key bytes"):
        eng.verify_aggregates_cached_device(_Cache(False), aggs, [2], k96[:1], msgs, d_verdicts=v)
    with pytest.raises(ValueError, match="affine key cache takes 192 key bytes"):
        eng.verify_aggregates_cached_device(_Cache(False), aggs, [2], None, msgs, d_verdicts=v)
    with pytest.raises(ValueError, match="one byte per key"):
        eng.verify_aggregates_cached_device(_Cache(False), aggs, [2], k96, msgs, d_verdicts=v,
                                            d_pk_inf=torch.zeros(3, dtype=torch.uint8))
    with pytest.raises(ValueError, match="pk_inf does not go with wire keys"):
        eng.verify_aggregates_cached_device(_Cache(True), aggs, [2], k49, msgs, d_verdicts=v,
                                            d_pk_inf=torch.zeros(2, dtype=torch.uint8))
