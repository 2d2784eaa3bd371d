"""Filtering half-aggregation through the key cache (ssa_aggregate_valid_many_cached), host side (no
GPU): the C ABI, the argument checks that return before any device call, and the packing of the Python mirror."""
import ctypes as C
import os

import numpy as np
import pytest

import schnorr_sig_amd as ssa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["ssa_aggregate_valid_many_cached", "ssa_aggregate_valid_many_cached_device",
               "ssa_aggregate_valid_keyed_many_cached", "ssa_aggregate_valid_keyed_many_cached_device"]


def test_new_symbols_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "schnorr_sig_amd.h")).read()
    lib = C.CDLL(ssa.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert "int " + name + "(" in hdr, name
        assert hasattr(lib, name), name
        assert name in ssa.ABI_SYMBOLS, name
    assert ssa._lib.ssa_abi_version() == 5           # additive: the ABI version does not move
    for name in ("aggregate_valid_cached", "aggregate_valid_cached_device", "aggregate_valid_keyed_cached",
                 "aggregate_valid_keyed_cached_device"):
        assert hasattr(ssa.Engine, name), name
    assert "cache" in ssa.AggregateSignature.aggregate_valid.__func__.__code__.co_varnames
    assert "NOT gathered" in hdr                     # the header says that the messages stay where they are
    mirror = open(os.path.join(ROOT, "schnorr-sig_amd", "host", "schnorr_sig.hpp")).read()
    assert mirror.count("aggregate_valid(Context &cx, KeyCache &cache") == 4          # two overloads, declared and defined


def test_null_context_cache_and_outputs_are_refused_without_a_device():
    lib = ssa._lib
    buf = (C.c_uint8 * 512)()
    fake = (C.c_uint8 * 65536)()                      # never dereferenced: a null argument is found first
    nk = C.c_uint64(7)
    stats = (C.c_uint64 * 12)(*([9] * 12))
    nkp = C.byref(nk)

    def affine(fn, ctx, kc, agg=buf, kept=buf, n_kept=nkp):
        return fn(ctx, kc, buf, buf, None, buf, None, 1, 1, 1, agg, kept, n_kept, buf, buf, buf, stats)

    def keyed(fn, ctx, kc, agg=buf, kept=buf, n_kept=nkp):
        return fn(ctx, kc, buf, buf, None, 1, 1, 1, agg, kept, n_kept, buf, buf, stats)
    for form, fns in ((affine, (lib.ssa_aggregate_valid_many_cached, lib.ssa_aggregate_valid_many_cached_device)),
                      (keyed, (lib.ssa_aggregate_valid_keyed_many_cached, lib.ssa_aggregate_valid_keyed_many_cached_device))):
        for fn in fns:
            assert form(fn, None, fake) == ssa.ERR_ARG
            assert form(fn, fake, None) == ssa.ERR_ARG
            assert form(fn, None, None) == ssa.ERR_ARG
    assert list(stats) == [9] * 12 and nk.value == 7   # a refused call writes nothing


def test_the_mirror_checks_the_cache_mode_and_packs_records():
    class FakeCache:
        handle = None

        def __init__(self, wire):
            self.wire = wire
    eng = ssa.Engine.__new__(ssa.Engine)             # no context: the checks below come first
    sigs, pks, msgs = np.zeros((2, 81), np.uint8), np.zeros((2, 96), np.uint8), np.zeros((2, 8), np.uint8)
    with pytest.raises(ValueError):
        eng.aggregate_valid_cached(FakeCache(True), sigs, pks, msgs)
    with pytest.raises(ValueError):
        eng.aggregate_valid_keyed_cached(FakeCache(False), np.zeros((2, 130), np.uint8), msgs)

    class Compressor:
        def compress_many(self, p, pk_inf=None):
            assert pk_inf is not None and pk_inf.tolist() == [0, 1]
            return np.arange(2 * 49, dtype=np.uint8).reshape(2, 49), np.zeros(2, np.uint8)
    sigs = np.arange(2 * 81, dtype=np.uint8).reshape(2, 81) ^ 0x80
    rec = ssa.pack_keyed_records(Compressor(), sigs.reshape(-1), pks, np.array([0, 1], np.uint8))
    assert rec.shape == (2, 130) and rec.dtype == np.uint8 and rec.flags["C_CONTIGUOUS"]
    assert (rec[:, :49] == np.arange(2 * 49, dtype=np.uint8).reshape(2, 49)).all() and (rec[:, 49:] == sigs).all()
    with pytest.raises(ssa.MalformedInput):
        ssa.pack_keyed_records(Compressor(), sigs, pks[:1])
    empty = ssa.pack_keyed_records(Compressor(), np.zeros((0, 81), np.uint8), np.zeros((0, 96), np.uint8))
    assert empty.shape == (0, 130)
