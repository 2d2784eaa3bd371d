"""Selections of held lanes (ssa_aggregator_finish_select, ssa_aggregator_remove_indices) on the
CPU: the symbols and their documented signatures, the argument errors that need no device, and the Python mirror's
refusal of lists that are no lists of places before any call.  (Everything here fails without the feature.)"""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIGNATURES = {
    "ssa_aggregator_finish_select":
        "int ssa_aggregator_finish_select(ssa_ctx *ctx, ssa_aggregator *ag, const uint32_t *order, size_t m, "
        "uint8_t *agg_out, uint8_t *keys49_out);",
    "ssa_aggregator_finish_select_device":
        "int ssa_aggregator_finish_select_device(ssa_ctx *ctx, ssa_aggregator *ag, const uint32_t *d_order, size_t m, "
        "uint8_t *d_agg_out, uint8_t *d_keys49_out, uint32_t *d_result_out);",
    "ssa_aggregator_remove_indices":
        "int ssa_aggregator_remove_indices(ssa_ctx *ctx, ssa_aggregator *ag, const uint32_t *order, size_t m, "
        "uint64_t *n_kept_out);",
    "ssa_aggregator_remove_indices_device":
        "int ssa_aggregator_remove_indices_device(ssa_ctx *ctx, ssa_aggregator *ag, const uint32_t *d_order, size_t m, "
        "uint64_t *n_kept_out);",
}


def test_symbols_are_declared_with_the_documented_signatures_and_exported():
    import schnorr_sig_amd as ssa
    header = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "schnorr_sig_amd.h")).read())
    vp, sz, u64p = C.c_void_p, C.c_size_t, C.POINTER(C.c_uint64)
    argtypes = {"ssa_aggregator_finish_select": [vp, vp, vp, sz, vp, vp],
                "ssa_aggregator_finish_select_device": [vp, vp, vp, sz, vp, vp, vp],
                "ssa_aggregator_remove_indices": [vp, vp, vp, sz, u64p],
                "ssa_aggregator_remove_indices_device": [vp, vp, vp, sz, u64p]}
    for name, decl in SIGNATURES.items():
        assert decl in header, name
        assert name in ssa.ABI_SYMBOLS
        fn = getattr(ssa._lib, name)
        assert fn.restype is C.c_int32 or fn.restype is C.c_int
        assert list(fn.argtypes) == argtypes[name], name
    assert ssa.ABI_VERSION == ssa._lib.ssa_abi_version() == 5                      # additive: the version stays
    # the contract no longer says that the object cannot choose
    assert "finishing an arbitrary subset without removing it" not in header
    for method in ("finish_select", "finish_select_device", "remove_indices", "remove_indices_device", "take_select"):
        assert callable(getattr(ssa.Aggregator, method))


def test_null_object_and_null_order_are_argument_errors():
    """what the entry points refuse before they touch a device; no output is written"""
    import schnorr_sig_amd as ssa
    lib, nk = ssa._lib, C.c_uint64(7)
    order = (C.c_uint32 * 4)(0, 1, 2, 3)
    agg = np.full(49 * 4 + 32, 0xEE, np.uint8)
    keys = np.full(49 * 4, 0xEE, np.uint8)
    res = (C.c_uint32 * 1)(0xEEEEEEEE)
    p = ssa._ptr
    for m, lst in ((4, order), (0, None), (4, None)):
        assert lib.ssa_aggregator_finish_select(None, None, lst, m, p(agg), p(keys)) == ssa.ERR_ARG
        assert lib.ssa_aggregator_finish_select_device(None, None, lst, m, p(agg), p(keys), res) == ssa.ERR_ARG
        assert lib.ssa_aggregator_remove_indices(None, None, lst, m, C.byref(nk)) == ssa.ERR_ARG
        assert lib.ssa_aggregator_remove_indices_device(None, None, lst, m, C.byref(nk)) == ssa.ERR_ARG
    assert nk.value == 7 and res[0] == 0xEEEEEEEE and (agg == 0xEE).all() and (keys == 0xEE).all()


class _NoCalls:
    """stands where the library does: any call through it fails the test"""

    def __getattr__(self, name):
        raise AssertionError("the library was called: %s" % name)


@pytest.mark.parametrize("order", [[-1], [0, 5, -3], [1 << 32], [3, (1 << 32) + 1], np.array([0, -1], dtype=np.int64),
                                   np.array([1 << 40], dtype=np.uint64), [1.5, 2.0], [[0, 1], [2, 3]]],
                         ids=["negative", "negative later", "2^32", "above 2^32", "int64 array", "uint64 array", "floats",
                              "two dimensions"])
@pytest.mark.parametrize("method", ["finish_select", "finish_select_bytes", "remove_indices", "take_select"])
def test_the_python_mirror_refuses_what_is_no_list_of_places_before_any_call(monkeypatch, method, order):
    import schnorr_sig_amd as ssa
    ag = ssa.Aggregator.__new__(ssa.Aggregator)          # no handle, no engine: nothing here may be reached
    ag.handle, ag.engine, ag.hold_keys = None, None, False
    monkeypatch.setattr(ssa, "_lib", _NoCalls())
    with pytest.raises(ValueError):
        getattr(ag, method)(order)


def test_the_order_reaches_the_library_as_uint32():
    import schnorr_sig_amd as ssa
    for order in ([3, 1, 2], (3, 1, 2), range(3), np.array([3, 1, 2], dtype=np.int64), np.array([3, 1, 2], dtype=np.uint8),
                  np.array([0, 0xFFFFFFFF], dtype=np.uint64)):
        a = ssa._order_u32(order)
        assert a.dtype == np.uint32 and a.flags.c_contiguous and a.tolist() == [int(v) for v in order]
    assert ssa._order_u32([]).size == 0 and ssa._order_u32(np.zeros(0)).size == 0
    strided = np.arange(10, dtype=np.uint32)[::2]
    assert ssa._order_u32(strided).flags.c_contiguous and ssa._order_u32(strided).tolist() == [0, 2, 4, 6, 8]


def test_the_device_mirrors_refuse_tensors_that_are_no_device_lists_before_any_call(monkeypatch):
    """the address of d_order goes to the kernel as it is: a float tensor, a strided view, a tensor in host memory and a
    result word of another type are ValueErrors in the mirror"""
    import torch
    import schnorr_sig_amd as ssa

    class Eng:
        device, _ctx = 0, None
    ag = ssa.Aggregator.__new__(ssa.Aggregator)
    ag.handle, ag.engine, ag.hold_keys = None, Eng(), False
    monkeypatch.setattr(ssa, "_lib", _NoCalls())
    out, res = torch.zeros(49 * 8 + 32, dtype=torch.uint8), torch.zeros(1, dtype=torch.int32)
    bad = [torch.zeros(8, dtype=torch.float32), torch.zeros(8, dtype=torch.int64), torch.zeros(16, dtype=torch.int32)[::2],
           torch.zeros((2, 4), dtype=torch.int32), torch.zeros(8, dtype=torch.int32)]          # the last: host memory
    for d_order in bad:
        with pytest.raises(ValueError):
            ag.finish_select_device(d_order, out, res)
        with pytest.raises(ValueError):
            ag.remove_indices_device(d_order)
