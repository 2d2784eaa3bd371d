"""The streaming aggregator's cached pushes and key column on the CPU: the new symbols, the bytes an
object allocates with and without SSA_AGGR_HOLD_KEYS49, what the entry points refuse before they touch a device, and a
model of the one rule by which both 49-byte columns are written (agx_put49 of ssa_aggregator.hpp) -- the invariant the
kernel helper must keep, stated here as tests/test_aggregator_host.py states the plan of a push."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["ssa_aggregator_push_cached", "ssa_aggregator_push_cached_device", "ssa_aggregator_push_keyed_cached",
       "ssa_aggregator_push_keyed_cached_device", "ssa_aggregator_keys", "ssa_aggregator_keys_device",
       "ssa_debug_aggregator_bytes"]


# ---------------------------------------------------------------------------------------------- symbols
def test_symbols_are_declared_exported_and_bound():
    import schnorr_sig_amd as ssa
    header = open(os.path.join(ROOT, "include", "schnorr_sig_amd.h")).read()
    lib = os.path.join(ROOT, "schnorr-sig_amd", "csrc", "libschnorr_sig_amd.so")
    exported = set(subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout.split())
    for name in NEW:
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in exported, name
        assert name in ssa.ABI_SYMBOLS and getattr(ssa._lib, name).argtypes is not None, name
    assert re.search(r"#define SSA_AGGR_HOLD_KEYS49 2u", header) and ssa.AGGR_HOLD_KEYS49 == 2
    assert ssa.ABI_VERSION == ssa._lib.ssa_abi_version() == 5                     # no exported signature changed
    for method in ("push_keyed", "push_keyed_device", "push_cached_device", "keys", "keys_device", "take_block"):
        assert callable(getattr(ssa.Aggregator, method))


def test_null_handles_are_argument_errors():
    import schnorr_sig_amd as ssa
    lib, nk, buf = ssa._lib, C.c_uint64(7), (C.c_uint8 * 64)()
    stats = (C.c_uint64 * 12)(*([9] * 12))
    for fn in (lib.ssa_aggregator_push_cached, lib.ssa_aggregator_push_cached_device):
        assert fn(None, None, None, None, None, None, None, None, 0, 0, 0, None, C.byref(nk), stats) == ssa.ERR_ARG
    for fn in (lib.ssa_aggregator_push_keyed_cached, lib.ssa_aggregator_push_keyed_cached_device):
        assert fn(None, None, None, None, None, None, 0, 0, 0, None, C.byref(nk), stats) == ssa.ERR_ARG
    assert lib.ssa_aggregator_keys(None, None, 0, buf) == ssa.ERR_ARG
    assert lib.ssa_aggregator_keys_device(None, None, 0, buf) == ssa.ERR_ARG
    assert nk.value == 7 and list(stats) == [9] * 12
    h = C.c_void_p()
    assert lib.ssa_aggregator_create(None, 16, 0, ssa.AGGR_HOLD_KEYS49, C.byref(h)) == ssa.ERR_ARG and not h.value


# ---------------------------------------------------------------------------------------------- what create allocates
@pytest.mark.parametrize("capacity,B", [(1, 0), (511, 0), (512, 0), (513, 0), (1000, 64), (1 << 20, 0), (7, 2)])
def test_bytes_with_and_without_the_key_column(capacity, B):
    import schnorr_sig_amd as ssa
    block = B or 512
    tops = -(-capacity // block)
    plain = ssa.aggregator_bytes(capacity, B)
    assert plain == (49 * capacity + 32, 32 * capacity, 32 * capacity, 32 * tops, 0)        # what it was: about 113 a lane
    held = ssa.aggregator_bytes(capacity, B, hold_keys=True)
    assert held[:4] == plain[:4]
    assert 49 * capacity <= held[4] <= 49 * capacity + 3 and -(-held[4] // 4) * 4 >= -(-49 * capacity // 4) * 4
    if capacity == 1 << 20:
        assert 161 < sum(held) / capacity < 163 and 112 < sum(plain) / capacity < 114


def test_bytes_refuses_what_create_refuses():
    import schnorr_sig_amd as ssa
    out = (C.c_uint64 * 5)()
    assert ssa._lib.ssa_debug_aggregator_bytes(16, 0, 2, None) == ssa.ERR_ARG
    assert ssa._lib.ssa_debug_aggregator_bytes(0, 0, 0, out) == ssa.ERR_ARG
    assert ssa._lib.ssa_debug_aggregator_bytes(16, 3, 0, out) == ssa.ERR_ARG
    for flags in (1, 4, 3, 0x80000000):                                          # SSA_AGGR_NO_SCREEN is a push flag
        assert ssa._lib.ssa_debug_aggregator_bytes(16, 0, flags, out) == ssa.ERR_ARG
    assert ssa._lib.ssa_debug_aggregator_bytes(16, 0, 2, out) == 0


# ---------------------------------------------------------------------------------------------- the rule of the 49-byte columns
class Column:
    """a dword-aligned byte array that records who wrote what: every store is a byte or an aligned dword"""

    def __init__(self, size):
        self.data = np.full(size, 0xEE, np.uint8)
        self.writes = np.zeros(size, np.int64)
        self.dword_owner = {}

    def store8(self, lane, addr, v):
        self.data[addr] = v
        self.writes[addr] += 1
        assert self.dword_owner.setdefault(addr // 4, lane) == lane, "two lanes write into one dword"

    def store32(self, lane, addr, vs):
        assert addr % 4 == 0
        self.data[addr:addr + 4] = vs
        self.writes[addr:addr + 4] += 1
        assert self.dword_owner.setdefault(addr // 4, lane) == lane, "two lanes write into one dword"


def put49(col, d0, d1, place, src, nxt):
    """agx_put49: a dword belongs to the lane its first byte lies in; its bytes behind the lane's 49 come from the next
    lane's source; dwords while they end within d1, bytes at the two edges"""
    lo, hi = 49 * place, 49 * place + 49
    w = (lo + 3) & ~3
    if lo == d0:
        for b in range(lo, min(w, d1)):
            col.store8(place, b, src[b - lo])
    while w < hi:
        if w + 4 <= d1:
            col.store32(place, w, [src[b - lo] if b < hi else nxt[b - hi] for b in range(w, w + 4)])
        else:
            for b in range(w, d1):
                col.store8(place, b, src[b - lo])
        w += 4


@pytest.mark.parametrize("m", [1, 2, 3, 5])
@pytest.mark.parametrize("held", [0, 1, 2, 3, 4, 5, 6, 7])
def test_both_columns_of_a_push_are_written_once_and_nowhere_else(held, m):
    """records of 130 bytes, the key column from offset 0 and the R's from offset 49, as agx_k_append writes them: every
    byte of [49 held, 49 (held + m)) exactly once with the right value, no byte outside, no dword shared"""
    rng = np.random.default_rng(100 * held + m)
    n = 2 * m + 3
    recs = rng.integers(0, 256, size=(n, 130), dtype=np.uint8)
    kept = np.sort(rng.choice(n, m, replace=False))
    size = (49 * (held + m + 2) + 3) // 4 * 4
    for off in (0, 49):
        col = Column(size)
        for c in rng.permutation(m):                       # the threads of a launch run in no order
            src = recs[kept[c], off:off + 49]
            nxt = recs[kept[c + 1], off:off + 49] if c + 1 < m else None
            put49(col, 49 * held, 49 * (held + m), held + c, src, nxt)
        d0, d1 = 49 * held, 49 * (held + m)
        assert (col.writes[d0:d1] == 1).all() and not col.writes[:d0].any() and not col.writes[d1:].any()
        assert (col.data[d0:d1] == recs[kept, off:off + 49].reshape(-1)).all()
        assert (col.data[:d0] == 0xEE).all() and (col.data[d1:] == 0xEE).all()


@pytest.mark.parametrize("cnt", [1, 2, 3, 4, 5, 9])
def test_a_staging_piece_is_the_same_rule_from_byte_zero(cnt):
    """agx_k_move: the piece is a column with d0 = 0; lane t's source is the object's column at 49 src(t), any alignment"""
    rng = np.random.default_rng(cnt)
    column = rng.integers(0, 256, size=49 * 40, dtype=np.uint8)
    src = np.sort(rng.choice(40, cnt, replace=False))
    col = Column((49 * cnt + 3) // 4 * 4)
    for t in rng.permutation(cnt):
        nxt = column[49 * src[t + 1]:49 * src[t + 1] + 49] if t + 1 < cnt else None
        put49(col, 0, 49 * cnt, t, column[49 * src[t]:49 * src[t] + 49], nxt)
    assert (col.writes[:49 * cnt] == 1).all() and not col.writes[49 * cnt:].any()
    assert (col.data[:49 * cnt] == column.reshape(40, 49)[src].reshape(-1)).all()
