"""ssa_aggregates_many without a GPU: the exports, the refusals that need no device, the partial
offsets of the segmented fold (ssa_debug_aggregates_fold_plan) against a brute-force count of (workgroup, aggregate) pairs,
and the mirror's splitting of the output against the packing verify_aggregates does."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "schnorr_sig_amd.h")
NEW = ("ssa_aggregates_many", "ssa_aggregates_many_device", "ssa_debug_aggregates_fold_plan")


def brute(counts):
    """pfirst by definition: for every aggregate the distinct workgroups (lane >> 8) its dense lanes stand in"""
    pf, lane = [0], 0
    for n in counts:
        pf.append(pf[-1] + len({(lane + l) >> 8 for l in range(n)}))
        lane += n
    return pf


def slot_pairs(counts):
    """every (workgroup, aggregate) pair that shares lanes, in the order of the lanes -> the slot the kernel gives it"""
    first = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    pf = brute(counts)
    seen = {}
    for j, n in enumerate(counts):
        for l in range(n):
            b = (int(first[j]) + l) >> 8
            seen[(b, j)] = pf[j] + b - (int(first[j]) >> 8)
    return seen, pf


def test_header_and_exports():
    import schnorr_sig_amd as ssa
    text = open(HEADER).read()
    at = text.index("int ssa_verify_aggregates_many(")
    for name in NEW:
        m = re.search(r"^int(64_t)? %s\(" % name, text, re.M)
        assert m and m.start() > at, name
        assert name in ssa.ABI_SYMBOLS and hasattr(ssa._lib, name)
    assert re.search(r"#define SSA_ABI_VERSION 5\b", text)
    assert ssa.ABI_VERSION == 5 and ssa._lib.ssa_abi_version() == 5
    for meth in ("aggregates", "aggregates_wire", "aggregates_device"):
        assert callable(getattr(ssa.Engine, meth))
    assert callable(ssa.AggregateSignature.aggregate_many)
    mirror = open(os.path.join(ROOT, "schnorr-sig_amd", "host", "schnorr_sig.hpp")).read()
    assert "aggregate_many(Context &cx" in mirror and "ssa_aggregates_many(" in mirror


def test_refusals_that_need_no_device():
    import schnorr_sig_amd as ssa
    one = (C.c_uint64 * 1)(1)
    for fn in (ssa._lib.ssa_aggregates_many, ssa._lib.ssa_aggregates_many_device):
        assert fn(None, None, None, 0, None, None, None, None, 0, 0, 0, None, None, None, None) == ssa.ERR_ARG   # no context
        assert fn(None, None, one, 1, None, None, None, None, 0, 0, 0, None, None, None, None) == ssa.ERR_ARG
    assert ssa._lib.ssa_debug_aggregates_fold_plan(None, 1, None, 0) == ssa.ERR_ARG       # counts missing
    assert ssa.debug_aggregates_fold_plan([1 << 29] * 3) is None                         # more than SSA_MAX_BATCH lanes
    total, pf = ssa.debug_aggregates_fold_plan([])
    assert total == 0 and pf.tolist() == [0]


SHAPES = [
    [0, 0, 5, 0, 300, 0, 0, 7, 0],                  # empty aggregates at the start, in the middle and at the end
    [255, 1, 3], [256, 3], [100, 155, 1], [100, 156, 1], [255], [256], [257], [1, 255, 256, 1],   # ends on lane 255 / 256
    [1] * 300,
    [1], [513], [70000],                            # k = 1
    [1, 0, 2, 255, 256, 257, 0, 513, 3, 1, 0],
]


@pytest.mark.parametrize("counts", SHAPES, ids=lambda c: "k%d_n%d" % (len(c), sum(c)))
def test_fold_plan_counts_the_pairs(counts):
    import schnorr_sig_amd as ssa
    total, pf = ssa.debug_aggregates_fold_plan(counts)
    assert pf.tolist() == brute(counts) and total == pf[-1]
    # the slots are a bijection onto [0, total): every pair has its own partial and no partial is left unwritten
    seen, _ = slot_pairs(counts)
    assert sorted(seen.values()) == list(range(total))
    for (b, j), s in seen.items():
        assert pf[j] <= s < pf[j + 1]


def test_fold_plan_random_counts():
    import schnorr_sig_amd as ssa
    rng = np.random.default_rng(0x26F01D)
    for _ in range(300):
        k = int(rng.integers(1, 40))
        kind = rng.integers(0, 3)
        hi = (4, 300, 1500)[kind]
        counts = [int(c) for c in rng.integers(0, hi, size=k)]
        total, pf = ssa.debug_aggregates_fold_plan(counts)
        assert pf.tolist() == brute(counts), counts
        assert total == pf[-1]
    # the words of the verifier's plan do not move
    pl = ssa.debug_aggregates_plan([3, 0, 700], msm_slice=4096, small_max=512)
    assert pl["lanes"] == 703 and len(pl["groups"]) == 1 and pl["descriptors"] == 4


def test_split_inverts_pack():
    import schnorr_sig_amd as ssa
    rng = np.random.default_rng(0x5B11)
    counts = [0, 3, 0, 0, 70, 1, 0, 513, 2, 0]
    blobs = [rng.integers(0, 256, size=49 * n + 32, dtype=np.uint8) for n in counts]
    got_counts, wire = ssa.pack_aggregates([b.tobytes() for b in blobs])
    assert got_counts.tolist() == counts
    parts = ssa.split_aggregates(got_counts, wire[:-1])                     # (pack_aggregates appends one spare byte)
    assert len(parts) == len(blobs) and all((p == b).all() for p, b in zip(parts, blobs))
    lo = 0
    for j, (n, p) in enumerate(zip(counts, parts)):                          # aggregate j at byte 49 first_j + 32 j
        assert lo == 49 * sum(counts[:j]) + 32 * j and p.size == 49 * n + 32
        lo += p.size
    again_counts, again = ssa.pack_aggregates([p.tobytes() for p in parts])
    assert again_counts.tolist() == counts and (again == wire).all()
    assert ssa.split_aggregates([], np.zeros(0, np.uint8)) == []
    with pytest.raises(ssa.MalformedInput):
        ssa.split_aggregates([2], np.zeros(49 * 2 + 31, np.uint8))
