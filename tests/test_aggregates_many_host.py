"""ssa_verify_aggregates_many without a GPU: the header and the exports, the ABI version, the
refusals that need no device, the byte offsets of the wire layout against Python integers, and the host-side planner
(ssa_debug_aggregates_plan): groups, paths, padded segments and the tree's descriptors, checked against a plain Python
statement of the rules."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "schnorr_sig_amd.h")
NEW = ("ssa_verify_aggregates_many", "ssa_verify_aggregates_many_device")
SPAN = 512


def test_header_declares_both_after_the_length_macro():
    text = open(HEADER).read()
    at = text.index("#define SSA_AGGREGATE_LENGTH")
    for name in NEW:
        m = re.search(r"^int %s\(ssa_ctx \*ctx, const uint8_t \*(d_)?aggs, const uint64_t \*counts, size_t k," % name, text, re.M)
        assert m and m.start() > at, name
    assert re.search(r"#define SSA_ABI_VERSION 5\b", text)


def test_library_exports_them_and_the_abi_version_stays():
    import schnorr_sig_amd as ssa
    for name in NEW + ("ssa_debug_aggregates_plan", "ssa_debug_aggregates_many_coeffs"):
        assert name in ssa.ABI_SYMBOLS and hasattr(ssa._lib, name)
    assert ssa.ABI_VERSION == 5 and ssa._lib.ssa_abi_version() == 5
    for meth in ("verify_aggregates", "verify_aggregates_device", "aggregates_coeffs"):
        assert callable(getattr(ssa.Engine, meth))


def test_refusals_that_need_no_device():
    import ctypes as C
    import schnorr_sig_amd as ssa
    one = (C.c_uint64 * 1)(1)
    for fn in (ssa._lib.ssa_verify_aggregates_many, ssa._lib.ssa_verify_aggregates_many_device):
        assert fn(None, None, None, 0, None, None, None, None, 0, 0, None) == ssa.ERR_ARG          # no context, even for k = 0
        assert fn(None, None, one, 1, None, None, None, None, 0, 0, None) == ssa.ERR_ARG
    assert ssa._lib.ssa_debug_aggregates_many_coeffs(None, None, one, 1, None, None, None, 0, 0, None) == ssa.ERR_ARG
    assert ssa._lib.ssa_debug_aggregates_plan(None, 1, 1 << 23, 3072, None, 0) == ssa.ERR_ARG       # counts missing
    # one aggregate above the MSM slice; more than SSA_MAX_BATCH (2^30) lanes in all
    assert ssa.debug_aggregates_plan([1024, 1025], msm_slice=1024) is None
    assert ssa.debug_aggregates_plan([1024, 1024], msm_slice=1024) is not None
    assert ssa.debug_aggregates_plan([1 << 29] * 3, msm_slice=1 << 30) is None
    assert ssa.debug_aggregates_plan([1 << 29] * 2, msm_slice=1 << 30)["lanes"] == 1 << 30
    with pytest.raises(ssa.MalformedInput):
        ssa.pack_aggregates([bytes(33)])


def test_wire_offsets_against_python_integers():
    """aggregate j starts at byte 49 (n_0 + ... + n_(j-1)) + 32 j; the planner's prefix sums are the lanes before it"""
    import schnorr_sig_amd as ssa
    counts = [0, 3, 0, 0, 700, 1, 0, 513, 2, 0]
    blobs = [bytes([j + 1]) * (49 * n + 32) for j, n in enumerate(counts)]
    wire = b"".join(blobs)
    lanes = 0
    for j, n in enumerate(counts):
        start = 49 * lanes + 32 * j
        assert wire[start:start + 49 * n + 32] == blobs[j]
        assert start + 49 * n == 49 * (lanes + n) + 32 * j           # where its e_agg stands
        lanes += n
    assert len(wire) == 49 * lanes + 32 * len(counts)
    got = ssa.pack_aggregates(blobs)
    assert got[0].tolist() == counts and got[1][:len(wire)].tobytes() == wire
    pl = ssa.debug_aggregates_plan(counts)
    assert pl["lanes"] == lanes
    # the top workgroups name each non-empty aggregate once, with its n_j, and the first pass starts at its first lane
    tops = sorted((d[2], d[3]) for p in pl["passes"] for d in p if d[3])
    assert tops == [(j, n) for j, n in enumerate(counts) if n]
    first = {}
    for d in pl["passes"][0]:
        j = d[2] if d[3] else None
        if j is not None:
            first[j] = d[0]
    before = np.concatenate([[0], np.cumsum(counts)])
    assert all(first[j] == before[j] for j in first)


def python_plan(counts, slice_, small_max):
    """the rules of DESIGN.md section 21, restated"""
    pad = lambda n: (n + 255) // 256 * 256
    groups, j, lane = [], 0, 0
    while j < len(counts):
        g, seg = [], 256
        while j < len(counts) and len(g) < 256:
            s2 = max(seg, pad(counts[j]))
            if g and s2 * (len(g) + 1) > slice_:
                break
            seg = s2
            g.append(counts[j])
            j += 1
        groups.append({"first_aggregate": j - len(g), "aggregates": len(g), "first_lane": lane, "lanes": sum(g),
                       "segment_lanes": seg, "bucket": int(sum(g) > small_max)})
        lane += sum(g)
    # the tree: per aggregate the nodes of each pass; one workgroup per 512, the last pass writes the root
    passes = []
    state = {j: (off, n) for j, (off, n) in enumerate(zip(np.concatenate([[0], np.cumsum(counts)])[:-1], counts)) if n}
    while state:
        descs, nxt, new = [], 0, {}
        for j in sorted(state):
            off, c = state[j]
            g = (c + SPAN - 1) // SPAN
            for b in range(g):
                descs.append((int(off) + SPAN * b, min(SPAN, c - SPAN * b), j if g == 1 else nxt + b, counts[j] if g == 1 else 0))
            if g > 1:
                new[j] = (nxt, g)
                nxt += g
        passes.append(descs)
        state = new
    return groups, passes


@pytest.mark.parametrize("counts,slice_,small_max", [
    ([513], 1 << 23, 3072),
    ([0, 0], 1 << 23, 3072),
    ([1] * 257, 1 << 23, 3072),
    ([1, 2, 3, 255, 256, 257, 511, 512, 513, 0, 1], 1 << 23, 3072),
    ([600, 300, 1024, 257], 1 << 23, 0),
    ([1000, 1000, 10, 2048, 1], 2048, 100),             # groups cut by the slice: 2 x 1024, then 10 alone before 2048
    ([512 * 512 + 1, 5, 512 * 3], 1 << 23, 3072),       # three passes for the first, two for the last
])
def test_planner_follows_the_rules(counts, slice_, small_max):
    import schnorr_sig_amd as ssa
    pl = ssa.debug_aggregates_plan(counts, msm_slice=slice_, small_max=small_max)
    groups, passes = python_plan(counts, slice_, small_max)
    assert pl["groups"] == groups
    assert pl["passes"] == passes and pl["descriptors"] == sum(len(p) for p in passes)
    for g in pl["groups"]:
        assert g["aggregates"] <= 256 and g["segment_lanes"] % 256 == 0
        assert g["aggregates"] == 1 or g["aggregates"] * g["segment_lanes"] <= slice_
    assert sum(g["aggregates"] for g in pl["groups"]) == len(counts)


def test_planner_examples_by_hand():
    import schnorr_sig_amd as ssa
    pl = ssa.debug_aggregates_plan([513])
    assert pl["passes"] == [[(0, 512, 0, 0), (512, 1, 1, 0)], [(0, 2, 0, 513)]]
    assert pl["groups"] == [{"first_aggregate": 0, "aggregates": 1, "first_lane": 0, "lanes": 513, "segment_lanes": 768,
                             "bucket": 0}]
    pl = ssa.debug_aggregates_plan([0, 0])
    assert pl["passes"] == [] and pl["lanes"] == 0 and len(pl["groups"]) == 1 and pl["groups"][0]["aggregates"] == 2
    pl = ssa.debug_aggregates_plan([1] * 257)
    assert [g["aggregates"] for g in pl["groups"]] == [256, 1] and len(pl["passes"]) == 1
    assert pl["passes"][0][256] == (256, 1, 256, 1)
    pl = ssa.debug_aggregates_plan([2048, 2048, 2048], msm_slice=4096, small_max=3072)
    assert [(g["aggregates"], g["bucket"]) for g in pl["groups"]] == [(2, 1), (1, 0)]


def test_cxx_mirror_declares_verify_many(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    src = tmp_path / "t.cpp"
    src.write_text('#include "%s/schnorr-sig_amd/host/schnorr_sig.hpp"\n'
                   "using namespace schnorr_sig;\n"
                   "std::vector<uint32_t> f(Context &cx, const std::vector<AggregateSignature> &a,\n"
                   "                        const std::vector<PublicKey> &p,\n"
                   "                        const std::vector<std::pair<const uint8_t *, size_t>> &m) {\n"
                   "  return AggregateSignature::verify_many(cx, a, p, m);\n"
                   "}\n" % ROOT)
    subprocess.check_call([cxx, "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", str(src)])
