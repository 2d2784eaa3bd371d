"""The aggregate steps of tests/callscript.py reach the plans they claim to reach: host code only (the library's plan
functions), no device.  What the GPU tests then compare is only as wide as this table."""
import numpy as np

import callscript as cs


def _steps(family):
    return cs.FAMILIES[family]


def test_every_aggregate_family_is_in_the_script_with_a_dirty_and_a_sliced_step():
    assert set(cs.AGG_FAMILIES) <= set(cs.FAMILIES)
    ids = [cs.step_id(s) for s in cs.SCRIPT]
    assert len(ids) == len(set(ids))
    for fam in ("aggregate", "verify_aggregate", "verify_aggregates", "aggregates", "aggregate_valid",
                "aggregate_valid_cached", "aggregator", "aggverifier"):
        assert cs.DIRTY[fam].family == fam and cs.DIRTY[fam].n == cs.DIRTY_N and cs.DIRTY[fam].variant.endswith(".dirty")
    assert set(cs.OLD_DIRTY).isdisjoint(cs.AGG_FAMILIES) and len(cs.DIRTY) == len(cs.OLD_DIRTY) + 8
    sliced = {(s.family, s.variant) for s in cs.SLICED if s.family in cs.AGG_FAMILIES}
    assert {("aggregate_sliced", "check.host.honest"), ("verify_aggregate_sliced", "honest.host"), ("aggregate_valid", "host"),
            ("aggregate_valid_keyed_cached", "host"), ("verify_aggregates_cached", "sliced.wire.host"),
            ("aggregator", "keyed.holdkeys"), ("aggverifier", "mixed.wire.require2")} <= sliced
    assert all(s.n == cs.SLICED_N for s in cs.SLICED)


def test_the_count_lists_reach_both_paths_more_than_one_group_and_every_slice_boundary():
    import schnorr_sig_amd as ssa
    for fam in ("aggregates", "verify_aggregates", "verify_aggregates_cached"):
        assert {s.variant.split(".")[0] for s in _steps(fam)} == {"edges", "paths", "many"}
        assert all(s.n == cs.N_OF[s.variant.split(".")[0]] for s in _steps(fam))
    many = ssa.debug_aggregates_plan(cs.COUNTS["many"])
    assert len(cs.COUNTS["many"]) > 256 and len(many["groups"]) > 1                      # AG_GROUP_MAX = 256
    assert {g["bucket"] for g in many["groups"]} == {0, 1}                                # a group on each path, in one call
    assert [g["bucket"] for g in ssa.debug_aggregates_plan(cs.COUNTS["edges"])["groups"]] == [0]
    assert [g["bucket"] for g in ssa.debug_aggregates_plan(cs.COUNTS["paths"])["groups"]] == [1]
    for name in ("edges", "many", "allbad"):       # empty aggregates: the first keeps its zero scalar, the second does not
        assert cs.COUNTS[name].count(0) >= (2 if name != "allbad" else 1)
    for name in ("edges", "many"):                # neighbours inside one 256-lane workgroup of the fold
        counts = cs.COUNTS[name]
        start, _ = cs.lane_starts(counts)
        assert any(counts[j] and counts[j + 1] and start[j + 1] % 256 for j in range(len(counts) - 1)), name
        parts, pfirst = ssa.debug_aggregates_fold_plan(counts)       # a shared workgroup gives each of the two a partial sum
        assert parts == int(pfirst[-1]) > -(-cs.N_OF[name] // 256), name
    # 12 345 lanes are three 5000-lane slices, and an aggregate straddles each of the two boundaries
    assert -(-cs.SLICED_N // cs.SLICE) == 3
    start, _ = cs.lane_starts(cs.COUNTS["sliced"])
    for edge in (cs.SLICE, 2 * cs.SLICE):
        assert any(a < edge < b for a, b in zip(start, start[1:])), edge
    assert max(cs.COUNTS["sliced"]) <= cs.SLICE                                           # no n_j above the MSM slice
    plan = ssa.debug_aggregates_plan(cs.COUNTS["sliced"], msm_slice=cs.SLICE)
    assert plan is not None and len(plan["groups"]) >= 3


def test_the_sizes_straddle_the_boundaries_of_the_aggregate_side():
    import schnorr_sig_amd as ssa
    for fam in ("aggregate", "aggregate_valid", "verify_aggregate"):
        sizes = {s.n for s in _steps(fam)}
        assert {1, 257, 512, 513, 3072, 3073, 4095, 4096, 20000} <= sizes, (fam, sizes)
    plan = ssa.debug_screen_plan(20000, 32)
    assert plan["segments"] > 1 and 20000 % plan["segment_lanes"] != 0
    assert any(s.n == 20000 and s.variant == "screened" for s in _steps("aggregator"))
    # the ragged pushes: one completes a block exactly, one completes none, one ends in a ragged tail
    seen = set()
    for lo, hi in cs.cuts(1500):
        _, done, _, tail = ssa.aggregator_plan(lo, hi - lo)
        seen.add((done > 0, tail > 0))
    assert {(True, False), (False, True), (True, True)} <= seen
    assert {s.n for s in _steps("aggregator")} >= {257, 1500, 5000, 20000}
    # at most 12 lanes of a batch are bad: the pools of 1500 lanes and more finish at 512 | 513
    assert all(s.n - 12 >= 513 for s in _steps("aggregator") if s.n >= 1500)
    # a finish prefix on each side of 512 and of 8192 (AGV_KST_SPAN), the latter through a key cache
    span = ssa.aggverifier_key_span()
    assert span == 8192 and {512, 513, span, span + 1} <= set(cs.FINISH_PREFIXES)
    for lo, hi in ((512, 513), (span, span + 1)):
        keyed = [s for s in _steps("aggverifier") + cs.SLICED if s.family == "aggverifier" and s.n >= hi
                 and (lo == 512 or s.variant.split(".")[0] in ("cached", "wire") or "require2" in s.variant)]
        assert keyed, (lo, hi)
    assert {s.variant.replace(".dev", "") for s in _steps("aggverifier")} >= {"plain", "cached", "wire", "mixed",
                                                                             "mixed.wire.require2"}
    assert {s.variant.replace(".dev", "") for s in _steps("aggregator")} == {"screened", "noscreen", "cached",
                                                                            "keyed.holdkeys", "index.admission"}


def test_the_scenario_of_the_aggregator_is_a_function_of_the_inputs():
    """the by-construction bookkeeping of the streaming scenario on inputs made up here: no signature is needed for it"""
    n = 1500
    step = cs.Step("aggregator", "index.admission", n, 5)
    inp = {"n": n, "kinds": {0: "e_bit", 7: "e_ge_q", 512: "offsub", 601: "identity", n - 1: "noncanon_pk"}, "dup": (2, n - 3)}
    sc = cs.aggregator_scenario(step, inp)
    hows = [h for _, _, h in sc["chunks"]]
    assert hows == ["noscreen", "screened", "cached", "noscreen", "screened"]
    # lane 0 goes in without a screen, lane 7 is malformed everywhere, lane 512 is the cached push: its key is dropped
    assert list(np.nonzero(sc["status"])[0]) == [7, 512, n - 1] and sc["status"][512] == 1
    assert sc["held"] == n - 3 and sc["takes"] == [1, 512, 513, n - 3]
    k0, k4 = sc["k0"], sc["k4"]
    assert k4.size == sc["k1"].size - 513 - sc["indices"].size and set(k4) <= set(sc["k1"]) <= set(k0)
    # the doubled lane answers with the lower place while that lane is held
    place = {int(lane): p for p, lane in enumerate(k0)}
    assert sc["places1"][-4] == place[2] != place[n - 3] and list(sc["places1"][-2:]) == [cs.UNKNOWN] * 2
    assert sc["places1"][-3] == 0 == sc["places1"][0]
