"""A call's result depends on its inputs alone: not on what the context's workspaces held before (poison), not on the call
that ran before it (dirty predecessor), not on the order of earlier calls, and not on a setting that was set and reset
("What a call may assume about its workspaces").  Every step of tests/callscript.py is first run alone on a
context that has run nothing else -- that result is checked by construction and against the CPU oracle -- and every other
run must equal it exactly."""
import ctypes as C
import os

import numpy as np
import pytest

import callscript as cs

pytestmark = pytest.mark.gpu

POISON_BYTES = [0x00, 0xFF, 0xA5]     # counters start from it / slot tables call it "empty" / everything else
SLICED_FAMILIES = sorted({s.family for s in cs.SLICED})


def _engine(sliced=False, **env):
    """an engine of this test's own; sliced: 5000-lane slices, so that 12 345 lanes take three and the twin is used"""
    import schnorr_sig_amd as ssa
    if sliced:
        env.update(SSA_LANE_SLICE=str(cs.SLICE), SSA_MSM_SLICE=str(cs.SLICE))
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return ssa.Engine(0)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


class Ctx:
    """an engine with the persistent objects of the script on it"""

    def __init__(self, maker, sliced=False, **env):
        self.eng = _engine(sliced, **env)
        self.objs = cs.Objs(self.eng, maker)
        self.maker = maker

    def run(self, step):
        return cs.run(step, self.eng, self.objs, self.maker)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.objs.close()
        self.eng.close()
        return False


_REF = {}


def reference(step, maker, sliced=False):
    """the step alone on a context that has run nothing else (computed once, shared, never changed)"""
    key = (step, sliced)
    if key not in _REF:
        with Ctx(maker, sliced) as c:
            res = c.run(step)
        for v in res.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _REF[key] = res
    return _REF[key]


def assert_equals_reference(c, step, oracle, sliced=False, what=""):
    got = c.run(step)
    diff = cs.same(got, reference(step, c.maker, sliced), oracle)
    assert diff is None, "%s %s: %s" % (what, cs.step_id(step), diff)


# ---------------------------------------------------------------------------------------------------- reference pass
@pytest.mark.parametrize("family", list(cs.FAMILIES) + ["sliced"])
def test_reference_pass_agrees_with_construction_and_oracle(engine, oracle, family):
    sliced = family == "sliced"
    for step in (cs.SLICED if sliced else cs.FAMILIES[family]):
        res = reference(step, engine, sliced)
        inp = cs.inputs(step, engine)
        cs.check_expected(step, inp, res)
        cs.check_oracle(step, inp, res, oracle)


def test_the_script_covers_the_plans_it_claims():
    """20 000 signatures are several screened segments with a ragged last one; 12 345 lanes are three 5000-lane slices"""
    import schnorr_sig_amd as ssa
    plan = ssa.debug_screen_plan(20000, 32)
    assert plan["segments"] > 1 and 20000 % plan["segment_lanes"] != 0 and plan["slices"] == 1
    eng = _engine(sliced=True)
    try:
        info = eng.info()
        assert info["lane_slice"] == info["msm_slice"] == cs.SLICE and info["two_streams"]
        assert -(-cs.SLICED_N // cs.SLICE) == 3
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------------- poison
@pytest.mark.parametrize("family", list(cs.FAMILIES))
@pytest.mark.parametrize("byte", POISON_BYTES, ids=lambda b: "0x%02X" % b)
def test_poisoned_workspaces_do_not_change_a_result(engine, oracle, byte, family):
    steps = cs.FAMILIES[family]
    with Ctx(engine) as c:
        c.run(max(steps, key=lambda s: s.n))             # sizes the workspaces: every later step fits, nothing is re-allocated
        for step in steps:
            c.eng.debug_poison_workspaces(byte)
            assert_equals_reference(c, step, oracle, what="poison 0x%02X" % byte)


@pytest.mark.parametrize("family", SLICED_FAMILIES)
@pytest.mark.parametrize("byte", POISON_BYTES, ids=lambda b: "0x%02X" % b)
def test_poisoned_workspaces_of_both_stream_sets_do_not_change_a_result(engine, oracle, byte, family):
    steps = [s for s in cs.SLICED if s.family == family]
    with Ctx(engine, sliced=True) as c:
        c.run(steps[0])                                   # makes the twin and sizes both sets
        for step in steps:
            c.eng.debug_poison_workspaces(byte)
            assert_equals_reference(c, step, oracle, sliced=True, what="poison 0x%02X (sliced)" % byte)


# ---------------------------------------------------------------------------------------------------- dirty predecessor
@pytest.mark.parametrize("second", list(cs.DIRTY))
@pytest.mark.parametrize("first", list(cs.DIRTY))
def test_a_dirty_predecessor_does_not_change_a_result(engine, oracle, first, second):
    """the families that share ws_h, ws_tab, the msm_*, scr_*, dd_*, kc_*, ky_* and staging buffers, every ordered pair"""
    with Ctx(engine) as c:
        if first in cs.SCREENED:
            c.eng.debug_screen_segments(256)              # as many segment slots as a slice can have
        try:
            dirty = c.run(cs.DIRTY[first])
        finally:
            c.eng.debug_screen_segments(0)
        if "status" in dirty:
            assert dirty["status"].all() and dirty["nfail"] == cs.DIRTY_N
        else:
            assert dirty["verdict"] == 3
        for step in sorted(cs.FAMILIES[second], key=lambda s: s.n):
            if step.n < cs.DIRTY_N:
                assert_equals_reference(c, step, oracle, what="after dirty " + first)


# ---------------------------------------------------------------------------------------------------- order
def _refused_calls(c):
    """calls that are refused with SSA_ERR_ARG: a batch size out of range, a null pointer, a cache of the wrong mode"""
    import schnorr_sig_amd as ssa
    lib, ctx = ssa._lib, c.eng._ctx
    buf = np.zeros(4 * 96, np.uint8)
    p, nf = C.c_void_p(buf.ctypes.data), C.c_uint64(7)
    assert lib.ssa_verify_many(ctx, p, p, None, p, None, 8, 8, (1 << 30) + 1, 1, p, C.byref(nf)) == ssa.ERR_ARG
    assert lib.ssa_verify_many(ctx, None, p, None, p, None, 8, 8, 4, 1, p, C.byref(nf)) == ssa.ERR_ARG
    assert lib.ssa_verify_batch_screened(ctx, p, p, None, p, None, 8, 8, 4, None, None, C.byref(nf)) == ssa.ERR_ARG
    st = np.zeros(12, np.uint64)
    assert lib.ssa_verify_many_cached(ctx, c.objs.get("wire").handle, p, p, None, p, None, 8, 8, 4, 1, None, p,
                                      C.byref(nf), C.c_void_p(st.ctypes.data)) == ssa.ERR_ARG
    assert nf.value == 7 and not buf.any()


@pytest.mark.parametrize("order", ["ascending", "descending", "shuffle-1", "shuffle-2"])
def test_the_order_of_earlier_calls_does_not_change_a_result(engine, oracle, order):
    """the whole script on ONE context; key set, caches and signer set are made once and live through the run"""
    steps = sorted(cs.SCRIPT, key=lambda s: (s.n, s.seed))
    if order == "descending":
        steps.reverse()
    elif order != "ascending":
        steps = [steps[k] for k in np.random.default_rng(int(order[-1])).permutation(len(steps))]
    with Ctx(engine) as c:
        for k, step in enumerate(steps):
            if k % 7 == 3:
                _refused_calls(c)
            assert_equals_reference(c, step, oracle, what="%s, call %d" % (order, k))


def test_the_order_of_earlier_calls_does_not_change_a_result_in_slices(engine, oracle):
    with Ctx(engine, sliced=True) as c:
        for step in list(reversed(cs.SLICED)) + cs.SLICED[::3]:
            assert_equals_reference(c, step, oracle, sliced=True, what="sliced")


# ---------------------------------------------------------------------------------------------------- sticky settings
def _ends(family):
    steps = sorted(cs.FAMILIES[family], key=lambda s: s.n)
    return [steps[0], steps[-1]]


# the smallest and the largest step of each family that a setting can reach
STICKY_STEPS = [s for f in ("verify_batch_screened", "verify_many_screened", "verify_many_dedup", "verify_many_cached",
                            "verify_batch_msm", "verify_many") for s in _ends(f)]
VERDICTS = ("status", "nfail", "status_warm", "nfail_warm", "verdict")


def _all_equal(c, oracle, what, only=None):
    """every sticky step equals its reference (only: these results of it -- the statistics follow the forced setting)"""
    for step in STICKY_STEPS:
        got, ref = c.run(step), reference(step, c.maker)
        if only:
            got, ref = ({k: r[k] for k in r if k in only} for r in (got, ref))
        diff = cs.same(got, ref, oracle)
        assert diff is None, "%s %s: %s" % (what, cs.step_id(step), diff)


def test_forced_segments_set_and_reset(engine, oracle):
    with Ctx(engine) as c:
        for k in (1, 7, 256):
            c.eng.debug_screen_segments(k)
            _all_equal(c, oracle, "K = %d" % k, only=VERDICTS)       # the statuses do not depend on k; the counts do
            c.eng.debug_screen_segments(0)
            _all_equal(c, oracle, "after K = %d and back" % k)


def test_forced_dedup_routes_set_and_reset(engine, oracle):
    with Ctx(engine) as c:
        for ratio, bound in ((0.0, 0), (2.0, 0), (2.0, 1)):     # the fallback, the keyed route, one probe per lane
            c.eng.debug_dedup_config(ratio, bound)
            _all_equal(c, oracle, "dedup ratio %s bound %d" % (ratio, bound), only=VERDICTS)
            c.eng.debug_dedup_config()
            _all_equal(c, oracle, "dedup defaults again")


def test_timing_on_and_off(engine, oracle):
    with Ctx(engine) as c:
        c.eng.enable_timing(True)
        _all_equal(c, oracle, "timing on")
        c.eng.enable_timing(False)
        _all_equal(c, oracle, "timing off again")


@pytest.mark.parametrize("overlap", ["0", "1"])
def test_msm_overlap_on_and_off(engine, oracle, overlap):
    with Ctx(engine, SSA_MSM_OVERLAP=overlap) as c:
        _all_equal(c, oracle, "SSA_MSM_OVERLAP=" + overlap)


def test_a_pinned_rng_stays_on_its_context(engine):
    import schnorr_sig_amd as ssa
    a, b = ssa.Engine(0), ssa.Engine(0)
    try:
        sks = cs.signer_keys()
        msgs = np.zeros((5, 16), np.uint8)
        a.debug_pin_rng(cs.RNG_PIN)
        _, pinned1 = a.keygen_sign_many_rng(sks, msgs)
        _, free1 = b.keygen_sign_many_rng(sks, msgs)
        _, pinned2 = a.keygen_sign_many_rng(sks, msgs)
        _, free2 = b.keygen_sign_many_rng(sks, msgs)
        assert (pinned1 == pinned2).all()
        assert not (free1 == free2).all(axis=1).any() and not (free1 == pinned1).all(axis=1).any()
        a.debug_pin_rng(None)
        _, unpinned = a.keygen_sign_many_rng(sks, msgs)
        assert not (unpinned == pinned1).all(axis=1).any()
    finally:
        a.close()
        b.close()
