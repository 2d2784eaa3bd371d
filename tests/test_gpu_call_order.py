"""A call's result depends on its inputs alone: not on what the context's workspaces held before (poison), not on the call
that ran before it (dirty predecessor), not on the order of earlier calls, and not on a setting that was set and reset
("What a call may assume about its workspaces").  Every step of tests/callscript.py is first run alone on a
context that has run nothing else -- that result is checked by construction and against the CPU oracle -- and every other
run must equal it exactly."""
import ctypes as C
import os
import time

import numpy as np
import pytest

import callscript as cs

pytestmark = pytest.mark.gpu

POISON_BYTES = [0x00, 0xFF, 0xA5]     # counters start from it / slot tables call it "empty" / everything else
SLICED_FAMILIES = sorted({s.family for s in cs.SLICED})


def _engine(sliced=False, **env):
    """an engine of this test's own; sliced: 5000-lane slices, so that 12 345 lanes take three and the twin is used
    ("lanes": the lane slice alone, for the calls that refuse a batch above the MSM slice: callscript.slicing)"""
    import schnorr_sig_amd as ssa
    if sliced:
        env.update(SSA_LANE_SLICE=str(cs.SLICE))
        if sliced != "lanes":
            env.update(SSA_MSM_SLICE=str(cs.SLICE))
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
        self.refusal = None

    def run(self, step):
        return cs.run(step, self.eng, self.objs, self.maker)

    def refusal_objects(self):
        """for the refused calls: an empty aggregator and an empty aggregate verifier of this context, and an aggregator of
        ANOTHER context that holds one lane (made at the first use, closed with the context)"""
        if self.refusal is None:
            inp = cs.inputs(cs.FAMILIES["aggregate"][0], self.maker)
            other = _engine()
            pool = other.aggregator(4)
            assert pool.push(inp["sigs"], inp["pks"], inp["msgs"])[1] == 1
            self.refusal = (self.eng.aggregator(4), self.eng.aggregate_verifier(4), pool, other)
        return self.refusal[:3]

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for obj in self.refusal or ():
            obj.close()
        self.objs.close()
        self.eng.close()
        return False


_REF = {}


def reference(step, maker, sliced=False):
    """the step alone on a context that has run nothing else (computed once, shared, never changed)"""
    sliced = cs.slicing(step) if sliced else False
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
def _reference_pass(engine, oracle, steps, sliced, name):
    t_run = t_model = 0.0
    for step in steps:
        inp = cs.inputs(step, engine)
        t0 = time.perf_counter()
        res = reference(step, engine, sliced)
        t1 = time.perf_counter()
        cs.check_expected(step, inp, res)
        cs.check_oracle(step, inp, res, oracle)
        t_run, t_model = t_run + t1 - t0, t_model + time.perf_counter() - t1
    print("reference pass %s: the calls %.2f s, expectations and models on the CPU %.2f s" % (name, t_run, t_model))


@pytest.mark.parametrize("family", [f for f in cs.FAMILIES if f not in cs.AGG_FAMILIES] + ["sliced"])
def test_reference_pass_agrees_with_construction_and_oracle(engine, oracle, family):
    sliced = family == "sliced"
    steps = [s for s in cs.SLICED if s.family not in cs.AGG_FAMILIES] if sliced else cs.FAMILIES[family]
    _reference_pass(engine, oracle, steps, sliced, family)


# the aggregate side, one item per step: its models hash every lane on the CPU (a transcript of 20 000 lanes is 80 000
# Rescue hashes in the C oracle, about two seconds), so a family in one item would take ten seconds and more
AGG_STEPS = [(s, False) for s in cs.SCRIPT if s.family in cs.AGG_FAMILIES] + \
            [(s, True) for s in cs.SLICED if s.family in cs.AGG_FAMILIES]


@pytest.mark.parametrize("step,sliced", AGG_STEPS, ids=[cs.step_id(s) + ("-sliced" if sl else "") for s, sl in AGG_STEPS])
def test_reference_pass_of_an_aggregate_step_agrees_with_construction_and_models(engine, oracle, step, sliced):
    _reference_pass(engine, oracle, [step], sliced, cs.step_id(step) + (" (sliced)" if sliced else ""))


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


def test_the_lane_slice_alone_cuts_the_calls_that_refuse_a_batch_above_the_msm_slice(engine):
    """the engine of callscript.LANE_SLICED: one MSM slice holds the batch, the key work runs in 5000-lane slices -- the
    keyed producer reports the slices it screened (word [5] of its statistics; the last slice, 2345 lanes, is below the
    small-batch bound and goes to the exact path without a screen)"""
    step = next(s for s in cs.SLICED if s.family == "aggregate_valid_keyed_cached")
    inp = cs.inputs(step, engine)
    eng = _engine(sliced="lanes")
    try:
        info = eng.info()
        assert info["lane_slice"] == cs.SLICE and info["msm_slice"] >= cs.SLICED_N
        with eng.keycache_create(4096, wire=True) as cache:
            stats = eng.aggregate_valid_keyed_cached(cache, inp["keyed"], inp["msgs"])[4]
        assert int(stats[5]) == 2 and int(stats[11]) == 0, [int(v) for v in stats]
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
    with Ctx(engine, sliced=cs.slicing(steps[0])) as c:
        # makes the twin and sizes both sets -- where the call uses a twin: the forms through a key cache run their slices
        # in order on the context's own stream, so for the families of callscript.LANE_SLICED there may be none, and the
        # poison then fills the one set there is (the hook fills a twin only if it exists)
        c.run(steps[0])
        for step in steps:
            c.eng.debug_poison_workspaces(byte)
            assert_equals_reference(c, step, oracle, sliced=True, what="poison 0x%02X (sliced)" % byte)


# ---------------------------------------------------------------------------------------------------- dirty predecessor
@pytest.mark.parametrize("second", list(cs.DIRTY))
@pytest.mark.parametrize("first", list(cs.DIRTY))
def test_a_dirty_predecessor_does_not_change_a_result(engine, oracle, first, second):
    """the families that share ws_h, ws_tab, the msm_*, scr_*, dd_*, kc_*, ky_* and staging buffers, and the aggregate
    families, which share those and the ag_* .. agv_* buffers among themselves: every ordered pair"""
    with Ctx(engine) as c:
        if first in cs.SCREENED:
            c.eng.debug_screen_segments(256)              # as many segment slots as a slice can have
        try:
            dirty = c.run(cs.DIRTY[first])
        finally:
            c.eng.debug_screen_segments(0)
        cs.dirty_check(cs.DIRTY[first], dirty)             # every lane bad or malformed: nothing kept, nothing accepted
        for step in sorted(cs.FAMILIES[second], key=lambda s: s.n):
            if step.n < cs.DIRTY_N:
                assert_equals_reference(c, step, oracle, what="after dirty " + first)


# ---------------------------------------------------------------------------------------------------- order
def _refused_calls(c):
    """calls that are refused with SSA_ERR_ARG: a batch size out of range, a null pointer, a cache of the wrong mode; on
    the aggregate side also an aggregator of another context handed to a mixed push and n_take above the lanes held"""
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
    # ---- the aggregate side: refused with SSA_ERR_ARG, nothing written, no object changed
    ag, av, foreign = c.refusal_objects()
    vp = C.c_void_p
    counts = np.array([2], np.uint64)
    cp = counts.ctypes.data_as(C.POINTER(C.c_uint64))
    place = np.zeros(1, np.uint32)
    before = (ag.info(), av.info(), foreign.info())
    assert lib.ssa_aggregate_many(ctx, p, p, None, p, None, 8, 8, (1 << 30) + 1, 0, p, p, C.byref(nf)) == ssa.ERR_ARG
    assert lib.ssa_aggregate_valid_many(ctx, p, p, None, p, None, 8, 8, (1 << 30) + 1, p, p, C.byref(nf), p) == ssa.ERR_ARG
    assert lib.ssa_verify_aggregate(ctx, None, p, None, p, None, 8, 8, 4) == ssa.ERR_ARG
    assert lib.ssa_verify_aggregates_many(ctx, p, cp, 1, None, None, p, None, 8, 8, p) == ssa.ERR_ARG
    assert lib.ssa_verify_aggregates_many_cached_wire(ctx, c.objs.get("cache").handle, p, cp, 1, p, p, None, 8, 8, p,
                                                      vp(st.ctypes.data)) == ssa.ERR_ARG
    assert lib.ssa_aggverifier_push_mixed(ctx, av.handle, foreign.handle, vp(place.ctypes.data), 1, None, None, None, None,
                                          None, 0, 0, 0) == ssa.ERR_ARG
    assert lib.ssa_aggregator_finish(ctx, ag.handle, 1, p) == ssa.ERR_ARG
    assert lib.ssa_aggverifier_finish(ctx, av.handle, p, 1) == ssa.ERR_ARG
    assert nf.value == 7 and not buf.any() and not st.any() and counts[0] == 2 and place[0] == 0
    assert before == (ag.info(), av.info(), foreign.info()) and foreign.info()["held"] == 1


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
    for mode in (True, "lanes"):              # one context for each way an engine is cut (callscript.slicing)
        steps = [s for s in cs.SLICED if cs.slicing(s) == mode]
        with Ctx(engine, sliced=mode) as c:
            for step in list(reversed(steps)) + steps[::3]:
                assert_equals_reference(c, step, oracle, sliced=True, what="sliced")


# ---------------------------------------------------------------------------------------------------- sticky settings
def _ends(family, variant=None):
    """the smallest and the largest step of a family (variant: of its steps of that variant, host or device form)"""
    steps = sorted((s for s in cs.FAMILIES[family] if variant is None or s.variant.replace(".dev", "") == variant),
                   key=lambda s: s.n)
    return [steps[0], steps[-1]]


# the smallest and the largest step of each family that a setting can reach
STICKY_STEPS = [s for f in ("verify_batch_screened", "verify_many_screened", "verify_many_dedup", "verify_many_cached",
                            "verify_batch_msm", "verify_many") for s in _ends(f)]
STICKY_STEPS += (_ends("aggregate_valid") + _ends("verify_aggregates") + _ends("aggregator", "screened")
                 + _ends("aggverifier", "cached"))
VERDICTS = ("status", "nfail", "status_warm", "nfail_warm", "verdict")


def _all_equal(c, oracle, what, only=None):
    """every sticky step equals its reference (only: these results of it -- the statistics follow the forced setting;
    the aggregate steps carry bytes, statuses, verdicts and counts that are functions of the inputs, and nothing else:
    all of it is compared under every setting)"""
    for step in STICKY_STEPS:
        got, ref = c.run(step), reference(step, c.maker)
        if only and step.family not in cs.AGG_FAMILIES:
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


# ---------------------------------------------------------------------------------------------------- other tables, other blobs
def _blob(variant):
    """variants 2 and 3 of test_alternative_parameter_blobs, the two that move what a fixed-width transcript could
    hard-code: (2) capacity first, padded, the digest from state[4..8]; (3) the length in state[0], the rate at state[4..12]"""
    import struct
    import schnorr_sig_amd as ssa
    b = bytearray(ssa.Engine.default_params())
    struct.pack_into("<IIiIII", b, 8, 7, 4, *{2: (-1, 1, 4, 0), 3: (0, 0, 4, 0)}[variant])
    return bytes(b)


BLOB_SEED = {2: 600000, 3: 700000}      # the steps under another blob have inputs of their own: signed by that engine


@pytest.mark.parametrize("end", ["smallest", "largest"])
@pytest.mark.parametrize("family", cs.AGG_FAMILIES)
@pytest.mark.parametrize("which", ["comb16", "blob2", "blob3"])
def test_other_tables_and_parameters_do_not_change_the_contract(engine, oracle, which, family, end):
    """the smallest and the largest step of every aggregate family (a) on a 16-bit comb for G -- ag_k_finish, the
    finishes and [e_agg - S]G walk it --: exactly the reference; (b) under another parameter blob -- the transcript hashes
    rows of 6 and 8 field elements --: signatures made by that engine, bytes against the models over the oracle with the
    same blob, statuses and verdicts by construction"""
    import schnorr_sig_amd as ssa
    from oracle import Oracle
    steps = sorted(cs.FAMILIES[family], key=lambda s: s.n)
    steps = [steps[0] if end == "smallest" else steps[-1]]          # (one step an item: the models cost seconds)
    if which == "comb16":
        eng = ssa.Engine(0, gtab_bits=16)
        objs = cs.Objs(eng, engine)
        try:
            assert eng.info()["gtab_bits"] == 16
            for step in steps:
                diff = cs.same(cs.run(step, eng, objs, engine), reference(step, engine), oracle)
                assert diff is None, "16-bit comb %s: %s" % (cs.step_id(step), diff)
        finally:
            objs.close()
            eng.close()
        return
    variant = int(which[-1])
    blob = _blob(variant)
    eng = ssa.Engine(0, params=blob)
    objs = cs.Objs(eng, eng)
    try:
        alt = Oracle(blob=blob)                              # (the oracle's parameters are process-wide: put back below)
        for s in steps:
            step = cs.Step(s.family, s.variant, s.n, s.seed + BLOB_SEED[variant])
            inp = cs.inputs(step, eng)
            res = cs.run(step, eng, objs, eng)
            cs.check_expected(step, inp, res)
            cs.check_oracle(step, inp, res, alt)
    finally:
        Oracle()
        objs.close()
        eng.close()
