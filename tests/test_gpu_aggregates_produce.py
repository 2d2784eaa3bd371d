"""Many half-aggregates produced in one call (ssa_aggregates_many).  The contract is one equality per
aggregate: its bytes, its result and the status bytes of its lanes are what ssa_aggregate_many gives that batch handed in
alone with the same flags.  Every test compares with that single call on the session's engine; aggregates of at most three
lanes also with the model of tests/aggregate_model.py over the C oracle."""
import ctypes as C
import os

import numpy as np
import pytest

import aggregate_model as am

pytestmark = pytest.mark.gpu

Q = am.Q
OK, INVALID, MALFORMED = 0, 2, 3
# several aggregates in one workgroup, aggregates that start and end mid-workgroup, one over three workgroups whose tree
# needs two passes, and empty ones at every position
COUNTS = [1, 0, 2, 255, 256, 257, 0, 513, 3, 1, 0]
N = sum(COUNTS)                                     # 1288
FIRST = np.concatenate([[0], np.cumsum(COUNTS)]).astype(int)
_STATE = {}


def make_scalars(rng, n):
    s = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    s[:, 31] &= 0x3F
    s[:, 0] |= 1
    return s


class Pool:
    """2048 honest signatures over 80-byte messages (made once)"""

    def __init__(self, engine):
        rng = np.random.default_rng(0x26A66)
        n = 2048
        self.msgs = rng.integers(0, 256, size=(n, 80), dtype=np.uint8)
        self.pks, self.sigs = engine.keygen_sign_many(make_scalars(rng, n), make_scalars(rng, n), self.msgs)


@pytest.fixture
def pool(engine):
    if "pool" not in _STATE:
        _STATE["pool"] = Pool(engine)
    return _STATE["pool"]


def ranges(counts):
    first = np.concatenate([[0], np.cumsum(counts)]).astype(int)
    return [(int(first[j]), int(first[j + 1])) for j in range(len(counts))]


def singles(engine, counts, sigs, pks, msgs, check, inf=None, only=None):
    """the reference: ssa_aggregate_many once per batch -> (list of aggregate bytes, results, statuses, n_fail)"""
    aggs, results, status, nfail = [], [], np.zeros(sum(counts), np.uint8), 0
    for j, (lo, hi) in enumerate(ranges(counts)):
        if only is not None and j not in only:
            aggs.append(None)
            results.append(None)
            continue
        st, agg, stat, nf = engine.aggregate(sigs[lo:hi], pks[lo:hi], msgs[lo:hi] if hi > lo else None,
                                             pk_inf=None if inf is None else inf[lo:hi], check=check)
        aggs.append(agg)
        results.append(st)
        status[lo:hi] = stat
        nfail += nf
    return aggs, results, status, nfail


def many(eng, counts, sigs, pks, msgs, check=False, inf=None):
    """one call over flat arrays -> (the aggregates as the call wrote them, results, statuses, n_fail, the wire bytes)"""
    n = sum(counts)
    _, wire, results, status, nfail = eng.aggregates_wire((sigs[:n], pks[:n], msgs[:n]), check=check, counts=counts,
                                                          pk_inf=None if inf is None else inf[:n])
    import schnorr_sig_amd as ssa
    assert wire.size == 49 * n + 32 * len(counts)
    return ssa.split_aggregates(counts, wire), results.tolist(), status, nfail, wire


def assert_equal_to_singles(got, want, which=None):
    g_aggs, g_res = got[0], got[1]
    w_aggs, w_res, w_status, w_nf = want
    for j in range(len(w_aggs)) if which is None else which:
        assert g_res[j] == w_res[j], j
        assert g_aggs[j].tobytes() == w_aggs[j].tobytes(), j
    if which is None:
        assert (got[2] == w_status).all() and got[3] == w_nf


def clean(engine, pool, check):
    key = ("clean", check)
    if key not in _STATE:
        _STATE[key] = singles(engine, COUNTS, pool.sigs[:N], pool.pks[:N], pool.msgs[:N], check)
        assert _STATE[key][1] == [OK] * len(COUNTS) and _STATE[key][3] == 0
    return _STATE[key]


@pytest.mark.parametrize("check", [False, True])
def test_many_equals_single_on_the_boundary_counts(engine, oracle, pool, check):
    got = many(engine, COUNTS, pool.sigs, pool.pks, pool.msgs, check)
    assert_equal_to_singles(got, clean(engine, pool, check))
    assert got[1] == [OK] * len(COUNTS) and got[3] == 0 and not got[2].any()
    if "model" not in _STATE:
        be = am.oracle_backend(oracle)
        _STATE["model"] = {j: am.aggregate(be, pool.sigs[lo:hi], pool.pks[lo:hi], pool.msgs[lo:hi])
                           for j, (lo, hi) in enumerate(ranges(COUNTS)) if hi - lo <= 3}
    assert sorted(_STATE["model"]) == [0, 1, 2, 6, 8, 9, 10]
    for j, want in _STATE["model"].items():
        assert got[0][j].tobytes() == want, j
    # the list form and the object mirror give the same aggregates
    import schnorr_sig_amd as ssa
    batches = [(pool.sigs[lo:hi], pool.pks[lo:hi], pool.msgs[lo:hi]) for lo, hi in ranges(COUNTS)]
    aggs, results, status, nfail = engine.aggregates(batches, check=check)
    assert [a.bytes for a in aggs] == [g.tobytes() for g in got[0]] and results.tolist() == got[1] and nfail == 0
    assert all(isinstance(a, ssa.AggregateSignature) for a in aggs)


@pytest.mark.parametrize("check", [False, True])
def test_more_heads_than_a_workgroup_has_lanes(engine, pool, check):
    rng = np.random.default_rng(0x300)
    counts = [int(c) for c in rng.integers(1, 6, size=300)]
    n = sum(counts)
    got = many(engine, counts, pool.sigs, pool.pks, pool.msgs, check)
    assert_equal_to_singles(got, singles(engine, counts, pool.sigs[:n], pool.pks[:n], pool.msgs[:n], check))
    # round trip: more than one group of the verifier
    assert engine.verify_aggregates(got[0], pool.pks[:n], pool.msgs[:n]).tolist() == [OK] * 300


@pytest.mark.parametrize("n", [1, 300])
def test_one_aggregate(engine, pool, n):
    got = many(engine, [n], pool.sigs, pool.pks, pool.msgs)
    assert_equal_to_singles(got, singles(engine, [n], pool.sigs[:n], pool.pks[:n], pool.msgs[:n], False))
    assert got[1] == [OK]


def test_round_trip_through_the_verifier(engine, pool):
    import schnorr_sig_amd as ssa
    wire = many(engine, COUNTS, pool.sigs, pool.pks, pool.msgs)[4]
    out = np.full(len(COUNTS), 255, dtype=np.uint32)
    counts = np.array(COUNTS, dtype=np.uint64)
    buf = np.concatenate([wire, np.zeros(1, np.uint8)])           # the output buffer as it is, not split and packed again
    rc = ssa._lib.ssa_verify_aggregates_many(engine._ctx, C.c_void_p(buf.ctypes.data),
                                             counts.ctypes.data_as(C.POINTER(C.c_uint64)), len(COUNTS),
                                             C.c_void_p(pool.pks.ctypes.data), None, C.c_void_p(pool.msgs.ctypes.data), None,
                                             80, 80, C.c_void_p(out.ctypes.data))
    assert rc == 0 and out.tolist() == [OK] * len(COUNTS)


def malform(kind, sigs, pks, i):
    if kind == "e>=q":
        sigs[i, 49:81] = np.frombuffer(int(Q).to_bytes(32, "little"), np.uint8)
    elif kind == "key":
        pks[i, 50] ^= 1                             # a key off the curve
    else:
        sigs[i, 48] |= 0x01                         # an undecodable flag byte of R


@pytest.mark.parametrize("kind", ["e>=q", "key", "R"])
def test_refusal_stays_inside_its_aggregate(engine, pool, kind):
    want = clean(engine, pool, False)
    for lane in (0, N - 1, 255, 256):
        j = int(np.searchsorted(FIRST, lane, side="right")) - 1
        sigs, pks = pool.sigs[:N].copy(), pool.pks[:N].copy()
        malform(kind, sigs, pks, lane)
        aggs, results, status, nfail, _ = many(engine, COUNTS, sigs, pks, pool.msgs)
        assert results == [MALFORMED if a == j else OK for a in range(len(COUNTS))], (lane, results)
        assert not aggs[j].any() and aggs[j].size == 49 * COUNTS[j] + 32
        expect = np.zeros(N, np.uint8)
        expect[lane] = MALFORMED
        assert (status == expect).all() and nfail == 1
        assert_equal_to_singles((aggs, results), want, [a for a in range(len(COUNTS)) if a != j])
        # and the single call refuses that batch in the same way
        one = singles(engine, COUNTS, sigs, pks, pool.msgs[:N], False, only=[j])
        assert one[1][j] == MALFORMED and not one[0][j].any() and (one[2] == expect).all()


def test_check_names_the_smallest_status(engine, pool):
    lane, j = 600, 5                                 # aggregate 5: lanes 514 .. 770
    assert FIRST[j] <= lane < FIRST[j + 1]
    sigs, pks = pool.sigs[:N].copy(), pool.pks[:N].copy()
    sigs[lane, 49] ^= 1                              # well formed, does not verify
    only = [INVALID if a == j else OK for a in range(len(COUNTS))]
    want = clean(engine, pool, True)
    aggs, results, status, nfail, _ = many(engine, COUNTS, sigs, pks, pool.msgs, check=True)
    assert results == only and status[lane] == INVALID and status.sum() == INVALID and nfail == 1
    assert not aggs[j].any()
    assert_equal_to_singles((aggs, results), want, [a for a in range(len(COUNTS)) if a != j])
    one = singles(engine, COUNTS, sigs, pks, pool.msgs[:N], True, only=[j])
    assert one[1][j] == INVALID and (one[2] == status).all()
    # without the check the same input is aggregated, and the verifier rejects exactly that aggregate
    aggs0, results0, status0, nfail0, _ = many(engine, COUNTS, sigs, pks, pool.msgs, check=False)
    assert results0 == [OK] * len(COUNTS) and nfail0 == 0 and not status0.any()
    assert engine.verify_aggregates(aggs0, pks, pool.msgs[:N]).tolist() == only
    # a malformed lane beside it: the smaller status is the aggregate's
    malform("R", sigs, pks, lane + 1)
    aggs, results, status, nfail, _ = many(engine, COUNTS, sigs, pks, pool.msgs, check=True)
    assert results == only and status[lane] == INVALID and status[lane + 1] == MALFORMED and nfail == 2
    one = singles(engine, COUNTS, sigs, pks, pool.msgs[:N], True, only=[j])
    assert one[1][j] == INVALID and (one[2] == status).all()
    # and a malformed lane in another aggregate names its own
    malform("key", sigs, pks, 2)
    results = many(engine, COUNTS, sigs, pks, pool.msgs, check=True)[1]
    assert results == [MALFORMED if a == 2 else v for a, v in enumerate(only)]


def test_no_state_leaks(engine, pool):
    import schnorr_sig_amd as ssa
    sigs = pool.sigs[:N].copy()
    sigs[700, 48] |= 0x01                            # one refused aggregate, so that counters and results are not all zero
    fresh = ssa.Engine(0)
    try:
        want = {c: many(fresh, COUNTS, sigs, pool.pks, pool.msgs, check=c) for c in (False, True)}
        fresh.close()
        fresh = ssa.Engine(0)
        eng = fresh
        big = [700, 0, 900, 5, 443]
        good = many(engine, COUNTS, pool.sigs, pool.pks, pool.msgs)[0]
        for prelude in (lambda: eng.debug_poison_workspaces(0xA5),
                        lambda: many(eng, big, pool.sigs, pool.pks, pool.msgs, check=True),
                        lambda: eng.verify_aggregates(good, pool.pks[:N], pool.msgs[:N]),
                        lambda: eng.debug_poison_workspaces(0xFF)):
            prelude()
            for c in (False, True):
                got = many(eng, COUNTS, sigs, pool.pks, pool.msgs, check=c)
                assert got[1] == want[c][1] and got[3] == want[c][3] == 1
                assert (got[2] == want[c][2]).all() and (got[4] == want[c][4]).all()
    finally:
        fresh.close()
    assert want[False][1][5] == MALFORMED and want[True][1][5] == MALFORMED


def raw(eng, counts, sigs, pks, msgs, flags=0, out=True):
    import schnorr_sig_amd as ssa
    counts = np.array(counts, dtype=np.uint64)
    k, n = counts.size, int(counts.sum())
    wire = np.full(49 * n + 32 * k + 1, 255, dtype=np.uint8)
    results = np.full(max(k, 1), 255, dtype=np.uint32)
    rc = ssa._lib.ssa_aggregates_many(
        eng._ctx, C.c_void_p(sigs.ctypes.data) if n else None, counts.ctypes.data_as(C.POINTER(C.c_uint64)) if k else None, k,
        C.c_void_p(pks.ctypes.data) if n else None, None, C.c_void_p(msgs.ctypes.data) if n else None, None, 80, 80, flags,
        C.c_void_p(wire.ctypes.data) if out else None, C.c_void_p(results.ctypes.data), None, None)
    return rc, wire[:-1], results[:k]


def test_arguments(pool):
    import schnorr_sig_amd as ssa
    old = os.environ.get("SSA_MSM_SLICE")
    os.environ["SSA_MSM_SLICE"] = "512"
    try:
        eng = ssa.Engine(0)
    finally:
        if old is None:
            os.environ.pop("SSA_MSM_SLICE", None)
        else:
            os.environ["SSA_MSM_SLICE"] = old
    try:
        assert eng.info()["msm_slice"] == 512
        s, p, m = pool.sigs, pool.pks, pool.msgs
        assert raw(eng, [3, 513], s, p, m)[0] == ssa.ERR_ARG                    # an n_j above the slice
        rc, wire, results = raw(eng, [3, 512, 2], s, p, m)
        assert rc == 0 and results.tolist() == [OK] * 3
        assert raw(eng, [3, 2], s, p, m, flags=2)[0] == ssa.ERR_ARG             # an unknown flag bit
        assert raw(eng, [3, 2], s, p, m, flags=ssa.AGG_CHECK | 4)[0] == ssa.ERR_ARG
        assert raw(eng, [3, 2], s, p, m, out=False)[0] == ssa.ERR_ARG           # a null output
        assert raw(eng, [0, 0], s, p, m, out=False)[0] == ssa.ERR_ARG
        assert raw(eng, [], s, p, m)[0] == 0 and raw(eng, [], s, p, m, out=False)[0] == 0     # k = 0
        for flags in (0, ssa.AGG_CHECK):
            rc, wire, results = raw(eng, [0, 0, 0], s, p, m, flags=flags)
            assert rc == 0 and wire.size == 96 and not wire.any() and results.tolist() == [OK] * 3
        # the mirror on the same context, and the outputs a caller may leave out
        got = many(eng, [3, 512, 2], s, p, m)
        assert (got[4] == raw(eng, [3, 512, 2], s, p, m)[1]).all()
        aggs, results, status, nfail = eng.aggregates([])
        assert aggs == [] and results.size == 0 and status.size == 0 and nfail == 0
    finally:
        eng.close()


def test_device_form_only_enqueues_and_runs_the_segmented_fold(pool):
    import torch
    import schnorr_sig_amd as ssa
    sigs = pool.sigs[:N].copy()
    sigs[700, 48] |= 0x01
    eng = ssa.Engine(0)
    try:
        want = many(eng, COUNTS, sigs, pool.pks, pool.msgs)
        d_sigs, d_pks, d_msgs = [torch.from_numpy(np.ascontiguousarray(a[:N])).to("cuda:0") for a in (sigs, pool.pks, pool.msgs)]
        d_aggs = torch.full((49 * N + 32 * len(COUNTS),), 255, dtype=torch.uint8, device="cuda:0")
        d_res = torch.full((len(COUNTS),), 255, dtype=torch.int32, device="cuda:0")
        d_status = torch.full((N,), 255, dtype=torch.uint8, device="cuda:0")
        d_nfail = torch.full((1,), -1, dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()
        eng.enable_timing(True)
        eng.aggregates_device(d_sigs, COUNTS, d_pks, d_msgs, d_aggs=d_aggs, d_results=d_res, d_status=d_status,
                              d_nfail=d_nfail)
        eng.sync()
        launches = {name: eng.read_timing(name)[1] for name in ("ag_k_fold_seg", "ag_k_fold_finish_seg", "ag_k_pack_many",
                                                                 "ag_k_lane_map", "ag_k_fold")}
        eng.enable_timing(False)
        assert launches == {"ag_k_fold_seg": 1, "ag_k_fold_finish_seg": 1, "ag_k_pack_many": 1, "ag_k_lane_map": 1,
                            "ag_k_fold": 0}
        assert d_res.cpu().tolist() == want[1] and int(d_nfail.cpu()[0]) == want[3] == 1
        assert (d_status.cpu().numpy() == want[2]).all() and (d_aggs.cpu().numpy() == want[4]).all()
        # with the check, and the outputs the call allocates itself
        want_c = many(eng, COUNTS, sigs, pool.pks, pool.msgs, check=True)
        d_aggs2, d_res2, d_status2, d_nfail2 = eng.aggregates_device(d_sigs, COUNTS, d_pks, d_msgs, check=True)
        eng.sync()
        assert d_res2.cpu().tolist() == want_c[1] and int(d_nfail2.cpu()[0]) == want_c[3]
        assert (d_status2.cpu().numpy() == want_c[2]).all() and (d_aggs2.cpu().numpy() == want_c[4]).all()
    finally:
        eng.close()
