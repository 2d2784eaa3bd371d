"""The streaming aggregate verifier through the key cache (ssa_aggverifier_push_cached*).  The
contract is section 23's equality: if the first n held lanes were all pushed through a cache,

    finish(e_agg, n) == ssa_verify_aggregates_many_cached(_wire) with k = 1, counts = {n},
                        aggs = R_0 || ... || R_(n-1) || e_agg, on the same keys and messages.

The right-hand side is always computed OUTSIDE the object: Engine.verify_aggregates_cached with k = 1 on a fresh cache
(rhs), V by Engine.verify_aggregate on the unpacked keys U (v_of), the key statuses by a ladder key set and pymodel
(key_statuses, py_key_status of tests/test_gpu_aggregates_cached.py), e_agg by the one-shot Engine.aggregate.  Every
case runs for affine and wire keys and for the host and the device form unless it says otherwise."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from aggregate_model import Q
from test_gpu_aggregates_cached import (BAD_KEY, FORMS, INVALID, MALFORMED, MODES, N, OK, SIGNERS, WANT_KS, WANT_VERDICT, Keys,
                                        dev, gap_case, key_statuses, launches, new_cache, py_key_status, spoil_classes,
                                        world)      # noqa: F401  (world: the fixture)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DISTINCT, HITS, INSERTED, EVICTIONS, BYPASSED, BOUND = range(6)
PUSHES = [1, 510, 1, 1, 0, 513, 3, 255, 4]          # as tests/test_gpu_aggverifier.py: ends on 511, 512, 513, an empty push
TOTAL = sum(PUSHES)                                  # 1288
BOUNDS = list(np.cumsum(PUSHES))                     # 1, 511, 512, 513, 513, 1026, 1029, 1284, 1288
# where a spoiled key is placed: push [513, 1026) holds the block edge 1023 | 1024
PLACES = {"first_lane_of_a_push": 513, "last_lane_of_a_push": 1025, "left_of_a_block_edge": 1023,
          "right_of_a_block_edge": 1024}
CLASSES = {"affine": ["p_plus_t2", "order_2_point", "noncanonical_limb", "identity", "off_curve"],
           "wire": ["p_plus_t2", "order_2_point", "noncanonical_limb", "identity", "bad_flag_bits", "no_square_root"]}
_MINE = {}


def distinct(keys):
    return len(np.unique(keys, axis=0)) if keys.shape[0] else 0


def neg(e):
    v = int.from_bytes(np.asarray(e, np.uint8).tobytes(), "little")
    return np.frombuffer(((Q - v) % Q).to_bytes(32, "little"), np.uint8)


class Body:
    """the lanes of a block body in every form a push takes them, and U for the plain push and the references"""

    def __init__(self, rs, pks, inf, wire, msgs):
        self.rs, self.pks, self.inf, self.wire, self.msgs = (np.ascontiguousarray(a) for a in (rs, pks, inf, wire, msgs))
        self.n = self.rs.shape[0]
        self._keys = {}

    def keys(self, engine, mode):
        if mode not in self._keys:
            self._keys[mode] = Keys(engine, mode, self.pks, self.inf, self.wire)
        return self._keys[mode]

    def agg(self, e, n):
        return np.concatenate([self.rs[:n].reshape(-1), np.asarray(e, np.uint8)])


def world_body(world, lanes, spoil=None, at=()):
    pks, inf, wire = world.pks[lanes].copy(), np.zeros(len(lanes), np.uint8), world.wire[lanes].copy()
    for i in at:
        spoil(pks, inf, wire, i)
    return Body(world.sigs[lanes][:, :49], pks, inf, wire, world.msgs[lanes])


def e_honest(engine, world, lanes, n):
    """e_agg of the honest aggregate over the first n of `lanes` (the one-shot producer), computed once each"""
    lanes = np.asarray(lanes)
    key = ("e", lanes[:n].tobytes())
    if key not in _MINE:
        if n == 0:
            _MINE[key] = np.zeros(32, np.uint8)
        else:
            ix = lanes[:n]
            st, agg, _, nf = engine.aggregate(world.sigs[ix], world.pks[ix], world.msgs[ix])
            assert st == OK and nf == 0
            _MINE[key] = agg[49 * n:].copy()
    return _MINE[key]


def rhs(engine, body, mode, e, n):
    """the right-hand side of the equality: the one-shot cached call with k = 1 on a fresh cache"""
    keys = body.keys(engine, mode)
    with new_cache(engine, mode, capacity=128) as cache:
        v, _ = engine.verify_aggregates_cached(cache, [body.agg(e, n)], keys.arg[:n], body.msgs[:n],
                                               pk_inf=None if keys.inf is None else keys.inf[:n])
    return int(v[0])


def v_of(engine, body, mode, e, n):
    """V: ssa_verify_aggregate on the first n lanes over U"""
    keys = body.keys(engine, mode)
    return int(engine.verify_aggregate(body.agg(e, n), keys.u_pks[:n], body.msgs[:n] if n else None, pk_inf=keys.u_inf[:n]))


class Run:
    """pushes and finishes in one mode and form"""

    def __init__(self, eng, mode, form):
        self.eng, self.mode, self.form = eng, mode, form

    def push(self, av, body, lo, hi, cache):
        """lanes [lo, hi) of the body: plainly (cache None; the keys as U) or through the cache -> stats or None"""
        eng, rs, msgs = self.eng, body.rs[lo:hi], body.msgs[lo:hi]
        if cache is None:
            k = body.keys(eng, self.mode)
            if self.form == "host":
                assert av.push(rs, k.u_pks[lo:hi], msgs, pk_inf=k.u_inf[lo:hi]) == hi - lo
            else:
                d = dev(rs, k.u_pks[lo:hi], msgs, k.u_inf[lo:hi])
                assert av.push_device(d[0], d[1], d[2], d_pk_inf=d[3]) == hi - lo
                eng.sync()
            return None
        if self.mode == "affine":
            if self.form == "host":
                n, st = av.push(rs, body.pks[lo:hi], msgs, pk_inf=body.inf[lo:hi], cache=cache)
            else:
                d = dev(rs, body.pks[lo:hi], msgs, body.inf[lo:hi])
                n, st = av.push_device(d[0], d[1], d[2], d_pk_inf=d[3], cache=cache)
                eng.sync()
        else:
            if self.form == "host":
                n, st = av.push_wire(rs, body.wire[lo:hi], msgs, cache=cache)
            else:
                d = dev(rs, body.wire[lo:hi], msgs)
                n, st = av.push_wire_device(d[0], d[1], d[2], cache=cache)
                eng.sync()
        st = [int(x) for x in st]
        assert n == hi - lo and len(st) == 8 and st[6] == st[7] == 0, st
        assert st[HITS] + st[INSERTED] == st[DISTINCT] or st[BYPASSED], st
        return st

    def push_all(self, av, body, cuts, cache):
        lo, out = 0, []
        for cnt in cuts:
            out.append(self.push(av, body, lo, lo + cnt, cache))
            lo += cnt
        assert lo == body.n
        return out

    def finish(self, av, e, n=None):
        if self.form == "host":
            return av.finish(e, n)
        import torch
        words = torch.full((8,), 0x6EEEEEEE, dtype=torch.int32, device="cuda:0")
        d_e = dev(np.array(e))[0]
        av.finish_device(d_e, words[3:4], n)                              # an odd word offset
        self.eng.sync()
        got = words.cpu().numpy()
        assert (np.delete(got, 3) == 0x6EEEEEEE).all(), got               # its neighbours are untouched
        return int(got[3])


# ------------------------------------------------------------------ the gap the feature closes
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("mode", MODES)
def test_the_gap_is_accepted_by_the_plain_push_and_refused_through_the_cache(engine, world, mode, form):
    """gap_case: five lanes, one signed for P + T2 with a h mod q even -- ssa_verify_aggregate accepts them, and so does
    the verifier under plain pushes.  Through a cache the same body is refused: the guarantee of Signature::verify."""
    aggs, pks, wire, msgs, at = gap_case(engine, world)
    body = Body(aggs[1][:-32].reshape(5, 49), pks[3:8], np.zeros(5, np.uint8), wire[3:8], msgs[3:8])
    e = aggs[1][-32:]
    run = Run(engine, mode, form)
    assert py_key_status(pks[at], 0) == BAD_KEY
    assert v_of(engine, body, mode, e, 5) == OK and rhs(engine, body, mode, e, 5) == BAD_KEY
    with engine.aggregate_verifier(8) as plain, engine.aggregate_verifier(8) as keyed, new_cache(engine, mode) as cache:
        run.push(plain, body, 0, 5, None)
        assert run.finish(plain, e) == OK                                 # the gap
        assert plain.info()["reserved"] == 0
        st = run.push(keyed, body, 0, 5, cache)
        assert run.finish(keyed, e) == BAD_KEY                            # closed
        assert st[DISTINCT] == st[INSERTED] == distinct(body.pks) and keyed.info()["reserved"] == 5 == keyed.cached_lanes()
        # the lanes in front of the key are answered as before
        assert run.finish(keyed, e, at - 3) == v_of(engine, body, mode, e, at - 3)
        assert run.finish(keyed, np.zeros(32, np.uint8), 0) == OK         # the empty aggregate keeps its rule
        assert run.finish(keyed, e, 0) == INVALID


# ------------------------------------------------------------------ the equality per prefix
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("mode", MODES)
def test_honest_pushes_with_a_finish_after_every_push(engine, world, mode, form):
    lanes = np.arange(TOTAL)
    body = world_body(world, lanes)
    run = Run(engine, mode, form)
    with engine.aggregate_verifier(TOTAL) as av, new_cache(engine, mode) as cache:
        lo, seen = 0, 0
        for j, cnt in enumerate(PUSHES):
            st = run.push(av, body, lo, lo + cnt, cache)
            lo += cnt
            seen += st[INSERTED]
            assert st[BYPASSED] == st[BOUND] == st[EVICTIONS] == 0 and st[DISTINCT] == distinct(body.pks[lo - cnt:lo])
            e = e_honest(engine, world, lanes, lo)
            for scalar, want in ((e, OK), (neg(e), INVALID)):
                got = run.finish(av, scalar)
                assert got == want == rhs(engine, body, mode, scalar, lo), (j, lo, got)
            info = av.info()
            assert info["held"] == info["pushed"] == info["reserved"] == lo and info["pushes"] == j + 1
        assert seen == distinct(body.pks) == cache.info()["held"] <= SIGNERS      # every key was checked once


def spoiled_cases(engine, world, mode, cname):
    """per placement: the body, the same body with a malformed R two lanes in front of the key, and the right-hand side
    for every (variant, n_take) -- computed once, outside the object, for both forms"""
    key = ("spoiled", mode, cname)
    if key not in _MINE:
        lanes, out = np.arange(TOTAL), []
        spoil = spoil_classes(engine, mode)[cname]
        for pname, p in PLACES.items():
            good = world_body(world, lanes, spoil, [p])
            rs = good.rs.copy()
            rs[p - 2, 48] |= 0x01
            bad_r = Body(rs, good.pks, good.inf, good.wire, good.msgs)
            keys = good.keys(engine, mode)
            kst = key_statuses(engine, keys)
            assert kst[p] == WANT_KS[cname] == py_key_status(keys.u_pks[p], keys.u_inf[p]), (cname, pname)
            assert int((kst != OK).sum()) == (0 if cname == "identity" else 1)
            takes = sorted({p, p + 1, p + 2, TOTAL} | {int(b) for b in BOUNDS if b > p})
            want = {}
            for n in takes:
                e = e_honest(engine, world, lanes, n)
                for variant, b, scalar in (("honest", good, e), ("negated", good, neg(e)), ("malformed_r", bad_r, e)):
                    v, r = v_of(engine, b, mode, scalar, n), rhs(engine, b, mode, scalar, n)
                    assert r == (BAD_KEY if (kst[:n] == BAD_KEY).any() else v), (cname, pname, variant, n)
                    # what the classes mean: in front of the key V; from the key on the key decides
                    if n <= p:
                        assert r == {"honest": OK, "negated": INVALID, "malformed_r": MALFORMED}[variant]
                    elif WANT_KS[cname] != OK:
                        assert r == WANT_VERDICT[cname], (cname, pname, variant, n)
                    want[(variant, n)] = r
            out.append((pname, p, good, bad_r, takes, want))
        _MINE[key] = out
    return _MINE[key]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("mode,cname", [(m, c) for m in MODES for c in CLASSES[m]])
def test_the_equality_for_every_class_of_key_at_every_edge(engine, world, mode, form, cname):
    """one spoiled key per case; with it a negated e_agg and a malformed R in front of it: the key decides"""
    assert sorted(spoil_classes(engine, mode)) == sorted(CLASSES[mode])
    run = Run(engine, mode, form)
    lanes = np.arange(TOTAL)
    with new_cache(engine, mode) as cache:
        for pname, p, good, bad_r, takes, want in spoiled_cases(engine, world, mode, cname):
            with engine.aggregate_verifier(TOTAL) as av, engine.aggregate_verifier(TOTAL) as av_r:
                run.push_all(av, good, PUSHES, cache)
                run.push_all(av_r, bad_r, PUSHES, cache)
                for n in takes:
                    e = e_honest(engine, world, lanes, n)
                    for variant, obj, scalar in (("honest", av, e), ("negated", av, neg(e)), ("malformed_r", av_r, e)):
                        got = run.finish(obj, scalar, n)
                        assert got == want[(variant, n)], (cname, pname, variant, n, got)
                assert av.info()["reserved"] == TOTAL


# ------------------------------------------------------------------ the fold's edges
def fold_world(engine, world):
    import schnorr_sig_amd as ssa
    span = ssa.aggverifier_key_span()
    total = 2 * span + 17
    assert span % 4096 == 0 and total <= 20000
    lanes = np.arange(total) % N                         # (the world's lanes, taken round again)
    places = {"lane_0": 0, "lane_15": 15, "lane_16": 16, "last_lane": total - 1, "span_minus_1": span - 1, "span": span,
              "two_spans_minus_1": 2 * span - 1, "two_spans": 2 * span, "ragged_tail": 2 * span + 9}
    return span, total, lanes, places


def fold_takes(p, total):
    """p, p + 1, p + 2, all, and on either side of the key the nearest n with n % 16 in {0, 1, 15}"""
    takes = {p, p + 1, p + 2, total}
    for r in (0, 1, 15):
        takes.add(p - (p - r) % 16)                      # the largest n <= p with n % 16 == r: the key is not taken
        takes.add(p + 1 + (r - p - 1) % 16)              # the smallest n >= p + 1 with n % 16 == r: it is
    return sorted(n for n in takes if 0 <= n <= total)


def fold_case(engine, world, mode, pname):
    key = ("fold", mode, pname)
    if key not in _MINE:
        span, total, lanes, places = fold_world(engine, world)
        p = places[pname]
        body = world_body(world, lanes, spoil_classes(engine, mode)["p_plus_t2"], [p])
        takes = fold_takes(p, total)
        assert {n % 16 for n in takes} >= {0, 1, 15}
        want = {}
        for n in takes:
            want[n] = rhs(engine, body, mode, e_honest(engine, world, lanes, n), n)
            assert want[n] == (BAD_KEY if n > p else OK), (pname, n, want[n])
        _MINE[key] = (body, takes, want)
    return _MINE[key]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("pname", ["lane_0", "lane_15", "lane_16", "last_lane", "span_minus_1", "span", "two_spans_minus_1",
                                   "two_spans", "ragged_tail"])
def test_the_fold_at_its_edges(engine, world, mode, form, pname):
    """2 * AGV_KST_SPAN + 17 lanes in one keyed object: three workgroups of agv_k_key_verdict, the last with a ragged tail.
    P + T2 where a fold can lose a byte, finished at prefixes on both sides of it and at every 16-byte phase; then all
    of it again with the context's workspaces poisoned with byte 1 ("bad key"): kst is the object's own."""
    span, total, lanes, places = fold_world(engine, world)
    body, takes, want = fold_case(engine, world, mode, pname)
    cuts = [span + 5, 17, total - span - 22] if places[pname] % 2 == 0 else [total - 100, 100]
    run = Run(engine, mode, form)
    with engine.aggregate_verifier(total) as av, new_cache(engine, mode) as cache:
        run.push_all(av, body, cuts, cache)
        assert av.info()["reserved"] == av.info()["held"] == total
        for poison in (None, 0x01):
            for n in takes:
                if poison is not None:
                    engine.debug_poison_workspaces(poison)
                got = run.finish(av, e_honest(engine, world, lanes, n), n)
                assert got == want[n], (pname, poison, n, got)


# ------------------------------------------------------------------ mixed pushes and reset
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("mode", MODES)
def test_plain_and_cached_pushes_mixed_and_reset(engine, world, mode, form):
    lanes = np.arange(600)
    a, b = 100, 300                                      # the same key P + T2 in a plain push and in a cached one
    body = world_body(world, lanes, spoil_classes(engine, mode)["p_plus_t2"], [a, b])
    run = Run(engine, mode, form)
    e = lambda n: e_honest(engine, world, lanes, n)      # noqa: E731
    with engine.aggregate_verifier(600) as av, new_cache(engine, mode) as cache:
        run.push(av, body, 0, 200, None)
        run.push(av, body, 200, 400, cache)
        run.push(av, body, 400, 600, None)
        assert av.info()["reserved"] == 200 and av.info()["pushed"] == 600
        for n in (a, a + 1, 200, b, b + 1, 400, 600):
            v = v_of(engine, body, mode, e(n), n)
            assert v == (OK if n <= a else INVALID)
            # the plain-pushed lane does not refuse; the cached one does
            assert run.finish(av, e(n), n) == (BAD_KEY if n > b else v), n
        # after reset and plain pushes only, the object answers as a fresh one
        av.reset()
        assert av.info() == dict(held=0, capacity=600, block_lanes=512, pushes=0, pushed=0, reserved=0, blocks=0, finishes=0)
        run.push(av, body, 0, 600, None)
        with engine.aggregate_verifier(600) as fresh:
            run.push(fresh, body, 0, 600, None)
            for n in (b, b + 1, 600):
                assert run.finish(av, e(n), n) == run.finish(fresh, e(n), n) == v_of(engine, body, mode, e(n), n)
        assert av.info()["reserved"] == 0
        # a cached push that comes first after plain ones zeroes the old bytes: a bad key through the cache, reset, as many
        # good lanes plainly, one good lane through the cache
        av.reset()
        run.push(av, body, 200, 400, cache)
        assert run.finish(av, e(0), 200) == BAD_KEY
        av.reset()
        order = np.concatenate([np.arange(400, 600), [0]])
        good = world_body(world, order)
        run.push(av, good, 0, 200, None)
        run.push(av, good, 200, 201, cache)
        assert av.info()["reserved"] == 1
        assert run.finish(av, e_honest(engine, world, order, 201)) == OK
        assert run.finish(av, e_honest(engine, world, order, 200), 200) == OK


# ------------------------------------------------------------------ cache states
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("mode", MODES)
def test_cold_then_warm_builds_and_decompresses_nothing_twice(engine, world, mode, form):
    import schnorr_sig_amd as ssa
    lanes = np.arange(TOTAL)
    p = PLACES["first_lane_of_a_push"]
    body = world_body(world, lanes, spoil_classes(engine, mode)["p_plus_t2"], [p])
    e_all, e_p = e_honest(engine, world, lanes, TOTAL), e_honest(engine, world, lanes, p)
    assert rhs(engine, body, mode, e_all, TOTAL) == BAD_KEY and rhs(engine, body, mode, e_p, p) == OK
    u = distinct(body.pks)                               # the bad key is a key like any other
    assert SIGNERS - 2 <= u <= SIGNERS + 1
    eng = ssa.Engine(0)
    run = Run(eng, mode, form)
    names = ("ssa_k_keyset_build", "ssa_k_keyed_decompress", "agc_expand", "agv_k_key_verdict", "agc_k_key_verdicts")
    try:
        with new_cache(eng, mode) as cache, eng.aggregate_verifier(TOTAL) as cold, eng.aggregate_verifier(TOTAL) as warm:
            eng.enable_timing(True)
            for name in names:
                eng.read_timing(name)                    # drains the key
            st = run.push(cold, body, 0, TOTAL, cache)
            assert st[:6] == [u, 0, u, 0, 0, 0] and cache.info()["held"] == u
            assert launches(eng, "ssa_k_keyset_build") == 1
            assert launches(eng, "ssa_k_keyed_decompress") == (1 if mode == "wire" else 0)
            assert launches(eng, "agc_expand") == 1
            st = run.push(warm, body, 0, TOTAL, cache)
            assert st[:6] == [u, u, 0, 0, 0, 0] and cache.info()["held"] == u
            assert launches(eng, "ssa_k_keyset_build") == 0 and launches(eng, "ssa_k_keyed_decompress") == 0
            assert launches(eng, "agc_expand") == 1
            for av in (cold, warm):
                assert run.finish(av, e_all) == BAD_KEY and run.finish(av, e_p, p) == OK
                assert run.finish(av, np.zeros(32, np.uint8), 0) == OK   # no lane: no fold
                assert av.info()["reserved"] == TOTAL
            assert launches(eng, "agv_k_key_verdict") == 4 and launches(eng, "agc_k_key_verdicts") == 0
            eng.enable_timing(False)
            # cleared between two pushes of one object: cold again, the same verdicts
            with eng.aggregate_verifier(TOTAL) as av:
                run.push(av, body, 0, 600, cache)
                cache.clear()
                st = run.push(av, body, 600, TOTAL, cache)
                assert st[HITS] == 0 and st[INSERTED] == st[DISTINCT]
                assert run.finish(av, e_all) == BAD_KEY and run.finish(av, e_p, p) == OK
    finally:
        eng.close()


_CHILD = r"""
import json, os, sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, os.path.join(%(root)r, "oracle"))
sys.path.insert(0, os.path.join(%(root)r, "tests"))
import numpy as np
import torch
import schnorr_sig_amd as ssa
from test_gpu_screened_torsion import special_key_lanes
rng = np.random.default_rng(29801)
n, per = 12345, 40
takes = [4999, 5000, 5001, 9999, 10000, 10001, n]
e = ssa.Engine(0)
def sc(k):
    v = rng.integers(0, 256, size=(k, 32), dtype=np.uint8); v[:, 31] &= 0x3f; v[:, 0] |= 1
    return v
# slice-disjoint key sets: lanes [0, 5000) by signers 0..39, [5000, 10000) by 40..79, the rest by 80..119
idx = np.concatenate([s * per + np.resize(np.arange(per), c) for s, c in enumerate((5000, 5000, 2345))])
m = rng.integers(0, 256, size=(n, 80), dtype=np.uint8)
pk, sg = e.keygen_sign_many(sc(3 * per)[idx], sc(n), m)
rs = np.ascontiguousarray(sg[:, :49])
es = {}
for t in takes:
    st, a, _, _ = e.aggregate(sg[:t], pk[:t], m[:t])
    assert st == 0
    es[t] = a[49 * t:].copy()
out = {"lane_slice": e.info()["lane_slice"], "cases": []}
os.environ["SSA_LANE_SLICE"] = str(1 << 20)
one = ssa.Engine(0)                                      # the reference: one slice, a cache that never fills
assert one.info()["lane_slice"] == 1 << 20
dev = torch.device("cuda", 0)
for side, lanes in (("left", (4999, 9999)), ("right", (5000, 10000)), ("none", ())):
    p = pk.copy()
    for i in lanes:
        p[i] = special_key_lanes(rng, 1, True)[0]
    w, st = e.compress_many(p)
    assert (st == 0).all()
    for mode, keys in (("affine", p), ("wire", w)):
        ref = []
        for t in takes:
            with one.keycache_create(4096, wire=(mode == "wire")) as big:
                agg = np.concatenate([rs[:t].reshape(-1), es[t]])
                ref.append(int(one.verify_aggregates_cached(big, [agg], keys[:t], m[:t])[0][0]))
        for evict, rows in (("clear", 64), ("recent", 64), ("bypass", 8)):
            for form in ("host", "device"):
                kc = e.keycache_create(rows, wire=(mode == "wire"), evict="clear" if evict == "bypass" else evict)
                av = e.aggregate_verifier(n)
                if form == "host":
                    cnt, stats = av.push(rs, keys, m, cache=kc) if mode == "affine" else av.push_wire(rs, keys, m, cache=kc)
                else:
                    drs, dk, dm = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (rs, keys, m))
                    torch.cuda.synchronize()
                    cnt, stats = (av.push_device(drs, dk, dm, cache=kc) if mode == "affine"
                                  else av.push_wire_device(drs, dk, dm, cache=kc))
                    e.sync()
                assert cnt == n
                v = [int(av.finish(es[t], t)) for t in takes]
                out["cases"].append({"side": side, "mode": mode, "evict": evict, "form": form, "v": v, "ref": ref,
                                     "stats": [int(x) for x in stats], "held": kc.info()["held"],
                                     "clears": kc.info()["clears"], "compactions": kc.eviction_info()["compactions"],
                                     "cached": av.info()["reserved"]})
                av.close()
                kc.close()
print("RESULT " + json.dumps(out))
e.close(); one.close()
"""


def test_one_push_of_three_cache_slices_eviction_and_bypass_in_a_child_process():
    """SSA_LANE_SLICE = 5000 in a fresh child process: ONE push of 12 345 lanes is three slices of the cache with
    disjoint key sets (40 signers each).  A cache of 64 rows is cleared (evict="clear") or compacted (evict="recent")
    by the second and third slice, under the rows the first left -- after agc_k_expand moved their statuses into the
    object; a cache of 8 rows is bypassed by every slice.  A key outside the subgroup on the left or on the right of both
    slice edges; the verdicts of seven prefixes are those of a one-slice engine's one-shot call on a large fresh cache."""
    env = dict(os.environ)
    env["SSA_LANE_SLICE"] = "5000"
    r = subprocess.run([sys.executable, "-c", _CHILD % {"root": ROOT}], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    assert out["lane_slice"] == 5000
    assert len(out["cases"]) == 3 * 2 * 3 * 2
    takes = [4999, 5000, 5001, 9999, 10000, 10001, 12345]
    for c in out["cases"]:
        first_bad = {"left": 4999, "right": 5000, "none": 1 << 30}[c["side"]]
        want = [BAD_KEY if t > first_bad else OK for t in takes]
        assert c["v"] == c["ref"] == want, c
        bad = 0 if c["side"] == "none" else 2
        s = c["stats"]
        assert s[DISTINCT] == 120 + bad and s[BOUND] == 0 and s[6] == s[7] == 0 and c["cached"] == 12345, c
        if c["evict"] == "bypass":
            assert s[BYPASSED] == 3 and s[HITS] == s[INSERTED] == s[EVICTIONS] == 0, c
            assert c["held"] == 0 and c["clears"] == 0, c
            continue
        assert s[BYPASSED] == 0 and s[HITS] + s[INSERTED] == s[DISTINCT], c
        assert s[EVICTIONS] == 2 and s[HITS] == 0, c            # nothing of an earlier slice returns
        if c["evict"] == "clear":
            assert c["clears"] == 2 and c["compactions"] == 0, c
        else:
            assert c["clears"] + c["compactions"] == 2, c
        assert 40 <= c["held"] <= 64, c


# ------------------------------------------------------------------ refusals
def test_refusals_change_nothing(engine, world):
    import ctypes as C
    import schnorr_sig_amd as ssa
    lib = ssa._lib
    body = world_body(world, np.arange(12))
    rs, pks, w49, msgs = (np.ascontiguousarray(a[4:]) for a in (body.rs, body.pks, body.wire, body.msgs))
    d_rs, d_pks, d_w49, d_msgs = dev(rs, pks, w49, msgs)
    p = lambda a: C.c_void_p(a.ctypes.data)      # noqa: E731
    dp = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    stats = np.full(8, 9, np.uint64)
    sp = stats.ctypes.data
    other, gone = ssa.Engine(0), ssa.Engine(0)
    orphans = [new_cache(gone, "affine"), new_cache(gone, "wire")]
    gone.close()                                         # the context goes first: its caches are orphaned
    try:
        with new_cache(engine, "affine") as ca, new_cache(engine, "wire") as cw, new_cache(other, "affine") as co, \
                new_cache(other, "wire") as cow, engine.aggregate_verifier(10) as av:
            ctx, h = engine._ctx, av.handle
            assert av.push(body.rs[:4], body.pks[:4], body.msgs[:4], cache=ca)[0] == 4
            assert av.push_wire(body.rs[:0], body.wire[:0], body.msgs[:0], cache=cw)[1].tolist() == [0] * 8   # n = 0: a push
            info, rec = av.info(), av.record()
            assert info["held"] == 4 and info["pushes"] == 2 and info["reserved"] == 4
            cinfo = [c.info() for c in (ca, cw, co, cow)]
            assert cinfo[0]["held"] == distinct(body.pks[:4]) and cinfo[1]["held"] == 0      # the empty push touched no cache

            def affine(kc, n=2, c=ctx):
                return [lib.ssa_aggverifier_push_cached(c, h, kc, p(rs), p(pks), None, p(msgs), None, 80, 80, n, sp),
                        lib.ssa_aggverifier_push_cached_device(c, h, kc, dp(d_rs), dp(d_pks), None, dp(d_msgs), None, 80, 80,
                                                               n, sp)]

            def wire(kc, n=2, c=ctx):
                return [lib.ssa_aggverifier_push_cached_wire(c, h, kc, p(rs), p(w49), p(msgs), None, 80, 80, n, sp),
                        lib.ssa_aggverifier_push_cached_wire_device(c, h, kc, dp(d_rs), dp(d_w49), dp(d_msgs), None, 80, 80,
                                                                    n, sp)]
            refused = [ssa.ERR_ARG, ssa.ERR_ARG]
            assert affine(cw.handle) == refused and wire(ca.handle) == refused          # the other mode
            assert affine(co.handle) == refused and wire(cow.handle) == refused         # another context's cache
            assert affine(None) == refused and wire(None) == refused                    # none
            assert affine(orphans[0].handle) == refused and wire(orphans[1].handle) == refused
            assert affine(ca.handle, 7) == refused and wire(cw.handle, 7) == refused    # n > capacity - held
            assert affine(co.handle, 2, other._ctx) == refused                          # a context other than the object's
            assert stats.tolist() == [9] * 8                                            # a refused call writes nothing
            assert av.info() == info and [c.info() for c in (ca, cw, co, cow)] == cinfo
            assert (av.record() == rec).all()
            # and the object still takes what fits
            assert affine(ca.handle, 6)[0] == 0 and av.info()["held"] == 10 and stats[6] == stats[7] == 0
            assert av.finish(e_honest(engine, world, np.arange(12), 10)) == OK
    finally:
        for c in orphans:
            c.close()
        other.close()


# ------------------------------------------------------------------ hygiene
@pytest.mark.parametrize("mode", MODES)
def test_the_record_of_a_keyed_object_is_the_record_of_a_plain_one(engine, world, mode):
    """the key status never enters the MSM"""
    body = world_body(world, np.arange(TOTAL), spoil_classes(engine, mode)["p_plus_t2"], [PLACES["left_of_a_block_edge"]])
    run = Run(engine, mode, "host")
    with engine.aggregate_verifier(TOTAL) as plain, engine.aggregate_verifier(TOTAL) as keyed, new_cache(engine, mode) as cache:
        run.push_all(plain, body, PUSHES, None)
        run.push_all(keyed, body, PUSHES, cache)
        for n in (TOTAL, 1025, 1024, 1023, 513, 512, 1):
            assert (plain.record(n) == keyed.record(n)).all(), n


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("mode", MODES)
def test_two_verifiers_share_one_cache(engine, world, mode, form):
    lanes_a, lanes_b = np.arange(TOTAL), np.arange(100, 100 + TOTAL)
    p = PLACES["last_lane_of_a_push"]
    body_a = world_body(world, lanes_a, spoil_classes(engine, mode)["p_plus_t2"], [p])
    body_b = world_body(world, lanes_b)
    run = Run(engine, mode, form)
    with engine.aggregate_verifier(TOTAL) as a, engine.aggregate_verifier(TOTAL) as b, new_cache(engine, mode) as cache:
        la = lb = 0
        for j, cnt in enumerate(PUSHES):
            run.push(a, body_a, la, la + cnt, cache)
            la += cnt
            engine.debug_poison_workspaces(0x01)
            run.push(b, body_b, lb, lb + PUSHES[-1 - j], cache)
            lb += PUSHES[-1 - j]
            assert run.finish(a, e_honest(engine, world, lanes_a, la)) == (BAD_KEY if la > p else OK), j
        assert run.finish(b, e_honest(engine, world, lanes_b, TOTAL)) == OK
        assert run.finish(b, e_honest(engine, world, lanes_a, TOTAL)) == INVALID
        assert run.finish(a, e_honest(engine, world, lanes_a, p), p) == OK
        assert cache.info()["held"] == distinct(np.concatenate([body_a.pks, body_b.pks]))


@pytest.mark.parametrize("form", FORMS)
def test_what_the_cached_producer_emits_is_accepted_through_the_same_cache(engine, world, form):
    """ssa_aggregate_valid_keyed_many_cached over 130-byte records, then its aggregate and kept keys pushed through the
    same wire cache: every key is found, and the verdict is SSA_OK.  (4000 lanes, the world's taken round again: above
    SSA_MSM_SMALL_MAX, where the producer's screen goes through the cache.)"""
    n = 4000
    lanes = np.arange(n) % N
    keyed = np.ascontiguousarray(np.concatenate([world.wire[lanes], world.sigs[lanes]], axis=1))
    run = Run(engine, "wire", form)
    with new_cache(engine, "wire") as cache, engine.aggregate_verifier(n) as av:
        agg, kept, status, keys49, _ = engine.aggregate_valid_keyed_cached(cache, keyed, world.msgs[lanes])
        assert kept.tolist() == list(range(n)) and not status.any()
        assert cache.info()["held"] == distinct(world.wire[lanes])
        body = Body(agg[:-32].reshape(n, 49), world.pks[lanes], np.zeros(n, np.uint8), keys49, world.msgs[lanes])
        st = run.push(av, body, 0, n, cache)
        assert st[HITS] == st[DISTINCT] == distinct(body.wire) and st[INSERTED] == 0
        assert run.finish(av, agg[-32:]) == OK
