"""The streaming aggregator through the key cache, and its key column (ssa_aggregator_push_cached,
ssa_aggregator_push_keyed_cached, SSA_AGGR_HOLD_KEYS49, ssa_aggregator_keys).  Two equalities:

  the admission   status, kept count, the 12 statistics words and the cache's state afterwards are those of the one-shot
                  call (Engine.aggregate_valid_cached / aggregate_valid_keyed_cached) on this batch alone and a second
                  cache in the same prior state;
  the object      every finish(n) is Engine.aggregate on the first n admitted lanes handed in alone, and keys(n) the
                  first 49 bytes of their records -- after pushes of any kind, front drops, masks and takes.

Expected values come from those calls and from numpy indexing of the caller's arrays, never from an aggregator.  The bad
lanes are those of tests/test_gpu_aggregate_valid_cached.py: their statuses are deterministic.

"affine" pushes affine keys through an affine cache, "wire" 130-byte records through a wire cache."""
import ctypes as C
import os

import numpy as np
import pytest

from test_gpu_aggregate_valid_cached import BAD_KEY, FORMS, INVALID, MODES, Case, Honest, dev, even_t2_lane, spoiled_case
from test_gpu_aggregates_cached import new_cache, spoil_classes
from test_gpu_aggregator import PUSHES

pytestmark = pytest.mark.gpu

OK = 0
BIG = 3200                                           # just above the default small-batch bound of 3072: the cache is used
SEQ = PUSHES[:7] + [BIG] + PUSHES[7:]                # ends on 511, 512, 513 held lanes, crosses two blocks, an empty push
FIRST = sum(PUSHES[:7])                              # the first lane of the push of BIG
TOTAL = sum(SEQ)
EXTRA = 300                                          # one more push behind every removal
LOAD = [513, 511, 264]                               # the pushes of the removal tests: 1288 lanes
HELD = sum(LOAD)
BASE = FIRST + 100                                   # ... on honest lanes of the pool, from this one on
EDGES = [0, 1, 2, 3, 63, 64, 65, 511, 512, 513, 1023, 1024, 1025, 1287, 1288, 1289, 4095, 4096, 4097]
_STATE = {}


# ------------------------------------------------------------------ batches
class Batch:
    """lanes in both key forms; [lo:hi] or an index array gives the lanes alone"""

    def __init__(self, sigs, pks, inf, wire, msgs):
        self.sigs, self.pks, self.inf, self.wire, self.msgs = sigs, pks, inf, wire, msgs
        self.n = sigs.shape[0]

    def __getitem__(self, s):
        return Batch(*(np.ascontiguousarray(a[s]) for a in (self.sigs, self.pks, self.inf, self.wire, self.msgs)))

    @property
    def rec(self):
        return np.ascontiguousarray(np.concatenate([self.wire, self.sigs], axis=1))


def of_case(c):
    return Batch(c.sigs, c.pks, c.inf, c.wire, c.msgs)


def pool(engine):
    """TOTAL + EXTRA honest lanes by 40 repeating signers; in the push of BIG a lane under P + T2, a bad signature and a lane
    with both (the key decides)"""
    if "pool" not in _STATE:
        c = Case(Honest(engine, TOTAL + EXTRA, seed=0x31A6))
        t2 = spoil_classes(engine, "affine")["p_plus_t2"]
        t2(c.pks, c.inf, c.wire, FIRST + 5)
        c.sigs[FIRST + 64, 49] ^= 1
        t2(c.pks, c.inf, c.wire, FIRST + BIG - 1)
        c.sigs[FIRST + BIG - 1, 49] ^= 1
        c.want[[FIRST + 5, FIRST + BIG - 1]] = BAD_KEY
        c.want[FIRST + 64] = INVALID
        _STATE["pool"] = (of_case(c), c.want.copy())
    return _STATE["pool"]


def honest_lanes(engine):
    """HELD + EXTRA honest lanes of the pool"""
    if "honest lanes" not in _STATE:
        b, want = pool(engine)
        assert not want[BASE:BASE + HELD + EXTRA].any()
        _STATE["honest lanes"] = b[BASE:BASE + HELD + EXTRA]
    return _STATE["honest lanes"]


def ref(engine, b, idx):
    """Engine.aggregate of the lanes idx of b handed in alone, computed once each and never changed"""
    idx = np.asarray(idx, dtype=np.int64)
    key = (id(b), idx.tobytes())
    if key not in _STATE:
        if idx.size == 0:
            agg = np.zeros(32, np.uint8)
        else:
            st, agg, _, nf = engine.aggregate(b.sigs[idx], b.pks[idx], b.msgs[idx], pk_inf=b.inf[idx])
            assert st == OK and nf == 0
        agg.setflags(write=False)
        _STATE[key] = (b, agg)                       # (b: keeps the id alive)
    return _STATE[key][1]


def one_shot(eng, cache, mode, b):
    """the call the admission is defined by -> (status, kept count, stats)"""
    if mode == "affine":
        out = eng.aggregate_valid_cached(cache, b.sigs, b.pks, b.msgs, pk_inf=b.inf)
    else:
        out = eng.aggregate_valid_keyed_cached(cache, b.rec, b.msgs)
    return out[2], int(out[1].size), [int(x) for x in out[-1]]


def push(ag, cache, mode, b, form="host"):
    """the push under test -> (status, kept count, stats)"""
    import torch
    if form == "host":
        st, m, stats = ag.push(b.sigs, b.pks, b.msgs, pk_inf=b.inf, cache=cache) if mode == "affine" else \
            ag.push_keyed(cache, b.rec, b.msgs)
    else:
        d_st = torch.full((max(b.n, 1),), 0xEE, dtype=torch.uint8, device="cuda:0")
        if mode == "affine":
            ds, dk, di, dm = dev(b.sigs, b.pks, b.inf, b.msgs)
            m, stats = ag.push_cached_device(cache, ds, dk, dm, d_status=d_st, d_pk_inf=di)
        else:
            dr, dm = dev(b.rec, b.msgs)
            m, stats = ag.push_keyed_device(cache, dr, dm, d_status=d_st)
        ag.engine.sync()
        st = d_st.cpu().numpy()[:b.n]
    return st, m, [int(x) for x in stats]


def prefixes(held):
    return [n for n in EDGES if n < held] + [held]


# ------------------------------------------------------------------ the admission
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("mode", MODES)
def test_admission_equals_the_one_shot_call_cold_and_warm(engine, mode, form):
    key = ("spoiled", mode)
    if key not in _STATE:
        cname, spoil = list(spoil_classes(engine, mode).items())[0]
        _STATE[key] = spoiled_case(engine, Honest(engine, BIG), cname, spoil, 0)
    c = _STATE[key]
    b = of_case(c)
    K = np.flatnonzero(c.want == 0)
    with new_cache(engine, mode) as cache, new_cache(engine, mode) as twin, engine.aggregator(2 * BIG + 300) as ag:
        for state in ("cold", "warm"):
            want = one_shot(engine, twin, mode, b)
            assert (want[0] == c.want).all() and want[2][5] == 1            # one screened slice: the cache is used
            got = push(ag, cache, mode, b, form)
            assert (got[0] == want[0]).all() and got[1:] == want[1:], (state, got[1:], want[1:])
            assert cache.info() == twin.info() and cache.info()["held"] > 0
            assert got[2][9] == (got[2][0] if state == "cold" else 0)       # inserted cold, found warm
        assert (ag.finish_bytes() == ref(engine, b, np.concatenate([K, K]))).all()
        # at most the small-batch bound: the exact path, the cache is not used
        small = b[:300]
        held = cache.info()
        want = one_shot(engine, twin, mode, small)
        got = push(ag, cache, mode, small, form)
        assert (got[0] == want[0]).all() and got[1:] == want[1:] and (want[2][5], want[2][6]) == (0, 1)
        assert cache.info() == twin.info() == held
        info = ag.info()
        assert (info["held"], info["pushes"], info["offered"]) == (2 * K.size + got[1], 3, 2 * BIG + 300)
        assert info["dropped"] == info["offered"] - info["held"]
    # a cache with fewer rows than the batch has distinct keys: whatever the one-shot call does with it, the push does
    with new_cache(engine, mode, 16) as cache, new_cache(engine, mode, 16) as twin, engine.aggregator(BIG) as ag:
        for state in ("cold", "again"):
            want = one_shot(engine, twin, mode, b)
            got = push(ag, cache, mode, b, form)
            assert (got[0] == want[0]).all() and (got[0] == c.want).all() and got[1:] == want[1:], (state, got[1:], want[1:])
            assert cache.info() == twin.info() and cache.eviction_info() == twin.eviction_info()
            assert (ag.finish_bytes() == ref(engine, b, K)).all()
            ag.reset()


@pytest.fixture(scope="module")
def sliced():
    """a context whose lane slice is 1024 lanes and whose small-batch bound is 500"""
    import schnorr_sig_amd as ssa
    old = {k: os.environ.get(k) for k in ("SSA_LANE_SLICE", "SSA_MSM_SMALL_MAX")}
    os.environ["SSA_LANE_SLICE"], os.environ["SSA_MSM_SMALL_MAX"] = "1024", "500"
    try:
        eng = ssa.Engine(0)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
    assert eng.info()["lane_slice"] == 1024
    yield eng
    eng.close()


@pytest.mark.parametrize("mode", MODES)
def test_a_cache_cleared_compacted_or_bypassed_between_the_slices_of_a_push(engine, sliced, mode):
    """2 500 lanes in slices of 1024, 1024 and 452 (the last on the exact path) with disjoint sets of 40 signers: a cache
    of 64 rows is cleared or compacted by the second slice, one of 8 rows is bypassed; a dropped lane on either side of
    each slice edge"""
    from test_gpu_screened_torsion import make_scalars
    key = "sliced batch"
    if key not in _STATE:
        rng = np.random.default_rng(0x511CE)
        n, per = 2500, 40
        idx = np.concatenate([s * per + np.resize(np.arange(per), c) for s, c in enumerate((1024, 1024, 452))])
        m = rng.integers(0, 256, size=(n, 80), dtype=np.uint8)
        pk, sg = engine.keygen_sign_many(make_scalars(rng, 3 * per)[idx], make_scalars(rng, n), m)
        w, st = engine.compress_many(pk)
        assert (np.asarray(st) == 0).all()
        w, inf = np.asarray(w, np.uint8).reshape(-1, 49).copy(), np.zeros(n, np.uint8)
        for i in (1023, 1024, 2047):
            spoil_classes(engine, "affine")["p_plus_t2"](pk, inf, w, i)
        sg[2048, 49] ^= 1
        _STATE[key] = Batch(sg, pk, inf, w, m)
    b = _STATE[key]
    dropped = [1023, 1024, 2047, 2048]
    K = np.setdiff1d(np.arange(b.n), dropped)
    for evict, cap, form in (("clear", 64, "host"), ("recent", 64, "device"), ("clear", 8, "host")):
        with new_cache(sliced, mode, cap, evict) as cache, new_cache(sliced, mode, cap, evict) as twin, \
                sliced.aggregator(b.n) as ag:
            want = one_shot(sliced, twin, mode, b)
            got = push(ag, cache, mode, b, form)
            assert np.flatnonzero(want[0]).tolist() == dropped
            assert (got[0] == want[0]).all() and got[1:] == want[1:], (evict, cap, got[1:], want[1:])
            assert cache.info() == twin.info() and cache.eviction_info() == twin.eviction_info()
            s = got[2]
            assert s[5] == 2 and s[6] == 1                   # two screened slices, one exact
            assert (s[11] == 2 and cache.info()["held"] == 0) if cap == 8 else (s[11] == 0 and s[10] == 1), s
            assert (ag.finish_bytes() == ref(engine, b, K)).all()


# ------------------------------------------------------------------ the key decides
@pytest.mark.parametrize("mode", MODES)
def test_a_key_outside_the_subgroup_is_admitted_by_the_plain_push_and_dropped_by_the_cached_ones(engine, mode):
    """A lane under P + T2 with an even challenge passes verify_batch: the plain push holds it, and every validator
    refuses the block.  The cached pushes give it SSA_INVALID_PUBLIC_KEY and drop it.  (Fails without the feature.)"""
    pkb, w49, sig, msg = even_t2_lane(engine, lambda s, p, m: engine.verify_many(s, p, m, check_torsion=False)[0])
    c, at = Case(Honest(engine, 5)), 2
    c.pks[at], c.wire[at], c.sigs[at], c.msgs[at] = pkb, w49, sig, msg
    b = of_case(c)
    others = np.setdiff1d(np.arange(5), [at])
    with new_cache(engine, mode) as cache, engine.aggregator(16) as plain, engine.aggregator(16) as ag:
        st, kept = plain.push(b.sigs, b.pks, b.msgs, pk_inf=b.inf)
        assert kept == 5 and not st.any()
        st, kept, _ = push(ag, cache, mode, b)
        assert kept == 4 and st.tolist() == [OK, OK, BAD_KEY, OK, OK]
        assert (ag.finish_bytes() == ref(engine, b, others)).all()
        assert ag.info()["dropped"] == 1


# ------------------------------------------------------------------ the object
def run_sequence(engine, kind, B):
    """SEQ pushed onto one object; after every push, prefixes around each block edge against Engine.aggregate on the
    admitted lanes.  kind: "affine" / "wire" (cached pushes of one kind; "wire" on an object with a key column), or
    "mixed" (plain, affine and keyed pushes in turn on an object made with flags 0)"""
    b, want_status = pool(engine)
    with new_cache(engine, "affine") as ca, new_cache(engine, "wire") as cw, new_cache(engine, "affine") as ta, \
            new_cache(engine, "wire") as tw, engine.aggregator(TOTAL, B, hold_keys=(kind == "wire")) as ag:
        K, lo, held_mod4 = np.zeros(0, np.int64), 0, set()
        for i, cnt in enumerate(SEQ):
            how = kind if kind != "mixed" else ("plain", "affine", "wire")[i % 3]
            sl = b[lo:lo + cnt]
            held_mod4.add(K.size % 4)
            old = None
            if kind == "wire" and K.size:
                old = ag.keys(K.size)
            if how == "plain":
                assert cnt != BIG
                st, m = ag.push(sl.sigs, sl.pks, sl.msgs, pk_inf=sl.inf)
                assert not st.any()
            else:
                cache, twin = (ca, ta) if how == "affine" else (cw, tw)
                st, m, stats = push(ag, cache, how, sl)
                want = one_shot(engine, twin, how, sl) if cnt else (np.zeros(0, np.uint8), 0, [0] * 12)
                assert (st == want[0]).all() and (m, stats) == want[1:] and cache.info() == twin.info()
                assert (st == want_status[lo:lo + cnt]).all()
            K = np.concatenate([K, lo + np.flatnonzero(st == 0)])
            lo += cnt
            info = ag.info()
            assert m == int((st == 0).sum()) and info["held"] == K.size and info["pushes"] == i + 1 and info["offered"] == lo
            for n in prefixes(K.size):
                got = ag.finish_bytes(n)
                assert got.size == 49 * n + 32 and (got == ref(engine, b, K[:n])).all(), (i, n)
                if kind == "wire":
                    assert (ag.keys(n) == b.wire[K[:n]]).all(), (i, n)
            if old is not None:                              # nothing in front of 49 * held was written
                assert (ag.keys(old.shape[0]) == old).all()
        assert held_mod4 == {0, 1, 2, 3} and K.size == TOTAL - 3
        assert {511, 512, 513} <= {int(x) for x in np.cumsum(SEQ)}


@pytest.mark.parametrize("B", [0, 64], ids=["B512", "B64"])
@pytest.mark.parametrize("kind", ["affine", "wire", "mixed"])
def test_finish_and_keys_after_every_push(engine, kind, B):
    run_sequence(engine, kind, B)


# ------------------------------------------------------------------ the key column under removals
def loaded(eng, cache, b, B=0, capacity=HELD + EXTRA, pushes=LOAD):
    ag, lo = eng.aggregator(capacity, B, hold_keys=True), 0
    for cnt in pushes:
        st, m, _ = ag.push_keyed(cache, b.rec[lo:lo + cnt], b.msgs[lo:lo + cnt])
        assert m == cnt and not st.any()
        lo += cnt
    return ag


def check(engine, ag, cache, b, K, extra=(HELD, HELD + EXTRA)):
    """the object holds exactly the lanes K of b, keys included, and one more push lands behind them"""
    K = np.asarray(K, dtype=np.int64)
    info = ag.info()
    assert info["held"] == K.size and info["blocks"] == K.size // info["block_lanes"]
    pre = prefixes(K.size)
    for n in pre[::-1] + pre:
        assert (ag.finish_bytes(n) == ref(engine, b, K[:n])).all(), n
        keys = ag.keys(n)
        assert keys.shape == (n, 49) and (keys == b.wire[K[:n]]).all(), n
    lo, hi = extra
    st, m, _ = ag.push_keyed(cache, b.rec[lo:hi], b.msgs[lo:hi])
    assert m == hi - lo and not st.any()
    K = np.concatenate([K, np.arange(lo, hi)])
    assert (ag.finish_bytes() == ref(engine, b, K)).all() and (ag.keys() == b.wire[K]).all()


@pytest.mark.parametrize("n", [1, 2, 3, 4, 511, 512, 513])
def test_drop_front_moves_the_keys_with_the_lanes(engine, n):
    b = honest_lanes(engine)
    with new_cache(engine, "wire") as cache, loaded(engine, cache, b) as ag:
        ag.drop_front(n)
        check(engine, ag, cache, b, np.arange(n, HELD))


@pytest.mark.parametrize("B", [0, 64], ids=["B512", "B64"])
@pytest.mark.parametrize("name", ["random", "lane 0"])
def test_remove_by_mask_moves_the_keys_with_the_lanes(engine, name, B):
    b = honest_lanes(engine)
    drop = np.zeros(HELD, np.uint8)
    if name == "random":
        drop[np.random.default_rng(0x0DD).choice(HELD, HELD // 3, replace=False)] = 2
    else:
        drop[0] = 1
    K = np.flatnonzero(drop == 0)
    with new_cache(engine, "wire") as cache, loaded(engine, cache, b, B) as ag:
        assert ag.remove(drop) == K.size
        check(engine, ag, cache, b, K)


def test_remove_device_take_block_and_reset(engine):
    import schnorr_sig_amd as ssa
    import torch
    b = honest_lanes(engine)
    with new_cache(engine, "wire") as cache, loaded(engine, cache, b) as ag:
        drop = np.zeros(HELD, np.uint8)
        drop[3::7] = 1
        K = np.flatnonzero(drop == 0)
        assert ag.remove_device(dev(drop)[0]) == K.size
        agg, keys = ag.take_block(700)
        assert isinstance(agg, ssa.AggregateSignature) and agg.to_bytes() == ref(engine, b, K[:700]).tobytes()
        assert (keys == b.wire[K[:700]]).all() and ag.info()["held"] == K.size - 700
        # the device forms, at odd offsets: finish and keys only enqueue
        rest = K[700:]
        d_agg = torch.full((49 * rest.size + 32 + 8,), 0xEE, dtype=torch.uint8, device="cuda:0")
        d_keys = torch.full((49 * 100 + 8,), 0xEE, dtype=torch.uint8, device="cuda:0")
        assert ag.finish_device(d_agg[3:]) == rest.size and ag.keys_device(d_keys[5:], 100) == 100
        engine.sync()
        got = d_keys.cpu().numpy()
        assert (got[5:5 + 4900].reshape(100, 49) == b.wire[rest[:100]]).all() and (got[:5] == 0xEE).all() and (got[4905:] == 0xEE).all()
        assert (d_agg.cpu().numpy()[3:3 + 49 * rest.size + 32] == ref(engine, b, rest)).all()
        check(engine, ag, cache, b, rest)
        ag.reset()
        assert ag.info()["held"] == 0 and ag.keys().shape == (0, 49)
        st, m, _ = ag.push_keyed(cache, b.rec[7:107], b.msgs[7:107])
        assert m == 100 and (ag.keys() == b.wire[7:107]).all()


def test_a_removal_in_pieces_carries_the_keys(engine):
    """a context whose MSM slice is 512 lanes: the move walks three pieces, each through the four-part staging"""
    import schnorr_sig_amd as ssa
    b = honest_lanes(engine)
    old = os.environ.get("SSA_MSM_SLICE")
    os.environ["SSA_MSM_SLICE"] = "512"
    try:
        tight = ssa.Engine(0)
    finally:
        if old is None:
            del os.environ["SSA_MSM_SLICE"]
        else:
            os.environ["SSA_MSM_SLICE"] = old
    try:
        assert tight.info()["msm_slice"] == 512
        drop = np.zeros(HELD, np.uint8)
        drop[1::4] = 1
        for K, act in ((np.arange(1, HELD), lambda ag: ag.drop_front(1)),
                       (np.flatnonzero(drop == 0), lambda ag: ag.remove(drop))):
            with new_cache(tight, "wire") as cache, loaded(tight, cache, b, pushes=[512, 511, 265]) as ag:
                act(ag)
                check(engine, ag, cache, b, K, extra=(HELD, HELD + 100))
    finally:
        tight.close()


# ------------------------------------------------------------------ the round trip
def test_finish_and_keys_are_what_the_validator_takes(engine):
    b = pool(engine)[0]
    sl = b[FIRST:FIRST + BIG]
    with new_cache(engine, "wire") as cache, engine.aggregator(BIG, hold_keys=True) as ag:
        st, m, stats = ag.push_keyed(cache, sl.rec, sl.msgs)
        K = np.flatnonzero(st == 0)
        assert m == BIG - 3 and stats[5] == 1
        v, vst = engine.verify_aggregates_cached(cache, [ag.finish_bytes()], ag.keys(), sl.msgs[K])
        assert v.tolist() == [OK] and int(vst[2]) == 0 and int(vst[1]) == int(vst[0])


# ------------------------------------------------------------------ errors
def test_refusals_change_neither_object_nor_cache(engine):
    import schnorr_sig_amd as ssa
    lib, p = ssa._lib, ssa._ptr
    b = pool(engine)[0][:40]
    rec, nk, stats = b.rec, C.c_uint64(77), np.full(12, 9, np.uint64)
    st = np.full(40, 0xEE, np.uint8)

    def affine(ctx, ag, kc, n=20):
        return lib.ssa_aggregator_push_cached(ctx, ag.handle, kc, p(b.sigs), p(b.pks), None, p(b.msgs), None, 80, 80, n,
                                              p(st), C.byref(nk), stats.ctypes.data)

    def keyed(ctx, ag, kc, n=20):
        return lib.ssa_aggregator_push_keyed_cached(ctx, ag.handle, kc, p(rec), p(b.msgs), None, 80, 80, n, p(st),
                                                    C.byref(nk), stats.ctypes.data)
    other = ssa.Engine(0)
    try:
        with new_cache(engine, "affine") as ca, new_cache(engine, "wire") as cw, new_cache(other, "affine") as co, \
                new_cache(other, "wire") as cow, engine.aggregator(30, 4) as ag, \
                engine.aggregator(30, 4, hold_keys=True) as hk:
            assert ag.push(b.sigs[:6], b.pks[:6], b.msgs[:6], cache=ca)[1] == 6
            assert hk.push_keyed(cw, rec[:6], b.msgs[:6])[1] == 6
            caches = (ca, cw, co, cow)
            before = [c.info() for c in caches]
            state = [(o.info(), o.finish_bytes()) for o in (ag, hk)]
            keys = hk.keys()
            ctx = engine._ctx
            assert affine(ctx, ag, cw.handle) == ssa.ERR_ARG and keyed(ctx, ag, ca.handle) == ssa.ERR_ARG     # the other mode
            assert affine(ctx, ag, co.handle) == ssa.ERR_ARG and keyed(ctx, ag, cow.handle) == ssa.ERR_ARG    # foreign
            assert affine(ctx, ag, None) == ssa.ERR_ARG and keyed(ctx, ag, None) == ssa.ERR_ARG               # none
            assert affine(other._ctx, ag, co.handle) == ssa.ERR_ARG                          # not the object's context
            assert affine(ctx, ag, ca.handle, n=25) == ssa.ERR_ARG and keyed(ctx, ag, cw.handle, n=25) == ssa.ERR_ARG
            assert keyed(ctx, hk, cw.handle, n=25) == ssa.ERR_ARG                            # n above the room left
            # an object with a key column takes records alone
            assert affine(ctx, hk, ca.handle) == ssa.ERR_ARG
            assert lib.ssa_aggregator_push(ctx, hk.handle, p(b.sigs), p(b.pks), None, p(b.msgs), None, 80, 80, 20, 0, p(st),
                                           C.byref(nk)) == ssa.ERR_ARG
            # keys on an object without one, and more keys than lanes
            out = np.full(49 * 8, 0xEE, np.uint8)
            assert lib.ssa_aggregator_keys(ctx, ag.handle, 6, p(out)) == ssa.ERR_ARG
            assert lib.ssa_aggregator_keys(ctx, hk.handle, 7, p(out)) == ssa.ERR_ARG
            assert lib.ssa_aggregator_keys_device(ctx, ag.handle, 0, None) == ssa.ERR_ARG
            assert lib.ssa_aggregator_keys(ctx, hk.handle, 0, None) == 0                     # n_take == 0 writes nothing
            with pytest.raises(RuntimeError):
                ag.keys()
            with pytest.raises(RuntimeError):
                ag.push_keyed(None, rec[:2], b.msgs[:2])
            assert (out == 0xEE).all() and (st == 0xEE).all() and nk.value == 77 and stats.tolist() == [9] * 12
            assert [c.info() for c in caches] == before
            for o, (info, agg) in zip((ag, hk), state):
                assert o.info() == dict(info, finishes=o.info()["finishes"]) and (o.finish_bytes() == agg).all()
            assert (hk.keys() == keys).all() and (keys == b.wire[:6]).all()
            # an empty push counts a push and touches neither
            assert keyed(ctx, hk, cw.handle, n=0) == 0 and affine(ctx, ag, ca.handle, n=0) == 0
            assert nk.value == 0 and stats.tolist() == [0] * 12 and [c.info() for c in caches] == before
            assert hk.info() == dict(state[1][0], pushes=2, finishes=hk.info()["finishes"])
            # ... and at the room left the pushes run
            assert keyed(ctx, hk, cw.handle, n=24) == 0 and nk.value == 24 and (hk.keys() == b.wire[list(range(6)) + list(range(24))]).all()
    finally:
        other.close()


# ------------------------------------------------------------------ independence
@pytest.mark.parametrize("mode", MODES)
def test_poisoned_workspaces_and_a_dirty_predecessor_change_nothing(engine, mode):
    import schnorr_sig_amd as ssa
    b = pool(engine)[0]
    sl, small = b[FIRST:FIRST + BIG], b[:700]

    def once(eng, prelude):
        with new_cache(eng, mode) as cache, eng.aggregator(BIG, hold_keys=(mode == "wire")) as ag:
            prelude(eng)
            st, m, stats = push(ag, cache, mode, sl)
            return st.tobytes(), m, stats, ag.finish_bytes().tobytes(), ag.keys().tobytes() if mode == "wire" else b""

    def dirty(eng):
        with new_cache(eng, "wire") as kc:
            eng.aggregate_valid_keyed_cached(kc, small.rec, small.msgs)
    fresh = ssa.Engine(0)
    try:
        want = once(fresh, lambda e: None)
    finally:
        fresh.close()
    K = FIRST + np.flatnonzero(np.frombuffer(want[0], np.uint8) == 0)
    assert want[3] == ref(engine, b, K).tobytes()
    assert once(engine, lambda e: e.debug_poison_workspaces(0xA5)) == want
    assert once(engine, dirty) == want
    assert once(engine, lambda e: e.debug_poison_workspaces(0x01)) == want
