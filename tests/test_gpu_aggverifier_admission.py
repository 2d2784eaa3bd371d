"""The admission column of the streaming aggregator and mixed pushes through the key cache with a required class
(ssa_aggregator_admission, ssa_aggverifier_push_mixed_cached*).  Two things are held here:

    the column    admission() is the class of the push that admitted each lane, and moves with its lane under every
                  removal; the expected classes come from numpy indexing of the classes the test itself pushed with;
    the equality  for a prefix whose lanes all came through a cache or are known lanes of class 2 pushed with
                  require = 2, finish(e_agg, n) == Engine.verify_aggregates_cached (wire keys: the wire form) with
                  k = 1 on the whole block.  The right-hand side is always computed outside the object, on a fresh
                  cache (rhs); e_agg by the one-shot Engine.aggregate; S from Python integers.

A lane refused on the device is held as failed and answers SSA_MALFORMED, as in section 34."""
import os
import struct
import subprocess

import numpy as np
import pytest

from aggregate_model import Q
from test_gpu_aggregates_cached import spoil_classes
from test_gpu_aggverifier import make_scalars, scalar_bytes

pytestmark = pytest.mark.gpu

OK, BAD_KEY, INVALID, MALFORMED = 0, 1, 2, 3
UNKNOWN = 0xFFFFFFFF
WORLD, HELD = 1300, 1160                             # lanes signed; the first HELD of them are in the pools
POOL_B = 8                                           # the aggregators' B: never the verifier's
GROUP, PER = 434, 40                                 # world lane w < HELD is signed by signer 40 (w // 434) + w % 40;
                                                     # the lanes behind HELD by a signer of their own each
CUTS = [(0, 290, "unscreened", 0), (290, 580, "screened", 1), (580, 870, "cached", 2), (870, HELD, "screened", 1)]
DISTINCT, HITS, INSERTED, EVICTIONS, BYPASSED, BOUND = range(6)
MODES, FORMS = ["affine", "wire"], ["host", "device"]
NEW_LAUNCHES = ("agv_k_classify_adm", "agv_k_kst_at", "agv_k_require")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dev(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    torch.cuda.synchronize()
    return t


def distinct(keys):
    return len(np.unique(keys, axis=0)) if keys.shape[0] else 0


class World:
    """WORLD honest signatures over 80-byte messages, the first HELD by 120 signers in three groups; lanes [0, HELD)
    stand in the pools in a random order.  place[w]: where world lane w stands in a pool; classes: the class of every place of the pool
    that CUTS builds.  ref(lanes): the one-shot aggregate of a block, computed once and never changed."""

    def __init__(self, engine):
        rng = np.random.default_rng(0xA635)
        self.engine = engine
        self.msgs = rng.integers(0, 256, size=(WORLD, 80), dtype=np.uint8)
        w = np.arange(WORLD)
        sks = make_scalars(rng, 3 * PER + WORLD - HELD)[np.where(w < HELD, PER * (w // GROUP) + w % PER, 3 * PER + w - HELD)]
        self.pks, self.sigs = engine.keygen_sign_many(sks, make_scalars(rng, WORLD), self.msgs)
        self.wire, st = engine.compress_many(self.pks)
        assert (st == 0).all()
        self.rs = np.ascontiguousarray(self.sigs[:, :49])
        self.keyed = np.ascontiguousarray(np.concatenate([self.wire, self.sigs], axis=1))
        self.s = [int.from_bytes(self.sigs[i, 49:].tobytes(), "little") for i in range(WORLD)]
        self.order = rng.permutation(HELD)
        self.place = np.full(WORLD, UNKNOWN, dtype=np.int64)
        self.place[self.order] = np.arange(HELD)
        self.classes = np.concatenate([np.full(hi - lo, c, np.uint8) for lo, hi, _, c in CUTS])
        self._refs, self._coeffs, self._rhs = {}, {}, {}

    def new_pool(self, engine=None, after_push=None, hold_admission=True):
        """the pool of CUTS: one push without the screen, one screened, one through an affine cache, one screened"""
        eng = engine or self.engine
        ag, o = eng.aggregator(HELD, POOL_B, hold_admission=hold_admission), self.order
        with eng.keycache_create(256) as cache:
            for lo, hi, how, _ in CUTS:
                ix = o[lo:hi]
                out = ag.push(self.sigs[ix], self.pks[ix], self.msgs[ix], screen=how != "unscreened",
                              cache=cache if how == "cached" else None)
                assert out[1] == hi - lo and not out[0].any()
                if after_push:
                    after_push(ag, hi)
        return ag

    def new_keyed_pool(self, engine=None):
        """every lane through push_keyed and a wire cache: the key column, and class 2 everywhere"""
        eng = engine or self.engine
        ag, o = eng.aggregator(HELD, POOL_B, hold_keys=True, hold_admission=True), self.order
        with eng.keycache_create(256, wire=True) as cache:
            for lo, hi in ((0, 513), (513, HELD)):
                status, kept, _ = ag.push_keyed(cache, self.keyed[o[lo:hi]], self.msgs[o[lo:hi]])
                assert kept == hi - lo and not status.any()
        return ag

    def ref(self, lanes):
        key = tuple(int(v) for v in lanes)
        if key not in self._refs:
            ix = np.asarray(key, dtype=np.int64)
            st, agg, _, nf = self.engine.aggregate(self.sigs[ix], self.pks[ix], self.msgs[ix])
            assert st == OK and nf == 0
            agg.setflags(write=False)
            self._refs[key] = agg
        return self._refs[key]

    def e(self, lanes):
        return self.ref(lanes)[49 * len(lanes):] if len(lanes) else np.zeros(32, np.uint8)

    def known_sum(self, lanes, known):
        """S by Python integers: the coefficients of the one-shot transcript of the block, the scalars of the signatures"""
        key = tuple(int(v) for v in lanes)
        if key not in self._coeffs:
            ix = np.asarray(key, dtype=np.int64)
            a = self.engine.aggregate_coeffs(self.rs[ix], self.pks[ix], self.msgs[ix])
            self._coeffs[key] = [int.from_bytes(a[i].tobytes(), "little") for i in range(len(ix))]
        a = self._coeffs[key]
        return sum(a[i] * self.s[lanes[i]] for i in range(len(lanes)) if known[i]) % Q

    def rhs(self, body, mode, scalar, n=None, tag=None):
        """the right-hand side: the one-shot cached call, k = 1, on a FRESH cache, over the first n lanes of the block
        body (rs, pks, wire, msgs).  tag: what names the body, for the memo (None: do not keep)"""
        rs, pks, wire, msgs = body
        n = rs.shape[0] if n is None else n
        key = None if tag is None else (tag, mode, n, bytes(scalar))
        if key is None or key not in self._rhs:
            agg = np.concatenate([rs[:n].reshape(-1), np.asarray(scalar, np.uint8)])
            with self.engine.keycache_create(256, wire=(mode == "wire")) as cache:
                v, _ = self.engine.verify_aggregates_cached(cache, [agg], (wire if mode == "wire" else pks)[:n], msgs[:n])
            if key is None:
                return int(v[0])
            self._rhs[key] = int(v[0])
        return self._rhs[key]

    def body(self, lanes):
        ix = np.asarray(lanes, dtype=np.int64)
        return self.rs[ix], self.pks[ix], self.wire[ix], self.msgs[ix]


@pytest.fixture(scope="module")
def world(engine):
    return World(engine)


@pytest.fixture(scope="module")
def pool(world):
    ag = world.new_pool()
    yield ag
    ag.close()


@pytest.fixture(scope="module")
def keyed_pool(world):
    ag = world.new_keyed_pool()
    yield ag
    ag.close()


def engine_with(**env):
    import schnorr_sig_amd as ssa
    old = {k: os.environ.get(k) for k in env}
    os.environ.update({k: str(v) for k, v in env.items()})
    try:
        return ssa.Engine(0)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def push_cached(av, ag, places, body_u, mode, form, cache, require, engine=None):
    """ONE mixed push through the cache in the given mode and form -> (stats as ints, the result word or None)"""
    rs, pks, wire, msgs = body_u
    places = np.asarray(places, dtype=np.uint32)
    u = rs.shape[0]
    if form == "host":
        if mode == "affine":
            n, st = av.push_mixed(ag, places, rs, pks, msgs if u else None, cache=cache, require=require, engine=engine)
        else:
            n, st = av.push_mixed_wire(ag, places, rs, wire, msgs if u else None, cache=cache, require=require, engine=engine)
        word = None
    else:
        import torch
        words = torch.full((8,), 0x6EEEEEEE, dtype=torch.int32, device="cuda:0")
        d_places = dev(places.view(np.int32))
        d = [dev(a) if u else None for a in (rs, wire if mode == "wire" else pks, msgs)]
        if mode == "affine":
            n, st = av.push_mixed_device(ag, d_places, words[3:4], d[0], d[1], d[2], cache=cache, require=require)
        else:
            n, st = av.push_mixed_wire_device(ag, d_places, words[3:4], d[0], d[1], d[2], cache=cache, require=require)
        av.engine.sync()
        got = words.cpu().numpy()
        assert (np.delete(got, 3) == 0x6EEEEEEE).all(), got                # the words next to the result word are untouched
        word = int(got[3])
    st = [int(x) for x in st]
    assert n == places.size and len(st) == 8 and st[6] == st[7] == 0, st
    return st, word


def push_block(av, ag, world, lanes, known, mode, form, cache, require=2, body=None):
    """the block `lanes` (world lanes, in block order) as ONE push: known[i] -> lane i by its place in the pool; body:
    the block's (rs, pks, wire, msgs) where it differs from the world's"""
    lanes, known = np.asarray(lanes, dtype=np.int64), np.asarray(known, dtype=bool)
    places = np.where(known, world.place[lanes], UNKNOWN)
    assert (places[known] != UNKNOWN).all()
    body = body or world.body(lanes)
    return push_cached(av, ag, places, tuple(a[~known] for a in body), mode, form, cache, require)


def known_sets(n, B, rng):
    idx = np.arange(n)
    sets = {"all": idx >= 0, "none": idx < 0, "every second": idx % 2 == 0, "random": rng.integers(0, 2, n) == 1}
    for at in sorted({0, n - 1, B - 1, B} & set(range(n))):                 # first, last, either side of a block edge
        sets["one unknown at %d" % at] = idx != at
    return sets


def block_lanes(n):
    """a block of n lanes the pools hold, in an order of its own; above HELD lanes the first ones come again"""
    return np.resize((np.arange(HELD) * 7 + 3) % HELD, n)


def neg(e):
    return scalar_bytes((Q - int.from_bytes(np.asarray(e, np.uint8).tobytes(), "little")) % Q)


def plus_one(e):
    return scalar_bytes((int.from_bytes(np.asarray(e, np.uint8).tobytes(), "little") + 1) % Q)


# ---------------------------------------------------------------------------------------------- 1. the column
@pytest.mark.parametrize("pieces", ["one piece", "three pieces"])
def test_admission_after_each_push_and_under_every_removal(engine, world, pieces):
    """admission() against the classes the test pushed with, after each push and after drop_front(B), drop_front(B + 1),
    a mask, a list, take(n) and reset; finish is the one-shot aggregate of the kept lanes every time.  "three pieces": a
    context whose MSM slice is 512 lanes, so that a move over 1100 lanes walks three pieces"""
    import torch
    eng = engine if pieces == "one piece" else engine_with(SSA_MSM_SLICE=512)
    try:
        def after_push(ag, held):
            assert (ag.admission() == world.classes[:held]).all(), held
            assert (ag.admission(held - 1) == world.classes[:held - 1]).all() and ag.admission(0).size == 0
        with world.new_pool(eng, after_push) as ag:
            lanes, cls = world.order.copy(), world.classes.copy()          # the model: world lane and class by place

            def check(what):
                got = ag.admission()
                assert got.dtype == np.uint8 and (got == cls).all(), what
                assert ag.info()["held"] == len(lanes)
                assert (ag.finish_bytes() == world.ref(lanes)).all(), what  # byte-equal for the kept lanes
                for n in (1, len(lanes) // 2):
                    assert (ag.admission(n) == cls[:n]).all()
            check("pushed")
            if pieces == "three pieces":
                eng.enable_timing(True)
                eng.read_timing("agx_k_move")
            ag.drop_front(POOL_B)
            lanes, cls = lanes[POOL_B:], cls[POOL_B:]
            check("drop_front(B)")
            if pieces == "three pieces":
                assert eng.read_timing("agx_k_move")[1] == 3               # 1152 kept lanes in pieces of 512
                eng.enable_timing(False)
            ag.drop_front(POOL_B + 1)
            lanes, cls = lanes[POOL_B + 1:], cls[POOL_B + 1:]
            check("drop_front(B + 1)")
            drop = (np.arange(len(lanes)) % 2 == 1).astype(np.uint8)
            assert ag.remove(drop) == int((drop == 0).sum())
            lanes, cls = lanes[drop == 0], cls[drop == 0]
            check("every second")
            rng = np.random.default_rng(35)
            gone = rng.permutation(len(lanes))[:len(lanes) // 3]
            keep = np.ones(len(lanes), bool)
            keep[gone] = False
            assert ag.remove_indices(gone) == int(keep.sum())
            lanes, cls = lanes[keep], cls[keep]
            check("a random third")
            assert len(set(cls.tolist())) == 3                             # all three classes are still there
            # the device form, at an odd offset
            d_out = torch.full((len(lanes) + 8,), 0xEE, dtype=torch.uint8, device="cuda:0")
            torch.cuda.synchronize()
            assert ag.admission_device(d_out[3:], 100) == 100
            eng.sync()
            got = d_out.cpu().numpy()
            assert (got[3:103] == cls[:100]).all() and (got[:3] == 0xEE).all() and (got[103:] == 0xEE).all()
            taken = ag.take(101)
            assert taken.bytes == world.ref(lanes[:101]).tobytes()
            lanes, cls = lanes[101:], cls[101:]
            check("take(101)")
            # pushes behind a removal: classes of their own, behind the kept ones
            ix = world.order[:20]
            assert ag.push(world.sigs[ix], world.pks[ix], world.msgs[ix], screen=False)[1] == 20
            lanes, cls = np.concatenate([lanes, ix]), np.concatenate([cls, np.zeros(20, np.uint8)])
            check("a push behind the removals")
            ag.reset()
            assert ag.admission().size == 0 and ag.info()["held"] == 0
            assert ag.push(world.sigs[ix], world.pks[ix], world.msgs[ix])[1] == 20
            assert (ag.admission() == 1).all()                             # nothing of the earlier life is left
            with pytest.raises(RuntimeError):
                ag.admission(21)
    finally:
        if eng is not engine:
            eng.close()


def test_the_keyed_pool_is_class_two_everywhere_and_keeps_its_keys(world, keyed_pool):
    assert (keyed_pool.admission() == 2).all() and keyed_pool.admission().size == HELD
    assert (keyed_pool.keys() == world.wire[world.order]).all()
    assert (keyed_pool.finish_bytes(600) == world.ref(world.order[:600])).all()


def test_a_pool_without_the_flag_refuses_admission_and_launches_what_it_did(world):
    """the same pushes, removals and finishes on an object with and without the column: the same launches by name and
    number, none of this section's; admission() on the object without the flag is refused"""
    import schnorr_sig_amd as ssa
    eng = ssa.Engine(0)
    names = ("agx_k_append", "agx_k_check", "agx_k_move", "agx_k_first_changed", "av_k_keep", "agx_k_coeff_fold",
             "ag_k_fold_finish", "ag_k_tree", "ag_k_level", "ssa_k_hash", "agx_k_mark", "agx_k_bits_to_mask") + NEW_LAUNCHES
    try:
        counts, finals = {}, {}
        for flag in (False, True):
            eng.enable_timing(True)
            for name in names:
                eng.read_timing(name)                                      # drains the key
            with world.new_pool(eng, hold_admission=flag) as ag:
                drop = (np.arange(HELD) % 3 == 0).astype(np.uint8)
                ag.remove(drop)
                ag.drop_front(POOL_B + 3)
                ag.remove_indices([5, 1, 77])
                finals[flag] = ag.finish_bytes().copy()
                counts[flag] = {name: eng.read_timing(name)[1] for name in names}
                eng.enable_timing(False)
                one = np.array([0], np.uint32)
                if flag:
                    assert ag.admission().size == ag.info()["held"]
                else:
                    with pytest.raises(RuntimeError):
                        ag.admission()
                    with pytest.raises(RuntimeError):
                        ag.admission(0)
                    info = ag.info()
                    with eng.keycache_create(64) as cache, eng.aggregate_verifier(8) as av:
                        for require in (1, 2):                             # a class needs the column: refused on the host
                            rc = ssa._lib.ssa_aggverifier_push_mixed_cached(
                                eng._ctx, av.handle, ag.handle, cache.handle, ssa._ptr(one), 1, None, None, None, None, None,
                                0, 0, 0, require, None)
                            assert rc == ssa.ERR_ARG
                        assert av.info()["held"] == 0 and av.info()["pushes"] == 0 and ag.info() == info
                        rc = ssa._lib.ssa_aggverifier_push_mixed_cached(                       # require == 0: any pool
                            eng._ctx, av.handle, ag.handle, cache.handle, ssa._ptr(one), 1, None, None, None, None, None,
                            0, 0, 0, 0, None)
                        assert rc == 0 and av.info()["held"] == 1
        assert counts[False] == counts[True], (counts[False], counts[True])
        assert all(counts[False][name] == 0 for name in NEW_LAUNCHES) and counts[False]["agx_k_move"] >= 3
        assert (finals[False] == finals[True]).all()
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------- 2. the equality
@pytest.mark.parametrize("B,n", [(B, n) for B in (4, 512) for n in sorted({1, 2, 3, B - 1, B, B + 1, 513, 1288})])
def test_blocks_and_known_sets_equal_the_one_shot_cached_call(engine, world, keyed_pool, B, n):
    """every known set, affine and wire keys, host and device forms; the cache cold for the first set, warm for the
    next, cleared and partly warmed (the first half of the block's keys) in front of "random".  require = 2 on a pool whose
    every lane is class 2"""
    rng = np.random.default_rng(B)
    lanes = block_lanes(n)
    body = world.body(lanes)
    sets = known_sets(n, B, rng)
    if n >= 3:
        sets["a repeated place"] = None
    for mode in MODES:
        with engine.keycache_create(512, wire=(mode == "wire")) as cache, engine.aggregate_verifier(n, B) as av, \
                engine.aggregate_verifier(n, 64) as scratch:
            seen = set()                                                   # the keys the cache holds, by their bytes
            for name, known in sets.items():
                ln, bd, tag = lanes, body, ("block", n)
                if known is None:                                          # one place named twice
                    ln = lanes.copy()
                    ln[n - 1] = ln[0]
                    known = np.ones(n, bool)
                    bd, tag = world.body(ln), ("repeated", n)
                keys = bd[2] if mode == "wire" else bd[1]
                if name == "random" and n >= 2:
                    cache.clear()
                    half = n // 2
                    if mode == "affine":
                        scratch.push(bd[0][:half], bd[1][:half], bd[3][:half], cache=cache)
                    else:
                        scratch.push_wire(bd[0][:half], bd[2][:half], bd[3][:half], cache=cache)
                    seen = {k.tobytes() for k in keys[:half]}
                e_ln = world.e(ln)
                for form in FORMS:
                    av.reset()
                    st, word = push_block(av, keyed_pool, world, ln, known, mode, form, cache)
                    assert word in (None, 0)
                    mine = {k.tobytes() for k in keys[~known]}
                    assert st[DISTINCT] == len(mine) and st[BYPASSED] == st[EVICTIONS] == 0, st
                    assert (st[HITS], st[INSERTED]) == (len(mine & seen), len(mine - seen)), (name, mode, form, st)   # cold, warm, partly
                    seen |= mine
                    info = av.info()
                    assert info["held"] == info["pushed"] == n and info["reserved"] == int((~known).sum())
                    for scalar, honest in ((e_ln, True), (plus_one(e_ln), False), (neg(e_ln), False)):
                        got, want = av.finish(scalar), world.rhs(bd, mode, scalar, tag=tag)
                        assert got == want == (OK if honest else INVALID), (name, mode, form, got, want)
                    assert av.known_sum() == world.known_sum(ln, known), (name, mode, form)


def spoiled_block(engine, world, mode, cname, n, known, at):
    """the block's body with the key of lane `at` (an unknown lane) spoiled"""
    lanes = block_lanes(n)
    pks, inf, wire = world.pks[lanes].copy(), np.zeros(n, np.uint8), world.wire[lanes].copy()
    assert not known[at]
    spoil_classes(engine, mode)[cname](pks, inf, wire, at)
    return lanes, (world.rs[lanes].copy(), pks, wire, world.msgs[lanes].copy())


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("mode", MODES)
def test_wrong_blocks_and_the_key_status_at_the_lanes_true_place(engine, world, keyed_pool, mode, form):
    """P + T2 at the LAST unknown position of the push (compact lane u - 1, place n - 3): exactly the prefixes that
    reach the place answer INVALID_PUBLIC_KEY -- a status written at held + j would decide far in front of it --, the
    key decides over a malformed R in the same prefix, and the prefixes are finished descending, then ascending.  Then a
    wire key that does not decode, and a changed message byte."""
    n = 600
    known = np.arange(n) % 4 != 1
    at = int(np.flatnonzero(~known)[-1])
    assert at == n - 3 and int((~known).sum()) == 150
    lanes, body = spoiled_block(engine, world, mode, "p_plus_t2", n, known, at)
    bad_r = tuple(a.copy() for a in body)
    r_at = int(np.flatnonzero(~known)[70])                                 # an unknown lane in front of the key
    bad_r[0][r_at, 48] |= 0x01
    prefixes = [1, 2, 150, 151, r_at, r_at + 1, 512, 513, at - 1, at, at + 1, at + 2, n]
    with engine.keycache_create(256, wire=(mode == "wire")) as cache, engine.aggregate_verifier(2 * n, 4) as av:
        push_block(av, keyed_pool, world, lanes, known, mode, form, cache, body=body)
        push_block(av, keyed_pool, world, lanes, known, mode, form, cache, body=bad_r)     # behind it, in the same object
        for p in prefixes[::-1] + prefixes:
            e = world.e(lanes[:p])
            got, want = av.finish(e, p), world.rhs(body, mode, e, p, tag=("pt", n))
            assert got == want == (BAD_KEY if p > at else OK), (p, got, want)
            if p <= at:                                                    # (another key is another leaf, root and S)
                assert av.known_sum(p) == world.known_sum(lanes[:p], known[:p]), p
        e_all = world.e(lanes)
        assert av.finish(neg(e_all), n) == BAD_KEY == world.rhs(body, mode, neg(e_all), tag=("pt", n))
        # the second push: its own prefixes, with the malformed R in front of the key
        both = np.concatenate([lanes, lanes])
        full = tuple(np.concatenate([a, b]) for a, b in zip(body, bad_r))
        for p in (n + r_at, n + r_at + 1, n + at, n + at + 1, 2 * n):
            e = world.e(both[:p])
            got, want = av.finish(e, p), world.rhs(full, mode, e, p, tag=("pt2", n))
            assert got == want == BAD_KEY, (p, got, want)                  # the first push's key is in every one of them
        # without the first push the malformed R decides until the key is reached
        av.reset()
        push_block(av, keyed_pool, world, lanes, known, mode, form, cache, body=bad_r)
        for p, verdict in ((r_at, OK), (r_at + 1, MALFORMED), (at, MALFORMED), (at + 1, BAD_KEY), (n, BAD_KEY)):
            e = world.e(lanes[:p])
            assert av.finish(e, p) == verdict == world.rhs(bad_r, mode, e, p, tag=("ptr", n)), p
        # a changed message byte in an unknown lane
        av.reset()
        msgs = body[3].copy()
        msgs[r_at, 11] ^= 0x20
        honest = world.body(lanes)
        changed = (honest[0], honest[1], honest[2], msgs)
        push_block(av, keyed_pool, world, lanes, known, mode, form, cache, body=changed)
        assert av.finish(e_all) == INVALID == world.rhs(changed, mode, e_all, tag=("msg", n))
        assert av.finish(world.e(lanes[:r_at]), r_at) == OK
        if mode == "wire":                                                 # a wire key that does not decode
            lanes2, nodec = spoiled_block(engine, world, mode, "no_square_root", n, known, at)
            av.reset()
            push_block(av, keyed_pool, world, lanes2, known, mode, form, cache, body=nodec)
            for p in (at, at + 1, n):
                e = world.e(lanes[:p])
                got, want = av.finish(e, p), world.rhs(nodec, mode, e, p, tag=("nodec", n))
                assert got == want == (MALFORMED if p > at else OK), (p, got, want)


@pytest.mark.parametrize("evict", ["clear", "recent"])
def test_the_unknown_keys_cross_two_slice_edges_of_the_cache(world, evict):
    """a context whose lane slice is 256 lanes: 768 unknown lanes by three disjoint groups of 40 signers go through a
    cache of 64 rows in three slices, which the second and third clear or compact -- after agc_k_expand moved the
    statuses out.  P + T2 on either side of a slice edge; the verdicts are the session engine's one-shot call's"""
    eng = engine_with(SSA_LANE_SLICE=256)
    try:
        assert eng.info()["lane_slice"] == 256
        unk = np.concatenate([np.arange(g * GROUP, g * GROUP + 256) for g in range(3)])      # compact lane j: group j // 256
        n = 1100
        known = np.ones(n, bool)
        known[np.arange(768) * 10 // 7] = False                            # 768 unknown places, spread over the block
        assert int((~known).sum()) == 768
        lanes = np.empty(n, np.int64)
        lanes[~known] = unk
        lanes[known] = block_lanes(n - 768)
        with world.new_keyed_pool(eng) as ag:
            for mode in MODES:
                for edge in (255, 256):                                    # the last lane of slice 0, the first of slice 1
                    at = int(np.flatnonzero(~known)[edge])
                    pks, inf, wire = world.pks[lanes].copy(), np.zeros(n, np.uint8), world.wire[lanes].copy()
                    spoil_classes(world.engine, mode)["p_plus_t2"](pks, inf, wire, at)
                    body = (world.rs[lanes], pks, wire, world.msgs[lanes])
                    for form in FORMS:
                        with eng.keycache_create(64, wire=(mode == "wire"), evict=evict) as cache, \
                                eng.aggregate_verifier(n, 512) as av:
                            st, word = push_block(av, ag, world, lanes, known, mode, form, cache, body=body)
                            assert word in (None, 0)
                            assert st[DISTINCT] == 121 and st[EVICTIONS] == 2 and st[BYPASSED] == 0 and st[HITS] == 0, st
                            for p in (at, at + 1, n):
                                e = world.e(lanes[:p])
                                got, want = av.finish(e, p), world.rhs(body, mode, e, p, tag=("slice", edge))
                                assert got == want == (BAD_KEY if p > at else OK), (mode, form, edge, p, got, want)
                            assert av.known_sum(at) == world.known_sum(lanes[:at], known[:at])
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------- 3. refusals
def class_block(world, wanted, n=60):
    """n world lanes whose places in the pool of CUTS have the classes `wanted`, cycling"""
    by_class = {c: world.order[world.classes == c] for c in (0, 1, 2)}
    return np.array([by_class[wanted[i % len(wanted)]][i] for i in range(n)], dtype=np.int64)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("require,lowest", [(1, 0), (2, 1)])
def test_host_forms_refuse_a_lane_below_the_class_before_anything_is_applied(engine, world, pool, mode, require, lowest):
    """naming a class-0 lane with require = 1 and a class-1 lane with require = 2: SSA_ERR_ARG, and the held count, the
    info words, the cache and a following finish are what they were; the same list with the class the lanes have is
    accepted, and with require = 0 it is section 34's call"""
    good = [c for c in (2, 1) if c >= require]
    lanes = class_block(world, good)
    low = class_block(world, [lowest])[:1]
    n = len(lanes)
    known = np.arange(n) % 5 != 2
    unknown_new = np.arange(HELD, HELD + 12)                               # signers of group 2: keys the cache has not seen
    with engine.keycache_create(256, wire=(mode == "wire")) as cache, engine.aggregate_verifier(3 * n + 40, 4) as av:
        push_block(av, pool, world, lanes, known, mode, "host", cache, require=require)
        e = world.e(lanes)
        info, cinfo, rec = av.info(), cache.info(), av.record()
        assert av.finish(e) == OK
        info = av.info()
        spoiled = np.concatenate([lanes[:7], low, unknown_new, lanes[7:20]])
        k2 = np.ones(len(spoiled), bool)
        k2[8:20] = False
        assert world.classes[world.place[low[0]]] == lowest
        with pytest.raises(RuntimeError):
            push_block(av, pool, world, spoiled, k2, mode, "host", cache, require=require)
        assert av.info() == info and cache.info() == cinfo and (av.record() == rec).all()
        assert av.finish(e) == OK and av.finish(neg(e)) == INVALID
        info = av.info()
        # require = 3 is no class; a class on the plain call's terms: require at the lane's own class passes
        import schnorr_sig_amd as ssa
        rc = ssa._lib.ssa_aggverifier_push_mixed_cached(engine._ctx, av.handle, pool.handle, cache.handle,
                                                        ssa._ptr(np.array([0], np.uint32)), 1, None, None, None, None, None,
                                                        0, 0, 0, 3, None)
        assert rc == ssa.ERR_ARG and av.info() == info
        st, _ = push_block(av, pool, world, spoiled, k2, mode, "host", cache, require=lowest)
        assert st[DISTINCT] == distinct(world.pks[unknown_new]) == st[INSERTED]
        both = np.concatenate([lanes, spoiled])
        assert av.finish(world.e(both)) == OK and av.info()["held"] == n + len(spoiled)
        # require = 0: section 34's verdict, ssa_verify_aggregate's on the block
        st, _ = push_block(av, pool, world, spoiled, k2, mode, "host", cache, require=0)
        three = np.concatenate([both, spoiled])
        b3 = world.body(three)
        assert av.finish(world.e(three)) == OK == engine.verify_aggregate(world.ref(three), b3[1], b3[3])
        assert av.known_sum() == world.known_sum(three, np.concatenate([known, k2, k2]))


@pytest.mark.parametrize("what", ["class 0 under require 1", "class 1 under require 2", "a sentinel too many",
                                  "both faults"])
def test_device_forms_fail_closed_with_the_bits_of_the_result_word(engine, world, pool, what):
    """bit 0: the list is invalid; bit 1: a known lane below the class.  The refused lane is held as failed: every
    prefix that reaches it answers MALFORMED, the prefixes in front of it are untouched, and after a reset the object
    serves a valid call"""
    require = 1 if what == "class 0 under require 1" else 2
    lanes = class_block(world, [2], 80)
    known = np.arange(80) % 4 != 1
    places = np.where(known, world.place[lanes], UNKNOWN).astype(np.int64)
    low = class_block(world, [require - 1])[3]
    first_bad, want_word = 0, 0
    if what != "a sentinel too many":
        places[50], first_bad, want_word = world.place[low], 50, 2         # a known lane, of a class below
    if what in ("a sentinel too many", "both faults"):
        places[2] = UNKNOWN                                                # one sentinel more than the call brings
        want_word |= 1
        first_bad = 0
    body_u = tuple(a[~known] for a in world.body(lanes))
    front = class_block(world, [2], 30)
    for mode in MODES:
        with engine.keycache_create(256, wire=(mode == "wire")) as cache, engine.aggregate_verifier(400, 4) as av:
            push_block(av, pool, world, front, np.arange(30) % 2 == 0, mode, "device", cache, require=2)
            st, word = push_cached(av, pool, places, body_u, mode, "device", cache, require)
            assert word == want_word, (what, word)
            assert av.info()["held"] == 110
            e_front = world.e(front)
            assert av.finish(e_front, 30) == OK                            # the prefix in front is unaffected
            for p in (30 + first_bad + 1, 110):
                for scalar in (e_front, np.zeros(32, np.uint8), scalar_bytes(1)):
                    assert av.finish(scalar, p) == MALFORMED, (what, p)
            if first_bad:                                                  # the refused place spoils its own lane alone
                both = np.concatenate([front, lanes[:first_bad]])
                assert av.finish(world.e(both), 30 + first_bad) == OK
            av.reset()
            st, word = push_block(av, pool, world, lanes, known, mode, "device", cache, require=2)
            assert word == 0 and av.finish(world.e(lanes)) == OK
            # the same named lane with require = 0 is accepted, with section 34's verdict
            if what in ("class 0 under require 1", "class 1 under require 2"):
                av.reset()
                st, word = push_cached(av, pool, places, body_u, mode, "device", cache, 0)
                block = lanes.copy()
                block[50] = low
                b = world.body(block)
                assert word == 0 and av.finish(world.e(block)) == OK == engine.verify_aggregate(world.ref(block), b[1], b[3])


def test_the_class_follows_the_lane_when_the_pool_moves(engine, world):
    """after a remove on the pool a place holds another lane: a place that now holds a class-2 lane passes under
    require = 2, a place that now holds a class-0 lane is refused"""
    with world.new_pool() as ag, engine.keycache_create(64) as cache, engine.aggregate_verifier(64, 4) as av:
        drop = (np.arange(HELD) % 2 == 0).astype(np.uint8)
        assert ag.remove(drop) == HELD // 2
        lanes, cls = world.order[drop == 0], world.classes[drop == 0]
        assert (ag.admission() == cls).all()
        p2, p0 = int(np.flatnonzero(cls == 2)[5]), int(np.flatnonzero(cls == 0)[5])
        assert world.classes[p2] != 2                                      # what stood at that place before was of another class
        none = tuple(a[:0] for a in world.body([0]))
        st, _ = push_cached(av, ag, [p2], none, "affine", "host", cache, 2)
        assert av.finish(world.e([lanes[p2]])) == OK
        with pytest.raises(RuntimeError):
            push_cached(av, ag, [p2, p0], none, "affine", "host", cache, 2)
        with pytest.raises(RuntimeError):
            push_cached(av, ag, [p0], none, "affine", "host", cache, 1)
        assert av.info()["held"] == 1
        st, word = push_cached(av, ag, [p0, p2], none, "affine", "device", cache, 2)
        assert word == 2 and av.finish(world.e([lanes[p2]]), 1) == OK and av.finish(np.zeros(32, np.uint8), 2) == MALFORMED
        # push_known(require=) is the same call with u = 0
        av.reset()
        assert av.push_known(ag, [p2, p2], cache=cache, require=2) == 2 and av.info()["held"] == 2
        with pytest.raises(RuntimeError):
            av.push_known(ag, [p0], cache=cache, require=1)


# ---------------------------------------------------------------------------------------------- 4. other cases
def test_every_kind_of_push_in_one_object_with_poisoned_workspaces(engine, world, pool, keyed_pool):
    """plain, cached, mixed and mixed-cached pushes in one object, in both orders around the moment it becomes keyed;
    the context's workspaces are poisoned between the calls: nothing the object needs lives in one"""
    lanes = block_lanes(1000)
    rs, pks, wire, msgs = world.body(lanes)
    known = np.zeros(1000, bool)
    known[200:400] = np.arange(200) % 2 == 0                               # mixed (section 34), from the pool of CUTS
    known[600:900] = np.arange(300) % 3 != 0                               # mixed through the cache, from the keyed pool
    with engine.keycache_create(256) as cache, engine.aggregate_verifier(1000, 4) as av:
        av.push(rs[:100], pks[:100], msgs[:100])                           # plain
        engine.debug_poison_workspaces(0x01)
        st, _ = push_block(av, keyed_pool, world, lanes[100:200], np.ones(100, bool), "affine", "host", cache)     # known: keyed from here
        engine.debug_poison_workspaces(0x5A)
        sl = slice(200, 400)
        places = np.where(known[sl], world.place[lanes[sl]], UNKNOWN)
        av.push_mixed(pool, places, rs[sl][~known[sl]], pks[sl][~known[sl]], msgs[sl][~known[sl]])
        engine.debug_poison_workspaces(0x01)
        av.push(rs[400:500], pks[400:500], msgs[400:500], cache=cache)      # cached
        av.push(rs[500:600], pks[500:600], msgs[500:600])                   # plain into a keyed, mixed object
        engine.debug_poison_workspaces(0xA5)
        push_block(av, keyed_pool, world, lanes[600:900], known[600:900], "affine", "device", cache)
        engine.debug_poison_workspaces(0x01)
        push_block(av, keyed_pool, world, lanes[900:], known[900:], "affine", "host", cache)
        known[100:200] = True
        assert av.info()["held"] == 1000 and av.cached_lanes() == 100 + 100 + 100
        for n in (1000, 900, 750, 600, 599, 450, 400, 300, 200, 150, 100, 99):
            engine.debug_poison_workspaces(0x01)                           # byte 1: "bad key", were a status read from one
            assert av.finish(world.e(lanes[:n]), n) == OK, n
            assert av.known_sum(n) == world.known_sum(lanes[:n], known[:n]), n
        assert av.finish(world.e(lanes[:999])) == INVALID


def test_a_cache_or_a_pool_of_another_context_is_refused(engine, world, pool):
    import schnorr_sig_amd as ssa
    lanes = class_block(world, [2], 8)
    none = tuple(a[:0] for a in world.body([0]))
    other = ssa.Engine(0)
    try:
        with engine.keycache_create(64) as cache, other.keycache_create(64) as far_cache, \
                other.aggregator(8, hold_admission=True) as far_pool, engine.aggregate_verifier(16, 4) as av:
            push_cached(av, pool, world.place[lanes], none, "affine", "host", cache, 2)
            info, cinfo = av.info(), far_cache.info()
            with pytest.raises(RuntimeError):
                push_cached(av, pool, world.place[lanes], none, "affine", "host", far_cache, 2)
            with pytest.raises(RuntimeError):
                push_cached(av, far_pool, [], none, "affine", "host", cache, 2)
            with pytest.raises(RuntimeError):
                push_cached(av, pool, world.place[lanes], none, "affine", "host", cache, 2, engine=other)
            with pytest.raises(ValueError):
                with engine.keycache_create(64, wire=True) as wcache:
                    push_cached(av, pool, world.place[lanes], none, "affine", "host", wcache, 2)
            assert av.info() == info and far_cache.info() == cinfo
            assert av.finish(world.e(lanes)) == OK
    finally:
        other.close()


def test_launches_of_the_new_path(world):
    """the plain mixed push on a pool with the column launches none of this section's kernels; the cached one with a
    class launches agv_k_classify_adm in place of agv_k_classify and one agv_k_kst_at; the host form adds agv_k_require"""
    import schnorr_sig_amd as ssa
    eng = ssa.Engine(0)
    names = ("agv_k_classify", "agv_k_append_at", "agv_k_mixed_close", "ssa_k_hash", "agc_expand") + NEW_LAUNCHES
    lanes = block_lanes(300)
    known = np.arange(300) % 3 != 0
    try:
        with world.new_keyed_pool(eng) as ag, eng.keycache_create(256) as cache, eng.aggregate_verifier(300, 64) as av:
            eng.enable_timing(True)

            def counts(run):
                for name in names:
                    eng.read_timing(name)
                av.reset()
                run()
                assert av.finish(world.e(lanes)) == OK
                return {name: eng.read_timing(name)[1] for name in names}
            rs, pks, wire, msgs = (a[~known] for a in world.body(lanes))
            places = np.where(known, world.place[lanes], UNKNOWN)
            got = counts(lambda: av.push_mixed(ag, places, rs, pks, msgs))
            assert all(got[name] == 0 for name in NEW_LAUNCHES + ("agc_expand",)) and got["agv_k_classify"] == 1, got
            got = counts(lambda: push_block(av, ag, world, lanes, known, "affine", "device", cache, require=2))
            assert (got["agv_k_classify"], got["agv_k_classify_adm"], got["agv_k_kst_at"], got["agv_k_require"]) == (0, 1, 1, 0), got
            assert (got["agv_k_append_at"], got["agv_k_mixed_close"], got["ssa_k_hash"], got["agc_expand"]) == (1, 1, 1, 1), got
            got = counts(lambda: push_block(av, ag, world, lanes, known, "affine", "host", cache, require=1))
            assert (got["agv_k_classify"], got["agv_k_classify_adm"], got["agv_k_kst_at"], got["agv_k_require"]) == (0, 1, 1, 1), got
            got = counts(lambda: push_block(av, ag, world, lanes, known, "affine", "host", cache, require=0))
            assert (got["agv_k_classify"], got["agv_k_classify_adm"], got["agv_k_kst_at"], got["agv_k_require"]) == (1, 0, 1, 0), got
            eng.enable_timing(False)
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------- 5. the C++ mirror
def test_cxx_mirror_gives_the_python_mirrors_bytes(engine, world, tmp_path):
    libdir = os.path.join(ROOT, "schnorr-sig_amd", "csrc")
    exe = str(tmp_path / "aggverifier_admission_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                           os.path.join(ROOT, "tests", "csrc", "aggverifier_admission_driver.cpp"), "-L" + libdir,
                           "-lschnorr_sig_amd", "-Wl,-rpath," + libdir, "-L/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    p = 300
    held = np.arange(p)[::-1]                                              # the pool: world lanes p-1 .. 0
    place = {int(w): at for at, w in enumerate(held)}
    cls_of = lambda w: place[int(w)] // 100                                # three pushes of 100 lanes: classes 0, 1, 2
    by_class = {c: [int(w) for w in held if cls_of(w) == c] for c in (0, 1, 2)}
    extra = list(range(HELD, HELD + 40))                                   # unknown lanes
    pushes = [  # (wire, require, block lanes, known mask)
        (0, 2, by_class[2][:30] + extra[:10], [True] * 30 + [False] * 10),
        (1, 1, by_class[1][:20] + extra[10:20] + by_class[2][30:40], [True] * 20 + [False] * 10 + [True] * 10),
        (0, 1, by_class[0][:3], [True] * 3),                               # refused: class 0 under require 1
        (1, 2, by_class[2][40:45] + by_class[1][20:21] + extra[20:22], [True] * 6 + [False] * 2),      # refused: class 1
        (0, 0, by_class[0][:5] + extra[22:25], [True] * 5 + [False] * 3),
    ]
    accepted = [0, 1, 4]
    block = np.array(sum((pushes[j][2] for j in accepted), []), dtype=np.int64)
    n = len(block)
    ALL = (1 << 64) - 1
    e_all = np.array(world.e(block))
    finishes = [(ALL, e_all), (40, np.array(world.e(block[:40]))), (41, e_all), (n, scalar_bytes(Q)), (0, np.zeros(32, np.uint8))]
    lens = lambda k: struct.pack("<%dQ" % k, *([80] * k))
    blob = struct.pack("<3Q", p, POOL_B, 3)
    for c in range(3):
        ix = held[100 * c:100 * c + 100]
        blob += struct.pack("<2Q", c, 100) + world.sigs[ix].tobytes() + world.pks[ix].tobytes() + lens(100) + world.msgs[ix].tobytes()
    blob += struct.pack("<3Q", n + 8, 64, len(pushes))
    want = b""
    with engine.aggregator(p, POOL_B, hold_admission=True) as ag, engine.aggregate_verifier(n + 8, 64) as av, \
            engine.keycache_create(4096) as affine, engine.keycache_create(4096, wire=True) as wcache:
        for c in range(3):
            ix = held[100 * c:100 * c + 100]
            out = ag.push(world.sigs[ix], world.pks[ix], world.msgs[ix], screen=c != 0, cache=affine if c == 2 else None)
            assert out[1] == 100
            want += out[0].tobytes()
        classes = ag.admission()
        assert (classes == np.repeat([0, 1, 2], 100)).all()
        want += classes.tobytes()
        for j, (is_wire, require, ln, known) in enumerate(pushes):
            ln, known = np.array(ln, dtype=np.int64), np.array(known, dtype=bool)
            pl = np.array([place[int(w)] if k else UNKNOWN for w, k in zip(ln, known)], dtype=np.uint32)
            unk = ln[~known]
            blob += struct.pack("<3Q", is_wire, require, len(ln)) + pl.tobytes() + struct.pack("<Q", len(unk))
            blob += world.rs[unk].tobytes() + (world.wire[unk] if is_wire else world.pks[unk]).tobytes()
            blob += lens(len(unk)) + world.msgs[unk].tobytes()
            try:
                push_cached(av, ag, pl, tuple(a[unk] for a in (world.rs, world.pks, world.wire, world.msgs)),
                            "wire" if is_wire else "affine", "host", wcache if is_wire else affine, require)
                threw = 0
            except RuntimeError:
                threw = 1
            assert threw == (0 if j in accepted else 1), j
            want += bytes([threw])
        got = [av.finish(e, None if take == ALL else take) for take, e in finishes]
        assert got == [OK, OK, INVALID, MALFORMED, OK]
        info = av.info()
    blob += struct.pack("<Q", len(finishes)) + b"".join(struct.pack("<Q", take) + e.tobytes() for take, e in finishes)
    want += struct.pack("<%di" % len(got), *got)
    want += struct.pack("<8Q", info["held"], info["capacity"], info["block_lanes"], info["pushes"], info["pushed"],
                        info["reserved"], info["blocks"], info["finishes"])
    path, outp = str(tmp_path / "cases.bin"), str(tmp_path / "out.bin")
    with open(path, "wb") as f:
        f.write(blob)
    r = subprocess.run([exe, path, outp], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    got = open(outp, "rb").read()
    assert len(got) == len(want) and got == want
