"""A block against the pool (ssa_aggverifier_push_mixed*).  The contract is one equality: with the
known lanes taken from a streaming aggregator that admitted them by a screened or cached push, finish(e_agg, n_take)
returns what ssa_verify_aggregate returns for the block handed in at once.  Expected values never come from the code
under test: e_agg from Engine.aggregate on the assembled block, verdicts from Engine.verify_aggregate on it, and
S = sum a_i s_i mod q from Python integers -- a_i from ssa_debug_aggregate_coeffs, s_i from the signature bytes.

A device refusal (a place out of range, a sentinel count other than u) marks lanes as failed, and a failed lane answers
SSA_MALFORMED through the record's malformed word, like every lane that fails a check (DESIGN.md section 34 says why the
status is that one)."""
import os
import struct
import subprocess

import numpy as np
import pytest

from aggregate_model import Q
from test_gpu_aggverifier import expected_record, make_scalars, scalar_bytes, with_e

pytestmark = pytest.mark.gpu

OK, INVALID, MALFORMED = 0, 2, 3
UNKNOWN = 0xFFFFFFFF
WORLD, HELD = 1300, 1160                             # lanes signed; the first HELD of them are in the pool
POOL_B = 8                                           # the aggregator's B: never the verifier's
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_KERNELS = ("agv_k_classify", "agv_k_append_at", "agv_k_mixed_close", "agv_k_scalars_at", "agv_k_known_fold",
               "agv_k_known_close")


class World:
    """WORLD honest signatures over 80-byte messages; lanes [0, HELD) admitted to a streaming aggregator in a random
    order, the first 600 of that order by screened pushes, the rest through a key cache.  place[w]: where world lane w
    stands in the pool.  ref(lanes): the one-shot aggregate of a block, computed once and never changed."""

    def __init__(self, engine):
        rng = np.random.default_rng(0xA634)
        self.engine = engine
        self.msgs = rng.integers(0, 256, size=(WORLD, 80), dtype=np.uint8)
        self.pks, self.sigs = engine.keygen_sign_many(make_scalars(rng, WORLD), make_scalars(rng, WORLD), self.msgs)
        self.rs = np.ascontiguousarray(self.sigs[:, :49])
        self.s = [int.from_bytes(self.sigs[i, 49:].tobytes(), "little") for i in range(WORLD)]
        self.order = rng.permutation(HELD)
        self.place = np.full(WORLD, UNKNOWN, dtype=np.int64)
        self.place[self.order] = np.arange(HELD)
        self.rng = rng
        self._refs, self._coeffs = {}, {}

    def new_pool(self, engine=None, capacity=HELD):
        eng = engine or self.engine
        ag, o = eng.aggregator(capacity, POOL_B), self.order
        with eng.keycache_create(2048) as cache:
            for lo, hi, how in ((0, 300, None), (300, 600, None), (600, 880, cache), (880, HELD, cache)):
                out = ag.push(self.sigs[o[lo:hi]], self.pks[o[lo:hi]], self.msgs[o[lo:hi]], cache=how)
                assert out[1] == hi - lo and not out[0].any()
        assert ag.info()["held"] == HELD
        return ag

    def body(self, lanes):
        lanes = np.asarray(lanes, dtype=np.int64)
        return self.rs[lanes], self.pks[lanes], self.msgs[lanes]

    def ref(self, lanes):
        key = tuple(int(v) for v in lanes)
        if key not in self._refs:
            lanes = np.asarray(key, dtype=np.int64)
            st, agg, _, nf = self.engine.aggregate(self.sigs[lanes], self.pks[lanes], self.msgs[lanes])
            assert st == OK and nf == 0
            agg.setflags(write=False)
            self._refs[key] = agg
        return self._refs[key]

    def e(self, lanes):
        return self.ref(lanes)[49 * len(lanes):]

    def known_sum(self, lanes, known):
        """S by Python integers: the coefficients of the one-shot transcript of the block, the scalars of the signatures"""
        key = tuple(int(v) for v in lanes)
        if key not in self._coeffs:
            a = self.engine.aggregate_coeffs(*self.body(lanes))
            self._coeffs[key] = [int.from_bytes(a[i].tobytes(), "little") for i in range(len(lanes))]
        a = self._coeffs[key]
        return sum(a[i] * self.s[lanes[i]] for i in range(len(lanes)) if known[i]) % Q


@pytest.fixture(scope="module")
def world(engine):
    return World(engine)


@pytest.fixture(scope="module")
def pool(world):
    ag = world.new_pool()
    yield ag
    ag.close()


def push_block(av, ag, world, lanes, known, engine=None):
    """the block `lanes` (world lanes, in block order) as ONE mixed push: known[i] -> lane i by its place in the pool"""
    lanes, known = np.asarray(lanes, dtype=np.int64), np.asarray(known, dtype=bool)
    places = np.where(known, world.place[lanes], UNKNOWN)
    assert (places[known] != UNKNOWN).all()
    unk = lanes[~known]
    if known.all():
        return av.push_known(ag, places, engine=engine)
    return av.push_mixed(ag, places, world.rs[unk], world.pks[unk], world.msgs[unk], engine=engine)


def known_sets(n, B, rng):
    """name -> the known mask of a block of n lanes (all of them lanes the pool holds)"""
    idx = np.arange(n)
    sets = {"all": idx >= 0, "none": idx < 0, "every second": idx % 2 == 0, "random": rng.integers(0, 2, n) == 1}
    edges = sorted({0, n - 1, B - 1, B} & set(range(n)))                  # first, last, either side of a block edge
    for at in edges:
        sets["one unknown at %d" % at] = idx != at
        sets["one known at %d" % at] = idx == at
    return sets


def block_sizes(B):
    return sorted({1, 2, 3, B - 1, B, B + 1, 511, 512, 513, 1288})


def block_lanes(world, n):
    """a block of n lanes the pool holds, in an order of its own; above HELD lanes the first ones come again"""
    base = (np.arange(HELD) * 7 + 3) % HELD                                # a permutation: 7 and 1160 share no factor
    return np.resize(base, n)


def check_block(engine, world, av, ag, lanes, known, name, scalars=False):
    n = len(lanes)
    av.reset()
    assert push_block(av, ag, world, lanes, known) == n
    agg, body = world.ref(lanes), world.body(lanes)
    e = int.from_bytes(agg[49 * n:].tobytes(), "little")
    got, want = av.finish(agg[49 * n:]), engine.verify_aggregate(agg, body[1], body[2])
    s_got, s_want = av.known_sum(), world.known_sum(lanes, known)
    print("%s, %d lanes, %d known: finish %d, one-shot %d, S %s" % (name, n, int(np.sum(known)), got, want, hex(s_got)[:12]))
    assert got == want == OK, (name, n)
    assert s_got == s_want, (name, n)
    if scalars:
        for scalar in (e + 1, (Q - e) % Q):
            got = av.finish(scalar_bytes(scalar))
            assert got == INVALID == engine.verify_aggregate(with_e(agg, scalar_bytes(scalar)), body[1], body[2]), (name, n)
    info = av.info()
    assert info["held"] == n and info["pushed"] == n and info["pushes"] == 1 and info["blocks"] == n // info["block_lanes"]


# ---------------------------------------------------------------------------------------------- 1. blocks and known sets
@pytest.mark.parametrize("B,n", [(B, n) for B in (4, 64, 512) for n in block_sizes(B)])
def test_blocks_and_known_sets(engine, world, pool, B, n):
    rng = np.random.default_rng(B)
    lanes = block_lanes(world, n)
    with engine.aggregate_verifier(n, B) as av:
        for name, known in known_sets(n, B, rng).items():
            check_block(engine, world, av, pool, lanes, known, name, scalars=name in ("all", "every second"))


def test_no_known_lane_is_a_plain_push_word_for_word(engine, world, pool):
    for n in (1, 513, 1288):
        lanes = block_lanes(world, n)
        with engine.aggregate_verifier(n, 64) as av, engine.aggregate_verifier(n, 64) as plain:
            push_block(av, pool, world, lanes, np.zeros(n, bool))
            plain.push(*world.body(lanes))
            want = expected_record(engine, *world.body(lanes))
            assert (av.record() == want).all() and (plain.record() == want).all(), n
            assert av.known_sum() == 0 and av.finish(world.e(lanes)) == OK


def test_places_in_reversed_and_random_order_and_a_repeated_place(engine, world, pool):
    rng = np.random.default_rng(0x34)
    held = world.order                                                     # world lanes by pool place
    blocks = {"reversed": held[::-1][:700], "ascending": held[:600], "random": rng.permutation(held)[:515]}
    rep = np.array(held[:66])
    rep[65] = rep[2]                                                       # one lane twice, both known
    rep[64] = rep[3]                                                       # one lane twice, once known and once with the call
    with engine.aggregate_verifier(700, 64) as av:
        for name, lanes in blocks.items():
            for known in (np.ones(len(lanes), bool), np.arange(len(lanes)) % 3 != 1):
                check_block(engine, world, av, pool, lanes, known, name)
        known = np.ones(66, bool)
        check_block(engine, world, av, pool, rep, known, "repeated, both known")
        known[64] = False
        check_block(engine, world, av, pool, rep, known, "repeated, one of them unknown", scalars=True)


# ---------------------------------------------------------------------------------------------- 2. what must be refused
def test_wrong_blocks_are_invalid(engine, world, pool):
    n = 600
    lanes = block_lanes(world, n)
    known = np.arange(n) % 4 != 0
    agg, (rs, pks, msgs) = world.ref(lanes), world.body(lanes)
    with engine.aggregate_verifier(n, 64) as av:
        # an unknown lane's message byte changed
        places = np.where(known, world.place[lanes], UNKNOWN)
        unk = lanes[~known]
        m_bad = world.msgs[unk].copy()
        m_bad[7, 11] ^= 0x20
        av.push_mixed(pool, places, world.rs[unk], world.pks[unk], m_bad)
        msgs_bad = msgs.copy()
        msgs_bad[np.flatnonzero(~known)[7]] = m_bad[7]
        assert av.finish(agg[49 * n:]) == INVALID == engine.verify_aggregate(agg, pks, msgs_bad)
        # two known places swapped: the block is another one, and its honest scalar another
        av.reset()
        a, b = np.flatnonzero(known)[[5, 300]]
        swapped = lanes.copy()
        swapped[[a, b]] = swapped[[b, a]]
        push_block(av, pool, world, swapped, known)
        assert av.finish(agg[49 * n:]) == INVALID
        body = world.body(swapped)
        assert engine.verify_aggregate(np.concatenate([body[0].reshape(-1), agg[49 * n:]]), body[1], body[2]) == INVALID
        assert av.finish(world.e(swapped)) == OK
        # a non-canonical scalar, with and without an MSM
        assert av.finish(scalar_bytes(Q)) == MALFORMED
        av.reset()
        push_block(av, pool, world, lanes, np.ones(n, bool))
        assert av.finish(scalar_bytes(Q)) == MALFORMED and av.finish(agg[49 * n:]) == OK
        assert av.finish(scalar_bytes((int.from_bytes(agg[49 * n:].tobytes(), "little") + 1) % Q)) == INVALID


# ---------------------------------------------------------------------------------------------- 3. prefixes
@pytest.mark.parametrize("B", [4, 512])
def test_prefix_finishes_end_inside_a_mixed_push(engine, world, pool, B):
    """three pushes -- plain, mixed, known -- and prefixes that end inside each, descending first: a finish below the
    lanes held reduces a ragged block where the object holds a complete block's top"""
    lanes = block_lanes(world, 1100)
    cuts = [(0, 300, "plain"), (300, 900, "mixed"), (900, 1100, "known")]
    known = np.zeros(1100, bool)
    known[300:900] = np.arange(600) % 3 != 0
    known[900:] = True
    prefixes = [0, 1, 299, 300, 301, 302, 511, 512, 513, 899, 900, 901, 1099, 1100]
    with engine.aggregate_verifier(1100, B) as av:
        for lo, hi, how in cuts:
            if how == "plain":
                av.push(*world.body(lanes[lo:hi]))
            else:
                push_block(av, pool, world, lanes[lo:hi], known[lo:hi])
        rec = av.record()
        for n in prefixes[::-1] + prefixes:
            assert av.finish(world.e(lanes[:n]) if n else np.zeros(32, np.uint8), n) == OK, n
            assert av.known_sum(n) == world.known_sum(lanes[:n], known[:n]), n
            if n:
                assert av.finish(world.e(lanes[:n - 1]) if n > 1 else np.zeros(32, np.uint8), n) == INVALID, n
        assert (av.record() == rec).all() and av.info()["held"] == 1100
        # the record is the unknown lanes' alone: a prefix without a known lane gives the plain one
        assert (av.record(300) == expected_record(engine, *world.body(lanes[:300]))).all()
    # a prefix that ends in front of the push's first unknown lane: the host sizes the MSM for one row, the device lists
    # none, and the record of the empty rows is the identity
    with engine.aggregate_verifier(8, B) as av:
        push_block(av, pool, world, lanes[:5], np.array([True, True, True, False, True]))
        for n in (3, 2, 1, 5, 4):
            assert av.finish(world.e(lanes[:n]), n) == OK, n
            assert av.finish(world.e(lanes[:n + 1]), n) == INVALID, n
        assert not av.record(3)[:18].any()


# ---------------------------------------------------------------------------------------------- 4. three pieces
def tight_engine():
    import schnorr_sig_amd as ssa
    old = os.environ.get("SSA_MSM_SLICE")
    os.environ["SSA_MSM_SLICE"] = "512"
    try:
        return ssa.Engine(0)
    finally:
        if old is None:
            del os.environ["SSA_MSM_SLICE"]
        else:
            os.environ["SSA_MSM_SLICE"] = old


def test_more_unknown_lanes_than_one_msm_slice(world):
    """a context whose MSM slice is 512 lanes: 1288 lanes in pushes of at most 512, 1100 of them unknown, so finish runs the
    bucket pipeline in three pieces; then a bad unknown lane in the second piece"""
    tight = tight_engine()
    try:
        assert tight.info()["msm_slice"] == 512
        lanes = block_lanes(world, 1288)
        known = np.zeros(1288, bool)
        known[np.arange(0, 1288, 7)[:188]] = True                         # 188 known, 1100 unknown
        with world.new_pool(tight) as ag, tight.aggregate_verifier(1288, 64) as av:
            for spoil in (False, True):
                av.reset()
                rs, pks, msgs = (a.copy() for a in world.body(lanes))
                bad_at = np.flatnonzero(~known)[700]                       # unknown row 700: the second piece
                if spoil:
                    pks[bad_at, 48] ^= 0x01                                # key off the curve
                for lo in range(0, 1288, 500):
                    sl = slice(lo, min(lo + 500, 1288))
                    places = np.where(known[sl], world.place[lanes[sl]], UNKNOWN)
                    u = ~known[sl]
                    av.push_mixed(ag, places, rs[sl][u], pks[sl][u], msgs[sl][u])
                agg = world.ref(lanes)
                want = world.engine.verify_aggregate(agg, pks, msgs)
                assert av.finish(agg[49 * 1288:]) == want == (MALFORMED if spoil else OK)
                assert av.finish(world.e(lanes[:bad_at]), bad_at) == OK
                assert av.finish(world.e(lanes[:bad_at + 1]), bad_at + 1) == (MALFORMED if spoil else OK)
                if not spoil:                                              # (another key is another leaf, root and S)
                    assert av.known_sum() == world.known_sum(lanes, known)
            # above the slice: refused, nothing changed
            av.reset()
            with pytest.raises(RuntimeError):
                av.push_known(ag, world.place[lanes[:513]])
            assert av.info()["held"] == 0 and av.info()["pushes"] == 0
    finally:
        tight.close()


# ---------------------------------------------------------------------------------------------- 5. malformed classes
@pytest.mark.parametrize("what", ["non-canonical limb in R.x", "non-canonical limb in the key", "key off the curve",
                                  "R does not decode", "identity key, pk_inf set", "flag byte of R"])
def test_unknown_lanes_of_every_class_next_to_known_lanes(engine, world, pool, what):
    import pymodel as pm
    n, k = 130, 64                                                        # the bad lane: first of block 1, known on both sides
    lanes = block_lanes(world, n)
    known = np.ones(n, bool)
    known[[k, 5, 129]] = False
    sigs, pks, msgs = world.sigs[lanes].copy(), world.pks[lanes].copy(), world.msgs[lanes].copy()
    inf = np.zeros(n, np.uint8)
    e_agg, want = world.e(lanes), MALFORMED
    if what == "non-canonical limb in R.x":
        sigs[k, 8:16] = 0xFF
    elif what == "non-canonical limb in the key":
        pks[k, 56:64] = 0xFF
    elif what == "key off the curve":
        pks[k, 48] ^= 0x01
    elif what == "R does not decode":
        for t in range(1, 64):
            x = world.sigs[lanes[k], :49].copy()
            x[8] ^= t
            if pm.pt_decompress(x.tobytes())[0] == "invalid":
                break
        sigs[k, :49] = x
    elif what == "identity key, pk_inf set":
        e = make_scalars(np.random.default_rng(0x1D), 1)
        comp, st = engine.compress_many(engine.pubkey_many(e))
        assert (st == 0).all()
        sigs[k], pks[k], inf[k] = np.concatenate([comp[0], e[0]]), 0, 1
        st, agg, _, nf = engine.aggregate(sigs, pks, msgs, pk_inf=inf)
        assert st == OK and nf == 0
        e_agg, want = agg[49 * n:], OK
    else:
        sigs[k, 48] ^= 0x40
        want = INVALID
    rs = np.ascontiguousarray(sigs[:, :49])
    u = ~known
    with engine.aggregate_verifier(n, 64) as av:
        av.push_mixed(pool, np.where(known, world.place[lanes], UNKNOWN), rs[u], pks[u], msgs[u], pk_inf=inf[u])
        got = av.finish(e_agg)
        assert got == want == engine.verify_aggregate(np.concatenate([rs.reshape(-1), e_agg]), pks, msgs, pk_inf=inf), what
        assert av.finish(world.e(lanes[:k]), k) == OK                    # the lanes in front of it are untouched by it
        if want == MALFORMED:
            assert av.finish(world.e(lanes[:k + 1]), k + 1) == MALFORMED


# ---------------------------------------------------------------------------------------------- 6. every kind of push
def test_plain_cached_and_mixed_pushes_in_one_object(engine, world, pool):
    """every kind of push in one object, in both orders around the moments it becomes keyed and mixed: the known bytes of
    lanes pushed otherwise are zero, and the key status of every lane of a mixed push says "not checked".  The key
    verdict of section 29 is unchanged: the next test."""
    lanes = block_lanes(world, 900)
    rs, pks, msgs = world.body(lanes)
    known = np.zeros(900, bool)
    known[300:600] = np.arange(300) % 2 == 0
    with engine.keycache_create(1024) as cache, engine.aggregate_verifier(900, 4) as av:
        av.push(rs[:100], pks[:100], msgs[:100])                           # plain
        push_block(av, pool, world, lanes[100:200], np.ones(100, bool))   # known, before the object is keyed
        n_, stats = av.push(rs[200:300], pks[200:300], msgs[200:300], cache=cache)        # cached: keyed from here on
        push_block(av, pool, world, lanes[300:600], known[300:600])      # mixed into a keyed object
        av.push(rs[600:700], pks[600:700], msgs[600:700])                  # plain into a mixed, keyed object
        n_, stats = av.push(rs[700:900], pks[700:900], msgs[700:900], cache=cache)
        known[100:200] = True
        assert av.cached_lanes() == 300 and av.info()["held"] == 900
        for n in (900, 700, 650, 600, 450, 300, 250, 200, 150, 100, 99):
            assert av.finish(world.e(lanes[:n]), n) == OK, n
            assert av.known_sum(n) == world.known_sum(lanes[:n], known[:n]), n
        assert av.finish(world.e(lanes[:899])) == INVALID


def test_a_bad_key_decides_only_where_it_came_through_the_cache(engine, world, pool):
    """P + T2 in an unknown lane of a mixed push is "not checked" (the plain push's semantics); the same key pushed through
    a cache in front of the mixed push makes every prefix that reaches it INVALID_PUBLIC_KEY, known lanes or not"""
    import pymodel as pm
    BAD_KEY = 1
    lanes = block_lanes(world, 200)
    rs, pks, msgs = (a.copy() for a in world.body(lanes))
    pt = (pm.fp6_from_bytes48(bytes(pks[10, :48])), pm.fp6_from_bytes48(bytes(pks[10, 48:])))
    bad = pm.pt_add(pt, pm.SMALL_ORDER_POINTS[2])
    pks[10] = np.frombuffer(pm.fp6_to_bytes48(bad[0]) + pm.fp6_to_bytes48(bad[1]), np.uint8)
    known = np.arange(200) >= 50
    with engine.keycache_create(256) as cache, engine.aggregate_verifier(200, 64) as av:
        av.push(rs[:50], pks[:50], msgs[:50], cache=cache)
        push_block(av, pool, world, lanes[50:], known[50:])
        e = world.e(lanes)
        assert av.finish(e) == BAD_KEY and av.finish(world.e(lanes[:10]), 10) == OK
        assert av.finish(world.e(lanes[:120]), 120) == BAD_KEY
        av.reset()
        av.push(rs[:50], pks[:50], msgs[:50])                              # the same lanes, not checked
        push_block(av, pool, world, lanes[50:], known[50:])
        one_shot = engine.verify_aggregate(np.concatenate([rs.reshape(-1), e]), pks, msgs)
        assert av.finish(e) == one_shot and one_shot in (OK, INVALID)


# ---------------------------------------------------------------------------------------------- 7. the pool moves on
def test_the_verifier_holds_copies(engine, world):
    lanes = block_lanes(world, 700)
    known = np.arange(700) % 5 != 0
    with world.new_pool() as ag, engine.aggregate_verifier(700, 64) as av:
        push_block(av, ag, world, lanes, known)
        e, rec, s = world.e(lanes), av.record(), av.known_sum()
        assert av.finish(e) == OK and s == world.known_sum(lanes, known)
        drop = np.zeros(HELD, np.uint8)
        drop[::3] = 1
        kept = ag.remove(drop)
        ag.drop_front(100)
        assert ag.info()["held"] == kept - 100
        engine.debug_poison_workspaces(0x3C)
        assert av.finish(e) == OK and av.known_sum() == s and (av.record() == rec).all()
        assert av.finish(world.e(lanes[:512]), 512) == OK


# ---------------------------------------------------------------------------------------------- 8. no state in workspaces
def test_state_does_not_live_in_workspaces(engine, world, pool):
    other = np.arange(HELD, WORLD)
    agg_other = world.ref(other)

    def disturb(step):
        engine.debug_poison_workspaces(0xA5)
        if step % 3 == 0:
            status, nf = engine.verify_many(world.sigs[other], world.pks[other], world.msgs[other])
            assert nf == 0 and not status.any()
        elif step % 3 == 1:
            assert engine.verify_aggregate(agg_other, world.pks[other], world.msgs[other]) == OK
        else:
            assert (pool.finish_bytes(300)[:49] == world.rs[world.order[0]]).all()
        engine.debug_poison_workspaces(0x5A)

    la, lb = block_lanes(world, 800), block_lanes(world, 1160)[400:1100]
    ka, kb = np.arange(800) % 2 == 1, np.arange(700) % 7 != 0
    with engine.aggregate_verifier(800, 512) as a, engine.aggregate_verifier(700, 8) as b:
        for j, (lo, hi) in enumerate(((0, 250), (250, 513), (513, 800))):
            push_block(a, pool, world, la[lo:hi], ka[lo:hi])
            disturb(j)
            push_block(b, pool, world, lb[lo:min(hi, 700)], kb[lo:min(hi, 700)])
            disturb(j + 1)
            assert a.finish(world.e(la[:hi]), hi) == OK
            disturb(j + 2)
        assert b.finish(world.e(lb)) == OK and b.finish(world.e(la[:700])) == INVALID
        disturb(0)
        assert a.known_sum() == world.known_sum(la, ka) and b.known_sum(513) == world.known_sum(lb[:513], kb[:513])
        assert a.finish(world.e(la)) == OK


# ---------------------------------------------------------------------------------------------- 9. host refusals
def test_host_refusals_change_nothing(engine, world, pool):
    import schnorr_sig_amd as ssa
    lanes = block_lanes(world, 12)
    known = np.arange(12) % 2 == 0
    with engine.aggregate_verifier(10, 4) as av:
        push_block(av, pool, world, lanes[:6], known[:6])
        info, rec = av.info(), av.record()
        unchanged = lambda: av.info() == info and (av.record() == rec).all()
        body = lambda k: (world.rs[HELD:HELD + k], world.pks[HELD:HELD + k], world.msgs[HELD:HELD + k])
        with pytest.raises(RuntimeError):
            av.push_known(pool, [HELD])                                   # a place the pool does not hold
        with pytest.raises(RuntimeError):
            av.push_known(pool, [0, 2 ** 32 - 2])
        assert unchanged()
        with pytest.raises(RuntimeError):
            av.push_mixed(pool, [0, None, None], *body(1))                # two sentinels, one lane
        with pytest.raises(RuntimeError):
            av.push_mixed(pool, [0, 1, None], *body(2))                   # one sentinel, two lanes
        with pytest.raises(RuntimeError):
            av.push_known(pool, [0, None])
        assert unchanged()
        with pytest.raises(RuntimeError):
            av.push_known(pool, [0, 1, 2, 3, 4])                          # 5 lanes, room for 4
        assert unchanged()
        other = ssa.Engine(0)
        try:
            with pytest.raises(RuntimeError):
                av.push_known(pool, [0], engine=other)                    # a context other than the objects'
            with other.aggregator(8) as ag2:
                with pytest.raises(RuntimeError):
                    av.push_known(ag2, [], engine=engine)                 # a pool of another context
                with pytest.raises(RuntimeError):
                    av.push_known(ag2, [], engine=other)
        finally:
            other.close()
        assert unchanged()
        m = np.zeros((1, 4), np.uint8)
        rc = ssa._lib.ssa_aggverifier_push_mixed(engine._ctx, av.handle, pool.handle, ssa._ptr(np.array([UNKNOWN], np.uint32)), 1,
                                                 ssa._ptr(world.rs[:1]), ssa._ptr(world.pks[:1]), None, ssa._ptr(m), None, 2, 4, 1)
        assert rc == ssa.ERR_ARG and unchanged()                          # a message stride below the length
        assert av.push_known(pool, []) == 0                               # an empty push still counts, and changes no lane
        assert av.info()["pushes"] == info["pushes"] + 1 and (av.record() == rec).all()
        push_block(av, pool, world, lanes[6:10], known[6:10])             # exactly fills the capacity
        assert av.finish(world.e(lanes[:10])) == OK
    orphan_eng = ssa.Engine(0)
    ag3, av3 = orphan_eng.aggregator(8), orphan_eng.aggregate_verifier(8)
    orphan_eng.close()                                                    # the context is gone: the handles are refused
    assert ssa._lib.ssa_aggverifier_push_known(engine._ctx, av3.handle, ag3.handle, None, 0) == ssa.ERR_ARG
    ag3.close()
    av3.close()


# ---------------------------------------------------------------------------------------------- 10. device forms
def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def test_device_forms_write_the_result_word_alone(engine, world, pool):
    import torch
    lanes = block_lanes(world, 700)
    known = np.arange(700) % 3 != 0
    places = np.where(known, world.place[lanes], UNKNOWN).astype(np.uint32)
    unk = lanes[~known]
    d_rs, d_pks, d_msgs = dev(world.rs[unk]), dev(world.pks[unk]), dev(world.msgs[unk])
    with engine.aggregate_verifier(1400, 64) as av:
        words = torch.full((8,), 0x6EEEEEEE, dtype=torch.int32, device="cuda:0")
        d_places = dev(places.view(np.int32))
        torch.cuda.synchronize()
        assert av.push_mixed_device(pool, d_places, words[3:4], d_rs, d_pks, d_msgs) == 700
        d_known = dev(world.place[lanes].astype(np.uint32).view(np.int32))
        torch.cuda.synchronize()
        assert av.push_known_device(pool, d_known, words[5:6]) == 700
        engine.sync()
        got = words.cpu().numpy()
        assert got[3] == 0 and got[5] == 0 and (np.delete(got, [3, 5]) == 0x6EEEEEEE).all(), got
        both = np.concatenate([lanes, lanes])
        assert av.finish(world.e(both)) == OK and av.finish(world.e(lanes), 700) == OK
        assert av.known_sum() == world.known_sum(both, np.concatenate([known, np.ones(700, bool)]))
        d_e, verdict = dev(np.array(world.e(both))), torch.full((4,), 0x6EEEEEEE, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        av.finish_device(d_e, verdict[1:2])
        engine.sync()
        assert verdict.cpu().numpy().tolist() == [0x6EEEEEEE, OK, 0x6EEEEEEE, 0x6EEEEEEE]


@pytest.mark.parametrize("what", ["place == held", "place capacity - 1 after a remove", "sentinel count above u",
                                  "sentinel count below u"])
def test_device_refusals_fail_closed(engine, world, what):
    """the device decides and fails closed: the result word is 1, every prefix that reaches a refused lane answers
    MALFORMED -- the status of a lane that failed a check --, the words next to the result word are untouched, and after a
    reset the object serves a valid call"""
    import torch
    lanes = world.order[(np.arange(300) * 7 + 3) % 300]                   # the lanes at places 0 .. 299, in another order
    known = np.arange(300) % 4 != 1
    places = np.where(known, world.place[lanes], UNKNOWN).astype(np.uint32)
    unk = lanes[~known]
    u, first_bad = len(unk), 0
    with world.new_pool() as ag, engine.aggregate_verifier(600, 64) as av:
        if what == "place == held":
            places[200], first_bad = HELD, 200
        elif what == "place capacity - 1 after a remove":
            drop = np.zeros(HELD, np.uint8)
            drop[HELD - 40:] = 1                                           # the last 40 places leave: no place in front moves
            assert ag.remove(drop) == HELD - 40
            places[200], first_bad = HELD - 1, 200                         # held lanes once, beyond `held` now
        elif what == "sentinel count above u":
            places[2] = UNKNOWN                                            # one sentinel more than the call brings
        else:
            places[np.flatnonzero(~known)[0]] = world.place[lanes[0]]      # one sentinel fewer
        push_block(av, ag, world, lanes[:100], known[:100])                # a valid push in front
        words = torch.full((8,), 0x6EEEEEEE, dtype=torch.int32, device="cuda:0")
        d_places, d_rs, d_pks, d_msgs = dev(places.view(np.int32)), dev(world.rs[unk]), dev(world.pks[unk]), dev(world.msgs[unk])
        torch.cuda.synchronize()
        assert av.push_mixed_device(ag, d_places, words[3:4], d_rs, d_pks, d_msgs) == 300
        engine.sync()
        got = words.cpu().numpy()
        assert got[3] == 1 and (np.delete(got, 3) == 0x6EEEEEEE).all(), got
        assert av.info()["held"] == 400
        e_front = world.e(lanes[:100])
        assert av.finish(e_front, 100) == OK                              # the lanes in front are untouched
        for n in (100 + first_bad + 1, 400):
            for scalar in (e_front, np.zeros(32, np.uint8), scalar_bytes(1)):
                assert av.finish(scalar, n) == MALFORMED, (what, n)
        if first_bad:                                                     # a refused place spoils its own lane alone
            both = np.concatenate([lanes[:100], lanes[:first_bad]])
            assert av.finish(world.e(both), 100 + first_bad) == OK
        av.reset()
        if what == "place capacity - 1 after a remove":
            assert av.push_known(ag, world.place[lanes[:64]]) == 64 and av.finish(world.e(lanes[:64])) == OK
        else:
            push_block(av, ag, world, lanes, known)
            assert av.finish(world.e(lanes)) == OK


# ---------------------------------------------------------------------------------------------- 11. the unused path
def test_plain_pushes_launch_none_of_the_new_kernels(world):
    import schnorr_sig_amd as ssa
    eng = ssa.Engine(0)
    lanes = np.arange(600)
    try:
        with eng.aggregate_verifier(600, 64) as av:
            eng.enable_timing(True)
            names = NEW_KERNELS + ("ssa_k_hash", "ag_k_expand", "agv_k_append", "agv_k_scalars", "ag_k_finish", "av_k_keep")
            for name in names:
                eng.read_timing(name)                                     # drains the key
            av.push(*world.body(lanes[:300]))
            av.push(*world.body(lanes[300:]))
            assert av.finish(world.e(lanes)) == OK and av.finish(world.e(lanes[:64]), 64) == OK
            counts = {name: eng.read_timing(name)[1] for name in names}
            assert all(counts[name] == 0 for name in NEW_KERNELS + ("av_k_keep",)), counts
            assert (counts["ssa_k_hash"], counts["ag_k_expand"], counts["agv_k_append"]) == (2, 2, 2), counts
            assert (counts["agv_k_scalars"], counts["ag_k_finish"]) == (2, 2), counts
            # and the mixed path is the one that launches them
            with world.new_pool(eng) as ag:
                av.reset()
                for name in names:
                    eng.read_timing(name)
                push_block(av, ag, world, lanes, np.arange(600) % 2 == 0)
                assert av.finish(world.e(lanes)) == OK
                counts = {name: eng.read_timing(name)[1] for name in names}
                assert all(counts[name] == 1 for name in NEW_KERNELS), counts
                assert (counts["agv_k_append"], counts["agv_k_scalars"], counts["ssa_k_hash"]) == (0, 0, 1), counts
            eng.enable_timing(False)
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------- 12. the C++ mirror
def test_cxx_mirror_gives_the_python_mirrors_bytes(engine, world, tmp_path):
    libdir = os.path.join(ROOT, "schnorr-sig_amd", "csrc")
    exe = str(tmp_path / "aggverifier_mixed_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                           os.path.join(ROOT, "tests", "csrc", "aggverifier_mixed_driver.cpp"), "-L" + libdir,
                           "-lschnorr_sig_amd", "-Wl,-rpath," + libdir, "-L/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    p, n = 300, 200
    held = np.arange(p)[::-1]                                             # the pool: world lanes p-1 .. 0, one screened push
    place = {int(w): at for at, w in enumerate(held)}
    lanes = (np.arange(n) * 3 + 1) % p
    known = np.arange(n) % 3 != 0
    cuts = [(0, 70), (70, 130), (130, 200)]
    known[70:130] = True                                                  # the middle push: push_known
    ALL = (1 << 64) - 1
    e_all = np.array(world.e(lanes))
    finishes = [(ALL, e_all), (n, e_all), (100, np.array(world.e(lanes[:100]))), (100, e_all), (0, np.zeros(32, np.uint8)),
                (n, scalar_bytes(Q))]
    blob = struct.pack("<Q", p) + world.sigs[held].tobytes() + world.pks[held].tobytes()
    blob += struct.pack("<%dQ" % p, *([80] * p)) + world.msgs[held].tobytes() + struct.pack("<Q", POOL_B)
    blob += struct.pack("<3Q", n, 64, len(cuts))
    with engine.aggregator(p, POOL_B) as ag, engine.aggregate_verifier(n, 64) as av:
        status, kept = ag.push(world.sigs[held], world.pks[held], world.msgs[held])
        assert kept == p
        for lo, hi in cuts:
            pl = np.array([place[int(w)] if k else UNKNOWN for w, k in zip(lanes[lo:hi], known[lo:hi])], dtype=np.uint32)
            unk = lanes[lo:hi][~known[lo:hi]]
            if len(unk):
                av.push_mixed(ag, pl, world.rs[unk], world.pks[unk], world.msgs[unk])
            else:
                av.push_known(ag, pl)
            blob += struct.pack("<Q", hi - lo) + pl.tobytes() + struct.pack("<Q", len(unk))
            blob += world.rs[unk].tobytes() + world.pks[unk].tobytes()
            blob += struct.pack("<%dQ" % len(unk), *([80] * len(unk))) + world.msgs[unk].tobytes()
        got = [av.finish(e, None if take == ALL else take) for take, e in finishes]
        assert got == [OK, OK, OK, INVALID, OK, MALFORMED]
        info = av.info()
    blob += struct.pack("<Q", len(finishes)) + b"".join(struct.pack("<Q", take) + e.tobytes() for take, e in finishes)
    want = status.tobytes() + struct.pack("<%di" % len(got), *got)
    want += struct.pack("<8Q", info["held"], info["capacity"], info["block_lanes"], info["pushes"], info["pushed"],
                        info["reserved"], info["blocks"], info["finishes"])
    path, outp = str(tmp_path / "cases.bin"), str(tmp_path / "out.bin")
    with open(path, "wb") as f:
        f.write(blob)
    r = subprocess.run([exe, path, outp], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    got = open(outp, "rb").read()
    assert len(got) == len(want) and got == want
