"""The leaf column and the leaf index of the streaming aggregator (ssa_aggregator_leaves*, ssa_aggregator_lookup*,
ssa_aggregator_index_sync / _info).  Three things are held here:

    the column    leaves() is the transcript's leaf of every admitted lane, byte for byte (tests/aggregate_model.py over
                  the C oracle), in arrival order; leaves_select is numpy indexing of it;
    the index     lookup(ids) is a Python dictionary leaf -> lowest place, built from leaves() AFTER every change of the
                  pool; with the default probe bound every held id is found (index_info()["overflowed"] == 0), so no
                  case can hide behind "unknown"; with a bound of one slot a returned place is still always right;
    the reason    ids -> places on the device -> a mixed push through the key cache -> the verdict of the one-shot
                  cached call on the whole block.
"""
import ctypes as C

import numpy as np
import pytest

import aggregate_model as am
from aggregate_model import Q
from test_gpu_aggverifier import make_scalars, scalar_bytes

pytestmark = pytest.mark.gpu

OK, BAD_KEY, INVALID, MALFORMED = 0, 1, 2, 3
UNKNOWN = 0xFFFFFFFF
BLOCK, OTHERS = 1288, 312                            # the lanes a block is made of; lanes no block holds
WORLD = BLOCK + OTHERS
POOL_B, CAPACITY = 8, 2048
DISTINCT, DOUBLED = 1140, 20                         # the pool: 1140 world lanes, then the first 20 of them again
HELD = DISTINCT + DOUBLED
KINDS = ["plain", "keyed"]
NS = [1, 2, 3, 63, 64, 65, 1160, 1288]


def dev(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    torch.cuda.synchronize()
    return t


def id_of(rows):
    return [r.tobytes() for r in np.asarray(rows, np.uint8).reshape(-1, 32)]


def dictionary(leaves):
    """leaf -> the lowest place that holds it"""
    d = {}
    for p, leaf in enumerate(id_of(leaves)):
        d.setdefault(leaf, p)
    return d


def expected(d, ids):
    want = np.array([d.get(x, UNKNOWN) for x in id_of(ids)], dtype=np.uint32)
    return want, int((want == UNKNOWN).sum())


class World:
    """WORLD honest signatures over 80-byte messages by 64 signers (the lanes behind BLOCK: a signer each), their wire
    keys and records, and the model's leaf of every lane, computed once and never changed"""

    def __init__(self, engine, oracle):
        rng = np.random.default_rng(0xA636)
        self.engine = engine
        self.msgs = rng.integers(0, 256, size=(WORLD, 80), dtype=np.uint8)
        w = np.arange(WORLD)
        sks = make_scalars(rng, 64 + OTHERS)[np.where(w < BLOCK, w % 64, 64 + w - BLOCK)]
        self.pks, self.sigs = engine.keygen_sign_many(sks, make_scalars(rng, WORLD), self.msgs)
        self.wire, st = engine.compress_many(self.pks)
        assert (st == 0).all()
        self.rs = np.ascontiguousarray(self.sigs[:, :49])
        self.keyed = np.ascontiguousarray(np.concatenate([self.wire, self.sigs], axis=1))
        felts = am.leaves(am.oracle_backend(oracle), list(self.rs), list(self.pks), list(self.msgs))
        self.leaves = np.array(felts, dtype=np.uint64).view(np.uint8).reshape(WORLD, 32)
        self.leaves.setflags(write=False)
        assert len(set(id_of(self.leaves))) == WORLD
        self.order = np.concatenate([rng.permutation(DISTINCT), np.arange(DOUBLED)])      # world lane by place
        self.absent = rng.integers(0, 256, size=(BLOCK, 32), dtype=np.uint8)              # ids nobody holds
        self._refs = {}

    def fill(self, ag, kind, lanes, eng=None):
        """admits the world lanes `lanes`, in that order"""
        eng = eng or self.engine
        lanes = np.asarray(lanes, dtype=np.int64)
        if kind == "keyed":
            with eng.keycache_create(256, wire=True) as cache:
                status, kept, _ = ag.push_keyed(cache, self.keyed[lanes], self.msgs[lanes])
        else:
            half = (len(lanes) + 1) // 2
            a, b = lanes[:half], lanes[half:]
            status, kept = ag.push(self.sigs[a], self.pks[a], self.msgs[a])                # the screened push
            assert kept == len(a) and not status.any()
            if len(b):
                with eng.keycache_create(256) as cache:
                    status, kept, _ = ag.push(self.sigs[b], self.pks[b], self.msgs[b], cache=cache)
                assert kept == len(b)
            return
        assert kept == len(lanes) and not status.any()

    def new_pool(self, kind, eng=None, lanes=None, capacity=CAPACITY, index=True):
        eng = eng or self.engine
        ag = eng.aggregator(capacity, POOL_B, hold_keys=(kind == "keyed"), hold_admission=True, index=index)
        self.fill(ag, kind, self.order if lanes is None else lanes, eng)
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
        return self.ref(lanes)[49 * len(lanes):]


@pytest.fixture(scope="module")
def world(engine, oracle):
    return World(engine, oracle)


@pytest.fixture(scope="module")
def pools(world):
    made = {kind: world.new_pool(kind) for kind in KINDS}
    yield made
    for ag in made.values():
        ag.close()


def lookup_device(ag, ids, offset=0):
    """the device form with the ids at `offset` bytes behind an aligned base -> (places, count), read back"""
    import torch
    ids = np.ascontiguousarray(ids, np.uint8).reshape(-1)
    n = ids.size // 32
    d_raw = torch.full((ids.size + 16,), 0xEE, dtype=torch.uint8, device="cuda:0")
    d_raw[offset:offset + ids.size] = torch.from_numpy(ids).to("cuda:0")
    d_places = torch.full((n + 2,), 0x6EEEEEEE, dtype=torch.int32, device="cuda:0")
    d_count = torch.full((3,), 0x6EEEEEEE, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    assert d_raw.data_ptr() % 8 == 0
    assert ag.lookup_device(d_raw[offset:offset + ids.size], d_places[1:n + 1], d_count[1:2]) == n
    ag.engine.sync()
    places, count = d_places.cpu().numpy().view(np.uint32), d_count.cpu().numpy()
    assert places[0] == places[n + 1] == 0x6EEEEEEE and count[0] == count[2] == 0x6EEEEEEE      # nothing beside the outputs
    return places[1:n + 1].copy(), int(count[1])


def check_lookup(ag, ids, d=None, forms=("host", "device"), what=None):
    d = dictionary(ag.leaves()) if d is None else d
    want, unknown = expected(d, ids)
    for form in forms:
        got = ag.lookup(ids) if form == "host" else lookup_device(ag, ids)
        assert got[1] == unknown and (got[0] == want).all(), (what, form, got[1], unknown)
    return want, unknown


# ---------------------------------------------------------------------------------------------- 1. the column
@pytest.mark.parametrize("kind", KINDS)
def test_leaves_are_the_models(world, pools, kind):
    import torch
    ag = pools[kind]
    want = world.leaves[world.order]
    got = ag.leaves()
    assert got.shape == (HELD, 32) and (got == want).all()
    assert (ag.leaves(HELD - 1) == want[:HELD - 1]).all() and ag.leaves(0).shape == (0, 32) and (ag.leaves(1) == want[:1]).all()
    with pytest.raises(RuntimeError):
        ag.leaves(HELD + 1)
    d_out = torch.full((32 * 100 + 8,), 0xEE, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    assert ag.leaves_device(d_out[3:], 100) == 100
    ag.engine.sync()
    raw = d_out.cpu().numpy()
    assert (raw[3:3203].reshape(100, 32) == want[:100]).all() and (raw[:3] == 0xEE).all() and (raw[3203:] == 0xEE).all()


@pytest.mark.parametrize("kind", KINDS)
def test_leaves_select_is_indexing(world, pools, kind):
    import torch
    import schnorr_sig_amd as ssa
    ag, rng = pools[kind], np.random.default_rng(361)
    col = world.leaves[world.order]
    orders = {"reversed": np.arange(HELD)[::-1].copy(), "random": rng.permutation(HELD), "one": np.array([HELD - 1]),
              "a place twice": np.array([5, 7, 5, 5]), "short": rng.permutation(HELD)[:257]}
    for name, order in orders.items():
        assert (ag.leaves_select(order) == col[order]).all(), name
        d_order = dev(order.astype(np.int32))
        d_out = torch.full((32 * len(order) + 9,), 0xEE, dtype=torch.uint8, device="cuda:0")
        d_res = torch.full((3,), 0x6EEEEEEE, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        assert ag.leaves_select_device(d_order, d_out[1:], d_res[1:2]) == len(order)        # the output at an odd address
        ag.engine.sync()
        raw, res = d_out.cpu().numpy(), d_res.cpu().numpy()
        assert (raw[1:1 + 32 * len(order)].reshape(-1, 32) == col[order]).all(), name
        assert raw[0] == 0xEE and (raw[1 + 32 * len(order):] == 0xEE).all() and list(res) == [0x6EEEEEEE, 0, 0x6EEEEEEE]
    assert ag.leaves_select([]).shape == (0, 32)
    # an index == held: refused, the output zeroed, result word 1; the object serves the next call
    for bad in (np.array([3, HELD, 4], np.uint32), np.array([HELD], np.uint32), np.array([0, 1, 0xFFFFFFFF], np.uint32)):
        out = np.full((len(bad), 32), 0xEE, dtype=np.uint8)
        rc = ssa._lib.ssa_aggregator_leaves_select(ag.engine._ctx, ag.handle, ssa._ptr(bad), len(bad), ssa._ptr(out))
        assert rc == ssa.ERR_ARG and not out.any()
        with pytest.raises(RuntimeError):
            ag.leaves_select(bad)
        d_out = torch.full((32 * len(bad) + 8,), 0xEE, dtype=torch.uint8, device="cuda:0")
        d_res = torch.full((1,), 0x6EEEEEEE, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        ag.leaves_select_device(dev(bad.view(np.int32)), d_out, d_res)
        ag.engine.sync()
        raw = d_out.cpu().numpy()
        assert int(d_res.cpu()[0]) == 1 and not raw[:32 * len(bad)].any() and (raw[32 * len(bad):] == 0xEE).all()
    assert (ag.leaves_select([HELD - 1, 0]) == col[[HELD - 1, 0]]).all()


# ---------------------------------------------------------------------------------------------- 2. the index
def id_sets(world, n, rng):
    """n ids each: world lanes the pool holds, ids nobody holds, and mixtures"""
    held_lanes = np.resize(rng.permutation(DISTINCT), n)
    held = world.leaves[held_lanes]
    absent = world.absent[:n]
    idx = np.arange(n)
    sets = {"all held": held, "none held": absent, "every second": np.where((idx % 2 == 0)[:, None], held, absent),
            "random": np.where((rng.integers(0, 2, n) == 1)[:, None], held, absent),
            "not in the pool": np.resize(world.leaves[DISTINCT:BLOCK], (n, 32)),
            "the doubled ones": np.resize(world.leaves[:DOUBLED], (n, 32)),
            "one id repeated": np.repeat(world.leaves[7:8], n, axis=0)}
    return sets


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("kind", KINDS)
def test_lookup_is_the_dictionary(world, pools, kind, n):
    ag, rng = pools[kind], np.random.default_rng(3620 + n)
    d = dictionary(world.leaves[world.order])
    assert len(d) == DISTINCT
    for name, ids in id_sets(world, n, rng).items():
        want, unknown = check_lookup(ag, ids, d, what=(name, n))
        if name in ("all held", "the doubled ones", "one id repeated"):
            assert unknown == 0
        if name in ("none held", "not in the pool"):
            assert unknown == n
        if name == "the doubled ones":                                     # two places hold the leaf: the lower one
            assert (want < DISTINCT).all()
            assert (world.order[want] == np.resize(np.arange(DOUBLED), n)).all()
    info = ag.index_info()
    assert info["overflowed"] == 0 and info["stale"] == 0 and info["indexed"] == HELD
    assert info["slots"] == 8192


@pytest.mark.parametrize("kind", KINDS)
def test_one_changed_bit_in_any_word_is_unknown(world, pools, kind):
    ag = pools[kind]
    base = world.leaves[world.order[:64]].copy()
    ids = [base]
    for word in range(4):
        for bit in (0, 31, 63):
            x = base.copy()
            x[:, 8 * word + bit // 8] ^= 1 << (bit % 8)
            ids.append(x)
    ids = np.concatenate(ids)
    places, unknown = ag.lookup(ids)
    assert (places[:64] == np.arange(64)).all() and (places[64:] == UNKNOWN).all() and unknown == len(ids) - 64
    got = lookup_device(ag, ids)
    assert (got[0] == places).all() and got[1] == unknown


@pytest.mark.parametrize("kind", KINDS)
def test_device_ids_at_any_byte_offset(world, pools, kind):
    ag, rng = pools[kind], np.random.default_rng(77)
    ids = np.where((rng.integers(0, 2, 700) == 1)[:, None], world.leaves[rng.permutation(BLOCK)[:700]], world.absent[:700])
    want, unknown = expected(dictionary(world.leaves[world.order]), ids)
    assert 0 < unknown < 700
    for offset in (0, 1, 7, 8):
        got = lookup_device(ag, ids, offset)
        assert (got[0] == want).all() and got[1] == unknown, offset


def test_no_ids_and_too_many(world, pools):
    import torch
    import schnorr_sig_amd as ssa
    ag = pools["plain"]
    before = ag.index_info()
    places, unknown = ag.lookup(np.zeros((0, 32), np.uint8))
    assert places.size == 0 and unknown == 0
    d_count = torch.full((1,), 77, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    assert ag.lookup_device(torch.zeros(0, dtype=torch.uint8, device="cuda:0"), torch.zeros(1, dtype=torch.int32, device="cuda:0"),
                            d_count) == 0
    ag.engine.sync()
    assert int(d_count.cpu()[0]) == 0
    assert ag.index_info() == before                                       # n == 0 launches nothing and counts nothing
    word = np.zeros(4, np.uint32)
    count = C.c_uint64(9)
    rc = ssa._lib.ssa_aggregator_lookup(ag.engine._ctx, ag.handle, ssa._ptr(word), (1 << 30) + 1, ssa._ptr(word), C.byref(count))
    assert rc == ssa.ERR_ARG and count.value == 9 and not word.any()


# ---------------------------------------------------------------------------------------------- 3. small and full tables
@pytest.mark.parametrize("kind", KINDS)
def test_small_and_full_tables(engine, world, kind):
    with world.new_pool(kind, lanes=world.order[:1], capacity=256) as ag:
        assert ag.index_info()["slots"] == 1024 and ag.index_info()["stale"] == 1
        check_lookup(ag, world.leaves[world.order[:5]])
        world.fill(ag, kind, world.order[1:256])
        assert ag.info()["held"] == 256
        ids = np.concatenate([world.leaves[world.order[:300]], world.absent[:40]])
        want, unknown = check_lookup(ag, ids)
        assert unknown == 44 + 40 and (want[:256] == np.arange(256)).all()
        info = ag.index_info()
        assert info["indexed"] == 256 and info["overflowed"] == 0 and info["rebuilds"] == 1
    with world.new_pool(kind, lanes=world.order[:1], capacity=1) as ag:
        assert ag.index_info()["slots"] == 1024
        want, unknown = check_lookup(ag, world.leaves[world.order[:3]])
        assert list(want) == [0, UNKNOWN, UNKNOWN] and unknown == 2


# ---------------------------------------------------------------------------------------------- 4. the state machine
@pytest.mark.parametrize("kind", KINDS)
def test_the_index_follows_every_change_of_the_pool(engine, world, kind):
    """after each change a FRESH dictionary from leaves(); the default bound: every held id is found"""
    rng = np.random.default_rng(364)
    probe = np.concatenate([world.leaves[:BLOCK], world.absent[:50]])       # every id a block may hold, and some nobody holds
    with world.new_pool(kind) as ag:
        lanes = world.order.copy()                                          # the model: world lane by place

        def check(what, sync=False):
            assert (ag.leaves() == world.leaves[lanes]).all(), what
            if sync:
                ag.index_sync()
            want, unknown = check_lookup(ag, probe, what=what)
            held_ids = set(id_of(world.leaves[lanes]))
            assert unknown == sum(1 for x in id_of(probe) if x not in held_ids), what
            info = ag.index_info()
            assert info["overflowed"] == 0 and info["stale"] == 0 and info["indexed"] == len(lanes) == ag.info()["held"], what
            return info
        first = check("filled")
        assert first["rebuilds"] == 1
        more = np.arange(DISTINCT, DISTINCT + 100)
        world.fill(ag, kind, more)
        lanes = np.concatenate([lanes, more])
        assert ag.index_info()["indexed"] == HELD                          # a push does no index work
        info = check("a further push")
        assert info["rebuilds"] == first["rebuilds"]                       # incremental
        for k in (POOL_B, POOL_B + 1):
            ag.drop_front(k)
            lanes = lanes[k:]
            info = ag.index_info()
            assert info["stale"] == 1 and info["indexed"] == 0 and info["overflowed"] == 0
            check("drop_front(%d)" % k, sync=(k == POOL_B))
        assert ag.index_info()["rebuilds"] == first["rebuilds"] + 2
        drop = (np.arange(len(lanes)) % 2 == 1).astype(np.uint8)
        assert ag.remove_device(dev(drop)) == int((drop == 0).sum())
        lanes = lanes[drop == 0]
        check("every second, by a mask on the device")
        gone = rng.permutation(len(lanes))[:len(lanes) // 3]
        keep = np.ones(len(lanes), bool)
        keep[gone] = False
        assert ag.remove_indices(gone) == int(keep.sum())
        lanes = lanes[keep]
        check("a random third", sync=True)
        rebuilds = ag.index_info()["rebuilds"]
        ag.index_sync()                                                    # nothing to do: no clear, no insert
        assert ag.remove(np.zeros(len(lanes), np.uint8)) == len(lanes)     # a removal that removes nothing
        info = ag.index_info()
        assert info["rebuilds"] == rebuilds and info["stale"] == 0 and info["indexed"] == len(lanes)
        taken = ag.take(101)
        assert taken.bytes == world.ref(lanes[:101]).tobytes()
        lanes = lanes[101:]
        check("take(101)")
        ag.reset()
        assert ag.index_info()["stale"] == 1 and ag.lookup(probe[:10])[1] == 10
        world.fill(ag, kind, world.order[:40])
        lanes = world.order[:40]
        check("reset, then a push")


# ---------------------------------------------------------------------------------------------- 5. a probe bound of one slot
def test_with_a_bound_of_one_slot_the_index_fails_open(world):
    """a FRESH engine whose walks are one slot long: 1140 distinct lanes in 8192 slots.  Every place returned holds the
    id; the held ids answered unknown are exactly the lanes counted as overflowed -- at least one (no collision among
    1140 keys in 8192 slots: below 2^-80) and fewer than half; a mixed push with those places gives the one-shot verdict"""
    import schnorr_sig_amd as ssa
    eng = ssa.Engine(0)
    try:
        eng.debug_dedup_config(0, 1)
        lanes = world.order[:DISTINCT]
        with eng.aggregator(CAPACITY, POOL_B, hold_admission=True, index=True) as ag, eng.aggregate_verifier(BLOCK, 64) as av:
            status, kept = ag.push(world.sigs[lanes], world.pks[lanes], world.msgs[lanes])
            assert kept == DISTINCT
            col = ag.leaves()
            assert (col == world.leaves[lanes]).all()
            block = np.arange(BLOCK)
            ids = world.leaves[block]
            for form in ("host", "device"):
                places, unknown = ag.lookup(ids) if form == "host" else lookup_device(ag, ids)
                found = places != UNKNOWN
                assert unknown == int((~found).sum())
                assert (col[places[found]] == ids[found]).all()            # a returned place holds the id (distinct: the lowest)
                held = np.isin(block, lanes)
                assert not found[~held].any()
                lost = int((held & ~found).sum())
                info = ag.index_info()
                assert lost == info["overflowed"] and 1 <= lost < DISTINCT // 2, (lost, info)
                assert info["slots"] == 8192 and info["indexed"] == DISTINCT
            unk = block[~found]
            assert av.push_mixed(ag, places, world.rs[unk], world.pks[unk], world.msgs[unk]) == BLOCK
            e = world.e(block)
            assert av.finish(e) == OK
            assert av.finish(scalar_bytes((int.from_bytes(e.tobytes(), "little") + 1) % Q)) == INVALID
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------- 6. the reason for the feature
def plus_one(e):
    return scalar_bytes((int.from_bytes(np.asarray(e, np.uint8).tobytes(), "little") + 1) % Q)


class Chain:
    """a producer pool that holds the BLOCK records and their keys; a validator pool that admitted a shuffled 90 % of
    them among other lanes, a third of which left again in between"""

    def __init__(self, world):
        eng, rng = world.engine, np.random.default_rng(366)
        self.world = world
        self.producer = world.new_pool("keyed", lanes=np.arange(BLOCK), index=False)
        self.order = rng.permutation(BLOCK)                                # the block: the producer's places, in its order
        self.agg, self.keys = self.producer.finish_select_bytes(self.order, keys=True)
        self.ids = self.producer.leaves_select(self.order)
        self.msgs = world.msgs[self.order]
        shuffled = rng.permutation(BLOCK)
        self.known_lanes = shuffled[:BLOCK * 9 // 10]
        others = np.arange(BLOCK, WORLD)
        self.cache = eng.keycache_create(512, wire=True)
        self.validator = eng.aggregator(CAPACITY, POOL_B, hold_admission=True, index=True)
        half = len(self.known_lanes) // 2
        for part in (others, self.known_lanes[:half]):
            status, kept, _ = self.validator.push_keyed(self.cache, world.keyed[part], world.msgs[part])
            assert kept == len(part)
        drop = np.zeros(OTHERS + half, np.uint8)
        drop[rng.permutation(OTHERS)[:OTHERS // 3]] = 1                    # a third of the other lanes leaves
        assert self.validator.remove(drop) == OTHERS + half - OTHERS // 3
        part = self.known_lanes[half:]
        status, kept, _ = self.validator.push_keyed(self.cache, world.keyed[part], world.msgs[part])
        assert kept == len(part)
        self.is_known = np.isin(self.order, self.known_lanes)

    def close(self):
        for h in (self.producer, self.validator, self.cache):
            h.close()

    def one_shot(self, agg, msgs):
        with self.world.engine.keycache_create(512, wire=True) as fresh:
            v, _ = self.world.engine.verify_aggregates_cached(fresh, [agg], self.keys, msgs)
        return int(v[0])


@pytest.fixture(scope="module")
def chain(world):
    c = Chain(world)
    yield c
    c.close()


def test_the_block_is_the_one_shot_block(world, chain):
    assert (chain.agg == world.ref(chain.order)).all()
    assert (chain.keys == world.wire[chain.order]).all() and (chain.ids == world.leaves[chain.order]).all()


@pytest.mark.parametrize("form", ["host", "device"])
def test_ids_to_a_verdict(engine, world, chain, form):
    """lookup -> push_mixed_wire(require = 2) -> finish == the one-shot cached call on the whole block: valid for the
    honest block, invalid for e_agg + 1 and for a changed message byte in a lane the validator lacks.  device: the
    places never leave the device; only u is read back"""
    import torch
    n = BLOCK
    rs, e_agg = chain.agg[:49 * n].reshape(n, 49), chain.agg[49 * n:]
    unk = ~chain.is_known
    changed = chain.msgs.copy()
    changed[int(np.flatnonzero(unk)[5]), 3] ^= 0x10
    cases = [(chain.msgs, e_agg, OK), (chain.msgs, plus_one(e_agg), INVALID), (changed, e_agg, INVALID)]
    with engine.aggregate_verifier(n, 64) as av:
        for msgs, scalar, verdict in cases:
            av.reset()
            if form == "host":
                places, u = chain.validator.lookup(chain.ids)
                wrong = np.flatnonzero((places == UNKNOWN) != unk)
                assert wrong.size == 0 and u == int(unk.sum()), (verdict, wrong[:8], places[wrong[:8]], u, int(unk.sum()))
                av.push_mixed_wire(chain.validator, places, rs[unk], chain.keys[unk], msgs[unk], cache=chain.cache, require=2)
            else:
                d_ids = dev(chain.ids)
                d_places = torch.full((n,), 0x6EEEEEEE, dtype=torch.int32, device="cuda:0")
                words = torch.full((2,), 0x6EEEEEEE, dtype=torch.int32, device="cuda:0")
                d_unknown = [dev(a[unk]) for a in (rs, chain.keys, msgs)]
                torch.cuda.synchronize()
                chain.validator.lookup_device(d_ids.reshape(-1), d_places, words[0:1])
                engine.sync()
                assert int(words.cpu()[0]) == int(unk.sum())               # u: the one word that is read back
                av.push_mixed_wire_device(chain.validator, d_places, words[1:2], *d_unknown, cache=chain.cache, require=2)
                engine.sync()
                assert int(words.cpu()[1]) == 0
            agg = np.concatenate([rs.reshape(-1), np.asarray(scalar, np.uint8)])
            assert av.finish(scalar) == verdict == chain.one_shot(agg, msgs), (form, verdict)


def test_a_block_the_pool_holds_entirely(engine, world, chain):
    import torch
    order = chain.order[chain.is_known][:1000]
    agg = chain.producer.finish_select_bytes(order)
    ids = chain.producer.leaves_select(order)
    d_places = torch.zeros(1000, dtype=torch.int32, device="cuda:0")
    words = torch.full((2,), 0x6EEEEEEE, dtype=torch.int32, device="cuda:0")
    d_ids = dev(ids)
    with engine.aggregate_verifier(1000, 64) as av:
        chain.validator.lookup_device(d_ids.reshape(-1), d_places, words[0:1])
        av.push_known_device(chain.validator, d_places, words[1:2])
        engine.sync()
        assert list(words.cpu().numpy()) == [0, 0]
        assert av.finish(agg[49000:]) == OK and av.finish(plus_one(agg[49000:])) == INVALID
    assert (agg == world.ref(order)).all()


# ---------------------------------------------------------------------------------------------- 7. launches
OLD_LAUNCHES = ("agx_k_append", "agx_k_check", "agx_k_move", "agx_k_first_changed", "av_k_keep", "agx_k_coeff_fold",
                "ag_k_fold_finish", "ag_k_tree", "ag_k_level", "ssa_k_hash", "agx_k_mark", "agx_k_bits_to_mask", "agx_k_select",
                "agx_k_select_verdict")
INDEX_LAUNCHES = ("agi_k_insert", "agi_k_lookup", "agx_k_leaves_select")


def test_the_index_is_lazy_by_name_and_count_of_every_launch(world):
    """push, finish, remove, drop_front and finish_select launch the same kernels, as often, on an object with and
    without the flag, and none of this section's; all index work is in index_sync and in front of a lookup"""
    import schnorr_sig_amd as ssa
    eng = ssa.Engine(0)
    names = OLD_LAUNCHES + INDEX_LAUNCHES
    try:
        counts, finals = {}, {}

        def drain():
            return {name: eng.read_timing(name)[1] for name in names}
        for flag in (False, True):
            eng.enable_timing(True)
            drain()
            with world.new_pool("plain", eng, index=flag) as ag:
                drop = (np.arange(HELD) % 3 == 0).astype(np.uint8)
                ag.remove(drop)
                ag.drop_front(POOL_B + 3)
                ag.remove_indices([5, 1, 77])
                world.fill(ag, "plain", np.arange(DISTINCT, DISTINCT + 30), eng)
                sel = ag.finish_select_bytes(np.arange(200)[::-1])
                finals[flag] = (ag.finish_bytes().copy(), sel)
                counts[flag] = drain()
                if flag:
                    ids = ag.leaves()
                    ag.index_sync()
                    got = drain()
                    assert got["agi_k_insert"] == 1 and sum(got.values()) == 1, got
                    ag.lookup(ids[:300])
                    got = drain()
                    assert got["agi_k_lookup"] == 1 and sum(got.values()) == 1, got       # a synced index: the query alone
                    ag.drop_front(3)
                    want = expected(dictionary(ag.leaves()), ids[:300])
                    drain()
                    places, unknown = ag.lookup(ids[:300])
                    got = drain()
                    assert (got["agi_k_insert"], got["agi_k_lookup"]) == (1, 1) and sum(got.values()) == 2, got
                    assert unknown == want[1] and (places == want[0]).all() and (places[3:] == np.arange(297)).all()
                    world.fill(ag, "plain", np.arange(DISTINCT + 30, DISTINCT + 40), eng)
                    drain()
                    ag.lookup(ids[:300])
                    got = drain()
                    assert (got["agi_k_insert"], got["agi_k_lookup"]) == (1, 1) and sum(got.values()) == 2, got   # incremental
                    assert ag.index_info()["rebuilds"] == 2
                    ag.leaves_select([1, 2, 3])
                    got = drain()
                    assert (got["agx_k_leaves_select"], got["agx_k_select_verdict"]) == (1, 1) and sum(got.values()) == 2, got
                else:
                    with pytest.raises(ValueError):
                        ag.lookup(np.zeros((1, 32), np.uint8))
                eng.enable_timing(False)
        assert counts[False] == counts[True], (counts[False], counts[True])
        assert all(counts[False][name] == 0 for name in INDEX_LAUNCHES) and counts[False]["agx_k_move"] >= 3
        assert counts[False]["agx_k_append"] >= 3 and counts[False]["agx_k_select"] == 1
        assert all((a == b).all() for a, b in zip(finals[False], finals[True]))
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------- 8. other cases
def test_nothing_the_index_needs_lives_in_a_workspace(engine, world):
    with world.new_pool("plain") as ag:
        ids = np.concatenate([world.leaves[:BLOCK], world.absent[:30]])
        engine.debug_poison_workspaces(0x5A)
        ag.index_sync()
        engine.debug_poison_workspaces(0xFF)
        want, unknown = check_lookup(ag, ids)
        engine.debug_poison_workspaces(0x01)
        got = ag.lookup(ids)
        assert (got[0] == want).all() and got[1] == unknown
        ag.drop_front(5)
        engine.debug_poison_workspaces(0xA5)
        got = lookup_device(ag, ids)
        engine.debug_poison_workspaces(0x01)
        want, unknown = check_lookup(ag, ids)
        assert (got[0] == want).all() and got[1] == unknown and ag.index_info()["overflowed"] == 0


def test_a_pool_of_another_context_or_without_the_flag_is_refused(engine, world, pools):
    import schnorr_sig_amd as ssa
    lib, ag = ssa._lib, pools["plain"]
    ids = np.ascontiguousarray(world.leaves[world.order[:4]])
    places = np.full(4, 0x77777777, np.uint32)
    count = C.c_uint64(9)
    words = np.full(8, 9, np.uint64)
    other = ssa.Engine(0)
    try:
        before = ag.index_info()
        with world.new_pool("plain", lanes=world.order[:40], capacity=64, index=False) as bare:
            cases = [(other._ctx, ag.handle), (engine._ctx, bare.handle)]
            for ctx, handle in cases:
                assert lib.ssa_aggregator_lookup(ctx, handle, ssa._ptr(ids), 4, ssa._ptr(places), C.byref(count)) == ssa.ERR_ARG
                assert lib.ssa_aggregator_index_sync(ctx, handle) == ssa.ERR_ARG
                assert lib.ssa_aggregator_index_info(ctx, handle, words.ctypes.data_as(C.POINTER(C.c_uint64))) == ssa.ERR_ARG
            # the leaf column needs no flag, but the object's own context
            assert (bare.leaves() == world.leaves[world.order[:40]]).all()
            assert (bare.leaves_select([39, 0]) == world.leaves[world.order[[39, 0]]]).all()
            out = np.full((4, 32), 0xEE, np.uint8)
            assert lib.ssa_aggregator_leaves(other._ctx, bare.handle, 4, ssa._ptr(out)) == ssa.ERR_ARG
            order = np.arange(4, dtype=np.uint32)
            assert lib.ssa_aggregator_leaves_select(other._ctx, bare.handle, ssa._ptr(order), 4, ssa._ptr(out)) == ssa.ERR_ARG
            assert (out == 0xEE).all() and bare.info()["held"] == 40
        assert (places == 0x77777777).all() and count.value == 9 and (words == 9).all()
        assert ag.index_info() == before
        assert (ag.lookup(ids)[0] == np.arange(4)).all()
    finally:
        other.close()
