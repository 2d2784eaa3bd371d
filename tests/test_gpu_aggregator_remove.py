"""Removing lanes from the streaming aggregator in place (ssa_aggregator_drop_front, ssa_aggregator_remove; DESIGN.md
section 30).  The contract is one equality: with K the ascending list of kept lanes, the object is afterwards what it
would be had it admitted those lanes alone -- finish(n_take) writes, byte for byte, what ssa_aggregate_many (flags 0)
returns for the first n_take kept lanes handed in alone.  Expected values always come from the one-shot call of the
session's engine (Engine.aggregate) on the kept signatures, never from an aggregator."""
import ctypes as C
import os

import numpy as np
import pytest

from test_gpu_aggregator import BAD, BAD_PUSHES, PUSHES, TOTAL, make_scalars, spoil

pytestmark = pytest.mark.gpu

OK = 0
EXTRA = 300                                          # one more push behind every removal
POOL = TOTAL + EXTRA
# 0, 1, 2, around every edge of a block of 512 (and of 64, and of 2), then all lanes: descending first, then ascending
PREFIXES = [0, 1, 2, 3, 63, 64, 65, 511, 512, 513, 1023, 1024, 1025]


class Pool:
    """POOL honest signatures over 80-byte messages, made once; ref(idx): the one-shot aggregate of the lanes idx (an
    ascending index array) handed in alone, computed once each and never changed"""

    def __init__(self, engine):
        rng = np.random.default_rng(0xD809)
        self.engine = engine
        self.msgs = rng.integers(0, 256, size=(POOL, 80), dtype=np.uint8)
        self.pks, self.sigs = engine.keygen_sign_many(make_scalars(rng, POOL), make_scalars(rng, POOL), self.msgs)
        self._refs = {}

    def lanes(self, lo, hi):
        return self.sigs[lo:hi], self.pks[lo:hi], self.msgs[lo:hi]

    def ref(self, idx):
        idx = np.asarray(idx, dtype=np.int64)
        key = idx.tobytes()
        if key not in self._refs:
            if idx.size == 0:
                agg = np.zeros(32, np.uint8)
            else:
                st, agg, _, nf = self.engine.aggregate(self.sigs[idx], self.pks[idx], self.msgs[idx])
                assert st == OK and nf == 0
            agg.setflags(write=False)
            self._refs[key] = agg
        return self._refs[key]


@pytest.fixture(scope="module")
def pool(engine):
    return Pool(engine)


def loaded(engine, pool, block_lanes=0, capacity=POOL):
    """an object holding lanes [0, TOTAL) of the pool, brought by PUSHES (no screen: the lanes are honest)"""
    ag, lo = engine.aggregator(capacity, block_lanes), 0
    for cnt in PUSHES:
        status, kept = ag.push(*pool.lanes(lo, lo + cnt), screen=False)
        assert kept == cnt and not status.any()
        lo += cnt
    assert lo == TOTAL
    return ag


def check(ag, pool, K, counters=None):
    """the object holds exactly the lanes K of the pool: info, every prefix finish (descending, then ascending), and
    one more push lands behind them"""
    K = np.asarray(K, dtype=np.int64)
    info = ag.info()
    assert info["held"] == K.size and info["blocks"] == K.size // info["block_lanes"]
    if counters is not None:
        assert {k: info[k] for k in ("pushes", "offered", "dropped")} == counters
    pre = [n for n in PREFIXES if n < K.size] + [K.size]
    for n in pre[::-1] + pre:
        got = ag.finish_bytes(n)
        assert got.size == 49 * n + 32 and (got == pool.ref(K[:n])).all(), n
    status, kept = ag.push(*pool.lanes(TOTAL, POOL), screen=False)
    assert kept == EXTRA and not status.any()
    assert ag.info()["held"] == K.size + EXTRA
    assert (ag.finish_bytes() == pool.ref(np.concatenate([K, np.arange(TOTAL, POOL)]))).all()


COUNTERS = dict(pushes=len(PUSHES), offered=TOTAL, dropped=0)


# ---------------------------------------------------------------------------------------------- 1. front drops
@pytest.mark.parametrize("n", [0, 1, 2, 3, 4, 511, 512, 513, 1024, 1287, 1288])
def test_drop_front(engine, pool, n):
    """0 .. 4: every shift of the R's mod 4; 512, 1024: tops moved; the rest: blocks reduced again"""
    with loaded(engine, pool) as ag:
        finishes = ag.info()["finishes"]
        ag.drop_front(n)
        assert ag.info()["finishes"] == finishes                          # a withdrawal is no finish
        check(ag, pool, np.arange(n, TOTAL), COUNTERS)


def test_drop_front_of_everything_by_default(engine, pool):
    with loaded(engine, pool) as ag:
        ag.drop_front()
        check(ag, pool, [], COUNTERS)


def test_two_drops_in_a_row(engine, pool):
    with loaded(engine, pool) as ag:
        ag.drop_front(512)
        ag.drop_front(1)
        check(ag, pool, np.arange(513, TOTAL), COUNTERS)


@pytest.mark.parametrize("B", [64, 2])
def test_drop_front_small_blocks(engine, pool, B):
    for n in (1, 64, 130, 512):
        with loaded(engine, pool, B) as ag:
            ag.drop_front(n)
            check(ag, pool, np.arange(n, TOTAL), COUNTERS)


# ---------------------------------------------------------------------------------------------- 2. masks
def masks():
    m = {name: np.zeros(TOTAL, np.uint8) for name in ("none", "lane 0", "last lane", "every second", "block 1", "quarter")}
    m["all"] = np.full(TOTAL, 3, np.uint8)
    m["lane 0"][0] = 1
    m["last lane"][TOTAL - 1] = 255
    for k in (510, 511, 512, 513):
        m["lane %d" % k] = np.zeros(TOTAL, np.uint8)
        m["lane %d" % k][k] = 2
    m["every second"][0::2] = 3                       # lane 0 goes: no front drop, although the first change is at 0
    m["block 1"][512:1024] = 1
    m["quarter"][np.random.default_rng(0x0DD).choice(TOTAL, TOTAL // 4, replace=False)] = 2
    return m


MASKS = masks()


@pytest.mark.parametrize("B", [0, 64, 2], ids=["B512", "B64", "B2"])
@pytest.mark.parametrize("name", sorted(MASKS))
def test_remove_by_mask(engine, pool, name, B):
    """B = 2: 550 tops at 1100 kept lanes and a two-pass root"""
    drop = MASKS[name]
    K = np.flatnonzero(drop == 0)
    with loaded(engine, pool, B) as ag:
        assert ag.remove(drop) == K.size
        check(ag, pool, K, COUNTERS)


def test_status_bytes_as_a_mask(engine, pool):
    """the status_out of a screened push with one bad lane of each class, handed to remove as it is on an object that
    admitted all of those lanes"""
    sigs, pks, msgs, inf = spoil(engine, *pool.lanes(0, TOTAL))
    only_screen = [k for k, v in BAD.items() if v[2]]                     # what the unscreened checks let in
    with engine.aggregator(TOTAL) as screened, engine.aggregator(TOTAL) as ag:
        lo, statuses = 0, []
        for cnt in BAD_PUSHES:
            sl = slice(lo, lo + cnt)
            statuses.append(screened.push(sigs[sl], pks[sl], msgs[sl], pk_inf=inf[sl])[0])
            lo += cnt
        status = np.concatenate(statuses)
        K = np.flatnonzero(status == 0)
        assert K.size == TOTAL - sum(1 for v in BAD.values() if not v[1])
        # the second object: every lane the unscreened checks admit (the malformed ones cannot be held at all)
        held = np.array([k for k in range(TOTAL) if k not in BAD or BAD[k][2]])
        st2, kept2 = ag.push(sigs, pks, msgs, pk_inf=inf, screen=False)
        assert kept2 == held.size and (np.flatnonzero(st2 == 0) == held).all() and set(only_screen) <= set(held)
        assert ag.remove(status[held]) == K.size
        want = engine.aggregate(sigs[K], pks[K], msgs[K], pk_inf=inf[K])
        assert want[0] == OK and (ag.finish_bytes() == want[1]).all()
        assert (ag.finish_bytes() == screened.finish_bytes()).all()
        info = ag.info()
        assert info["held"] == K.size and info["dropped"] == TOTAL - held.size       # refused admissions only


# ---------------------------------------------------------------------------------------------- 3. tops moved, not reduced
def launches(engine, *names):
    return tuple(engine.read_timing(k)[1] for k in names)


def test_aligned_front_drops_move_the_tops(engine, pool):
    keys = ("ag_k_tree", "ag_k_level", "agx_k_move")
    for B in (0, 64):
        tree = "ag_k_tree" if B == 0 else "ag_k_level"
        with loaded(engine, pool, B) as ag:
            engine.enable_timing(True)
            try:
                launches(engine, *keys)
                ag.drop_front(512)
                assert launches(engine, *keys) == (0, 0, 1)
                ag.drop_front(0)
                assert launches(engine, *keys) == (0, 0, 0)               # n == 0 launches nothing
            finally:
                engine.enable_timing(False)
            assert (ag.finish_bytes() == pool.ref(np.arange(512, TOTAL))).all()
        with loaded(engine, pool, B) as ag:
            engine.enable_timing(True)
            try:
                launches(engine, *keys)
                ag.drop_front(1024)
                assert launches(engine, *keys) == (0, 0, 1)
                ag.drop_front(1)
                got = dict(zip(keys, launches(engine, *keys)))
                assert got["agx_k_move"] == 1 and got[tree] == (1 if (TOTAL - 1025) // (B or 512) else 0)
            finally:
                engine.enable_timing(False)
            assert (ag.finish_bytes() == pool.ref(np.arange(1025, TOTAL))).all()
    with loaded(engine, pool) as ag:
        engine.enable_timing(True)
        try:
            launches(engine, *keys)
            ag.drop_front(1)
            assert launches(engine, *keys) == (1, 0, 1)                   # the re-reduction: one launch over two blocks
        finally:
            engine.enable_timing(False)


# ---------------------------------------------------------------------------------------------- 4. the hazard
@pytest.fixture(scope="module")
def tight():
    """a context whose MSM slice is 512 lanes: a removal on 1288 lanes walks three pieces"""
    import schnorr_sig_amd as ssa
    old = os.environ.get("SSA_MSM_SLICE")
    os.environ["SSA_MSM_SLICE"] = "512"
    try:
        eng = ssa.Engine(0)
    finally:
        if old is None:
            del os.environ["SSA_MSM_SLICE"]
        else:
            os.environ["SSA_MSM_SLICE"] = old
    assert eng.info()["msm_slice"] == 512
    yield eng
    eng.close()


def loaded_tight(tight, pool):
    ag, lo = tight.aggregator(POOL), 0
    for cnt in (512, 511, 265):
        status, kept = ag.push(*pool.lanes(lo, lo + cnt), screen=False)
        assert kept == cnt
        lo += cnt
    return ag


@pytest.mark.parametrize("case", ["drop_front 1", "drop_front 3", "drop_front 513", "every second", "quarter"])
def test_pieces_whose_sources_overlap_the_next_destinations(tight, pool, case):
    """every piece's sources lie in the next piece's places (drop_front(1): lane 512, the first source of piece 1, is
    the last place of piece 0 plus one); moved in one launch, or in pieces in the wrong order, the bytes differ"""
    with loaded_tight(tight, pool) as ag:
        tight.enable_timing(True)
        try:
            tight.read_timing("agx_k_move")
            if case.startswith("drop_front"):
                n = int(case.split()[1])
                ag.drop_front(n)
                K = np.arange(n, TOTAL)
            else:
                K = np.flatnonzero(MASKS[case] == 0)
                assert ag.remove(MASKS[case]) == K.size
            first = 0 if case != "quarter" else int(np.flatnonzero(MASKS[case])[0])
            assert tight.read_timing("agx_k_move")[1] == -(-(K.size - first) // 512)          # 3, 3, 2, 2, 2 pieces
        finally:
            tight.enable_timing(False)
        info = ag.info()
        assert info["held"] == K.size and info["blocks"] == K.size // 512
        pre = [n for n in PREFIXES if n < K.size] + [K.size]
        for n in pre[::-1] + pre:
            assert (ag.finish_bytes(n) == pool.ref(K[:n])).all(), n
        ag.push(pool.sigs[TOTAL:TOTAL + 100], pool.pks[TOTAL:TOTAL + 100], pool.msgs[TOTAL:TOTAL + 100], screen=False)
        assert (ag.finish_bytes() == pool.ref(np.concatenate([K, np.arange(TOTAL, TOTAL + 100)]))).all()


# ---------------------------------------------------------------------------------------------- 5. nothing in front is written
def test_nothing_in_front_of_the_first_removed_lane_changes(engine, pool):
    drop = np.zeros(TOTAL, np.uint8)
    drop[1000] = 1
    K = np.flatnonzero(drop == 0)
    with loaded(engine, pool) as ag, loaded(engine, pool, 8) as other:
        before = {n: ag.finish_bytes(n) for n in (1000, 999, 513, 512, 511, 1)}
        other_before = {n: other.finish_bytes(n) for n in (TOTAL, 1025, 8, 7)}
        engine.enable_timing(True)
        try:
            engine.read_timing("agx_k_move")
            engine.read_timing("ag_k_tree")
            assert ag.remove(drop) == TOTAL - 1
            assert engine.read_timing("agx_k_move")[1] == 1 and engine.read_timing("ag_k_tree")[1] == 1
        finally:
            engine.enable_timing(False)
        for n, want in before.items():
            assert (ag.finish_bytes(n) == want).all() and (want == pool.ref(np.arange(n))).all(), n
        for n in (1001, 1024, 1025, TOTAL - 1):
            assert (ag.finish_bytes(n) == pool.ref(K[:n])).all(), n
        for n, want in other_before.items():                              # a second object on the context: untouched
            assert (other.finish_bytes(n) == want).all() and (want == pool.ref(np.arange(n))).all(), n
        other.drop_front(9)
        assert (ag.finish_bytes() == pool.ref(K)).all()
        assert (other.finish_bytes() == pool.ref(np.arange(9, TOTAL))).all()


# ---------------------------------------------------------------------------------------------- 6. no state in workspaces
def test_poisoned_workspaces_and_unrelated_calls(engine, pool):
    other = pool.lanes(700, 1400)
    agg_other = pool.ref(np.arange(700, 1400))

    def disturb(step):
        engine.debug_poison_workspaces(0xA5)
        if step % 2 == 0:
            status, nf = engine.verify_many(*other)
            assert nf == 0 and not status.any()
        else:
            st, agg, _, nf = engine.aggregate(*other)
            assert st == OK and (agg == agg_other).all()
        engine.debug_poison_workspaces(0x5A)

    with loaded(engine, pool) as ag:
        disturb(0)
        ag.drop_front(3)
        disturb(1)
        assert (ag.finish_bytes() == pool.ref(np.arange(3, TOTAL))).all()
        drop = MASKS["quarter"][3:]
        K = 3 + np.flatnonzero(drop == 0)
        disturb(0)
        assert ag.remove(drop) == K.size
        disturb(1)
        assert (ag.finish_bytes(600) == pool.ref(K[:600])).all()
        disturb(0)
        ag.drop_front(512)
        disturb(1)
        check(ag, pool, K[512:], COUNTERS)


# ---------------------------------------------------------------------------------------------- 7. refusals
def test_refusals_change_nothing(engine, pool):
    import schnorr_sig_amd as ssa
    lib = ssa._lib
    with engine.aggregator(10, 4) as ag:
        ag.push(*pool.lanes(0, 6), screen=False)
        before, info = ag.finish_bytes(), ag.info()
        unchanged = lambda: ag.info() == dict(info, finishes=ag.info()["finishes"]) and (ag.finish_bytes() == before).all()
        nk, mask = C.c_uint64(77), np.ones(8, np.uint8)
        with pytest.raises(RuntimeError):
            ag.drop_front(7)                                              # more than are held
        for size in (5, 7, 0):                                            # a length other than the lanes held
            with pytest.raises(RuntimeError):
                ag.remove(mask[:size])
            assert lib.ssa_aggregator_remove_device(engine._ctx, ag.handle, None, size, C.byref(nk)) == ssa.ERR_ARG
        assert lib.ssa_aggregator_remove(engine._ctx, ag.handle, None, 6, C.byref(nk)) == ssa.ERR_ARG     # a NULL mask
        assert lib.ssa_aggregator_remove_device(engine._ctx, ag.handle, None, 6, C.byref(nk)) == ssa.ERR_ARG
        assert lib.ssa_aggregator_remove(engine._ctx, ag.handle, ssa._ptr(mask), 6, None) == ssa.ERR_ARG  # no count
        assert nk.value == 77 and unchanged()
        other = ssa.Engine(0)
        try:                                                              # a context other than the object's
            with pytest.raises(RuntimeError):
                ag.drop_front(1, engine=other)
            with pytest.raises(RuntimeError):
                ag.remove(mask[:6], engine=other)
            assert lib.ssa_aggregator_remove_device(other._ctx, ag.handle, None, 6, C.byref(nk)) == ssa.ERR_ARG
            orphan = other.aggregator(4, 2)
            orphan.push(*pool.lanes(0, 2), screen=False)
        finally:
            other.close()
        try:                                                              # an orphaned object: its context is gone
            assert lib.ssa_aggregator_drop_front(engine._ctx, orphan.handle, 1) == ssa.ERR_ARG
            assert lib.ssa_aggregator_remove(engine._ctx, orphan.handle, ssa._ptr(mask), 2, C.byref(nk)) == ssa.ERR_ARG
        finally:
            orphan.close()
        assert nk.value == 77 and unchanged()
        ag.drop_front(0)
        assert ag.remove(np.zeros(6, np.uint8)) == 6
        assert unchanged()
        assert ag.remove(np.array([0, 0, 9, 0, 0, 0], np.uint8)) == 5
        assert (ag.finish_bytes() == pool.ref([0, 1, 3, 4, 5])).all()
        ag.drop_front(5)
        assert ag.remove(np.zeros(0, np.uint8)) == 0 and ag.info()["held"] == 0        # an empty object, an empty mask
        assert not ag.finish_bytes().any()


# ---------------------------------------------------------------------------------------------- 8. mirrors, device forms, reset
def test_take_gives_the_block_and_keeps_the_rest(engine, pool):
    with loaded(engine, pool) as ag:
        block = ag.take(700)
        assert len(block) == 700 and block.to_bytes() == pool.ref(np.arange(700)).tobytes()
        assert ag.info()["held"] == TOTAL - 700
        block = ag.take(512)
        assert block.to_bytes() == pool.ref(np.arange(700, 1212)).tobytes()
        ag.push(*pool.lanes(TOTAL, POOL), screen=False)
        rest = np.concatenate([np.arange(1212, TOTAL), np.arange(TOTAL, POOL)])
        assert (ag.finish_bytes(77) == pool.ref(rest[:77])).all()
        assert ag.take().to_bytes() == pool.ref(rest).tobytes()
        info = ag.info()
        assert info["held"] == 0 and info["finishes"] == 4 and info["pushes"] == len(PUSHES) + 1


def test_remove_device_at_an_odd_offset(engine, pool):
    import torch
    drop = MASKS["quarter"]
    K = np.flatnonzero(drop == 0)
    big = torch.full((TOTAL + 64,), 1, dtype=torch.uint8, device="cuda:0")
    big[13:13 + TOTAL] = torch.from_numpy(drop).to("cuda:0")
    with loaded(engine, pool) as ag:
        assert ag.remove_device(big[13:13 + TOTAL]) == K.size
        assert (big.cpu().numpy()[13:13 + TOTAL] == drop).all()           # the mask is read, not written
        check(ag, pool, K, COUNTERS)
        with pytest.raises(RuntimeError):
            ag.remove_device(big[:TOTAL])                                 # not the lanes held now


def test_reset_after_a_removal_starts_over(engine, pool):
    with loaded(engine, pool) as ag:
        assert ag.remove(MASKS["every second"]) == TOTAL // 2
        ag.reset()
        assert ag.info() == dict(held=0, capacity=POOL, block_lanes=512, pushes=0, offered=0, dropped=0, blocks=0,
                                 finishes=0)
        assert not ag.finish_bytes().any()
        ag.push(*pool.lanes(100, 1200), screen=False)
        assert (ag.finish_bytes() == pool.ref(np.arange(100, 1200))).all()
