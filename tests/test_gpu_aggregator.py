"""The streaming aggregator (ssa_aggregator_*).  The contract is one equality: finish(n_take) writes,
byte for byte, what ssa_aggregate_many (flags 0) returns for the first n_take admitted lanes handed in alone, whatever the
pushes were that brought them.  Expected values always come from the one-shot calls of the session's engine
(Engine.aggregate, Engine.aggregate_valid, Engine.verify_batch_screened -- the call whose statuses a push promises), never
from the aggregator; for totals of at most three lanes also from the model of tests/aggregate_model.py over the C oracle."""
import ctypes as C
import os

import numpy as np
import pytest

import aggregate_model as am

pytestmark = pytest.mark.gpu

OK, INVALID, MALFORMED = 0, 2, 3
POOL = 4600
PUSHES = [1, 510, 1, 1, 0, 513, 3, 255, 4]          # ends on 511, 512, 513, two blocks crossed in one push, an empty push
TOTAL = sum(PUSHES)                                  # 1288
PREFIXES = [0, 1, 2, 511, 512, 513, 1023, 1024, 1025, 1288]


def make_scalars(rng, n):
    s = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    s[:, 31] &= 0x3F
    s[:, 0] |= 1
    return s


class Pool:
    """POOL honest signatures over 80-byte messages, made once; ref(lo, hi): the one-shot aggregate of lanes [lo, hi),
    computed once each and never changed"""

    def __init__(self, engine):
        rng = np.random.default_rng(0xA66E)
        self.engine = engine
        self.msgs = rng.integers(0, 256, size=(POOL, 80), dtype=np.uint8)
        self.pks, self.sigs = engine.keygen_sign_many(make_scalars(rng, POOL), make_scalars(rng, POOL), self.msgs)
        self.inf = np.zeros(POOL, np.uint8)
        self._refs = {}

    def lanes(self, lo, hi):
        return self.sigs[lo:hi], self.pks[lo:hi], self.msgs[lo:hi]

    def ref(self, lo, hi):
        if (lo, hi) not in self._refs:
            st, agg, _, nf = self.engine.aggregate(*self.lanes(lo, hi))
            assert st == OK and nf == 0
            agg.setflags(write=False)
            self._refs[(lo, hi)] = agg
        return self._refs[(lo, hi)]


@pytest.fixture(scope="module")
def pool(engine):
    return Pool(engine)


def one_shot(engine, sigs, pks, msgs, inf=None):
    """Engine.aggregate of these lanes alone"""
    st, agg, _, nf = engine.aggregate(sigs, pks, msgs, pk_inf=inf)
    assert st == OK and nf == 0
    return agg


def push_range(ag, pool, lo, cnt, screen=True):
    status, kept = ag.push(*pool.lanes(lo, lo + cnt), screen=screen)
    assert kept == cnt and status.size == cnt and not status.any()
    return lo + cnt


def loaded(engine, pool, screen=True, block_lanes=0, capacity=TOTAL):
    ag, lo = engine.aggregator(capacity, block_lanes), 0
    for cnt in PUSHES:
        lo = push_range(ag, pool, lo, cnt, screen)
    return ag


# ---------------------------------------------------------------------------------------------- 1. honest pushes
@pytest.mark.parametrize("screen", [True, False], ids=["screened", "no screen"])
def test_honest_pushes_finish_after_every_push(engine, oracle, pool, screen):
    with engine.aggregator(TOTAL) as ag:
        assert (ag.finish_bytes() == np.zeros(32, np.uint8)).all()
        lo = 0
        for j, cnt in enumerate(PUSHES):
            lo = push_range(ag, pool, lo, cnt, screen)
            got = ag.finish_bytes()
            assert got.size == 49 * lo + 32 and (got == pool.ref(0, lo)).all(), (j, lo)
            if lo <= 3:
                model = am.aggregate(am.oracle_backend(oracle), *pool.lanes(0, lo))
                assert got.tobytes() == model
        info = ag.info()
        assert info["held"] == TOTAL and info["pushes"] == len(PUSHES) and info["blocks"] == TOTAL // 512
        assert info["offered"] == TOTAL and info["dropped"] == 0 and info["finishes"] == len(PUSHES) + 1
        whole = ag.finish()
        assert len(whole) == TOTAL and whole.to_bytes() == pool.ref(0, TOTAL).tobytes()


def test_two_and_three_lanes_against_the_model(engine, oracle, pool):
    """totals of at most three lanes, every split into pushes of one and two lanes"""
    be = am.oracle_backend(oracle)
    for cut in ([1, 1], [2], [1, 1, 1], [1, 2], [2, 1], [3]):
        with engine.aggregator(3, 2) as ag:
            lo = 0
            for cnt in cut:
                lo = push_range(ag, pool, lo, cnt)
            for n in range(lo, -1, -1):
                assert ag.finish_bytes(n).tobytes() == am.aggregate(be, *pool.lanes(0, n)), (cut, n)


# ---------------------------------------------------------------------------------------------- 2. prefix finishes
def test_prefix_finishes_leave_the_object_alone(engine, pool):
    """descending first: finish(n_take) below the lanes held reduces a ragged block where the object holds a complete
    block's top -- written there, it would spoil every later finish above it"""
    with loaded(engine, pool) as ag:
        for n in PREFIXES[::-1] + PREFIXES:
            got = ag.finish_bytes(n)
            assert got.size == 49 * n + 32 and (got == pool.ref(0, n)).all(), n
        assert (ag.finish_bytes() == pool.ref(0, TOTAL)).all()
        assert ag.info()["held"] == TOTAL


# ---------------------------------------------------------------------------------------------- 3. small blocks
def test_small_blocks_two_pass_root(engine, pool):
    """block_lanes = 2: 550 tops at 1100 lanes, more than one workgroup of the root's first pass"""
    with engine.aggregator(1100, 2) as ag:
        lo = 0
        for cnt in [3, 1, 600, 496]:
            lo = push_range(ag, pool, lo, cnt)
            assert (ag.finish_bytes() == pool.ref(0, lo)).all(), lo
        assert ag.info()["blocks"] == 550
        for n in (1099, 1025, 1024, 1023, 513, 3, 2, 1):
            assert (ag.finish_bytes(n) == pool.ref(0, n)).all(), n


def test_blocks_of_64(engine, pool):
    with engine.aggregator(130, 64) as ag:
        lo = 0
        for cnt in [63, 1, 1, 65]:
            lo = push_range(ag, pool, lo, cnt)
            assert (ag.finish_bytes() == pool.ref(0, lo)).all(), lo
        assert ag.info()["blocks"] == 2
        for n in (129, 128, 127, 65, 64, 63):
            assert (ag.finish_bytes(n) == pool.ref(0, n)).all(), n


# ---------------------------------------------------------------------------------------------- 4. bad lanes
BAD_PUSHES = [512, 513, 263]                         # the lanes of TOTAL again, cut at block edges
#   lane of the concatenation -> what is wrong with it; (kept under the screen, kept without it)
BAD = {
    0: ("bit of e", False, True),
    511: ("message bit", False, True),               # the last lane of push 0 and of block 0
    512: ("R does not decode", False, False),        # the first lane of push 1
    513: ("e >= q", False, False),
    1023: ("key off the curve", False, False),       # the last lane of block 1
    1024: ("identity key, pk_inf set", True, True),  # the last lane of push 1: R = [e]G verifies under the identity
    1025: ("identity key, no pk_inf", False, False), # the first lane of push 2: (0, 0) is not on the curve
    1287: ("flag byte of R", False, True),           # the sort bit: another point, which the equation rejects
}


def spoil(engine, honest_sigs, honest_pks, honest_msgs):
    """copies of TOTAL honest lanes with the lanes of BAD made what BAD says, and the pk_inf bytes"""
    import pymodel as pm
    sigs, pks, msgs = honest_sigs.copy(), honest_pks.copy(), honest_msgs.copy()
    inf = np.zeros(TOTAL, np.uint8)
    e = make_scalars(np.random.default_rng(0x1D), 2)
    comp, st = engine.compress_many(engine.pubkey_many(e))
    assert (st == 0).all()
    for k, (what, _, _) in BAD.items():
        if what == "bit of e":
            sigs[k, 49] ^= 0x01
        elif what == "message bit":
            msgs[k, 17] ^= 0x04
        elif what == "R does not decode":
            for t in range(1, 64):
                x = honest_sigs[k, :49].copy()
                x[8] ^= t
                if pm.pt_decompress(x.tobytes())[0] == "invalid":
                    break
            sigs[k, :49] = x
        elif what == "e >= q":
            sigs[k, 49:81] = 0xFF
        elif what == "key off the curve":
            pks[k, 48] ^= 0x01
        elif what == "identity key, pk_inf set":
            sigs[k], pks[k], inf[k] = np.concatenate([comp[0], e[0]]), 0, 1
        elif what == "identity key, no pk_inf":
            sigs[k], pks[k] = np.concatenate([comp[1], e[1]]), 0
        else:
            sigs[k, 48] ^= 0x40
    return sigs, pks, msgs, inf


@pytest.fixture(scope="module")
def spoiled(engine, pool):
    return spoil(engine, *pool.lanes(0, TOTAL))


@pytest.mark.parametrize("screen", [True, False], ids=["screened", "no screen"])
def test_bad_lanes_are_dropped_push_by_push(engine, pool, spoiled, screen):
    sigs, pks, msgs, inf = spoiled
    want_kept = np.array([k for k in range(TOTAL) if k not in BAD or BAD[k][1 if screen else 2]])
    with engine.aggregator(TOTAL) as ag:
        lo, statuses = 0, []
        for cnt in BAD_PUSHES:
            sl = slice(lo, lo + cnt)
            status, kept = ag.push(sigs[sl], pks[sl], msgs[sl], pk_inf=inf[sl], screen=screen)
            if screen:
                want = engine.verify_batch_screened(sigs[sl], pks[sl], msgs[sl], pk_inf=inf[sl])[0]
            else:
                want = engine.aggregate(sigs[sl], pks[sl], msgs[sl], pk_inf=inf[sl], check=False)[2]
                assert set(np.unique(status)) <= {OK, MALFORMED}
            assert (status == want).all(), (lo, np.flatnonzero(status != want)[:8])
            assert kept == int((status == 0).sum())
            statuses.append(status)
            lo += cnt
        K = np.flatnonzero(np.concatenate(statuses) == 0)
        assert (K == want_kept).all()
        got = ag.finish_bytes()
        assert got.size == 49 * K.size + 32
        if screen:
            agg, kept_lanes, _ = engine.aggregate_valid(sigs, pks, msgs, pk_inf=inf)
            assert (kept_lanes == K).all() and (got == agg).all()
            assert engine.verify_aggregate(got, pks[K], msgs[K], pk_inf=inf[K]) == OK
        else:
            assert (got == one_shot(engine, sigs[K], pks[K], msgs[K], inf[K])).all()
        info = ag.info()
        assert info["held"] == K.size and info["offered"] == TOTAL and info["dropped"] == TOTAL - K.size
        assert info["pushes"] == len(BAD_PUSHES) and info["blocks"] == K.size // 512 and info["finishes"] == 1


# ---------------------------------------------------------------------------------------------- 5. the screened path
def test_one_push_through_the_msm_screen(engine, pool):
    """3500 lanes, above SSA_MSM_SMALL_MAX: the MSM screen runs on the scalars of the push's one hash launch"""
    n, bad = 3500, [0, 63, 1777, 3071, 3499]
    sigs, pks, msgs = (a.copy() for a in pool.lanes(POOL - n, POOL))
    sigs[bad[0], 49] ^= 0x01
    msgs[bad[1], 3] ^= 0x10
    sigs[bad[2], 49:81] = 0xFF
    pks[bad[3], 48] ^= 0x01
    sigs[bad[4], 48] ^= 0x40
    K = np.setdiff1d(np.arange(n), bad)
    with engine.aggregator(n) as ag:
        status, kept = ag.push(sigs, pks, msgs)
        assert (status == engine.verify_batch_screened(sigs, pks, msgs)[0]).all()
        assert kept == K.size and (np.flatnonzero(status == 0) == K).all()
        got = ag.finish_bytes()
        agg, kept_lanes, _ = engine.aggregate_valid(sigs, pks, msgs)
        assert (kept_lanes == K).all() and (got == agg).all()
        assert engine.verify_aggregate(got, pks[K], msgs[K]) == OK
        assert (ag.finish_bytes(3000) == one_shot(engine, sigs[K[:3000]], pks[K[:3000]], msgs[K[:3000]])).all()


# ---------------------------------------------------------------------------------------------- 6. refusals
def raw_push(engine, ag, sigs, pks, msgs, flags):
    import schnorr_sig_amd as ssa
    n, batch, keep = engine._agg_batch(sigs, 81, pks, msgs, None, None)
    nk = C.c_uint64(1 << 40)
    return ssa._lib.ssa_aggregator_push(engine._ctx, ag.handle, *batch, flags, None, C.byref(nk)), int(nk.value)


def test_refusals_change_nothing(engine, pool):
    import schnorr_sig_amd as ssa
    for capacity, block in ((0, 0), (8, 3), (8, 1024), (8, 1), ((1 << 30) + 1, 0)):
        with pytest.raises(RuntimeError):
            engine.aggregator(capacity, block)
    with engine.aggregator(10, 4) as ag:
        push_range(ag, pool, 0, 6)
        before, info = ag.finish_bytes(), ag.info()
        unchanged = lambda: ag.info() == dict(info, finishes=ag.info()["finishes"]) and (ag.finish_bytes() == before).all()
        with pytest.raises(RuntimeError):
            ag.push(*pool.lanes(6, 11))                                   # 5 lanes, room for 4: refused by n
        assert unchanged()
        with pytest.raises(RuntimeError):
            ag.finish_bytes(7)                                            # n_take above the lanes held
        assert raw_push(engine, ag, *pool.lanes(6, 8), 2)[0] == ssa.ERR_ARG       # an unknown flag
        assert raw_push(engine, ag, *pool.lanes(6, 8), 3)[0] == ssa.ERR_ARG
        assert unchanged()
        other = ssa.Engine(0)
        try:
            with pytest.raises(RuntimeError):
                ag.push(*pool.lanes(6, 8), engine=other)                  # a context other than the object's
            out = np.zeros(49 * 6 + 32, np.uint8)
            assert ssa._lib.ssa_aggregator_finish(other._ctx, ag.handle, 6, ssa._ptr(out)) == ssa.ERR_ARG
        finally:
            other.close()
        assert unchanged()
        push_range(ag, pool, 6, 4)                                        # exactly fills the capacity
        assert ag.info()["held"] == 10 and (ag.finish_bytes() == pool.ref(0, 10)).all()
        with pytest.raises(RuntimeError):
            ag.push(*pool.lanes(10, 11))
        assert ag.push(*pool.lanes(10, 10))[1] == 0                       # an empty push still fits


# ---------------------------------------------------------------------------------------------- 7. no state in workspaces
def test_state_does_not_live_in_workspaces(engine, pool):
    """two aggregators on one context, pushes interleaved, the context's workspaces poisoned and used by unrelated calls
    in between: each object's bytes are those of its own lanes"""
    lo_b = 2000
    other = pool.lanes(3000, 3700)
    agg_other = pool.ref(3000, 3700)

    def disturb(step):
        engine.debug_poison_workspaces(0xA5)
        if step % 3 == 0:
            status, nf = engine.verify_many(*other)
            assert nf == 0 and not status.any()
        elif step % 3 == 1:
            assert (one_shot(engine, *other) == agg_other).all()
        else:
            assert (engine.verify_aggregates([agg_other, pool.ref(0, 512)],
                                             np.concatenate([other[1], pool.pks[:512]]),
                                             np.concatenate([other[2], pool.msgs[:512]])) == OK).all()
        engine.debug_poison_workspaces(0x5A)

    with engine.aggregator(TOTAL) as a, engine.aggregator(TOTAL, 8) as b:
        la, lb = 0, lo_b
        for j, cnt in enumerate(PUSHES):
            la = push_range(a, pool, la, cnt)
            disturb(j)
            lb = push_range(b, pool, lb, PUSHES[-1 - j])
            disturb(j + 1)
            assert (a.finish_bytes() == pool.ref(0, la)).all(), j
        disturb(0)
        assert (b.finish_bytes() == pool.ref(lo_b, lo_b + TOTAL)).all()
        disturb(1)
        assert (a.finish_bytes(513) == pool.ref(0, 513)).all()
        assert (a.finish_bytes() == pool.ref(0, TOTAL)).all()


# ---------------------------------------------------------------------------------------------- 8. reset
def test_reset_starts_over(engine, pool):
    with engine.aggregator(TOTAL) as ag:
        push_range(ag, pool, 700, 700)                                    # other lanes first: a block and a ragged tail
        assert (ag.finish_bytes() == pool.ref(700, 1400)).all()
        ag.reset()
        assert ag.info() == dict(held=0, capacity=TOTAL, block_lanes=512, pushes=0, offered=0, dropped=0, blocks=0,
                                 finishes=0)
        assert not ag.finish_bytes().any()
        lo = 0
        for cnt in PUSHES:
            lo = push_range(ag, pool, lo, cnt)
        assert (ag.finish_bytes() == pool.ref(0, TOTAL)).all()
        assert ag.info() == dict(held=TOTAL, capacity=TOTAL, block_lanes=512, pushes=len(PUSHES), offered=TOTAL,
                                 dropped=0, blocks=2, finishes=2)


# ---------------------------------------------------------------------------------------------- 9. device forms
def test_device_forms_unaligned_output(engine, pool):
    import torch
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    d_sigs, d_pks, d_msgs = (dev(a) for a in pool.lanes(0, TOTAL))
    with engine.aggregator(TOTAL) as ag:
        lo = 0
        for j, cnt in enumerate(PUSHES):
            d_status = torch.full((max(cnt, 1),), 0xEE, dtype=torch.uint8, device="cuda:0")[:cnt]
            kept = ag.push_device(d_sigs[lo:lo + cnt], d_pks[lo:lo + cnt], d_msgs[lo:lo + cnt], d_status=d_status,
                                  screen=bool(j & 1))
            assert kept == cnt and not d_status.cpu().numpy().any()
            lo += cnt
        for n, shift in ((TOTAL, 13), (1025, 1), (512, 2), (1, 3), (0, 7)):
            size = 49 * n + 32
            big = torch.full((size + 64,), 0xEE, dtype=torch.uint8, device="cuda:0")
            assert ag.finish_device(big[shift:shift + size], n) == n
            torch.cuda.synchronize()
            got = big.cpu().numpy()
            assert (got[shift:shift + size] == pool.ref(0, n)).all(), (n, shift)
            assert (got[:shift] == 0xEE).all() and (got[shift + size:] == 0xEE).all(), (n, shift)
            assert (ag.finish_bytes(n) == got[shift:shift + size]).all()
        with pytest.raises(RuntimeError):
            ag.finish_device(torch.zeros(49 * (TOTAL + 1) + 32, dtype=torch.uint8, device="cuda:0"), TOTAL + 1)


# ---------------------------------------------------------------------------------------------- 10. above one MSM slice
def test_more_lanes_than_one_msm_slice(pool):
    """a context whose MSM slice is 512 lanes: a push above it is refused, and finish walks the 1288 held lanes in three
    pieces -- the same bytes"""
    import schnorr_sig_amd as ssa
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
        with tight.aggregator(TOTAL) as ag:
            with pytest.raises(RuntimeError):
                ag.push(*pool.lanes(0, 513))
            lo = 0
            for cnt in (512, 511, 265):
                lo = push_range(ag, pool, lo, cnt)
            for n in (TOTAL, 1025, 1024, 513, 512):
                assert (ag.finish_bytes(n) == pool.ref(0, n)).all(), n
    finally:
        tight.close()
