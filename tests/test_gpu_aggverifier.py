"""The streaming aggregate verifier (ssa_aggverifier_*).  The contract is one equality: finish(e_agg,
n_take) returns what ssa_verify_aggregate returns for the first n_take pushed lanes handed in at once with that scalar,
whatever the pushes were that brought them.  Expected values always come from the one-shot calls of the session's engine --
Engine.aggregate for e_agg, Engine.verify_aggregate for verdicts, Engine.verify_aggregate_shard_device over the root of
Engine.aggregate_root_device for exact records -- never from the verifier."""
import os

import numpy as np
import pytest

from aggregate_model import Q

pytestmark = pytest.mark.gpu

OK, INVALID, MALFORMED = 0, 2, 3
POOL = 4100
PUSHES = [1, 510, 1, 1, 0, 513, 3, 255, 4]          # ends on 511, 512, 513, two blocks crossed in one push, an empty push
TOTAL = sum(PUSHES)                                  # 1288
PREFIXES = [0, 1, 2, 511, 512, 513, 1023, 1024, 1025, 1288]


def make_scalars(rng, n):
    s = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    s[:, 31] &= 0x3F
    s[:, 0] |= 1
    return s


def scalar_bytes(v):
    return np.frombuffer(int(v).to_bytes(32, "little"), np.uint8)


class Pool:
    """POOL honest signatures over 80-byte messages, made once; ref(lo, hi): the one-shot aggregate of lanes [lo, hi),
    computed once each and never changed"""

    def __init__(self, engine):
        rng = np.random.default_rng(0xA66F)
        self.engine = engine
        self.msgs = rng.integers(0, 256, size=(POOL, 80), dtype=np.uint8)
        self.pks, self.sigs = engine.keygen_sign_many(make_scalars(rng, POOL), make_scalars(rng, POOL), self.msgs)
        self.rs = np.ascontiguousarray(self.sigs[:, :49])
        self._refs = {}

    def body(self, lo, hi):
        """what a validator receives of lanes [lo, hi)"""
        return self.rs[lo:hi], self.pks[lo:hi], self.msgs[lo:hi]

    def ref(self, lo, hi):
        if (lo, hi) not in self._refs:
            st, agg, _, nf = self.engine.aggregate(self.sigs[lo:hi], self.pks[lo:hi], self.msgs[lo:hi])
            assert st == OK and nf == 0
            agg.setflags(write=False)
            self._refs[(lo, hi)] = agg
        return self._refs[(lo, hi)]

    def e(self, lo, hi):
        return self.ref(lo, hi)[49 * (hi - lo):]


@pytest.fixture(scope="module")
def pool(engine):
    return Pool(engine)


def with_e(agg, e):
    out = np.array(agg, dtype=np.uint8)
    out[-32:] = e
    return out


def loaded(engine, pool, block_lanes=0, capacity=TOTAL, pushes=PUSHES):
    av, lo = engine.aggregate_verifier(capacity, block_lanes), 0
    for cnt in pushes:
        assert av.push(*pool.body(lo, lo + cnt)) == cnt
        lo += cnt
    return av


def expected_record(engine, rs, pks, msgs):
    """the record of the one-shot primitives over these lanes: tops and challenge scalars, the root, the shard's record"""
    import torch
    n = rs.shape[0]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    d_rs, d_pks, d_msgs = dev(rs), dev(pks), dev(msgs)
    tops = torch.zeros(32 * -(-n // 512), dtype=torch.uint8, device="cuda:0")
    root = torch.zeros(32, dtype=torch.uint8, device="cuda:0")
    h = torch.zeros(32 * n, dtype=torch.uint8, device="cuda:0")
    rec = torch.zeros(24, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    engine.aggregate_shard_tops_device(d_rs.data_ptr(), 49, d_pks.data_ptr(), d_msgs.data_ptr(), n, msgs.shape[1], 512,
                                       tops.data_ptr(), d_h=h.data_ptr())
    engine.aggregate_root_device(tops.data_ptr(), tops.numel() // 32, n, root.data_ptr(), block_lanes=512)
    engine.verify_aggregate_shard_device(d_rs.data_ptr(), d_pks.data_ptr(), d_msgs.data_ptr(), n, msgs.shape[1],
                                         h.data_ptr(), 0, root.data_ptr(), rec.data_ptr())
    engine.sync()
    return rec.cpu().numpy().view(np.uint64)


# ---------------------------------------------------------------------------------------------- 1. honest pushes
def test_pushes_with_a_finish_after_every_push(engine, pool):
    """the one-shot takes msm_k_small at these sizes: this also pins bucket-path verdicts = small-path verdicts"""
    msgs_bad = pool.msgs[:TOTAL].copy()
    msgs_bad[0, 17] ^= 0x04                                               # lane 0: in every prefix
    with engine.aggregate_verifier(TOTAL) as av, engine.aggregate_verifier(TOTAL) as av_m:
        assert av.finish(np.zeros(32, np.uint8)) == OK                    # the empty aggregate
        assert av.finish(scalar_bytes(1)) == INVALID and av.finish(scalar_bytes(Q)) == MALFORMED
        lo = 0
        for j, cnt in enumerate(PUSHES):
            av.push(*pool.body(lo, lo + cnt))
            av_m.push(pool.rs[lo:lo + cnt], pool.pks[lo:lo + cnt], msgs_bad[lo:lo + cnt])
            lo += cnt
            agg, pks, msgs = pool.ref(0, lo), pool.pks[:lo], pool.msgs[:lo]
            e = int.from_bytes(agg[49 * lo:].tobytes(), "little")
            assert e + 1 < Q
            for scalar, want in ((e, OK), (e + 1, INVALID), ((Q - e) % Q, INVALID)):
                got = av.finish(scalar_bytes(scalar))
                one_shot = engine.verify_aggregate(with_e(agg, scalar_bytes(scalar)), pks, msgs)
                print("push %d, %d lanes, scalar %s: finish %d, one-shot %d" % (j, lo, hex(scalar)[:10], got, one_shot))
                assert got == want and got == one_shot, (j, lo)
            got = av_m.finish(scalar_bytes(e))
            assert got == INVALID and got == engine.verify_aggregate(agg, pks, msgs_bad[:lo]), (j, lo)
        info = av.info()
        assert info["held"] == TOTAL and info["pushes"] == len(PUSHES) and info["blocks"] == TOTAL // 512
        assert info["pushed"] == TOTAL and info["finishes"] == 3 + 3 * len(PUSHES)


# ---------------------------------------------------------------------------------------------- 2. exact records
def test_exact_records(engine, pool):
    """the record is a canonical affine point, the scalar zero (e = 0 on every lane), the flag and the magic: word for
    word the one-shot record of the same lanes, which msm_k_small makes at these sizes"""
    with loaded(engine, pool) as av:
        for n in (1288, 513, 512, 511, 3, 2, 1):
            got, want = av.record(n), expected_record(engine, *pool.body(0, n))
            assert want[22] == 0 and not want[18:22].any()
            assert (got == want).all(), (n, np.flatnonzero(got != want))
        assert (av.record() == av.record(TOTAL)).all()


# ---------------------------------------------------------------------------------------------- 3. prefix finishes
def test_prefix_finishes_leave_the_object_alone(engine, pool):
    """descending first: finish(n_take) below the lanes held reduces a ragged block where the object holds a complete
    block's top -- written there, it would spoil every later finish above it"""
    with loaded(engine, pool) as av:
        before = av.record()
        for n in PREFIXES[::-1] + PREFIXES:
            assert av.finish(pool.e(0, n), n) == OK, n
            if n:
                assert av.finish(pool.e(0, n - 1), n) == INVALID, n
        assert av.finish(pool.e(0, TOTAL)) == OK
        assert av.info()["held"] == TOTAL and (av.record() == before).all()


# ---------------------------------------------------------------------------------------------- 4. small blocks
def test_small_blocks_two_pass_root(engine, pool):
    """block_lanes = 2: 550 tops at 1100 lanes, more than one workgroup of the root's first pass"""
    with engine.aggregate_verifier(1100, 2) as av:
        lo = 0
        for cnt in [3, 1, 600, 496]:
            av.push(*pool.body(lo, lo + cnt))
            lo += cnt
            assert av.finish(pool.e(0, lo)) == OK, lo
        assert av.info()["blocks"] == 550
        for n in (1099, 1025, 1024, 1023, 513, 3, 2, 1):
            assert av.finish(pool.e(0, n), n) == OK, n
            assert av.finish(pool.e(0, n + 1), n) == INVALID, n


def test_blocks_of_64(engine, pool):
    with engine.aggregate_verifier(130, 64) as av:
        lo = 0
        for cnt in [63, 1, 1, 65]:
            av.push(*pool.body(lo, lo + cnt))
            lo += cnt
            assert av.finish(pool.e(0, lo)) == OK, lo
        assert av.info()["blocks"] == 2
        for n in (129, 128, 127, 65, 64, 63):
            assert av.finish(pool.e(0, n), n) == OK, n
            assert av.finish(pool.e(0, n + 1), n) == INVALID, n


# ---------------------------------------------------------------------------------------------- 5. one lane of every class
BAD_PUSHES = [512, 513, 263]                         # the lanes of TOTAL again, cut at block edges
#   class -> (lane of the concatenation, the verdict it must give)
BAD = {
    "non-canonical limb in R.x": (511, MALFORMED),   # the last lane of push 0 and of block 0
    "non-canonical limb in the key": (512, MALFORMED),   # the first lane of push 1
    "key off the curve": (1023, MALFORMED),          # the last lane of block 1
    "R does not decode": (1024, MALFORMED),          # the last lane of push 1
    "identity key, pk_inf set": (1025, OK),          # the first lane of push 2; signed so: R = [e]G
    "flag byte of R": (1287, INVALID),               # the sort bit: another point, which the equation rejects
    "two lanes swapped": (510, INVALID),             # with lane 513: across a push and a block edge
}


def spoil(engine, pool, what):
    """-> (R's, keys, messages, pk_inf, e_agg) of TOTAL lanes with the lane of BAD[what] made what it says.  e_agg is the
    honest producer's: of the lanes as they are for the identity key, of the lanes before the change otherwise."""
    import pymodel as pm
    k = BAD[what][0]
    sigs, pks, msgs = pool.sigs[:TOTAL].copy(), pool.pks[:TOTAL].copy(), pool.msgs[:TOTAL].copy()
    inf = np.zeros(TOTAL, np.uint8)
    e_agg = pool.e(0, TOTAL)
    if what == "non-canonical limb in R.x":
        sigs[k, 8:16] = 0xFF
    elif what == "non-canonical limb in the key":
        pks[k, 56:64] = 0xFF
    elif what == "key off the curve":
        pks[k, 48] ^= 0x01
    elif what == "R does not decode":
        for t in range(1, 64):
            x = pool.sigs[k, :49].copy()
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
        e_agg = agg[49 * TOTAL:]
    elif what == "flag byte of R":
        sigs[k, 48] ^= 0x40
    else:
        for a in (sigs, pks, msgs):
            a[[k, 513]] = a[[513, k]]
    return np.ascontiguousarray(sigs[:, :49]), pks, msgs, inf, e_agg


@pytest.mark.parametrize("what", list(BAD))
def test_one_lane_of_every_class(engine, pool, what):
    rs, pks, msgs, inf, e_agg = spoil(engine, pool, what)
    k, want = BAD[what]
    with engine.aggregate_verifier(TOTAL) as av:
        lo = 0
        for cnt in BAD_PUSHES:
            sl = slice(lo, lo + cnt)
            av.push(rs[sl], pks[sl], msgs[sl], pk_inf=inf[sl])
            lo += cnt
        got = av.finish(e_agg)
        one_shot = engine.verify_aggregate(np.concatenate([rs.reshape(-1), e_agg]), pks, msgs, pk_inf=inf)
        assert got == want and got == one_shot, what
        # the lanes in front of it are untouched by it: the honest prefix verifies
        assert av.finish(pool.e(0, k), k) == OK
        if want == MALFORMED:
            assert av.finish(pool.e(0, k + 1), k + 1) == MALFORMED


# ---------------------------------------------------------------------------------------------- 6. larger pushes
@pytest.mark.parametrize("n", [3500, 4100], ids=["3500: 8-bit windows", "4100: 16-bit windows"])
def test_one_large_push(engine, pool, n):
    """above SSA_MSM_SMALL_MAX the one-shot takes the bucket path too; from 4096 lanes on the windows are 16 bits wide"""
    agg = pool.ref(0, n)
    with engine.aggregate_verifier(n) as av:
        av.push_aggregate(agg, pool.pks[:n], pool.msgs[:n])
        assert engine.verify_aggregate(agg, pool.pks[:n], pool.msgs[:n]) == OK
        assert av.finish(agg[49 * n:]) == OK
        assert av.finish(pool.e(0, n - 1)) == INVALID
        assert (av.record() == expected_record(engine, *pool.body(0, n))).all()
        assert av.finish(pool.e(0, 3000), 3000) == OK


# ---------------------------------------------------------------------------------------------- 7. above one MSM slice
def test_more_lanes_than_one_msm_slice(pool):
    """a context whose MSM slice is 512 lanes: a push above it is refused, and finish walks the 1288 held lanes in three
    pieces whose records are added up -- the same verdicts"""
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
        with tight.aggregate_verifier(TOTAL) as av:
            av.push(*pool.body(0, 100))
            info, rec = av.info(), av.record()
            with pytest.raises(RuntimeError):
                av.push(*pool.body(100, 613))                             # n above the slice
            assert av.info() == info and (av.record() == rec).all()
            lo = 100
            for cnt in (412, 511, 265):
                av.push(*pool.body(lo, lo + cnt))
                lo += cnt
            for n in (TOTAL, 1025, 1024, 513, 512):
                assert av.finish(pool.e(0, n), n) == OK, n
                assert av.finish(pool.e(0, n - 1), n) == INVALID, n
        rs, pks, msgs, inf, e_agg = spoil(tight, pool, "key off the curve")
        with tight.aggregate_verifier(TOTAL) as av:                       # the bad lane sits in the second piece
            for lo in range(0, TOTAL, 500):
                av.push(rs[lo:lo + 500], pks[lo:lo + 500], msgs[lo:lo + 500])
            assert av.finish(e_agg) == MALFORMED
            assert av.finish(pool.e(0, 1023), 1023) == OK
    finally:
        tight.close()


# ---------------------------------------------------------------------------------------------- 8. refusals
def test_refusals_change_nothing(engine, pool):
    import schnorr_sig_amd as ssa
    for capacity, block in ((0, 0), (8, 3), (8, 1024), (8, 1), ((1 << 30) + 1, 0)):
        with pytest.raises(RuntimeError):
            engine.aggregate_verifier(capacity, block)
    h = ssa.C.c_void_p()
    assert ssa._lib.ssa_aggverifier_create(engine._ctx, 8, 0, 1, ssa.C.byref(h)) == ssa.ERR_ARG and not h.value   # a flag
    with engine.aggregate_verifier(10, 4) as av:
        av.push(*pool.body(0, 6))
        info, rec = av.info(), av.record()
        unchanged = lambda: av.info() == info and (av.record() == rec).all()
        with pytest.raises(RuntimeError):
            av.push(*pool.body(6, 11))                                    # 5 lanes, room for 4
        assert unchanged()
        with pytest.raises(RuntimeError):
            av.finish(pool.e(0, 7), 7)                                    # n_take above the lanes held
        with pytest.raises(RuntimeError):
            av.record(7)
        assert unchanged()
        other = ssa.Engine(0)
        try:
            with pytest.raises(RuntimeError):
                av.push(*pool.body(6, 8), engine=other)                   # a context other than the object's
            e = np.array(pool.e(0, 6))
            assert ssa._lib.ssa_aggverifier_finish(other._ctx, av.handle, ssa._ptr(e), 6) == ssa.ERR_ARG
        finally:
            other.close()
        assert unchanged()
        av.push(*pool.body(6, 10))                                        # exactly fills the capacity
        assert av.info()["held"] == 10 and av.finish(pool.e(0, 10)) == OK
        with pytest.raises(RuntimeError):
            av.push(*pool.body(10, 11))
        assert av.push(*pool.body(10, 10)) == 0                           # an empty push still fits
        assert av.finish(pool.e(0, 10)) == OK


# ---------------------------------------------------------------------------------------------- 9. no state in workspaces
def test_state_does_not_live_in_workspaces(engine, pool):
    """two verifiers on one context, pushes interleaved, the context's workspaces poisoned and used by unrelated calls in
    between: each object's verdicts are those of its own lanes"""
    lo_b = 2000
    other = (pool.sigs[3000:3700], pool.pks[3000:3700], pool.msgs[3000:3700])
    agg_other = pool.ref(3000, 3700)

    def disturb(step):
        engine.debug_poison_workspaces(0xA5)
        if step % 3 == 0:
            status, nf = engine.verify_many(*other)
            assert nf == 0 and not status.any()
        elif step % 3 == 1:
            assert engine.verify_aggregate(agg_other, other[1], other[2]) == OK
        else:
            st, agg, _, nf = engine.aggregate(*other)
            assert st == OK and (agg == agg_other).all()
        engine.debug_poison_workspaces(0x5A)

    with engine.aggregate_verifier(TOTAL) as a, engine.aggregate_verifier(TOTAL, 8) as b:
        la, lb = 0, lo_b
        for j, cnt in enumerate(PUSHES):
            a.push(*pool.body(la, la + cnt))
            la += cnt
            disturb(j)
            b.push(*pool.body(lb, lb + PUSHES[-1 - j]))
            lb += PUSHES[-1 - j]
            disturb(j + 1)
            assert a.finish(pool.e(0, la)) == OK, j
        disturb(0)
        assert b.finish(pool.e(lo_b, lo_b + TOTAL)) == OK
        assert b.finish(pool.e(0, TOTAL)) == INVALID
        disturb(1)
        assert a.finish(pool.e(0, 513), 513) == OK
        assert a.finish(pool.e(0, TOTAL)) == OK


def test_producer_bytes_are_accepted(engine, pool):
    """one aggregator and one verifier over the same signatures, push by push: what the producer finishes, the validator
    accepts"""
    with engine.aggregator(TOTAL) as ag, engine.aggregate_verifier(TOTAL) as av:
        lo = 0
        for cnt in PUSHES:
            status, kept = ag.push(pool.sigs[lo:lo + cnt], pool.pks[lo:lo + cnt], pool.msgs[lo:lo + cnt])
            assert kept == cnt
            av.push(*pool.body(lo, lo + cnt))
            lo += cnt
            engine.debug_poison_workspaces(0xC3)
            produced = ag.finish_bytes()
            assert (produced == pool.ref(0, lo)).all()
            assert av.finish(produced[49 * lo:]) == OK, lo
        half = ag.finish_bytes(600)
        assert av.finish(half[49 * 600:], 600) == OK and av.finish(half[49 * 600:], 601) == INVALID


# ---------------------------------------------------------------------------------------------- 10. reset
def test_reset_starts_over(engine, pool):
    with engine.aggregate_verifier(TOTAL) as av:
        av.push(*pool.body(700, 1400))                                    # other lanes first: a block and a ragged tail
        assert av.finish(pool.e(700, 1400)) == OK
        av.reset()
        assert av.info() == dict(held=0, capacity=TOTAL, block_lanes=512, pushes=0, pushed=0, reserved=0, blocks=0,
                                 finishes=0)
        assert av.finish(np.zeros(32, np.uint8)) == OK
        lo = 0
        for cnt in PUSHES:
            av.push(*pool.body(lo, lo + cnt))
            lo += cnt
        assert av.finish(pool.e(0, TOTAL)) == OK
        assert av.info() == dict(held=TOTAL, capacity=TOTAL, block_lanes=512, pushes=len(PUSHES), pushed=TOTAL,
                                 reserved=0, blocks=2, finishes=2)


# ---------------------------------------------------------------------------------------------- 11. device forms
def test_device_forms_verdict_word_alone_is_written(engine, pool):
    import torch
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    d_rs, d_pks, d_msgs = (dev(a) for a in pool.body(0, TOTAL))
    with engine.aggregate_verifier(TOTAL) as av:
        lo = 0
        for cnt in PUSHES:
            assert av.push_device(d_rs[lo:lo + cnt], d_pks[lo:lo + cnt], d_msgs[lo:lo + cnt]) == cnt
            lo += cnt
        assert av.info()["held"] == TOTAL
        for n, scalar, want in ((TOTAL, pool.e(0, TOTAL), OK), (1025, pool.e(0, 1025), OK), (512, pool.e(0, 513), INVALID),
                                (1, pool.e(0, 1), OK), (0, np.zeros(32, np.uint8), OK), (0, pool.e(0, 1), INVALID)):
            words = torch.full((8,), 0x6EEEEEEE, dtype=torch.int32, device="cuda:0")
            d_e = dev(np.array(scalar))
            torch.cuda.synchronize()
            av.finish_device(d_e, words[3:4], n)                          # an odd word offset
            engine.sync()
            got = words.cpu().numpy()
            assert got[3] == want, (n, got)
            assert (np.delete(got, 3) == 0x6EEEEEEE).all(), (n, got)
            assert av.finish(scalar, n) == want
