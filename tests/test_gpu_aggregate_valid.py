"""Filtering half-aggregation (ssa_aggregate_valid_many).  The contract is one equality: with S the
statuses of ssa_verify_batch_screened and K the lanes whose status is zero, the call returns K, S and -- byte for byte --
the aggregate ssa_aggregate_many gives the lanes of K handed in alone, with zeros behind both.  The tests hold the
compaction alone against numpy, the equality against the CPU oracle, the model of tests/aggregate_model.py and the
existing calls, and the independence of whatever ran before on the context."""
import ctypes as C
import os

import numpy as np
import pytest

import aggregate_model as am

pytestmark = pytest.mark.gpu

OK, INVALID, MALFORMED = 0, 2, 3
FILL = 0xEE
EQUALITY_SIZES = [1, 2, 3, 64, 65, 257, 1025, 3072, 3073, 3300]          # both sides of the default msm_small_max
KEEP_SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 65535, 65536, 65537, (1 << 23) - 1, 1 << 23]


def make_scalars(rng, n):
    s = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    s[:, 31] &= 0x3F
    s[:, 0] |= 1
    return s


def dev(*arrays):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0") for a in arrays]


# ---------------------------------------------------------------------------------------------- 1. the compaction alone
def keep_patterns(n):
    """status vectors of n bytes: zero = kept; the nonzero bytes take both values a status has, 2 and 3"""
    rng = np.random.default_rng(0x4EE9 + n)
    bad = lambda: rng.choice(np.array([2, 3], np.uint8), size=n)
    out = {"all kept": np.zeros(n, np.uint8), "none kept": bad()}
    if n == 0:
        return out
    for name, lane in (("only lane 0", 0), ("only the last lane", n - 1)):
        s = bad()
        s[lane] = 0
        out[name] = s
    out["alternating"] = ((np.arange(n) & 1) * 2).astype(np.uint8)
    out["alternating, lane 0 dropped"] = (((np.arange(n) + 1) & 1) * 3).astype(np.uint8)
    for name, p_bad in (("half dropped", 0.5), ("1 % dropped", 0.01), ("1 % kept", 0.99)):
        out[name] = np.where(rng.random(n) < p_bad, bad(), 0).astype(np.uint8)
    s = np.where(rng.random(n) < 0.1, bad(), 0).astype(np.uint8)
    s[:256 * min(3, n // 256)] = 2                                         # whole workgroups dropped at the front
    out["blocks dropped at the front"] = s
    s = np.where(rng.random(n) < 0.1, bad(), 0).astype(np.uint8)
    mid = (n // 512) * 256
    s[mid:mid + 512] = 3                                                   # ... and in the middle
    out["blocks dropped in the middle"] = s
    return out


@pytest.mark.parametrize("n", KEEP_SIZES)
def test_compaction_alone(engine, n):
    for name, status in keep_patterns(n).items():
        kept, whole = engine.debug_aggregate_keep(status)
        want = np.flatnonzero(status == 0).astype(np.uint32)
        assert kept.size == want.size, (name, kept.size, want.size)
        assert (kept == want).all(), (name, np.flatnonzero(kept != want)[:8])
        assert whole.size == n and not whole[want.size:].any(), name


# ---------------------------------------------------------------------------------------------- batches with bad lanes
class Batch:
    """n honest signatures over 80-byte messages; with_identity_lane puts one of them under the identity key"""

    def __init__(self, engine, n):
        rng = np.random.default_rng(0xA7A11D + n)
        self.n = n
        self.msgs = rng.integers(0, 256, size=(n, 80), dtype=np.uint8)
        self.pks, self.sigs = engine.keygen_sign_many(make_scalars(rng, n), make_scalars(rng, n), self.msgs)
        self.inf = np.zeros(n, np.uint8)
        self.ident = None

    def with_identity_lane(self, engine, k):
        """lane k: R = [e]G verifies under the identity key with any message, since [h]O adds nothing"""
        e = make_scalars(np.random.default_rng(0x1D + self.n), 1)
        comp, st = engine.compress_many(engine.pubkey_many(e))
        assert (st == 0).all()
        self.sigs[k], self.pks[k], self.inf[k], self.ident = np.concatenate([comp[0], e[0]]), 0, 1, k
        return self


WAYS = ("message bit", "bit of e", "sort bit of R", "e >= q", "key off the curve", "R does not decode")


def corrupt(b, lanes, ways=WAYS):
    """copies of b's arrays with lane lanes[j] made a rejection the way ways[j % len(ways)] says"""
    import pymodel as pm
    sigs, pks, msgs = b.sigs.copy(), b.pks.copy(), b.msgs.copy()
    for j, k in enumerate(lanes):
        way = ways[j % len(ways)]
        if way == "message bit":
            msgs[k, 17] ^= 0x04
        elif way == "bit of e":
            sigs[k, 49] ^= 0x01
        elif way == "sort bit of R":
            sigs[k, 48] ^= 0x40
        elif way == "e >= q":
            sigs[k, 49:81] = 0xFF
        elif way == "key off the curve":
            pks[k, 48] ^= 0x01
        else:
            for t in range(1, 64):                                         # an x with no point on the curve
                x = b.sigs[k, :49].copy()
                x[8] ^= t
                if pm.pt_decompress(x.tobytes())[0] == "invalid":
                    break
            sigs[k, :49] = x
    return sigs, pks, msgs


def bad_lanes(n, rng):
    """lane 0, lane n - 1, both sides of the first wave edge, and about 1 % at random; small batches keep a lane"""
    if n == 1:
        return []
    if n == 2:
        return [1]
    lanes = {0, n - 1} | ({63, 64} if n > 65 else {63} if n > 64 else set())
    lanes |= set(int(k) for k in rng.choice(n, size=n // 100, replace=False)) if n >= 100 else set()
    return sorted(lanes)


def raw_valid(engine, sigs, pks, msgs, offsets=None, pk_inf=None, with_status=True):
    """the C call on buffers of full capacity filled with 0xEE -> (rc, agg[49 n + 32], kept[n], n_kept, status[n])"""
    import schnorr_sig_amd as ssa
    n, batch, keep = engine._agg_batch(sigs, 81, pks, msgs, offsets, pk_inf)
    agg = np.full(49 * n + 32, FILL, np.uint8)
    kept = np.full(max(n, 1), 0xEEEEEEEE, np.uint32)
    status = np.full(max(n, 1), FILL, np.uint8)
    nk = C.c_uint64(1 << 40)
    rc = ssa._lib.ssa_aggregate_valid_many(engine._ctx, *batch, ssa._ptr(agg), ssa._ptr(kept), C.byref(nk),
                                           ssa._ptr(status) if with_status else None)
    return rc, agg, kept[:n], int(nk.value), status[:n]


def check_contract(engine, sigs, pks, msgs, inf, want_kept):
    """every clause of the header's contract but the oracle's; returns the aggregate of the kept lanes"""
    n = len(sigs)
    rc, agg, kept, m, status = raw_valid(engine, sigs, pks, msgs, pk_inf=inf)
    want_kept = np.asarray(want_kept, np.uint32)
    assert rc == 0 and m == want_kept.size and (kept[:m] == want_kept).all()
    assert not kept[m:].any() and not agg[49 * m + 32:].any()
    scr, nf = engine.verify_batch_screened(sigs, pks, msgs, pk_inf=inf)
    assert (status == scr).all() and nf == n - m
    K = kept[:m].astype(np.int64)
    if m == 0:
        assert not agg.any()
        return agg[:32]
    st, alone, st_lanes, nfa = engine.aggregate(sigs[K], pks[K], msgs[K], pk_inf=inf[K])
    assert st == OK and nfa == 0
    assert (agg[:49 * m + 32] == alone).all()
    return agg[:49 * m + 32]


@pytest.mark.parametrize("n", EQUALITY_SIZES)
def test_the_equality(engine, oracle, n):
    rng = np.random.default_rng(0xE90A + n)
    b = Batch(engine, n)
    lanes = bad_lanes(n, rng)
    if n >= 64:                                                           # an honest lane under the identity key: kept
        b.with_identity_lane(engine, next(k for k in range(n) if k not in lanes))
    sigs, pks, msgs = corrupt(b, lanes)
    want_kept = np.setdiff1d(np.arange(n), lanes)
    # the CPU oracle, lane by lane, under verify_batch's semantics
    per_lane = oracle.verify_many_fast(sigs, pks, msgs, check_torsion=False, pk_inf=b.inf, sig_flag_byte=True, threads=16)
    assert (np.flatnonzero(per_lane == 0) == want_kept).all()
    agg = check_contract(engine, sigs, pks, msgs, b.inf, want_kept)
    K = want_kept
    if K.size:
        model = np.frombuffer(am.aggregate(am.oracle_backend(oracle), sigs[K], pks[K], msgs[K]), np.uint8)
        assert (agg == model).all()
    # the mirror's trimmed results
    got_agg, got_kept, got_status = engine.aggregate_valid(sigs, pks, msgs, pk_inf=b.inf)
    assert (got_agg == agg).all() and (got_kept == K).all() and (np.flatnonzero(got_status == 0) == K).all()
    assert (got_status[lanes] != 0).all()
    # the aggregate verifies with the kept keys and messages, and not with one kept lane's message exchanged
    assert engine.verify_aggregate(agg, pks[K], msgs[K], pk_inf=b.inf[K]) == OK
    if K.size:
        other = msgs[K].copy()
        j = next(i for i in range(K.size) if K[i] != b.ident)             # (the identity lane verifies with any message,
        other[j, 3] ^= 0x10                                               #  but its digest still enters the transcript)
        assert engine.verify_aggregate(agg, pks[K], other, pk_inf=b.inf[K]) == INVALID


# ---------------------------------------------------------------------------------------------- 3. |K| across the tree span
_B600 = {}


def batch600(engine):
    if not _B600:
        _B600["b"] = Batch(engine, 600)
    return _B600["b"]


@pytest.mark.parametrize("dropped", [87, 88, 89])
def test_kept_count_across_the_tree_span(engine, dropped):
    """|K| = 513, 512 and 511: one workgroup of ag_k_tree more or less, sized by |K| and not by n"""
    b = batch600(engine)
    rng = np.random.default_rng(0x513 + dropped)
    lanes = sorted(int(k) for k in rng.choice(600, size=dropped, replace=False))
    sigs, pks, msgs = corrupt(b, lanes, WAYS[:5])
    agg = check_contract(engine, sigs, pks, msgs, b.inf, np.setdiff1d(np.arange(600), lanes))
    assert agg.size == 49 * (600 - dropped) + 32


def test_all_bad_and_none_bad(engine):
    b = batch600(engine)
    sigs, pks, msgs = corrupt(b, list(range(600)), WAYS[:5])
    agg = check_contract(engine, sigs, pks, msgs, b.inf, [])
    assert agg.size == 32 and not agg.any()
    assert engine.verify_aggregate(agg, np.zeros((0, 96), np.uint8), None) == OK
    got_agg, got_kept, got_status = engine.aggregate_valid(sigs, pks, msgs)
    assert got_agg.size == 32 and got_kept.size == 0 and (got_status != 0).all()
    agg = check_contract(engine, b.sigs, b.pks, b.msgs, b.inf, np.arange(600))
    st, whole, _, _ = engine.aggregate(b.sigs, b.pks, b.msgs)
    assert st == OK and (agg == whole).all()


def test_empty_batch(engine):
    rc, agg, kept, m, status = raw_valid(engine, np.zeros((0, 81), np.uint8), np.zeros((0, 96), np.uint8), None)
    assert rc == 0 and m == 0 and agg.size == 32 and not agg.any()
    got_agg, got_kept, got_status = engine.aggregate_valid(np.zeros((0, 81), np.uint8), np.zeros((0, 96), np.uint8), None)
    assert got_agg.size == 32 and not got_agg.any() and got_kept.size == 0 and got_status.size == 0


# ---------------------------------------------------------------------------------------------- 4. more than 256 block totals
def test_more_than_256_block_totals(engine):
    n = 65536 + 300
    b = Batch(engine, n)
    rng = np.random.default_rng(0xB10C)
    lanes = sorted(int(k) for k in rng.choice(n, size=n // 100, replace=False))
    sigs, pks, msgs = corrupt(b, lanes, WAYS[:4])
    check_contract(engine, sigs, pks, msgs, b.inf, np.setdiff1d(np.arange(n), lanes))


# ---------------------------------------------------------------------------------------------- 5. layouts, paths, forms
@pytest.fixture(scope="module")
def engines():
    """contexts whose screen takes one path whatever the size: "small" the exact per-lane kernel, "bucket" the MSM"""
    import schnorr_sig_amd as ssa
    made = {}
    old = os.environ.get("SSA_MSM_SMALL_MAX")
    try:
        for name, bound in (("small", 1 << 40), ("bucket", 0)):
            os.environ["SSA_MSM_SMALL_MAX"] = str(bound)
            made[name] = ssa.Engine(0)
    finally:
        if old is None:
            os.environ.pop("SSA_MSM_SMALL_MAX", None)
        else:
            os.environ["SSA_MSM_SMALL_MAX"] = old
    yield made
    for e in made.values():
        e.close()


def valid_on_device(eng, sigs, pks, msgs, offsets=None, inf=None, with_status=True):
    """the device form on buffers of full capacity filled with 0xEE -> (agg, kept, n_kept, status), all of them whole"""
    import torch
    n = len(sigs)
    ds, dp, dm = dev(sigs, pks, msgs)
    d_off = dev(np.asarray(offsets, np.uint64).view(np.int64))[0] if offsets is not None else None
    d_inf = dev(inf)[0] if inf is not None else None
    d_agg = torch.full((49 * n + 32,), FILL, dtype=torch.uint8, device="cuda:0")
    d_kept = torch.full((n,), -1, dtype=torch.int32, device="cuda:0")
    d_st = torch.full((n,), FILL, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    m = eng.aggregate_valid_device(ds.data_ptr(), dp.data_ptr(), dm.data_ptr(), n, 0 if offsets is not None else msgs.shape[1],
                                   d_agg.data_ptr(), d_kept.data_ptr(), d_st.data_ptr() if with_status else 0,
                                   d_offsets=d_off.data_ptr() if d_off is not None else 0,
                                   d_pk_inf=d_inf.data_ptr() if d_inf is not None else 0)
    eng.sync()
    return d_agg.cpu().numpy(), d_kept.cpu().numpy().view(np.uint32), m, d_st.cpu().numpy()


@pytest.mark.parametrize("layout", ["stride", "offsets"])
def test_layouts_screen_paths_and_device_form(engine, engines, layout):
    import schnorr_sig_amd as ssa
    n = 300
    rng = np.random.default_rng(0x1A70 + len(layout))
    if layout == "stride":
        msgs, off = rng.integers(0, 256, size=(n, 80), dtype=np.uint8), None
    else:
        lens = rng.integers(0, 100, size=n)
        lens[[0, 7, n - 1]] = 0                                            # zero-length messages, the first and last too
        rows = [rng.bytes(int(k)) for k in lens]
        msgs, off = ssa.pack_messages(rows)
    pks, sigs = engine.keygen_sign_many(make_scalars(rng, n), make_scalars(rng, n), msgs, offsets=off)
    lanes = [0, 63, 64, 150, 255, 256, n - 1]
    sigs = sigs.copy()
    sigs[lanes[::2], 49] ^= 1
    sigs[lanes[1::2], 49:81] = 0xFF
    inf = np.zeros(n, np.uint8)
    want_kept = np.setdiff1d(np.arange(n), lanes).astype(np.uint32)
    m = want_kept.size
    rc, agg, kept, nk, status = raw_valid(engine, sigs, pks, msgs, offsets=off, pk_inf=inf)
    assert rc == 0 and nk == m and (kept[:m] == want_kept).all()
    assert (status[lanes[::2]] == INVALID).all() and (status[lanes[1::2]] == MALFORMED).all()
    for name in ("small", "bucket"):
        eng = engines[name]
        rc2, agg2, kept2, nk2, status2 = raw_valid(eng, sigs, pks, msgs, offsets=off, pk_inf=inf)
        assert rc2 == 0 and nk2 == m, name
        assert (agg2 == agg).all() and (kept2 == kept).all() and (status2 == status).all(), name
        for with_inf in (inf, None):
            d_agg, d_kept, d_m, d_status = valid_on_device(eng, sigs, pks, msgs, offsets=off, inf=with_inf)
            assert d_m == m, name
            assert (d_agg == agg).all() and (d_kept == kept).all() and (d_status == status).all(), name
    # the kept lanes' aggregate verifies with their keys and messages, in the same layout
    K = want_kept.astype(np.int64)
    if off is None:
        k_msgs, k_off = msgs[K], None
    else:
        k_msgs, k_off = ssa.pack_messages([rows[i] for i in K])
    assert engine.verify_aggregate(agg[:49 * m + 32], pks[K], k_msgs, offsets=k_off) == OK
    st, alone, _, _ = engine.aggregate(sigs[K], pks[K], k_msgs, offsets=k_off)
    assert st == OK and (alone == agg[:49 * m + 32]).all()


# ---------------------------------------------------------------------------------------------- 6. independence
def test_independence_of_earlier_calls(engine):
    import schnorr_sig_amd as ssa
    b = Batch(engine, 3300)
    rng = np.random.default_rng(0x1DE9)
    lanes = bad_lanes(3300, rng)
    sigs, pks, msgs = corrupt(b, lanes, WAYS[:5])
    small = batch600(engine)
    fresh = ssa.Engine(0)
    try:
        want = raw_valid(fresh, sigs, pks, msgs, pk_inf=b.inf)
    finally:
        fresh.close()
    assert want[0] == 0 and want[3] == 3300 - len(lanes)

    def same(got):
        assert got[0] == want[0] and got[3] == want[3]
        assert all((g == w).all() for g, w in zip((got[1], got[2], got[4]), (want[1], want[2], want[4])))

    def dirty():
        engine.verify_many(small.sigs, small.pks, small.msgs)                          # another family
        st, agg, _, nf = engine.aggregate(sigs, pks, msgs, pk_inf=b.inf, check=True)   # refused: a zeroed aggregate
        assert st != OK and nf == len(lanes) and not agg.any()

    # what the existing calls give before ...
    before = (engine.aggregate(b.sigs, b.pks, b.msgs, pk_inf=b.inf, check=True),
              engine.verify_aggregate(want[1][:49 * want[3] + 32], pks[want[2][:want[3]]], msgs[want[2][:want[3]]],
                                      pk_inf=b.inf[want[2][:want[3]]]),
              engine.verify_many(sigs, pks, msgs, pk_inf=b.inf, check_torsion=False, sig_flag_byte=True))
    assert before[0][0] == OK and before[1] == OK and before[2][1] == len(lanes)
    for prelude in (lambda: engine.debug_poison_workspaces(0xA5), dirty, lambda: engine.debug_poison_workspaces(0xFF),
                    lambda: None):                                                     # (the last: twice in a row)
        prelude()
        same(raw_valid(engine, sigs, pks, msgs, pk_inf=b.inf))
    # ... and after the new call
    after = (engine.aggregate(b.sigs, b.pks, b.msgs, pk_inf=b.inf, check=True),
             engine.verify_aggregate(want[1][:49 * want[3] + 32], pks[want[2][:want[3]]], msgs[want[2][:want[3]]],
                                     pk_inf=b.inf[want[2][:want[3]]]),
             engine.verify_many(sigs, pks, msgs, pk_inf=b.inf, check_torsion=False, sig_flag_byte=True))
    assert after[0][0] == before[0][0] and (after[0][1] == before[0][1]).all() and (after[0][2] == before[0][2]).all()
    assert after[1] == before[1]
    assert (after[2][0] == before[2][0]).all() and after[2][1] == before[2][1]
    # no status vector wanted: host and device form
    got = raw_valid(engine, sigs, pks, msgs, pk_inf=b.inf, with_status=False)
    assert got[0] == 0 and got[3] == want[3] and (got[1] == want[1]).all() and (got[2] == want[2]).all()
    assert (got[4] == FILL).all()
    d_agg, d_kept, d_m, d_status = valid_on_device(engine, sigs, pks, msgs, inf=b.inf, with_status=False)
    assert d_m == want[3] and (d_agg == want[1]).all() and (d_kept == want[2]).all() and (d_status == FILL).all()


def test_argument_errors(engine):
    import schnorr_sig_amd as ssa
    b = batch600(engine)
    n, batch, keep = engine._agg_batch(b.sigs, 81, b.pks, b.msgs, None, None)
    agg, kept, nk = np.zeros(49 * n + 32, np.uint8), np.zeros(n, np.uint32), C.c_uint64(0)
    p = ssa._ptr
    call = lambda ctx, a, k, c: ssa._lib.ssa_aggregate_valid_many(ctx, *batch, a, k, c, None)
    assert call(engine._ctx, p(agg), p(kept), C.byref(nk)) == 0 and nk.value == n
    assert call(None, p(agg), p(kept), C.byref(nk)) == ssa.ERR_ARG
    assert call(engine._ctx, None, p(kept), C.byref(nk)) == ssa.ERR_ARG
    assert call(engine._ctx, p(agg), None, C.byref(nk)) == ssa.ERR_ARG
    assert call(engine._ctx, p(agg), p(kept), None) == ssa.ERR_ARG
    import torch
    ds, dp, dm = dev(b.sigs, b.pks, b.msgs)
    d_agg = torch.zeros(49 * n + 32, dtype=torch.uint8, device="cuda:0")
    d_kept = torch.zeros(n, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    dcall = lambda a, k, c: ssa._lib.ssa_aggregate_valid_many_device(
        engine._ctx, ds.data_ptr(), dp.data_ptr(), None, dm.data_ptr(), None, 80, 80, n, a, k, c, None)
    assert dcall(d_agg.data_ptr(), d_kept.data_ptr(), C.byref(nk)) == 0 and nk.value == n
    assert dcall(None, d_kept.data_ptr(), C.byref(nk)) == ssa.ERR_ARG
    assert dcall(d_agg.data_ptr(), None, C.byref(nk)) == ssa.ERR_ARG
    assert dcall(d_agg.data_ptr(), d_kept.data_ptr(), None) == ssa.ERR_ARG
    engine.sync()
    assert ssa._lib.ssa_debug_aggregate_keep(engine._ctx, None, 5, p(kept), C.byref(nk)) == ssa.ERR_ARG
    assert ssa._lib.ssa_debug_aggregate_keep(engine._ctx, p(agg), 5, p(kept), None) == ssa.ERR_ARG
    # n above the context's MSM slice
    old = os.environ.get("SSA_MSM_SLICE")
    os.environ["SSA_MSM_SLICE"] = "512"
    try:
        tight = ssa.Engine(0)
    finally:
        if old is None:
            os.environ.pop("SSA_MSM_SLICE", None)
        else:
            os.environ["SSA_MSM_SLICE"] = old
    try:
        assert ssa._lib.ssa_aggregate_valid_many(tight._ctx, *batch, p(agg), p(kept), C.byref(nk), None) == ssa.ERR_ARG
        got_agg, got_kept, _ = tight.aggregate_valid(b.sigs[:512], b.pks[:512], b.msgs[:512])
        assert got_kept.size == 512 and (got_agg == engine.aggregate(b.sigs[:512], b.pks[:512], b.msgs[:512])[1]).all()
    finally:
        tight.close()


# ---------------------------------------------------------------------------------------------- 7. the object mirror
def test_objects_mirror(engine):
    import schnorr_sig_amd as ssa
    gen = np.random.default_rng(0x0B1EC8)
    rng = lambda k: gen.bytes(k)
    pairs = [ssa.KeyPair.new(rng, engine) for _ in range(4)]
    msgs = [b"one", b"", b"three" * 20, b"four"]
    sigs = [kp.sign(m, rng, engine) for kp, m in zip(pairs, msgs)]
    pks = [kp.public_key for kp in pairs]
    forged = list(sigs)
    forged[2] = sigs[3]                                                    # an honest signature of another triple
    agg, kept = ssa.AggregateSignature.aggregate_valid(forged, pks, msgs, engine=engine)
    assert kept == [0, 1, 3] and len(agg) == 3
    sub = lambda xs: [xs[i] for i in kept]
    assert agg == ssa.AggregateSignature.aggregate(sub(sigs), sub(pks), sub(msgs), engine=engine)
    assert agg.verify(sub(pks), sub(msgs), engine=engine) is None
    with pytest.raises(ssa.SignatureError):
        agg.verify(sub(pks), [b"one", b"x", b"four"], engine=engine)
    whole, all_kept = ssa.AggregateSignature.aggregate_valid(sigs, pks, msgs, engine=engine)
    assert all_kept == [0, 1, 2, 3] and whole == ssa.AggregateSignature.aggregate(sigs, pks, msgs, engine=engine)
    empty, none = ssa.AggregateSignature.aggregate_valid([], [], [], engine=engine)
    assert none == [] and empty.verify([], [], engine=engine) is None
