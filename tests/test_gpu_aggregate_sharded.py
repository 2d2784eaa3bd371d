"""Sharded half-aggregation on the GPU: slices of one context, several contexts in one process and
several processes produce the aggregate of ssa_aggregate_many byte for byte and the verdict of ssa_verify_aggregate, for
sizes on both sides of every slice and block boundary.  Every comparison is of exact bytes or exact verdicts; the
references are the single calls on a default context and, for the coefficients, tests/aggregate_model.py over the oracle."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import aggregate_model as am

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q = am.Q
OK, INVALID, MALFORMED = 0, 2, 3
N3 = 3 * 512 + 1            # three slices of 512 and a ragged fourth of one lane


def make_scalars(rng, n):
    s = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    s[:, 31] &= 0x3F
    s[:, 0] |= 1
    return s


def engine_under(**env):
    """an Engine (or, devices=[...], a MultiEngine) created under these environment knobs, which are restored at once:
    a context reads them when it is made"""
    import schnorr_sig_amd as ssa
    devices = env.pop("devices", None)
    old = {k: os.environ.get(k) for k in env}
    os.environ.update({k: str(v) for k, v in env.items()})
    try:
        return ssa.MultiEngine(devices) if devices else ssa.Engine(0)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def tight():
    eng = engine_under(SSA_MSM_SLICE=512)
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def bucket():
    eng = engine_under(SSA_MSM_SLICE=2048, SSA_MSM_SMALL_MAX=256)
    yield eng
    eng.close()


class Batch:
    """n honest signatures and what the single call on the default context makes of them (computed once per shape)"""

    def __init__(self, engine, n, ragged, seed=0x5A4D0):
        import schnorr_sig_amd as ssa
        rng = np.random.default_rng(seed + 2 * n + ragged)
        self.n = n
        if ragged:
            self.msgs, self.off = ssa.pack_messages([rng.bytes(int(rng.integers(0, 100))) for _ in range(n)])
        else:
            self.msgs, self.off = rng.integers(0, 256, size=(n, 80), dtype=np.uint8), None
        self.pks, self.sigs = engine.keygen_sign_many(make_scalars(rng, n), make_scalars(rng, n), self.msgs, offsets=self.off)
        st, self.agg, _, _ = engine.aggregate(self.sigs, self.pks, self.msgs, offsets=self.off)
        assert st == OK and engine.verify_aggregate(self.agg, self.pks, self.msgs, offsets=self.off) == OK
        self.e_agg = int.from_bytes(self.agg[-32:].tobytes(), "little")


_BATCHES = {}


@pytest.fixture
def batch(engine):
    def get(n, ragged=False):
        if (n, ragged) not in _BATCHES:
            _BATCHES[(n, ragged)] = Batch(engine, n, ragged)
        return _BATCHES[(n, ragged)]
    return get


def with_e(agg, e):
    out = agg.copy()
    out[-32:] = np.frombuffer(int(e).to_bytes(32, "little"), np.uint8)
    return out


def sliced_equals_single(eng, engine, b):
    st, agg, status, nf = eng.aggregate_sliced(b.sigs, b.pks, b.msgs, offsets=b.off)
    assert st == OK and nf == 0 and (status == 0).all()
    assert agg.size == b.agg.size and (agg == b.agg).all()
    assert eng.verify_aggregate_sliced(agg, b.pks, b.msgs, offsets=b.off) == OK
    assert engine.verify_aggregate(agg, b.pks, b.msgs, offsets=b.off) == OK


# ------------------------------------------------------------------------------------------ 1. sliced equals single
@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("n", [1, 511, 512, 513, 1024, 1025, 1537])
def test_sliced_equals_single(engine, tight, batch, n, ragged):
    import schnorr_sig_amd as ssa
    b = batch(n, ragged)
    if n > 512:          # what the sliced forms are for: the single calls of this context refuse the size
        none = C.c_void_p()
        assert ssa._lib.ssa_verify_aggregate(tight._ctx, b.agg.ctypes.data, b.pks.ctypes.data, none, b.msgs.ctypes.data,
                                             none if b.off is None else b.off.ctypes.data, 0 if ragged else 80,
                                             0 if ragged else 80, n) == ssa.ERR_ARG
    sliced_equals_single(tight, engine, b)


@pytest.mark.parametrize("ragged", [False, True])
def test_sliced_equals_single_on_the_bucket_path(engine, bucket, batch, ragged):
    """slices of 2048, 2048 and 904 lanes, every one above the small-batch bound of the MSM"""
    sliced_equals_single(bucket, engine, batch(5000, ragged))


def test_empty_aggregate_follows_its_rule(tight):
    none = np.zeros((0, 96), np.uint8)
    st, agg, status, nf = tight.aggregate_sliced(np.zeros((0, 81), np.uint8), none, None)
    assert st == OK and agg.size == 32 and not agg.any() and nf == 0
    assert tight.verify_aggregate_sliced(agg, none, None) == OK
    assert tight.verify_aggregate_sliced(with_e(agg, 1), none, None) == INVALID
    assert tight.verify_aggregate_sliced(with_e(agg, Q), none, None) == MALFORMED


def test_device_forms_on_poisoned_workspaces_and_after_a_dirty_predecessor(engine, tight, batch):
    """the device forms give the host forms' bytes, and on ONE context -- after its workspaces were poisoned, and after an
    unrelated screened call and an aggregate of another size -- the sliced calls give what they gave before"""
    import torch
    b, other = batch(N3), batch(1025)
    ds, dp, dm = [torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0") for a in (b.sigs, b.pks, b.msgs)]
    d_agg = torch.full((49 * b.n + 32,), 255, dtype=torch.uint8, device="cuda:0")
    d_st = torch.full((b.n,), 255, dtype=torch.uint8, device="cuda:0")
    d_nf = torch.full((1,), -1, dtype=torch.int64, device="cuda:0")
    d_v = torch.full((1,), 255, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    for check in (False, True):
        st = tight.aggregate_sliced_device(ds.data_ptr(), dp.data_ptr(), dm.data_ptr(), b.n, 80, d_agg.data_ptr(),
                                           d_st.data_ptr(), d_nf.data_ptr(), check=check)
        tight.verify_aggregate_sliced_device(d_agg.data_ptr(), dp.data_ptr(), dm.data_ptr(), b.n, 80, d_v.data_ptr())
        tight.sync()
        assert (st, int(d_nf.item()), int(d_v.item())) == (OK, 0, OK)
        assert (d_agg.cpu().numpy() == b.agg).all() and not d_st.cpu().numpy().any()
    for prelude in (lambda: tight.debug_poison_workspaces(0xA5),
                    lambda: (tight.verify_batch_screened(other.sigs[:512], other.pks[:512], other.msgs[:512]),
                             tight.aggregate_sliced(other.sigs, other.pks, other.msgs)),
                    lambda: tight.debug_poison_workspaces(0xFF)):
        prelude()
        st, agg, status, nf = tight.aggregate_sliced(b.sigs, b.pks, b.msgs, check=True)
        assert st == OK and nf == 0 and (agg == b.agg).all() and not status.any()
        prelude()
        assert tight.verify_aggregate_sliced(b.agg, b.pks, b.msgs) == OK


# ------------------------------------------------------------------------------- 2. the result does not depend on B
def test_result_does_not_depend_on_the_block(engine, batch):
    """B = 1 makes every leaf a top, so the whole tree runs through ag_k_tree as in the single call; B = 4 takes two flat
    levels, B = 512 nine; B = 2048 is a block above the slice"""
    b = batch(N3)
    for B in (1, 4, 512, 2048):
        eng = engine_under(SSA_MSM_SLICE=512, SSA_AGG_BLOCK=B)
        try:
            st, agg, _, nf = eng.aggregate_sliced(b.sigs, b.pks, b.msgs)
            assert st == OK and nf == 0 and (agg == b.agg).all(), B
            assert eng.verify_aggregate_sliced(b.agg, b.pks, b.msgs) == OK, B
        finally:
            eng.close()


def tops_and_root(eng, d_lanes, stride, d_pks, d_msgs, n, B, d_h=0):
    import torch
    tops = torch.full((32 * -(-n // B),), 255, dtype=torch.uint8, device="cuda:0")
    root = torch.full((32,), 255, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    eng.aggregate_shard_tops_device(d_lanes.data_ptr(), stride, d_pks.data_ptr(), d_msgs.data_ptr(), n, 80, B,
                                    tops.data_ptr(), d_h=d_h)
    eng.aggregate_root_device(tops.data_ptr(), tops.numel() // 32, n, root.data_ptr(), block_lanes=B)
    eng.sync()
    return tops.cpu().numpy(), root.cpu().numpy()


def test_flat_levels_against_the_lds_tree_and_the_model(engine, oracle, batch):
    """the primitives directly: tops of B = 1 are the leaves, of B = 4 two launches of ag_k_level; the roots agree with
    each other and with the model's, and so do the coefficients derived from them, at lane 0 and from a lane base"""
    import torch
    b = batch(N3)
    be = am.oracle_backend(oracle)
    rs = np.ascontiguousarray(b.sigs[:, :49])
    leaves = am.leaves(be, rs, b.pks, b.msgs)
    felts = lambda node: np.array([int(v) for v in node], dtype=np.uint64).view(np.uint8)
    want_root = am.root_of(be, am.tree_top(be, leaves), b.n)
    want = am.coeff_bytes(am.coeffs_of_root(be, want_root, b.n))
    ds, dr, dp, dm = [torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0") for a in (b.sigs, rs, b.pks, b.msgs)]
    tops1, root1 = tops_and_root(engine, ds, 81, dp, dm, b.n, 1)
    assert (tops1.reshape(-1, 32) == np.stack([felts(v) for v in leaves])).all()
    tops4, root4 = tops_and_root(engine, dr, 49, dp, dm, b.n, 4)                 # (R's at stride 49: the validator's form)
    want_tops4 = [am.tree_top(be, leaves[lo:lo + 4]) for lo in range(0, b.n, 4)]
    assert (tops4.reshape(-1, 32) == np.stack([felts(v) for v in want_tops4])).all()
    assert (root1 == felts(want_root)).all() and (root4 == root1).all()
    got = engine.aggregate_shard_coeffs(root4, b.n, 0)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, (bad[:8], got[bad[:2]], want[bad[:2]])
    assert (engine.aggregate_shard_coeffs(root4, 300, 1027) == want[1027:1327]).all()
    assert (engine.aggregate_coeffs(rs, b.pks, b.msgs) == want).all()           # (the single call's, for the record)


# ----------------------------------------------------------------------------------- 3. rejections across the slices
def test_rejections_placed_across_slices(engine, tight, batch):
    import pymodel as pm
    b = batch(N3)
    both = lambda agg, pks=b.pks, inf=None: (tight.verify_aggregate_sliced(agg, pks, b.msgs, pk_inf=inf),
                                             engine.verify_aggregate(agg, pks, b.msgs, pk_inf=inf))
    forged = b.sigs.copy()
    forged[700, 49:] = b.sigs[701, 49:]                                    # lane 700 (the middle slice) carries another e
    st, agg_f, _, nf = tight.aggregate_sliced(forged, b.pks, b.msgs)       # (unchecked: nothing is malformed)
    assert st == OK and nf == 0 and (agg_f == engine.aggregate(forged, b.pks, b.msgs)[1]).all()
    assert both(agg_f) == (INVALID, INVALID)
    sw = b.agg.copy()
    sw[49 * 511: 49 * 512], sw[49 * 512: 49 * 513] = b.agg[49 * 512: 49 * 513], b.agg[49 * 511: 49 * 512]
    assert both(sw) == (INVALID, INVALID)                                  # the order is bound across a slice boundary
    assert both(with_e(b.agg, Q - b.e_agg)) == (INVALID, INVALID)          # -[e_agg]G has the x of [e_agg]G
    assert both(with_e(b.agg, Q)) == (MALFORMED, MALFORMED)
    assert both(with_e(b.agg, (1 << 256) - 1)) == (MALFORMED, MALFORMED)
    for t in range(1, 64):                                                 # an x with no point on the curve, lane 1536
        x = b.agg[49 * 1536: 49 * 1537].copy()
        x[8] ^= t
        if pm.pt_decompress(x.tobytes())[0] == "invalid":
            break
    un = b.agg.copy()
    un[49 * 1536: 49 * 1537] = x
    assert both(un) == (MALFORMED, MALFORMED)                              # in the last, ragged slice
    un[49 * 700: 49 * 701] = b.agg[49 * 701: 49 * 702]
    assert both(un) == (MALFORMED, MALFORMED)                              # ... and with a forgery in another slice too
    off_curve = b.pks.copy()
    off_curve[600, 48] ^= 1                                                # y of lane 600's key
    assert both(b.agg, pks=off_curve) == (MALFORMED, MALFORMED)


def test_fully_negated_left_side_is_rejected_across_slices(engine, tight):
    """every key the identity, every R negated: the left side is -[e_agg']G, equal in x only"""
    rng = np.random.default_rng(0x1DE0 + N3)
    es = make_scalars(rng, N3)
    comp, st = engine.compress_many(engine.pubkey_many(es))
    assert (st == 0).all()
    sigs, pks, inf = np.concatenate([comp, es], axis=1), np.zeros((N3, 96), np.uint8), np.ones(N3, np.uint8)
    msgs = rng.integers(0, 256, size=(N3, 80), dtype=np.uint8)
    honest = tight.aggregate_sliced(sigs, pks, msgs, pk_inf=inf)[1]
    assert tight.verify_aggregate_sliced(honest, pks, msgs, pk_inf=inf) == OK
    neg = sigs.copy()
    neg[:, 48] ^= 0x40
    agg = tight.aggregate_sliced(neg, pks, msgs, pk_inf=inf)[1]            # the R's negated, e_agg' = sum a_i' e_i
    assert (agg == engine.aggregate(neg, pks, msgs, pk_inf=inf)[1]).all()
    e_neg = int.from_bytes(agg[-32:].tobytes(), "little")
    for eng_verify in (tight.verify_aggregate_sliced, engine.verify_aggregate):
        assert eng_verify(agg, pks, msgs, pk_inf=inf) == INVALID
        assert eng_verify(with_e(agg, (Q - e_neg) % Q), pks, msgs, pk_inf=inf) == OK


def test_producer_refusals_name_the_lane_in_its_slice(engine, tight, batch):
    b = batch(N3)
    bad = b.sigs.copy()
    bad[1100, 49:81] = 0xFF                                                # e >= q in the third slice
    got, want = tight.aggregate_sliced(bad, b.pks, b.msgs), engine.aggregate(bad, b.pks, b.msgs)
    assert got[0] == want[0] == MALFORMED and got[3] == want[3] == 1
    assert (got[2] == want[2]).all() and got[2][1100] == MALFORMED and not np.delete(got[2], 1100).any()
    assert got[1].size == 49 * N3 + 32 and not got[1].any()
    bad = b.sigs.copy()
    bad[1536, 49] ^= 1                                                     # a wrong e in the fourth slice
    got, want = tight.aggregate_sliced(bad, b.pks, b.msgs, check=True), engine.aggregate(bad, b.pks, b.msgs, check=True)
    assert got[0] == want[0] == INVALID and got[3] == want[3] == 1 and not got[1].any()
    assert got[2][1536] == INVALID and not got[2][:1536].any()
    st, agg, status, nf = tight.aggregate_sliced(b.sigs, b.pks, b.msgs, check=True)
    assert st == OK and nf == 0 and not status.any() and (agg == b.agg).all()


# --------------------------------------------------------------------------------- 4. primitives and the combination
N4, B4 = 1100, 256
SHARDS4 = [(0, 512), (512, 768), (768, 1100), (1100, 1100)]             # whole blocks, a ragged last one, an empty fourth


def test_three_shards_by_hand_reproduce_the_single_call(engine, batch):
    import torch
    b = batch(N4)
    rs = np.ascontiguousarray(b.agg[:49 * N4])
    ds, dr, dp, dm, de = [torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0") for a in (b.sigs, rs, b.pks, b.msgs, b.agg[-32:])]
    n_tops = -(-N4 // B4)
    tops = torch.zeros((2, 32 * n_tops), dtype=torch.uint8, device="cuda:0")     # from signatures, from R's
    roots = torch.zeros((2, 32), dtype=torch.uint8, device="cuda:0")
    h = torch.zeros(32 * N4, dtype=torch.uint8, device="cuda:0")
    parts = torch.full((4, 32), 255, dtype=torch.uint8, device="cuda:0")
    recs = torch.full((4, 24), -1, dtype=torch.int64, device="cuda:0")
    out_rs = torch.zeros(49 * N4, dtype=torch.uint8, device="cuda:0")
    e_agg = torch.zeros(32, dtype=torch.uint8, device="cuda:0")
    status = torch.full((N4,), 255, dtype=torch.uint8, device="cuda:0")
    verdicts = torch.full((4,), 255, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    at = lambda t, off: t.data_ptr() + off
    for lo, hi in SHARDS4:
        engine.aggregate_shard_tops_device(at(ds, 81 * lo), 81, at(dp, 96 * lo), at(dm, 80 * lo), hi - lo, 80, B4,
                                           at(tops[0], 32 * (lo // B4)))
        engine.aggregate_shard_tops_device(at(dr, 49 * lo), 49, at(dp, 96 * lo), at(dm, 80 * lo), hi - lo, 80, B4,
                                           at(tops[1], 32 * (lo // B4)), d_h=at(h, 32 * lo))
    for k in range(2):
        engine.aggregate_root_device(tops[k].data_ptr(), n_tops, N4, roots[k].data_ptr(), block_lanes=B4)
    for j, (lo, hi) in enumerate(SHARDS4):
        engine.aggregate_shard_fold_device(at(ds, 81 * lo), at(dp, 96 * lo), hi - lo, lo, roots[0].data_ptr(),
                                           parts[j].data_ptr(), at(out_rs, 49 * lo), d_status=at(status, lo))
        engine.verify_aggregate_shard_device(at(dr, 49 * lo), at(dp, 96 * lo), at(dm, 80 * lo), hi - lo, 80, at(h, 32 * lo), lo,
                                             roots[1].data_ptr(), recs[j].data_ptr())
    engine.aggregate_combine_device(parts.data_ptr(), 4, e_agg.data_ptr())
    engine.verify_aggregate_combine_device(recs.data_ptr(), 4, de.data_ptr(), N4, at(verdicts, 0))
    engine.sync()
    assert (tops[0] == tops[1]).all() and (roots[0] == roots[1]).all()
    assert (out_rs.cpu().numpy() == rs).all() and (e_agg.cpu().numpy() == b.agg[-32:]).all()
    assert not status.cpu().numpy().any() and not parts[3].cpu().numpy().any()
    r = recs.cpu().numpy().astype(np.uint64)
    assert not r[:, 18:23].any() and (r[:, 23] == 0x5353415245430004).all()        # e = 0 on every lane; the magic
    assert not r[3, :18].any()                                                      # the empty shard: the identity
    # the combination fails closed: a record nobody wrote, a set malformed word, a point pushed off the curve
    zeroed, flagged, garbled = recs.clone(), recs.clone(), recs.clone()
    zeroed[1] = 0
    flagged[2, 22] = 1
    garbled[0, 0] ^= 2
    torch.cuda.synchronize()
    for k, rr in enumerate((zeroed, flagged, garbled)):
        engine.verify_aggregate_combine_device(rr.data_ptr(), 4, de.data_ptr(), N4, at(verdicts, 4 * (k + 1)))
    engine.sync()
    assert verdicts.cpu().tolist() == [OK, MALFORMED, MALFORMED, MALFORMED]


def test_primitives_refuse_bad_arguments(engine, batch):
    import torch
    import schnorr_sig_amd as ssa
    lib, ctx, b = ssa._lib, engine._ctx, batch(N4)
    ds, dp, dm = [torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0") for a in (b.sigs, b.pks, b.msgs)]
    buf = torch.zeros(16384, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    p, none = buf.data_ptr(), None
    tops = lambda lanes, stride, pks, B, out, ctx_=ctx: lib.ssa_aggregate_shard_tops_device(
        ctx_, lanes, stride, pks, dm.data_ptr(), none, 80, 80, 100, B, out, none)
    assert tops(ds.data_ptr(), 81, dp.data_ptr(), 4, p) == 0
    for B in (0, 3, 6, 100):
        assert tops(ds.data_ptr(), 81, dp.data_ptr(), B, p) == ssa.ERR_ARG
    assert tops(ds.data_ptr(), 80, dp.data_ptr(), 4, p) == ssa.ERR_ARG              # lanes are 81 or 49 bytes
    assert tops(none, 81, dp.data_ptr(), 4, p) == ssa.ERR_ARG
    assert tops(ds.data_ptr(), 81, none, 4, p) == ssa.ERR_ARG
    assert tops(ds.data_ptr(), 81, dp.data_ptr(), 4, none) == ssa.ERR_ARG
    assert tops(ds.data_ptr(), 81, dp.data_ptr(), 4, p + 4) == ssa.ERR_ARG          # tops are 64-bit words
    assert tops(ds.data_ptr(), 81, dp.data_ptr(), 4, p, ctx_=none) == ssa.ERR_ARG
    root = lambda t, n_tops, n, B, out: lib.ssa_aggregate_root_device(ctx, t, n_tops, n, B, out)
    assert root(p, 25, 100, 4, p + 8192) == 0
    assert root(p, 25, 100, 0, p + 8192) == 0                                       # (B not given: nothing to hold against)
    for n_tops, n, B in ((24, 100, 4), (26, 100, 4), (25, 101, 4), (25, 100, 3), (0, 100, 0), (101, 100, 0), (1, 0, 0)):
        assert root(p, n_tops, n, B, p + 8192) == ssa.ERR_ARG, (n_tops, n, B)
    assert root(none, 25, 100, 4, p + 8192) == ssa.ERR_ARG and root(p, 25, 100, 4, none) == ssa.ERR_ARG
    fold = lambda sigs, root_, e, rs: lib.ssa_aggregate_shard_fold_device(ctx, sigs, dp.data_ptr(), none, 100, 0, root_, e, rs,
                                                                          none, none)
    assert fold(ds.data_ptr(), p + 8192, p, p + 64) == 0
    assert fold(none, p + 8192, p, p + 64) == ssa.ERR_ARG and fold(ds.data_ptr(), none, p, p + 64) == ssa.ERR_ARG
    assert fold(ds.data_ptr(), p + 8192, none, p + 64) == ssa.ERR_ARG and fold(ds.data_ptr(), p + 8192, p, none) == ssa.ERR_ARG
    shard = lambda rs, pks, root_, rec: lib.ssa_verify_aggregate_shard_device(ctx, rs, pks, none, dm.data_ptr(), none, 80, 80,
                                                                             none, 100, 0, root_, rec)
    assert shard(none, dp.data_ptr(), p + 8192, p) == ssa.ERR_ARG and shard(ds.data_ptr(), none, p + 8192, p) == ssa.ERR_ARG
    assert shard(ds.data_ptr(), dp.data_ptr(), none, p) == ssa.ERR_ARG and shard(ds.data_ptr(), dp.data_ptr(), p + 8192, none) == ssa.ERR_ARG
    assert lib.ssa_aggregate_combine_device(ctx, none, 2, p) == ssa.ERR_ARG
    assert lib.ssa_aggregate_combine_device(ctx, p, 0, p + 64) == ssa.ERR_ARG
    assert lib.ssa_aggregate_combine_device(ctx, p, 2, none) == ssa.ERR_ARG
    assert lib.ssa_verify_aggregate_combine_device(ctx, none, 2, p, 100, p + 64) == ssa.ERR_ARG
    assert lib.ssa_verify_aggregate_combine_device(ctx, p, 0, p + 1024, 100, p + 64) == ssa.ERR_ARG
    assert lib.ssa_verify_aggregate_combine_device(ctx, p, 2, none, 100, p + 64) == ssa.ERR_ARG
    assert lib.ssa_verify_aggregate_combine_device(ctx, p, 2, p + 1024, 100, none) == ssa.ERR_ARG
    engine.sync()
    st, _, _, _ = engine.aggregate_sliced(b.sigs, b.pks, b.msgs)                   # (the context is as good as before)
    assert st == OK


# ------------------------------------------------------------------------------------- 5. several contexts, one process
@pytest.mark.parametrize("B", [512, 256])
def test_multi_engine_equals_the_single_call(engine, batch, B):
    """three contexts on device 0; n = 3 * 512 + 77 is four blocks of 512 (2 + 1 + 1) or seven of 256 (3 + 2 + 2); n = 600
    leaves a context without lanes"""
    multi = engine_under(devices=[0, 0, 0], SSA_MSM_SLICE=512, SSA_AGG_BLOCK=B)
    try:
        for n in (3 * 512 + 77, 600):
            b = batch(n, ragged=(B == 256))
            st, agg, status, nf = multi.aggregate(b.sigs, b.pks, b.msgs, offsets=b.off)
            assert st == OK and nf == 0 and not status.any() and (agg == b.agg).all(), n
            assert multi.verify_aggregate(b.agg, b.pks, b.msgs, offsets=b.off) == OK, n
            st, agg, status, nf = multi.aggregate(b.sigs, b.pks, b.msgs, offsets=b.off, check=True)
            assert st == OK and nf == 0 and (agg == b.agg).all(), n
        forged = b.sigs.copy()                                            # (n = 600: lane 599 is on the last context with lanes)
        forged[599, 49] ^= 1
        st, agg_f, _, _ = multi.aggregate(forged, b.pks, b.msgs, offsets=b.off)
        assert st == OK and (agg_f == engine.aggregate(forged, b.pks, b.msgs, offsets=b.off)[1]).all()
        assert multi.verify_aggregate(agg_f, b.pks, b.msgs, offsets=b.off) == INVALID
        st, agg_f, status, nf = multi.aggregate(forged, b.pks, b.msgs, offsets=b.off, check=True)
        assert st == INVALID and nf == 1 and status[599] == INVALID and not agg_f.any()
        b = batch(3 * 512 + 77, ragged=(B == 256))
        forged = b.sigs.copy()
        forged[1600, 49] ^= 1                                             # on the last device
        agg_f = engine.aggregate(forged, b.pks, b.msgs, offsets=b.off)[1]
        assert multi.verify_aggregate(agg_f, b.pks, b.msgs, offsets=b.off) == INVALID
        bad = b.sigs.copy()
        bad[1600, 49:81] = 0xFF
        st, agg_b, status, nf = multi.aggregate(bad, b.pks, b.msgs, offsets=b.off)
        assert st == MALFORMED and nf == 1 and status[1600] == MALFORMED and not agg_b.any()
    finally:
        multi.close()


def test_objects_mirror(engine, tight):
    import schnorr_sig_amd as ssa
    gen = np.random.default_rng(0x0B1EC9)
    rng = lambda k: gen.bytes(k)
    pairs = [ssa.KeyPair.new(rng, engine) for _ in range(3)]
    msgs = [b"one", b"", b"three" * 20]
    sigs = [kp.sign(m, rng, engine) for kp, m in zip(pairs, msgs)]
    pks = [kp.public_key for kp in pairs]
    want = ssa.AggregateSignature.aggregate(sigs, pks, msgs, engine=engine)
    multi = engine_under(devices=[0, 0], SSA_AGG_BLOCK=2)
    try:
        for eng in (tight, multi):
            agg = ssa.AggregateSignature.aggregate(sigs, pks, msgs, engine=eng, sliced=True)
            assert agg == want and agg.verify(pks, msgs, engine=eng, sliced=True) is None
            with pytest.raises(ssa.SignatureError):
                agg.verify(pks, [b"one", b"x", msgs[2]], engine=eng, sliced=True)
        assert ssa.AggregateSignature.aggregate(sigs, pks, msgs, engine=multi) == want
        assert want.verify(pks, msgs, engine=multi) is None
    finally:
        multi.close()


# ------------------------------------------------------------------------------------------------ 6. the process form
NP, BP = 1100, 256


def _process_batch(engine):
    rng = np.random.default_rng(0x9A0C)
    msgs = rng.integers(0, 256, size=(NP, 80), dtype=np.uint8)
    pks, sigs = engine.keygen_sign_many(make_scalars(rng, NP), make_scalars(rng, NP), msgs)
    return sigs, pks, msgs


def _rank(rank, world, port, q):
    """one rank: its own process, its own context on GPU 0, a gloo group on loopback"""
    try:
        sys.path.insert(0, ROOT)
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        import torch
        import torch.distributed as dist
        import schnorr_sig_amd as ssa
        from schnorr_sig_amd.sharding import aggregate_block_range, aggregate_sharded, verify_aggregate_sharded
        dist.init_process_group("gloo", rank=rank, world_size=world)
        eng = ssa.Engine(0)
        sigs, pks, msgs = _process_batch(eng)
        lo, hi = aggregate_block_range(NP, BP, rank, world)
        ds, dp, dm = [torch.from_numpy(np.ascontiguousarray(a[lo:hi])).to("cuda:0") for a in (sigs, pks, msgs)]
        st, e_agg, rs, status = aggregate_sharded(eng, ds, dp, dm, NP, BP, rank, world, dist)
        rs49 = rs.reshape(-1, 49)
        v_ok = verify_aggregate_sharded(eng, rs49, dp, dm, e_agg, NP, BP, rank, world, dist)
        forged = dm.clone()
        if rank == world - 1:
            forged[-1, 3] ^= 1                                            # one message bit on the last rank
        v_bad = verify_aggregate_sharded(eng, rs49, dp, forged, e_agg, NP, BP, rank, world, dist)
        q.put((rank, lo, hi, st, e_agg.cpu().numpy().tobytes(), rs.cpu().numpy().tobytes(), int(status.sum().item()),
               v_ok, v_bad))
        dist.barrier()
        dist.destroy_process_group()
        eng.close()
    except BaseException as exc:      # noqa: BLE001  (the parent must hear of it instead of waiting)
        q.put((rank, repr(exc)))
        raise


def test_two_processes_equal_the_single_call(engine):
    import torch.multiprocessing as mp
    world = 2
    sigs, pks, msgs = _process_batch(engine)
    st, want, _, _ = engine.aggregate(sigs, pks, msgs)
    assert st == OK
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 33500 + (os.getpid() % 2000)
    procs = [ctx.Process(target=_rank, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    try:
        res = sorted(q.get(timeout=240) for _ in range(world))
        assert all(len(r) == 9 for r in res), res
        for p in procs:
            p.join(timeout=60)
            assert p.exitcode == 0
    finally:
        for p in procs:
            if p.is_alive():
                p.kill()
    assert [(r[1], r[2]) for r in res] == [(0, 768), (768, 1100)]
    assert all(r[3] == OK and r[6] == 0 for r in res)
    assert all(r[4] == want[-32:].tobytes() for r in res)                  # every rank holds e_agg
    assert b"".join(r[5] for r in res) == want[:-32].tobytes()
    assert [(r[7], r[8]) for r in res] == [(OK, INVALID)] * world
