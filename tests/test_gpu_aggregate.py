"""Half-aggregation on the GPU (ssa_aggregate_many / ssa_verify_aggregate) against the model of
tests/aggregate_model.py over the C oracle: the coefficients byte for byte, the aggregate's bytes, honest aggregates at
sizes on a wave edge, a workgroup edge, both sides of the small-batch bound of the MSM and through every pass of the tree,
rejections with the verdict they must get by construction, and independence of whatever ran before on the context."""
import numpy as np
import pytest

import aggregate_model as am

pytestmark = pytest.mark.gpu

Q = am.Q
SIZES = [1, 2, 3, 64, 65, 257, 1025, 3072, 3073, 65537]
REJECT_SIZES = [3, 1025, 3073]
OK, INVALID, MALFORMED = 0, 2, 3


def make_scalars(rng, n):
    s = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    s[:, 31] &= 0x3F
    s[:, 0] |= 1
    return s


def dev(*arrays):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0") for a in arrays]


class Case:
    """n honest signatures over 80-byte messages, the model's coefficients and e_agg (computed once per size)"""

    def __init__(self, engine, oracle, n):
        rng = np.random.default_rng(0xA6600 + n)
        self.n = n
        self.msgs = rng.integers(0, 256, size=(n, 80), dtype=np.uint8)
        self.pks, self.sigs = engine.keygen_sign_many(make_scalars(rng, n), make_scalars(rng, n), self.msgs)
        self.rs = np.ascontiguousarray(self.sigs[:, :49])
        self.a = am.coefficients(am.oracle_backend(oracle), self.rs, self.pks, self.msgs)
        self.e_agg = am.fold(self.a, self.sigs)
        self.agg = np.concatenate([self.rs.reshape(-1), np.frombuffer(self.e_agg.to_bytes(32, "little"), np.uint8)])


_CASES = {}


@pytest.fixture
def case(engine, oracle):
    def get(n):
        if n not in _CASES:
            _CASES[n] = Case(engine, oracle, n)
        return _CASES[n]
    return get


def with_e(agg, e):
    out = agg.copy()
    out[-32:] = np.frombuffer(int(e).to_bytes(32, "little"), np.uint8)
    return out


def model_agg(oracle, sigs, pks, msgs):
    return np.frombuffer(am.aggregate(am.oracle_backend(oracle), sigs, pks, msgs), np.uint8).copy()


@pytest.mark.parametrize("n", SIZES)
def test_coefficients_are_the_models_byte_for_byte(engine, case, n):
    c = case(n)
    got = engine.aggregate_coeffs(c.rs, c.pks, c.msgs)
    want = am.coeff_bytes(c.a)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, (bad[:8], got[bad[:2]], want[bad[:2]])
    assert (got[:, 15] < 0x40).all()                                      # 126 bits


@pytest.mark.parametrize("n", [1, 2, 512, 513, 262145])
def test_null_plan_and_uploaded_plan_give_the_same_coefficients(engine, n):
    """One, two and three passes of the tree (262 145 = 512^2 + 1 is the smallest n with three): the single call forms
    its descriptors in the kernel, the many-call of ONE aggregate reads them from the uploaded plan.  Same kernels,
    same bytes; the test above ties the first to the model."""
    rng = np.random.default_rng(0xA6600 + n)
    msgs = rng.integers(0, 256, size=(n, 80), dtype=np.uint8)
    pks, sigs = engine.keygen_sign_many(make_scalars(rng, n), make_scalars(rng, n), msgs)
    rs = np.ascontiguousarray(sigs[:, :49])
    agg = np.concatenate([rs.reshape(-1), np.zeros(32, np.uint8)])       # (the transcript does not read e_agg)
    null_plan = engine.aggregate_coeffs(rs, pks, msgs)
    uploaded = engine.aggregates_coeffs([agg], pks, msgs)
    assert null_plan.shape == uploaded.shape == (n, 16)
    bad = np.nonzero((null_plan != uploaded).any(axis=1))[0]
    assert bad.size == 0, (bad[:8], null_plan[bad[:2]], uploaded[bad[:2]])
    assert null_plan.any(axis=1).all()                                     # no coefficient is 0


@pytest.mark.parametrize("n", SIZES)
def test_aggregate_bytes(engine, case, n):
    c = case(n)
    st, agg, status, nf = engine.aggregate(c.sigs, c.pks, c.msgs)
    assert st == OK and nf == 0 and (status == 0).all()
    assert agg.size == 49 * n + 32 and (agg[:49 * n].reshape(n, 49) == c.sigs[:, :49]).all()
    assert int.from_bytes(agg[49 * n:].tobytes(), "little") == c.e_agg
    assert (agg == c.agg).all()


@pytest.mark.parametrize("n", SIZES)
def test_honest_aggregates_verify_and_the_coefficient_is_shape_independent(engine, case, n):
    import torch
    c = case(n)
    assert engine.verify_aggregate(c.agg, c.pks, c.msgs) == OK
    # the original signatures under the MSM verdict with coeffs = a_i: 16 bytes, and zero-extended to 32
    a16 = am.coeff_bytes(c.a)
    a32 = np.concatenate([a16, np.zeros((n, 16), np.uint8)], axis=1)
    assert engine.verify_batch_msm(c.sigs, c.pks, c.msgs, coeffs=a32) == OK
    ds, dp, dm, d16, d32 = dev(c.sigs, c.pks, c.msgs, a16, a32)
    verdict = torch.full((2,), 255, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    engine.verify_batch_msm_device(ds.data_ptr(), dp.data_ptr(), dm.data_ptr(), n, 80, d16.data_ptr(), 16, verdict.data_ptr())
    engine.verify_batch_msm_device(ds.data_ptr(), dp.data_ptr(), dm.data_ptr(), n, 80, d32.data_ptr(), 32,
                                   verdict.data_ptr() + 4)
    engine.sync()
    assert verdict.cpu().tolist() == [OK, OK]


def identity_lanes(engine, rng, n):
    """n signatures that verify under the IDENTITY key with any message: R = [e]G, since [h]O adds nothing"""
    es = make_scalars(rng, n)
    comp, st = engine.compress_many(engine.pubkey_many(es))
    assert (st == 0).all()
    return np.concatenate([comp, es], axis=1), np.zeros((n, 96), np.uint8), np.ones(n, np.uint8)


@pytest.mark.parametrize("n", REJECT_SIZES)
def test_rejections_get_the_verdict_they_must(engine, oracle, case, n):
    import pymodel as pm
    c = case(n)
    rng = np.random.default_rng(0xBAD00 + n)
    k = int(rng.integers(0, n))
    verdict = lambda agg, pks=c.pks, msgs=c.msgs, inf=None: engine.verify_aggregate(agg, pks, msgs, pk_inf=inf)
    assert verdict(c.agg) == OK

    e_bit = c.e_agg ^ 1 if c.e_agg ^ 1 < Q else c.e_agg ^ 2                 # one bit of e_agg, still below q
    assert verdict(with_e(c.agg, e_bit)) == INVALID
    m = c.msgs.copy()
    m[k, 17] ^= 0x04
    assert verdict(c.agg, msgs=m) == INVALID                               # one message bit
    sw = c.agg.copy()
    sw[:49], sw[49:98] = c.agg[49:98], c.agg[:49]
    assert verdict(sw) == INVALID                                          # two R's swapped
    p = c.pks.copy()
    p[k] = c.pks[(k + 1) % n]
    assert verdict(c.agg, pks=p) == INVALID                                # one key replaced by its neighbour
    fl = c.agg.copy()
    fl[49 * k + 48] ^= 0x40
    assert verdict(fl) == INVALID                                          # one R's sort bit
    bad = c.sigs.copy()
    bad[k, 49] ^= 1
    st, agg_bad, status, nf = engine.aggregate(bad, c.pks, c.msgs)         # (unchecked: nothing is malformed)
    assert st == OK and nf == 0
    assert (agg_bad == model_agg(oracle, bad, c.pks, c.msgs)).all()
    assert verdict(agg_bad) == INVALID                                     # one input signature had a wrong e
    # the global sign: -[e_agg]G has the x of [e_agg]G, an x-only comparison would accept this
    assert verdict(with_e(c.agg, Q - c.e_agg)) == INVALID

    assert verdict(with_e(c.agg, Q)) == MALFORMED                          # e_agg = q
    nc = c.agg.copy()
    nc[49 * k: 49 * k + 8] = 0xFF
    assert verdict(nc) == MALFORMED                                        # a limb >= p in an R
    for t in range(1, 64):                                                 # an x with no point on the curve
        x = c.agg[49 * k: 49 * k + 49].copy()
        x[8] ^= t
        if pm.pt_decompress(x.tobytes())[0] == "invalid":
            break
    un = c.agg.copy()
    un[49 * k: 49 * k + 49] = x
    assert verdict(un) == MALFORMED
    fb = c.agg.copy()
    fb[49 * k + 48] |= 0x01
    assert verdict(fb) == MALFORMED                                        # an undecodable flag byte


@pytest.mark.parametrize("n", REJECT_SIZES)
def test_fully_negated_left_side_is_rejected(engine, oracle, n):
    """Every key the identity: the left side is sum a_i R_i alone.  With every R negated and e_agg' = sum a_i' e_i over the
    new transcript's coefficients, left = -[e_agg']G: the x coordinates agree, the points do not.  q - e_agg' is the honest
    aggregate of the signatures (-R_i, -e_i) and verifies."""
    rng = np.random.default_rng(0x1DE0 + n)
    sigs, pks, inf = identity_lanes(engine, rng, n)
    msgs = rng.integers(0, 256, size=(n, 80), dtype=np.uint8)
    be = am.oracle_backend(oracle)
    assert engine.verify_aggregate(model_agg(oracle, sigs, pks, msgs), pks, msgs, pk_inf=inf) == OK
    neg = sigs.copy()
    neg[:, 48] ^= 0x40
    e_neg = am.fold(am.coefficients(be, neg[:, :49], pks, msgs), sigs)
    agg = np.concatenate([neg[:, :49].reshape(-1), np.zeros(32, np.uint8)])
    assert engine.verify_aggregate(with_e(agg, e_neg), pks, msgs, pk_inf=inf) == INVALID
    assert engine.verify_aggregate(with_e(agg, (Q - e_neg) % Q), pks, msgs, pk_inf=inf) == OK


@pytest.mark.parametrize("n", [1025, 3073])
def test_checked_aggregation_names_the_bad_lane_and_gives_no_aggregate(engine, case, n):
    c = case(n)
    st, agg, status, nf = engine.aggregate(c.sigs, c.pks, c.msgs, check=True)
    assert st == OK and nf == 0 and (status == 0).all() and (agg == c.agg).all()     # byte-identical to the unchecked call
    bad = c.sigs.copy()
    bad[n // 2, 49] ^= 1
    st, agg, status, nf = engine.aggregate(bad, c.pks, c.msgs, check=True)
    want, wnf = engine.verify_batch_screened(bad, c.pks, c.msgs)
    assert st == INVALID and nf == wnf == 1 and (status == want).all() and status[n // 2] == INVALID
    assert agg.size == 49 * n + 32 and not agg.any()
    # unchecked: only malformed inputs are refused
    bad[n // 2, 49:81] = 0xFF
    st, agg, status, nf = engine.aggregate(bad, c.pks, c.msgs)
    assert st == MALFORMED and nf == 1 and status[n // 2] == MALFORMED and (np.delete(status, n // 2) == 0).all()
    assert not agg.any()
    st, agg, status, nf = engine.aggregate(bad, c.pks, c.msgs, check=True)
    assert st == MALFORMED and nf == 1 and status[n // 2] == MALFORMED and not agg.any()


@pytest.mark.parametrize("n", [5, 3073])
def test_identity_key_lane(engine, oracle, case, n):
    c = case(n)
    rng = np.random.default_rng(0x1D00 + n)
    sigs, pks, msgs = c.sigs.copy(), c.pks.copy(), c.msgs
    inf = np.zeros(n, np.uint8)
    k = n - 2
    sigs[k:k + 1], pks[k:k + 1], inf[k:k + 1] = identity_lanes(engine, rng, 1)
    st, agg, status, nf = engine.aggregate(sigs, pks, msgs, pk_inf=inf, check=True)
    assert st == OK and nf == 0
    assert (agg == model_agg(oracle, sigs, pks, msgs)).all()
    assert engine.verify_aggregate(agg, pks, msgs, pk_inf=inf) == OK
    assert engine.verify_aggregate(agg, pks, msgs) == MALFORMED            # (0, 0) is no point of the curve


def test_empty_aggregate(engine):
    none = np.zeros((0, 96), np.uint8)
    st, agg, status, nf = engine.aggregate(np.zeros((0, 81), np.uint8), none, None)
    assert st == OK and agg.size == 32 and not agg.any() and nf == 0
    assert engine.verify_aggregate(agg, none, None) == OK
    assert engine.verify_aggregate(with_e(agg, 1), none, None) == INVALID
    assert engine.verify_aggregate(with_e(agg, Q), none, None) == MALFORMED
    assert engine.aggregate_coeffs(np.zeros((0, 49), np.uint8), none, None).shape == (0, 16)


def aggregate_on_device(eng, c, check=False):
    import torch
    ds, dp, dm = dev(c.sigs, c.pks, c.msgs)
    d_agg = torch.full((49 * c.n + 32,), 255, dtype=torch.uint8, device="cuda:0")
    d_st = torch.full((c.n,), 255, dtype=torch.uint8, device="cuda:0")
    d_nf = torch.full((1,), -1, dtype=torch.int64, device="cuda:0")
    d_v = torch.full((1,), 255, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    st = eng.aggregate_device(ds.data_ptr(), dp.data_ptr(), dm.data_ptr(), c.n, 80, d_agg.data_ptr(), d_st.data_ptr(),
                              d_nf.data_ptr(), check=check)
    eng.verify_aggregate_device(d_agg.data_ptr(), dp.data_ptr(), dm.data_ptr(), c.n, 80, d_v.data_ptr())
    eng.sync()
    return st, d_agg.cpu().numpy(), d_st.cpu().numpy(), int(d_nf.item()), int(d_v.item())


@pytest.mark.parametrize("n", [257, 3073])
def test_device_forms_and_order_independence(engine, case, n):
    """device forms give the host forms' bytes; on ONE context, after the workspaces were poisoned and after an unrelated
    screened call, aggregate and verify_aggregate give what a fresh context gives"""
    import schnorr_sig_amd as ssa
    c = case(n)
    for check in (False, True):
        st, agg, status, nf, v = aggregate_on_device(engine, c, check)
        assert (st, nf, v) == (OK, 0, OK) and (agg == c.agg).all() and (status == 0).all()
    fresh = ssa.Engine(0)
    try:
        want = fresh.aggregate(c.sigs, c.pks, c.msgs, check=True)
        want_v = fresh.verify_aggregate(c.agg, c.pks, c.msgs)
        want_c = fresh.aggregate_coeffs(c.rs, c.pks, c.msgs)
    finally:
        fresh.close()
    other = case(1025 if n != 1025 else 257)
    for prelude in (lambda: engine.debug_poison_workspaces(0xA5),
                    lambda: engine.verify_batch_screened(other.sigs, other.pks, other.msgs),
                    lambda: engine.debug_poison_workspaces(0xFF)):
        prelude()
        got = engine.aggregate(c.sigs, c.pks, c.msgs, check=True)
        assert got[0] == want[0] == OK and (got[1] == want[1]).all() and (got[2] == want[2]).all() and got[3] == want[3]
        prelude()
        assert engine.verify_aggregate(c.agg, c.pks, c.msgs) == want_v == OK
        prelude()
        assert (engine.aggregate_coeffs(c.rs, c.pks, c.msgs) == want_c).all()


def test_aggregate_calls_leave_existing_calls_alone(engine, case):
    c = case(3073)
    rng = np.random.default_rng(0x51DE)
    sigs = c.sigs.copy()
    sigs[[7, 1500, 3072], 49] ^= 1
    co = make_scalars(rng, c.n)
    before = engine.verify_batch_screened(sigs, c.pks, c.msgs, coeffs=co)
    before_v = (engine.verify_batch_msm(c.sigs, c.pks, c.msgs, coeffs=co), engine.verify_batch_msm(sigs, c.pks, c.msgs, coeffs=co))
    assert before_v == (OK, INVALID) and before[1] == 3
    engine.aggregate(c.sigs, c.pks, c.msgs, check=True)
    engine.aggregate(sigs, c.pks, c.msgs, check=True)
    assert engine.verify_aggregate(c.agg, c.pks, c.msgs) == OK
    engine.aggregate_coeffs(c.rs, c.pks, c.msgs)
    after = engine.verify_batch_screened(sigs, c.pks, c.msgs, coeffs=co)
    assert (after[0] == before[0]).all() and after[1] == before[1]
    assert (engine.verify_batch_msm(c.sigs, c.pks, c.msgs, coeffs=co), engine.verify_batch_msm(sigs, c.pks, c.msgs, coeffs=co)) == before_v


def test_objects_mirror(engine):
    import schnorr_sig_amd as ssa
    gen = np.random.default_rng(0x0B1EC7)
    rng = lambda k: gen.bytes(k)
    pairs = [ssa.KeyPair.new(rng, engine) for _ in range(3)]
    msgs = [b"one", b"", b"three" * 20]
    sigs = [kp.sign(m, rng, engine) for kp, m in zip(pairs, msgs)]
    pks = [kp.public_key for kp in pairs]
    agg = ssa.AggregateSignature.aggregate(sigs, pks, msgs, engine=engine)
    assert len(agg) == 3 and len(agg.to_bytes()) == 49 * 3 + 32
    assert ssa.AggregateSignature.from_bytes(agg.to_bytes()).verify(pks, msgs, engine=engine) is None
    with pytest.raises(ssa.SignatureError):
        agg.verify(pks, [b"one", b"x", msgs[2]], engine=engine)
    with pytest.raises(ssa.SignatureError):
        ssa.AggregateSignature.aggregate([sigs[1], sigs[0], sigs[2]], pks, msgs, engine=engine)
    assert ssa.AggregateSignature.aggregate([], [], [], engine=engine).verify([], [], engine=engine) is None
