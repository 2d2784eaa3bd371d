"""The exceptional additions of the MSM's bucket path, each made to run at a known place and checked by the exact shard
record ("Exceptional additions"; the cases and the proof that they reach their branches:
tests/msm_edge_model.py, tests/test_msm_edge_model_host.py).  Every comparison is of exact points, scalars or bytes; the
reference is tests/msm_records.py::cpu_partial over the oracle, computed once per case on the active lanes."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import msm_edge_model as em      # noqa: E402
import msm_records as mr         # noqa: E402

pytestmark = pytest.mark.gpu

Q, P = mr.Q, mr.P
OK, INVALID = 0, 2


def engine_under(**env):
    """an Engine created under these environment knobs, which are restored at once: a context reads them when it is
    made.  gtab_bits = 16: the record path never reads the comb."""
    import schnorr_sig_amd as ssa
    old = {k: os.environ.get(k) for k in env}
    os.environ.update({k: str(v) for k, v in env.items()})
    try:
        return ssa.Engine(0, gtab_bits=16)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def engines():
    """bucket: every n through the bucket path; tg*: the same under other tree groups; small: every n through the
    per-lane path"""
    made = {}
    try:
        made["bucket"] = engine_under(SSA_MSM_SMALL_MAX=0)
        for tg in (2, 3, 64):
            made["tg%d" % tg] = engine_under(SSA_MSM_SMALL_MAX=0, SSA_MSM_TREE_GROUP=tg)
        made["small"] = engine_under(SSA_MSM_SMALL_MAX=2 ** 40)
        yield made
    finally:
        for eng in made.values():
            eng.close()


@pytest.fixture(scope="module")
def builder(oracle):
    return em.Builder(oracle)


_REF = {}


def reference(builder, oracle, case):
    """(the built call, cpu_partial's point, lin) of a case, computed once"""
    if case.name not in _REF:
        b = builder.build_case(case)
        pt, lin, mal = mr.cpu_partial(oracle, *em.active(b))
        assert not mal and lin == b.lin
        _REF[case.name] = (b, pt, lin)
    return _REF[case.name]


def record_of(eng, b):
    return eng.verify_batch_msm_partial(b.sigs, b.pks, b.msgs, coeffs=b.coeffs, pk_inf=b.pk_inf)


def check_record(oracle, rec, pt, lin):
    """not malformed, the magic word, the exact point in its canonical form, the exact scalar"""
    assert int(rec[22]) == 0 and int(rec[23]) == mr.MAGIC
    assert mr.record_point(oracle, rec) == pt
    assert mr.record_lin(rec) == lin
    if pt is None:
        assert not rec[:18].any()
    else:
        assert [int(v) for v in rec[12:18]] == [1, 0, 0, 0, 0, 0]
        assert tuple(int(v) for v in rec[:6]) == pt[0] and tuple(int(v) for v in rec[6:12]) == pt[1]


@pytest.mark.parametrize("case", em.CASES, ids=lambda k: k.name)
def test_case_record_is_exact(engines, builder, oracle, case):
    """one case of the table (the stage is the first word of its name): the bucket path's record is cpu_partial's point
    and lin in canonical form; the same bytes under every tree group and, for c = 8 lanes, under 16-bit windows; the
    same point and lin on the per-lane path"""
    b, pt, lin = reference(builder, oracle, case)
    rec = record_of(engines["bucket"], b)
    check_record(oracle, rec, pt, lin)
    for tg in (2, 3, 64):        # SSA_MSM_TREE_GROUP has no effect on results: the same bytes
        assert record_of(engines["tg%d" % tg], b).tobytes() == rec.tobytes(), tg
    check_record(oracle, record_of(engines["small"], b), pt, lin)
    if case.c == 8:              # the same lanes padded to 4096 are the same MSM under 16-bit windows
        b16 = builder.build_case(case, em.PAD_C16)
        assert record_of(engines["bucket"], b16).tobytes() == rec.tobytes()


def test_scalar_edges_of_lin(engines, builder, oracle):
    """e in {0, 1, q - 1} times coefficients {1, q - 1, q, q + 1, 2^256 - 1} on lanes 0, 255, 256 and 599 of 600: lin by
    Python integers (sc_reduce256, sc_mul_mod, the block sums, wave_sum_mod_q), on both paths"""
    for combos in em.scalar_instances():
        b = builder.build_scalars(combos)
        want = sum((co % Q) * e for co, e in combos) % Q
        pt, lin, mal = mr.cpu_partial(oracle, *em.active(b))
        assert not mal and lin == want
        for name in ("bucket", "small"):
            check_record(oracle, record_of(engines[name], b), pt, lin)


def test_device_form_gives_the_same_bytes(engines, builder, oracle):
    """one case per stage through ssa_verify_batch_msm_partial_device"""
    import torch
    dev = torch.device("cuda", 0)
    eng = engines["bucket"]
    for name in ("bucket_p_sentinel_p_idkey_neg_c8", "chunk_k0_40_order5_c8", "tree_copy_then_same_c8",
                 "tree_level3_opposite_c16", "horner_opposite_lower_filled_c16"):
        case = next(k for k in em.CASES if k.name == name)
        b, pt, lin = reference(builder, oracle, case)
        host = record_of(eng, b)
        check_record(oracle, host, pt, lin)
        ds, dp, dm, dc, di = (torch.from_numpy(a).to(dev) for a in (b.sigs, b.pks, b.msgs, b.coeffs, b.pk_inf))
        rec = torch.zeros(24, dtype=torch.int64, device=dev)
        eng.verify_batch_msm_partial_device(ds.data_ptr(), dp.data_ptr(), dm.data_ptr(), b.n, em.MSG_LEN, dc.data_ptr(), 32,
                                            rec.data_ptr(), d_pk_inf=di.data_ptr())
        eng.sync()
        assert rec.cpu().numpy().astype(np.uint64).tobytes() == host.tobytes(), name


def negated(rec):
    """the record of the opposite shard: y and lin negated"""
    out = rec.copy()
    if out[12:18].any():
        out[6:12] = [(P - int(v)) % P for v in rec[6:12]]
    lin = (Q - mr.record_lin(rec)) % Q
    out[18:22] = [(lin >> (64 * k)) & (2 ** 64 - 1) for k in range(4)]
    return out


def test_combination_meets_the_same_branches(engine, engines, builder, oracle):
    """ssa_msm_combine / _device on records that are equal, opposite and the identity, against cpu_combine.  The records
    are those of lanes with e_i = m_i for R_i = [m_i]G: each is its own [lin]G, so every honest combination says Ok and
    a wrong sum would say InvalidSignature."""
    import torch

    def honest_like(ms, coeffs):
        b = builder.build([("R", ("G", m), ("raw", s, m)) for m, s in zip(ms, coeffs)], 8)
        pt, lin, mal = mr.cpu_partial(oracle, *em.active(b))
        rec = record_of(engines["bucket"], b)
        check_record(oracle, rec, pt, lin)
        assert pt == builder.element_point((lin, 0))
        return rec

    r = honest_like([5, 9], [0x1234567, 77])
    s = honest_like([11], [Q - 3])
    ident = record_of(engines["bucket"], builder.build([], 8))
    assert not ident[:22].any()
    nothing_below = reference(builder, oracle, next(k for k in em.CASES if k.name == "horner_opposite_nothing_below_c8"))
    zero_point = record_of(engines["bucket"], nothing_below[0])       # the identity with a nonzero lin: not [lin]G
    assert not zero_point[:18].any() and zero_point[18:22].any()
    dev = torch.device("cuda", 0)
    for recs, want in (([r, r], OK), ([r, negated(r)], OK), ([ident, r], OK), ([r, negated(r), s], OK),
                       ([r, s, r, negated(s), negated(r)], OK), ([ident, ident], OK), ([r, s], OK),
                       ([r, negated(s)], OK), ([r, zero_point], INVALID), ([zero_point], INVALID),
                       ([r, negated(r), zero_point], INVALID)):
        recs = np.stack(recs)
        assert mr.cpu_combine(oracle, recs) == want
        assert engine.msm_combine(recs) == want
        d = torch.from_numpy(recs.view(np.int64)).to(dev)
        verdict = torch.full((1,), 255, dtype=torch.int32, device=dev)
        engine.msm_combine_device(d.data_ptr(), len(recs), verdict.data_ptr())
        engine.sync()
        assert int(verdict.item()) == want


def honest(engine, rng, n, one_key=False):
    sks = rng.integers(0, 256, size=(1 if one_key else n, 32), dtype=np.uint8)
    sks[:, 31] &= 0x3F
    if one_key:
        sks = np.repeat(sks, n, axis=0)
    nonces = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    nonces[:, 31] &= 0x3F
    msgs = rng.integers(0, 256, size=(n, em.MSG_LEN), dtype=np.uint8)
    pks, sigs = engine.keygen_sign_many(sks, nonces, msgs)
    return sigs, pks, msgs


def lin_of(sigs, coeffs):
    return sum((int.from_bytes(bytes(c), "little") % Q) * int.from_bytes(bytes(s[49:]), "little")
               for s, c in zip(sigs, coeffs)) % Q


def generator_multiple(oracle, k):
    return oracle.point_mul(k, mr._aff(oracle.keygen((1).to_bytes(32, "little"))[0]))


@pytest.mark.parametrize("n", [8200, 16400])
def test_skewed_batch_one_bucket_of_all_the_rs(engine, engines, oracle, n):
    """one key and one coefficient for every lane of an honest batch: in every window all n R's share one digit, that is
    one bucket of n points, above the size clamp of 1023 of msm_k_sizes.  (The -P's do not: their digits are those of
    s h_i, and h_i differs from lane to lane.)  A window's items are R_0 .. R_n-1, then -P_0 .. -P_n-1, in tiles of 16384:
    at n = 8200 a window has two tiles, but all R's lie in the first (the second holds the last 16 -P's); at n = 16400 the
    R's 16384 .. 16399 lie in the second tile of three, so the one bucket is counted and scattered by two tiles (one run
    of a (window, group) row split in msm_k_rowscan).  The batch is honest: the record's point is [lin]G."""
    assert 2 * n > 16384 and (n > 16384) == (n == 16400)
    rng = np.random.default_rng(n)
    sigs, pks, msgs = honest(engine, rng, n, one_key=True)
    assert (pks == pks[0]).all()
    co = rng.integers(0, 256, size=(1, 32), dtype=np.uint8)
    co[0, 31] &= 0x3F
    coeffs = np.repeat(co, n, axis=0)
    lin = lin_of(sigs, coeffs)
    want = generator_multiple(oracle, lin)
    rec = engines["bucket"].verify_batch_msm_partial(sigs, pks, msgs, coeffs=coeffs)
    check_record(oracle, rec, want, lin)
    assert engine.verify_batch_msm(sigs, pks, msgs, coeffs=coeffs) == OK
    bad = msgs.copy()
    bad[n - 1, 0] ^= 1
    rec_bad = engines["bucket"].verify_batch_msm_partial(sigs, pks, bad, coeffs=coeffs)
    assert int(rec_bad[22]) == 0 and mr.record_lin(rec_bad) == lin
    assert mr.record_point(oracle, rec_bad) != want and mr.record_is_wellformed(oracle, rec_bad)
    assert engine.verify_batch_msm(sigs, pks, bad, coeffs=coeffs) == INVALID


def test_duplicated_honest_lanes_on_the_bucket_path(engine, oracle):
    """5000 honest lanes, lanes 0..9 copied over lanes 10..19, random 32-byte coefficients: equal points with
    different digits, on the path a caller takes"""
    n = 5000
    rng = np.random.default_rng(0x5000)
    sigs, pks, msgs = honest(engine, rng, n)
    for a in (sigs, pks, msgs):
        a[10:20] = a[0:10]
    coeffs = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    assert engine.verify_batch_msm(sigs, pks, msgs, coeffs=coeffs) == OK
    lin = lin_of(sigs, coeffs)
    rec = engine.verify_batch_msm_partial(sigs, pks, msgs, coeffs=coeffs)
    check_record(oracle, rec, generator_multiple(oracle, lin), lin)
