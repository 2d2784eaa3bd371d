"""Many half-aggregates in one call (ssa_verify_aggregates_many).  The contract is one equality:
verdict j of the call is what ssa_verify_aggregate gives aggregate j handed in alone.  Every test compares with that
single call (on the session's engine) and, for aggregates of a few lanes, with the model of tests/aggregate_model.py over
the C oracle.  Both internal paths are driven by contexts created under SSA_MSM_SMALL_MAX: "small" (every group through
msm_k_small and the segmented record sum) and "bucket" (every group padded and through the screened MSM)."""
import os

import numpy as np
import pytest

import aggregate_model as am

pytestmark = pytest.mark.gpu

Q = am.Q
OK, INVALID, MALFORMED = 0, 2, 3
BOUNDARY = [1, 2, 3, 255, 256, 257, 511, 512, 513, 0, 1]
POOL = sum(BOUNDARY)            # 2311 honest lanes, every test cuts its aggregates out of them
PATHS = ["small", "bucket"]


def make_scalars(rng, n):
    s = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    s[:, 31] &= 0x3F
    s[:, 0] |= 1
    return s


def e_bytes(e):
    return np.frombuffer(int(e).to_bytes(32, "little"), np.uint8)


def e_of(agg):
    return int.from_bytes(agg[-32:].tobytes(), "little")


def with_e(agg, e):
    out = agg.copy()
    out[-32:] = e_bytes(e)
    return out


class Pool:
    """POOL honest signatures over 80-byte messages (made once)"""

    def __init__(self, engine):
        rng = np.random.default_rng(0xA6621)
        self.msgs = rng.integers(0, 256, size=(POOL, 80), dtype=np.uint8)
        self.pks, self.sigs = engine.keygen_sign_many(make_scalars(rng, POOL), make_scalars(rng, POOL), self.msgs)
        self._built = {}

    def build(self, engine, counts):
        """honest aggregates of consecutive pool lanes -> list of uint8 arrays (made once per list of counts)"""
        key = tuple(counts)
        if key not in self._built:
            out, lo = [], 0
            for n in counts:
                st, agg, _, nf = engine.aggregate(self.sigs[lo:lo + n], self.pks[lo:lo + n], self.msgs[lo:lo + n])
                assert st == OK and nf == 0
                out.append(agg)
                lo += n
            self._built[key] = out
        return [a.copy() for a in self._built[key]]


_STATE = {}


@pytest.fixture
def pool(engine):
    if "pool" not in _STATE:
        _STATE["pool"] = Pool(engine)
    return _STATE["pool"]


@pytest.fixture(scope="module")
def engines():
    """contexts that take one path for every group, whatever its size"""
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


def counts_of(aggs):
    return [(a.size - 32) // 49 for a in aggs]


def ranges_of(aggs):
    lo, out = 0, []
    for n in counts_of(aggs):
        out.append((lo, lo + n))
        lo += n
    return out


def singles(engine, aggs, pks, msgs, inf=None):
    """the reference: ssa_verify_aggregate once per aggregate, with its own keys and messages"""
    out = []
    for a, (lo, hi) in zip(aggs, ranges_of(aggs)):
        out.append(engine.verify_aggregate(a, pks[lo:hi], msgs[lo:hi] if hi > lo else None,
                                           pk_inf=None if inf is None else inf[lo:hi]))
    return out


def model(oracle, aggs, pks, msgs, which, inf=None):
    be, rg = am.oracle_backend(oracle), ranges_of(aggs)
    return [am.verify(be, aggs[j], pks[rg[j][0]:rg[j][1]], msgs[rg[j][0]:rg[j][1]],
                      None if inf is None else inf[rg[j][0]:rg[j][1]]) for j in which]


def many(eng, aggs, pks, msgs, inf=None):
    n = sum(counts_of(aggs))
    return eng.verify_aggregates(aggs, pks[:n], msgs[:n], pk_inf=None if inf is None else inf[:n]).tolist()


@pytest.mark.parametrize("path", PATHS)
def test_boundary_sizes_in_one_call(engine, engines, oracle, pool, path):
    aggs = pool.build(engine, BOUNDARY)
    got = many(engines[path], aggs, pool.pks, pool.msgs)
    assert got == [OK] * len(BOUNDARY)
    if "boundary_single" not in _STATE:
        _STATE["boundary_single"] = singles(engine, aggs, pool.pks, pool.msgs)
        _STATE["boundary_model"] = model(oracle, aggs, pool.pks, pool.msgs, [0, 1, 9, 10])
    assert got == _STATE["boundary_single"]
    assert [got[j] for j in (0, 1, 9, 10)] == _STATE["boundary_model"]
    # the coefficients are those of each aggregate alone: local lane index, its own n and root
    co = engines[path].aggregates_coeffs(aggs, pool.pks, pool.msgs)
    rg = ranges_of(aggs)
    for j in (0, 5, 8):
        lo, hi = rg[j]
        alone = engine.aggregate_coeffs(aggs[j][:-32], pool.pks[lo:hi], pool.msgs[lo:hi])
        assert (co[lo:hi] == alone).all(), j
    # and the model's, for EVERY aggregate of the pool: the single call runs the same transcript kernels, the model does not
    if "boundary_coeffs" not in _STATE:
        be = am.oracle_backend(oracle)
        _STATE["boundary_coeffs"] = [am.coeff_bytes(am.coefficients(be, pool.sigs[lo:hi, :49], pool.pks[lo:hi], pool.msgs[lo:hi]))
                                     if hi > lo else np.zeros((0, 16), np.uint8) for lo, hi in rg]
    assert co.shape == (POOL, 16)
    for j, (lo, hi) in enumerate(rg):
        assert (co[lo:hi] == _STATE["boundary_coeffs"][j]).all(), j


@pytest.mark.parametrize("path", PATHS)
def test_more_aggregates_than_a_group_holds(engine, engines, oracle, pool, path):
    rng = np.random.default_rng(0x300)
    counts = [int(c) for c in rng.integers(1, 5, size=300)]
    aggs = pool.build(engine, counts)
    rg = ranges_of(aggs)
    msgs = pool.msgs.copy()
    e0 = e_of(aggs[0])
    aggs[0] = with_e(aggs[0], e0 ^ 1 if e0 ^ 1 < Q else e0 ^ 2)     # one bit of e_agg
    msgs[rg[255][0], 3] ^= 0x10                                     # one message bit
    aggs[256] = with_e(aggs[256], Q + 5)                            # e_agg >= q
    aggs[299][48] |= 0x01                                           # an undecodable flag byte
    got = many(engines[path], aggs, pool.pks, msgs)
    if "many300" not in _STATE:
        _STATE["many300"] = singles(engine, aggs, pool.pks, msgs)
        _STATE["many300_model"] = model(oracle, aggs, pool.pks, msgs, [0, 1, 255, 256, 298, 299])
    want = _STATE["many300"]
    assert [want[j] for j in (0, 255, 256, 299)] == [INVALID, INVALID, MALFORMED, MALFORMED]
    assert sum(v != OK for v in want) == 4
    assert got == want
    assert [got[j] for j in (0, 1, 255, 256, 298, 299)] == _STATE["many300_model"]


def identity_lanes(engine, rng, n):
    """n signatures that verify under the IDENTITY key with any message: R = [e]G"""
    es = make_scalars(rng, n)
    comp, st = engine.compress_many(engine.pubkey_many(es))
    assert (st == 0).all()
    return np.concatenate([comp, es], axis=1), np.zeros((n, 96), np.uint8), np.ones(n, np.uint8)


@pytest.mark.parametrize("path", PATHS)
def test_every_rejection_among_honest_neighbours(engine, engines, oracle, pool, path):
    import pymodel as pm
    eng = engines[path]
    counts = [3, 5, 4, 2]
    T, lo = 1, 3                                   # the touched aggregate and its first lane
    honest = pool.build(engine, counts)
    n_all = sum(counts)
    pks, msgs = pool.pks[:n_all], pool.msgs[:n_all]
    assert many(eng, honest, pks, msgs) == [OK] * 4

    def check(aggs, expect, pks=pks, msgs=msgs, inf=None, model_too=()):
        got = many(eng, aggs, pks, msgs, inf)
        want = singles(engine, aggs, pks, msgs, inf)
        assert got == want == expect, (got, want, expect)
        if model_too:                              # (the model's answer does not depend on the path: asked once)
            key = ("rejections", len(_STATE.setdefault("rej_seen_" + path, [])))
            _STATE["rej_seen_" + path].append(key)
            if key not in _STATE:
                _STATE[key] = model(oracle, aggs, pks, msgs, model_too, inf)
            assert _STATE[key] == [expect[j] for j in model_too]

    def touched(change):
        aggs = [a.copy() for a in honest]
        change(aggs[T])
        return aggs

    def only(v):
        return [v if j == T else OK for j in range(4)]

    check(touched(lambda a: a.__setitem__(49 * 2 + 48, a[49 * 2 + 48] ^ 0x40)), only(INVALID), model_too=(T,))   # R's sort bit
    e = e_of(honest[T])
    check(touched(lambda a: a.__setitem__(slice(-32, None), e_bytes(Q - e))), only(INVALID), model_too=(T,))     # global sign
    check(touched(lambda a: a.__setitem__(slice(-32, None), e_bytes(Q))), only(MALFORMED))                       # e_agg = q
    check(touched(lambda a: a.__setitem__(slice(49, 57), 0xFF)), only(MALFORMED))                                # a limb >= p
    for t in range(1, 64):                                                     # an x with no point on the curve
        x = honest[T][49 * 3: 49 * 4].copy()
        x[8] ^= t
        if pm.pt_decompress(x.tobytes())[0] == "invalid":
            break
    check(touched(lambda a: a.__setitem__(slice(49 * 3, 49 * 4), x)), only(MALFORMED))
    off_curve = pks.copy()
    off_curve[lo + 4, 50] ^= 1                                                 # a key off the curve
    check(honest, only(MALFORMED), pks=off_curve)

    def swap(a):
        a[:49], a[49:98] = a[49:98].copy(), a[:49].copy()
    check(touched(swap), only(INVALID))                                        # two lanes swapped
    # the last lane of aggregate 1 handed to aggregate 2 (counts 3, 4, 5, 2): keys and messages keep their order
    moved = [a.copy() for a in honest]
    moved[1] = np.concatenate([honest[1][:49 * 4], honest[1][-32:]])
    moved[2] = np.concatenate([honest[1][49 * 4: 49 * 5], honest[2]])
    assert counts_of(moved) == [3, 4, 5, 2]
    check(moved, [OK, INVALID, INVALID, OK], model_too=(1, 2))

    # the fully negated left side under identity keys, in place of aggregate 1
    rng = np.random.default_rng(0x1DE0)
    isigs, ipks, iinf = identity_lanes(engine, rng, 5)
    pk2, inf2 = pks.copy(), np.zeros(n_all, np.uint8)
    pk2[lo:lo + 5], inf2[lo:lo + 5] = ipks, iinf
    be = am.oracle_backend(oracle)
    neg = isigs.copy()
    neg[:, 48] ^= 0x40
    e_neg = am.fold(am.coefficients(be, neg[:, :49], ipks, msgs[lo:lo + 5]), isigs)
    body = np.concatenate([neg[:, :49].reshape(-1), np.zeros(32, np.uint8)])
    aggs = [a.copy() for a in honest]
    aggs[T] = with_e(body, e_neg)
    check(aggs, only(INVALID), pks=pk2, inf=inf2)
    aggs[T] = with_e(body, (Q - e_neg) % Q)
    check(aggs, [OK] * 4, pks=pk2, inf=inf2)
    aggs[T] = np.frombuffer(am.aggregate(be, isigs, ipks, msgs[lo:lo + 5]), np.uint8).copy()
    check(aggs, [OK] * 4, pks=pk2, inf=inf2)
    check(aggs, only(MALFORMED), pks=pk2)                                      # (0, 0) without its flag is no point


@pytest.mark.parametrize("path", PATHS)
def test_errors_that_cancel_in_a_joint_sum_are_both_caught(engine, engines, oracle, pool, path):
    aggs = pool.build(engine, [3, 2])
    delta = 0x1234567
    aggs[0] = with_e(aggs[0], (e_of(aggs[0]) + delta) % Q)
    aggs[1] = with_e(aggs[1], (e_of(aggs[1]) - delta) % Q)
    got = many(engines[path], aggs, pool.pks, pool.msgs)
    assert got == [INVALID, INVALID] == singles(engine, aggs, pool.pks, pool.msgs)
    assert model(oracle, aggs, pool.pks, pool.msgs, [0, 1]) == got


@pytest.mark.parametrize("path", PATHS)
def test_layouts_and_forms_agree(engine, engines, pool, path):
    import torch
    import schnorr_sig_amd as ssa
    eng = engines[path]
    counts = [4, 0, 7, 300, 1]
    n = sum(counts)
    aggs = pool.build(engine, counts)
    pks, msgs, inf = pool.pks[:n].copy(), pool.msgs[:n].copy(), np.zeros(n, np.uint8)
    rng = np.random.default_rng(0x1A7)
    rg = ranges_of(aggs)
    # aggregate 2 becomes identity-key lanes; aggregate 3 gets a wrong message; the empty one a nonzero scalar
    isigs, ipks, iinf = identity_lanes(engine, rng, 7)
    lo, hi = rg[2]
    pks[lo:hi], inf[lo:hi] = ipks, iinf
    st, aggs[2], _, _ = engine.aggregate(isigs, ipks, msgs[lo:hi], pk_inf=iinf)
    assert st == OK
    msgs[rg[3][0] + 299, 0] ^= 1
    aggs[1] = with_e(aggs[1], 1)
    want = singles(engine, aggs, pks, msgs, inf)
    assert want == [OK, INVALID, OK, INVALID, OK]
    assert many(eng, aggs, pks, msgs, inf) == want
    # messages by offset table, of ragged lengths: lane i keeps 80 - (i % 3) bytes
    rows = [bytes(msgs[i, :80 - (i % 3)]) for i in range(n)]
    flat, off = ssa.pack_messages(rows)
    want_r = []
    for a, (lo, hi) in zip(aggs, rg):
        f, o = ssa.pack_messages(rows[lo:hi])
        want_r.append(engine.verify_aggregate(a, pks[lo:hi], f, offsets=o, pk_inf=inf[lo:hi]))
    assert eng.verify_aggregates(aggs, pks, flat, pk_inf=inf, offsets=off).tolist() == want_r
    # the device form: strided messages, then the offset table
    wire = np.concatenate(aggs)
    d_wire, d_pks, d_msgs, d_inf, d_flat, d_off = [torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0") for a in
                                                   (wire, pks, msgs, inf, flat, off.astype(np.int64))]
    v = torch.full((len(counts),), 255, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    eng.verify_aggregates_device(d_wire, counts, d_pks, d_msgs, d_verdicts=v, d_pk_inf=d_inf)
    eng.sync()
    assert v.cpu().tolist() == want
    v.fill_(255)
    torch.cuda.synchronize()
    eng.verify_aggregates_device(d_wire, counts, d_pks, d_flat, d_verdicts=v, d_pk_inf=d_inf, d_offsets=d_off)
    eng.sync()
    assert v.cpu().tolist() == want_r
    # reversing the aggregates (with their keys, flags and messages) reverses the verdicts
    order = list(range(len(counts)))[::-1]
    idx = np.concatenate([np.arange(*rg[j]) for j in order]).astype(np.int64)
    assert many(eng, [aggs[j] for j in order], pks[idx], msgs[idx], inf[idx]) == want[::-1]


@pytest.mark.parametrize("path", ["bucket", "default"])
def test_unequal_sizes_in_one_group(engine, engines, pool, path):
    eng = engine if path == "default" else engines[path]
    counts = [600, 300, 1024, 257]
    aggs = pool.build(engine, counts)
    n = sum(counts)
    lo = 600 + 300 + 1024
    assert many(eng, aggs, pool.pks, pool.msgs) == [OK] * 4
    msgs = pool.msgs[:n].copy()
    msgs[lo + 256, 79] ^= 0x80                       # the last lane of the shortest aggregate, next to the padding
    assert many(eng, aggs, pool.pks, msgs) == [OK, OK, OK, INVALID] == singles(engine, aggs, pool.pks, msgs)
    pks = pool.pks[:n].copy()
    pks[lo, 0] ^= 1                                  # its first lane: a key off the curve
    assert many(eng, aggs, pks, pool.msgs) == [OK, OK, OK, MALFORMED] == singles(engine, aggs, pks, pool.msgs)
    # padding is not malformed: a bad R in the longest aggregate touches that one alone
    aggs[2][49 * 1023 + 48] |= 0x01
    assert many(eng, aggs, pool.pks, pool.msgs) == [OK, OK, MALFORMED, OK] == singles(engine, aggs, pool.pks, pool.msgs)


@pytest.mark.parametrize("path", PATHS)
def test_identity_on_both_sides_and_on_one_side_only(engine, engines, oracle, path):
    """Every lane the identity key with the identity R: the left side is the identity whatever the coefficients are, so
    the comparison meets identity == identity where e_agg = 0 (valid) and the identity against [e_agg]G where it is not
    (invalid) -- in one call, in the single call on the same path, and in the model."""
    counts = [1, 3, 0, 17]
    n = sum(counts)
    rng = np.random.default_rng(0x1D1D)
    pks, inf = np.zeros((n, 96), np.uint8), np.ones(n, np.uint8)
    msgs = rng.integers(0, 256, size=(n, 80), dtype=np.uint8)
    r = np.zeros(49, np.uint8)
    r[48] = 0x80                                     # x = 0 with the infinity flag
    for k, es in enumerate(([0, 0, 0, 0], [1, Q - 1, 0, 0x1234567 << 200], [0, 5, 0, 0])):
        aggs = [np.concatenate([np.tile(r, c), e_bytes(e)]) for c, e in zip(counts, es)]
        expect = [OK if e == 0 else INVALID for e in es]
        got = many(engines[path], aggs, pks, msgs, inf)
        assert got == expect == singles(engines[path], aggs, pks, msgs, inf) == singles(engine, aggs, pks, msgs, inf)
        key = ("identity_sides", k)
        if key not in _STATE:                        # (the model's answer does not depend on the path: asked once)
            _STATE[key] = model(oracle, aggs, pks, msgs, range(4), inf)
        assert _STATE[key] == expect


@pytest.mark.parametrize("path", PATHS)
def test_hygiene(engine, engines, pool, path):
    import schnorr_sig_amd as ssa
    eng = engines[path]
    counts = [5, 257, 0, 40]
    n = sum(counts)
    aggs = pool.build(engine, counts)
    aggs[3][48] ^= 0x40
    want = [OK, OK, OK, INVALID]
    bad = pool.sigs.copy()
    bad[[7, 1500, 2300], 49] ^= 1
    fresh = ssa.Engine(0)
    try:
        want_scr = fresh.verify_batch_screened(bad, pool.pks, pool.msgs)
        want_one = fresh.verify_aggregate(aggs[1], pool.pks[5:262], pool.msgs[5:262])
    finally:
        fresh.close()
    assert want_scr[1] == 3 and want_one == OK
    for prelude in (lambda: eng.debug_poison_workspaces(0xA5),
                    lambda: eng.verify_batch_screened(bad, pool.pks, pool.msgs),     # leaves failing segments behind
                    lambda: eng.debug_poison_workspaces(0xFF)):
        prelude()
        assert many(eng, aggs, pool.pks, pool.msgs) == want
        got = eng.verify_batch_screened(bad, pool.pks, pool.msgs)
        assert (got[0] == want_scr[0]).all() and got[1] == want_scr[1]
        assert many(eng, aggs, pool.pks, pool.msgs) == want
        assert eng.verify_aggregate(aggs[1], pool.pks[5:262], pool.msgs[5:262]) == want_one


def test_no_aggregates_and_only_empty_ones(engine):
    none = np.zeros((0, 96), np.uint8)
    assert engine.verify_aggregates([], none, None).tolist() == []
    z = np.zeros(32, np.uint8)
    assert engine.verify_aggregates([z, with_e(z, 1), with_e(z, Q)], none, None).tolist() == [OK, INVALID, MALFORMED]
