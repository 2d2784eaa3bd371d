"""Screened batch verification (ssa_verify_batch_screened): every status vector is compared with
the exact per-lane vector of ssa_verify_many(..., SSA_FLAG_SIG_FLAG_BYTE, no subgroup check) on the same inputs, and
the statuses of the corrupted lanes with the CPU oracle."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 2**64 - 2**32 + 1
Q = 0x7AF2599B3B3F22D0563FBF0F990A37B5327AA72330157722D443623EAED4ACCF


def make_scalars(rng, n):
    s = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    s[:, 31] &= 0x3F
    s[:, 0] |= 1
    return s


def honest(engine, rng, n, msg_len=80, sks=None):
    sks = make_scalars(rng, n) if sks is None else sks
    nonces = make_scalars(rng, n)
    msgs = rng.integers(0, 256, size=(n, msg_len), dtype=np.uint8)
    pks, sigs = engine.keygen_sign_many(sks, nonces, msgs)
    return sigs, pks, msgs


def coeffs32(rng, n):
    c = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    c[:, 31] &= 0x3F
    return c


def per_lane(engine, sigs, pks, msgs, pk_inf=None):
    return engine.verify_many(sigs, pks, msgs, check_torsion=False, pk_inf=pk_inf, sig_flag_byte=True)


def assert_matches(engine, sigs, pks, msgs, coeffs=None, pk_inf=None):
    st, nf = engine.verify_batch_screened(sigs, pks, msgs, coeffs=coeffs, pk_inf=pk_inf)
    want, wnf = per_lane(engine, sigs, pks, msgs, pk_inf)
    bad = np.nonzero(st != want)[0]
    assert bad.size == 0, (bad[:10], st[bad[:10]], want[bad[:10]])
    assert nf == wnf == int((want != 0).sum())
    return st


def corrupt(rng, sigs, pks, msgs, lanes):
    """one corruption of every class, cycling over `lanes`"""
    kinds = ["e_bit", "msg_bit", "sort_bit", "swap_key", "noncanon_pk", "e_ge_q", "pk_off_curve", "x_changed", "flag_byte"]
    n = sigs.shape[0]
    for k, i in enumerate(lanes):
        kind = kinds[k % len(kinds)]
        if kind == "e_bit":
            sigs[i, 49] ^= 1
        elif kind == "msg_bit":
            msgs[i, rng.integers(0, msgs.shape[1])] ^= 0x10
        elif kind == "sort_bit":
            sigs[i, 48] ^= 0x40                                   # R -> -R
        elif kind == "swap_key":
            pks[i] = pks[(i + 1) % n]
        elif kind == "noncanon_pk":
            pks[i, 0:8] = 0xFF
        elif kind == "e_ge_q":
            sigs[i, 49:81] = 0xFF
        elif kind == "pk_off_curve":
            pks[i, 48] ^= 1
        elif kind == "x_changed":                                 # off the curve about half of the time: 2 or 3
            sigs[i, 0] ^= 1
        else:
            sigs[i, 48] |= 0x01
    return kinds


@pytest.mark.parametrize("n", [5000, 1 << 16, 1 << 20])
def test_honest_batches_pass_with_caller_and_library_coefficients(engine, n):
    rng = np.random.default_rng(9100 + n)
    sigs, pks, msgs = honest(engine, rng, n)
    for co in (coeffs32(rng, n), None):
        st, nf = engine.verify_batch_screened(sigs, pks, msgs, coeffs=co)
        assert st.shape == (n,) and (st == 0).all() and nf == 0


def test_every_class_of_bad_lane_gets_its_per_lane_status(engine, oracle):
    rng = np.random.default_rng(9201)
    n = 20000
    sigs, pks, msgs = honest(engine, rng, n)
    co = coeffs32(rng, n)
    import schnorr_sig_amd as ssa
    plan = ssa.debug_screen_plan(n)
    seg = plan["segment_lanes"]
    edges = [0, seg - 1, seg, 2 * seg - 1, 5 * seg, n - 1]
    lanes = sorted(set(edges + list(rng.choice(n, 30, replace=False))))
    corrupt(rng, sigs, pks, msgs, lanes)
    for c in (co, None):
        st = assert_matches(engine, sigs, pks, msgs, coeffs=c)
        assert (st[lanes] != 0).all()
    # the per-lane statuses of these lanes are the oracle's
    samp = np.array(lanes + [1, 2, seg + 1, n - 2])
    want = oracle.verify_many(sigs[samp], pks[samp], msgs[samp], check_torsion=False, sig_flag_byte=True)
    assert (st[samp] == want).all()
    assert set(int(v) for v in st[lanes]) <= {2, 3} and (st == 3).sum() >= 4 and (st == 2).sum() >= 4


@pytest.mark.parametrize("k", [2, 16, 256])
def test_forced_segment_counts_give_identical_vectors(k):
    """one context per K (the setting is per context); n = 20000 leaves the last segment ragged for every K"""
    import schnorr_sig_amd as ssa
    eng = ssa.Engine(0)
    try:
        rng = np.random.default_rng(9301)
        n = 20000
        sigs, pks, msgs = honest(eng, rng, n)
        co = coeffs32(rng, n)
        lanes = sorted(set([0, 255, 256, n - 1] + list(rng.choice(n, 12, replace=False))))
        corrupt(rng, sigs, pks, msgs, lanes)
        base, _ = eng.verify_batch_screened(sigs, pks, msgs, coeffs=co)
        eng.debug_screen_segments(k)
        st = assert_matches(eng, sigs, pks, msgs, coeffs=co)
        assert (st == base).all()
        eng.debug_screen_segments(0)
    finally:
        eng.close()


def test_one_bad_lane_in_1024_takes_the_whole_slice_path(engine):
    rng = np.random.default_rng(9401)
    n = 1 << 16
    sigs, pks, msgs = honest(engine, rng, n)
    lanes = list(range(17, n, 1024))                              # every segment fails
    corrupt(rng, sigs, pks, msgs, lanes)
    st = assert_matches(engine, sigs, pks, msgs, coeffs=coeffs32(rng, n))
    assert (st[lanes] != 0).all() and (st != 0).sum() == len(lanes)


def test_identity_keys_identity_r_and_one_key_with_equal_coefficients(engine, oracle):
    import pymodel as m
    rng = np.random.default_rng(9501)
    n = 6000
    sigs, pks, msgs = honest(engine, rng, n)
    inf = np.zeros(n, np.uint8)
    co = coeffs32(rng, n)
    # identity keys: a signature with e = r and R = [r]G verifies (pk = O contributes nothing); one of them is wrong
    kl = np.array([3, 700, 4095, 4096, 5999])
    r = make_scalars(rng, kl.size)
    rp, _ = engine.keygen_sign_many(r, r, msgs[kl])
    rc, _ = engine.compress_many(rp)
    pks[kl] = 0
    inf[kl] = 1
    sigs[kl, :49] = rc
    sigs[kl, 49:] = r
    sigs[kl[-1], 49] ^= 2
    # identity R (x = 0, infinity flag): e = -h sk makes [h]P + [e]G = O, one of them is off by one
    il = np.array([10, 2047, 2048, 5000])
    sks = make_scalars(rng, il.size)
    ipk, _ = engine.keygen_sign_many(sks, sks, msgs[il])
    pks[il] = ipk
    sigs[il, :48] = 0
    sigs[il, 48] = 0x80
    dig = engine.hash_message_many(sigs[il], pks[il], msgs[il])
    for j, i in enumerate(il):
        h = m.scalar_from_digest(bytes(dig[j]))
        sk = int.from_bytes(sks[j].tobytes(), "little")
        e = (-h * sk) % Q
        if j == 1:
            e = (e + 1) % Q
        sigs[i, 49:] = np.frombuffer(e.to_bytes(32, "little"), np.uint8)
    # 256 signatures under one key with equal coefficients: equal points in one bucket
    same = np.arange(1024, 1280)
    one_sk = np.tile(make_scalars(rng, 1), (same.size, 1))
    s2, p2, m2 = honest(engine, rng, same.size, sks=one_sk)
    sigs[same], pks[same], msgs[same] = s2, p2, m2
    co[same] = co[same[0]]
    st = assert_matches(engine, sigs, pks, msgs, coeffs=co, pk_inf=inf)
    assert (st[kl[:-1]] == 0).all() and st[kl[-1]] == 2
    assert st[il[0]] == 0 and st[il[1]] == 2 and (st[il[2:]] == 0).all()
    assert (st[same] == 0).all()
    samp = np.concatenate([kl, il])
    want = oracle.verify_many(sigs[samp], pks[samp], msgs[samp], check_torsion=False, pk_inf=inf[samp],
                              sig_flag_byte=True)
    assert (st[samp] == want).all()
    sigs[same[77], 60] ^= 1                                       # one of the equal-coefficient lanes is bad
    st = assert_matches(engine, sigs, pks, msgs, coeffs=co, pk_inf=inf)
    assert st[same[77]] == 2 and (np.delete(st[same], 77) == 0).all()


def test_segments_whose_two_sides_are_the_identity_or_only_one_is(oracle):
    """Every lane the identity key with the identity R: a segment's left side is the identity, its right side
    [sum s_i e_i]G.  Where every e is 0 the comparison meets identity == identity and the segment passes; where not, the
    identity against a point, and its lanes fail the exact check too.  600 lanes in three forced segments above a
    small-batch bound of 256: three 256-lane blocks, the last ragged."""
    import schnorr_sig_amd as ssa
    old = os.environ.get("SSA_MSM_SMALL_MAX")
    os.environ["SSA_MSM_SMALL_MAX"] = "256"
    try:
        eng = ssa.Engine(0)
    finally:
        if old is None:
            os.environ.pop("SSA_MSM_SMALL_MAX", None)
        else:
            os.environ["SSA_MSM_SMALL_MAX"] = old
    try:
        eng.debug_screen_segments(3)
        rng = np.random.default_rng(9551)
        n = 600
        pks, inf = np.zeros((n, 96), np.uint8), np.ones(n, np.uint8)
        msgs = rng.integers(0, 256, size=(n, 80), dtype=np.uint8)
        co = coeffs32(rng, n)
        samp = np.array([0, 255, 256, 511, 512, 599])
        for nonzero in (slice(0, 0), slice(0, n), slice(256, 512)):
            sigs = np.zeros((n, 81), np.uint8)
            sigs[:, 48] = 0x80                                    # x = 0 with the infinity flag; e = 0
            sigs[nonzero, 49:] = make_scalars(rng, n)[nonzero]
            expect = np.zeros(n, np.uint8)
            expect[nonzero] = 2
            for c in (co, None):
                st = assert_matches(eng, sigs, pks, msgs, coeffs=c, pk_inf=inf)
                assert (st == expect).all()
            want = oracle.verify_many(sigs[samp], pks[samp], msgs[samp], check_torsion=False, pk_inf=inf[samp],
                                      sig_flag_byte=True)
            assert (expect[samp] == want).all()
    finally:
        eng.close()


def test_global_sign_is_rejected_lane_by_lane(engine):
    """e -> q - e in every signature: the x-only MSM verdict accepts (class 2), the screened
    form compares points and rejects every lane"""
    rng = np.random.default_rng(9601)
    n = 4096
    sigs, pks, msgs = honest(engine, rng, n)
    neg = sigs.copy()
    for i in range(n):
        e = int.from_bytes(sigs[i, 49:].tobytes(), "little")
        neg[i, 49:] = np.frombuffer(((Q - e) % Q).to_bytes(32, "little"), np.uint8)
    co = coeffs32(rng, n)
    assert engine.verify_batch_msm(neg, pks, msgs, coeffs=co) == 0
    st, nf = engine.verify_batch_screened(neg, pks, msgs, coeffs=co)
    assert (st == 2).all() and nf == n


def test_small_order_error_is_caught_exactly_when_the_reduced_product_is_odd(engine):
    """key P + T2 (T2 of order 2), h odd: the per-lane check rejects (E = T2).  The segment's sum sees the key through
    the reduced scalar b = s h mod q (src/batch.rs:109-111), so its T2 part is [b] T2 -- the documented 1/l case: a
    coefficient with b odd rejects the lane, one with b even accepts it"""
    import pymodel as m
    rng = np.random.default_rng(9701)
    n = 4096
    sigs, pks, msgs = honest(engine, rng, n)
    g = m.default_params().generator()
    t2 = m.SMALL_ORDER_POINTS[2]
    sk, r = 0x1234567 + 2 * int(rng.integers(1, 1 << 30)), 0x7654321
    pk = m.pt_add(m.pt_mul(sk, g), t2)
    rp = m.pt_mul(r, g)
    msg = bytearray(rng.integers(0, 256, 80, dtype=np.uint8).tobytes())
    while True:
        h = m.scalar_from_digest(m.hash_message(rp[0], pk, bytes(msg)))
        if h & 1:
            break
        msg[0] = (msg[0] + 1) & 0xFF
    e = (r - sk * h) % Q
    i = 1500
    sigs[i] = np.frombuffer(m.pt_compress(rp) + e.to_bytes(32, "little"), np.uint8)
    pks[i] = np.frombuffer(m.fp6_to_bytes48(pk[0]) + m.fp6_to_bytes48(pk[1]), np.uint8)
    msgs[i] = np.frombuffer(bytes(msg), np.uint8)
    want, _ = per_lane(engine, sigs, pks, msgs)
    assert want[i] == 2 and (np.delete(want, i) == 0).all()
    co = coeffs32(rng, n)
    for parity, expect in ((1, 2), (0, 0), (1, 2), (0, 0)):
        while True:
            s = int.from_bytes(rng.bytes(32), "little") % Q
            if (s * h % Q) & 1 == parity:
                break
        co[i] = np.frombuffer(s.to_bytes(32, "little"), np.uint8)
        st, nf = engine.verify_batch_screened(sigs, pks, msgs, coeffs=co)
        assert st[i] == expect and nf == (1 if expect else 0) and (np.delete(st, i) == 0).all(), (parity, s)


_CHILD = r"""
import json, os, sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, os.path.join(%(root)r, "oracle"))
import numpy as np
import torch
import schnorr_sig_amd as ssa
rng = np.random.default_rng(9801)
n = 12000
e = ssa.Engine(0)
sk = rng.integers(0, 256, size=(n, 32), dtype=np.uint8); sk[:, 31] &= 0x3f; sk[:, 0] |= 1
nn = rng.integers(0, 256, size=(n, 32), dtype=np.uint8); nn[:, 31] &= 0x3f; nn[:, 0] |= 1
m = rng.integers(0, 256, size=(n, 80), dtype=np.uint8)
pk, sg = e.keygen_sign_many(sk, nn, m)
bad = [0, 4999, 5000, 6123, 9999, 10000, 11999]
for i in bad:
    sg[i, 50] ^= 4
sg[7000, 48] |= 1
co = rng.integers(0, 256, size=(n, 32), dtype=np.uint8); co[:, 31] &= 0x3f
st, nf = e.verify_batch_screened(sg, pk, m, coeffs=co)
want, wnf = e.verify_many(sg, pk, m, check_torsion=False, sig_flag_byte=True)
dev = torch.device("cuda", 0)
ds, dp, dm, dc = (torch.from_numpy(a).to(dev) for a in (sg, pk, m, co))
dst = torch.full((n,), 255, dtype=torch.uint8, device=dev)
dnf = torch.zeros(1, dtype=torch.int64, device=dev)
torch.cuda.synchronize()
s = torch.cuda.Stream(device=dev)
e.set_stream(s.cuda_stream)
e.verify_batch_screened_device(ds.data_ptr(), dp.data_ptr(), dm.data_ptr(), n, 80, dc.data_ptr(), 32, dst.data_ptr(),
                               dnf.data_ptr())
with torch.cuda.stream(s):             # ordered on the context's stream, no host synchronisation in between
    dev_st = dst.cpu().numpy()
    dev_nf = int(dnf.cpu().item())
e.set_stream(None)
print("RESULT " + json.dumps({"equal": bool((st == want).all()), "nf": [int(nf), int(wnf), dev_nf],
                              "dev_equal": bool((dev_st == st).all()), "bad": [int(st[i]) for i in bad + [7000]]}))
e.close()
"""


def test_more_than_one_slice_host_and_device_forms():
    """SSA_MSM_SLICE = 5000: slices of 5000, 5000 and 2000 lanes (the last one on the per-lane path); the device form,
    on a caller stream, equals the host form"""
    env = dict(os.environ)
    env["SSA_MSM_SLICE"] = "5000"
    r = subprocess.run([sys.executable, "-c", _CHILD % {"root": ROOT}], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    assert out["equal"] and out["dev_equal"]
    assert out["nf"] == [8, 8, 8]
    assert out["bad"] == [2] * 7 + [3]
