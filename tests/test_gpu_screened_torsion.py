"""Screened Signature::verify (ssa_verify_many_screened): every status vector is compared, lane for
lane, with ssa_verify_many on the same inputs and flags, the count with its count, and the corrupted lanes and a sample
of clean ones with the CPU oracle.  The three new flag settings are SSA_FLAG_CHECK_TORSION (Signature::verify), both
flags, and neither; SSA_FLAG_SIG_FLAG_BYTE alone is ssa_verify_batch_screened."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q = 0x7AF2599B3B3F22D0563FBF0F990A37B5327AA72330157722D443623EAED4ACCF
T, TF, NONE, F = (dict(check_torsion=True, sig_flag_byte=False), dict(check_torsion=True, sig_flag_byte=True),
                  dict(check_torsion=False, sig_flag_byte=False), dict(check_torsion=False, sig_flag_byte=True))
NEW_SETTINGS = [T, TF, NONE]
ALL_SETTINGS = [T, TF, NONE, F]


def make_scalars(rng, n):
    s = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    s[:, 31] &= 0x3F
    s[:, 0] |= 1
    return s


def key_choice(rng, n, u):
    idx = rng.integers(0, u, size=n)
    idx[:u] = np.arange(u)
    rng.shuffle(idx)
    return idx


def honest(engine, rng, n, u, msg_len=80):
    """n honest signatures by u distinct signers"""
    sks = make_scalars(rng, u)[key_choice(rng, n, u)]
    msgs = rng.integers(0, 256, size=(n, msg_len), dtype=np.uint8)
    pks, sigs = engine.keygen_sign_many(sks, make_scalars(rng, n), msgs)
    return sigs, pks, msgs


def coeffs32(rng, n):
    c = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    c[:, 31] &= 0x3F
    return c


def corrupt(rng, sigs, pks, msgs, lanes):
    """one corruption of every class of tests/test_gpu_screened.py::corrupt, cycling over `lanes`"""
    kinds = ["e_bit", "msg_bit", "sort_bit", "swap_key", "noncanon_pk", "e_ge_q", "pk_off_curve", "x_changed", "flag_byte"]
    n = sigs.shape[0]
    for k, i in enumerate(lanes):
        kind = kinds[k % len(kinds)]
        if kind == "e_bit":
            sigs[i, 49] ^= 1
        elif kind == "msg_bit":
            msgs[i, rng.integers(0, msgs.shape[1])] ^= 0x10
        elif kind == "sort_bit":
            sigs[i, 48] ^= 0x40
        elif kind == "swap_key":
            pks[i] = pks[(i + 1) % n]
        elif kind == "noncanon_pk":
            pks[i, 0:8] = 0xFF
        elif kind == "e_ge_q":
            sigs[i, 49:81] = 0xFF
        elif kind == "pk_off_curve":
            pks[i, 48] ^= 1
        elif kind == "x_changed":
            sigs[i, 0] ^= 1
        else:
            sigs[i, 48] |= 0x01
    return [kinds[k % len(kinds)] for k in range(len(lanes))]


def dev(*arrays):
    import torch
    out = [torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0") for a in arrays]
    torch.cuda.synchronize()
    return out


def screened_device(engine, sigs, pks, msgs, coeffs=None, pk_inf=None, **fl):
    import torch
    n = sigs.shape[0]
    ds, dp, dm = dev(sigs, pks, msgs)
    dc = dev(coeffs)[0] if coeffs is not None else None
    di = dev(pk_inf)[0] if pk_inf is not None else None
    st = torch.full((n,), 255, dtype=torch.uint8, device="cuda:0")
    nf = torch.full((1,), -1, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    stats = engine.verify_many_screened_device(ds.data_ptr(), dp.data_ptr(), dm.data_ptr(), n, msgs.shape[1],
                                               dc.data_ptr() if dc is not None else 0, 32, st.data_ptr(), nf.data_ptr(),
                                               d_pk_inf=di.data_ptr() if di is not None else 0, **fl)
    engine.sync()
    return st.cpu().numpy(), int(nf.item()), stats


def assert_matches(engine, sigs, pks, msgs, fl, coeffs=None, pk_inf=None, form="host", want=None):
    """one call against ssa_verify_many on the same inputs and flags -> (status, stats)"""
    if want is None:
        want = engine.verify_many(sigs, pks, msgs, pk_inf=pk_inf, **fl)
    w, wnf = want
    assert wnf == int((w != 0).sum())
    if form == "host":
        st, nf, stats = engine.verify_many_screened(sigs, pks, msgs, coeffs=coeffs, pk_inf=pk_inf, **fl)
    else:
        st, nf, stats = screened_device(engine, sigs, pks, msgs, coeffs=coeffs, pk_inf=pk_inf, **fl)
    bad = np.nonzero(st != w)[0]
    assert bad.size == 0, (fl, form, bad[:10], st[bad[:10]], w[bad[:10]])
    assert nf == wnf, (fl, form, nf, wnf)
    return st, [int(v) for v in stats]


@pytest.mark.parametrize("n", [5000, 1 << 16, 1 << 20])
@pytest.mark.parametrize("u_of", ["1", "7", "n/16", "n"])
def test_honest_batches_are_accepted_by_the_screen_alone(engine, n, u_of):
    u = {"1": 1, "7": 7, "n/16": n // 16, "n": n}[u_of]
    rng = np.random.default_rng(11100 + n % 1000 + u % 97)
    sigs, pks, msgs = honest(engine, rng, n, u)
    for fl in NEW_SETTINGS:
        want = engine.verify_many(sigs, pks, msgs, **fl)
        for co, form in ((coeffs32(rng, n), "host"), (None, "device")):
            st, stats = assert_matches(engine, sigs, pks, msgs, fl, coeffs=co, form=form, want=want)
            assert (st == 0).all()
            assert stats[0] == u and stats[2] == 0 and stats[3] == 0 and stats[4] == 0, (fl, form, stats)
            assert stats[5] == 1 and stats[6] == 0 and stats[7] == 0, (fl, form, stats)


def special_key_lanes(rng, count, with_t2):
    """`count` signatures made for ONE key sk G (+ T2, a point of order 2, when with_t2): e = r - sk h, so the exact
    check's error term is [h] T2 -- without the subgroup check the lane verifies exactly when h is even"""
    import pymodel as m
    g = m.default_params().generator()
    sk = 0x1234567 + 2 * int(rng.integers(1, 1 << 30))
    pk = m.pt_mul(sk, g)
    if with_t2:
        pk = m.pt_add(pk, m.SMALL_ORDER_POINTS[2])
    pkb = np.frombuffer(m.fp6_to_bytes48(pk[0]) + m.fp6_to_bytes48(pk[1]), np.uint8)
    sigs, msgs = [], []
    for j in range(count):
        r = 0x7654321 + 2 * j
        rp = m.pt_mul(r, g)
        msg = rng.integers(0, 256, 80, dtype=np.uint8).tobytes()
        h = m.scalar_from_digest(m.hash_message(rp[0], pk, msg))
        e = (r - sk * h) % Q
        sigs.append(np.frombuffer(m.pt_compress(rp) + e.to_bytes(32, "little"), np.uint8))
        msgs.append(np.frombuffer(msg, np.uint8))
    return pkb, np.array(sigs), np.array(msgs)


def spoiled_batch(engine, rng, n=20000, u=50):
    """every class of bad lane on keys that repeat, lanes at segment edges, and the special keys"""
    import pymodel as m
    import schnorr_sig_amd as ssa
    sigs, pks, msgs = honest(engine, rng, n, u)
    inf = np.zeros(n, np.uint8)
    seg = ssa.debug_screen_plan(n)["segment_lanes"]
    edges = [0, seg - 1, seg, 2 * seg - 1, 5 * seg, n - 1]
    lanes = sorted(set(edges + [255, 256] + list(rng.choice(n, 48, replace=False))))
    kinds = corrupt(rng, sigs, pks, msgs, lanes)
    free = np.setdiff1d(np.arange(n), np.array(lanes + [(i + 1) % n for i in lanes]))
    rng.shuffle(free)
    g = {}
    # a key P + T2 on 40 lanes: four with signatures made for it, the others with someone else's
    t2 = free[:40]
    pkb, s4, m4 = special_key_lanes(rng, 4, True)
    pks[t2] = pkb
    sigs[t2[:4]], msgs[t2[:4]] = s4, m4
    g["p_plus_t2"] = t2
    # the small-order fixture point itself as a key (order 2)
    so = free[40:60]
    t2p = m.SMALL_ORDER_POINTS[2]
    pks[so] = np.frombuffer(m.fp6_to_bytes48(t2p[0]) + m.fp6_to_bytes48(t2p[1]), np.uint8)
    g["small_order"] = so
    # identity keys via pk_inf: e = r and R = [r]G verifies (the key contributes nothing); the last one is wrong
    kl = free[60:66]
    r = make_scalars(rng, kl.size)
    rp, _ = engine.keygen_sign_many(r, r, msgs[kl])
    rc, _ = engine.compress_many(rp)
    pks[kl] = 0
    inf[kl] = 1
    sigs[kl, :49] = rc
    sigs[kl, 49:] = r
    sigs[kl[-1], 49] ^= 2
    g["identity"] = kl
    # a bad key AND a malformed signature: the key decides (src/signature.rs:182-186)
    bb = free[66:72]
    pks[bb[:2]] = pkb                    # outside the subgroup + e >= q
    sigs[bb[:2], 49:81] = 0xFF
    pks[bb[2:4], 0:8] = 0xFF             # non-canonical key + non-canonical x
    sigs[bb[2:4], 0:8] = 0xFF
    pks[bb[4:6]] = pkb                   # outside the subgroup + undecodable flag byte
    sigs[bb[4:6], 48] |= 0x03
    g["both_bad"] = bb
    # a non-canonical key on 100 lanes
    nc = free[72:172]
    pks[nc] = pks[nc[0]]
    pks[nc, 0:8] = 0xFF
    g["noncanon"] = nc
    touched = np.unique(np.concatenate([np.array(lanes), t2, so, kl, bb, nc]))
    return (sigs, pks, msgs, inf), touched, g, dict(zip(lanes, kinds))


def test_every_class_of_bad_lane_gets_the_status_of_verify_many(engine, oracle):
    rng = np.random.default_rng(11201)
    (sigs, pks, msgs, inf), touched, g, kinds = spoiled_batch(engine, rng)
    n = sigs.shape[0]
    samp = np.unique(np.concatenate([touched, np.arange(0, n, 41)]))
    co = coeffs32(rng, n)
    co2 = co.copy()
    co2[g["p_plus_t2"], 0] ^= 1          # the other parity on every lane that holds the key P + T2
    co2[g["small_order"], 0] ^= 1
    for fl in ALL_SETTINGS:
        want = engine.verify_many(sigs, pks, msgs, pk_inf=inf, **fl)
        vecs = []
        runs = ((co, "host"), (co2, "device"), (None, "host"))
        if fl is F:
            # verify_batch semantics let the key P + T2 into the sums: the documented 1/l case of section 13.  The lanes
            # whose signatures were made for that key (error term [h]T2) get coefficients with s h mod q odd, which
            # report them; library-drawn coefficients would miss each with probability 1/2 and are not used here
            import pymodel as m
            t4 = g["p_plus_t2"][:4]
            dig = engine.hash_message_many(sigs[t4], pks[t4], msgs[t4])
            cf = co.copy()
            for j, i in enumerate(t4):
                h = m.scalar_from_digest(bytes(dig[j]))
                while True:
                    s = int.from_bytes(rng.bytes(32), "little") % Q
                    if (s * h % Q) & 1:
                        break
                cf[i] = np.frombuffer(s.to_bytes(32, "little"), np.uint8)
            runs = ((cf, "host"), (cf, "device"))
        for c, form in runs:
            st, stats = assert_matches(engine, sigs, pks, msgs, fl, coeffs=c, pk_inf=inf, form=form, want=want)
            vecs.append(st)
        st = vecs[0]
        wo = oracle.verify_many(sigs[samp], pks[samp], msgs[samp], pk_inf=inf[samp], **fl)
        bad = np.nonzero(st[samp] != wo)[0]
        assert bad.size == 0, (fl, samp[bad[:10]], st[samp][bad[:10]], wo[bad[:10]])
        if fl["check_torsion"]:
            # never in a sum: status 1 whatever the parity of the lane's coefficient
            assert all((v[g["p_plus_t2"]] == 1).all() and (v[g["small_order"]] == 1).all() for v in vecs)
            assert (st[g["both_bad"][:2]] == 1).all() and (st[g["both_bad"][4:]] == 1).all()
        assert (st[g["both_bad"][2:4]] == 3).all() and (st[g["noncanon"]] == 3).all()
        assert (st[g["identity"][:-1]] == 0).all() and st[g["identity"][-1]] == 2
        for i, kind in kinds.items():
            if kind in ("e_bit", "msg_bit"):
                assert st[i] == 2, (fl, i, kind)
            elif kind in ("noncanon_pk", "pk_off_curve", "e_ge_q"):
                assert st[i] == 3, (fl, i, kind)
            elif kind in ("sort_bit", "flag_byte"):
                assert st[i] == ((2 if kind == "sort_bit" else 3) if fl["sig_flag_byte"] else 0), (fl, i, kind)


def test_flag_byte_ignored_wrong_sort_bit_and_undecodable_byte_are_accepted(engine):
    """Signature::verify ignores byte 48.  A valid signature with its sort bit flipped enters its segment as -R: the
    segment fails and the re-check accepts the lane.  A byte that does not decode gives the screen no R: the lane is
    left out of the sums and re-checked, and its segment passes."""
    rng = np.random.default_rng(11251)
    n = 20000
    sigs, pks, msgs = honest(engine, rng, n, 30)
    import schnorr_sig_amd as ssa
    seg = ssa.debug_screen_plan(n)["segment_lanes"]
    for fl in (T, NONE):
        for kind, lane in (("sort", 3 * seg + 5), ("undecodable", 7 * seg + 9)):
            s2 = sigs.copy()
            if kind == "sort":
                s2[lane, 48] ^= 0x40
            else:
                s2[lane, 48] |= 0x21
            st, stats = assert_matches(engine, s2, pks, msgs, fl, coeffs=coeffs32(rng, n))
            assert (st == 0).all()
            if kind == "sort":
                assert stats[2] == 1 and stats[4] == 0 and stats[3] == seg, (fl, stats)
            else:
                assert stats[2] == 0 and stats[4] == 1 and stats[3] == 1, (fl, stats)


def test_unscreenable_lanes_do_not_fail_their_segment(engine):
    rng = np.random.default_rng(11301)
    n = 20000
    sigs, pks, msgs = honest(engine, rng, n, 40)
    holders = np.nonzero((pks == pks[123]).all(axis=1))[0]
    assert 100 < holders.size < n
    pks[holders, 0:8] = 0xFF                                      # ONE malformed key
    for fl in NEW_SETTINGS:
        for form in ("host", "device"):
            st, stats = assert_matches(engine, sigs, pks, msgs, fl, coeffs=coeffs32(rng, n), form=form)
            assert (st[holders] == 3).all() and (np.delete(st, holders) == 0).all()
            assert stats[2] == 0 and stats[3] == holders.size and stats[4] == holders.size, (fl, form, stats)
            assert stats[0] == 40 and stats[6] == 0


def test_small_order_part_of_r_is_caught_exactly_when_its_coefficient_is_odd(engine, oracle):
    """The one error the subgroup check on the keys leaves to the 1/l case.  Lane i: R = [r]G + T2 (T2 of order 2),
    e = r - sk h with h = hash_message(R.x, P, m), P = [sk]G in the prime-order subgroup.  The exact check computes
    [h]P + [e]G = [r]G, whose x is not R.x: status 2.  In its segment's sum the lane's term is
        s_i R_i - (s_i h_i) P_i - (s_i e_i) G = s_i ([r]G + T2) - [s_i (h_i sk + e_i)]G = [s_i] T2
    (the prime-order parts cancel mod q).  R_i is multiplied by the coefficient itself, s_i reduced mod q (a 32-byte
    coefficient below q is its own residue), through its digits -- not by a product reduced mod q as on the key side --
    so [s_i]T2 = T2 when s_i is odd and O when s_i is even: the lane is reported (2) exactly when s_i is odd, and
    accepted (0) when s_i is even."""
    import pymodel as m
    rng = np.random.default_rng(11401)
    n = 8192
    sigs, pks, msgs = honest(engine, rng, n, 16)
    g = m.default_params().generator()
    sk, r = 0x2345671 + 2 * int(rng.integers(1, 1 << 30)), 0x6543217
    pk = m.pt_mul(sk, g)
    rp = m.pt_add(m.pt_mul(r, g), m.SMALL_ORDER_POINTS[2])
    msg = rng.integers(0, 256, 80, dtype=np.uint8).tobytes()
    h = m.scalar_from_digest(m.hash_message(rp[0], pk, msg))
    e = (r - sk * h) % Q
    i = 5000
    sigs[i] = np.frombuffer(m.pt_compress(rp) + e.to_bytes(32, "little"), np.uint8)
    pks[i] = np.frombuffer(m.fp6_to_bytes48(pk[0]) + m.fp6_to_bytes48(pk[1]), np.uint8)
    msgs[i] = np.frombuffer(msg, np.uint8)
    co = coeffs32(rng, n)
    for fl in (T, TF):
        want, _ = engine.verify_many(sigs, pks, msgs, **fl)
        assert want[i] == 2 and (np.delete(want, i) == 0).all()
        assert oracle.verify_many(sigs[i:i + 1], pks[i:i + 1], msgs[i:i + 1], **fl)[0] == 2
        for parity, expect in ((1, 2), (0, 0), (1, 2), (0, 0)):
            s = (int.from_bytes(rng.bytes(32), "little") % Q) & ~1 | parity
            co[i] = np.frombuffer(s.to_bytes(32, "little"), np.uint8)
            st, nf, stats = engine.verify_many_screened(sigs, pks, msgs, coeffs=co, **fl)
            assert st[i] == expect and nf == (1 if expect else 0) and (np.delete(st, i) == 0).all(), (fl, parity, s)
            assert int(stats[2]) == (1 if expect else 0)


@pytest.mark.parametrize("k", [2, 16, 256])
def test_forced_segment_counts_give_identical_vectors(k):
    import schnorr_sig_amd as ssa
    eng = ssa.Engine(0)
    try:
        rng = np.random.default_rng(11501)
        (sigs, pks, msgs, inf), _, _, _ = spoiled_batch(eng, rng)
        co = coeffs32(rng, sigs.shape[0])
        for fl in NEW_SETTINGS:
            base, _, _ = eng.verify_many_screened(sigs, pks, msgs, coeffs=co, pk_inf=inf, **fl)
            eng.debug_screen_segments(k)
            st, stats = assert_matches(eng, sigs, pks, msgs, fl, coeffs=co, pk_inf=inf)
            eng.debug_screen_segments(0)
            assert (st == base).all() and stats[1] <= k
    finally:
        eng.close()


_CHILD = r"""
import json, os, sys
sys.path.insert(0, %(root)r)
import numpy as np
import torch
import schnorr_sig_amd as ssa
rng = np.random.default_rng(11601)
n, u = %(n)d, 25
e = ssa.Engine(0)
def sc(k):
    v = rng.integers(0, 256, size=(k, 32), dtype=np.uint8); v[:, 31] &= 0x3f; v[:, 0] |= 1
    return v
idx = rng.integers(0, u, size=n); idx[:u] = np.arange(u)
m = rng.integers(0, 256, size=(n, 80), dtype=np.uint8)
pk, sg = e.keygen_sign_many(sc(u)[idx], sc(n), m)
bad = [0, 4999, 5000, 6123, 9999, 10000, n - 1]
for i in bad:
    sg[i, 50] ^= 4
pk[7000, 0:8] = 0xff
pk[10500, 0:8] = 0xff
co = rng.integers(0, 256, size=(n, 32), dtype=np.uint8); co[:, 31] &= 0x3f
out = {"info": e.info()["lane_slice"], "cases": []}
dev = torch.device("cuda", 0)
for fl in (dict(check_torsion=True, sig_flag_byte=False), dict(check_torsion=True, sig_flag_byte=True),
           dict(check_torsion=False, sig_flag_byte=False)):
    st, nf, stats = e.verify_many_screened(sg, pk, m, coeffs=co, **fl)
    want, wnf = e.verify_many(sg, pk, m, **fl)
    ds, dp, dm, dc = (torch.from_numpy(a).to(dev) for a in (sg, pk, m, co))
    dst = torch.full((n,), 255, dtype=torch.uint8, device=dev)
    dnf = torch.zeros(1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    dstats = e.verify_many_screened_device(ds.data_ptr(), dp.data_ptr(), dm.data_ptr(), n, 80, dc.data_ptr(), 32,
                                           dst.data_ptr(), dnf.data_ptr(), **fl)
    e.sync()
    out["cases"].append({"equal": bool((st == want).all()), "dev_equal": bool((dst.cpu().numpy() == want).all()),
                         "nf": [int(nf), int(wnf), int(dnf.item())], "bad": [int(st[i]) for i in bad + [7000, 10500]],
                         "stats": [int(v) for v in stats], "dstats": [int(v) for v in dstats]})
print("RESULT " + json.dumps(out))
e.close()
"""


@pytest.mark.parametrize("n", [12000, 14500])
def test_more_than_one_slice_host_and_device_forms(n):
    """SSA_LANE_SLICE = 5000, host and device forms (the host form alternates slices between the context and its twin).
    n = 12000: slices of 5000, 5000 and 2000 lanes -- a last slice below the small-batch bound, which takes the exact
    path with the caller's flags.  n = 14500: slices of 5000, 5000 and 4500 -- a ragged last slice that IS screened,
    with its own plan (fewer blocks, a ragged last segment of its own: 4 segments of 1280 lanes, the bad lanes in the
    first and the last, 1940 lanes re-checked, fewer than half) and its own distinct keys.  A bad lane on either side of
    every slice boundary and at both ends; one malformed key in the second slice and one in the last."""
    env = dict(os.environ)
    env["SSA_LANE_SLICE"] = "5000"
    r = subprocess.run([sys.executable, "-c", _CHILD % {"root": ROOT, "n": n}], env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    assert out["info"] == 5000
    # slices screened, slices on the exact path, distinct keys over the screened slices (25 honest keys each, plus the
    # malformed one where it lies in a screened slice), lanes that could not be screened
    expect = {12000: [2, 1, 25 + 26, 1], 14500: [3, 0, 25 + 26 + 26, 2]}[n]
    for c in out["cases"]:
        assert c["equal"] and c["dev_equal"], c
        assert c["nf"] == [9, 9, 9] and c["bad"] == [2] * 7 + [3, 3], c
        for s in (c["stats"], c["dstats"]):
            assert [s[5], s[6], s[0], s[4]] == expect and s[7] == 0, c


def test_full_occupancy_is_deterministic(engine):
    rng = np.random.default_rng(11701)
    n, u = 1 << 20, 1000
    sigs, pks, msgs = honest(engine, rng, n, u)
    corrupt(rng, sigs, pks, msgs, list(range(11, n, 40009)))
    co = coeffs32(rng, n)
    want = engine.verify_many(sigs, pks, msgs, **T)
    runs = [assert_matches(engine, sigs, pks, msgs, T, coeffs=co, form="device", want=want) for _ in range(2)]
    assert (runs[0][0] == runs[1][0]).all() and runs[0][1] == runs[1][1]
    assert runs[0][1][0] >= u and runs[0][1][5] == 1 and runs[0][1][6] == 0


def test_workspaces_do_not_grow_from_the_second_call_on():
    import schnorr_sig_amd as ssa
    eng = ssa.Engine(0)
    try:
        rng = np.random.default_rng(11801)
        n = 30000
        sigs, pks, msgs = honest(eng, rng, n, 500)
        corrupt(rng, sigs, pks, msgs, list(range(5, n, 3001)))
        sizes = []
        for k in range(6):
            eng.verify_many_screened(sigs, pks, msgs, **T)
            screened_device(eng, sigs, pks, msgs, **T)
            sizes.append(eng.info()["workspace_bytes"])
        assert sizes[0] > 0 and sizes[5] == sizes[1], sizes
    finally:
        eng.close()


def test_more_than_half_the_lanes_bad_takes_the_whole_slice_exact_path(engine):
    rng = np.random.default_rng(11901)
    n = 1 << 16
    sigs, pks, msgs = honest(engine, rng, n, 300)
    lanes = list(range(17, n, 1024))
    sigs[lanes, 49] ^= 1                                          # a wrong e in every segment: every segment fails
    for fl in NEW_SETTINGS:
        for form in ("host", "device"):
            st, stats = assert_matches(engine, sigs, pks, msgs, fl, coeffs=coeffs32(rng, n), form=form)
            assert (st[lanes] == 2).all() and (st != 0).sum() == len(lanes)
            assert stats[6] == 1 and stats[5] == 1 and stats[2] == stats[1] and stats[3] == n, (fl, form, stats)
    # and with most keys malformed: the lanes cannot be screened, no segment fails, the same path
    s2, p2, m2 = honest(engine, rng, n, 300)
    p2[: (n * 3) // 4, 0:8] = 0xFF
    st, stats = assert_matches(engine, s2, p2, m2, T, coeffs=coeffs32(rng, n))
    assert stats[6] == 1 and stats[2] == 0 and stats[4] == (n * 3) // 4 and (st[: (n * 3) // 4] == 3).all()


def test_flag_byte_alone_is_the_screened_form(engine):
    rng = np.random.default_rng(12001)
    (sigs, pks, msgs, inf), _, _, _ = spoiled_batch(engine, rng)
    co = coeffs32(rng, sigs.shape[0])
    st, nf, stats = engine.verify_many_screened(sigs, pks, msgs, coeffs=co, pk_inf=inf, **F)
    want, wnf = engine.verify_batch_screened(sigs, pks, msgs, coeffs=co, pk_inf=inf)
    assert st.tobytes() == want.tobytes() and nf == wnf
    dst, dnf, _ = screened_device(engine, sigs, pks, msgs, coeffs=co, pk_inf=inf, **F)
    assert dst.tobytes() == want.tobytes() and dnf == wnf


def test_module_level_verify_many_screened_over_objects(engine):
    import schnorr_sig_amd as ssa
    rng = np.random.default_rng(12101)
    n, u = 12, 3
    sigs, pks, msgs = honest(engine, rng, n, u)
    sigs[4, 50] ^= 1
    pks[9, 0:8] = 0xFF
    res = ssa.verify_many_screened([ssa.Signature(s.tobytes()) for s in sigs], [ssa.PublicKey(p.tobytes()) for p in pks],
                                   [m.tobytes() for m in msgs], engine=engine)
    assert len(res) == n
    for i, r in enumerate(res):
        if i == 4:
            assert isinstance(r, ssa.SignatureError) and r.kind == ssa.SignatureError.InvalidSignature
        elif i == 9:
            assert isinstance(r, ssa.MalformedInput)
        else:
            assert r is None
