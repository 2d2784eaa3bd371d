"""Key dedup (ssa_verify_many_dedup): every status vector is compared, lane for lane, with
ssa_verify_many on the same inputs and flags, and the statuses of the corrupted lanes with the CPU oracle.  The two flag
settings are SSA_FLAG_CHECK_TORSION and SSA_FLAG_SIG_FLAG_BYTE without it."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

Q = 0x7AF2599B3B3F22D0563FBF0F990A37B5327AA72330157722D443623EAED4ACCF
FLAG_SETTINGS = [dict(check_torsion=True, sig_flag_byte=False), dict(check_torsion=False, sig_flag_byte=True)]


def make_scalars(rng, n):
    s = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    s[:, 31] &= 0x3F
    s[:, 0] |= 1
    return s


def key_choice(rng, n, u):
    """which of u keys each of n lanes holds: every key at least once, in random order"""
    idx = rng.integers(0, u, size=n)
    idx[:u] = np.arange(u)
    rng.shuffle(idx)
    return idx


def honest(engine, rng, n, u, msg_len=80):
    """n honest signatures by u distinct signers"""
    sks = make_scalars(rng, u)[key_choice(rng, n, u)]
    nonces = make_scalars(rng, n)
    msgs = rng.integers(0, 256, size=(n, msg_len), dtype=np.uint8)
    pks, sigs = engine.keygen_sign_many(sks, nonces, msgs)
    return sigs, pks, msgs


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
    return kinds


def rows97(pks, inf=None):
    """the 97 bytes two lanes must share to share a key: the key bytes and the flag as a boolean"""
    n = pks.shape[0]
    flag = np.zeros((n, 1), np.uint8) if inf is None else (np.asarray(inf) != 0).astype(np.uint8).reshape(n, 1)
    return np.ascontiguousarray(np.concatenate([pks.reshape(n, 96), flag], axis=1))


def distinct_rows(rows):
    """(number of distinct rows, class number per row)"""
    v = rows.view(np.dtype((np.void, rows.shape[1]))).reshape(-1)
    uniq, inv = np.unique(v, return_inverse=True)
    return uniq.size, inv.reshape(-1)


def same_classes(a, b):
    """two labelings of the lanes describe the same partition"""
    ua, ub = np.unique(a).size, np.unique(b).size
    pairs = np.unique(a.astype(np.int64) * (int(b.max()) + 1) + b.astype(np.int64)).size
    return ua == ub == pairs


def dev(*arrays):
    import torch
    out = [torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0") for a in arrays]
    torch.cuda.synchronize()
    return out


def dedup_device(engine, sigs, pks, msgs, pk_inf=None, mode=None, **flags):
    import torch
    n = sigs.shape[0]
    ds, dp, dm = dev(sigs, pks, msgs)
    di = dev(pk_inf)[0] if pk_inf is not None else None
    st = torch.full((n,), 255, dtype=torch.uint8, device="cuda:0")
    nf = torch.full((1,), -1, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    stats = engine.verify_many_dedup_device(ds.data_ptr(), dp.data_ptr(), dm.data_ptr(), n, msgs.shape[1], st.data_ptr(),
                                            nf.data_ptr(), d_pk_inf=di.data_ptr() if di is not None else 0, mode=mode,
                                            **flags)
    engine.sync()
    return st.cpu().numpy(), int(nf.item()), stats


def debug_dedup(engine, pks, pk_inf=None):
    import torch
    n = pks.shape[0]
    dp = dev(pks)[0]
    di = dev(pk_inf)[0] if pk_inf is not None else None
    idx = torch.full((n,), -1, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    u, hits = engine.debug_dedup_device(dp.data_ptr(), n, d_key_idx=idx.data_ptr(),
                                        d_pk_inf=di.data_ptr() if di is not None else 0)
    return u, hits, idx.cpu().numpy().astype(np.int64)


def assert_matches(engine, sigs, pks, msgs, pk_inf=None, mode=None, forms=("host", "device"), u=None):
    """both flag settings, the host and the device form, against ssa_verify_many; returns the vectors of the last form"""
    out = []
    for fl in FLAG_SETTINGS:
        want, wnf = engine.verify_many(sigs, pks, msgs, pk_inf=pk_inf, mode=mode, **fl)
        assert wnf == int((want != 0).sum())
        for form in forms:
            if form == "host":
                st, nf, stats = engine.verify_many_dedup(sigs, pks, msgs, pk_inf=pk_inf, mode=mode, **fl)
            else:
                st, nf, stats = dedup_device(engine, sigs, pks, msgs, pk_inf=pk_inf, mode=mode, **fl)
            bad = np.nonzero(st != want)[0]
            assert bad.size == 0, (fl, form, bad[:10], st[bad[:10]], want[bad[:10]])
            assert nf == wnf, (fl, form, nf, wnf)
            if u is not None:
                assert int(stats[0]) == u, (fl, form, stats)
            assert int(stats[1]) + int(stats[2]) >= 1 and int(stats[3]) == 0, (fl, form, stats)
        out.append(st)
    return out


@pytest.mark.parametrize("n", [4096, 1 << 16, 1 << 20])
@pytest.mark.parametrize("u_of", ["1", "7", "n/16", "n"])
def test_honest_batches_match_verify_many(engine, n, u_of):
    u = {"1": 1, "7": 7, "n/16": n // 16, "n": n}[u_of]
    rng = np.random.default_rng(10100 + n % 1000 + u % 97)
    sigs, pks, msgs = honest(engine, rng, n, u)
    assert distinct_rows(rows97(pks))[0] == u
    for st in assert_matches(engine, sigs, pks, msgs, u=u):
        assert (st == 0).all()
    if n == 4096:       # the same batch through the lane kernels (by default it goes to the cooperative kernel, unchanged)
        assert_matches(engine, sigs, pks, msgs, mode="lane", u=u)


def test_key_index_classes_are_the_byte_classes(engine):
    rng = np.random.default_rng(10201)
    for n, u in ((1 << 16, 4096), (1 << 20, 1000), (1 << 20, 1 << 18), (3001, 3001), (1, 1)):
        _, pks, _ = honest(engine, rng, n, u)
        inf = (rng.integers(0, 8, size=n) == 0).astype(np.uint8) * rng.integers(1, 256, size=n).astype(np.uint8)
        for flags in (None, inf):
            want_u, inv = distinct_rows(rows97(pks, flags))
            got_u, hits, idx = debug_dedup(engine, pks, flags)
            assert got_u == want_u and hits == 0, (n, u, got_u, want_u, hits)
            assert idx.min() == 0 and idx.max() == got_u - 1
            assert same_classes(inv, idx), (n, u)


def small_order_key_lanes(engine, rng, count):
    """`count` honest-looking signatures under ONE key P + T2 (T2 of order 2), as tests/test_gpu_screened.py builds it:
    e = r - sk h, so the check's error term is [h] T2 -- the lane verifies without the subgroup check exactly when h is even"""
    import pymodel as m
    g = m.default_params().generator()
    t2 = m.SMALL_ORDER_POINTS[2]
    sk = 0x1234567 + 2 * int(rng.integers(1, 1 << 30))
    pk = m.pt_add(m.pt_mul(sk, g), t2)
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
    """every class of bad lane on keys that repeat; returns the batch, the lanes touched and the lanes of each special key"""
    sigs, pks, msgs = honest(engine, rng, n, u)
    inf = np.zeros(n, np.uint8)
    lanes = sorted(set([0, 255, 256, n - 1] + list(rng.choice(n, 60, replace=False))))
    corrupt(rng, sigs, pks, msgs, lanes)
    free = np.setdiff1d(np.arange(n), lanes)
    rng.shuffle(free)
    groups = {}
    # a key outside the prime subgroup on 300 lanes: six with signatures made for it, the others with someone else's
    t2 = free[:300]
    pkb, s6, m6 = small_order_key_lanes(engine, rng, 6)
    pks[t2] = pkb
    sigs[t2[:6]], msgs[t2[:6]] = s6, m6
    groups["small_order"] = t2
    # a non-canonical key and an off-curve key, each on 200 lanes
    nc = free[300:500]
    pks[nc] = pks[nc[0]]
    pks[nc, 0:8] = 0xFF
    groups["noncanon"] = nc
    oc = free[500:700]
    pks[oc] = pks[oc[0]]
    pks[oc, 48] ^= 1
    groups["off_curve"] = oc
    # equal key bytes, different pk_inf (any non-zero byte means the identity)
    pi = free[700:740]
    pks[pi] = pks[pi[0]]
    inf[pi[::2]] = rng.integers(1, 256, size=pi[::2].size).astype(np.uint8)
    groups["inf_pair"] = pi
    # near-equal keys: a valid key and copies that differ in one byte of y, or in one limb only
    ne = free[740:800]
    pks[ne] = pks[ne[0]]
    for j, i in enumerate(ne[1:25]):
        pks[i, 48 + 2 * j] ^= 1 << (j % 8)
    for j, i in enumerate(ne[25:37]):
        pks[i, 8 * j + 3] ^= 0x20
    groups["near_equal"] = ne
    touched = np.unique(np.concatenate([np.array(lanes), t2, nc, oc, pi, ne]))
    return (sigs, pks, msgs, inf), touched, groups


def test_every_class_of_bad_lane_on_repeated_keys(engine, oracle):
    rng = np.random.default_rng(10301)
    (sigs, pks, msgs, inf), touched, groups = spoiled_batch(engine, rng)
    n = sigs.shape[0]
    with_t, without_t = assert_matches(engine, sigs, pks, msgs, pk_inf=inf)
    # the touched lanes and every 37th lane against the CPU oracle, under both flag settings
    samp = np.unique(np.concatenate([touched, np.arange(0, n, 37)]))
    for st, fl in zip((with_t, without_t), FLAG_SETTINGS):
        want = oracle.verify_many(sigs[samp], pks[samp], msgs[samp], pk_inf=inf[samp], **fl)
        bad = np.nonzero(st[samp] != want)[0]
        assert bad.size == 0, (fl, samp[bad[:10]], st[samp][bad[:10]], want[bad[:10]])
    assert (with_t[groups["small_order"]] == 1).all()
    assert set(int(v) for v in without_t[groups["small_order"][:6]]) <= {0, 2}       # h even / h odd
    assert (without_t[groups["small_order"][6:]] == 2).all()
    assert (with_t[groups["noncanon"]] == 3).all() and (without_t[groups["noncanon"]] == 3).all()
    assert (with_t[groups["off_curve"]] == 3).all() and (without_t[groups["off_curve"]] == 3).all()
    ne = groups["near_equal"]
    assert with_t[ne[0]] == 0 and (with_t[ne[1:37]] == 3).all()                     # (the copies are off the curve)
    # the dedup itself: flags split equal bytes, near-equal keys are not merged
    want_u, inv = distinct_rows(rows97(pks, inf))
    got_u, hits, idx = debug_dedup(engine, pks, inf)
    assert got_u == want_u and hits == 0 and same_classes(inv, idx)
    pi = groups["inf_pair"]
    assert np.unique(idx[pi]).size == 2 and idx[pi[0]] != idx[pi[1]]
    assert np.unique(idx[ne]).size == 37
    # every statistic of the call
    st, nf, stats = engine.verify_many_dedup(sigs, pks, msgs, pk_inf=inf, check_torsion=True)
    assert [int(v) for v in stats] == [want_u, 1, 0, 0]


def test_forced_routes_give_identical_vectors():
    """one context of its own (the policy is per context): fallback, keyed route (on all-distinct keys too), probe
    bound 1"""
    import schnorr_sig_amd as ssa
    eng = ssa.Engine(0)
    try:
        rng = np.random.default_rng(10401)
        (sigs, pks, msgs, inf), _, _ = spoiled_batch(eng, rng)
        n = sigs.shape[0]
        u = distinct_rows(rows97(pks, inf))[0]
        base = assert_matches(eng, sigs, pks, msgs, pk_inf=inf, u=u)
        for ratio, route in ((0.0, (0, 1)), (2.0, (1, 0))):
            eng.debug_dedup_config(max_distinct_ratio=ratio)
            got = assert_matches(eng, sigs, pks, msgs, pk_inf=inf, u=u)
            assert all((g == b).all() for g, b in zip(got, base)), ratio
            for fl in FLAG_SETTINGS:
                _, _, stats = eng.verify_many_dedup(sigs, pks, msgs, pk_inf=inf, **fl)
                assert (int(stats[1]), int(stats[2])) == route, (ratio, fl, stats)
        # all-distinct keys on the keyed route (u tables = one per lane)
        s2, p2, m2 = honest(eng, rng, n, n)
        corrupt(rng, s2, p2, m2, list(range(5, n, 997)))
        eng.debug_dedup_config(max_distinct_ratio=2.0)
        assert_matches(eng, s2, p2, m2)
        _, _, stats = eng.verify_many_dedup(s2, p2, m2, check_torsion=True)
        assert int(stats[1]) == 1 and int(stats[0]) >= n - 30            # (swap_key lanes repeat a neighbour's key)
        # probe bound 1: a lane whose first slot is taken by another key becomes a key of its own
        n3 = 1 << 16
        s3, p3, m3 = honest(eng, rng, n3, n3 // 4)
        corrupt(rng, s3, p3, m3, list(range(3, n3, 1500)))
        eng.debug_dedup_config(max_distinct_ratio=2.0, probe_bound=0)
        want = [eng.verify_many(s3, p3, m3, **fl)[0] for fl in FLAG_SETTINGS]
        true_u = distinct_rows(rows97(p3))[0]
        eng.debug_dedup_config(max_distinct_ratio=2.0, probe_bound=1)
        for fl, w in zip(FLAG_SETTINGS, want):
            for call in (lambda: eng.verify_many_dedup(s3, p3, m3, **fl), lambda: dedup_device(eng, s3, p3, m3, **fl)):
                st, nf, stats = call()
                assert (st == w).all() and nf == int((w != 0).sum())
                # (a key whose first slot is taken has no representative in the table: every one of its lanes is a key)
                assert int(stats[3]) > 0 and true_u <= int(stats[0]) <= true_u + int(stats[3]) and int(stats[1]) == 1, stats
        eng.debug_dedup_config()
    finally:
        eng.close()


def test_full_occupancy_is_deterministic(engine):
    rng = np.random.default_rng(10501)
    n, u = 1 << 20, 1000
    sigs, pks, msgs = honest(engine, rng, n, u)
    corrupt(rng, sigs, pks, msgs, list(range(11, n, 40009)))
    runs = []
    for _ in range(2):
        st, nf, stats = dedup_device(engine, sigs, pks, msgs, check_torsion=True)
        got_u, hits, idx = debug_dedup(engine, pks)
        runs.append((st, nf, [int(v) for v in stats], got_u, idx))
    assert (runs[0][0] == runs[1][0]).all() and runs[0][1] == runs[1][1] and runs[0][2] == runs[1][2]
    assert runs[0][3] == runs[1][3] == distinct_rows(rows97(pks))[0]
    assert same_classes(runs[0][4], runs[1][4])
    want, wnf = engine.verify_many(sigs, pks, msgs, check_torsion=True)
    assert (runs[0][0] == want).all() and runs[0][1] == wnf
    assert runs[0][2][1:] == [1, 0, 0]


def test_more_than_one_slice_host_and_device_forms(engine):
    """2^20 + 5000 lanes: two slices, keys that repeat across the boundary; each slice finds its own distinct keys"""
    rng = np.random.default_rng(10601)
    n, u, cut = (1 << 20) + 5000, 1000, 1 << 20
    sigs, pks, msgs = honest(engine, rng, n, u)
    corrupt(rng, sigs, pks, msgs, [0, cut - 1, cut, cut + 1, n - 1] + list(range(7, n, 50021)))
    per_slice = distinct_rows(rows97(pks[:cut]))[0] + distinct_rows(rows97(pks[cut:]))[0]
    for fl in FLAG_SETTINGS:
        want, wnf = engine.verify_many(sigs, pks, msgs, **fl)
        # the host form chooses the kernels slice by slice, as ssa_verify_many does: its 5000-lane slice goes to the
        # cooperative kernel; the device form chooses once for the whole batch
        # (without the subgroup check every slice falls back: the measured policy)
        keyed = fl["check_torsion"]
        for call, routes in ((lambda: engine.verify_many_dedup(sigs, pks, msgs, **fl), [1, 1] if keyed else [0, 2]),
                             (lambda: dedup_device(engine, sigs, pks, msgs, **fl), [2, 0] if keyed else [0, 2])):
            st, nf, stats = call()
            bad = np.nonzero(st != want)[0]
            assert bad.size == 0 and nf == wnf, (fl, bad[:10])
            assert [int(v) for v in stats] == [per_slice] + routes + [0], (fl, stats)


def test_unaligned_device_keys(engine):
    """a key array that does not start on an 8-byte boundary is read byte by byte"""
    import torch
    rng = np.random.default_rng(10701)
    n, u = 20000, 300
    sigs, pks, msgs = honest(engine, rng, n, u)
    corrupt(rng, sigs, pks, msgs, list(range(2, n, 1111)))
    ds, dm = dev(sigs, msgs)
    raw = torch.zeros(n * 96 + 16, dtype=torch.uint8, device="cuda:0")
    raw[3:3 + n * 96] = torch.from_numpy(pks.reshape(-1)).to("cuda:0")
    st = torch.full((n,), 255, dtype=torch.uint8, device="cuda:0")
    nf = torch.full((1,), -1, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    assert (raw.data_ptr() + 3) % 8 != 0
    stats = engine.verify_many_dedup_device(ds.data_ptr(), raw.data_ptr() + 3, dm.data_ptr(), n, 80, st.data_ptr(),
                                            nf.data_ptr(), check_torsion=True)
    engine.sync()
    want, wnf = engine.verify_many(sigs, pks, msgs, check_torsion=True)
    assert (st.cpu().numpy() == want).all() and int(nf.item()) == wnf
    assert int(stats[0]) == distinct_rows(rows97(pks))[0] and int(stats[1]) == 1


def test_without_statistics_the_vectors_are_the_same(engine):
    """stats_out = NULL: the dedup is skipped where it cannot change the route"""
    import ctypes as C
    import schnorr_sig_amd as ssa
    rng = np.random.default_rng(10751)
    n = 20000
    sigs, pks, msgs = honest(engine, rng, n, 40)
    corrupt(rng, sigs, pks, msgs, list(range(1, n, 701)))
    for flags in (ssa.FLAG_CHECK_TORSION, ssa.FLAG_SIG_FLAG_BYTE):
        want, wnf = engine.verify_many(sigs, pks, msgs, check_torsion=bool(flags & 1), sig_flag_byte=bool(flags & 8))
        st = np.full(n, 255, np.uint8)
        nf = C.c_uint64(0)
        rc = ssa._lib.ssa_verify_many_dedup(engine._ctx, sigs.ctypes.data, pks.ctypes.data, None, msgs.ctypes.data, None, 80,
                                            80, n, flags, st.ctypes.data, C.byref(nf), None)
        assert rc == 0 and (st == want).all() and nf.value == wnf


def test_workspaces_do_not_grow_from_call_to_call():
    import schnorr_sig_amd as ssa
    eng = ssa.Engine(0)
    try:
        rng = np.random.default_rng(10801)
        sigs, pks, msgs = honest(eng, rng, 30000, 500)
        sizes = []
        for k in range(10):
            st, nf, _ = eng.verify_many_dedup(sigs, pks, msgs, check_torsion=True)
            dedup_device(eng, sigs, pks, msgs, check_torsion=True)
            assert nf == 0
            sizes.append(eng.info()["workspace_bytes"])
        assert sizes[0] > 0 and sizes[9] == sizes[0], sizes
    finally:
        eng.close()


def test_module_level_verify_many_over_objects(engine):
    import schnorr_sig_amd as ssa
    rng = np.random.default_rng(10901)
    n, u = 12, 3
    sigs, pks, msgs = honest(engine, rng, n, u)
    sigs[4, 50] ^= 1
    pks[9, 0:8] = 0xFF
    res = ssa.verify_many([ssa.Signature(s.tobytes()) for s in sigs], [ssa.PublicKey(p.tobytes()) for p in pks],
                          [m.tobytes() for m in msgs], engine=engine)
    assert len(res) == n
    for i, r in enumerate(res):
        if i == 4:
            assert isinstance(r, ssa.SignatureError) and r.kind == ssa.SignatureError.InvalidSignature
        elif i == 9:
            assert isinstance(r, ssa.MalformedInput)
        else:
            assert r is None
