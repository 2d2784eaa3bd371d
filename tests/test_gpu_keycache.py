"""Key cache (ssa_keycache_create, ssa_verify_many_cached).  Every status vector is compared lane
for lane with ssa_verify_many on the same inputs and flags (exact), byte for byte with ssa_verify_many_screened under
the same coefficients, stats[0..6] with that call's, and -- for the corrupted lanes and a sample of clean ones -- with
the CPU oracle.  Every batch is larger than SSA_MSM_SMALL_MAX (3072): below it the cache is never reached."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_screened_torsion import (NEW_SETTINGS, T, coeffs32, corrupt, dev, honest, make_scalars, spoiled_batch)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HITS, INSERTED, CLEARS, BYPASSED = 8, 9, 10, 11


def cached_device(engine, cache, sigs, pks, msgs, coeffs=None, pk_inf=None, **fl):
    import torch
    n = sigs.shape[0]
    ds, dp, dm = dev(sigs, pks, msgs)
    dc = dev(coeffs)[0] if coeffs is not None else None
    di = dev(pk_inf)[0] if pk_inf is not None else None
    st = torch.full((n,), 255, dtype=torch.uint8, device="cuda:0")
    nf = torch.full((1,), -1, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    stats = engine.verify_many_cached_device(cache, ds.data_ptr(), dp.data_ptr(), dm.data_ptr(), n, msgs.shape[1],
                                             dc.data_ptr() if dc is not None else 0, 32, st.data_ptr(), nf.data_ptr(),
                                             d_pk_inf=di.data_ptr() if di is not None else 0, **fl)
    engine.sync()
    return st.cpu().numpy(), int(nf.item()), stats


def reference(engine, sigs, pks, msgs, fl, coeffs, pk_inf=None):
    """what a cached call must return: ssa_verify_many's vector and count, ssa_verify_many_screened's bytes and stats"""
    w, wnf = engine.verify_many(sigs, pks, msgs, pk_inf=pk_inf, **fl)
    assert wnf == int((w != 0).sum())
    s, snf, sstats = engine.verify_many_screened(sigs, pks, msgs, coeffs=coeffs, pk_inf=pk_inf, **fl)
    assert s.tobytes() == w.tobytes() and snf == wnf
    return w, wnf, [int(v) for v in sstats]


def cached(engine, cache, sigs, pks, msgs, fl, coeffs, ref, pk_inf=None, form="host"):
    """one cached call against `ref` -> (status, stats)"""
    w, wnf, sstats = ref
    if form == "host":
        st, nf, stats = engine.verify_many_cached(cache, sigs, pks, msgs, coeffs=coeffs, pk_inf=pk_inf, **fl)
    else:
        st, nf, stats = cached_device(engine, cache, sigs, pks, msgs, coeffs=coeffs, pk_inf=pk_inf, **fl)
    stats = [int(v) for v in stats]
    bad = np.nonzero(st != w)[0]
    assert bad.size == 0, (fl, form, bad[:10], st[bad[:10]], w[bad[:10]])
    assert st.tobytes() == w.tobytes() and nf == wnf, (fl, form, nf, wnf)
    assert stats[:7] == sstats[:7], (fl, form, stats, sstats)
    assert stats[7] >= sstats[7]
    return st, stats


def build_launches(engine):
    return engine.read_timing("ssa_k_keyset_build")[1]


@pytest.mark.parametrize("n", [5000, 1 << 16, 1 << 20])
@pytest.mark.parametrize("u_of", ["1", "7", "n/16", "n"])
def test_cold_then_warm(engine, n, u_of):
    u = {"1": 1, "7": 7, "n/16": n // 16, "n": n}[u_of]
    rng = np.random.default_rng(16100 + n % 1000 + u % 97)
    sigs, pks, msgs = honest(engine, rng, n, u)
    co = coeffs32(rng, n)
    ref = reference(engine, sigs, pks, msgs, T, co)
    with engine.keycache_create(max(u, 64)) as cache:
        engine.enable_timing(True)
        try:
            build_launches(engine)                                  # drains the key
            st, stats = cached(engine, cache, sigs, pks, msgs, T, co, ref, form="device")
            assert (st == 0).all() and stats[3] == 0
            assert stats[INSERTED] == u and stats[HITS] == 0 and stats[0] == u, stats
            assert stats[CLEARS] == 0 and stats[BYPASSED] == 0 and stats[7] == 0, stats
            assert build_launches(engine) == 1
            assert cache.info()["held"] == u
            for form in ("device", "host"):
                st, stats = cached(engine, cache, sigs, pks, msgs, T, co, ref, form=form)
                assert (st == 0).all() and stats[3] == 0
                assert stats[HITS] == u and stats[INSERTED] == 0 and stats[0] == u, (form, stats)
                assert stats[CLEARS] == 0 and stats[BYPASSED] == 0 and stats[7] == 0, (form, stats)
            assert build_launches(engine) == 0, "a warm call launches no key check"
            assert engine.read_timing("keycache_lookup")[1] == 3 and engine.read_timing("keycache_map")[1] == 3
        finally:
            engine.enable_timing(False)
        assert cache.info()["held"] == u and cache.info()["clears"] == 0


def test_partly_warm(engine):
    rng = np.random.default_rng(16201)
    n, u = 20000, 400
    sks = make_scalars(rng, u + u // 2)
    from test_gpu_screened_torsion import key_choice

    def batch(keys):
        msgs = rng.integers(0, 256, size=(n, 80), dtype=np.uint8)
        pks, sigs = engine.keygen_sign_many(keys[key_choice(rng, n, keys.shape[0])], make_scalars(rng, n), msgs)
        return sigs, pks, msgs

    a = batch(sks[:u])
    b = batch(sks[u // 2:])                    # u keys: the second half of A's and u / 2 new ones
    with engine.keycache_create(1024) as cache:
        for fl in NEW_SETTINGS:
            cache.clear()
            co = coeffs32(rng, n)
            _, stats = cached(engine, cache, *a, fl, co, reference(engine, *a, fl, co))
            assert stats[HITS] == 0 and stats[INSERTED] == u
            _, stats = cached(engine, cache, *b, fl, co, reference(engine, *b, fl, co), form="device")
            assert stats[HITS] == u // 2 and stats[INSERTED] == u // 2 and stats[0] == u, stats
            assert cache.info()["held"] == u + u // 2
            _, stats = cached(engine, cache, *a, fl, co, reference(engine, *a, fl, co), form="device")
            assert stats[HITS] == u and stats[INSERTED] == 0, stats


def test_every_class_of_bad_lane_cold_and_warm(engine, oracle):
    rng = np.random.default_rng(16301)
    (sigs, pks, msgs, inf), touched, g, kinds = spoiled_batch(engine, rng)
    n = sigs.shape[0]
    samp = np.unique(np.concatenate([touched, np.arange(0, n, 41)]))
    co = coeffs32(rng, n)
    with engine.keycache_create(4096) as cache:
        for fl in NEW_SETTINGS:                                     # flags 1, 9 and 0
            ref = reference(engine, sigs, pks, msgs, fl, co, pk_inf=inf)
            u = ref[2][0]
            cache.clear()
            st, stats = cached(engine, cache, sigs, pks, msgs, fl, co, ref, pk_inf=inf)
            assert stats[INSERTED] == u and stats[HITS] == 0, (fl, stats)
            for form in ("host", "device"):
                sw, stats = cached(engine, cache, sigs, pks, msgs, fl, co, ref, pk_inf=inf, form=form)
                assert stats[INSERTED] == 0 and stats[HITS] == u, (fl, form, stats)   # the bad keys are hits too
                assert sw.tobytes() == st.tobytes()
            # library-drawn coefficients: the exact vector again
            w = ref[0]
            sd, nf, _ = engine.verify_many_cached(cache, sigs, pks, msgs, pk_inf=inf, **fl)
            assert sd.tobytes() == w.tobytes() and nf == ref[1]
            wo = oracle.verify_many(sigs[samp], pks[samp], msgs[samp], pk_inf=inf[samp], **fl)
            bad = np.nonzero(st[samp] != wo)[0]
            assert bad.size == 0, (fl, samp[bad[:10]], st[samp][bad[:10]], wo[bad[:10]])
            if fl["check_torsion"]:
                assert (st[g["p_plus_t2"]] == 1).all() and (st[g["small_order"]] == 1).all()
                assert (st[g["both_bad"][:2]] == 1).all() and (st[g["both_bad"][4:]] == 1).all()
            assert (st[g["both_bad"][2:4]] == 3).all() and (st[g["noncanon"]] == 3).all()
            assert (st[g["identity"][:-1]] == 0).all() and st[g["identity"][-1]] == 2
            for i, kind in kinds.items():
                if kind in ("e_bit", "msg_bit"):
                    assert st[i] == 2, (fl, i, kind)
                elif kind in ("noncanon_pk", "pk_off_curve", "e_ge_q"):
                    assert st[i] == 3, (fl, i, kind)


def test_keys_that_differ_only_in_pk_inf_are_two_keys(engine):
    rng = np.random.default_rng(16351)
    n = 6000
    sigs, pks, msgs = honest(engine, rng, n, 5)
    inf = np.zeros(n, np.uint8)
    holders = np.nonzero((pks == pks[17]).all(axis=1))[0]
    inf[holders[::2]] = 1                      # the same 96 bytes with and without the identity flag
    co = coeffs32(rng, n)
    with engine.keycache_create(64) as cache:
        ref = reference(engine, sigs, pks, msgs, T, co, pk_inf=inf)
        assert ref[2][0] == 6
        _, stats = cached(engine, cache, sigs, pks, msgs, T, co, ref, pk_inf=inf)
        assert stats[INSERTED] == 6
        _, stats = cached(engine, cache, sigs, pks, msgs, T, co, ref, pk_inf=inf, form="device")
        assert stats[HITS] == 6 and stats[INSERTED] == 0
        # without the flags the flagged holders' key is a hit, and nothing is inserted
        ref0 = reference(engine, sigs, pks, msgs, T, co)
        _, stats = cached(engine, cache, sigs, pks, msgs, T, co, ref0)
        assert stats[HITS] == 5 and stats[INSERTED] == 0 and stats[0] == 5


def test_automatic_clear(engine):
    rng = np.random.default_rng(16401)
    n = 6000
    a = honest(engine, rng, n, 50)
    b = honest(engine, rng, n, 50)
    a[1][5, 0:8] = 0xFF                        # a malformed key among A's: 51 keys
    co = coeffs32(rng, n)
    ra, rb = reference(engine, *a, T, co), reference(engine, *b, T, co)
    ua = ra[2][0]
    assert ua == 51 and rb[2][0] == 50
    with engine.keycache_create(64) as cache:
        for k, (batch, ref, clears, form) in enumerate(((a, ra, 0, "host"), (b, rb, 1, "device"), (a, ra, 1, "host"))):
            _, stats = cached(engine, cache, *batch, T, co, ref, form=form)
            assert stats[CLEARS] == clears and stats[BYPASSED] == 0, (k, stats)
            assert stats[INSERTED] == ref[2][0] and stats[HITS] == 0, (k, stats)
            assert cache.info()["held"] == ref[2][0]
        assert cache.info()["clears"] == 2


def test_automatic_clear_with_fifty_keys_each(engine):
    """the case of the issue to the letter: capacity 64, 50 keys, 50 others, the first 50 again"""
    rng = np.random.default_rng(16402)
    n = 5000
    a, b = honest(engine, rng, n, 50), honest(engine, rng, n, 50)
    co = coeffs32(rng, n)
    ra, rb = reference(engine, *a, T, co), reference(engine, *b, T, co)
    with engine.keycache_create(64) as cache:
        for batch, ref, clears in ((a, ra, 0), (b, rb, 1), (a, ra, 1)):
            _, stats = cached(engine, cache, *batch, T, co, ref, form="device")
            assert stats[CLEARS] == clears and cache.info()["held"] == 50, stats
            assert stats[INSERTED] == 50 and stats[HITS] == 0


def test_bypass(engine):
    rng = np.random.default_rng(16501)
    n = 20000
    sigs, pks, msgs = honest(engine, rng, n, 50)
    corrupt(rng, sigs, pks, msgs, list(range(7, n, 1999)))
    few = honest(engine, rng, 5000, 9)
    co = coeffs32(rng, n)
    with engine.keycache_create(16) as cache:
        cached(engine, cache, *few, T, co[:5000], reference(engine, *few, T, co[:5000]))
        assert cache.info()["held"] == 9
        for fl in NEW_SETTINGS:
            ref = reference(engine, sigs, pks, msgs, fl, co)
            for form in ("host", "device"):
                _, stats = cached(engine, cache, sigs, pks, msgs, fl, co, ref, form=form)
                assert stats[BYPASSED] == 1 == stats[5] and stats[HITS] == 0 and stats[INSERTED] == 0, (fl, form, stats)
                assert stats == ref[2] + [0, 0, 0, 1]
                info = cache.info()
                assert info["held"] == 9 and info["clears"] == 0
        # the cache still serves what it held
        _, stats = cached(engine, cache, *few, T, co[:5000], reference(engine, *few, T, co[:5000]), form="device")
        assert stats[HITS] == 9 and stats[INSERTED] == 0


def test_clear_makes_the_next_call_cold(engine):
    rng = np.random.default_rng(16601)
    n, u = 8000, 120
    sigs, pks, msgs = honest(engine, rng, n, u)
    sigs[4000, 50] ^= 1
    co = coeffs32(rng, n)
    ref = reference(engine, sigs, pks, msgs, T, co)
    with engine.keycache_create(256) as cache:
        for k in range(3):
            _, stats = cached(engine, cache, sigs, pks, msgs, T, co, ref, form="device")
            assert stats[INSERTED] == u and stats[HITS] == 0 and stats[CLEARS] == 0
            _, stats = cached(engine, cache, sigs, pks, msgs, T, co, ref)
            assert stats[HITS] == u and stats[INSERTED] == 0
            cache.clear()
            info = cache.info()
            assert info["held"] == 0 and info["clears"] == k + 1 and info["capacity"] == 256


def test_short_probe_bound():
    import schnorr_sig_amd as ssa
    eng = ssa.Engine(0)
    try:
        rng = np.random.default_rng(16701)
        n, u = 20000, 1000
        sigs, pks, msgs = honest(eng, rng, n, u)
        corrupt(rng, sigs, pks, msgs, list(range(3, n, 2503)))
        co = coeffs32(rng, n)
        want, wnf = eng.verify_many(sigs, pks, msgs, **T)
        eng.debug_dedup_config(-1.0, 1)
        with eng.keycache_create(4096) as cache:
            for k in range(2):
                for form in ("host", "device"):
                    if form == "host":
                        st, nf, stats = eng.verify_many_cached(cache, sigs, pks, msgs, coeffs=co, **T)
                    else:
                        st, nf, stats = cached_device(eng, cache, sigs, pks, msgs, coeffs=co, **T)
                    print("probe bound 1: call", k, form, [int(v) for v in stats], cache.info())
                    assert st.tobytes() == want.tobytes() and nf == wnf          # whatever stats[7] says
                    assert int(stats[HITS]) + int(stats[INSERTED]) == int(stats[0]) >= u
                    assert cache.info()["held"] <= 4096
    finally:
        eng.close()


_CHILD = r"""
import json, os, sys
sys.path.insert(0, %(root)r)
import numpy as np
import torch
import schnorr_sig_amd as ssa
rng = np.random.default_rng(16801)
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
screened = n if n %% 5000 > 3072 else n - n %% 5000      # lanes in slices that reach the cache
out = {"info": e.info()["lane_slice"], "cases": [], "distinct": int(np.unique(pk[:screened], axis=0).shape[0])}
dev = torch.device("cuda", 0)
for fl in (dict(check_torsion=True, sig_flag_byte=False), dict(check_torsion=True, sig_flag_byte=True),
           dict(check_torsion=False, sig_flag_byte=False)):
    want, wnf = e.verify_many(sg, pk, m, **fl)
    scr, snf, sstats = e.verify_many_screened(sg, pk, m, coeffs=co, **fl)
    kc = e.keycache_create(64)
    st, nf, stats = e.verify_many_cached(kc, sg, pk, m, coeffs=co, **fl)
    held_host = kc.info()["held"]
    kc.clear()
    ds, dp, dm, dc = (torch.from_numpy(a).to(dev) for a in (sg, pk, m, co))
    dst = torch.full((n,), 255, dtype=torch.uint8, device=dev)
    dnf = torch.zeros(1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    dstats = e.verify_many_cached_device(kc, ds.data_ptr(), dp.data_ptr(), dm.data_ptr(), n, 80, dc.data_ptr(), 32,
                                         dst.data_ptr(), dnf.data_ptr(), **fl)
    e.sync()
    held_dev = kc.info()["held"]
    st2, nf2, stats2 = e.verify_many_cached(kc, sg, pk, m, coeffs=co, **fl)      # warm
    out["cases"].append({"equal": bool((st == want).all()), "dev_equal": bool((dst.cpu().numpy() == want).all()),
                         "warm_equal": bool((st2 == want).all()), "scr_equal": st.tobytes() == scr.tobytes(),
                         "forms_equal": st.tobytes() == dst.cpu().numpy().tobytes(),
                         "nf": [int(nf), int(wnf), int(dnf.item()), int(nf2), int(snf)],
                         "bad": [int(st[i]) for i in bad + [7000, 10500]],
                         "stats": [int(v) for v in stats], "dstats": [int(v) for v in dstats],
                         "wstats": [int(v) for v in stats2], "sstats": [int(v) for v in sstats],
                         "held": [held_host, held_dev, kc.info()["held"]]})
    kc.close()
print("RESULT " + json.dumps(out))
e.close()
"""


@pytest.mark.parametrize("n", [12000, 14500])
def test_more_than_one_slice_host_and_device_forms(n):
    """SSA_LANE_SLICE = 5000 in a fresh child process, both forms, bad lanes on both sides of every slice boundary and a
    malformed key in the second and in the last slice.  n = 14500: three screened slices.  n = 12000: a last slice of
    2000 lanes on the exact path, which leaves the cache alone.  The 25 honest keys of slice 0 return in every later
    slice and are hits there within the same call; the malformed keys are new where they first appear."""
    env = dict(os.environ)
    env["SSA_LANE_SLICE"] = "5000"
    r = subprocess.run([sys.executable, "-c", _CHILD % {"root": ROOT, "n": n}], env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    assert out["info"] == 5000
    # the distinct keys of the slices that reach the cache (25 honest ones and the malformed ones; that of lane 10500
    # lies in such a slice only for n = 14500) are inserted once each; every later appearance is a hit
    d = out["distinct"]
    assert d in ({12000: (26,), 14500: (26, 27)}[n])
    for c in out["cases"]:
        per_slice = c["sstats"][0]               # distinct keys summed over the screened slices
        assert per_slice >= {12000: 51, 14500: 76}[n]
        cold, warm = [per_slice - d, d], [per_slice, 0]
        assert c["equal"] and c["dev_equal"] and c["warm_equal"] and c["scr_equal"] and c["forms_equal"], c
        assert c["nf"] == [9] * 5 and c["bad"] == [2] * 7 + [3, 3], c
        for s in (c["stats"], c["dstats"], c["wstats"]):
            assert s[:7] == c["sstats"][:7] and s[7] == 0 and s[CLEARS] == 0 and s[BYPASSED] == 0, c
            assert s[HITS] + s[INSERTED] == s[0]
        assert c["stats"][HITS:INSERTED + 1] == cold and c["dstats"][HITS:INSERTED + 1] == cold, c
        assert c["wstats"][HITS:INSERTED + 1] == warm, c
        assert c["held"] == [cold[1]] * 3, c


def test_workspaces_do_not_grow_from_the_second_call_on():
    import schnorr_sig_amd as ssa
    eng = ssa.Engine(0)
    try:
        rng = np.random.default_rng(16901)
        n = 30000
        sigs, pks, msgs = honest(eng, rng, n, 500)
        corrupt(rng, sigs, pks, msgs, list(range(5, n, 3001)))
        with eng.keycache_create(2048) as cache:
            bytes0 = cache.info()["device_bytes"]
            assert bytes0 >= 2048 * (4096 + 96 + 2 + 32)
            sizes = []
            for k in range(6):
                if k == 3:
                    cache.clear()
                eng.verify_many_cached(cache, sigs, pks, msgs, **T)
                cached_device(eng, cache, sigs, pks, msgs, **T)
                sizes.append(eng.info()["workspace_bytes"])
                assert cache.info()["device_bytes"] == bytes0
            assert sizes[0] > 0 and sizes[5] == sizes[1], sizes
    finally:
        eng.close()


def test_full_occupancy_is_deterministic(engine):
    rng = np.random.default_rng(17001)
    n, u = 1 << 20, 1000
    sigs, pks, msgs = honest(engine, rng, n, u)
    corrupt(rng, sigs, pks, msgs, list(range(11, n, 40009)))
    co = coeffs32(rng, n)
    ref = reference(engine, sigs, pks, msgs, T, co)
    runs = []
    for _ in range(2):
        with engine.keycache_create(1 << 12) as cache:
            cold = cached(engine, cache, sigs, pks, msgs, T, co, ref, form="device")
            warm = cached(engine, cache, sigs, pks, msgs, T, co, ref, form="device")
            assert cold[1][INSERTED] == cold[1][0] >= u and warm[1][HITS] == warm[1][0] and warm[1][INSERTED] == 0
            runs += [cold[0], warm[0]]
    assert all(r.tobytes() == runs[0].tobytes() for r in runs)


def test_module_level_verify_many_cached_over_objects(engine):
    import schnorr_sig_amd as ssa
    rng = np.random.default_rng(17101)
    n, u = 3200, 3
    sigs, pks, msgs = honest(engine, rng, n, u, msg_len=16)
    sigs[4, 50] ^= 1
    pks[9, 0:8] = 0xFF
    so, po, mo = ([ssa.Signature(s.tobytes()) for s in sigs], [ssa.PublicKey(p.tobytes()) for p in pks],
                  [m.tobytes() for m in msgs])
    with engine.keycache_create(16) as cache:
        for k in range(2):
            res = ssa.verify_many_cached(so, po, mo, cache)
            assert len(res) == n
            for i, r in enumerate(res):
                if i == 4:
                    assert isinstance(r, ssa.SignatureError) and r.kind == ssa.SignatureError.InvalidSignature
                elif i == 9:
                    assert isinstance(r, ssa.MalformedInput)
                else:
                    assert r is None
            assert cache.info()["held"] == u + 1
        assert ssa.verify_many_cached(so[:12], po[:12], mo[:12], cache)[4] is not None     # a small batch: the exact path
        assert cache.info()["held"] == u + 1


def test_a_cache_of_another_context_is_refused(engine):
    import schnorr_sig_amd as ssa
    other = ssa.Engine(0)
    try:
        rng = np.random.default_rng(17151)
        sigs, pks, msgs = honest(engine, rng, 4000, 3)
        with other.keycache_create(16) as cache:
            with pytest.raises(Exception):
                engine.verify_many_cached(cache, sigs, pks, msgs, **T)
            assert cache.info()["held"] == 0
    finally:
        other.close()


def test_a_cache_that_outlives_its_context_is_orphaned_not_dangling():
    import ctypes as C
    import schnorr_sig_amd as ssa
    eng = ssa.Engine(0)
    rng = np.random.default_rng(17201)
    sigs, pks, msgs = honest(eng, rng, 4000, 10)
    cache = eng.keycache_create(64)
    st, nf, stats = eng.verify_many_cached(cache, sigs, pks, msgs, **T)
    assert (st == 0).all() and int(stats[INSERTED]) == 10
    handle = cache.handle
    eng.close()                                   # the context goes first
    out = (C.c_uint64 * 4)()
    assert ssa._lib.ssa_keycache_info(handle, out) == ssa.ERR_ARG
    assert ssa._lib.ssa_keycache_clear(handle) == ssa.ERR_ARG
    cache.close()                                 # no crash
    cache.close()                                 # and only once
