"""KeyedSignature wire records through a key cache in wire mode (ssa_verify_keyed_many_cached).
The reference for every vector is ssa_verify_keyed_many on the same records (exact); with the coefficients pinned it is
also ssa_verify_many_screened on the unpacked records, byte for byte.  Touched lanes and a sample of clean ones are
checked against the CPU oracle.  Every batch that is meant to reach the cache has more than SSA_MSM_SMALL_MAX (3072)
lanes."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_screened_torsion import NEW_SETTINGS, T, coeffs32, corrupt, dev, key_choice, make_scalars

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HITS, INSERTED, CLEARS, BYPASSED = 8, 9, 10, 11
DECOMPRESS_KEY, BUILD_KEY = "ssa_k_keyed_decompress", "ssa_k_keyset_build"


def keyed_honest(engine, rng, n, u, msg_len=80, sks=None):
    """n honest 130-byte records by u distinct signers (or by the given secret keys) -> (records, messages)"""
    sks = make_scalars(rng, u) if sks is None else sks
    msgs = rng.integers(0, 256, size=(n, msg_len), dtype=np.uint8)
    _, keyed = engine.keygen_sign_many(sks[key_choice(rng, n, sks.shape[0])], make_scalars(rng, n), msgs, keyed=True)
    assert keyed.shape == (n, 130)
    return keyed, msgs


def unpack(engine, keyed):
    """P(keyed): what ssa_k_unpack_keyed produces -- affine keys ((0, 0) for undecodable ones), pk_inf, signatures"""
    pks, inf, st = engine.decompress_many(keyed[:, :49])
    assert not pks[st != 0].any() and not inf[st != 0].any()
    return np.ascontiguousarray(keyed[:, 49:]), pks, inf


def reference(engine, keyed, msgs, fl, coeffs):
    """what a cached wire call must return: ssa_verify_keyed_many's vector and count (flags without the flag-byte bit),
    ssa_verify_many's on the unpacked records, and ssa_verify_many_screened's bytes and statistics"""
    sigs, pks, inf = unpack(engine, keyed)
    w, wnf = engine.verify_many(sigs, pks, msgs, pk_inf=inf, **fl)
    assert wnf == int((w != 0).sum())
    if not fl["sig_flag_byte"]:
        k, knf = engine.verify_keyed_many(keyed, msgs, check_torsion=fl["check_torsion"])
        assert k.tobytes() == w.tobytes() and knf == wnf
    s, snf, sstats = engine.verify_many_screened(sigs, pks, msgs, coeffs=coeffs, pk_inf=inf, **fl)
    assert s.tobytes() == w.tobytes() and snf == wnf
    return w, wnf, [int(v) for v in sstats]


def keyed_cached_device(engine, cache, keyed, msgs, coeffs=None, **fl):
    import torch
    n = keyed.shape[0]
    dk, dm = dev(keyed, msgs)
    dc = dev(coeffs)[0] if coeffs is not None else None
    st = torch.full((n,), 255, dtype=torch.uint8, device="cuda:0")
    nf = torch.full((1,), -1, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    stats = engine.verify_keyed_many_cached_device(cache, dk.data_ptr(), dm.data_ptr(), n, msgs.shape[1],
                                                   dc.data_ptr() if dc is not None else 0, 32, st.data_ptr(),
                                                   nf.data_ptr(), **fl)
    engine.sync()
    return st.cpu().numpy(), int(nf.item()), stats


def cached(engine, cache, keyed, msgs, fl, coeffs, ref, form="host", same_keys=True):
    """one cached wire call against `ref` -> (status, stats).  same_keys: every key decodes, so the distinct 49-byte
    strings are the distinct affine keys and stats[0] is the screened call's too."""
    w, wnf, sstats = ref
    if form == "host":
        st, nf, stats = engine.verify_keyed_many_cached(cache, keyed, msgs, coeffs=coeffs, **fl)
    else:
        st, nf, stats = keyed_cached_device(engine, cache, keyed, msgs, coeffs=coeffs, **fl)
    stats = [int(v) for v in stats]
    bad = np.nonzero(st != w)[0]
    assert bad.size == 0, (fl, form, bad[:10], st[bad[:10]], w[bad[:10]])
    assert st.tobytes() == w.tobytes() and nf == wnf, (fl, form, nf, wnf)
    assert stats[1:7] == sstats[1:7], (fl, form, stats, sstats)
    assert stats[0] == sstats[0] if same_keys else stats[0] >= sstats[0], (fl, form, stats, sstats)
    assert stats[7] >= sstats[7]
    return st, stats


def launches(engine):
    return engine.read_timing(BUILD_KEY)[1], engine.read_timing(DECOMPRESS_KEY)[1]


@pytest.mark.parametrize("n", [5000, 1 << 16])
@pytest.mark.parametrize("u_of", ["1", "7", "n/16", "n"])
def test_cold_then_warm(engine, n, u_of):
    u = {"1": 1, "7": 7, "n/16": n // 16, "n": n}[u_of]
    rng = np.random.default_rng(18100 + n % 1000 + u % 97)
    keyed, msgs = keyed_honest(engine, rng, n, u)
    co = coeffs32(rng, n)
    ref = reference(engine, keyed, msgs, T, co)
    with engine.keycache_create(max(u, 64), wire=True) as cache:
        assert cache.wire
        engine.enable_timing(True)
        try:
            launches(engine)                                        # drains the keys
            st, stats = cached(engine, cache, keyed, msgs, T, co, ref, form="device")
            assert (st == 0).all() and stats[3] == 0
            assert stats[INSERTED] == u and stats[HITS] == 0 and stats[0] == u, stats
            assert stats[CLEARS] == 0 and stats[BYPASSED] == 0 and stats[7] == 0, stats
            assert launches(engine) == (1, 1)
            assert cache.info()["held"] == u
            for form in ("device", "host"):
                st, stats = cached(engine, cache, keyed, msgs, T, co, ref, form=form)
                assert (st == 0).all() and stats[3] == 0
                assert stats[HITS] == u and stats[INSERTED] == 0 and stats[0] == u, (form, stats)
                assert stats[CLEARS] == 0 and stats[BYPASSED] == 0 and stats[7] == 0, (form, stats)
            assert launches(engine) == (0, 0), "a warm call decompresses no key and checks none"
            assert engine.read_timing("keyed_split")[1] == 3 and engine.read_timing("keyed_expand")[1] == 3
            assert engine.read_timing("keycache_lookup")[1] == 3 and engine.read_timing("keycache_map")[1] == 3
        finally:
            engine.enable_timing(False)
        assert cache.info()["held"] == u and cache.info()["clears"] == 0


def _fixture_key():
    """the reference's non-subgroup point (src/signature.rs:387-404) as 96 affine bytes"""
    with open(os.path.join(ROOT, "tests", "golden", "vectors.json")) as fh:
        f = json.load(fh)["fixture_small_order_pk"]
    return np.frombuffer(b"".join(int(x).to_bytes(8, "little") for x in (f["x"] + f["y"])), dtype=np.uint8)


def spoiled_records(engine, oracle, rng, n=20000, u=50):
    """every class of bad lane of the issue on keys that repeat, lanes at segment edges -> records, messages, the
    touched lanes, the lanes by class"""
    import schnorr_sig_amd as ssa
    keyed, msgs = keyed_honest(engine, rng, n, u)
    clean = keyed.copy()
    seg = ssa.debug_screen_plan(n)["segment_lanes"]
    edges = [0, seg - 1, seg, 2 * seg - 1, 5 * seg, n - 1]
    lanes = sorted(set(edges + [255, 256] + [int(v) for v in rng.choice(n, 48, replace=False)]))
    # a. the signature classes of corrupt(); its key classes act on a scratch copy of affine keys and are redone on the
    #    wire bytes by the classes below
    kinds = corrupt(rng, keyed[:, 49:], np.zeros((n, 96), np.uint8), msgs, lanes)
    for i, kind in zip(lanes, kinds):
        if kind == "swap_key":
            keyed[i, :49] = clean[(i + 1) % n, :49]
        elif kind == "noncanon_pk":
            keyed[i, 0:8] = 0xFF
        elif kind == "pk_off_curve":
            keyed[i, 8] ^= 1                      # another x: another key, or none
    free = np.setdiff1d(np.arange(n), np.array(lanes + [(i + 1) % n for i in lanes]))
    rng.shuffle(free)
    is_free = set(free.tolist())
    edge_pool = [k * seg + d for k in range(1, (n + seg - 1) // seg) for d in (-1, 0) if k * seg + d in is_free]
    free = np.array([i for i in free if i not in set(edge_pool)])
    g, at = {}, 0

    def take(k, at_edge=0):
        """k free lanes, the first at_edge of them (while there are any) next to a segment boundary"""
        nonlocal at
        out = [edge_pool.pop() for _ in range(min(at_edge, len(edge_pool)))]
        rest = k - len(out)
        out += [int(v) for v in free[at:at + rest]]
        at += rest
        return np.array(out)

    # b. an off-subgroup key: the reference's fixture through compress_many
    comp, st = engine.compress_many(_fixture_key())
    assert st[0] == 0
    g["off_subgroup"] = take(20, 1)
    keyed[g["off_subgroup"], :49] = comp[0]
    # c. the identity encoding: e = r and R = [r]G verifies (the key contributes nothing); the last one is wrong
    kl = take(6, 1)
    r = make_scalars(rng, kl.size)
    rp, _ = engine.keygen_sign_many(r, r, msgs[kl])
    rc, _ = engine.compress_many(rp)
    keyed[kl, :48] = 0
    keyed[kl, 48] = 0x80
    keyed[kl, 49:98] = rc
    keyed[kl, 98:] = r
    keyed[kl[-1], 98] ^= 2
    g["identity"] = kl
    # d. 0xc0, e. x != 0 with 0x80, f. 0xff * 49, g. a limb >= p: none of them decodes
    g["c0"] = take(4, 1)
    keyed[g["c0"], :48] = 0
    keyed[g["c0"], 48] = 0xC0
    g["inf_x"] = take(4, 1)
    keyed[g["inf_x"], 48] = 0x80
    g["all_ff"] = take(4, 1)
    keyed[g["all_ff"], :49] = 0xFF
    g["limb_ge_p"] = take(4, 1)
    keyed[g["limb_ge_p"], 16:24] = np.frombuffer((0xFFFFFFFF00000001).to_bytes(8, "little"), np.uint8)     # == p
    # h. a flipped sort bit on an honest key: it decodes to -P
    g["neg_key"] = take(6, 1)
    keyed[g["neg_key"], 48] ^= 0x40
    # i. 64 keys of random x with bit 63 of every limb cleared and alternating sort bit, two lanes each
    krng = np.random.default_rng(18001)
    xs = krng.integers(0, 256, size=(64, 49), dtype=np.uint8)
    xs[:, 7:48:8] &= 0x7F
    xs[:, 48] = np.where(np.arange(64) % 2 == 0, 0x00, 0x40)
    lanes_i = take(128, 40)
    keyed[lanes_i[:64], :49] = xs
    keyed[lanes_i[64:], :49] = xs
    g["random_x"] = lanes_i
    decodes = [oracle.decompress(x.tobytes()) is not None for x in xs]
    assert sum(decodes) >= 8 and 64 - sum(decodes) >= 8, sum(decodes)
    assert sum(int(i) % seg in (0, seg - 1) for i in lanes_i) >= 8      # lanes of this class at segment edges
    touched = np.unique(np.concatenate([np.array(lanes)] + list(g.values())))
    return keyed, msgs, touched, g, dict(zip(lanes, kinds))


def oracle_statuses(oracle, keyed, msgs, lanes, fl):
    """KeyedSignature::from_bytes then verify on the CPU: 3 where the key does not decode"""
    out = np.zeros(len(lanes), np.uint8)
    for k, i in enumerate(lanes):
        d = oracle.decompress(keyed[i, :49].tobytes())
        if d is None:
            out[k] = 3
            continue
        pk, inf = d
        out[k] = oracle.verify_many(keyed[i:i + 1, 49:], np.frombuffer(pk, np.uint8).reshape(1, 96), msgs[i:i + 1],
                                    pk_inf=np.array([1 if inf else 0], np.uint8), **fl)[0]
    return out


def test_every_class_of_bad_lane_cold_and_warm(engine, oracle):
    rng = np.random.default_rng(18301)
    keyed, msgs, touched, g, kinds = spoiled_records(engine, oracle, rng)
    n = keyed.shape[0]
    samp = np.unique(np.concatenate([touched, np.arange(0, n, 41)]))
    co = coeffs32(rng, n)
    u = np.unique(keyed[:, :49], axis=0).shape[0]                   # distinct 49-byte strings
    with engine.keycache_create(4096, wire=True) as cache:
        for fl in NEW_SETTINGS:                                     # flags 1, 9 and 0
            ref = reference(engine, keyed, msgs, fl, co)
            assert u > ref[2][0], "several undecodable strings are one affine key (0, 0) and several wire keys"
            cache.clear()
            st, stats = cached(engine, cache, keyed, msgs, fl, co, ref, same_keys=False)
            assert stats[0] == u and stats[INSERTED] == u and stats[HITS] == 0, (fl, stats)
            for form in ("host", "device"):
                sw, stats = cached(engine, cache, keyed, msgs, fl, co, ref, form=form, same_keys=False)
                assert stats[INSERTED] == 0 and stats[HITS] == u, (fl, form, stats)   # the bad keys are hits too
                assert sw.tobytes() == st.tobytes()
            assert cache.info()["held"] == u
            # library-drawn coefficients: the exact vector again
            sd, nf, _ = engine.verify_keyed_many_cached(cache, keyed, msgs, **fl)
            assert sd.tobytes() == ref[0].tobytes() and nf == ref[1]
            wo = oracle_statuses(oracle, keyed, msgs, samp, fl)
            bad = np.nonzero(st[samp] != wo)[0]
            assert bad.size == 0, (fl, samp[bad[:10]], st[samp][bad[:10]], wo[bad[:10]])
            if fl["check_torsion"]:
                assert (st[g["off_subgroup"]] == 1).all()
            assert (st[g["identity"][:-1]] == 0).all() and st[g["identity"][-1]] == 2
            for name in ("c0", "inf_x", "all_ff", "limb_ge_p"):
                assert (st[g[name]] == 3).all(), (fl, name)
            assert (st[g["neg_key"]] == 2).all()
            ri = g["random_x"]
            assert (st[ri[:64]] == st[ri[64:]]).all() and set(st[ri].tolist()) <= {1, 2, 3}
            assert (st[ri] == 3).sum() >= 16 and (st[ri] != 3).sum() >= 16
            for i, kind in kinds.items():
                if kind in ("e_bit", "msg_bit"):
                    assert st[i] == 2, (fl, i, kind)
                elif kind in ("noncanon_pk", "e_ge_q"):
                    assert st[i] == 3, (fl, i, kind)


def test_partly_warm(engine):
    rng = np.random.default_rng(18201)
    n, u = 20000, 400
    sks = make_scalars(rng, u + u // 2)
    a = keyed_honest(engine, rng, n, u, sks=sks[:u])
    b = keyed_honest(engine, rng, n, u, sks=sks[u // 2:])          # u keys: the second half of A's and u / 2 new ones
    with engine.keycache_create(1024, wire=True) as cache:
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


def test_bypass_leaves_the_cache_unchanged(engine):
    """capacity < u"""
    rng = np.random.default_rng(18501)
    n = 20000
    keyed, msgs = keyed_honest(engine, rng, n, 50)
    corrupt(rng, keyed[:, 49:], np.zeros((n, 96), np.uint8), msgs, list(range(7, n, 1999)))
    keyed[11, :49] = 0xFF                                           # and a key that does not decode: 51 keys
    few = keyed_honest(engine, rng, 5000, 9)
    co = coeffs32(rng, n)
    with engine.keycache_create(16, wire=True) as cache:
        cached(engine, cache, *few, T, co[:5000], reference(engine, *few, T, co[:5000]))
        assert cache.info()["held"] == 9
        for fl in NEW_SETTINGS:
            ref = reference(engine, keyed, msgs, fl, co)
            for form in ("host", "device"):
                _, stats = cached(engine, cache, keyed, msgs, fl, co, ref, form=form)
                assert stats[BYPASSED] == 1 == stats[5] and stats[HITS] == 0 and stats[INSERTED] == 0, (fl, form, stats)
                assert stats == ref[2] + [0, 0, 0, 1] and stats[0] == 51
                info = cache.info()
                assert info["held"] == 9 and info["clears"] == 0
        # the cache still serves what it held
        _, stats = cached(engine, cache, *few, T, co[:5000], reference(engine, *few, T, co[:5000]), form="device")
        assert stats[HITS] == 9 and stats[INSERTED] == 0


def test_automatic_clear(engine):
    """held + m > capacity >= u"""
    rng = np.random.default_rng(18401)
    n = 6000
    a, b = keyed_honest(engine, rng, n, 50), keyed_honest(engine, rng, n, 50)
    a[0][5, 0:8] = 0xFF                        # an undecodable key among A's: 51 keys
    co = coeffs32(rng, n)
    ra, rb = reference(engine, *a, T, co), reference(engine, *b, T, co)
    assert ra[2][0] == 51 and rb[2][0] == 50
    with engine.keycache_create(64, wire=True) as cache:
        for k, (batch, ref, clears, form) in enumerate(((a, ra, 0, "host"), (b, rb, 1, "device"), (a, ra, 1, "host"))):
            _, stats = cached(engine, cache, *batch, T, co, ref, form=form)
            assert stats[CLEARS] == clears and stats[BYPASSED] == 0, (k, stats)
            assert stats[INSERTED] == ref[2][0] and stats[HITS] == 0, (k, stats)
            assert cache.info()["held"] == ref[2][0]
        assert cache.info()["clears"] == 2


def test_a_full_cache_and_one_new_key_is_a_clear(engine):
    """capacity == u, then one new key"""
    rng = np.random.default_rng(18451)
    n, u = 5000, 64
    keyed, msgs = keyed_honest(engine, rng, n, u)
    co = coeffs32(rng, n)
    ref = reference(engine, keyed, msgs, T, co)
    new_rec, new_msg = keyed_honest(engine, rng, 1, 1)             # somebody else's record: a key never seen
    more, more_msgs = keyed.copy(), msgs.copy()
    more[n - 1], more_msgs[n - 1] = new_rec[0], new_msg[0]
    ref_more = reference(engine, more, more_msgs, T, co)
    assert ref_more[2][0] == u + 1
    with engine.keycache_create(u, wire=True) as cache:
        _, stats = cached(engine, cache, keyed, msgs, T, co, ref, form="device")
        assert stats[INSERTED] == u and stats[CLEARS] == 0 and cache.info()["held"] == u
        _, stats = cached(engine, cache, keyed, msgs, T, co, ref)
        assert stats[HITS] == u and stats[INSERTED] == 0 and stats[CLEARS] == 0
        # u + 1 keys do not fit: the slice bypasses; u keys of which one is new: a clear
        _, stats = cached(engine, cache, more, more_msgs, T, co, ref_more, form="device")
        assert stats[BYPASSED] == 1 and cache.info()["held"] == u and cache.info()["clears"] == 0
        swapped = keyed.copy()
        holders = np.nonzero((keyed[:, :49] == keyed[0, :49]).all(axis=1))[0]
        swapped[holders] = new_rec[0]                               # one key leaves, a new one comes: still u keys
        swapped_msgs = msgs.copy()
        swapped_msgs[holders] = new_msg[0]
        ref_sw = reference(engine, swapped, swapped_msgs, T, co)
        assert ref_sw[2][0] == u
        st, stats = cached(engine, cache, swapped, swapped_msgs, T, co, ref_sw)
        assert stats[CLEARS] == 1 and stats[INSERTED] == u and stats[HITS] == 0 and stats[BYPASSED] == 0, stats
        assert (st[holders] == 0).all()
        assert cache.info()["held"] == u and cache.info()["clears"] == 1


def test_the_mode_of_the_cache_is_checked_against_the_call(engine):
    rng = np.random.default_rng(18551)
    n = 4000
    keyed, msgs = keyed_honest(engine, rng, n, 5)
    sigs, pks, inf = unpack(engine, keyed)
    with engine.keycache_create(64, wire=True) as wire, engine.keycache_create(64) as affine:
        assert wire.wire and not affine.wire
        assert wire.info()["device_bytes"] >= affine.info()["device_bytes"] + 64 * 49
        before = (wire.info(), affine.info())
        with pytest.raises(RuntimeError, match="ssa_verify_many_cached"):
            engine.verify_many_cached(wire, sigs, pks, msgs, **T)
        with pytest.raises(RuntimeError, match="ssa_verify_keyed_many_cached"):
            engine.verify_keyed_many_cached(affine, keyed, msgs, **T)
        import torch
        dk, ds, dp, dm = dev(keyed, sigs, pks, msgs)
        st = torch.full((n,), 255, dtype=torch.uint8, device="cuda:0")
        with pytest.raises(RuntimeError, match="ssa_verify_many_cached_device"):
            engine.verify_many_cached_device(wire, ds.data_ptr(), dp.data_ptr(), dm.data_ptr(), n, 80, 0, 32, st.data_ptr(), 0)
        with pytest.raises(RuntimeError, match="ssa_verify_keyed_many_cached_device"):
            engine.verify_keyed_many_cached_device(affine, dk.data_ptr(), dm.data_ptr(), n, 80, 0, 32, st.data_ptr(), 0)
        engine.sync()
        assert (st.cpu().numpy() == 255).all()
        assert (wire.info(), affine.info()) == before
        # and each serves its own call
        assert (engine.verify_keyed_many_cached(wire, keyed, msgs, **T)[0] == 0).all()
        assert (engine.verify_many_cached(affine, sigs, pks, msgs, pk_inf=inf, **T)[0] == 0).all()
        assert wire.info()["held"] == 5 == affine.info()["held"]


@pytest.mark.parametrize("n", [3072, 1])
def test_small_batches_take_the_exact_keyed_path(engine, n):
    rng = np.random.default_rng(18601 + n)
    keyed, msgs = keyed_honest(engine, rng, n, min(n, 9))
    keyed[0, 99] ^= 1
    if n > 1:
        keyed[n - 1, :49] = 0xFF
    co = coeffs32(rng, n)
    want, wnf = engine.verify_keyed_many(keyed, msgs, check_torsion=True)
    assert wnf == min(n, 2)
    with engine.keycache_create(64, wire=True) as cache:
        for form in ("host", "device"):
            if form == "host":
                st, nf, stats = engine.verify_keyed_many_cached(cache, keyed, msgs, coeffs=co, **T)
            else:
                st, nf, stats = keyed_cached_device(engine, cache, keyed, msgs, coeffs=co, **T)
            assert st.tobytes() == want.tobytes() and nf == wnf
            assert [int(v) for v in stats] == [0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0], (form, stats)
            assert cache.info()["held"] == 0 and cache.info()["clears"] == 0


def test_the_flag_byte_alone_is_the_screened_batch_form(engine):
    rng = np.random.default_rng(18651)
    n = 6000
    keyed, msgs = keyed_honest(engine, rng, n, 20)
    corrupt(rng, keyed[:, 49:], np.zeros((n, 96), np.uint8), msgs, list(range(5, n, 601)))
    keyed[77, :49] = 0xFF
    co = coeffs32(rng, n)
    sigs, pks, inf = unpack(engine, keyed)
    fl = dict(check_torsion=False, sig_flag_byte=True)
    want, wnf = engine.verify_many(sigs, pks, msgs, pk_inf=inf, **fl)
    scr, snf = engine.verify_batch_screened(sigs, pks, msgs, coeffs=co, pk_inf=inf)
    assert scr.tobytes() == want.tobytes() and snf == wnf and want[77] == 3
    with engine.keycache_create(64, wire=True) as cache:
        for form in ("host", "device"):
            if form == "host":
                st, nf, stats = engine.verify_keyed_many_cached(cache, keyed, msgs, coeffs=co, **fl)
            else:
                st, nf, stats = keyed_cached_device(engine, cache, keyed, msgs, coeffs=co, **fl)
            assert st.tobytes() == want.tobytes() and nf == wnf, form
            assert not np.asarray(stats).any()
            assert cache.info()["held"] == 0 and cache.info()["clears"] == 0


@pytest.mark.parametrize("n", [1, 300, 5000])
def test_verify_keyed_many_device_equals_the_host_form(engine, n):
    import torch
    rng = np.random.default_rng(18701 + n)
    keyed, msgs = keyed_honest(engine, rng, n, min(n, 13))
    keyed[0, 60] ^= 1
    if n > 1:
        keyed[n // 2, 48] |= 0x01
        keyed[n - 1, 48] ^= 0x40
    for torsion in (True, False):
        want, wnf = engine.verify_keyed_many(keyed, msgs, check_torsion=torsion)
        dk, dm = dev(keyed, msgs)
        st = torch.full((n,), 255, dtype=torch.uint8, device="cuda:0")
        nf = torch.full((1,), -1, dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()
        engine.verify_keyed_many_device(dk.data_ptr(), dm.data_ptr(), n, 80, st.data_ptr(), nf.data_ptr(),
                                        check_torsion=torsion)
        engine.sync()
        assert st.cpu().numpy().tobytes() == want.tobytes() and int(nf.item()) == wnf == min(n, 3)
        st.fill_(255)
        engine.verify_keyed_many_device(dk.data_ptr(), dm.data_ptr(), n, 80, st.data_ptr(), 0, check_torsion=torsion)
        engine.sync()
        assert st.cpu().numpy().tobytes() == want.tobytes()


_CHILD = r"""
import json, os, sys
sys.path.insert(0, %(root)r)
import numpy as np
import torch
import schnorr_sig_amd as ssa
rng = np.random.default_rng(18801)
n, u = 12345, 25
e = ssa.Engine(0)
def sc(k):
    v = rng.integers(0, 256, size=(k, 32), dtype=np.uint8); v[:, 31] &= 0x3f; v[:, 0] |= 1
    return v
idx = rng.integers(0, u, size=n); idx[:u] = np.arange(u)
idx[[4999, 5000, 9999, 10000]] = 3                # one key on both sides of every boundary
m = rng.integers(0, 256, size=(n, 80), dtype=np.uint8)
_, kd = e.keygen_sign_many(sc(u)[idx], sc(n), m, keyed=True)
bad = [0, 4998, 5001, 6123, 9998, 10001, n - 1]
for i in bad:
    kd[i, 99] ^= 4
kd[7000, 0:8] = 0xff                              # undecodable keys in the second slice and in the last
kd[10500, 0:8] = 0xff
co = rng.integers(0, 256, size=(n, 32), dtype=np.uint8); co[:, 31] &= 0x3f
out = {"info": e.info()["lane_slice"], "cases": []}
pk, inf, dst_ = e.decompress_many(kd[:, :49])
sg = np.ascontiguousarray(kd[:, 49:])
dev = torch.device("cuda", 0)
for fl in (dict(check_torsion=True, sig_flag_byte=False), dict(check_torsion=True, sig_flag_byte=True),
           dict(check_torsion=False, sig_flag_byte=False)):
    want, wnf = e.verify_many(sg, pk, m, pk_inf=inf, **fl)
    keyed_equal = True
    if not fl["sig_flag_byte"]:
        kw, knf = e.verify_keyed_many(kd, m, check_torsion=fl["check_torsion"])
        keyed_equal = kw.tobytes() == want.tobytes() and knf == wnf
    scr, snf, sstats = e.verify_many_screened(sg, pk, m, coeffs=co, pk_inf=inf, **fl)
    kc = e.keycache_create(64, wire=True)
    st, nf, stats = e.verify_keyed_many_cached(kc, kd, m, coeffs=co, **fl)
    held_host = kc.info()["held"]
    kc.clear()
    dk, dm, dc = (torch.from_numpy(a).to(dev) for a in (kd, m, co))
    dst = torch.full((n,), 255, dtype=torch.uint8, device=dev)
    dnf = torch.zeros(1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    dstats = e.verify_keyed_many_cached_device(kc, dk.data_ptr(), dm.data_ptr(), n, 80, dc.data_ptr(), 32,
                                               dst.data_ptr(), dnf.data_ptr(), **fl)
    e.sync()
    held_dev = kc.info()["held"]
    st2, nf2, stats2 = e.verify_keyed_many_cached(kc, kd, m, coeffs=co, **fl)      # warm
    out["cases"].append({"equal": bool((st == want).all()), "dev_equal": bool((dst.cpu().numpy() == want).all()),
                         "warm_equal": bool((st2 == want).all()), "scr_equal": st.tobytes() == scr.tobytes(),
                         "forms_equal": st.tobytes() == dst.cpu().numpy().tobytes(), "keyed_equal": keyed_equal,
                         "nf": [int(nf), int(wnf), int(dnf.item()), int(nf2), int(snf)],
                         "bad": [int(st[i]) for i in bad + [7000, 10500]],
                         "stats": [int(v) for v in stats], "dstats": [int(v) for v in dstats],
                         "wstats": [int(v) for v in stats2], "sstats": [int(v) for v in sstats],
                         "held": [held_host, held_dev, kc.info()["held"]]})
    kc.close()
print("RESULT " + json.dumps(out))
e.close()
"""


def test_more_than_one_slice_host_and_device_forms():
    """SSA_LANE_SLICE = 5000 in a fresh child process, n = 12345, both forms: two slices through the cache and a last one
    of 2345 lanes on the exact keyed path, which leaves the cache alone.  Bad lanes and one key lie on both sides of
    every boundary; an undecodable key sits in the second slice and in the last.  The 25 honest keys of slice 0 return in
    slice 1 and are hits there within the same call."""
    env = dict(os.environ)
    env["SSA_LANE_SLICE"] = "5000"
    r = subprocess.run([sys.executable, "-c", _CHILD % {"root": ROOT}], env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    assert out["info"] == 5000
    for c in out["cases"]:
        assert c["equal"] and c["dev_equal"] and c["warm_equal"] and c["scr_equal"] and c["forms_equal"], c
        assert c["keyed_equal"], c
        assert c["nf"] == [9] * 5 and c["bad"] == [2] * 7 + [3, 3], c
        assert c["sstats"][0] == 25 + 26 and c["sstats"][6] == 1, c     # slices 0 and 1; the last one is exact
        for s in (c["stats"], c["dstats"], c["wstats"]):
            assert s[:7] == c["sstats"][:7] and s[7] == 0 and s[CLEARS] == 0 and s[BYPASSED] == 0, c
            assert s[HITS] + s[INSERTED] == s[0]
        # cold: 25 inserted by slice 0, hits in slice 1, where the undecodable key of lane 7000 is new
        assert c["stats"][HITS:INSERTED + 1] == [25, 26] == c["dstats"][HITS:INSERTED + 1], c
        assert c["wstats"][HITS:INSERTED + 1] == [51, 0], c
        assert c["held"] == [26] * 3, c


def _honest_row(cache, u):
    """a row that holds a key of status 0"""
    import schnorr_sig_amd as ssa
    for r in range(u):
        if int(cache.debug_keytab_read(ssa.KEYTAB_STATUS, r)[0]) == 0:
            return r
    raise AssertionError("no row of status 0")


def test_selfcheck_of_a_wire_cache_reports_and_repairs_one_flipped_bit(engine):
    import schnorr_sig_amd as ssa
    rng = np.random.default_rng(18901)
    n, u = 5000, 40
    keyed, msgs = keyed_honest(engine, rng, n, u)
    keyed[17, :49] = 0xFF                                           # rows of status 3: by form, and "not a square"
    krng = np.random.default_rng(18001)
    xs = krng.integers(0, 256, size=(24, 49), dtype=np.uint8)
    xs[:, 7:48:8] &= 0x7F
    xs[:, 48] = 0
    keyed[100:124, :49] = xs
    total = np.unique(keyed[:, :49], axis=0).shape[0]
    co = coeffs32(rng, n)
    ref = reference(engine, keyed, msgs, T, co)
    with engine.keycache_create(128, wire=True) as cache:
        cached(engine, cache, keyed, msgs, T, co, ref, same_keys=False)
        assert cache.info()["held"] == total
        for deep in (False, True):
            res = cache.selfcheck(deep=deep)
            assert res["ok"] and res["keys_checked"] == total and res["keys_bad"] == 0, (deep, res)
        row = _honest_row(cache, total)
        wire_words = cache.debug_keytab_read(ssa.KEYTAB_WIRE, row)
        key_words = cache.debug_keytab_read(ssa.KEYTAB_KEY, row)
        assert (wire_words[:6] == key_words[:6]).all() and int(wire_words[6]) in (0x00, 0x40)
        # (what, word, mask, needs deep, keys the next call inserts)
        flips = ((ssa.KEYTAB_KEY, 1, 1 << 9, False, 0), (ssa.KEYTAB_KEY, 7, 1 << 3, False, 0),
                 (ssa.KEYTAB_STATUS, 0, 1, True, 0), (ssa.KEYTAB_LADDER, 40, 1 << 20, False, 0),
                 (ssa.KEYTAB_PK_INF, 0, 1, False, 0),
                 # the 49 bytes are the root of trust: the row becomes a correct row for the string it now holds, and
                 # the original key misses and is inserted again
                 (ssa.KEYTAB_WIRE, 2, 1 << 5, False, 1), (ssa.KEYTAB_WIRE, 6, 0x40, False, 1))
        for what, word, mask, needs_deep, inserted in flips:
            held = cache.info()["held"]
            cache.debug_keytab_xor(what, row, word, mask)
            if needs_deep:
                assert cache.selfcheck()["ok"], "a status flipped between 0 and 1 is seen by the deep check only"
            res = cache.selfcheck(deep=needs_deep)
            assert not res["ok"] and res["keys_bad"] == 1 and res["first_bad_key"] == row, (what, word, res)
            res = cache.selfcheck(deep=needs_deep, repair=True)
            assert res["ok"] and res["keys_bad"] == 1 and res["rows_repaired"] == 1, (what, word, res)
            assert cache.selfcheck(deep=True)["ok"]
            if not inserted:
                assert (cache.debug_keytab_read(ssa.KEYTAB_KEY, row) == key_words).all()
                assert (cache.debug_keytab_read(ssa.KEYTAB_WIRE, row) == wire_words).all()
            _, stats = cached(engine, cache, keyed, msgs, T, co, ref, form="device", same_keys=False)
            assert stats[INSERTED] == inserted and stats[HITS] == total - inserted, (what, word, stats)
            assert cache.info()["held"] == held + inserted
            if inserted:
                row = cache.info()["held"] - 1                      # the key's new row
                assert (cache.debug_keytab_read(ssa.KEYTAB_WIRE, row) == wire_words).all()
        # a row of status 3 whose 49 bytes decode after all: the plain check has no square root to see it with
        row = _honest_row(cache, cache.info()["held"])
        for k, w in enumerate(cache.debug_keytab_read(ssa.KEYTAB_KEY, row)):
            cache.debug_keytab_xor(ssa.KEYTAB_KEY, row, k, int(w))
        cache.debug_keytab_xor(ssa.KEYTAB_STATUS, row, 0, 3)
        assert cache.selfcheck()["ok"]
        res = cache.selfcheck(deep=True)
        assert not res["ok"] and res["keys_bad"] == 1 and res["first_bad_key"] == row, res
        assert cache.selfcheck(deep=True, repair=True)["ok"]
        _, stats = cached(engine, cache, keyed, msgs, T, co, ref, same_keys=False)
        assert stats[INSERTED] == 0
        # an affine cache has no wire bytes to read or poke
        with engine.keycache_create(16) as affine:
            engine.verify_many_cached(affine, *unpack(engine, keyed)[:2], msgs, **T)
            with pytest.raises(RuntimeError):
                affine.debug_keytab_read(ssa.KEYTAB_WIRE, 0)


def test_module_level_call_over_keyed_signature_objects(engine):
    import schnorr_sig_amd as ssa
    rng = np.random.default_rng(18951)
    n, u = 3200, 3
    keyed, msgs = keyed_honest(engine, rng, n, u, msg_len=16)
    keyed[4, 99] ^= 1
    objs = [ssa.KeyedSignature.from_bytes(k.tobytes(), engine) for k in keyed[:40]]
    assert all(o is not None for o in objs) and objs[0].to_bytes(engine) == keyed[0].tobytes()
    pks, inf, st = engine.decompress_many(keyed[:, :49])
    assert not st.any()
    objs = [ssa.KeyedSignature(ssa.PublicKey(p.tobytes()), ssa.Signature(k[49:].tobytes())) for p, k in zip(pks, keyed)]
    mo = [m.tobytes() for m in msgs]
    with engine.keycache_create(16, wire=True) as cache:
        for k in range(2):
            res = ssa.verify_keyed_many_cached(objs, mo, cache)
            assert len(res) == n
            for i, r in enumerate(res):
                if i == 4:
                    assert isinstance(r, ssa.SignatureError) and r.kind == ssa.SignatureError.InvalidSignature
                else:
                    assert r is None
            assert cache.info()["held"] == u
        assert ssa.verify_keyed_many_cached(objs[:12], mo[:12], cache)[4] is not None     # a small batch: the exact path
        assert cache.info()["held"] == u


def test_short_probe_bound(engine):
    """the wire twin of tests/test_gpu_keycache.py::test_short_probe_bound: with a probe bound of 1 lanes become keys of
    their own and rows stay unpublished, and every status is still the exact one.  (On the suite's engine; its
    dedup policy is put back whatever happens.  Run alone, the test also pays for the first use of the device through
    torch in its process, which takes seconds.)"""
    rng = np.random.default_rng(18961)
    n, u = 5000, 250
    keyed, msgs = keyed_honest(engine, rng, n, u)
    for i in range(3, n, 701):                                      # a handful of bad signatures and one bad key
        keyed[i, 99] ^= 1
    keyed[11, :49] = 0xFF
    co = coeffs32(rng, n)
    want, wnf = engine.verify_keyed_many(keyed, msgs, check_torsion=True)
    assert wnf == int((want != 0).sum()) >= 8
    engine.debug_dedup_config(-1.0, 1)
    try:
        with engine.keycache_create(1024, wire=True) as cache:
            for k in range(2):
                for form in ("host", "device"):
                    if form == "host":
                        st, nf, stats = engine.verify_keyed_many_cached(cache, keyed, msgs, coeffs=co, **T)
                    else:
                        st, nf, stats = keyed_cached_device(engine, cache, keyed, msgs, coeffs=co, **T)
                    print("probe bound 1: call", k, form, [int(v) for v in stats], cache.info())
                    assert st.tobytes() == want.tobytes() and nf == wnf          # whatever stats[7] says
                    assert int(stats[HITS]) + int(stats[INSERTED]) == int(stats[0]) >= u
                    assert cache.info()["held"] <= 1024
    finally:
        engine.debug_dedup_config()


@pytest.mark.parametrize("evict", ["clear", "recent"])
def test_affine_and_wire_caches_walk_the_same_plans(engine, evict):
    """One slice routine serves both kinds of cache: over the same keys, call after call, an affine cache and a wire
    cache of one capacity take the same plan (insert, hit, clear or compact, bypass) and hold the same number of rows.
    Every key decodes, so the distinct 49-byte strings are the distinct affine keys."""
    rng = np.random.default_rng(18971)
    n, cap = 4096, 256
    sks = make_scalars(rng, 750)
    steps = (("cold", sks[:100], (0, 100, 0, 0)), ("warm", sks[:100], (100, 0, 0, 0)),
             ("partly warm", sks[50:200], (50, 100, 0, 0)), ("overflow", sks[200:400], (0, 200, 1, 0)),
             ("bypass", sks[400:700], (0, 0, 0, 1)))
    with engine.keycache_create(cap, evict=evict) as affine, engine.keycache_create(cap, wire=True, evict=evict) as wire:
        for name, keys, plan in steps:
            keyed, msgs = keyed_honest(engine, rng, n, keys.shape[0], sks=keys)
            for i in range(5, n, 577):
                keyed[i, 99] ^= 1
            sigs, pks, inf = unpack(engine, keyed)
            assert not inf.any()
            co = coeffs32(rng, n)
            want, wnf = engine.verify_many(sigs, pks, msgs, pk_inf=inf, **T)
            assert wnf == int((want != 0).sum()) == len(range(5, n, 577))
            sa, nfa, stats_a = engine.verify_many_cached(affine, sigs, pks, msgs, coeffs=co, pk_inf=inf, **T)
            sw, nfw, stats_w = engine.verify_keyed_many_cached(wire, keyed, msgs, coeffs=co, **T)
            stats_a, stats_w = [int(v) for v in stats_a], [int(v) for v in stats_w]
            print(evict, name, stats_a, stats_w, affine.info(), wire.info())
            assert sa.tobytes() == sw.tobytes() == want.tobytes() and nfa == nfw == wnf, name
            assert stats_a[7] == 0 and stats_w[7] == 0, name
            assert stats_a[0] == stats_w[0] == keys.shape[0], name
            assert stats_a[HITS:BYPASSED + 1] == stats_w[HITS:BYPASSED + 1] == list(plan), name
            assert affine.info()["held"] == wire.info()["held"], name
        if evict == "recent":
            assert affine.eviction_info()["compactions"] == wire.eviction_info()["compactions"] == 1
