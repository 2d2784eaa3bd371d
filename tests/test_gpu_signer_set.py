"""Signer sets (ssa_signer_set_*, ssa_sign_many_indexed[_device]): KeyPair::sign / sign_and_bind_pkey
(reference src/signature.rs:114-156) for many messages by few key pairs held on the device.  The central property: for
every valid lane the output is byte-identical to ssa_keygen_sign_many_ex (PrivateKey::sign) with the same flags on the
gathered rows sks[key_idx[i]]; a sample is checked against the CPU oracle's KeyPair::sign as well."""
import ctypes as C

import numpy as np
import pytest

import schnorr_sig_amd as ssa

pytestmark = pytest.mark.gpu

Q_LE = ssa.Q.to_bytes(32, "little")


def _scalars(rng, n):
    """n canonical non-zero scalars (below 2^254 < q)"""
    s = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    s[:, 31] &= 0x3F
    s[:, 0] |= 1
    return s


def _ragged(rng, n):
    lens = rng.integers(0, 201, size=n)
    msgs = [rng.integers(0, 256, size=int(k), dtype=np.uint8).tobytes() for k in lens]
    return msgs, ssa.pack_messages(msgs)


def _case(rng, m, n):
    sks = _scalars(rng, m)
    idx = rng.integers(0, m, size=n).astype(np.uint32)
    if n >= 2 and m >= 2:
        idx[1] = idx[0]                        # a repeated key on neighbouring lanes
    return sks, idx, _scalars(rng, n)


# ---- 1. byte equality with the existing signer ---------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 7, 64, 1000])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1000, 2 ** 16 + 3])
def test_outputs_equal_keygen_sign_on_gathered_rows(engine, m, n):
    rng = np.random.default_rng(1000 * m + n)
    sks, idx, nonces = _case(rng, m, n)
    ss = engine.signer_set_create(sks)
    try:
        assert (engine.signer_set_status(ss) == 0).all()
        msgs, (flat, off) = _ragged(rng, n)
        dense = rng.integers(0, 256, size=(n, 80), dtype=np.uint8)
        for ct in (False, True):
            for keyed in (False, True):
                for args, kw in (((flat,), {"offsets": off}), ((dense,), {})):
                    got = engine.sign_many_indexed(ss, idx, nonces, *args, constant_time=ct, keyed=keyed, **kw)
                    _, want = engine.keygen_sign_many(sks[idx], nonces, *args, constant_time=ct, keyed=keyed, **kw)
                    assert got.shape == (n, 130 if keyed else 81)
                    assert (got == want).all(), (ct, keyed, "offsets" in kw)
    finally:
        ss.close()


# ---- 2. oracle agreement, verification ---------------------------------------------------------------------------
@pytest.mark.parametrize("ct", [False, True])
def test_signatures_match_the_oracle_and_verify(engine, oracle, ct):
    rng = np.random.default_rng(2000 + ct)
    m, n = 64, 4096
    sks, idx, nonces = _case(rng, m, n)
    msgs, (flat, off) = _ragged(rng, n)
    ss = engine.signer_set_create(sks)
    try:
        pks, _ = engine.signer_set_public_keys(ss)
        sigs = engine.sign_many_indexed(ss, idx, nonces, flat, offsets=off, constant_time=ct)
        keyed = engine.sign_many_indexed(ss, idx, nonces, flat, offsets=off, constant_time=ct, keyed=True)
    finally:
        ss.close()
    for i in rng.choice(n, size=24, replace=False):
        k = idx[i]
        assert sigs[i].tobytes() == oracle.sign(sks[k].tobytes(), nonces[i].tobytes(), pks[k].tobytes(), msgs[i])
    st, nf = engine.verify_many(sigs, pks[idx], flat, offsets=off, check_torsion=True)
    assert nf == 0 and (st == 0).all()
    st, nf = engine.verify_keyed_many(keyed, flat, offsets=off, check_torsion=True)
    assert nf == 0 and (st == 0).all()
    assert (keyed[:, 49:] == sigs).all()


# ---- 3. public keys ------------------------------------------------------------------------------------------------
def test_public_keys_equal_pubkey_and_compress(engine):
    rng = np.random.default_rng(3000)
    sks = _scalars(rng, 1000)
    ss = engine.signer_set_create(sks)
    try:
        pks, cpks = engine.signer_set_public_keys(ss)
        only96, only49 = np.zeros((1000, 96), np.uint8), np.zeros((1000, 49), np.uint8)    # either output may be NULL
        ssa._check(ssa._lib.ssa_signer_set_public_keys(ss.handle, ssa._ptr(only96), None), "public_keys")
        ssa._check(ssa._lib.ssa_signer_set_public_keys(ss.handle, None, ssa._ptr(only49)), "public_keys")
        assert (only96 == pks).all() and (only49 == cpks).all()
    finally:
        ss.close()
    want = engine.pubkey_many(sks)
    assert (pks == want).all()
    cwant, cst = engine.compress_many(want)
    assert (cst == 0).all() and (cpks == cwant).all()


# ---- 4. keys derived on the device ---------------------------------------------------------------------------------
def test_derived_children_become_signers_on_the_device(engine):
    import torch
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(4000)
    parent = np.concatenate([_scalars(rng, 1)[0], rng.integers(0, 256, 32, dtype=np.uint8)])
    m = 300
    cidx = np.arange(m, dtype=np.uint32) | np.where(np.arange(m) % 2, np.uint32(0x80000000), np.uint32(0))
    d_par = torch.from_numpy(parent.copy()).to(dev)
    d_idx = torch.from_numpy(cidx.view(np.int32)).to(dev)
    d_children = torch.zeros((m, 64), dtype=torch.uint8, device=dev)
    d_st = torch.full((m,), 0xAA, dtype=torch.uint8, device=dev)
    engine.xprv_derive_many_device(d_par.data_ptr(), 1, d_idx.data_ptr(), m, d_children.data_ptr(), d_st.data_ptr())
    engine.sync()
    assert (d_st.cpu().numpy() == 0).all()
    ss = engine.signer_set_create_device(d_children.data_ptr(), m, sk_stride=64)
    try:
        assert (engine.signer_set_status(ss) == 0).all()
        pks, cpks = engine.signer_set_public_keys(ss)
        pub, pst = engine.xprv_derive_many(parent, cidx, derive_public=True)
        assert (pst == 0).all() and (cpks == pub[:, :49]).all()
        dpk, dinf, dst = engine.decompress_many(pub[:, :49])
        assert (dst == 0).all() and (dinf == 0).all() and (dpk == pks).all()
        n = 2000
        idx = rng.integers(0, m, size=n).astype(np.uint32)
        nonces = _scalars(rng, n)
        msgs = rng.integers(0, 256, size=(n, 80), dtype=np.uint8)
        for ct in (False, True):
            sigs = engine.sign_many_indexed(ss, idx, nonces, msgs, constant_time=ct)
            st, nf = engine.verify_many(sigs, dpk[idx], msgs, check_torsion=True)
            assert nf == 0 and (st == 0).all()
    finally:
        ss.close()


# ---- 5. argument and status checks ---------------------------------------------------------------------------------
def _refused(fn, *args, **kw):
    with pytest.raises(RuntimeError, match="invalid argument"):
        fn(*args, **kw)


def test_host_forms_refuse_bad_arguments(engine):
    rng = np.random.default_rng(5000)
    sks = _scalars(rng, 8)
    for bad in (np.zeros(32, np.uint8), np.frombuffer(Q_LE, np.uint8), np.full(32, 0xFF, np.uint8)):
        s = sks.copy()
        s[3] = bad
        _refused(engine.signer_set_create, s)
    _refused(engine.signer_set_create, np.zeros((0, 32), np.uint8))
    out = C.c_void_p()
    _refused(ssa._check, ssa._lib.ssa_signer_set_create(engine._ctx, None, 4, C.byref(out)), "create")
    _refused(ssa._check, ssa._lib.ssa_signer_set_create(engine._ctx, ssa._ptr(sks), 8, None), "create")
    _refused(ssa._check, ssa._lib.ssa_signer_set_create_device(engine._ctx, None, 32, 4, C.byref(out)), "create_device")
    ss = engine.signer_set_create(sks)
    try:
        n = 16
        idx = rng.integers(0, 8, size=n).astype(np.uint32)
        nonces = _scalars(rng, n)
        msgs = rng.integers(0, 256, size=(n, 40), dtype=np.uint8)
        ok = engine.sign_many_indexed(ss, idx, nonces, msgs)
        for bad in (np.zeros(32, np.uint8), np.frombuffer(Q_LE, np.uint8)):
            nn = nonces.copy()
            nn[5] = bad
            _refused(engine.sign_many_indexed, ss, idx, nn, msgs)
            _refused(engine.sign_many_indexed, ss, idx, nn, msgs, constant_time=True)
        big = idx.copy()
        big[7] = 8
        _refused(engine.sign_many_indexed, ss, big, nonces, msgs)
        flat = ssa._ptr(msgs)
        for flags in (1, 2, 64, 1 << 31):
            _refused(ssa._check, ssa._lib.ssa_sign_many_indexed(engine._ctx, ss.handle, ssa._ptr(idx), ssa._ptr(nonces),
                                                                flat, None, 40, 40, n, flags, ssa._ptr(ok)), "sign")
        for which in range(3):
            a = [ssa._ptr(idx), ssa._ptr(nonces), ssa._ptr(ok)]
            a[which] = None
            _refused(ssa._check, ssa._lib.ssa_sign_many_indexed(engine._ctx, ss.handle, a[0], a[1], flat, None, 40, 40,
                                                                n, 0, a[2]), "sign")
        _refused(ssa._check, ssa._lib.ssa_sign_many_indexed(engine._ctx, None, ssa._ptr(idx), ssa._ptr(nonces), flat,
                                                            None, 40, 40, n, 0, ssa._ptr(ok)), "sign")
        _refused(ssa._check, ssa._lib.ssa_signer_set_status(ss.handle, None), "status")
        # a set belongs to its context
        eng2 = ssa.Engine(0)
        try:
            _refused(eng2.sign_many_indexed, ss, idx, nonces, msgs)
        finally:
            eng2.close()
        # nothing above disturbed the set
        assert (engine.sign_many_indexed(ss, idx, nonces, msgs) == ok).all()
    finally:
        ss.close()


@pytest.mark.parametrize("ct", [False, True])
@pytest.mark.parametrize("keyed", [False, True])
def test_device_forms_report_unusable_keys_per_lane(engine, ct, keyed):
    import torch
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(5100 + 2 * ct + keyed)
    m, n = 64, 3000
    sks = _scalars(rng, m)
    sks[5] = 0                                               # zero key
    sks[9] = np.frombuffer(Q_LE, np.uint8)                   # non-canonical key
    ss = engine.signer_set_create_device(torch.from_numpy(sks.copy()).to(dev).data_ptr(), m)
    try:
        st = engine.signer_set_status(ss)
        want_st = np.zeros(m, np.uint8)
        want_st[[5, 9]] = 3
        assert (st == want_st).all()
        pks, cpks = engine.signer_set_public_keys(ss)
        assert not pks[[5, 9]].any() and not cpks[[5, 9]].any()
        good = np.setdiff1d(np.arange(m), [5, 9])
        assert (pks[good] == engine.pubkey_many(sks[good])).all()
        idx = rng.integers(0, m, size=n).astype(np.uint32)
        idx[:4] = [5, 9, m, 0xFFFFFFFF]
        nonces = _scalars(rng, n)
        msgs, (flat, off) = _ragged(rng, n)
        # the host form refuses the unusable keys
        _refused(engine.sign_many_indexed, ss, idx, nonces, flat, offsets=off, constant_time=ct, keyed=keyed)
        d_idx = torch.from_numpy(idx.view(np.int32)).to(dev)
        d_nonces = torch.from_numpy(nonces).to(dev)
        d_msgs = torch.from_numpy(flat).to(dev)
        d_off = torch.from_numpy(off.view(np.int64)).to(dev)
        rec = 130 if keyed else 81
        d_sigs = torch.full((n, rec), 0xAA, dtype=torch.uint8, device=dev)
        d_st = torch.full((n,), 0xAA, dtype=torch.uint8, device=dev)
        engine.sign_many_indexed_device(ss, d_idx.data_ptr(), d_nonces.data_ptr(), d_msgs.data_ptr(), n, 0,
                                        d_sigs.data_ptr(), d_status=d_st.data_ptr(), msg_stride=0,
                                        d_offsets=d_off.data_ptr(), constant_time=ct, keyed=keyed)
        d_sigs2 = torch.full((n, rec), 0xAA, dtype=torch.uint8, device=dev)
        engine.sign_many_indexed_device(ss, d_idx.data_ptr(), d_nonces.data_ptr(), d_msgs.data_ptr(), n, 0,
                                        d_sigs2.data_ptr(), msg_stride=0, d_offsets=d_off.data_ptr(),
                                        constant_time=ct, keyed=keyed)    # no status buffer
        engine.sync()
        got, lane_st, got2 = d_sigs.cpu().numpy(), d_st.cpu().numpy(), d_sigs2.cpu().numpy()
        bad = (idx >= m) | np.isin(idx, [5, 9])
        assert bad[:4].all() and bad.sum() < n
        assert (lane_st == np.where(bad, 3, 0)).all()
        assert not got[bad].any()
        assert (got2 == got).all()
        keep = np.flatnonzero(~bad)
        gflat, goff = ssa.pack_messages([msgs[i] for i in keep])
        _, want = engine.keygen_sign_many(sks[idx[keep]], nonces[keep], gflat, offsets=goff, constant_time=ct,
                                          keyed=keyed)
        assert (got[keep] == want).all()
    finally:
        ss.close()


def test_device_form_reduces_nonces_and_takes_a_stride(engine):
    import torch
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(5200)
    m, n = 7, 500
    sks = _scalars(rng, m)
    rows = np.zeros((m, 48), np.uint8)                       # stride 48: the key, then 16 bytes of other data
    rows[:, :32] = sks
    rows[:, 32:] = 0xFF
    ss = engine.signer_set_create_device(torch.from_numpy(rows).to(dev).data_ptr(), m, sk_stride=48)
    try:
        assert (engine.signer_set_status(ss) == 0).all()
        assert (engine.signer_set_public_keys(ss)[0] == engine.pubkey_many(sks)).all()
        idx = rng.integers(0, m, size=n).astype(np.uint32)
        nonces = _scalars(rng, n)
        wide = nonces.copy()                                  # nonce + q: the same scalar mod q, not canonical
        v = [int.from_bytes(x.tobytes(), "little") + ssa.Q for x in nonces[:50]]
        wide[:50] = np.frombuffer(b"".join(x.to_bytes(32, "little") for x in v), np.uint8).reshape(50, 32)
        msgs = rng.integers(0, 256, size=(n, 80), dtype=np.uint8)
        d = {k: torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(dev)
             for k, a in (("idx", idx), ("nonces", wide), ("msgs", msgs))}
        out = torch.zeros((n, 81), dtype=torch.uint8, device=dev)
        engine.sign_many_indexed_device(ss, d["idx"].data_ptr(), d["nonces"].data_ptr(), d["msgs"].data_ptr(), n, 80,
                                        out.data_ptr())
        engine.sync()
        assert (out.cpu().numpy() == engine.sign_many_indexed(ss, idx, nonces, msgs)).all()
        _refused(engine.signer_set_create_device, d["msgs"].data_ptr(), 4, sk_stride=31)
    finally:
        ss.close()


# ---- 6. lifetime ---------------------------------------------------------------------------------------------------
def test_signer_set_may_outlive_its_engine():
    eng = ssa.Engine(0)
    rng = np.random.default_rng(6000)
    sks = _scalars(rng, 4)
    ss = eng.signer_set_create(sks)
    idx = np.arange(4, dtype=np.uint32)
    nonces = _scalars(rng, 4)
    msgs = rng.integers(0, 256, size=(4, 16), dtype=np.uint8)
    eng.sign_many_indexed(ss, idx, nonces, msgs)
    assert ss.engine is eng                      # the wrapper keeps the engine alive
    eng.close()                                  # context destroyed first: the set is orphaned (keys wiped), not dangling
    eng2 = ssa.Engine(0)
    try:
        for call in (lambda: eng2.signer_set_status(ss), lambda: eng2.signer_set_public_keys(ss),
                     lambda: eng2.sign_many_indexed(ss, idx, nonces, msgs)):
            _refused(call)
        pk = np.zeros((4, 96), np.uint8)
        _refused(ssa._check, ssa._lib.ssa_signer_set_public_keys(ss.handle, ssa._ptr(pk), None), "public_keys")
    finally:
        eng2.close()
    ss.close()                                   # frees the host handle only; no use-after-free
    ss.close()


# ---- 7. the object mirror ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ct", [False, True])
def test_mirror_signer_set_signs_for_its_key_pairs(engine, ct):
    import random
    r = random.Random(7000 + ct)

    def rng(k):
        return bytes(r.randrange(256) for _ in range(k))

    pairs = [ssa.KeyPair.new(rng, engine) for _ in range(5)]
    ss = ssa.SignerSet.from_key_pairs(pairs, engine)
    try:
        idx = [0, 4, 4, 2, 1, 3, 0]
        msgs = [b"", b"a", b"deposit sweep", bytes(range(200)), b"x" * 7, b"y" * 14, b"z" * 99]
        sigs = ss.sign(idx, msgs, rng, constant_time=ct)
        assert all(isinstance(s, ssa.Signature) for s in sigs)
        for k, m, s in zip(idx, msgs, sigs):
            assert s.verify(m, pairs[k].public_key, engine) is None
        keyed = ss.sign(idx, msgs, rng, constant_time=ct, keyed=True)
        for k, m, ks in zip(idx, msgs, keyed):
            assert isinstance(ks, ssa.KeyedSignature) and ks.public_key == pairs[k].public_key
            b = ks.to_bytes(engine)
            back = ssa.KeyedSignature.from_bytes(b, engine)
            assert back == ks and back.verify(m, engine) is None
        assert ss.sign([], [], rng) == []
    finally:
        ss.close()
