"""Nonces and keys drawn on the device (ssa_keygen_sign_many_rng, ssa_sign_many_indexed_rng, ssa_signer_set_generate;
DESIGN.md section 12).  The central property: under a pinned seed the _rng forms are byte-identical to the caller-nonce
forms fed the nonces of the Python model (tests/device_rng_model.py); unpinned, every call draws fresh nonces that sign
correctly and never repeat."""
import ctypes as C
import os

import numpy as np
import pytest

import device_rng_model as model
import schnorr_sig_amd as ssa

pytestmark = pytest.mark.gpu

SEED = bytes((7 * i + 3) & 0xFF for i in range(44))
N_BIG = 2 ** 16 + 3
_NONCES = {}


def _model_nonces(n, seed=SEED):
    """the model's first n scalars under `seed` (computed once per seed, as a prefix of the largest n)"""
    have = _NONCES.get(seed)
    if have is None or have.shape[0] < n:
        have = _NONCES[seed] = model.draw(seed, np.arange(max(n, N_BIG)))
    return have[:n]


def _scalars(rng, n):
    s = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    s[:, 31] &= 0x3F
    s[:, 0] |= 1
    return s


def _messages(rng, n, ragged):
    if ragged:
        lens = rng.integers(0, 120, size=n)
        msgs = [rng.integers(0, 256, size=int(k), dtype=np.uint8).tobytes() for k in lens]
        flat, off = ssa.pack_messages(msgs)
        return flat, off
    return rng.integers(0, 256, size=(n, 37), dtype=np.uint8), None


def _refused(fn, *args, **kw):
    with pytest.raises(RuntimeError, match="invalid argument"):
        fn(*args, **kw)


@pytest.fixture
def pinned(engine):
    engine.debug_pin_rng(SEED)
    yield engine
    engine.debug_pin_rng(None)


# ---- 1. the draw rule on chosen blocks ----------------------------------------------------------------------------
def test_draw_edges_equal_the_model(engine):
    q = model.Q
    rng = np.random.default_rng(9100)
    b1 = rng.bytes(64)
    b0_values = [0, 1, q - 1, q, q + 1, 2 * q, 12345 * q, 2 ** 256, 2 ** 512 - 1,
                 (2 ** 512 - 1) // q * q, int.from_bytes(rng.bytes(64), "little")]
    blocks = [v.to_bytes(64, "little") + b1 for v in b0_values]
    blocks += [rng.bytes(128) for _ in range(500)]
    got = engine.debug_draw_scalars(np.frombuffer(b"".join(blocks), np.uint8).reshape(-1, 128))
    for row, blk in zip(got, blocks):
        assert row.tobytes() == model.draw_from_blocks(blk[:64], blk[64:])
    want_b1 = model.from_bytes_wide(b1).to_bytes(32, "little")
    for k, v in enumerate(b0_values):
        if v % q == 0:
            assert got[k].tobytes() == want_b1
    assert engine.debug_draw_scalars(np.zeros((0, 128), np.uint8)).shape == (0, 32)


# ---- 2. pinned nonces: byte-identical to the caller-nonce forms ------------------------------------------------------
@pytest.mark.parametrize("ct", [False, True])
@pytest.mark.parametrize("keyed", [False, True])
@pytest.mark.parametrize("m", [1, 64])
def test_pinned_outputs_equal_the_caller_nonce_forms(pinned, ct, keyed, m):
    engine = pinned
    rng = np.random.default_rng(9200 + 4 * m + 2 * ct + keyed)
    sks = _scalars(rng, m)
    ss = engine.signer_set_create(sks)
    try:
        for j, n in enumerate((0, 1, 63, 64, 65, 1000, N_BIG)):
            for ragged in ((False, True) if n == 1000 else (bool(j % 2),)):
                idx = rng.integers(0, m, size=n).astype(np.uint32)
                flat, off = _messages(rng, n, ragged)
                nonces = _model_nonces(n)
                kw = dict(offsets=off, constant_time=ct, keyed=keyed)
                got = engine.sign_many_indexed_rng(ss, idx, flat, **kw)
                want = engine.sign_many_indexed(ss, idx, nonces, flat, **kw) if n else got
                assert got.shape == (n, 130 if keyed else 81)
                assert (got == want).all(), (n, ragged)
                gpk, gsig = engine.keygen_sign_many_rng(sks[idx], flat, **kw)
                if n:
                    wpk, wsig = engine.keygen_sign_many(sks[idx], nonces, flat, **kw)
                    assert (gpk == wpk).all() and (gsig == wsig).all(), (n, ragged)
                    assert (gsig[:, -81:] == got[:, -81:]).all()
    finally:
        ss.close()


# ---- 3. the lane counter runs over the whole call, across slices -------------------------------------------------------
def test_lane_counter_is_global_across_the_slice_boundary(pinned):
    engine = pinned
    slice_ = engine.info()["lane_slice"]
    n = slice_ + 5
    rng = np.random.default_rng(9300)
    m = 64
    sks = _scalars(rng, m)
    ss = engine.signer_set_create(sks)
    try:
        idx = (np.arange(n) % m).astype(np.uint32)
        msgs = np.zeros((n, 8), np.uint8)
        msgs[:, :4] = np.arange(n, dtype=np.uint32).view(np.uint8).reshape(n, 4)
        got = engine.sign_many_indexed_rng(ss, idx, msgs)
        lanes = np.r_[0:3, slice_ - 3:n]
        nonces = model.draw(SEED, lanes)
        want = engine.sign_many_indexed(ss, idx[lanes], nonces, msgs[lanes])
        assert (got[lanes] == want).all()
    finally:
        ss.close()


def test_small_slices_draw_the_same_scalars(monkeypatch):
    """a context with 256-lane slices (SSA_LANE_SLICE) gives the bytes of the one-slice call"""
    monkeypatch.setenv("SSA_LANE_SLICE", "256")
    eng = ssa.Engine(0)
    try:
        assert eng.info()["lane_slice"] == 256
        eng.debug_pin_rng(SEED)
        rng = np.random.default_rng(9350)
        sks = _scalars(rng, 5)
        ss = eng.signer_set_create(sks)
        n = 1000
        idx = rng.integers(0, 5, size=n).astype(np.uint32)
        flat, off = _messages(rng, n, True)
        for ct in (False, True):
            got = eng.sign_many_indexed_rng(ss, idx, flat, offsets=off, constant_time=ct)
            assert (got == eng.sign_many_indexed(ss, idx, _model_nonces(n), flat, offsets=off, constant_time=ct)).all()
            _, gs = eng.keygen_sign_many_rng(sks[idx], flat, offsets=off, constant_time=ct, keyed=True)
            _, ws = eng.keygen_sign_many(sks[idx], _model_nonces(n), flat, offsets=off, constant_time=ct, keyed=True)
            assert (gs == ws).all()
        gen = eng.signer_set_generate(700)
        assert (eng.signer_set_secret_keys(gen) == _model_nonces(700)).all()
        gen.close()
        ss.close()
    finally:
        eng.close()


# ---- 4. unpinned draws ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ct", [False, True])
def test_unpinned_draws_verify_and_never_repeat(engine, ct):
    rng = np.random.default_rng(9400 + ct)
    m, n = 64, 2 ** 16
    sks = _scalars(rng, m)
    ss = engine.signer_set_create(sks)
    try:
        pks, _ = engine.signer_set_public_keys(ss)
        idx = rng.integers(0, m, size=n).astype(np.uint32)
        msgs = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
        a = engine.sign_many_indexed_rng(ss, idx, msgs, constant_time=ct)
        b = engine.sign_many_indexed_rng(ss, idx, msgs, constant_time=ct)
        for sigs in (a, b):
            st, nf = engine.verify_many(sigs, pks[idx], msgs)
            assert nf == 0 and not st.any()
        rx = {bytes(r[:49]) for r in np.concatenate([a, b])}
        assert len(rx) == 2 * n
        assert not (a == b).all(axis=1).any()
        pk2, s2 = engine.keygen_sign_many_rng(sks[idx[:4096]], msgs[:4096], constant_time=ct)
        st, nf = engine.verify_many(s2, pk2, msgs[:4096])
        assert nf == 0
    finally:
        ss.close()


# ---- 5. device forms -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ct", [False, True])
@pytest.mark.parametrize("keyed", [False, True])
def test_device_forms_statuses_and_pinned_equality(engine, ct, keyed):
    import torch
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(9500 + 2 * ct + keyed)
    m, n = 64, 3000
    sks = _scalars(rng, m)
    sks[5] = 0
    sks[9] = np.frombuffer(model.Q.to_bytes(32, "little"), np.uint8)
    ss = engine.signer_set_create_device(torch.from_numpy(sks.copy()).to(dev).data_ptr(), m)
    engine.debug_pin_rng(SEED)
    try:
        idx = rng.integers(0, m, size=n).astype(np.uint32)
        idx[:4] = [5, 9, m, 0xFFFFFFFF]
        flat, off = _messages(rng, n, True)
        d_idx = torch.from_numpy(idx.view(np.int32)).to(dev)
        d_msgs = torch.from_numpy(flat).to(dev)
        d_off = torch.from_numpy(off.view(np.int64)).to(dev)
        rec = 130 if keyed else 81
        d_sigs = torch.full((n, rec), 0xAA, dtype=torch.uint8, device=dev)
        d_st = torch.full((n,), 0xAA, dtype=torch.uint8, device=dev)
        d_sigs2 = torch.full((n, rec), 0xAA, dtype=torch.uint8, device=dev)
        engine.sign_many_indexed_rng_device(ss, d_idx.data_ptr(), d_msgs.data_ptr(), n, 0, d_sigs.data_ptr(),
                                            d_status=d_st.data_ptr(), msg_stride=0, d_offsets=d_off.data_ptr(),
                                            constant_time=ct, keyed=keyed)
        # ordering on the context's stream: a second call behind it, without a synchronisation in between
        engine.sign_many_indexed_rng_device(ss, d_idx.data_ptr(), d_msgs.data_ptr(), n, 0, d_sigs2.data_ptr(),
                                            msg_stride=0, d_offsets=d_off.data_ptr(), constant_time=ct, keyed=keyed)
        engine.sync()
        got, lane_st, got2 = d_sigs.cpu().numpy(), d_st.cpu().numpy(), d_sigs2.cpu().numpy()
        bad = (idx >= m) | np.isin(idx, [5, 9])
        assert (lane_st == np.where(bad, 3, 0)).all()
        assert not got[bad].any()
        assert (got2 == got).all()                              # pinned: the same draw
        keep = np.flatnonzero(~bad)
        nonces = _model_nonces(n)
        good_idx = idx.copy()
        good_idx[bad] = 0
        want = engine.sign_many_indexed(ss, good_idx, nonces, flat, offsets=off, constant_time=ct, keyed=keyed)
        assert (got[keep] == want[keep]).all()
        # keygen device form on the gathered rows equals its host form
        kidx = idx[keep]
        ks = torch.from_numpy(sks[kidx].copy()).to(dev)
        kflat, koff = ssa.pack_messages([bytes(flat[off[i]:off[i + 1]]) for i in keep])
        d_kmsgs, d_koff = torch.from_numpy(kflat).to(dev), torch.from_numpy(koff.view(np.int64)).to(dev)
        d_pk = torch.zeros((keep.size, 96), dtype=torch.uint8, device=dev)
        d_ks = torch.zeros((keep.size, rec), dtype=torch.uint8, device=dev)
        engine.keygen_sign_many_rng_device(ks.data_ptr(), d_kmsgs.data_ptr(), keep.size, 0, d_pk.data_ptr(),
                                           d_ks.data_ptr(), msg_stride=0, d_offsets=d_koff.data_ptr(),
                                           constant_time=ct, keyed=keyed)
        engine.sync()
        hpk, hsig = engine.keygen_sign_many_rng(sks[kidx], kflat, offsets=koff, constant_time=ct, keyed=keyed)
        assert (d_pk.cpu().numpy() == hpk).all() and (d_ks.cpu().numpy() == hsig).all()
    finally:
        engine.debug_pin_rng(None)
        ss.close()


# ---- 6. generated signer sets ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 64, 65536])
def test_generated_sets(engine, m):
    a = engine.signer_set_generate(m)
    b = engine.signer_set_generate(m)
    try:
        assert not engine.signer_set_status(a).any()
        sks = engine.signer_set_secret_keys(a)
        assert sks.shape == (m, 32)
        v = [int.from_bytes(r.tobytes(), "little") for r in sks[:2048]]
        assert all(0 < x < model.Q for x in v)
        pks, cpks = engine.signer_set_public_keys(a)
        assert (pks == engine.pubkey_many(sks)).all()
        assert (cpks == engine.compress_many(pks)[0]).all()
        assert not (engine.signer_set_secret_keys(b) == sks).all(axis=1).any()
        n = min(4 * m, 4096)
        rng = np.random.default_rng(9600 + m)
        idx = rng.integers(0, m, size=n).astype(np.uint32)
        msgs = rng.integers(0, 256, size=(n, 24), dtype=np.uint8)
        sigs = engine.sign_many_indexed_rng(a, idx, msgs, constant_time=True)
        st, nf = engine.verify_many(sigs, pks[idx], msgs)
        assert nf == 0
    finally:
        a.close()
        b.close()


def test_generated_set_under_a_pin_equals_the_model(pinned):
    ss = pinned.signer_set_generate(300)
    try:
        assert (pinned.signer_set_secret_keys(ss) == _model_nonces(300)).all()
    finally:
        ss.close()


# ---- 7. the Python sentinel -----------------------------------------------------------------------------------------
def test_device_rng_sentinel_signs_end_to_end(engine):
    kp = ssa.KeyPair.new(os.urandom, engine)
    for msg in (b"", b"device nonce", bytes(range(200))):
        kp.sign(msg, ssa.DEVICE_RNG, engine).verify(msg, kp.public_key, engine)
        kp.sign_and_bind_pkey(msg, ssa.DEVICE_RNG, engine).verify(msg, engine)
        kp.private_key.sign(msg, ssa.DEVICE_RNG, engine).verify(msg, kp.public_key, engine)
        kp.private_key.sign_and_bind_pkey(msg, ssa.DEVICE_RNG, engine).verify(msg, engine)
    assert kp.sign(b"x", ssa.DEVICE_RNG, engine) != kp.sign(b"x", ssa.DEVICE_RNG, engine)
    ss = ssa.SignerSet.generate(8, engine)
    try:
        pub = [ssa.PublicKey(p.tobytes()) for p in engine.signer_set_public_keys(ss)[0]]
        msgs = [b"m%d" % i for i in range(20)]
        idx = [i % 8 for i in range(20)]
        for s, k, msg in zip(ss.sign(idx, msgs, ssa.DEVICE_RNG), idx, msgs):
            s.verify(msg, pub[k], engine)
        for ks, msg in zip(ss.sign(idx, msgs, ssa.DEVICE_RNG, keyed=True), msgs):
            ks.verify(msg, engine)
        for s, k, msg in zip(ss.sign(idx, msgs, os.urandom), idx, msgs):      # a callable keeps today's path
            s.verify(msg, pub[k], engine)
        kps = [ssa.KeyPair.from_bytes(b.tobytes(), engine) for b in ss.secret_keys()]
        assert [kp.public_key for kp in kps] == pub
    finally:
        ss.close()


# ---- 8. argument errors ----------------------------------------------------------------------------------------------
def test_argument_errors(engine):
    rng = np.random.default_rng(9800)
    sks = _scalars(rng, 8)
    ss = engine.signer_set_create(sks)
    lib, ctx, P = ssa._lib, engine._ctx, ssa._ptr
    n = 16
    idx = rng.integers(0, 8, size=n).astype(np.uint32)
    msgs = rng.integers(0, 256, size=(n, 40), dtype=np.uint8)
    out = np.zeros((n, 130), np.uint8)
    pks = np.zeros((n, 96), np.uint8)
    ks = sks[idx].copy()
    chk = ssa._check
    try:
        for flags in (1, 2, 64, 1 << 31):
            _refused(chk, lib.ssa_sign_many_indexed_rng(ctx, ss.handle, P(idx), P(msgs), None, 40, 40, n, flags, P(out)), "s")
            _refused(chk, lib.ssa_keygen_sign_many_rng(ctx, P(ks), P(msgs), None, 40, 40, n, flags, P(pks), P(out)), "k")
            _refused(chk, lib.ssa_sign_many_indexed_rng_device(ctx, ss.handle, P(idx), P(msgs), None, 40, 40, n, flags,
                                                               P(out), None), "sd")
            _refused(chk, lib.ssa_keygen_sign_many_rng_device(ctx, P(ks), P(msgs), None, 40, 40, n, flags, P(pks),
                                                              P(out)), "kd")
        big = ssa.MAX_BATCH + 1 if hasattr(ssa, "MAX_BATCH") else (1 << 30) + 1
        _refused(chk, lib.ssa_sign_many_indexed_rng(ctx, ss.handle, P(idx), P(msgs), None, 40, 40, big, 0, P(out)), "s")
        _refused(chk, lib.ssa_keygen_sign_many_rng(ctx, P(ks), P(msgs), None, 40, 40, big, 0, P(pks), P(out)), "k")
        _refused(chk, lib.ssa_sign_many_indexed_rng_device(ctx, ss.handle, P(idx), P(msgs), None, 40, 40, big, 0, P(out),
                                                           None), "sd")
        _refused(chk, lib.ssa_keygen_sign_many_rng_device(ctx, P(ks), P(msgs), None, 40, 40, big, 0, P(pks), P(out)), "kd")
        _refused(chk, lib.ssa_debug_draw_scalars(ctx, P(out), big, P(out)), "draw")
        gen = C.c_void_p()
        _refused(chk, lib.ssa_signer_set_generate(ctx, big, C.byref(gen)), "gen")
        _refused(chk, lib.ssa_signer_set_generate(ctx, 0, C.byref(gen)), "gen")
        _refused(chk, lib.ssa_signer_set_generate(ctx, 4, None), "gen")
        for which in range(2):
            a = [P(idx), P(out)]
            a[which] = None
            _refused(chk, lib.ssa_sign_many_indexed_rng(ctx, ss.handle, a[0], P(msgs), None, 40, 40, n, 0, a[1]), "s")
            _refused(chk, lib.ssa_sign_many_indexed_rng_device(ctx, ss.handle, a[0], P(msgs), None, 40, 40, n, 0, a[1],
                                                               None), "sd")
        for which in range(3):
            a = [P(ks), P(pks), P(out)]
            a[which] = None
            _refused(chk, lib.ssa_keygen_sign_many_rng(ctx, a[0], P(msgs), None, 40, 40, n, 0, a[1], a[2]), "k")
            _refused(chk, lib.ssa_keygen_sign_many_rng_device(ctx, a[0], P(msgs), None, 40, 40, n, 0, a[1], a[2]), "kd")
        _refused(chk, lib.ssa_sign_many_indexed_rng(ctx, ss.handle, P(idx), None, None, 40, 40, n, 0, P(out)), "msgs")
        _refused(chk, lib.ssa_debug_draw_scalars(ctx, None, 1, P(out)), "draw")
        _refused(chk, lib.ssa_signer_set_secret_keys(ss.handle, None), "secret")
        bad_idx = idx.copy()
        bad_idx[3] = 8
        _refused(engine.sign_many_indexed_rng, ss, bad_idx, msgs)
        zero = ks.copy()
        zero[2] = 0
        _refused(engine.keygen_sign_many_rng, zero, msgs)
        eng2 = ssa.Engine(0)                         # a set belongs to its context
        try:
            _refused(eng2.sign_many_indexed_rng, ss, idx, msgs)
        finally:
            eng2.close()
    finally:
        ss.close()
    # an orphaned set: every call but destroy is refused
    eng = ssa.Engine(0)
    orphan = eng.signer_set_generate(4)
    eng.close()
    eng3 = ssa.Engine(0)
    try:
        idx4 = np.arange(4, dtype=np.uint32)
        _refused(eng3.sign_many_indexed_rng, orphan, idx4, msgs[:4])
        _refused(chk, lib.ssa_sign_many_indexed_rng_device(eng3._ctx, orphan.handle, P(idx4), P(msgs), None, 40, 40, 4,
                                                           0, P(out), None), "sd")
        _refused(eng3.signer_set_secret_keys, orphan)
    finally:
        eng3.close()
    orphan.close()
