"""Hierarchical key derivation on the GPU (ssa_derive.hpp; reference src/derivation.rs) against the independent model
tests/derive_model.py (hmac / hashlib + oracle/pymodel.py).  The model's point arithmetic costs ~40 ms per product,
so whole batches are checked through the exact HMAC side of the model (child scalars, chain codes, statuses) plus the
library's tested base multiplication (ssa_pubkey_many / ssa_compress_many), and a sample of each batch through the
model's own points."""
import hashlib
import hmac
import random

import numpy as np
import pytest

import derive_model as dm
import schnorr_sig_amd as ssa

pytestmark = pytest.mark.gpu

H = dm.HARDENED


def _seed(rng):
    return bytes(rng.randrange(256) for _ in range(32))


def _u8(b):
    return np.frombuffer(bytes(b), np.uint8)


def _master(seed):
    sk, cc = dm.master(seed)
    return sk, cc, dm.pt_compress(dm.pub(sk))


def _indices(rng, n):
    fixed = [0, 1, H - 1, H, 2 ** 32 - 1]
    rest = [rng.randrange(0, H) if k % 2 else rng.randrange(H, 2 ** 32) for k in range(n - len(fixed))]
    return np.array(fixed + rest, dtype=np.uint32)


def _model_children(parents, pidx, idx):
    """parents: list of (sk, cc, pk49) -> expected n x 64 bytes and statuses"""
    out = np.zeros((len(idx), 64), np.uint8)
    st = np.zeros(len(idx), np.uint8)
    for k, (p, i) in enumerate(zip(pidx, idx)):
        sk, cc, pk49 = parents[p]
        r = dm.derive_private(sk, cc, int(i), pk49)
        if r is None:
            st[k] = 1
        else:
            out[k] = _u8(dm.xprv_bytes(*r))
    return out, st


# ---- 1. SHA-512 / HMAC on its own -------------------------------------------------------------------------------
RFC4231 = [   # (key, data) of RFC 4231 test cases 1-7
    (b"\x0b" * 20, b"Hi There"),
    (b"Jefe", b"what do ya want for nothing?"),
    (b"\xaa" * 20, b"\xdd" * 50),
    (bytes(range(1, 26)), b"\xcd" * 50),
    (b"\x0c" * 20, b"Test With Truncation"),
    (b"\xaa" * 131, b"Test Using Larger Than Block-Size Key - Hash Key First"),
    (b"\xaa" * 131, b"This is a test using a larger than block-size key and a larger than block-size data. The key needs "
                    b"to be hashed before being used by the HMAC algorithm."),
]


def test_hmac_sha512_rfc4231(engine):
    for key, data in RFC4231:
        got = engine.debug_hmac_sha512(key, _u8(data))[0].tobytes()
        assert got == hmac.new(key, data, hashlib.sha512).digest(), key
    got = engine.debug_hmac_sha512(b"\x0b" * 20, _u8(b"Hi There"))[0].tobytes()
    assert got.hex() == ("87aa7cdea5ef619d4ff0b4241a1d6cb02379f4e2ce4ec2787ad0b30545e17cde"
                         "daa833b7d6b8a702038b274eaea3f4e4be9d914eeb61f1702e696c203a126854")


@pytest.mark.parametrize("mlen", [0, 1, 111, 112, 127, 128, 200, 239])
def test_hmac_sha512_random(engine, mlen):
    rng = np.random.default_rng(0x5A512 + mlen)
    for klen in (0, 1, 32, 34, 128, 129, 256):
        key = rng.integers(0, 256, klen, dtype=np.uint8).tobytes()
        msgs = rng.integers(0, 256, (67, mlen), dtype=np.uint8)
        got = engine.debug_hmac_sha512(key, msgs)
        for k in range(67):
            assert got[k].tobytes() == hmac.new(key, msgs[k].tobytes(), hashlib.sha512).digest(), (klen, mlen, k)


# ---- 2. master keys -----------------------------------------------------------------------------------------------
def test_master_keys_equal_model(engine):
    rng = np.random.default_rng(0x3A57E)
    seeds = rng.integers(0, 256, (4096, 32), dtype=np.uint8)
    out, st = engine.xprv_master_many(seeds)
    assert (st == 0).all()
    for k in range(4096):
        sk, cc = dm.master(seeds[k].tobytes())
        assert out[k].tobytes() == dm.xprv_bytes(sk, cc), k


# ---- 3. / 4. private and public children ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def one_parent():
    rng = random.Random(0xC41D)
    sk, cc, pk49 = _master(_seed(rng))
    return sk, cc, pk49, _indices(rng, 8192)


def test_xprv_children_of_one_parent(engine, one_parent):
    sk, cc, pk49, idx = one_parent
    got, st = engine.xprv_derive_many(_u8(dm.xprv_bytes(sk, cc)), idx)
    want, wst = _model_children([(sk, cc, pk49)], [0] * len(idx), idx)
    assert (st == wst).all() and (got == want).all()


def test_xprv_children_of_ragged_parents(engine):
    rng = random.Random(0x37)
    parents = [_master(_seed(rng)) for _ in range(37)]
    n = 3000
    pidx = np.array([rng.randrange(37) for _ in range(n)], np.uint32)
    pidx[:37] = np.arange(37)
    idx = _indices(rng, n)
    par = np.stack([_u8(dm.xprv_bytes(sk, cc)) for sk, cc, _ in parents])
    got, st = engine.xprv_derive_many(par, idx, parent_idx=pidx)
    want, wst = _model_children(parents, pidx, idx)
    assert (st == wst).all() and (got == want).all()
    # m == n without a table: lane i derives from parent i
    got2, st2 = engine.xprv_derive_many(par, idx[:37])
    want2, _ = _model_children(parents, list(range(37)), idx[:37])
    assert (st2 == 0).all() and (got2 == want2).all()


def test_xprv_to_xpub_children(engine, one_parent):
    sk, cc, pk49, idx = one_parent
    xprv = _u8(dm.xprv_bytes(sk, cc))
    priv, _ = engine.xprv_derive_many(xprv, idx)
    pub, st = engine.xprv_derive_many(xprv, idx, derive_public=True)
    assert (st == 0).all()
    comp, cst = engine.compress_many(engine.pubkey_many(priv[:, :32]))
    assert (cst == 0).all()
    assert (pub[:, :49] == comp).all() and (pub[:, 49:] == priv[:, 32:]).all()
    for k in list(range(5)) + random.Random(1).sample(range(5, len(idx)), 11):   # the model's own points
        p, c = dm.derive_public(sk, cc, int(idx[k]), pk49)
        assert pub[k].tobytes() == dm.xpub_bytes(p, c), k


def test_xpub_children(engine, one_parent):
    sk, cc, pk49, idx = one_parent
    xpub = _u8(pk49 + cc)
    got, pks, inf, st = engine.xpub_derive_many(xpub, idx)
    hard = idx >= H
    assert (st[hard] == 1).all() and not got[hard].any() and not pks[hard].any() and not inf.any()
    assert (st[~hard] == 0).all()
    via_xprv, _ = engine.xprv_derive_many(_u8(dm.xprv_bytes(sk, cc)), idx, derive_public=True)
    assert (got[~hard] == via_xprv[~hard]).all()
    dpks, dinf, dst = engine.decompress_many(got[~hard][:, :49].copy())
    assert (dst == 0).all() and (dpks == pks[~hard]).all()
    pk = dm.pub(sk)
    soft = np.nonzero(~hard)[0]
    for k in list(soft[:3]) + random.Random(2).sample(list(soft[3:]), 9):
        p, c = dm.derive_normal_public(pk, cc, int(idx[k]))
        assert got[k].tobytes() == dm.xpub_bytes(p, c), k
    # the context's workspace count includes the per-parent records (384 B each), the one context buffer the device
    # form reserves (no constant-time table on the public side, no staging)
    import torch
    dev = torch.device("cuda", 0)
    m = 2 ** 16
    eng = ssa.Engine(0)
    try:
        d_par = torch.from_numpy(np.tile(xpub, (m, 1))).to(dev)
        d_idx = torch.arange(m, dtype=torch.int32, device=dev)
        d_out, d_st = (torch.empty(shape, dtype=torch.uint8, device=dev) for shape in ((m, 81), (m,)))
        before = eng.info()["workspace_bytes"]
        eng.xpub_derive_many_device(d_par.data_ptr(), m, d_idx.data_ptr(), m, d_out.data_ptr(), d_st.data_ptr())
        eng.sync()
        assert eng.info()["workspace_bytes"] - before >= m * 384
    finally:
        eng.close()


# ---- 5. the pinned case ---------------------------------------------------------------------------------------------
# m/0'/1'/2' from the seed 00 01 .. 1f: HMAC-SHA512 and arithmetic mod q only (no G, no Rescue); the values were
# produced by tests/derive_model.py and are what any implementation of the reference's hardened path must give
HARDENED_CHAIN = [
    "1f24ff0c1b51991314cc52867b7e6a4203bfe28f545926e210fbadc75841cf5bcd8078832a988c34fec29e175a04ba0ff0af4e02d40feea703ae783ea4582362",
    "83330773426dfc624a91e027bd6cce6cd1919b952751d48bdc040473bcfbc95782c72800be02f690d0e56a5d81f88fce481c259cb855316bcd763cafa81556a2",
    "9f8173d830ce5b835b7d4203bf2340bd53f1c1b8da1d1cfe3c72a4b9b4c2ea5d02c5224d8af11b3fe590a9f255dba9c78bc82515d7aff8740878990482d02159",
    "d0a2ec0335ff92f44de0ca8dd59033b582ffb9266be21ef4f90cd91bdc38fa1475e822e711f963331be9fcf2956e9840f0f0416a1683035c258f3acf3e427465",
]


def test_hardened_chain_is_pinned(engine):
    seed = bytes(range(32))
    out, st = engine.xprv_master_many(_u8(seed))
    assert st[0] == 0 and out[0].tobytes().hex() == HARDENED_CHAIN[0]
    cur = out[0]
    for k in range(3):
        cur, st = engine.xprv_derive_many(cur, [H + k])
        cur = cur[0]
        assert st[0] == 0 and cur.tobytes().hex() == HARDENED_CHAIN[k + 1]
    # the model gives the same chain
    sk, cc = dm.master(seed)
    for k in range(3):
        sk, cc = dm.derive_private(sk, cc, H + k)
    assert dm.xprv_bytes(sk, cc).hex() == HARDENED_CHAIN[3]


# ---- 6. malformed parents -------------------------------------------------------------------------------------------
def test_malformed_parents_only_their_lanes(engine):
    rng = random.Random(0xBAD)
    sk, cc, pk49 = _master(_seed(rng))
    good_pub = pk49 + cc
    bad_flag = pk49[:48] + bytes([pk49[48] | 0x01]) + cc
    identity = bytes(48) + b"\x80" + cc
    noncanon = (2 ** 64 - 2 ** 32 + 1).to_bytes(8, "little") + pk49[8:] + cc       # limb 0 = p: not canonical
    undecodable = b"\xff" * 48 + b"\x00" + cc
    pubs = np.stack([_u8(x) for x in (good_pub, bad_flag, identity, noncanon, undecodable)])
    pidx = np.array([0, 1, 2, 3, 4, 0, 5, 0], np.uint32)
    idx = np.array([7, 7, 7, 7, 7, 8, 9, H], np.uint32)
    got, pks, inf, st = engine.xpub_derive_many(pubs, idx, parent_idx=pidx)
    assert list(st) == [0, 3, 3, 3, 3, 0, 3, 1]
    assert not got[[1, 2, 3, 4, 6, 7]].any() and not pks[[1, 2, 3, 4, 6, 7]].any()
    assert got[0].any() and got[5].any()
    good_prv = dm.xprv_bytes(sk, cc)
    prvs = np.stack([_u8(x) for x in (good_prv, bytes(32) + cc, b"\xff" * 32 + cc, dm.Q.to_bytes(32, "little") + cc)])
    pidx = np.array([0, 1, 2, 3, 0, 4, 0], np.uint32)
    idx = np.array([5, 5, 5, H + 5, H + 5, 5, 6], np.uint32)
    for pub in (False, True):
        got, st = engine.xprv_derive_many(prvs, idx, parent_idx=pidx, derive_public=pub)
        assert list(st) == [0, 3, 3, 3, 0, 3, 0], pub
        assert not got[[1, 2, 3, 5]].any() and got[[0, 4, 6]].any(axis=1).all()
    got, st = engine.xprv_derive_many(prvs[:1], idx[:1])
    want, _ = _model_children([(sk, cc, pk49)], [0], idx[:1])
    assert (got == want).all()


def test_argument_checks(engine):
    xprv = np.zeros((2, 64), np.uint8)
    with pytest.raises(RuntimeError):          # no table: m must be 1 or n
        engine.xprv_derive_many(xprv, [1, 2, 3])
    with pytest.raises(RuntimeError):
        engine.debug_hmac_sha512(b"k" * 257, np.zeros((1, 1), np.uint8))
    with pytest.raises(RuntimeError):
        engine.debug_hmac_sha512(b"k", np.zeros((1, 240), np.uint8))


# ---- 7. batch sizes, device forms -----------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1000, 2 ** 16 + 3])
def test_batch_sizes_and_device_forms(engine, n):
    import torch
    dev = torch.device("cuda", 0)
    rng = random.Random(n)
    sk, cc, pk49 = _master(_seed(rng))
    idx = np.array([rng.randrange(2 ** 32) for _ in range(n)], np.uint32)
    xprv, xpub = _u8(dm.xprv_bytes(sk, cc)), _u8(pk49 + cc)
    got, st = engine.xprv_derive_many(xprv, idx)
    assert got.shape == (n, 64) and st.shape == (n,)
    if n == 0:
        return
    want, wst = _model_children([(sk, cc, pk49)], [0] * n, idx)
    assert (st == wst).all() and (got == want).all()
    pub, pst = engine.xprv_derive_many(xprv, idx, derive_public=True)
    xch, xpk, xinf, xst = engine.xpub_derive_many(xpub, idx)
    seeds = np.frombuffer(bytes(rng.randrange(256) for _ in range(32 * n)), np.uint8).reshape(n, 32)
    mst_out, mst_st = engine.xprv_master_many(seeds)
    d_idx = torch.from_numpy(idx.view(np.int32)).to(dev)
    d_prv, d_pub = torch.from_numpy(xprv.copy()).to(dev), torch.from_numpy(xpub.copy()).to(dev)
    d_seeds = torch.from_numpy(seeds.copy()).to(dev)

    def buf(*shape):
        return torch.full(shape, 0xAA, dtype=torch.uint8, device=dev)

    o1, s1, o2, s2, o3, p3, i3, s3, o4, s4 = (buf(n, 64), buf(n), buf(n, 81), buf(n), buf(n, 81), buf(n, 96), buf(n),
                                              buf(n), buf(n, 64), buf(n))
    engine.xprv_derive_many_device(d_prv.data_ptr(), 1, d_idx.data_ptr(), n, o1.data_ptr(), s1.data_ptr())
    engine.xprv_derive_many_device(d_prv.data_ptr(), 1, d_idx.data_ptr(), n, o2.data_ptr(), s2.data_ptr(),
                                   derive_public=True)
    engine.xpub_derive_many_device(d_pub.data_ptr(), 1, d_idx.data_ptr(), n, o3.data_ptr(), s3.data_ptr(),
                                   d_pks=p3.data_ptr(), d_pk_inf=i3.data_ptr())
    engine.xprv_master_many_device(d_seeds.data_ptr(), n, o4.data_ptr(), s4.data_ptr())
    engine.sync()
    c = lambda t: t.cpu().numpy()   # noqa: E731
    assert (c(o1) == got).all() and (c(s1) == st).all()
    assert (c(o2) == pub).all() and (c(s2) == pst).all()
    assert (c(o3) == xch).all() and (c(p3) == xpk).all() and (c(i3) == xinf).all() and (c(s3) == xst).all()
    assert (c(o4) == mst_out).all() and (c(s4) == mst_st).all()
    soft = idx < H
    assert (xch[soft] == pub[soft]).all()
    for k in range(min(n, 64)):
        assert mst_out[k].tobytes() == dm.xprv_bytes(*dm.master(seeds[k].tobytes()))


# ---- 8. derived keys sign and verify --------------------------------------------------------------------------------
def test_derived_keys_sign_and_verify(engine):
    rng = random.Random(0xE2E)
    sk, cc, pk49 = _master(_seed(rng))
    n = 4096
    idx = np.array([rng.randrange(H) for _ in range(n)], np.uint32)
    priv, st = engine.xprv_derive_many(_u8(dm.xprv_bytes(sk, cc)), idx)
    assert (st == 0).all()
    xch, pks, inf, xst = engine.xpub_derive_many(_u8(pk49 + cc), idx)
    assert (xst == 0).all() and not inf.any()
    nrng = np.random.default_rng(8)
    nonces = np.frombuffer(b"".join((int.from_bytes(nrng.bytes(64), "little") % (dm.Q - 1) + 1).to_bytes(32, "little")
                                    for _ in range(n)), np.uint8).reshape(n, 32)
    msgs = nrng.integers(0, 256, (n, 40), dtype=np.uint8)
    spks, sigs = engine.keygen_sign_many(priv[:, :32].copy(), nonces, msgs, constant_time=True)
    assert (spks == pks).all()
    status, nfail = engine.verify_many(sigs, pks, msgs, check_torsion=True)
    assert nfail == 0 and (status == 0).all()
    sigs[1234, 60] ^= 1
    status, nfail = engine.verify_many(sigs, pks, msgs, check_torsion=True)
    assert nfail == 1 and status[1234] != 0 and (np.delete(status, 1234) == 0).all()


# ---- 9. the Python mirror: the reference's key_derivation scenario (tests/schnorr.rs:185-262) --------------------
def test_mirror_key_derivation_scenario(engine):
    import os
    rng = os.urandom
    key_pair = ssa.KeyPair.new(rng, engine)
    cc = ssa.ChainCode(rng(32))
    priv_child, priv_cc = key_pair.private_key.derive_private(cc, bytes([1, 0, 0, 0]), engine)
    pub_child, pub_cc = key_pair.public_key.derive_public(cc, bytes([1, 0, 0, 0]), engine)
    assert ssa.PublicKey.from_private(priv_child, engine) == pub_child
    assert priv_cc == pub_cc
    with pytest.raises(ssa.MalformedInput):     # the reference unwraps a none CtOption: a hardened index panics
        key_pair.public_key.derive_public(cc, bytes([0, 0, 0, 0x80]), engine)

    master = ssa.ExtendedPrivateKey.generate_master_key(rng(32), engine)
    master_pub = ssa.ExtendedPublicKey.from_extended_private_key(master, engine)
    index = bytes([1, 0, 0, 0])
    private_child = master.derive_private(index, engine)
    public_child = master.derive_public(index, engine)
    public_child2 = master_pub.derive_normal_public(index, engine)
    assert ssa.ExtendedPublicKey.from_extended_private_key(private_child, engine) == public_child
    assert public_child == public_child2
    index = bytes([255, 255, 255, 255])
    private_child = master.derive_private(index, engine)
    public_child = master.derive_public(index, engine)
    assert ssa.ExtendedPublicKey.from_extended_private_key(private_child, engine) == public_child
    assert master_pub.derive_normal_public(index, engine) is None
    pb, qb = private_child.to_bytes(), public_child.to_bytes(engine)
    assert len(pb) == ssa.EXTENDED_PRIVATE_KEY_LENGTH and len(qb) == ssa.EXTENDED_PUBLIC_KEY_LENGTH
    assert ssa.ExtendedPrivateKey.from_bytes(pb) == private_child
    assert ssa.ExtendedPublicKey.from_bytes(qb, engine) == public_child
    assert ssa.ExtendedPublicKey.from_bytes(bytes(48) + b"\x80" + bytes(32), engine) is None     # the identity
    # int indices are the same indices
    assert master.derive_private(2 ** 32 - 1, engine) == private_child
