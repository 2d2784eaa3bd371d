"""Hierarchical key derivation on the host: the ExtendedPrivateKey codecs of the Python mirror (they stay on the host)
against the reference's fixtures (src/derivation.rs tests), and the independent model (tests/derive_model.py) against
itself, as the reference's test_derive does."""
import os
import random

import schnorr_sig_amd as ssa
import derive_model as dm


def test_extended_private_key_encoding_fixture():
    # src/derivation.rs tests: {key: 1, chaincode: [1; 32]}
    xsk = ssa.ExtendedPrivateKey(ssa.PrivateKey((1).to_bytes(32, "little")), ssa.ChainCode(bytes([1] * 32)))
    b = xsk.to_bytes()
    assert b == bytes([1]) + bytes(31) + bytes([1] * 32)
    assert len(b) == ssa.EXTENDED_PRIVATE_KEY_LENGTH == 64
    assert ssa.ExtendedPrivateKey.from_bytes(b) == xsk


def test_extended_private_key_invalid_encodings():
    assert ssa.ExtendedPrivateKey.from_bytes(bytes(64)) is None                      # key 0
    assert ssa.ExtendedPrivateKey.from_bytes(b"\xff" * 32 + bytes(32)) is None       # key >= q
    assert ssa.ExtendedPrivateKey.from_bytes(dm.Q.to_bytes(32, "little") + bytes(32)) is None
    assert ssa.ExtendedPrivateKey.from_bytes((dm.Q - 1).to_bytes(32, "little") + bytes(32)) is not None


def test_extended_private_key_round_trip():
    rng = random.Random(0xD3E1)
    for _ in range(100):
        sk = rng.randrange(1, dm.Q)
        cc = bytes(rng.randrange(256) for _ in range(32))
        xsk = ssa.ExtendedPrivateKey(ssa.PrivateKey(sk.to_bytes(32, "little")), cc)
        b = xsk.to_bytes()
        assert b == dm.xprv_bytes(sk, cc)
        assert ssa.ExtendedPrivateKey.from_bytes(b) == xsk


def test_constants_and_index_forms():
    assert (ssa.CHAIN_CODE_LENGTH, ssa.EXTENDED_PUBLIC_KEY_LENGTH, ssa.FLAG_DERIVE_PUBLIC) == (32, 81, 64)
    assert ssa._index_bytes(1) == ssa._index_bytes(b"\x01\x00\x00\x00") == 1
    assert ssa._index_bytes(b"\xff\xff\xff\xff") == 2 ** 32 - 1
    assert ssa._index_bytes(bytes([0, 0, 0, 0x80])) == 2 ** 31


def test_model_derive_paths_agree():
    """src/derivation.rs test_derive: derive_private -> public == derive_public == derive_normal_public for random
    non-hardened indices; the public side refuses hardened ones"""
    rng = random.Random(int.from_bytes(os.urandom(4), "little"))
    seed = bytes(rng.randrange(256) for _ in range(32))
    m = dm.master(seed)
    assert m is not None
    sk, cc = m
    pk = dm.pub(sk)
    pk49 = dm.pt_compress(pk)
    for _ in range(100):
        i = rng.randrange(0, dm.HARDENED)
        child_sk, child_cc = dm.derive_private(sk, cc, i, pk49)
        p1 = dm.pub(child_sk)
        p2, cc2 = dm.derive_public(sk, cc, i, pk49)
        p3, cc3 = dm.derive_normal_public(pk, cc, i)
        assert p1 == p2 == p3
        assert child_cc == cc2 == cc3
    for i in (dm.HARDENED, 2 ** 32 - 1, rng.randrange(dm.HARDENED, 2 ** 32)):
        assert dm.derive_normal_public(pk, cc, i) is None
        assert dm.derive_private(sk, cc, i) is not None


def test_cxx_mirror_declares_the_derivation_types(tmp_path):
    """the C++ mirror (schnorr-sig_amd/host/schnorr_sig.hpp) compiles with the derivation types and their methods"""
    import shutil
    import subprocess
    import pytest
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "t.cpp"
    src.write_text('#include "%s/schnorr-sig_amd/host/schnorr_sig.hpp"\n'
                   "using namespace schnorr_sig;\n"
                   "void f(Context &cx, const ExtendedPrivateKey &x, const ExtendedPublicKey &p, const Index &i) {\n"
                   "  auto a = ExtendedPrivateKey::generate_master_key(cx, std::array<uint8_t, 32>{});\n"
                   "  auto b = x.derive_private(cx, i); auto c = x.derive_public(cx, i);\n"
                   "  auto d = p.derive_normal_public(cx, i); auto e = ExtendedPublicKey::from_extended_private_key(cx, x);\n"
                   "  auto g = derive_private(cx, x.key, x.chaincode, i); auto h = derive_public(cx, p.key, p.chaincode, i);\n"
                   "  auto k = ExtendedPrivateKey::from_bytes(x.to_bytes()); auto l = ExtendedPublicKey::from_bytes(cx, p.to_bytes(cx));\n"
                   "  (void)a; (void)b; (void)c; (void)d; (void)e; (void)g; (void)h; (void)k; (void)l;\n"
                   "}\n" % root)
    subprocess.check_call([cxx, "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", str(src)])
