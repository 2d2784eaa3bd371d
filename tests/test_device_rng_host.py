"""Device-drawn nonces and keys, the parts that need no GPU: the Python model of the draw
(tests/device_rng_model.py) against RFC 8439 and the reference's from_bytes_wide, the new C ABI symbols, and the argument
checks of the C ABI and of the mirrors."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import device_rng_model as model
import schnorr_sig_amd as ssa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("ssa_keygen_sign_many_rng", "ssa_keygen_sign_many_rng_device", "ssa_sign_many_indexed_rng",
               "ssa_sign_many_indexed_rng_device", "ssa_signer_set_generate", "ssa_signer_set_secret_keys",
               "ssa_debug_pin_rng", "ssa_debug_draw_scalars")


# ---- the model --------------------------------------------------------------------------------------------------
def test_chacha20_model_reproduces_rfc8439_block():
    assert model.chacha20_block(model.RFC8439_KEY, 1, model.RFC8439_NONCE) == model.RFC8439_BLOCK1   # section 2.3.2


def test_vectorised_blocks_equal_single_blocks():
    key, nonce = bytes(range(100, 132)), bytes(range(12))
    many = model.chacha20_blocks(key, [0, 1, 7, 2 ** 31, 2 ** 32 - 1], nonce)
    for row, ctr in zip(many, [0, 1, 7, 2 ** 31, 2 ** 32 - 1]):
        assert row.tobytes() == model.chacha20_block(key, ctr, nonce)


def test_from_bytes_wide_edges():
    q = model.Q
    le = lambda v: v.to_bytes(64, "little")
    assert model.from_bytes_wide(le(0)) == 0
    assert model.from_bytes_wide(le(q)) == 0 and model.from_bytes_wide(le(5 * q)) == 0
    assert model.from_bytes_wide(le(q + 1)) == 1 and model.from_bytes_wide(le(q - 1)) == q - 1
    assert model.from_bytes_wide(le(2 ** 512 - 1)) == (2 ** 512 - 1) % q
    assert model.from_bytes_wide(le(2 ** 256)) == 2 ** 256 % q
    # the same rule as PrivateKey::from_seed (src/private.rs:79-82) in the mirror
    seed = bytes(range(64))
    assert ssa.PrivateKey.from_seed(seed).to_bytes() == model.from_bytes_wide(seed).to_bytes(32, "little")


def test_draw_rule_falls_back_to_the_second_block_only_at_zero():
    q = model.Q
    b1 = bytes(range(64))
    want1 = model.from_bytes_wide(b1).to_bytes(32, "little")
    for zero in (0, q, 7 * q):
        assert model.draw_from_blocks(zero.to_bytes(64, "little"), b1) == want1
    assert model.draw_from_blocks((q + 3).to_bytes(64, "little"), b1) == (3).to_bytes(32, "little")


def test_draw_layout_lane_i_uses_blocks_2i_and_2i_plus_1():
    seed = bytes(range(44))
    got = model.draw(seed, [0, 1, 1000])
    for row, lane in zip(got, [0, 1, 1000]):
        b0 = model.chacha20_block(seed[:32], 2 * lane, seed[32:])
        b1 = model.chacha20_block(seed[:32], 2 * lane + 1, seed[32:])
        assert row.tobytes() == model.draw_from_blocks(b0, b1)
        assert 0 < int.from_bytes(row.tobytes(), "little") < model.Q


# ---- the C ABI ----------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "schnorr_sig_amd.h")).read()
    lib = C.CDLL(ssa.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name + "(" in hdr, name
        assert hasattr(lib, name), name
        assert name in ssa.ABI_SYMBOLS, name
    assert ssa._lib.ssa_abi_version() == 5


def test_null_context_and_handles_are_refused_without_a_device():
    lib = ssa._lib
    buf = (C.c_uint8 * 256)()
    out = C.c_void_p()
    assert lib.ssa_keygen_sign_many_rng(None, buf, buf, None, 1, 1, 1, 0, buf, buf) == ssa.ERR_ARG
    assert lib.ssa_keygen_sign_many_rng_device(None, buf, buf, None, 1, 1, 1, 0, buf, buf) == ssa.ERR_ARG
    assert lib.ssa_sign_many_indexed_rng(None, None, buf, buf, None, 1, 1, 1, 0, buf) == ssa.ERR_ARG
    assert lib.ssa_sign_many_indexed_rng_device(None, None, buf, buf, None, 1, 1, 1, 0, buf, None) == ssa.ERR_ARG
    assert lib.ssa_signer_set_generate(None, 4, C.byref(out)) == ssa.ERR_ARG
    assert lib.ssa_signer_set_secret_keys(None, buf) == ssa.ERR_ARG
    assert lib.ssa_debug_pin_rng(None, buf) == ssa.ERR_ARG
    assert lib.ssa_debug_draw_scalars(None, buf, 1, buf) == ssa.ERR_ARG


# ---- the mirrors ----------------------------------------------------------------------------------------------------
def test_device_rng_sentinel_yields_no_host_bytes():
    assert repr(ssa.DEVICE_RNG) == "DEVICE_RNG"
    with pytest.raises(TypeError):
        ssa.DEVICE_RNG(64)
    with pytest.raises(TypeError):                 # a host draw through the sentinel is an error, never silent bytes
        ssa.PrivateKey.new(ssa.DEVICE_RNG)


def test_signer_set_sign_checks_lengths_before_any_device_work():
    ss = ssa.SignerSet(None, None, 4)
    with pytest.raises(ValueError):
        ss.sign([0, 1], [b"a"], ssa.DEVICE_RNG)
    ss.handle = None


def test_debug_pin_rng_wants_44_bytes():
    eng = object.__new__(ssa.Engine)           # no context: the length check comes first
    eng._ctx = C.c_void_p()
    with pytest.raises(ValueError):
        eng.debug_pin_rng(b"\0" * 43)


def test_cxx_mirror_declares_the_device_rng_overloads(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    src = tmp_path / "t.cpp"
    src.write_text('#include "%s/schnorr-sig_amd/host/schnorr_sig.hpp"\n'
                   "using namespace schnorr_sig;\n"
                   "void f(Context &cx, const KeyPair &kp, const PrivateKey &sk, Rng rng) {\n"
                   "  SignerSet g(cx, 64, device_rng);\n"
                   "  std::vector<std::pair<const uint8_t *, size_t>> msgs;\n"
                   "  std::vector<Signature> a = g.sign({}, msgs, device_rng);\n"
                   "  std::vector<KeyedSignature> b = g.sign_and_bind_pkey({}, msgs, device_rng);\n"
                   "  std::vector<std::array<uint8_t, KEY_PAIR_LENGTH>> k = g.secret_keys();\n"
                   "  Signature c = kp.sign(cx, nullptr, 0, device_rng);\n"
                   "  KeyedSignature d = kp.sign_and_bind_pkey(cx, nullptr, 0, device_rng);\n"
                   "  Signature e = sk.sign(cx, nullptr, 0, device_rng);\n"
                   "  KeyedSignature h = sk.sign_and_bind_pkey(cx, nullptr, 0, device_rng);\n"
                   "  Signature i = kp.sign(cx, nullptr, 0, rng);\n"
                   "  (void)a; (void)b; (void)k; (void)c; (void)d; (void)e; (void)h; (void)i;\n"
                   "}\n" % ROOT)
    subprocess.check_call([cxx, "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", str(src)])
