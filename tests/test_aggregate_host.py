"""Half-aggregation on the CPU: the model of tests/aggregate_model.py over both of its back-ends,
the shape of the tree, the point equation of an honest aggregate, what the transcript binds -- and the host side of the
binding: symbols, argument checks, the mirrors."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import aggregate_model as am
import pymodel as pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def make_scalars(rng, n):
    s = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    s[:, 31] &= 0x3F
    s[:, 0] |= 1
    return s


@pytest.fixture(scope="module")
def signed(oracle):
    """eight honest signatures over 80-byte messages (the C oracle signs: byte-identical to pymodel.sign)"""
    rng = np.random.default_rng(0xA66)
    n = 8
    msgs = rng.integers(0, 256, size=(n, 80), dtype=np.uint8)
    pks, sigs = oracle.keygen_sign_many(make_scalars(rng, n), make_scalars(rng, n), msgs)
    return sigs, pks, msgs


def rs_of(sigs):
    return [bytes(s)[:49] for s in sigs]


@pytest.mark.parametrize("n", [1, 2, 3, 5, 8])
def test_both_backends_give_the_same_coefficients(oracle, signed, n):
    sigs, pks, msgs = (a[:n] for a in signed)
    a_py = am.coefficients(am.pymodel_backend(), rs_of(sigs), pks, msgs)
    a_c = am.coefficients(am.oracle_backend(oracle), rs_of(sigs), pks, msgs)
    assert a_py == a_c and len(a_c) == n
    assert all(0 < a < 1 << 126 for a in a_c)
    assert am.aggregate(am.pymodel_backend(), sigs, pks, msgs) == am.aggregate(am.oracle_backend(oracle), sigs, pks, msgs)


def test_tree_shape_odd_nodes_move_up_unchanged(oracle, signed):
    be = am.oracle_backend(oracle)
    h = lambda l, r: be[0]([list(l) + list(r)])[0]
    sigs, pks, msgs = signed
    lv = am.leaves(be, rs_of(sigs), pks, msgs)
    assert am.tree_top(be, lv[:1]) == lv[0]                                   # n = 1: top = leaf_0
    assert am.tree_top(be, lv[:2]) == h(lv[0], lv[1])
    assert am.tree_top(be, lv[:3]) == h(h(lv[0], lv[1]), lv[2])
    assert am.tree_top(be, lv[:5]) == h(h(h(lv[0], lv[1]), h(lv[2], lv[3])), lv[4])       # carried two levels
    assert am.tree_top(be, lv[:6]) == h(h(h(lv[0], lv[1]), h(lv[2], lv[3])), h(lv[4], lv[5]))
    assert am.tree_top(be, lv[:7]) == h(h(h(lv[0], lv[1]), h(lv[2], lv[3])), h(h(lv[4], lv[5]), lv[6]))
    # a leaf is the digest of six felts: the raw challenge digest, the flag byte, the tag
    d = am.digest_felts(be[1](bytes(sigs[0])[:48], bytes(pks[0]), bytes(msgs[0])))
    assert lv[0] == be[0]([d + [int(sigs[0][48]), 0xA1]])[0]


@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_honest_aggregate_satisfies_the_point_equation(oracle, signed, n):
    be = am.oracle_backend(oracle)
    sigs, pks, msgs = (a[:n] for a in signed)
    agg = am.aggregate(be, sigs, pks, msgs)
    assert len(agg) == 49 * n + 32 and agg[:49 * n] == b"".join(rs_of(sigs))
    assert am.verify(be, agg, pks, msgs) == am.OK
    e = int.from_bytes(agg[-32:], "little")
    assert am.verify(be, agg[:-32] + ((e + 1) % am.Q).to_bytes(32, "little"), pks, msgs) == am.INVALID_SIGNATURE
    # the globally negated right-hand side: an x-only comparison could not tell it from the honest one
    assert am.verify(be, agg[:-32] + ((am.Q - e) % am.Q).to_bytes(32, "little"), pks, msgs) == am.INVALID_SIGNATURE
    assert am.verify(be, agg[:-32] + am.Q.to_bytes(32, "little"), pks, msgs) == am.MALFORMED


def test_empty_aggregate():
    be = am.pymodel_backend()
    assert am.aggregate(be, [], [], []) == bytes(32)
    assert am.verify(be, bytes(32), [], []) == am.OK
    assert am.verify(be, bytes([1]) + bytes(31), [], []) == am.INVALID_SIGNATURE


def test_transcript_binds_order_count_and_flag_bytes(oracle, signed):
    be = am.oracle_backend(oracle)
    sigs, pks, msgs = signed
    rs = rs_of(sigs)
    base = am.coefficients(be, rs, pks, msgs)
    differs = lambda a, b: all(x != y for x, y in zip(a, b))
    perm = [1, 0] + list(range(2, 8))                                        # two lanes swapped
    assert differs(base, am.coefficients(be, [rs[i] for i in perm], pks[perm], msgs[perm]))
    assert differs(base, am.coefficients(be, rs[:7], pks[:7], msgs[:7]))      # n changed
    flipped = list(rs)
    flipped[5] = rs[5][:48] + bytes([rs[5][48] ^ 0x40])                      # one flag byte
    assert differs(base, am.coefficients(be, flipped, pks, msgs))
    m2 = msgs.copy()
    m2[3, 79] ^= 1                                                           # one message bit
    assert differs(base, am.coefficients(be, rs, pks, m2))


def test_abi_symbols_and_argument_checks_without_a_device():
    import schnorr_sig_amd as ssa
    for name in ("ssa_aggregate_many", "ssa_aggregate_many_device", "ssa_verify_aggregate", "ssa_verify_aggregate_device",
                 "ssa_debug_aggregate_coeffs"):
        assert name in ssa.ABI_SYMBOLS
    assert ssa._lib.ssa_verify_aggregate(None, None, None, None, None, None, 0, 0, 0) == ssa.ERR_ARG
    assert ssa._lib.ssa_aggregate_many(None, None, None, None, None, None, 0, 0, 0, 0, None, None, None) == ssa.ERR_ARG
    assert ssa._lib.ssa_debug_aggregate_coeffs(None, None, None, None, None, None, 0, 0, 0, None) == ssa.ERR_ARG
    assert ssa.ABI_VERSION == 5 and ssa.AGG_CHECK == 1
    for meth in ("aggregate", "verify_aggregate", "aggregate_coeffs", "aggregate_device", "verify_aggregate_device"):
        assert callable(getattr(ssa.Engine, meth))


def test_aggregate_signature_codec():
    import schnorr_sig_amd as ssa
    a = ssa.AggregateSignature(bytes(49 * 3 + 32))
    assert len(a) == 3 and ssa.AggregateSignature.from_bytes(a.to_bytes()) == a
    assert ssa.AggregateSignature.from_bytes(bytes(33)) is None
    assert ssa.AggregateSignature.from_bytes(bytes(49) + ssa.Q.to_bytes(32, "little")) is None
    assert len(ssa.AggregateSignature.from_bytes(bytes(49) + (ssa.Q - 1).to_bytes(32, "little"))) == 1
    with pytest.raises(ValueError):
        ssa.AggregateSignature(bytes(50))
    with pytest.raises(ssa.MalformedInput):
        a.verify([], [b"m"] * 3)


def test_cxx_mirror_declares_aggregate_signature(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    src = tmp_path / "t.cpp"
    src.write_text('#include "%s/schnorr-sig_amd/host/schnorr_sig.hpp"\n'
                   "using namespace schnorr_sig;\n"
                   "Result f(Context &cx, const std::vector<Signature> &s, const std::vector<PublicKey> &p,\n"
                   "         const std::vector<std::pair<const uint8_t *, size_t>> &m) {\n"
                   "  auto a = AggregateSignature::aggregate(cx, s, p, m);\n"
                   "  auto b = AggregateSignature::from_bytes(a->to_bytes());\n"
                   "  static_assert(SSA_AGGREGATE_LENGTH(2) == 130, \"49 n + 32\");\n"
                   "  return b->verify(cx, p, m);\n"
                   "}\n" % ROOT)
    subprocess.check_call([cxx, "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", str(src)])
