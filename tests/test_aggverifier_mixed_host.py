"""A block against the pool (ssa_aggverifier_push_mixed*) on the CPU: the entry points as
declared, what they refuse without a device, the Python mirror's ValueError, and the algorithm itself -- known lanes by
leaf and scalar from a pool, the unknown lanes' points, S, the comparison of the unknown lanes' sum with [e_agg - S]G --
restated in tests/aggverifier_mixed_model.py over the pymodel back-end and held against the one-shot root and am.verify
on the block: every n <= 10, EVERY subset of known lanes, B in {2, 4}, every split into at most two pushes; the same with
e_agg negated; the same with one known lane's scalar off by one, which must reject."""
import ctypes as C
import os

import numpy as np
import pytest

import aggregate_model as am
import pymodel as pm
from aggverifier_mixed_model import UNKNOWN, MixedModelVerifier, ModelPool
from test_aggregator_host import ModelAggregator, cached

N_MAX = 10
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["ssa_aggverifier_push_mixed", "ssa_aggverifier_push_mixed_device", "ssa_aggverifier_push_known",
         "ssa_aggverifier_push_known_device", "ssa_debug_aggverifier_known_sum"]


def test_symbols_are_declared_and_exported():
    import schnorr_sig_amd as ssa
    with open(os.path.join(ROOT, "include", "schnorr_sig_amd.h")) as fh:
        header = fh.read()
    assert all(n in ssa.ABI_SYMBOLS and ("int %s(ssa_ctx *ctx, ssa_aggverifier *av, " % n) in header for n in NAMES)
    assert "#define SSA_AGGV_UNKNOWN 0xFFFFFFFFu" in header and ssa.AGGV_UNKNOWN == UNKNOWN == 0xFFFFFFFF
    assert ssa.ABI_VERSION == ssa._lib.ssa_abi_version() == 5              # additive: the version stays
    # the documented argument lists: ctx, av, ag, places, n, [the u compact lanes as push takes them, u], [result]
    args = {n: len(getattr(ssa._lib, n).argtypes) for n in NAMES}
    assert args == {NAMES[0]: 13, NAMES[1]: 14, NAMES[2]: 5, NAMES[3]: 6, NAMES[4]: 4}
    for m in ("push_mixed", "push_known", "push_mixed_device", "push_known_device", "known_sum"):
        assert callable(getattr(ssa.AggregateVerifier, m))
    with open(os.path.join(ROOT, "schnorr-sig_amd", "host", "schnorr_sig.hpp")) as fh:
        mirror = fh.read()
    assert "void push_mixed(Aggregator &pool" in mirror and "void push_known(Aggregator &pool" in mirror


def test_null_objects_and_lists_are_argument_errors():
    """what the entry points refuse before they touch a device"""
    import schnorr_sig_amd as ssa
    lib, word = ssa._lib, (C.c_uint32 * 3)(7, 7, 7)
    places = (C.c_uint32 * 2)(0, UNKNOWN)
    assert lib.ssa_aggverifier_push_mixed(None, None, None, places, 2, None, None, None, None, None, 0, 0, 0) == ssa.ERR_ARG
    assert lib.ssa_aggverifier_push_mixed(None, None, None, None, 0, None, None, None, None, None, 0, 0, 0) == ssa.ERR_ARG
    assert lib.ssa_aggverifier_push_mixed_device(None, None, None, None, 2, None, None, None, None, None, 0, 0, 0,
                                                 C.byref(word, 4)) == ssa.ERR_ARG
    assert lib.ssa_aggverifier_push_known(None, None, None, places, 2) == ssa.ERR_ARG
    assert lib.ssa_aggverifier_push_known(None, None, None, None, 2) == ssa.ERR_ARG
    assert lib.ssa_aggverifier_push_known_device(None, None, None, None, 2, C.byref(word, 4)) == ssa.ERR_ARG
    assert lib.ssa_debug_aggverifier_known_sum(None, None, 0, None) == ssa.ERR_ARG
    assert list(word) == [7, 7, 7]


@pytest.mark.parametrize("bad", [[2 ** 32], [0, -2], [1.5], ["1"], [True], np.array([[0, 1]]), np.array([0.0])])
def test_the_mirror_refuses_places_that_do_not_fit_before_any_call(bad):
    import schnorr_sig_amd as ssa
    av = object.__new__(ssa.AggregateVerifier)            # no engine, no handle: a call would fail differently
    with pytest.raises(ValueError):
        av.push_known(None, bad)
    with pytest.raises(ValueError):
        av.push_mixed(None, bad, None, None, None)
    with pytest.raises(ValueError):
        ssa._places_u32(bad)


def test_the_mirror_takes_none_and_minus_one_for_unknown():
    import schnorr_sig_amd as ssa
    got = ssa._places_u32([3, None, -1, 0, 2 ** 32 - 2, np.int64(5), UNKNOWN])
    assert got.dtype == np.uint32 and got.tolist() == [3, UNKNOWN, UNKNOWN, 0, 2 ** 32 - 2, 5, UNKNOWN]
    assert ssa._places_u32(np.array([-1, 4], dtype=np.int64)).tolist() == [UNKNOWN, 4]
    assert ssa._places_u32([]).size == 0 and ssa._places_u32(range(3)).tolist() == [0, 1, 2]


# ---------------------------------------------------------------------------------------------- the algorithm over the model
def comb_mul(g):
    """[k]g for the fixed point g by 8-bit windows over a table of [d 2^(8 j)]g, built with pymodel's own additions"""
    table, base = [], g
    for _ in range(32):
        row, acc = [None], None
        for _ in range(255):
            acc = pm.pt_add(acc, base)
            row.append(acc)
        table.append(row)
        base = pm.pt_add(row[255], base)                                  # [256] of the window's base

    def mul(k):
        acc = None
        for j in range(32):
            acc = pm.pt_add(acc, table[j][(k >> (8 * j)) & 255])
        return acc
    return mul


@pytest.fixture(scope="module")
def world(oracle):
    """N_MAX honest signatures (the C oracle signs), admitted to a pool IN REVERSE ORDER (so that a lane's place in the
    pool is never its place in the block); the caching back-end; memoised point multiplications, those of G by a comb
    that is checked against pymodel's own; per n the honest scalar, the one-shot root and the one-shot verdicts"""
    rng = np.random.default_rng(0xA634)
    s = rng.integers(0, 256, size=(2, N_MAX, 32), dtype=np.uint8)
    s[:, :, 31] &= 0x3F
    s[:, :, 0] |= 1
    msgs = rng.integers(0, 256, size=(N_MAX, 80), dtype=np.uint8)
    pks, sigs = oracle.keygen_sign_many(s[0], s[1], msgs)
    be = cached(am.pymodel_backend())
    g = pm.default_params().generator()
    g_mul, memo, plain_mul, plain_decompress = comb_mul(g), {}, pm.pt_mul, pm.pt_decompress
    for k in (0, 1, 255, 256, am.Q - 1, int.from_bytes(bytes(sigs[0])[49:81], "little")):
        assert g_mul(k) == plain_mul(k, g)

    def mul(k, pt):
        key = (k, repr(pt))
        if key not in memo:
            memo[key] = g_mul(k) if pt == g else plain_mul(k, pt)
        return memo[key]

    def decompress(r):
        key = bytes(r)
        if key not in memo:
            memo[key] = plain_decompress(key)
        return memo[key]

    def decode(r, pk):
        if (r, pk) not in memo:
            px, py = pm.fp6_from_bytes48(pk[:48]), pm.fp6_from_bytes48(pk[48:96])
            memo[(r, pk)] = decompress(r) + (px, py, px is not None and py is not None and pm.on_curve((px, py)))
        return memo[(r, pk)]

    pool = ModelAggregator(be, 8)                                         # a B other than the verifier's
    order = list(range(N_MAX - 1, -1, -1))
    pool.push(sigs[order], pks[order], msgs[order])
    place = {lane: at for at, lane in enumerate(order)}
    rs = [bytes(x)[:49] for x in sigs]
    want = {}
    mp = pytest.MonkeyPatch()
    mp.setattr(pm, "pt_mul", lambda k, pt: mul(k, pt))
    mp.setattr(pm, "pt_decompress", decompress)
    try:
        for n in range(1, N_MAX + 1):
            e = int.from_bytes(am.aggregate(be, sigs[:n], pks[:n], msgs[:n])[49 * n:], "little")
            root = am.root_of(be, am.tree_top(be, am.leaves(be, rs[:n], pks[:n], msgs[:n])), n)
            neg = (am.Q - e) % am.Q
            want[n] = (root, e, am.verify(be, b"".join(rs[:n]) + e.to_bytes(32, "little"), pks[:n], msgs[:n]),
                       neg, am.verify(be, b"".join(rs[:n]) + neg.to_bytes(32, "little"), pks[:n], msgs[:n]))
            assert want[n][2] == am.OK and want[n][4] == am.INVALID_SIGNATURE
    finally:
        mp.undo()
    return be, (mul, decode), ModelPool(pool.leaves, pool.es), place, rs, pks, msgs, want


def push_block(av, pool, place, rs, pks, msgs, lo, hi, known):
    """lanes [lo, hi) of the block as ONE mixed push: the lanes of `known` by their place in the pool"""
    unk = [i for i in range(lo, hi) if i not in known]
    av.push_mixed(pool, [place[i] if i in known else UNKNOWN for i in range(lo, hi)], [rs[i] for i in unk],
                  [pks[i] for i in unk], [msgs[i] for i in unk])


@pytest.mark.parametrize("B", [2, 4])
@pytest.mark.parametrize("n", range(1, N_MAX + 1))
def test_model_of_the_mixed_verifier_equals_the_one_shot_verdict(world, n, B):
    be, mul, pool, place, rs, pks, msgs, want = world
    root, e, v_honest, neg, v_neg = want[n]
    for mask in range(1 << n):
        known = {i for i in range(n) if mask >> i & 1}
        state = None
        for cut in range(n + 1):                                          # at most two pushes, empty ones included
            av = MixedModelVerifier(be, B, *mul)
            push_block(av, pool, place, rs, pks, msgs, 0, cut, known)
            push_block(av, pool, place, rs, pks, msgs, cut, n, known)
            assert len(av.tops) == n // B and av.known == [i in known for i in range(n)]
            if state is not None:                # the state after the pushes depends on the block alone: finish once
                assert av.state() == state, (n, mask, cut)
                continue
            state = av.state()
            got_root, got = av.finish(n, e)
            assert got_root == root and got == v_honest, (n, B, mask)
            assert av.finish(n, neg) == (root, v_neg), (n, B, mask)
            assert av.finish(n, am.Q)[1] == am.MALFORMED
            assert av.state() == state
        # S is the known lanes' share of the honest scalar, and what is left is the unknown lanes'
        a = am.coeffs_of_root(be, root, n)
        es = [pool.es[place[i]] for i in range(n)]
        assert av.known_sum(n) == sum(a[i] * es[i] for i in known) % am.Q
        assert (e - av.known_sum(n)) % am.Q == sum(a[i] * es[i] for i in range(n) if i not in known) % am.Q


@pytest.mark.parametrize("B", [2, 4])
def test_a_known_scalar_off_by_one_rejects(world, B):
    """the contract's other side: with one known lane's stored scalar wrong the honest block fails, for every n, every
    subset and every choice of the wrong lane in it -- the coefficient of a lane is never zero"""
    be, mul, pool, place, rs, pks, msgs, want = world
    checked = 0
    for n in range(1, N_MAX + 1):
        root, e, v_honest, neg, v_neg = want[n]
        for mask in range(1, 1 << n):
            known = {i for i in range(n) if mask >> i & 1}
            wrong = sorted(known)[(mask * 7 + n) % len(known)]            # one of them, spread over the positions
            es = list(pool.es)
            es[place[wrong]] = (es[place[wrong]] + 1) % am.Q
            spoiled = ModelPool(pool.leaves, es)
            cut = (mask + n) % (n + 1)
            av = MixedModelVerifier(be, B, *mul)
            push_block(av, spoiled, place, rs, pks, msgs, 0, cut, known)
            push_block(av, spoiled, place, rs, pks, msgs, cut, n, known)
            assert av.finish(n, e) == (root, am.INVALID_SIGNATURE), (n, B, mask, wrong)
            checked += 1
    assert checked == sum((1 << n) - 1 for n in range(1, N_MAX + 1))


def test_model_refusals_change_nothing_and_a_copy_is_a_copy(world):
    be, mul, pool, place, rs, pks, msgs, want = world
    av = MixedModelVerifier(be, 2, *mul)
    push_block(av, pool, place, rs, pks, msgs, 0, 3, {0, 2})
    state = av.state()
    for places, cnt in (([len(pool.leaves)], 0), ([UNKNOWN, 0], 0), ([0, 1], 1), ([UNKNOWN], 0)):
        with pytest.raises(ValueError):
            av.push_mixed(pool, places, rs[:cnt], pks[:cnt], msgs[:cnt])
        assert av.state() == state
    # the pool changes afterwards: the verifier holds copies
    other = ModelPool(pool.leaves, pool.es)
    av2 = MixedModelVerifier(be, 2, *mul)
    push_block(av2, other, place, rs, pks, msgs, 0, 3, {0, 2})
    other.leaves[place[0]][0] ^= 1
    other.es[place[2]] = 0
    assert av2.state() == state and av2.finish(3, want[3][1])[1] == am.OK
    # a repeated place is a block with a repeated lane: the model takes it, S counts it twice
    av3 = MixedModelVerifier(be, 2, *mul)
    av3.push_mixed(pool, [place[1], place[1]], [], [], [])
    a = am.coeffs_of_root(be, av3.root(2), 2)
    assert av3.known_sum(2) == (a[0] + a[1]) * pool.es[place[1]] % am.Q
    assert av3.finish(2, av3.known_sum(2))[1] == am.OK and av3.finish(2, (av3.known_sum(2) + 1) % am.Q)[1] == am.INVALID_SIGNATURE
