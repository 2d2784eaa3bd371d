"""The streaming aggregate verifier through the key cache (ssa_aggverifier_push_cached*) on the
CPU.  The rule is restated over the model of tests/test_aggverifier_host.py: every push appends one key status per lane
-- the key check's for a lane pushed through a cache, 0 ("not checked") for a lane pushed plainly -- and finish folds the
statuses of the prefix it takes IN FRONT of the model's verdict: the key decides.  Held against section 23's model with
k = 1 (INVALID_PUBLIC_KEY if some lane of the aggregate has that key status, else the one-shot verdict of am.verify) for
every split of n <= 8 lanes into at most three pushes, every way to push each of them plainly or through the cache, every
prefix, and one key P + T2 (T2 of order 2) at each position."""
import itertools

import numpy as np
import pytest

import aggregate_model as am
import pymodel as pm
from test_aggregator_host import cached, splits
from test_aggverifier_host import ModelVerifier

N_MAX = 8
B = 2
OK, BAD_KEY, INVALID, MALFORMED = 0, 1, 2, 3


def test_symbols_are_declared_and_exported():
    import schnorr_sig_amd as ssa
    names = ["ssa_aggverifier_push_cached", "ssa_aggverifier_push_cached_device", "ssa_aggverifier_push_cached_wire",
             "ssa_aggverifier_push_cached_wire_device", "ssa_debug_aggverifier_key_span"]
    assert all(n in ssa.ABI_SYMBOLS for n in names)
    assert ssa.ABI_VERSION == ssa._lib.ssa_abi_version() == 5              # additive: the version stays
    span = ssa.aggverifier_key_span()
    assert span % 4096 == 0 and 2 * span + 17 <= 20000


def test_null_handles_are_argument_errors():
    """what the cached pushes refuse before they touch a device, the caller's statistics untouched"""
    import schnorr_sig_amd as ssa
    lib = ssa._lib
    stats = np.full(8, 9, np.uint64)
    assert lib.ssa_aggverifier_push_cached(None, None, None, None, None, None, None, None, 0, 0, 0, stats.ctypes.data) == ssa.ERR_ARG
    assert lib.ssa_aggverifier_push_cached_device(None, None, None, None, None, None, None, None, 0, 0, 0,
                                                  stats.ctypes.data) == ssa.ERR_ARG
    assert lib.ssa_aggverifier_push_cached_wire(None, None, None, None, None, None, None, 0, 0, 0, stats.ctypes.data) == ssa.ERR_ARG
    assert lib.ssa_aggverifier_push_cached_wire_device(None, None, None, None, None, None, None, 0, 0, 0,
                                                       stats.ctypes.data) == ssa.ERR_ARG
    assert stats.tolist() == [9] * 8


# ---------------------------------------------------------------------------------------------- the rule over the model
def py_key_status(pk96):
    """the key check restated over pymodel: limbs, curve, [q]P (what ssa_keyset_status reports for an affine key)"""
    x, y = pm.fp6_from_bytes48(bytes(pk96[:48])), pm.fp6_from_bytes48(bytes(pk96[48:96]))
    if x is None or y is None or not pm.on_curve((x, y)):
        return MALFORMED
    return OK if pm.is_torsion_free((x, y)) else BAD_KEY


class KeyedModelVerifier:
    """ssa_aggverifier with section 29's byte per lane: `inner` is the model of section 28, untouched"""

    def __init__(self, inner, key_status):
        self.inner, self.key_status, self.kst, self.keyed = inner, key_status, [], False

    def push(self, rs, pks, msgs, through_cache):
        if len(pks) == 0:
            return                                                         # an empty push touches nothing
        if through_cache and not self.keyed:
            self.kst, self.keyed = [0] * len(self.kst), True              # the first cached push zeroes kst[0, held)
        if self.keyed:
            self.kst += [self.key_status(bytes(pk)) if through_cache else 0 for pk in pks]
        else:
            self.kst += [0xEE] * len(pks)                                  # never written, never read: any byte
        self.inner.push(rs, pks, msgs)

    def finish(self, n, e_agg, verdict_of):
        """verdict_of(n, e_agg): the inner model's finish, which depends on the held lanes alone"""
        v = verdict_of(n, e_agg)
        if self.keyed and n >= 1 and any(s == BAD_KEY for s in self.kst[:n]):
            return BAD_KEY
        return v


@pytest.fixture(scope="module")
def world(oracle):
    """N_MAX honest signatures; per position p the keys with lane p's replaced by P_p + T2, and for every prefix the
    honest scalar and the one-shot verdict V (am.verify); the key statuses by pymodel"""
    rng = np.random.default_rng(0xA6C29)
    s = rng.integers(0, 256, size=(2, N_MAX, 32), dtype=np.uint8)
    s[:, :, 31] &= 0x3F
    s[:, :, 0] |= 1
    msgs = rng.integers(0, 256, size=(N_MAX, 80), dtype=np.uint8)
    pks, sigs = oracle.keygen_sign_many(s[0], s[1], msgs)
    be = cached(am.pymodel_backend())
    memo, plain_mul, plain_decompress = {}, pm.pt_mul, pm.pt_decompress

    def mul(k, pt):
        key = (k, repr(pt))
        if key not in memo:
            memo[key] = plain_mul(k, pt)
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

    def status(pk):
        if ("ks", pk) not in memo:
            memo[("ks", pk)] = py_key_status(pk)
        return memo[("ks", pk)]

    rs = [bytes(x)[:49] for x in sigs]
    e_of = [int.from_bytes(am.aggregate(be, sigs[:n], pks[:n], msgs[:n])[49 * n:], "little") for n in range(N_MAX + 1)]
    t2 = pm.SMALL_ORDER_POINTS[2]
    cases = {}
    mp = pytest.MonkeyPatch()
    mp.setattr(pm, "pt_mul", mul)
    mp.setattr(pm, "pt_decompress", decompress)
    try:
        for p in range(N_MAX):
            keys = pks.copy()
            pt = (pm.fp6_from_bytes48(bytes(pks[p, :48])), pm.fp6_from_bytes48(bytes(pks[p, 48:])))
            bad = pm.pt_add(pt, t2)
            keys[p] = np.frombuffer(pm.fp6_to_bytes48(bad[0]) + pm.fp6_to_bytes48(bad[1]), np.uint8)
            assert pm.on_curve(bad)
            ks = [status(bytes(k)) for k in keys]
            assert ks == [BAD_KEY if i == p else OK for i in range(N_MAX)]
            v = {}
            for n in range(N_MAX + 1):
                for name, e in (("honest", e_of[n]), ("negated", (am.Q - e_of[n]) % am.Q)):
                    v[(n, e)] = am.verify(be, b"".join(rs[:n]) + e.to_bytes(32, "little"), keys[:n], msgs[:n])
                # V alone: the honest prefix verifies up to the spoiled lane, and is INVALID (never BAD_KEY) from it on
                assert v[(n, e_of[n])] == (OK if n <= p else INVALID)
            cases[p] = (keys, ks, v)
    finally:
        mp.undo()
    return be, (mul, decode), status, rs, msgs, e_of, cases


def section_23(ks, v, n, e):
    """the model of ssa_verify_aggregates_many_cached with k = 1, counts = {n}: the key decides, else V"""
    return BAD_KEY if any(s == BAD_KEY for s in ks[:n]) else v[(n, e)]


@pytest.mark.parametrize("p", range(N_MAX))
def test_the_rule_equals_section_23_with_one_aggregate(world, p):
    be, mul, status, rs, msgs, e_of, cases = world
    keys, ks, v = cases[p]
    inner_verdicts = {}
    all_cached = mixed = refused = plain_copy = 0
    for n in range(1, N_MAX + 1):
        for cut in splits(n):
            for how in itertools.product((False, True), repeat=3):        # each push plainly or through the cache
                inner = ModelVerifier(be, B, *mul)
                av, lo, via = KeyedModelVerifier(inner, status), 0, []
                for cnt, through_cache in zip(cut, how):
                    av.push(rs[lo:lo + cnt], keys[lo:lo + cnt], msgs[lo:lo + cnt], through_cache)
                    via += [through_cache] * cnt
                    lo += cnt
                assert len(av.kst) == n == len(inner.leaves)

                def verdict_of(take, e, inner=inner, n=n):
                    if (n, take, e) not in inner_verdicts:                # (the state depends on the held lanes alone:
                        inner_verdicts[(n, take, e)] = inner.finish(take, e)[1]      # tests/test_aggverifier_host.py)
                    return inner_verdicts[(n, take, e)]

                for take in range(n + 1):
                    for e in (e_of[take], (am.Q - e_of[take]) % am.Q):
                        got = av.finish(take, e, verdict_of)
                        assert verdict_of(take, e) == v[(take, e)]        # section 28's equality, under the rule
                        if all(via[:take]):                               # the whole prefix came through a cache
                            assert got == section_23(ks, v, take, e), (n, cut, how, take)
                            all_cached += 1
                        else:
                            mixed += 1
                        # in every mix: the spoiled lane refuses exactly when IT came through the cache
                        want = BAD_KEY if (p < take and via[p]) else v[(take, e)]
                        assert got == want, (n, cut, how, take)
                        refused += got == BAD_KEY
                        if p < take and not via[p]:
                            assert got == INVALID                         # the plain-pushed copy of the lane: V, no refusal
                            plain_copy += 1
    assert all_cached and mixed and refused and plain_copy
    # take == 0 keeps the rule of the empty aggregate whatever was pushed
    assert section_23(ks, v, 0, 0) == OK == v[(0, 0)]


def test_a_cached_push_after_plain_ones_zeroes_the_old_bytes(world):
    """bytes an earlier life of the object left in kst are not read as statuses: the first cached push zeroes kst[0, held)"""
    be, mul, status, rs, msgs, e_of, cases = world
    keys, ks, v = cases[0]
    av = KeyedModelVerifier(ModelVerifier(be, B, *mul), status)
    av.kst = [BAD_KEY] * 3                                                # what a keyed life before a reset left there
    av.inner.push(rs[1:4], keys[1:4], msgs[1:4])                          # three good lanes, pushed plainly
    av.push(rs[4:5], keys[4:5], msgs[4:5], True)
    assert av.kst == [0, 0, 0, OK]
    assert av.finish(4, 0, lambda n, e: INVALID) == INVALID
