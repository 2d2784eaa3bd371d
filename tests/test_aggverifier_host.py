"""The streaming aggregate verifier (ssa_aggverifier_*) on the CPU: the algorithm itself -- leaves,
decoded points and challenge scalars appended push by push, the tops of completed blocks stored, finish from the stored
tops plus the ragged block, coefficients from that root, the equation over the stored points -- restated over the model of
tests/aggregate_model.py with the pymodel back-end and held against the one-shot root and am.verify on the concatenation,
for every split into pushes, every prefix, a lane that does not decode and a negated e_agg."""
import itertools

import numpy as np
import pytest

import aggregate_model as am
import pymodel as pm
from test_aggregator_host import cached, splits

N_MAX = 12
BAD_LANE = 5


def test_symbols_are_declared_and_exported():
    import schnorr_sig_amd as ssa
    names = ["ssa_aggverifier_create", "ssa_aggverifier_destroy", "ssa_aggverifier_reset", "ssa_aggverifier_info",
             "ssa_aggverifier_push", "ssa_aggverifier_push_device", "ssa_aggverifier_finish",
             "ssa_aggverifier_finish_device", "ssa_debug_aggverifier_record"]
    assert all(n in ssa.ABI_SYMBOLS for n in names)
    assert ssa.ABI_VERSION == ssa._lib.ssa_abi_version() == 5


def test_null_handles_are_argument_errors():
    """what the entry points refuse before they touch a device"""
    import ctypes as C
    import schnorr_sig_amd as ssa
    lib, h, out8, buf = ssa._lib, C.c_void_p(), (C.c_uint64 * 8)(), (C.c_uint8 * 32)()
    assert lib.ssa_aggverifier_create(None, 16, 0, 0, C.byref(h)) == ssa.ERR_ARG and not h.value
    assert lib.ssa_aggverifier_reset(None) == ssa.ERR_ARG
    assert lib.ssa_aggverifier_info(None, out8) == ssa.ERR_ARG
    assert lib.ssa_aggverifier_push(None, None, None, None, None, None, None, 0, 0, 0) == ssa.ERR_ARG
    assert lib.ssa_aggverifier_push_device(None, None, None, None, None, None, None, 0, 0, 0) == ssa.ERR_ARG
    assert lib.ssa_aggverifier_finish(None, None, buf, 0) == ssa.ERR_ARG
    assert lib.ssa_aggverifier_finish_device(None, None, buf, 0, buf) == ssa.ERR_ARG
    assert lib.ssa_debug_aggverifier_record(None, None, 0, buf) == ssa.ERR_ARG
    lib.ssa_aggverifier_destroy(None)


# ---------------------------------------------------------------------------------------------- the algorithm over the model
class ModelVerifier:
    """what ssa_aggverifier holds and does, in the model's terms"""

    def __init__(self, backend, B, mul, decode):
        self.be, self.B, self.mul, self.decode = backend, B, mul, decode
        self.rpts, self.ppts, self.hs, self.bad, self.leaves, self.tops = [], [], [], [], [], []

    def push(self, rs, pks, msgs):
        held, B = len(self.leaves), self.B
        rs = [bytes(r) for r in rs]
        for r, pk, m in zip(rs, pks, msgs):
            st, pt, px, py, on = self.decode(r, bytes(pk))
            ok = st == "ok" and px is not None and py is not None and on
            self.bad.append(not ok)
            self.rpts.append(pt if ok else None)                          # (None: the sentinel, adds nothing)
            self.ppts.append(pm.pt_neg((px, py)) if ok else None)
            self.hs.append(pm.scalar_from_digest(self.be[1](r[:48], bytes(pk), bytes(m))))
        self.leaves += am.leaves(self.be, rs, pks, msgs) if rs else []
        for b in range(held // B, len(self.leaves) // B):                 # the blocks this push completed
            assert len(self.tops) == b
            self.tops.append(am.tree_top(self.be, self.leaves[B * b: B * (b + 1)]))

    def state(self):
        return (tuple(map(tuple, self.leaves)), tuple(map(tuple, self.tops)), tuple(self.hs), tuple(self.bad),
                tuple(map(repr, self.rpts)), tuple(map(repr, self.ppts)))

    def finish(self, n, e_agg):
        """-> (root, verdict) of the first n lanes under e_agg; reads the state, writes none of it"""
        if e_agg >= am.Q:
            return None, am.MALFORMED
        if n == 0:
            return None, am.OK if e_agg == 0 else am.INVALID_SIGNATURE
        B = self.B
        tops = [list(t) for t in self.tops[:n // B]]                      # a copy: the workspace of the call
        if n % B:
            tops.append(am.tree_top(self.be, self.leaves[B * (n // B): n]))
        root = am.root_of(self.be, am.tree_top(self.be, tops), n)
        if any(self.bad[:n]):
            return root, am.MALFORMED
        left = None
        for i, a in enumerate(am.coeffs_of_root(self.be, root, n)):
            left = pm.pt_add(left, self.mul(a, self.rpts[i]))
            left = pm.pt_add(left, self.mul(a * self.hs[i] % am.Q, self.ppts[i]))
        right = self.mul(e_agg, pm.default_params().generator())
        return root, am.OK if left == right else am.INVALID_SIGNATURE


@pytest.fixture(scope="module")
def model(oracle):
    """N_MAX honest signatures (the C oracle signs), the caching pymodel back-end, memos of the model's point
    multiplications and decompressions (am.verify and the restated algorithm ask for the same ones again and again:
    pymodel's own pt_mul and pt_decompress stand behind them), and per scenario the R's and, for every prefix, the
    scalar, the one-shot root and the one-shot verdict"""
    rng = np.random.default_rng(0xA66B)
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
        """(status and point of R, the key's coordinates, key on the curve)"""
        if (r, pk) not in memo:
            px, py = pm.fp6_from_bytes48(pk[:48]), pm.fp6_from_bytes48(pk[48:96])
            memo[(r, pk)] = decompress(r) + (px, py, px is not None and py is not None and pm.on_curve((px, py)))
        return memo[(r, pk)]

    honest = [bytes(x)[:49] for x in sigs]
    broken = list(honest)
    for t in range(1, 64):
        x = bytearray(honest[BAD_LANE])
        x[8] ^= t
        if pm.pt_decompress(bytes(x))[0] == "invalid":
            break
    broken[BAD_LANE] = bytes(x)
    scenarios = {}
    mp = pytest.MonkeyPatch()
    mp.setattr(pm, "pt_mul", mul)
    mp.setattr(pm, "pt_decompress", decompress)
    try:
        for name, rs, negate in (("honest", honest, False), ("undecodable R", broken, False), ("negated", honest, True)):
            want = {}
            for n in range(0, N_MAX + 1):
                e = int.from_bytes(am.aggregate(be, sigs[:n], pks[:n], msgs[:n])[49 * n:], "little")
                if negate:
                    e = (am.Q - e) % am.Q
                root = am.root_of(be, am.tree_top(be, am.leaves(be, rs[:n], pks[:n], msgs[:n])), n) if n else None
                verdict = am.verify(be, b"".join(rs[:n]) + e.to_bytes(32, "little"), pks[:n], msgs[:n])
                want[n] = (e, root, verdict)
            scenarios[name] = (rs, want)
    finally:
        mp.undo()
    # the scenarios are what they claim to be
    assert all(scenarios["honest"][1][n][2] == am.OK for n in range(N_MAX + 1))
    assert all(scenarios["undecodable R"][1][n][2] == (am.MALFORMED if n > BAD_LANE else am.OK) for n in range(N_MAX + 1))
    assert all(scenarios["negated"][1][n][2] == am.INVALID_SIGNATURE for n in range(1, N_MAX + 1))
    return be, (mul, decode), pks, msgs, scenarios


@pytest.mark.parametrize("B", [2, 4])
@pytest.mark.parametrize("scenario", ["honest", "undecodable R", "negated"])
def test_model_of_the_verifier_equals_the_one_shot_verdict(model, scenario, B):
    be, mul, pks, msgs, scenarios = model
    rs, want = scenarios[scenario]
    seen = {}                                    # the state after a sequence of pushes depends on their sum alone
    for n in range(1, N_MAX + 1):
        for cut in splits(n):
            av, lo = ModelVerifier(be, B, *mul), 0
            for cnt in cut:
                av.push(rs[lo:lo + cnt], pks[lo:lo + cnt], msgs[lo:lo + cnt])
                lo += cnt
            assert len(av.tops) == n // B
            state = av.state()
            if n in seen:                        # ... so every prefix is finished once per n, and every split lands there
                assert state == seen[n], (n, cut)
                continue
            seen[n] = state
            for take in itertools.chain(range(n, -1, -1), range(n + 1)):          # descending, then ascending
                e, root, verdict = want[take]
                got_root, got = av.finish(take, e)
                assert got == verdict, (scenario, B, n, cut, take)
                assert take == 0 or got_root == root, (scenario, B, n, cut, take)
            assert av.state() == state


def test_model_fails_closed_on_a_noncanonical_scalar(model):
    be, mul, pks, msgs, scenarios = model
    rs, want = scenarios["honest"]
    av = ModelVerifier(be, 2, *mul)
    av.push(rs[:3], pks[:3], msgs[:3])
    for n in range(4):
        assert av.finish(n, am.Q)[1] == am.MALFORMED
        assert am.verify(be, b"".join(rs[:n]) + am.Q.to_bytes(32, "little"), pks[:n], msgs[:n]) == am.MALFORMED
