"""Half-aggregates through the key cache, subgroup check included (ssa_verify_aggregates_many_cached, DESIGN.md section
23).  The contract is one equality:

    verdict j = SSA_INVALID_PUBLIC_KEY   if some lane of aggregate j has key status SSA_INVALID_PUBLIC_KEY
              = V_j                      otherwise

Both sides of it are computed OUTSIDE the call under test: V_j by ssa_verify_aggregate on aggregate j alone over the
unpacked keys U (the session's engine), the key statuses by a ladder key set over the distinct keys of U.  Every touched
key is also classified by pymodel (on the curve, [q]P), and the model of tests/aggregate_model.py over the C oracle gives
V_j for the touched aggregates it can finish in seconds: those of at most two lanes in full, a longer one where it stops
at a malformed key in its first lane, and with its full point sum (pure Python, 0.04 s per lane: 2.5 s for 63 lanes, 10 s
for the 257-lane aggregate and 20 s for the 513-lane one, which it is not asked for) the 5-lane aggregate that shows the
gap and the 63- and 64-lane aggregates with P + T2 or the identity key in them.

Every case runs through an affine and a wire cache, the host and the device form, and engines forced onto either group
path of section 21 ("small": SSA_MSM_SMALL_MAX = 2^40, "bucket": 0)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import aggregate_model as am
from test_gpu_aggregates_many import (counts_of, e_bytes, e_of, make_scalars, model, ranges_of, singles, with_e)
from test_gpu_screened_torsion import key_choice, special_key_lanes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q = am.Q
OK, BAD_KEY, INVALID, MALFORMED = 0, 1, 2, 3
SIZES = [0, 1, 2, 63, 64, 65, 255, 256, 257, 513]
N = sum(SIZES)
SIGNERS = 40
MODES = ["affine", "wire"]
FORMS = ["host", "device"]
PATHS = ["small", "bucket"]
DISTINCT, HITS, INSERTED, EVICTIONS, BYPASSED, BOUND, BAD_AGGS = range(7)
_STATE = {}


@pytest.fixture(scope="module")
def engines():
    """contexts that take one path for every group, whatever its size"""
    import schnorr_sig_amd as ssa
    made = {}
    old = os.environ.get("SSA_MSM_SMALL_MAX")
    try:
        for name, bound in (("small", 1 << 40), ("bucket", 0)):
            os.environ["SSA_MSM_SMALL_MAX"] = str(bound)
            made[name] = ssa.Engine(0)
    finally:
        if old is None:
            os.environ.pop("SSA_MSM_SMALL_MAX", None)
        else:
            os.environ["SSA_MSM_SMALL_MAX"] = old
    yield made
    for e in made.values():
        e.close()


def affine_bytes(pt):
    import pymodel as pm
    return np.frombuffer(pm.fp6_to_bytes48(pt[0]) + pm.fp6_to_bytes48(pt[1]), np.uint8)


class World:
    """N honest signatures by SIGNERS repeating signers over 80-byte messages, cut into honest aggregates of SIZES lanes;
    the keys in both forms"""

    def __init__(self, engine):
        rng = np.random.default_rng(0xA6C23)
        self.msgs = rng.integers(0, 256, size=(N, 80), dtype=np.uint8)
        sks = make_scalars(rng, SIGNERS)[key_choice(rng, N, SIGNERS)]
        self.pks, self.sigs = engine.keygen_sign_many(sks, make_scalars(rng, N), self.msgs)
        self.wire, st = engine.compress_many(self.pks)
        assert (st == 0).all()
        self.aggs, lo = [], 0
        for c in SIZES:
            st, agg, _, nf = engine.aggregate(self.sigs[lo:lo + c], self.pks[lo:lo + c], self.msgs[lo:lo + c])
            assert st == OK and nf == 0
            self.aggs.append(agg)
            lo += c
        self.ranges = ranges_of(self.aggs)
        self.v = singles(engine, self.aggs, self.pks, self.msgs)      # V of the honest call
        assert self.v == [OK] * len(SIZES)


@pytest.fixture
def world(engine):
    if "world" not in _STATE:
        _STATE["world"] = World(engine)
    return _STATE["world"]


class Keys:
    """the keys of a call as its mode takes them, and U, what the aggregate verifier reads"""

    def __init__(self, engine, mode, pks, inf=None, wire=None):
        self.mode = mode
        if mode == "affine":
            self.arg, self.inf = pks, inf
            self.u_pks, self.u_inf = pks, inf if inf is not None else np.zeros(pks.shape[0], np.uint8)
        else:
            self.arg, self.inf = wire, None
            self.u_pks, self.u_inf, _ = engine.decompress_many(wire) if wire.shape[0] else (
                np.zeros((0, 96), np.uint8), np.zeros(0, np.uint8), None)


def key_statuses(engine, keys):
    """ks_i for every lane: the status bytes of a ladder key set over the DISTINCT keys of U"""
    if keys.u_pks.shape[0] == 0:
        return np.zeros(0, np.uint8)
    rows = np.concatenate([keys.u_pks, (keys.u_inf != 0).astype(np.uint8)[:, None]], axis=1)
    uniq, inv = np.unique(rows, axis=0, return_inverse=True)
    ks = engine.keyset_create(np.ascontiguousarray(uniq[:, :96]), np.ascontiguousarray(uniq[:, 96]), kind="ladder")
    try:
        st = engine.keyset_status(ks)
    finally:
        ks.close()
    return st[np.asarray(inv).reshape(-1)]


def expected(engine, aggs, keys, msgs, offsets=None, base=None, touched=()):
    """the right-hand side of the equality -> (verdicts, per-lane key statuses, V).  base: V of a call that differs from
    this one only in the aggregates `touched` (their bytes, keys or messages): the single calls of the others are the
    same calls on the same bytes and are not repeated."""
    if base is not None:
        v, rg = list(base), ranges_of(aggs)
        for j in touched:
            lo, hi = rg[j]
            v[j] = engine.verify_aggregate(aggs[j], keys.u_pks[lo:hi], msgs[lo:hi] if hi > lo else None,
                                           pk_inf=keys.u_inf[lo:hi])
    elif offsets is None:
        v = singles(engine, aggs, keys.u_pks, msgs, keys.u_inf)
    else:
        import schnorr_sig_amd as ssa
        v = []
        for a, (lo, hi) in zip(aggs, ranges_of(aggs)):
            rows = [bytes(msgs[int(offsets[i]):int(offsets[i + 1])]) for i in range(lo, hi)]
            f, o = ssa.pack_messages(rows)
            v.append(engine.verify_aggregate(a, keys.u_pks[lo:hi], f, offsets=o, pk_inf=keys.u_inf[lo:hi]))
    kst = key_statuses(engine, keys)
    out = [BAD_KEY if (kst[lo:hi] == BAD_KEY).any() else int(v[j]) for j, (lo, hi) in enumerate(ranges_of(aggs))]
    return out, kst, [int(x) for x in v]


def py_key_status(u_pk, u_inf):
    """the key check restated over pymodel: limbs, curve, [q]P"""
    import pymodel as pm
    x, y = pm.fp6_from_bytes48(bytes(u_pk[:48])), pm.fp6_from_bytes48(bytes(u_pk[48:]))
    if x is None or y is None:
        return MALFORMED
    if u_inf:
        return OK
    if not pm.on_curve((x, y)):
        return MALFORMED
    return OK if pm.is_torsion_free((x, y)) else BAD_KEY


def dev(*arrays):
    import torch
    out = [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0") for a in arrays]
    torch.cuda.synchronize()
    return out


def run(eng, cache, aggs, keys, msgs, form="host", offsets=None, tail=0):
    """one call -> (verdicts as a list, stats as a list of ints[, the device words behind verdicts[k)])"""
    import torch
    k = len(aggs)
    if form == "host":
        v, st = eng.verify_aggregates_cached(cache, aggs, keys.arg, msgs, pk_inf=keys.inf, offsets=offsets)
        return v.tolist(), [int(x) for x in st]
    wire = np.concatenate(aggs) if k else np.zeros(0, np.uint8)
    d_wire, d_keys, d_inf, d_msgs = dev(wire, keys.arg, keys.inf, msgs)
    d_off = dev(np.asarray(offsets).astype(np.int64))[0] if offsets is not None else None
    out = torch.full((k + tail,), 255, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    _, st = eng.verify_aggregates_cached_device(cache, d_wire, counts_of(aggs), d_keys, d_msgs, d_verdicts=out[:k],
                                                d_pk_inf=d_inf, d_offsets=d_off)
    eng.sync()
    got = out.cpu().tolist()
    res = (got[:k], [int(x) for x in st])
    return res + (got[k:],) if tail else res


def new_cache(eng, mode, capacity=4096, evict="clear"):
    return eng.keycache_create(capacity, wire=(mode == "wire"), evict=evict)


def check_stats(st, cold=None):
    assert st[HITS] + st[INSERTED] == st[DISTINCT] and st[BYPASSED] == 0 and st[BOUND] == 0 and st[7] == 0, st
    if cold is True:
        assert st[HITS] == 0
    if cold is False:
        assert st[INSERTED] == 0


# ------------------------------------------------------------------ the gap the feature closes
def gap_case(engine, world):
    """[3 honest lanes] [4 honest lanes and a lane signed for P + T2 whose h is even] [2 honest lanes] -> (aggregates,
    keys, wire keys, messages, the lane of the bad key).

    The lane's error term is [h] T2 in ssa_verify_many (zero when h is even) and [a h mod q] T2 in the aggregate, a the
    lane's transcript coefficient: q is odd, so the parity of a h mod q is a coin that every arrangement of the
    aggregate tosses again.  The even lanes are picked by ssa_verify_many without the subgroup check; the arrangement
    (which even lane, at which of the five positions) is the first that ssa_verify_aggregate accepts."""
    if "gap" not in _STATE:
        rng = np.random.default_rng(0x6A9)
        pkb, s8, m8 = special_key_lanes(rng, 8, True)
        st, _ = engine.verify_many(s8, np.tile(pkb, (8, 1)), m8, check_torsion=False)
        even = np.nonzero(st == 0)[0]
        assert even.size >= 1, "the seed must give a lane with an even h"
        # ... which the subgroup check alone refuses
        assert (engine.verify_many(s8, np.tile(pkb, (8, 1)), m8, check_torsion=True)[0] == BAD_KEY).all()
        lanes = list(range(100, 109))
        found = None
        for t in (int(x) for x in even):
            for pos in range(5):
                pks, sigs, msgs = world.pks[lanes].copy(), world.sigs[lanes].copy(), world.msgs[lanes].copy()
                at = 3 + pos
                pks[at], sigs[at], msgs[at] = pkb, s8[t], m8[t]
                st, agg, _, _ = engine.aggregate(sigs[3:8], pks[3:8], msgs[3:8])
                if st == OK and engine.verify_aggregate(agg, pks[3:8], msgs[3:8]) == OK:
                    found = (pks, sigs, msgs, at)
                    break
            if found:
                break
        assert found, "the seed must give an arrangement that verifies without the subgroup check"
        pks, sigs, msgs, at = found
        aggs, lo = [], 0
        for c in (3, 5, 2):
            st, agg, _, _ = engine.aggregate(sigs[lo:lo + c], pks[lo:lo + c], msgs[lo:lo + c])
            assert st == OK
            aggs.append(agg)
            lo += c
        wire, st = engine.compress_many(pks)
        assert (st == 0).all()
        _STATE["gap"] = (aggs, pks, wire, msgs, at)
    return _STATE["gap"]


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("mode", MODES)
def test_a_key_outside_the_subgroup_is_accepted_without_the_cache_and_refused_with_it(engine, engines, world, mode, form, path):
    """Why the call exists: a signature for the key P + T2 (T2 of order 2) verifies without the subgroup check whenever
    its h is even, and ssa_verify_aggregates_many accepts an aggregate that holds one whenever a h mod q is even
    (gap_case)."""
    import pymodel as pm
    eng = engines[path]
    aggs, pks, wire, msgs, at = gap_case(engine, world)
    assert eng.verify_aggregates(aggs, pks, msgs).tolist() == [OK, OK, OK]
    assert singles(engine, aggs, pks, msgs) == [OK, OK, OK]
    assert py_key_status(pks[at], 0) == BAD_KEY and py_key_status(pks[0], 0) == OK
    assert pm.pt_decompress(wire[at].tobytes())[0] == "ok"
    keys = Keys(engine, mode, pks, wire=wire)
    with new_cache(eng, mode) as cache:
        got, st = run(eng, cache, aggs, keys, msgs, form)
        assert got == [OK, BAD_KEY, OK]
        assert st[BAD_AGGS] == 1
        check_stats(st, cold=True)


# ------------------------------------------------------------------ the equality, at the sizes where a fold can go wrong
def spoil_classes(engine, mode):
    """name -> f(pks, inf, wire, i): spoil the key of lane i in the form the mode takes"""
    import pymodel as pm
    if "t2keys" not in _STATE:
        rng = np.random.default_rng(0x72)
        pkb = special_key_lanes(rng, 1, True)[0]
        t2 = affine_bytes(pm.SMALL_ORDER_POINTS[2])
        w, st = engine.compress_many(np.stack([pkb, t2]))
        assert (st == 0).all()
        _STATE["t2keys"] = (pkb, t2, w)
    pkb, t2, w = _STATE["t2keys"]

    def put(apk, wk):
        def f(pks, inf, wire, i):
            pks[i], wire[i] = apk, wk
        return f

    def noncanon(pks, inf, wire, i):
        pks[i, 0:8] = 0xFF
        wire[i, 0:8] = 0xFF

    def off_curve(pks, inf, wire, i):          # (affine only: 49 bytes cannot say it)
        pks[i, 48] ^= 1

    def bad_flag(pks, inf, wire, i):           # (wire only)
        wire[i, 48] |= 0x01

    def no_root(pks, inf, wire, i):            # (wire only) x^3 + x + u + 395 is not a square
        for t in range(1, 64):
            x = wire[i].copy()
            x[8] ^= t
            if pm.pt_decompress(x.tobytes())[0] == "invalid":
                wire[i] = x
                return
        raise AssertionError("no x without a point found")

    def identity(pks, inf, wire, i):
        pks[i], inf[i] = 0, 1
        wire[i, :48], wire[i, 48] = 0, 0x80

    both = {"p_plus_t2": put(pkb, w[0]), "order_2_point": put(t2, w[1]), "noncanonical_limb": noncanon, "identity": identity}
    if mode == "affine":
        both["off_curve"] = off_curve
    else:
        both["bad_flag_bits"], both["no_square_root"] = bad_flag, no_root
    return both


WANT_KS = {"p_plus_t2": BAD_KEY, "order_2_point": BAD_KEY, "noncanonical_limb": MALFORMED, "identity": OK,
           "off_curve": MALFORMED, "bad_flag_bits": MALFORMED, "no_square_root": MALFORMED}
# verdict of the touched aggregate: the key decides; an identity key is a good key under which the honest lane fails
WANT_VERDICT = {"p_plus_t2": BAD_KEY, "order_2_point": BAD_KEY, "noncanonical_limb": MALFORMED, "identity": INVALID,
                "off_curve": MALFORMED, "bad_flag_bits": MALFORMED, "no_square_root": MALFORMED}


def placements(world):
    """name -> (lane, its aggregate)"""
    rg = world.ranges
    j257, j1, j2 = SIZES.index(257), SIZES.index(1), SIZES.index(2)
    return {"first_lane": (rg[SIZES.index(63)][0], SIZES.index(63)),
            "last_lane": (rg[SIZES.index(64)][1] - 1, SIZES.index(64)),
            "lane_63_of_257": (rg[j257][0] + 63, j257), "lane_64_of_257": (rg[j257][0] + 64, j257),
            "left_of_a_boundary": (rg[j1][1] - 1, j1), "right_of_a_boundary": (rg[j2][0], j2)}


def equality_cases(engine, world, mode):
    """every (class, placement): aggregates, keys, messages, and the expectation computed outside the call"""
    key = ("equality", mode)
    if key not in _STATE:
        cases = []
        for cname, spoil in spoil_classes(engine, mode).items():
            for pname, (lane, j) in placements(world).items():
                pks, inf, wire = world.pks.copy(), np.zeros(N, np.uint8), world.wire.copy()
                spoil(pks, inf, wire, lane)
                keys = Keys(engine, mode, pks, inf, wire)
                want, kst, v = expected(engine, world.aggs, keys, world.msgs, base=world.v, touched=[j])
                assert kst[lane] == WANT_KS[cname] == py_key_status(keys.u_pks[lane], keys.u_inf[lane]), (cname, pname)
                assert int((kst != OK).sum()) == (0 if cname == "identity" else 1)
                # a bad key changes its own aggregate's verdict and no neighbour's
                assert want == [WANT_VERDICT[cname] if a == j else OK for a in range(len(SIZES))], (cname, pname, want)
                cases.append((cname, pname, j, keys, want, v))
        _STATE[key] = cases
    return _STATE[key]


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("mode", MODES)
def test_the_equality_for_every_class_of_key_at_every_edge(engine, engines, world, mode, form, path):
    eng = engines[path]
    with new_cache(eng, mode) as cache:
        for cname, pname, j, keys, want, _ in equality_cases(engine, world, mode):
            got, st = run(eng, cache, world.aggs, keys, world.msgs, form)
            assert got == want, (cname, pname, got, want)
            assert st[BAD_AGGS] == sum(w == BAD_KEY for w in want), (cname, pname, st)
            check_stats(st)


@pytest.mark.parametrize("mode", MODES)
def test_the_model_over_the_oracle_agrees_on_the_touched_aggregates(engine, oracle, world, mode):
    """V_j from tests/aggregate_model.py where it ends within about a second (see the head of this file)"""
    cheap = {"noncanonical_limb", "off_curve", "bad_flag_bits", "no_square_root"}      # the model stops at the key
    seen = 0
    for cname, pname, j, keys, want, v in equality_cases(engine, world, mode):
        if SIZES[j] <= 2 or (cname in cheap and pname == "first_lane"):
            key = ("model", cname, pname, keys.u_pks[slice(*world.ranges[j])].tobytes(), keys.u_inf.tobytes())
            if key not in _STATE:          # (wire and affine cases often unpack to the same U: asked once)
                _STATE[key] = model(oracle, world.aggs, keys.u_pks, world.msgs, [j], keys.u_inf)[0]
            assert _STATE[key] == v[j], (cname, pname)
            seen += 1
    assert seen >= 12


@pytest.mark.parametrize("case", ["gap", "p_plus_t2 first_lane", "identity first_lane", "p_plus_t2 last_lane",
                                  "identity last_lane"])
def test_the_model_confirms_v_where_the_key_overrides_it_or_the_sum_decides(engine, oracle, world, case):
    """V_j from the model's full point sum for touched aggregates of 5, 63 and 64 lanes (about 2.5 s for 63 lanes): the
    aggregate of gap_case, whose V_j is OK and whose verdict is not; P + T2 in the 63- and the 64-lane aggregate, where
    V_j is INVALID and the key overrides it; the identity key there, where V_j is the verdict."""
    if case == "gap":
        aggs, pks, _, msgs, at = gap_case(engine, world)
        assert model(oracle, aggs, pks, msgs, [1]) == [OK] == singles(engine, aggs, pks, msgs)[1:2]
        assert py_key_status(pks[at], 0) == BAD_KEY
        return
    cname, pname = case.split()
    _, _, j, keys, want, v = [c for c in equality_cases(engine, world, "affine") if c[:2] == (cname, pname)][0]
    assert SIZES[j] == (63 if pname == "first_lane" else 64)
    assert want[j] == (BAD_KEY if cname == "p_plus_t2" else INVALID)
    assert model(oracle, world.aggs, keys.u_pks, world.msgs, [j], keys.u_inf) == [INVALID] == [v[j]]


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("mode", MODES)
def test_bad_key_and_bad_signature_in_one_aggregate_the_key_decides(engine, engines, world, mode, form, path):
    eng = engines[path]
    key = ("combined", mode)
    if key not in _STATE:
        spoil = spoil_classes(engine, mode)
        j, rg = SIZES.index(65), world.ranges
        lo = rg[j][0]
        cases = []
        for kname in ("p_plus_t2", "noncanonical_limb"):
            for sname in ("wrong_message", "negated_e_agg", "malformed_r"):
                pks, inf, wire = world.pks.copy(), np.zeros(N, np.uint8), world.wire.copy()
                spoil[kname](pks, inf, wire, lo + 7)
                aggs, msgs = [a.copy() for a in world.aggs], world.msgs.copy()
                if sname == "wrong_message":
                    msgs[lo + 30, 5] ^= 0x20
                elif sname == "negated_e_agg":
                    aggs[j] = with_e(aggs[j], (Q - e_of(aggs[j])) % Q)
                else:
                    aggs[j][49 * 40 + 48] |= 0x01
                keys = Keys(engine, mode, pks, inf, wire)
                want, _, v = expected(engine, aggs, keys, msgs, base=world.v, touched=[j])
                # the key decides: a subgroup-bad key even over a malformed R; a malformed key is V_j's own answer
                assert v[j] == MALFORMED if (kname == "noncanonical_limb" or sname == "malformed_r") else v[j] == INVALID
                assert want[j] == (BAD_KEY if kname == "p_plus_t2" else MALFORMED)
                assert [w for a, w in enumerate(want) if a != j] == [OK] * (len(SIZES) - 1)
                cases.append((kname, sname, aggs, keys, msgs, want))
        _STATE[key] = cases
    with new_cache(eng, mode) as cache:
        for kname, sname, aggs, keys, msgs, want in _STATE[key]:
            got, st = run(eng, cache, aggs, keys, msgs, form)
            assert got == want, (kname, sname, got, want)


# ------------------------------------------------------------------ more aggregates than a group holds
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("mode", MODES)
def test_more_aggregates_than_a_group_holds(engine, engines, world, mode, form, path):
    eng = engines[path]
    counts = [3] * 300 + [1] * 700
    n = sum(counts)
    idx = np.arange(n) % N                               # (the world's lanes, taken round again)
    w_pks, w_sigs, w_msgs, w_wire = world.pks[idx], world.sigs[idx], world.msgs[idx], world.wire[idx]
    if "many" not in _STATE:
        aggs, lo = [], 0
        for c in counts:
            st, agg, _, _ = engine.aggregate(w_sigs[lo:lo + c], w_pks[lo:lo + c], w_msgs[lo:lo + c])
            assert st == OK
            aggs.append(agg)
            lo += c
        _STATE["many"] = (aggs, singles(engine, aggs, w_pks, w_msgs))
    aggs, honest_v = _STATE["many"]
    key = ("many", mode)
    if key not in _STATE:
        rg = ranges_of(aggs)
        spoil = spoil_classes(engine, mode)["p_plus_t2"]
        pks, inf, wire = w_pks.copy(), np.zeros(n, np.uint8), w_wire.copy()
        bad = [0, 255, 256, len(counts) - 1]
        for j, at in zip(bad, (0, 2, 1, 0)):
            spoil(pks, inf, wire, rg[j][0] + at)
        keys = Keys(engine, mode, pks, inf, wire)
        want, _, _ = expected(engine, aggs, keys, w_msgs, base=honest_v, touched=bad)
        assert want == [BAD_KEY if j in bad else OK for j in range(len(counts))]
        _STATE[key] = (keys, want)
    keys, want = _STATE[key]
    with new_cache(eng, mode) as cache:
        got, st = run(eng, cache, aggs, keys, w_msgs, form)
        assert got == want
        assert st[BAD_AGGS] == 4 and st[DISTINCT] == SIGNERS + 1


# ------------------------------------------------------------------ aggregates above one wave's share
LONG = [5, 4096, 4097, 10000]        # one workgroup of agc_k_key_verdicts: the wave branch (5, 4096 = AGC_WAVE_MAX) and the
                                     # whole-workgroup branch (4097, 10000) side by side, every range off a 16-byte edge


def long_world(engine, world):
    if "long" not in _STATE:
        n = sum(LONG)
        idx = np.arange(n) % N                           # (the world's lanes, taken round again)
        pks, sigs, msgs, wire = world.pks[idx], world.sigs[idx], world.msgs[idx], world.wire[idx]
        aggs, lo = [], 0
        for c in LONG:
            st, agg, _, _ = engine.aggregate(sigs[lo:lo + c], pks[lo:lo + c], msgs[lo:lo + c])
            assert st == OK
            aggs.append(agg)
            lo += c
        v = singles(engine, aggs, pks, msgs)
        assert v == [OK] * len(LONG)
        _STATE["long"] = (aggs, pks, wire, msgs, v)
    return _STATE["long"]


def long_placements():
    """name -> (lane, its aggregate): where the fold of a long aggregate can lose a byte.  With nt = 256 threads, thread t
    reads the 16-byte chunks t, t + 256, ... of the aligned middle [a, b) of its range and the head and tail bytes singly."""
    rg, lo = [], 0
    for c in LONG:
        rg.append((lo, lo + c))
        lo += c
    out = {}
    for j in (2, 3):
        lo, hi = rg[j]
        a, b = (lo + 15) & ~15, hi & ~15
        assert lo < a and b < hi and (b - a) // 16 >= 255
        tag = "_%d" % LONG[j]
        out["first_lane" + tag] = (lo, j)
        out["last_lane" + tag] = (hi - 1, j)
        out["head" + tag] = (a - 1, j)
        out["tail" + tag] = (b, j)
        out["wave_1_chunk" + tag] = (a + 16 * 100 + 5, j)            # chunk 100: thread 100, wave 1
        out["wave_3_chunk" + tag] = (a + 16 * 254 + 15, j)           # chunk 254: thread 254, wave 3 (the last chunk of 4 097)
    lo, hi = rg[3]
    a = (lo + 15) & ~15
    out["wave_2_second_round_10000"] = (a + 16 * (256 + 130), 3)       # chunk 386: thread 130 again, its second step
    lo, hi = rg[1]
    out["last_lane_4096"] = (hi - 1, 1)                              # the longest aggregate ONE wave folds
    out["middle_4096"] = (lo + 2049, 1)
    return out


def long_cases(engine, world, mode):
    key = ("long", mode)
    if key not in _STATE:
        aggs, w_pks, w_wire, msgs, base = long_world(engine, world)
        n = sum(LONG)
        spoil = spoil_classes(engine, mode)["p_plus_t2"]
        cases = []
        for pname, (lane, j) in long_placements().items():
            pks, inf, wire = w_pks.copy(), np.zeros(n, np.uint8), w_wire.copy()
            spoil(pks, inf, wire, lane)
            keys = Keys(engine, mode, pks, inf, wire)
            want, kst, v = expected(engine, aggs, keys, msgs, base=base, touched=[j])
            assert kst[lane] == BAD_KEY and int((kst != OK).sum()) == 1
            assert v[j] == INVALID                     # (the honest lane fails under the other key: V_j alone would say 2)
            assert want == [BAD_KEY if a == j else OK for a in range(len(LONG))], (pname, want)
            cases.append((pname, keys, want))
        keys = Keys(engine, mode, w_pks, np.zeros(n, np.uint8), w_wire)
        cases.append(("honest", keys, expected(engine, aggs, keys, msgs, base=base)[0]))
        assert cases[-1][2] == [OK] * len(LONG)
        _STATE[key] = cases
    return _STATE[key]


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("mode", MODES)
def test_aggregates_on_both_sides_of_the_whole_workgroup_fold(engine, engines, world, mode, form, path):
    """Aggregates of 4 096, 4 097 and 10 000 lanes in one call: agc_k_key_verdicts folds the first with one wave and the
    other two with the whole workgroup (LDS word per wave, two barriers).  One key outside the subgroup per case, at
    every place where that fold splits its range; then all of it again on workspaces whose every byte says "bad key"."""
    eng = engines[path]
    aggs, _, _, msgs, _ = long_world(engine, world)
    with new_cache(eng, mode) as cache:
        for poison in (None, 0x01):
            for pname, keys, want in long_cases(engine, world, mode):
                if poison is not None:
                    eng.debug_poison_workspaces(poison)
                got, st = run(eng, cache, aggs, keys, msgs, form)
                assert got == want, (pname, poison, got, want)
                assert st[BAD_AGGS] == sum(w == BAD_KEY for w in want), (pname, st)
                check_stats(st)


# ------------------------------------------------------------------ cache states
def launches(eng, name):
    return eng.read_timing(name)[1]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("mode", MODES)
def test_cold_then_warm_builds_and_decompresses_nothing_twice(engine, world, mode, form):
    import schnorr_sig_amd as ssa
    _, _, j, keys, want, _ = [c for c in equality_cases(engine, world, mode) if c[0] == "p_plus_t2"][0]
    u = SIGNERS + 1                                      # the bad key is a key like any other
    eng = ssa.Engine(0)
    try:
        with new_cache(eng, mode) as cache:
            eng.enable_timing(True)
            for name in ("ssa_k_keyset_build", "ssa_k_keyed_decompress", "agc_expand", "agc_k_key_verdicts"):
                eng.read_timing(name)                    # drains the key
            got, st = run(eng, cache, world.aggs, keys, world.msgs, form)
            assert got == want
            check_stats(st, cold=True)
            assert st[DISTINCT] == st[INSERTED] == u and cache.info()["held"] == u
            assert launches(eng, "ssa_k_keyset_build") == 1
            assert launches(eng, "ssa_k_keyed_decompress") == (1 if mode == "wire" else 0)
            assert launches(eng, "agc_expand") == 1 and launches(eng, "agc_k_key_verdicts") == 1
            got, st = run(eng, cache, world.aggs, keys, world.msgs, form)
            assert got == want
            check_stats(st, cold=False)
            assert st[DISTINCT] == st[HITS] == u and cache.info()["held"] == u
            assert launches(eng, "ssa_k_keyset_build") == 0 and launches(eng, "ssa_k_keyed_decompress") == 0
            assert launches(eng, "agc_expand") == 1 and launches(eng, "agc_k_key_verdicts") == 1
            assert launches(eng, "keyed_split") == 0 and launches(eng, "keyed_expand") == 0
            eng.enable_timing(False)
            # cleared between two calls: cold again, the same verdicts
            cache.clear()
            got, st = run(eng, cache, world.aggs, keys, world.msgs, form)
            assert got == want and st[INSERTED] == u and cache.info()["held"] == u
    finally:
        eng.close()


@pytest.mark.parametrize("mode", MODES)
def test_the_per_signature_calls_and_the_aggregate_call_warm_each_other(engine, world, mode):
    import schnorr_sig_amd as ssa
    _, _, j, keys, want, _ = [c for c in equality_cases(engine, world, mode) if c[0] == "order_2_point"][0]
    n = 4000                                             # (above SSA_MSM_SMALL_MAX: the per-signature call uses the cache)
    reps = -(-n // N)
    sigs = np.tile(world.sigs, (reps, 1))[:n]
    msgs = np.tile(world.msgs, (reps, 1))[:n]

    def per_signature(cache):
        if mode == "affine":
            return engine.verify_many_cached(cache, sigs, np.tile(keys.arg, (reps, 1))[:n], msgs)[2]
        keyed = np.concatenate([np.tile(keys.arg, (reps, 1))[:n], sigs], axis=1)
        return engine.verify_keyed_many_cached(cache, keyed, msgs)[2]
    u = SIGNERS + 1
    with new_cache(engine, mode) as cache:               # the per-signature call first
        st = per_signature(cache)
        assert int(st[9]) == u and cache.info()["held"] == u
        got, st = run(engine, cache, world.aggs, keys, world.msgs)
        assert got == want and st[HITS] == u and st[INSERTED] == 0
    with new_cache(engine, mode) as cache:               # the aggregate call first
        got, st = run(engine, cache, world.aggs, keys, world.msgs)
        assert got == want and st[INSERTED] == u
        st = per_signature(cache)
        assert int(st[8]) == u and int(st[9]) == 0 and cache.info()["held"] == u


# ------------------------------------------------------------------ slices, eviction, bypass
_CHILD = r"""
import json, os, sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, os.path.join(%(root)r, "oracle"))
sys.path.insert(0, os.path.join(%(root)r, "tests"))
import numpy as np
import torch
import schnorr_sig_amd as ssa
from test_gpu_screened_torsion import special_key_lanes
rng = np.random.default_rng(23801)
n, per = 12345, 40
counts = [2000, 2000, 2000, 2000, 2500, 1845]          # aggregate 2 straddles lane 5000, aggregate 4 lane 10000
e = ssa.Engine(0)
def sc(k):
    v = rng.integers(0, 256, size=(k, 32), dtype=np.uint8); v[:, 31] &= 0x3f; v[:, 0] |= 1
    return v
# slice-disjoint key sets: lanes [0, 5000) by signers 0..39, [5000, 10000) by 40..79, the rest by 80..119
idx = np.concatenate([s * per + np.resize(np.arange(per), c) for s, c in enumerate((5000, 5000, 2345))])
m = rng.integers(0, 256, size=(n, 80), dtype=np.uint8)
pk, sg = e.keygen_sign_many(sc(3 * per)[idx], sc(n), m)
aggs, lo = [], 0
for c in counts:
    st, a, _, _ = e.aggregate(sg[lo:lo + c], pk[lo:lo + c], m[lo:lo + c])
    assert st == 0
    aggs.append(a); lo += c
wire_all = np.concatenate(aggs)
out = {"lane_slice": e.info()["lane_slice"], "cases": []}
os.environ["SSA_LANE_SLICE"] = str(1 << 20)
one = ssa.Engine(0)                                      # the reference: one slice, a cache that never fills
assert one.info()["lane_slice"] == 1 << 20
dev = torch.device("cuda", 0)
for side, lanes in (("left", (4999, 9999)), ("right", (5000, 10000)), ("none", ())):
    p = pk.copy()
    for i in lanes:
        p[i] = special_key_lanes(rng, 1, True)[0]
    w, st = e.compress_many(p)
    assert (st == 0).all()
    for mode, keys in (("affine", p), ("wire", w)):
        with one.keycache_create(4096, wire=(mode == "wire")) as big:
            ref = one.verify_aggregates_cached(big, aggs, keys, m)[0].tolist()
        for evict in ("clear", "recent"):
            for form in ("host", "device"):
                kc = e.keycache_create(64, wire=(mode == "wire"), evict=evict)
                if form == "host":
                    v, stats = e.verify_aggregates_cached(kc, aggs, keys, m)
                    v = v.tolist()
                else:
                    dw, dk, dm = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (wire_all, keys, m))
                    torch.cuda.synchronize()
                    dv, stats = e.verify_aggregates_cached_device(kc, dw, counts, dk, dm)
                    e.sync()
                    v = dv.cpu().tolist()
                out["cases"].append({"side": side, "mode": mode, "evict": evict, "form": form, "v": v, "ref": ref,
                                     "stats": [int(x) for x in stats], "held": kc.info()["held"],
                                     "clears": kc.info()["clears"], "compactions": kc.eviction_info()["compactions"]})
                kc.close()
        # a cache of 8 rows against 40 distinct keys per slice: every slice bypasses it, and it stays as it was
        kc = e.keycache_create(8, wire=(mode == "wire"))
        v, stats = e.verify_aggregates_cached(kc, aggs, keys, m)
        out["cases"].append({"side": side, "mode": mode, "evict": "bypass", "form": "host", "v": v.tolist(), "ref": ref,
                             "stats": [int(x) for x in stats], "held": kc.info()["held"], "clears": kc.info()["clears"],
                             "compactions": 0})
        kc.close()
print("RESULT " + json.dumps(out))
e.close(); one.close()
"""


def test_three_slices_eviction_and_bypass_in_a_child_process():
    """SSA_LANE_SLICE = 5000 in a fresh child process, N = 12 345 in aggregates of which one straddles each slice
    boundary, a key outside the subgroup on the left or on the right of both boundaries.  The key sets of the slices are
    disjoint (40 signers each) and the cache holds 64 rows: the second and third slice clear it (evict="clear") or compact
    it (evict="recent") under the rows the first left, after those were materialised.  The verdicts are those of a
    one-slice engine with a large cache."""
    env = dict(os.environ)
    env["SSA_LANE_SLICE"] = "5000"
    r = subprocess.run([sys.executable, "-c", _CHILD % {"root": ROOT}], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    assert out["lane_slice"] == 5000
    assert len(out["cases"]) == 3 * 2 * 5
    for c in out["cases"]:
        bad = 0 if c["side"] == "none" else 2
        want = [OK, OK, BAD_KEY, OK, BAD_KEY, OK] if bad else [OK] * 6
        assert c["v"] == c["ref"] == want, c
        s = c["stats"]
        # per slice 40 signers, and on the chosen side of a boundary one more key
        assert s[DISTINCT] == 120 + bad and s[BAD_AGGS] == bad and s[BOUND] == 0, c
        if c["evict"] == "bypass":
            assert s[BYPASSED] == 3 and s[HITS] == s[INSERTED] == s[EVICTIONS] == 0, c
            assert c["held"] == 0 and c["clears"] == 0, c
            continue
        assert s[BYPASSED] == 0 and s[HITS] + s[INSERTED] == s[DISTINCT], c
        assert s[EVICTIONS] == 2 and s[HITS] == 0, c            # nothing of an earlier slice returns
        if c["evict"] == "clear":
            assert c["clears"] == 2 and c["compactions"] == 0, c
        else:
            assert c["clears"] + c["compactions"] == 2, c
        assert 40 <= c["held"] <= 64, c


# ------------------------------------------------------------------ hygiene
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("mode", MODES)
def test_hygiene(engine, engines, world, mode, form, path):
    import schnorr_sig_amd as ssa
    eng = engines[path]
    _, _, j, keys, want, _ = [c for c in equality_cases(engine, world, mode) if c[:2] == ("p_plus_t2", "lane_64_of_257")][0]
    bad = world.sigs.copy()
    bad[[7, 1000, 1400], 49] ^= 1
    with new_cache(eng, mode) as cache:
        got, _, tail = run(eng, cache, world.aggs, keys, world.msgs, form, tail=4) if form == "device" else (
            run(eng, cache, world.aggs, keys, world.msgs, form) + ([255] * 4,))
        assert got == want and tail == [255] * 4                 # nothing is written behind verdicts[k)
        for prelude in (lambda: eng.debug_poison_workspaces(0xA5),
                        lambda: eng.verify_batch_screened(bad, world.pks, world.msgs),      # another family's leavings
                        lambda: eng.debug_poison_workspaces(0x01),                          # every byte says "bad key"
                        lambda: None):                                                      # twice in a row
            prelude()
            got, st = run(eng, cache, world.aggs, keys, world.msgs, form)
            assert got == want, got
            check_stats(st, cold=False)
            assert st[BAD_AGGS] == 1
        # messages by offset table, of ragged lengths: lane i keeps 80 - (i % 3) bytes
        rows = [bytes(world.msgs[i, :80 - (i % 3)]) for i in range(N)]
        flat, off = ssa.pack_messages(rows)
        key = ("ragged", mode)
        if key not in _STATE:
            _STATE[key] = expected(engine, world.aggs, keys, flat, offsets=off)[0]
        want_r = _STATE[key]
        # (the honest aggregates were made over 80-byte messages: under shorter ones all but the empty one fail, and the
        #  key still decides in its own)
        assert want_r[j] == BAD_KEY and want_r[0] == OK and set(want_r) == {OK, BAD_KEY, INVALID}
        got, _ = run(eng, cache, world.aggs, keys, flat, form, offsets=off)
        assert got == want_r


# ------------------------------------------------------------------ arguments
def test_wrong_cache_mode_foreign_cache_and_null_cache_are_refused(engine, world):
    import ctypes as C
    import schnorr_sig_amd as ssa
    lib = ssa._lib
    aggs = world.aggs[1:3]
    counts, wire = ssa.pack_aggregates(aggs)
    lo, hi = world.ranges[1][0], world.ranges[2][1]
    pks, w49, msgs = world.pks[lo:hi].copy(), world.wire[lo:hi].copy(), world.msgs[lo:hi].copy()
    out = np.full(2, 255, np.uint32)
    stats = np.full(8, 9, np.uint64)
    cp = counts.ctypes.data_as(C.POINTER(C.c_uint64))
    p = lambda a: C.c_void_p(a.ctypes.data)      # noqa: E731

    def affine_call(ctx, kc):
        return lib.ssa_verify_aggregates_many_cached(ctx, kc, p(wire), cp, 2, p(pks), None, p(msgs), None, 80, 80, p(out),
                                                     stats.ctypes.data)

    def wire_call(ctx, kc):
        return lib.ssa_verify_aggregates_many_cached_wire(ctx, kc, p(wire), cp, 2, p(w49), p(msgs), None, 80, 80, p(out),
                                                          stats.ctypes.data)
    other = ssa.Engine(0)
    try:
        with new_cache(engine, "affine") as ca, new_cache(engine, "wire") as cw, new_cache(other, "affine") as co, \
                new_cache(other, "wire") as cow:
            assert affine_call(engine._ctx, ca.handle) == 0 and out.tolist() == [OK, OK]
            assert wire_call(engine._ctx, cw.handle) == 0
            held = [c.info()["held"] for c in (ca, cw, co, cow)]
            assert held == [len(np.unique(pks, axis=0)), len(np.unique(w49, axis=0)), 0, 0]
            out[:], stats[:] = 255, 9
            assert affine_call(engine._ctx, cw.handle) == ssa.ERR_ARG        # the other mode
            assert wire_call(engine._ctx, ca.handle) == ssa.ERR_ARG
            assert affine_call(engine._ctx, co.handle) == ssa.ERR_ARG        # another context's
            assert wire_call(engine._ctx, cow.handle) == ssa.ERR_ARG
            assert affine_call(engine._ctx, None) == ssa.ERR_ARG             # none
            assert wire_call(engine._ctx, None) == ssa.ERR_ARG
            assert out.tolist() == [255, 255] and stats.tolist() == [9] * 8  # a refused call writes nothing
            assert [c.info()["held"] for c in (ca, cw, co, cow)] == held
            # an error of ssa_verify_aggregates_many is reported as that call reports it, the cache untouched
            assert lib.ssa_verify_aggregates_many_cached(engine._ctx, ca.handle, p(wire), cp, 2, None, None, p(msgs), None,
                                                         80, 80, p(out), stats.ctypes.data) == ssa.ERR_ARG
            assert [c.info()["held"] for c in (ca, cw, co, cow)] == held
    finally:
        other.close()


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("mode", MODES)
def test_no_aggregates_and_only_empty_ones(engine, mode, form):
    width = 49 if mode == "wire" else 96
    none = Keys(engine, mode, np.zeros((0, 96), np.uint8), None, np.zeros((0, 49), np.uint8))
    assert none.arg.shape == (0, width)
    with new_cache(engine, mode) as cache:
        got, st = run(engine, cache, [], none, None, form)
        assert got == [] and st == [0] * 8
        z = np.zeros(32, np.uint8)
        got, st = run(engine, cache, [z, with_e(z, 1), with_e(z, Q)], none, None, form)
        assert got == [OK, INVALID, MALFORMED] and st == [0] * 8
        assert cache.info()["held"] == 0


# ------------------------------------------------------------------ mirrors
@pytest.mark.parametrize("mode", MODES)
def test_the_object_mirror_equals_the_array_call(engine, world, mode):
    import schnorr_sig_amd as ssa
    aggs, pks, wire, msgs, _ = gap_case(engine, world)
    keys = Keys(engine, mode, pks, np.zeros(pks.shape[0], np.uint8), wire)
    objs = [ssa.AggregateSignature(a.tobytes()) for a in aggs]
    pko = [ssa.PublicKey(bytes(k)) for k in pks]
    rows = [bytes(r) for r in msgs]
    with new_cache(engine, mode) as cache:
        want, _ = run(engine, cache, aggs, keys, msgs)
        got = ssa.AggregateSignature.verify_many(objs, pko, rows, cache=cache)
        assert got.tolist() == want == [OK, BAD_KEY, OK]
    assert ssa.AggregateSignature.verify_many(objs, pko, rows, engine=engine).tolist() == [OK, OK, OK]
