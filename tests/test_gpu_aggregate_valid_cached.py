"""Filtering half-aggregation through the key cache, subgroup check included (ssa_aggregate_valid_many_cached and
ssa_aggregate_valid_keyed_many_cached).  The contract is six equalities, each checked against
something computed OUTSIDE the call under test:

  1  status_out        = ssa_verify_many_screened on the unpacked input (subgroup check and flag byte), the 12 statistics
                         words and the state of the cache = those of ssa_verify_many_cached / ssa_verify_keyed_many_cached
  2  kept_out, n_kept  = the lanes of status 0, ascending -- and the lanes the CPU oracle accepts, lane by lane
  3  agg_out           = ssa_aggregate_many (flags 0) on the kept lanes alone, and tests/aggregate_model.py over the oracle
  4  the key outputs   = numpy fancy indexing of the caller's keys
  5  the tails         = zero up to the capacities for n lanes
  6  the validator     = ssa_verify_aggregates_many_cached(_wire) on the same cache answers SSA_OK for what came out

Statuses are deterministic here: every bad lane of these batches either has a key the per-key check refuses or an error
with a prime-order component, which a screened segment accepts with probability about 2^-128.  The
builders below take the signer as an argument, so the expected status vectors were reproduced with the CPU oracle alone
(signing included) before the first GPU run.

"affine" runs the affine form through an affine cache, "wire" the keyed form (130-byte records) through a wire cache."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import aggregate_model as am
from test_gpu_aggregate_valid import EQUALITY_SIZES, FILL, engines  # noqa: F401  (engines: a fixture)
from test_gpu_aggregates_cached import Keys, launches, new_cache, spoil_classes
from test_gpu_screened_torsion import key_choice, make_scalars, special_key_lanes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, BAD_KEY, INVALID, MALFORMED = 0, 1, 2, 3
MODES = ["affine", "wire"]
FORMS = ["host", "device"]
SIGNERS = 40
SMALL_MAX = 3072                       # the default msm_small_max: above it the call goes through the cache
WANT_KEY_STATUS = {"p_plus_t2": BAD_KEY, "order_2_point": BAD_KEY, "noncanonical_limb": MALFORMED, "identity": INVALID,
                   "off_curve": MALFORMED, "bad_flag_bits": MALFORMED, "no_square_root": MALFORMED}
_STATE = {}


# ------------------------------------------------------------------ batches
class Honest:
    """n honest signatures by SIGNERS repeating signers over 80-byte messages, the keys in both forms"""

    def __init__(self, maker, n, seed=0xA24C):
        rng = np.random.default_rng(seed + n)
        self.n = n
        self.msgs = rng.integers(0, 256, size=(n, 80), dtype=np.uint8)
        sks = make_scalars(rng, SIGNERS)[key_choice(rng, n, SIGNERS) if n >= SIGNERS else np.arange(n)]
        self.pks, self.sigs = maker.keygen_sign_many(sks, make_scalars(rng, n), self.msgs)
        self.wire, st = maker.compress_many(self.pks)
        assert (np.asarray(st) == 0).all()
        self.wire = np.asarray(self.wire, np.uint8).reshape(-1, 49)


def honest(engine, n):
    if ("honest", n) not in _STATE:
        _STATE[("honest", n)] = Honest(engine, n)
    return _STATE[("honest", n)]


def even_t2_lane(maker, verify_without_check):
    """(key P + T2, a signature for it whose challenge h is even, its message): ssa_verify_many accepts the lane without
    the subgroup check -- the error term [h] T2 vanishes -- and only the check of the key refuses it"""
    if "t2lane" not in _STATE:
        pkb, s8, m8 = special_key_lanes(np.random.default_rng(0x6A9), 8, True)
        st = verify_without_check(s8, np.tile(pkb, (8, 1)), m8)
        even = np.flatnonzero(np.asarray(st) == 0)
        assert even.size >= 1, "the seed must give a lane with an even h"
        w, cst = maker.compress_many(pkb[None, :])
        assert (np.asarray(cst) == 0).all()
        _STATE["t2lane"] = (pkb, np.asarray(w, np.uint8).reshape(49), s8[even[0]].copy(), m8[even[0]].copy())
    return _STATE["t2lane"]


def placements(n, rng):
    """lane 0, lane n - 1, both sides of the first wave edge, and one at random"""
    lanes = [0, n - 1] + ([63, 64] if n > 65 else [])
    if n > 8:
        lanes.append(int(rng.integers(1, n - 1)))
    return sorted(set(lanes))


def no_point(sig, pm):
    x = sig[:49].copy()
    for t in range(1, 64):
        x[:] = sig[:49]
        x[8] ^= t
        if pm.pt_decompress(x.tobytes())[0] == "invalid":
            return x
    raise AssertionError("no x without a point found")


class Case:
    """a batch with spoiled lanes: `want` is the status every lane must get"""

    def __init__(self, h):
        self.sigs, self.pks, self.wire, self.msgs = h.sigs.copy(), h.pks.copy(), h.wire.copy(), h.msgs.copy()
        self.inf = np.zeros(h.n, np.uint8)
        self.want = np.zeros(h.n, np.uint8)

    def keys(self, engine, mode):
        return Keys(engine, mode, self.pks, self.inf, self.wire)


def spoiled_case(maker, h, cname, spoil, ci):
    """key class `cname` at placement ci of the batch, the three signature classes at the other placements, and from 100
    lanes on one lane with a bad key AND a bad signature"""
    import pymodel as pm
    rng = np.random.default_rng(0x5B01 + 31 * h.n + ci)
    c = Case(h)
    lanes = placements(h.n, rng)
    at = lanes[ci % len(lanes)]
    spoil(c.pks, c.inf, c.wire, at)
    c.want[at] = WANT_KEY_STATUS[cname]
    ways = 0
    for k in lanes:
        if k == at:
            continue
        if ways % 3 == 0:
            c.msgs[k, 17] ^= 0x04                          # the wrong message
            c.want[k] = INVALID
        elif ways % 3 == 1:
            c.sigs[k, :49] = no_point(h.sigs[k], pm)       # R does not decode
            c.want[k] = MALFORMED
        else:
            c.sigs[k, 49:81] = 0xFF                        # e >= q
            c.want[k] = MALFORMED
        ways += 1
    if h.n >= 100:                                         # the key decides
        both = next(k for k in range(70, h.n) if k not in lanes)
        t2 = spoil_classes(maker, "affine")["p_plus_t2"]
        t2(c.pks, c.inf, c.wire, both)
        c.sigs[both, 49] ^= 1
        c.want[both] = BAD_KEY
    c.at = at
    return c


def cases_of(engine, n, mode):
    key = ("cases", n, mode)
    if key not in _STATE:
        h = honest(engine, n)
        _STATE[key] = [(cname, spoiled_case(engine, h, cname, spoil, ci))
                       for ci, (cname, spoil) in enumerate(spoil_classes(engine, mode).items())]
    return _STATE[key]


# ------------------------------------------------------------------ the call under test, on buffers of full capacity
class Got:
    pass


def dev(*arrays):
    import torch
    out = [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0") for a in arrays]
    torch.cuda.synchronize()
    return out


def records(keys, sigs):
    return np.ascontiguousarray(np.concatenate([keys.arg.reshape(-1, 49), sigs.reshape(-1, 81)], axis=1))


def call(eng, cache, mode, form, sigs, keys, msgs, offsets=None, optional=True):
    """one call on output buffers of full capacity filled with 0xEE -> Got: rc, agg[49 n + 32], kept[n], m, status[n],
    keys_out[n, 96 | 49], inf_out[n] (affine), stats[12]; optional=False: every optional output NULL"""
    import schnorr_sig_amd as ssa
    import torch
    n, w = sigs.shape[0], 49 if mode == "wire" else 96
    g = Got()
    stats = np.full(12, 9, np.uint64)
    nk = C.c_uint64(1 << 40)
    if form == "host":
        agg = np.full(49 * n + 32, FILL, np.uint8)
        kept = np.full(max(n, 1), 0xEEEEEEEE, np.uint32)
        status, kout, iout = np.full(max(n, 1), FILL, np.uint8), np.full((max(n, 1), w), FILL, np.uint8), np.full(max(n, 1), FILL, np.uint8)
        m_, off, stride, mlen = eng._msg_args(msgs, offsets, n) if n else (None, None, 0, 0)
        p = ssa._ptr
        opt = lambda a: p(a) if optional else None                                  # noqa: E731
        tail = (p(m_), p(off), stride, mlen, n, p(agg), p(kept), C.byref(nk), opt(status), opt(kout))
        if mode == "affine":
            s_, k_ = np.ascontiguousarray(sigs), np.ascontiguousarray(keys.arg)
            g.rc = ssa._lib.ssa_aggregate_valid_many_cached(eng._ctx, cache.handle, p(s_) if n else None, p(k_) if n else None,
                                                            p(keys.inf), *tail, opt(iout), stats.ctypes.data if optional else None)
        else:
            rec = records(keys, sigs)
            g.rc = ssa._lib.ssa_aggregate_valid_keyed_many_cached(eng._ctx, cache.handle, p(rec) if n else None, *tail,
                                                                  stats.ctypes.data if optional else None)
    else:
        d_msgs = dev(msgs)[0] if msgs is not None else None
        d_off = dev(np.asarray(offsets, np.uint64).view(np.int64))[0] if offsets is not None else None
        d_agg = torch.full((49 * n + 32,), FILL, dtype=torch.uint8, device="cuda:0")
        d_kept = torch.full((max(n, 1),), -0x11111112, dtype=torch.int32, device="cuda:0")
        d_st, d_io = (torch.full((max(n, 1),), FILL, dtype=torch.uint8, device="cuda:0") for _ in range(2))
        d_ko = torch.full((max(n, 1), w), FILL, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        a = lambda t: t.data_ptr() if t is not None and t.numel() else None         # noqa: E731
        opt = lambda t: t.data_ptr() if optional else None                          # noqa: E731
        mlen = 0 if offsets is not None or msgs is None else msgs.shape[1]
        tail = (a(d_msgs), a(d_off), mlen, mlen, n, d_agg.data_ptr(), d_kept.data_ptr(), C.byref(nk), opt(d_st), opt(d_ko))
        if mode == "affine":
            ds, dk, di = dev(sigs, keys.arg, keys.inf)
            g.rc = ssa._lib.ssa_aggregate_valid_many_cached_device(eng._ctx, cache.handle, a(ds), a(dk), a(di), *tail, opt(d_io),
                                                                   stats.ctypes.data if optional else None)
        else:
            dr = dev(records(keys, sigs))[0]
            g.rc = ssa._lib.ssa_aggregate_valid_keyed_many_cached_device(eng._ctx, cache.handle, a(dr), *tail,
                                                                         stats.ctypes.data if optional else None)
        eng.sync()
        agg, kept, status = d_agg.cpu().numpy(), d_kept.cpu().numpy().view(np.uint32), d_st.cpu().numpy()
        kout, iout = d_ko.cpu().numpy(), d_io.cpu().numpy()
    g.agg, g.kept, g.m, g.status, g.keys, g.inf = agg, kept[:n], int(nk.value), status[:n], kout[:n], iout[:n]
    g.stats = [int(x) for x in stats]
    return g


def same(a, b):
    return (a.rc == b.rc and a.m == b.m and a.stats == b.stats and
            all((x == y).all() for x, y in zip((a.agg, a.kept, a.status, a.keys, a.inf), (b.agg, b.kept, b.status, b.keys, b.inf))))


def reference(engine, sigs, keys, msgs, offsets=None):
    """equalities 1 and 3 from the existing calls -> (statuses, K, the aggregate of the kept lanes alone)"""
    import schnorr_sig_amd as ssa
    st = engine.verify_many_screened(sigs, keys.u_pks, msgs, offsets=offsets, check_torsion=True, sig_flag_byte=True,
                                     pk_inf=keys.u_inf)[0]
    K = np.flatnonzero(st == 0)
    if K.size == 0:
        return st, K, np.zeros(32, np.uint8)
    if offsets is None:
        k_msgs, k_off = msgs[K], None
    else:
        k_msgs, k_off = ssa.pack_messages([bytes(msgs[int(offsets[i]):int(offsets[i + 1])]) for i in K])
    rc, alone, _, nf = engine.aggregate(sigs[K], keys.u_pks[K], k_msgs, offsets=k_off, pk_inf=keys.u_inf[K])
    assert rc == OK and nf == 0
    return st, K, alone


def check(g, mode, keys, ref, validator=None, msgs=None):
    """equalities 1 to 6 for one call; validator = (engine, cache) runs the validator's call on what came out"""
    st, K, alone = ref
    n, m = st.size, K.size
    assert g.rc == 0 and g.m == m
    assert (g.status == st).all(), np.flatnonzero(g.status != st)[:8]                        # 1
    assert (g.kept[:m] == K).all() and not g.kept[m:].any()                                  # 2, 5
    assert (g.agg[:49 * m + 32] == alone).all() and not g.agg[49 * m + 32:].any()            # 3, 5
    assert (g.keys[:m] == keys.arg[K]).all() and not g.keys[m:].any()                        # 4, 5
    if mode == "affine":
        assert (g.inf[:m] == (keys.inf[K] if keys.inf is not None else 0)).all() and not g.inf[m:].any()
    if validator:                                                                            # 6
        eng, cache = validator
        v, vst = eng.verify_aggregates_cached(cache, [g.agg[:49 * m + 32]], g.keys[:m], msgs[K] if m else None,
                                              pk_inf=g.inf[:m] if mode == "affine" else None)
        assert v.tolist() == [OK], (v, n, m)
        return vst


# ------------------------------------------------------------------ the gap the feature closes
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n", [5, 3300])
def test_the_gap_between_producer_and_validator_is_closed(engine, n, mode, form):
    """A lane under P + T2 with an even challenge: ssa_aggregate_valid_many keeps it and every validator refuses the
    block; the new call drops it and the validator accepts.  (Fails without the feature: the entry points are missing.)"""
    h = honest(engine, n)
    pkb, w49, sig, msg = even_t2_lane(engine, lambda s, p, m: engine.verify_many(s, p, m, check_torsion=False)[0])
    c, at = Case(h), 2
    c.pks[at], c.wire[at], c.sigs[at], c.msgs[at] = pkb, w49, sig, msg
    keys = c.keys(engine, mode)
    others = np.setdiff1d(np.arange(n), [at])
    with new_cache(engine, mode) as cache:
        # today's producer call keeps the lane ...
        agg0, kept0, st0 = engine.aggregate_valid(c.sigs, keys.u_pks, c.msgs, pk_inf=keys.u_inf)
        assert st0[at] == OK and kept0.tolist() == list(range(n))
        # ... and the validator refuses what it made
        v, _ = engine.verify_aggregates_cached(cache, [agg0], keys.arg, c.msgs, pk_inf=keys.inf)
        assert v.tolist() == [BAD_KEY]
        # the new call gives the lane status 1 and drops it; its aggregate passes
        g = call(engine, cache, mode, form, c.sigs, keys, c.msgs)
        assert g.status[at] == BAD_KEY and g.kept[:g.m].tolist() == others.tolist()
        check(g, mode, keys, reference(engine, c.sigs, keys, c.msgs), validator=(engine, cache), msgs=c.msgs)


# ------------------------------------------------------------------ equalities 1 to 6
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n", EQUALITY_SIZES)
def test_the_equalities_for_every_class_of_bad_lane(engine, oracle, n, mode):
    h = honest(engine, n)
    if ("oracle", n) not in _STATE:         # the honest lanes through the oracle once; a lane's status is its own
        _STATE[("oracle", n)] = oracle.verify_many_fast(h.sigs, h.pks, h.msgs, check_torsion=True, sig_flag_byte=True, threads=16)
    assert not _STATE[("oracle", n)].any()
    modelled = False
    with new_cache(engine, mode) as cache:
        for cname, c in cases_of(engine, n, mode):
            keys = c.keys(engine, mode)
            bad = np.flatnonzero(c.want)
            per_lane = oracle.verify_many_fast(c.sigs[bad], keys.u_pks[bad], c.msgs[bad], check_torsion=True,
                                               sig_flag_byte=True, pk_inf=keys.u_inf[bad], threads=16)
            assert (per_lane == c.want[bad]).all(), (cname, bad, per_lane, c.want[bad])
            ref = reference(engine, c.sigs, keys, c.msgs)
            assert (ref[0] == c.want).all(), (cname, np.flatnonzero(ref[0] != c.want)[:8])
            if not modelled and ref[1].size:  # the model over the oracle: once per size and mode
                K = ref[1]
                model = np.frombuffer(am.aggregate(am.oracle_backend(oracle), c.sigs[K], keys.u_pks[K], c.msgs[K]), np.uint8)
                assert (ref[2] == model).all()
                modelled = True
            for form in FORMS:
                g = call(engine, cache, mode, form, c.sigs, keys, c.msgs)
                check(g, mode, keys, ref, validator=(engine, cache), msgs=c.msgs)
                # at most msm_small_max lanes: the exact path and no screened slice; above: one screened slice
                assert (g.stats[5], g.stats[6]) == (0, 1) if n <= SMALL_MAX else g.stats[5] == 1, (cname, form, g.stats)
    # a NULL pk_inf: pk_inf_out is all zero
    if mode == "affine":
        c = cases_of(engine, n, mode)[0][1]
        keys = Keys(engine, mode, c.pks, None, c.wire)
        with new_cache(engine, mode) as cache:
            for form in FORMS:
                g = call(engine, cache, mode, form, c.sigs, keys, c.msgs)
                check(g, mode, keys, reference(engine, c.sigs, keys, c.msgs))
                assert not g.inf.any()


# ------------------------------------------------------------------ |K| edges
@pytest.mark.parametrize("mode", MODES)
def test_kept_counts_across_the_tree_span_all_bad_none_bad_and_the_empty_batch(engine, mode):
    h = honest(engine, 600)
    with new_cache(engine, mode) as cache:
        for dropped in (87, 88, 89, 600, 0):       # |K| = 513, 512, 511: one workgroup of ag_k_tree more or less
            rng = np.random.default_rng(0x513 + dropped)
            c = Case(h)
            lanes = np.sort(rng.choice(600, size=dropped, replace=False))
            c.sigs[lanes[0::2], 49] ^= 1
            c.pks[lanes[1::2], 48] ^= 1                        # off the curve ...
            c.wire[lanes[1::2], 0:8] = 0xFF                    # ... or not canonical: malformed either way
            keys = c.keys(engine, mode)
            ref = reference(engine, c.sigs, keys, c.msgs)
            assert ref[1].tolist() == np.setdiff1d(np.arange(600), lanes).tolist()
            for form in FORMS:
                g = call(engine, cache, mode, form, c.sigs, keys, c.msgs)
                check(g, mode, keys, ref, validator=(engine, cache), msgs=c.msgs)
                if dropped == 600:
                    assert g.m == 0 and not g.agg.any()
        held = cache.info()["held"]
        none = Keys(engine, mode, np.zeros((0, 96), np.uint8), np.zeros(0, np.uint8), np.zeros((0, 49), np.uint8))
        for form in FORMS:
            g = call(engine, cache, mode, form, np.zeros((0, 81), np.uint8), none, None)
            assert g.rc == 0 and g.m == 0 and g.agg.size == 32 and not g.agg.any() and g.stats == [0] * 12
        assert cache.info()["held"] == held


# ------------------------------------------------------------------ cache states
def big_case(engine, mode):
    """4000 lanes (above msm_small_max: the call uses the cache) with a P + T2 lane and two bad signatures"""
    h = honest(engine, 4000)
    c = Case(h)
    spoil_classes(engine, mode)["p_plus_t2"](c.pks, c.inf, c.wire, 1234)
    c.sigs[[7, 3999], 49] ^= 1
    return c, c.keys(engine, mode)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("mode", MODES)
def test_cold_then_warm_hashes_once_and_builds_nothing_twice(engine, mode, form):
    import schnorr_sig_amd as ssa
    c, keys = big_case(engine, mode)
    ref = reference(engine, c.sigs, keys, c.msgs)
    assert np.flatnonzero(ref[0]).tolist() == [7, 1234, 3999] and ref[0][1234] == BAD_KEY
    u = SIGNERS + 1
    names = ("ssa_k_keyset_build", "ssa_k_keyed_decompress", "ssa_k_hash", "av_k_gather", "av_k_gather_keys", "av_k_keep")
    eng = ssa.Engine(0)
    try:
        with new_cache(eng, mode) as cache, new_cache(eng, mode) as twin:
            eng.enable_timing(True)

            def counts():
                return {k: launches(eng, k) for k in names}
            counts()                                         # drains the keys
            for cold in (True, False):
                g = call(eng, cache, mode, form, c.sigs, keys, c.msgs)
                got = counts()
                check(g, mode, keys, ref)
                assert got["ssa_k_hash"] == 1, got           # every message hashed once: one slice, one launch
                assert got["ssa_k_keyset_build"] == (1 if cold else 0), got
                assert got["ssa_k_keyed_decompress"] == (1 if cold and mode == "wire" else 0), got
                assert got["av_k_gather"] == got["av_k_gather_keys"] == got["av_k_keep"] == 1, got
                assert g.stats[0] == u and g.stats[8] == (0 if cold else u) and g.stats[9] == (u if cold else 0), g.stats
                # the statistics and the cache's state are those of the per-signature call on a cache of its own
                if mode == "affine":
                    st, _, stats = eng.verify_many_cached(twin, c.sigs, keys.arg, c.msgs, pk_inf=keys.inf, sig_flag_byte=True)
                else:
                    st, _, stats = eng.verify_keyed_many_cached(twin, records(keys, c.sigs), c.msgs, sig_flag_byte=True)
                assert (st == g.status).all() and [int(x) for x in stats] == g.stats
                assert cache.info() == twin.info() and cache.info()["held"] == u
                counts()
            # the validator's call on the same cache builds and decompresses nothing (equality 6)
            vst = check(g, mode, keys, ref, validator=(eng, cache), msgs=c.msgs)
            got = counts()
            assert got["ssa_k_keyset_build"] == 0 and got["ssa_k_keyed_decompress"] == 0, got
            assert int(vst[2]) == 0 and int(vst[1]) == int(vst[0])
            eng.enable_timing(False)
            cache.clear()                                    # cleared between two calls: cold again, the same bytes
            g2 = call(eng, cache, mode, form, c.sigs, keys, c.msgs)
            assert g2.stats[9] == u and (g2.agg == g.agg).all() and (g2.kept == g.kept).all()
    finally:
        eng.close()


@pytest.mark.parametrize("mode", MODES)
def test_the_per_signature_call_and_the_new_call_warm_each_other(engine, mode):
    c, keys = big_case(engine, mode)
    ref = reference(engine, c.sigs, keys, c.msgs)
    u = SIGNERS + 1

    def per_signature(cache):
        if mode == "affine":
            return engine.verify_many_cached(cache, c.sigs, keys.arg, c.msgs, pk_inf=keys.inf, sig_flag_byte=True)[2]
        return engine.verify_keyed_many_cached(cache, records(keys, c.sigs), c.msgs, sig_flag_byte=True)[2]
    with new_cache(engine, mode) as cache:
        assert int(per_signature(cache)[9]) == u
        g = call(engine, cache, mode, "host", c.sigs, keys, c.msgs)
        check(g, mode, keys, ref)
        assert g.stats[8] == u and g.stats[9] == 0
    with new_cache(engine, mode) as cache:
        g = call(engine, cache, mode, "device", c.sigs, keys, c.msgs)
        check(g, mode, keys, ref)
        assert g.stats[9] == u
        st = per_signature(cache)
        assert int(st[8]) == u and int(st[9]) == 0 and cache.info()["held"] == u
    # partly warm: the cache knows the signers of the first 20 lanes (their lanes repeated up to a batch that uses it)
    with new_cache(engine, mode) as cache:
        half = np.flatnonzero((c.pks[:, None, :8] == c.pks[None, :20, :8]).all(axis=2).any(axis=1))
        idx = np.resize(half, 3200)
        hk = Keys(engine, mode, c.pks[idx], c.inf[idx], c.wire[idx])
        assert call(engine, cache, mode, "host", c.sigs[idx], hk, c.msgs[idx]).rc == 0
        held = cache.info()["held"]
        assert 0 < held < u
        g = call(engine, cache, mode, "host", c.sigs, keys, c.msgs)
        check(g, mode, keys, ref, validator=(engine, cache), msgs=c.msgs)
        assert g.stats[8] == held and g.stats[9] == u - held


# ------------------------------------------------------------------ slices, eviction, bypass
_CHILD = r"""
import json, os, sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, os.path.join(%(root)r, "oracle"))
sys.path.insert(0, os.path.join(%(root)r, "tests"))
import numpy as np
import schnorr_sig_amd as ssa
import test_gpu_aggregate_valid_cached as t
from test_gpu_aggregates_cached import Keys, spoil_classes
e = ssa.Engine(0)                                        # SSA_LANE_SLICE=1024, SSA_MSM_SMALL_MAX=500
os.environ["SSA_LANE_SLICE"] = str(1 << 20)
one = ssa.Engine(0)                                      # the reference: one slice, a cache that never fills
rng = np.random.default_rng(0x511CE)
n, per = 2500, 40                                        # slices of 1024, 1024 and 452 lanes; the last takes the exact path
idx = np.concatenate([s * per + np.resize(np.arange(per), c) for s, c in enumerate((1024, 1024, 452))])
m = rng.integers(0, 256, size=(n, 80), dtype=np.uint8)
sks = t.make_scalars(rng, 3 * per)
pk, sg = e.keygen_sign_many(sks[idx], t.make_scalars(rng, n), m)
w, st = e.compress_many(pk)
assert (st == 0).all()
out = {"lane_slice": e.info()["lane_slice"], "one": one.info()["lane_slice"], "cases": []}
for side, lanes in (("left", (1023, 2047)), ("right", (1024, 2048)), ("none", ())):
    p, wk, inf, s = pk.copy(), w.copy(), np.zeros(n, np.uint8), sg.copy()
    for i in lanes:                                      # a dropped lane on one side of each edge, kept lanes around it
        spoil_classes(e, "affine")["p_plus_t2"](p, inf, wk, i)
    for mode in t.MODES:
        keys = Keys(e, mode, p, inf, wk)
        with one.keycache_create(4096, wire=(mode == "wire")) as big:
            ref = t.call(one, big, mode, "host", s, keys, m)
        t.check(ref, mode, keys, t.reference(one, s, keys, m))
        for evict, cap, forms in (("clear", 64, t.FORMS), ("recent", 64, t.FORMS[:1]), ("clear", 8, t.FORMS[1:])):
            for form in forms:
                kc = e.keycache_create(cap, wire=(mode == "wire"), evict=evict)
                tw = e.keycache_create(cap, wire=(mode == "wire"), evict=evict)
                e.enable_timing(True)
                e.read_timing("ssa_k_hash")
                g = t.call(e, kc, mode, form, s, keys, m)
                hashes = e.read_timing("ssa_k_hash")[1]
                e.enable_timing(False)
                if mode == "affine":
                    st2, _, stats2 = e.verify_many_cached(tw, s, keys.arg, m, pk_inf=keys.inf, sig_flag_byte=True)
                else:
                    st2, _, stats2 = e.verify_keyed_many_cached(tw, t.records(keys, s), m, sig_flag_byte=True)
                out["cases"].append({
                    "side": side, "mode": mode, "evict": evict, "cap": cap, "form": form, "hashes": int(hashes),
                    "same_bytes": bool((g.agg == ref.agg).all() and (g.kept == ref.kept).all() and (g.keys == ref.keys).all()
                                       and (g.inf == ref.inf).all() and (g.status == ref.status).all() and g.m == ref.m),
                    "dropped": np.flatnonzero(g.status).tolist(), "stats": g.stats, "stats_twin": [int(x) for x in stats2],
                    "same_status": bool((st2 == g.status).all()), "info": kc.info(), "info_twin": tw.info(),
                    "evict_info": [int(kc.eviction_info()[k]) for k in ("compactions", "dropped")],
                    "evict_twin": [int(tw.eviction_info()[k]) for k in ("compactions", "dropped")]})
                kc.close(); tw.close()
print("RESULT " + json.dumps(out))
e.close(); one.close()
"""


def test_three_slices_eviction_and_bypass_in_a_child_process():
    """SSA_LANE_SLICE = 1024 and SSA_MSM_SMALL_MAX = 500 in a child process, n = 2 500: two slices through the cache and a
    last one of 452 lanes on the exact path.  The key sets of the slices are disjoint (40 signers each): a cache of 64 rows
    is cleared or compacted by the second slice, one of 8 rows is bypassed.  A lane is dropped on the left or the right of
    both slice edges.  Every output is byte for byte that of a one-slice engine with a large cache; statistics and cache
    state are those of the per-signature call on a cache of its own; the affine form hashes once for the whole call, the
    keyed form once per slice."""
    env = dict(os.environ)
    env["SSA_LANE_SLICE"], env["SSA_MSM_SMALL_MAX"] = "1024", "500"
    r = subprocess.run([sys.executable, "-c", _CHILD % {"root": ROOT}], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    assert out["lane_slice"] == 1024 and out["one"] == 1 << 20
    assert len(out["cases"]) == 3 * 2 * 4                    # (both forms under "clear", one each under "recent" and the bypass)
    for c in out["cases"]:
        lanes = {"left": [1023, 2047], "right": [1024, 2048], "none": []}[c["side"]]
        assert c["same_bytes"] and c["same_status"] and c["dropped"] == lanes, c
        assert c["stats"] == c["stats_twin"] and c["info"] == c["info_twin"] and c["evict_info"] == c["evict_twin"], c
        assert c["hashes"] == (1 if c["mode"] == "affine" else 3), c
        s = c["stats"]
        bad_in_cached_slices = sum(1 for k in lanes if k < 2048)
        assert s[0] == 80 + bad_in_cached_slices and s[5] == 2 and s[6] == 1, c     # two screened slices, one exact
        if c["cap"] == 8:
            assert s[11] == 2 and s[8] == s[9] == s[10] == 0 and c["info"]["held"] == 0, c
        else:
            assert s[11] == 0 and s[8] + s[9] == s[0] and s[10] == 1 and 40 <= c["info"]["held"] <= 64, c


# ------------------------------------------------------------------ forms, layouts, screen paths
@pytest.mark.parametrize("path", ["small", "bucket"])
@pytest.mark.parametrize("mode", MODES)
def test_layouts_forms_and_both_screen_paths(engine, engines, mode, path):
    import schnorr_sig_amd as ssa
    eng = engines[path]
    n = 300
    c = cases_of(engine, n, mode)[0][1]
    keys = c.keys(engine, mode)
    ref = reference(engine, c.sigs, keys, c.msgs)
    # messages by offset table, of ragged lengths, some empty: signed anew, then the same spoils
    rng = np.random.default_rng(0x1A70)
    lens = rng.integers(0, 100, size=n)
    lens[[0, 7, n - 1]] = 0
    rows = [rng.bytes(int(k)) for k in lens]
    flat, off = ssa.pack_messages(rows)
    h = honest(engine, n)
    sks = make_scalars(np.random.default_rng(0x77), n)
    pks, sigs = engine.keygen_sign_many(sks, make_scalars(rng, n), flat, offsets=off)
    wire, _ = engine.compress_many(pks)
    r = Case(h)
    r.sigs, r.pks, r.wire = sigs.copy(), pks.copy(), np.asarray(wire, np.uint8).reshape(-1, 49).copy()
    spoil_classes(engine, mode)["p_plus_t2"](r.pks, r.inf, r.wire, 64)
    r.sigs[[0, 63, n - 1], 49] ^= 1
    rkeys = r.keys(engine, mode)
    rref = reference(engine, r.sigs, rkeys, flat, offsets=off)
    assert np.flatnonzero(rref[0]).tolist() == [0, 63, 64, n - 1] and rref[0][64] == BAD_KEY
    with new_cache(eng, mode) as cache:
        for form in FORMS:
            g = call(eng, cache, mode, form, c.sigs, keys, c.msgs)
            if form == FORMS[0]:                             # (the validator's call below uses the cache at every size)
                assert (cache.info()["held"] > 0) == (path == "bucket")
            check(g, mode, keys, ref, validator=(eng, cache), msgs=c.msgs)
            assert (g.stats[5], g.stats[6]) == ((0, 1) if path == "small" else (1, g.stats[6]))   # exact | one screened slice
            g = call(eng, cache, mode, form, r.sigs, rkeys, flat, offsets=off)
            check(g, mode, rkeys, rref)
            # no optional output wanted
            g0 = call(eng, cache, mode, form, c.sigs, keys, c.msgs, optional=False)
            assert g0.rc == 0 and g0.m == ref[1].size and (g0.agg[:49 * g0.m + 32] == ref[2]).all() and (g0.kept[:g0.m] == ref[1]).all()
            assert (g0.status == FILL).all() and (g0.keys == FILL).all() and (g0.inf == FILL).all() and g0.stats == [9] * 12


# ------------------------------------------------------------------ hygiene
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("mode", MODES)
def test_hygiene(engine, mode, form):
    """poisoned workspaces -- the byte that reads as "bad key" included -- and a dirty predecessor change nothing: every
    output is that of the same call on a fresh context"""
    import schnorr_sig_amd as ssa
    c, keys = big_case(engine, mode)
    small = cases_of(engine, 300, mode)[1][1]
    skeys = small.keys(engine, mode)
    fresh = ssa.Engine(0)
    try:
        with new_cache(fresh, mode) as fc:
            want = call(fresh, fc, mode, form, c.sigs, keys, c.msgs)
            want_warm = call(fresh, fc, mode, form, c.sigs, keys, c.msgs)
            want_small = call(fresh, fc, mode, form, small.sigs, skeys, small.msgs)
    finally:
        fresh.close()
    check(want, mode, keys, reference(engine, c.sigs, keys, c.msgs))
    bad = c.sigs.copy()
    bad[::3, 49] ^= 1

    def dirty():
        engine.verify_batch_screened(bad, keys.u_pks, c.msgs)                       # another family's leavings
        engine.aggregate_valid(bad[:700], keys.u_pks[:700], c.msgs[:700])           # fills ws_h, ag_dig, av_* of another size
    with new_cache(engine, mode) as cache:
        assert same(call(engine, cache, mode, form, c.sigs, keys, c.msgs), want)
        for prelude in (lambda: engine.debug_poison_workspaces(0xA5), dirty, lambda: engine.debug_poison_workspaces(0x01),
                        lambda: None):
            prelude()
            assert same(call(engine, cache, mode, form, c.sigs, keys, c.msgs), want_warm)
        engine.debug_poison_workspaces(0x01)
        assert same(call(engine, cache, mode, form, small.sigs, skeys, small.msgs), want_small)


# ------------------------------------------------------------------ arguments
def test_argument_errors_leave_the_cache_untouched(engine):
    import schnorr_sig_amd as ssa
    lib, p = ssa._lib, ssa._ptr
    h = honest(engine, 600)
    n = 600
    sigs, pks, msgs = h.sigs, h.pks, h.msgs
    rec = np.ascontiguousarray(np.concatenate([h.wire, sigs], axis=1))
    agg, kept, nk = np.full(49 * n + 32, FILL, np.uint8), np.full(n, 0xEEEEEEEE, np.uint32), C.c_uint64(77)
    stats = np.full(12, 9, np.uint64)

    def affine(ctx, kc, a=agg, k=kept, c=nk, count=n):
        return lib.ssa_aggregate_valid_many_cached(ctx, kc, p(sigs), p(pks), None, p(msgs), None, 80, 80, count,
                                                   p(a) if a is not None else None, p(k) if k is not None else None,
                                                   C.byref(c) if c is not None else None, None, None, None, stats.ctypes.data)

    def keyed(ctx, kc, a=agg, k=kept, c=nk, count=n):
        return lib.ssa_aggregate_valid_keyed_many_cached(ctx, kc, p(rec), p(msgs), None, 80, 80, count,
                                                         p(a) if a is not None else None, p(k) if k is not None else None,
                                                         C.byref(c) if c is not None else None, None, None, stats.ctypes.data)
    other = ssa.Engine(0)
    old = os.environ.get("SSA_MSM_SLICE")
    os.environ["SSA_MSM_SLICE"] = "512"
    try:
        tight = ssa.Engine(0)
    finally:
        if old is None:
            os.environ.pop("SSA_MSM_SLICE", None)
        else:
            os.environ["SSA_MSM_SLICE"] = old
    try:
        with new_cache(engine, "affine") as ca, new_cache(engine, "wire") as cw, new_cache(other, "affine") as co, \
                new_cache(other, "wire") as cow, new_cache(tight, "affine") as ta, new_cache(tight, "wire") as tw:
            # warm the two caches with a call that uses them
            big, bk = big_case(engine, "affine")
            assert call(engine, ca, "affine", "host", big.sigs, bk, big.msgs).rc == 0
            bkw = big.keys(engine, "wire")
            assert call(engine, cw, "wire", "host", big.sigs, bkw, big.msgs).rc == 0
            caches = (ca, cw, co, cow, ta, tw)
            before = [c.info() for c in caches]
            assert before[0]["held"] == before[1]["held"] == SIGNERS + 1
            agg[:], kept[:], stats[:], nk.value = FILL, 0xEEEEEEEE, 9, 77
            assert affine(engine._ctx, cw.handle) == ssa.ERR_ARG          # the other mode
            assert keyed(engine._ctx, ca.handle) == ssa.ERR_ARG
            assert affine(engine._ctx, co.handle) == ssa.ERR_ARG          # another context's
            assert keyed(engine._ctx, cow.handle) == ssa.ERR_ARG
            assert affine(engine._ctx, None) == ssa.ERR_ARG               # none
            assert keyed(engine._ctx, None) == ssa.ERR_ARG
            assert affine(None, ca.handle) == ssa.ERR_ARG
            for fn, kc in ((affine, ca), (keyed, cw)):
                assert fn(engine._ctx, kc.handle, a=None) == ssa.ERR_ARG
                assert fn(engine._ctx, kc.handle, k=None) == ssa.ERR_ARG
                assert fn(engine._ctx, kc.handle, c=None) == ssa.ERR_ARG
            # n above the context's MSM slice
            assert affine(tight._ctx, ta.handle) == ssa.ERR_ARG and keyed(tight._ctx, tw.handle) == ssa.ERR_ARG
            # a refused call writes nothing and leaves every cache as it was
            assert (agg == FILL).all() and (kept == 0xEEEEEEEE).all() and stats.tolist() == [9] * 12 and nk.value == 77
            assert [c.info() for c in caches] == before
            # ... and at the slice the calls run
            assert affine(tight._ctx, ta.handle, count=512) == 0 and nk.value == 512
            assert keyed(tight._ctx, tw.handle, count=512) == 0 and nk.value == 512
        # an orphaned cache: its context is gone
        gone = ssa.Engine(0)
        orphan = new_cache(gone, "affine")
        gone.close()
        assert affine(engine._ctx, orphan.handle) == ssa.ERR_ARG
        orphan.close()
    finally:
        other.close()
        tight.close()


# ------------------------------------------------------------------ the object mirror
@pytest.mark.parametrize("mode", MODES)
def test_the_object_mirror_equals_the_array_call(engine, mode):
    import schnorr_sig_amd as ssa
    h = honest(engine, 5)
    pkb, w49, sig, msg = even_t2_lane(engine, lambda s, p, m: engine.verify_many(s, p, m, check_torsion=False)[0])
    c = Case(h)
    c.pks[2], c.wire[2], c.sigs[2], c.msgs[2] = pkb, w49, sig, msg
    c.sigs[4, 49] ^= 1
    keys = c.keys(engine, mode)
    so = [ssa.Signature(bytes(s)) for s in c.sigs]
    pko = [ssa.PublicKey(bytes(k)) for k in c.pks]
    rows = [bytes(r) for r in c.msgs]
    with new_cache(engine, mode) as cache:
        g = call(engine, cache, mode, "host", c.sigs, keys, c.msgs)
        agg, kept = ssa.AggregateSignature.aggregate_valid(so, pko, rows, cache=cache)
        assert kept == g.kept[:g.m].tolist() == [0, 1, 3] and agg.bytes == g.agg[:49 * g.m + 32].tobytes()
        sub = lambda xs: [xs[i] for i in kept]               # noqa: E731
        assert ssa.AggregateSignature.verify_many([agg], sub(pko), sub(rows), cache=cache).tolist() == [OK]
        if mode == "affine":
            out = engine.aggregate_valid_cached(cache, c.sigs, c.pks, c.msgs, pk_inf=c.inf)
            assert (out[0] == g.agg[:49 * g.m + 32]).all() and out[1].tolist() == kept and (out[2] == g.status).all()
            assert (out[3] == c.pks[kept]).all() and not out[4].any() and [int(x) for x in out[5]] == g.stats
            with pytest.raises(ValueError):
                engine.aggregate_valid_keyed_cached(cache, records(c.keys(engine, "wire"), c.sigs), c.msgs)
        else:
            out = engine.aggregate_valid_keyed_cached(cache, records(keys, c.sigs), c.msgs)
            assert (out[0] == g.agg[:49 * g.m + 32]).all() and out[1].tolist() == kept and (out[2] == g.status).all()
            assert (out[3] == c.wire[kept]).all() and [int(x) for x in out[4]] == g.stats
            with pytest.raises(ValueError):
                engine.aggregate_valid_cached(cache, c.sigs, c.pks, c.msgs)
    # without a cache the method is what it was: the lane is kept
    agg0, kept0 = ssa.AggregateSignature.aggregate_valid(so, pko, rows, engine=engine)
    assert kept0 == [0, 1, 2, 3]
