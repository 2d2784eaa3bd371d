"""Key cache eviction by compaction (ssa_keycache_set_eviction).  Every cached call is compared as
tests/test_gpu_keycache.py and tests/test_gpu_keyed_cache.py compare theirs: lane for lane with ssa_verify_many, byte for
byte with ssa_verify_many_screened under the same coefficients.  The numbers each scenario expects (rows kept, moved,
dropped) were worked out by hand from the keep rule; tests/test_keycache_evict_host.py checks the same cases on the host.

Batches are 5000 lanes, just above SSA_MSM_SMALL_MAX, so that the cache is used.  The lanes of one key are contiguous and
the keys follow each other in the order of the list they come from: whichever lane represents a key, the rows of a call
are in list order, so the row numbers -- and with them the number of rows a compaction moves -- are determined."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import test_gpu_keycache as KC
import test_gpu_keyed_cache as KY
from test_gpu_screened_torsion import T, coeffs32, make_scalars, spoiled_batch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HITS, INSERTED, EVICTIONS, BYPASSED = 8, 9, 10, 11
N = 5000
MODES = ["affine", "wire"]


@pytest.fixture(scope="module")
def timing_engine():
    """an engine of this module's own for the tests that switch timing on: the events their calls record under keys they
    do not read would otherwise stay on the session's engine and be counted by whichever test reads those keys next"""
    import schnorr_sig_amd as ssa
    eng = ssa.Engine(0)
    yield eng
    eng.close()


class Batch:
    """N lanes signed by the secret keys `pool`, key k on the lanes [k N / len, (k + 1) N / len); its reference, once"""

    def __init__(self, engine, rng, pool, mode, n=N, bad=(), garbage=()):
        self.mode, self.n = mode, n
        self.idx = (np.arange(n) * pool.shape[0]) // n
        msgs = rng.integers(0, 256, size=(n, 80), dtype=np.uint8)
        pks, out = engine.keygen_sign_many(pool[self.idx], make_scalars(rng, n), msgs, keyed=(mode == "wire"))
        self.arrays = [out, msgs] if mode == "wire" else [out, pks, msgs]
        for i in bad:                                   # a signature that does not verify
            out[i, (99 if mode == "wire" else 50)] ^= 1
        for k in garbage:                               # key k of the pool replaced by a malformed one, on all its lanes
            (out if mode == "wire" else pks)[self.idx == k, 0:8] = 0xFF
        self.co = coeffs32(rng, n)
        self._ref = None

    def ref(self, engine):
        if self._ref is None:
            self._ref = (KY if self.mode == "wire" else KC).reference(engine, *self.arrays, T, self.co)
        return self._ref

    def run(self, engine, cache, form="host"):
        """one cached call, compared with the reference -> (statuses, statistics)"""
        return (KY if self.mode == "wire" else KC).cached(engine, cache, *self.arrays, T, self.co, self.ref(engine), form=form)


def new_cache(engine, capacity, mode, evict="recent"):
    return engine.keycache_create(capacity, wire=(mode == "wire"), evict=evict)


def expect(stats, cache, hits, inserted, evictions, held):
    assert (stats[HITS], stats[INSERTED], stats[EVICTIONS], stats[BYPASSED]) == (hits, inserted, evictions, 0), stats
    assert stats[HITS] + stats[INSERTED] == stats[0] and stats[7] == 0, stats
    assert cache.info()["held"] == held, cache.info()


def key_launches(engine):
    return engine.read_timing("ssa_k_keyset_build")[1], engine.read_timing("ssa_k_keyed_decompress")[1]


def survivors_at_the_top(engine, mode, form, before_third_call=None):
    """Scenario 1 of the issue, capacity 64 -> the statuses and statistics of its third call.  A (30 keys), B (20 others),
    then B and 20 new keys: 50 + 20 > 64, hist = {0: 20, 2: 30}, budget max(20, 44 / 2) = 22, a* = 1, K = 20.  B's rows
    are 30..49, all at or above K: every survivor moves."""
    rng = np.random.default_rng(19101)
    sks = make_scalars(rng, 70)
    a, b = Batch(engine, rng, sks[:30], mode, bad=(7, 4000)), Batch(engine, rng, sks[30:50], mode, bad=(0, N - 1))
    bc = Batch(engine, rng, sks[30:70], mode, bad=(3, 2499, 2500, N - 1))
    with new_cache(engine, 64, mode) as cache:
        assert cache.eviction_info() == {"policy": "recent", "compactions": 0, "dropped": 0, "last_kept": 0, "last_moved": 0,
                                         "epoch": 0}
        expect(a.run(engine, cache, form)[1], cache, 0, 30, 0, 30)
        expect(b.run(engine, cache, form)[1], cache, 0, 20, 0, 50)
        if before_third_call:
            before_third_call()
        st3, stats3 = bc.run(engine, cache, form)
        expect(stats3, cache, 20, 20, 1, 40)
        ev = cache.eviction_info()
        assert ev == {"policy": "recent", "compactions": 1, "dropped": 30, "last_kept": 20, "last_moved": 20, "epoch": 3}
        assert cache.info()["clears"] == 0                    # a compaction is no clear
        engine.enable_timing(True)
        try:
            key_launches(engine)                              # drains the keys
            expect(b.run(engine, cache, form)[1], cache, 20, 0, 0, 40)
            assert key_launches(engine) == (0, 0), "a key that is still in use is not checked twice"
            assert engine.read_timing("keycache_compact")[1] == 0
        finally:
            engine.enable_timing(False)
        # A again: 30 misses, 40 + 30 > 64, hist = {1: 20, 2: 20}, budget max(0, 34 / 2) = 17: nothing fits
        expect(a.run(engine, cache, form)[1], cache, 0, 30, 1, 30)
        ev = cache.eviction_info()
        assert (ev["compactions"], ev["dropped"], ev["last_kept"], ev["last_moved"]) == (2, 70, 0, 0), ev
        expect(a.run(engine, cache, "device" if form == "host" else "host")[1], cache, 30, 0, 0, 30)
        assert cache.selfcheck(deep=True)["ok"]
    return st3, stats3


@pytest.mark.parametrize("form", ["host", "device"])
@pytest.mark.parametrize("mode", MODES)
def test_survivors_at_the_top_everything_moves(timing_engine, mode, form):
    """(on the parent the third call clears the cache and reports no hit)"""
    survivors_at_the_top(timing_engine, mode, form)


@pytest.mark.parametrize("mode", MODES)
def test_survivors_at_the_bottom_nothing_moves(engine, mode):
    """A (30 keys), B (30 others), then A and 10 new keys: 60 + 10 > 64, hist = {0: 30, 1: 30}, budget max(30, 27) = 30,
    K = 30, and A's rows 0..29 are where they stay"""
    rng = np.random.default_rng(19201)
    sks = make_scalars(rng, 70)
    a, b = Batch(engine, rng, sks[:30], mode), Batch(engine, rng, sks[30:60], mode, bad=(5,))
    ac = Batch(engine, rng, np.concatenate([sks[:30], sks[60:]]), mode, bad=(11, 4990))
    with new_cache(engine, 64, mode) as cache:
        expect(a.run(engine, cache)[1], cache, 0, 30, 0, 30)
        expect(b.run(engine, cache, "device")[1], cache, 0, 30, 0, 60)
        expect(ac.run(engine, cache, "device")[1], cache, 30, 10, 1, 40)
        ev = cache.eviction_info()
        assert (ev["compactions"], ev["dropped"], ev["last_kept"], ev["last_moved"]) == (1, 30, 30, 0), ev
        expect(ac.run(engine, cache)[1], cache, 40, 0, 0, 40)
        expect(b.run(engine, cache)[1], cache, 0, 30, 1, 30)      # 40 + 30 > 64, budget 17 < 40: nothing fits
        assert cache.selfcheck(deep=True)["ok"]


@pytest.mark.parametrize("form", ["host", "device"])
@pytest.mark.parametrize("mode", MODES)
def test_a_flood_of_fresh_keys_never_evicts_the_validators(timing_engine, mode, form):
    """30 validator keys and 30 never-seen keys per call, interleaved, one of the fresh keys malformed garbage.  From the
    second call on: u = 60, m = 30, 60 + 30 > 64, hist = {0: 30, 1: 30}, budget max(30, 17) = 30: exactly the validators
    stay.  In the second call they sit at the even rows: 15 of them are at rows >= 30 and fill the 15 holes below."""
    engine = timing_engine
    rng = np.random.default_rng(19301)
    v = make_scalars(rng, 30)
    with new_cache(engine, 64, mode) as cache:
        engine.enable_timing(True)
        try:
            engine.read_timing("keycache_compact")            # drains the key
            for call in range(6):
                pool = np.empty((60, 32), np.uint8)
                pool[0::2], pool[1::2] = v, make_scalars(rng, 30)
                lanes_of_v = [int(x) for x in np.nonzero((np.arange(N) * 60 // N) % 2 == 0)[0][[0, 9, 777, -1]]]
                batch = Batch(engine, rng, pool, mode, bad=lanes_of_v, garbage=(2 * (call % 30) + 1,))
                st, stats = batch.run(engine, cache, form)
                assert (st[lanes_of_v] == 2).all() and int((st == 3).sum()) == int((batch.idx == 2 * (call % 30) + 1).sum())
                if call == 0:
                    expect(stats, cache, 0, 60, 0, 60)
                    continue
                expect(stats, cache, 30, 30, 1, 60)
                ev = cache.eviction_info()
                assert (ev["compactions"], ev["last_kept"], ev["last_moved"]) == (call, 30, 15 if call == 1 else 0), ev
                assert ev["dropped"] == 30 * call
            assert engine.read_timing("keycache_compact")[1] == 3 * 5      # three timed stages per compaction
        finally:
            engine.enable_timing(False)
        assert cache.info()["clears"] == 0 and cache.selfcheck(deep=True)["ok"]


@pytest.mark.parametrize("mode", MODES)
def test_more_than_one_workgroup(engine, mode):
    """capacity 1024: 900 keys, then every third of them and 200 new ones: 900 + 200 > 1024, hist = {0: 300, 1: 600},
    budget max(300, 824 / 2) = 412, K = 300.  The survivors are rows 0, 3, 6, ..: 100 below row 300, 200 to move."""
    rng = np.random.default_rng(19401)
    sks = make_scalars(rng, 1100)
    first = Batch(engine, rng, sks[:900], mode, bad=(1, 2600))
    third = Batch(engine, rng, sks[0:900:3], mode, bad=(17,))
    mixed = Batch(engine, rng, np.concatenate([sks[0:900:3], sks[900:]]), mode, bad=(0, 3001, N - 1))
    with new_cache(engine, 1024, mode) as cache:
        expect(first.run(engine, cache, "device")[1], cache, 0, 900, 0, 900)
        expect(mixed.run(engine, cache, "device")[1], cache, 300, 200, 1, 500)
        ev = cache.eviction_info()
        assert (ev["compactions"], ev["dropped"], ev["last_kept"], ev["last_moved"]) == (1, 600, 300, 200), ev
        expect(third.run(engine, cache)[1], cache, 300, 0, 0, 500)
        expect(mixed.run(engine, cache)[1], cache, 500, 0, 0, 500)
        res = cache.selfcheck(deep=True)
        assert res["ok"] and res["keys_checked"] == 500, res


def _rows(cache, mode):
    """every held row as {identity: (table, status, key words, pk_inf[, wire words])}"""
    out = {}
    for r in range(cache.info()["held"]):
        words = [cache.debug_keytab_read(w, r) for w in ((0, 1, 2, 3, 5) if mode == "wire" else (0, 1, 2, 3))]
        ident = words[4].tobytes() if mode == "wire" else words[2].tobytes() + bytes([int(words[3][0])])
        assert ident not in out
        out[ident] = (r, [w.copy() for w in words])
    return out


def test_rows_arrive_intact_affine(engine):
    """Rows are read before and after a compaction that moves every survivor; each survivor, found again by its key bytes
    and pk_inf, holds the same table, status, key and flag.  Among the survivors: the identity key (pk_inf = 1), a key of
    small order (status 1) and a malformed key (status 3), all out of spoiled_batch."""
    rng = np.random.default_rng(19501)
    (sigs, pks, msgs, inf), touched, g, _ = spoiled_batch(engine, rng, n=20000, u=80)
    clean = np.setdiff1d(np.arange(20000), touched)
    keys, first = np.unique(pks[clean], axis=0, return_index=True)
    assert keys.shape[0] == 80
    by_key = [clean[(pks[clean] == k).all(axis=1)] for k in keys]

    def batch(key_numbers, special=()):
        lanes = [ln for k in key_numbers for ln in by_key[k][:N // 48]]
        lanes += [int(ln) for name in special for ln in g[name]]
        lanes = np.array((lanes * (N // len(lanes) + 1))[:N + 300])
        return sigs[lanes], pks[lanes], msgs[lanes], inf[lanes]

    def run(cache, b):
        co = coeffs32(rng, b[0].shape[0])
        ref = KC.reference(engine, *b[:3], T, co, pk_inf=b[3])
        return KC.cached(engine, cache, *b[:3], T, co, ref, pk_inf=b[3])[1]

    old, mid = batch(range(30)), batch(range(30, 40), special=("identity", "small_order", "noncanon"))
    new = batch(range(30, 70), special=("identity", "small_order", "noncanon"))
    with new_cache(engine, 64, "affine") as cache:
        expect(run(cache, old), cache, 0, 30, 0, 30)
        expect(run(cache, mid), cache, 0, 13, 0, 43)
        before = _rows(cache, "affine")
        # 13 hits, 30 misses: 43 + 30 > 64, hist = {0: 13, 2: 30}, budget max(13, 17) = 17, K = 13; rows 30..42 all move
        expect(run(cache, new), cache, 13, 30, 1, 43)
        ev = cache.eviction_info()
        assert (ev["last_kept"], ev["last_moved"], ev["dropped"]) == (13, 13, 30), ev
        after = _rows(cache, "affine")
        kept = [k for k in before if before[k][0] >= 30]
        assert len(kept) == 13 and all(k in after and after[k][0] < 13 for k in kept)
        assert not any(k in after for k in before if before[k][0] < 30)
        for k in kept:
            for w0, w1 in zip(before[k][1], after[k][1]):
                assert w0.tobytes() == w1.tobytes(), (before[k][0], after[k][0])
        statuses = sorted(int(after[k][1][1][0]) for k in kept)
        assert statuses == [0] * 11 + [1, 3] and sum(int(after[k][1][3][0]) for k in kept) == 1, statuses
        res = cache.selfcheck(deep=True)
        assert res["ok"] and res["keys_checked"] == cache.info()["held"] == 43, res


def test_rows_arrive_intact_wire(engine, oracle):
    """the same through a wire cache, with the rows' 49 wire bytes (what 5): the identity encoding, the off-subgroup
    fixture (status 1) and two strings that do not decode (status 3) among the survivors, out of spoiled_records"""
    rng = np.random.default_rng(19502)
    keyed, msgs, touched, g, _ = KY.spoiled_records(engine, oracle, rng, n=20000, u=80)
    clean = np.setdiff1d(np.arange(20000), touched)
    keys = np.unique(keyed[clean, :49], axis=0)
    assert keys.shape[0] == 80
    by_key = [clean[(keyed[clean, :49] == k).all(axis=1)] for k in keys]
    special = ("identity", "off_subgroup", "all_ff", "c0")

    def batch(key_numbers, with_special):
        lanes = [ln for k in key_numbers for ln in by_key[k][:N // 48]]
        lanes += [int(ln) for name in (special if with_special else ()) for ln in g[name]]
        lanes = np.array((lanes * (N // len(lanes) + 1))[:N + 300])
        return keyed[lanes], msgs[lanes]

    def run(cache, b):
        co = coeffs32(rng, b[0].shape[0])
        return KY.cached(engine, cache, *b, T, co, KY.reference(engine, *b, T, co), same_keys=False)[1]

    old, mid, new = batch(range(30), False), batch(range(30, 40), True), batch(range(30, 70), True)
    with new_cache(engine, 64, "wire") as cache:
        run(cache, old)
        run(cache, mid)
        assert cache.info()["held"] == 44
        before = _rows(cache, "wire")
        # 14 hits, 30 misses: 44 + 30 > 64, hist = {0: 14, 2: 30}, budget max(14, 17) = 17, K = 14; rows 30..43 all move
        stats = run(cache, new)
        assert (stats[HITS], stats[INSERTED], stats[EVICTIONS]) == (14, 30, 1) and cache.info()["held"] == 44, stats
        ev = cache.eviction_info()
        assert (ev["last_kept"], ev["last_moved"], ev["dropped"]) == (14, 14, 30), ev
        after = _rows(cache, "wire")
        kept = [k for k in before if before[k][0] >= 30]
        assert len(kept) == 14 and all(k in after and after[k][0] < 14 for k in kept)
        for k in kept:
            for w0, w1 in zip(before[k][1], after[k][1]):
                assert w0.tobytes() == w1.tobytes(), (before[k][0], after[k][0])
        statuses = sorted(int(after[k][1][1][0]) for k in kept)
        assert statuses == [0] * 11 + [1, 3, 3] and sum(int(after[k][1][3][0]) for k in kept) == 1, statuses
        res = cache.selfcheck(deep=True)
        assert res["ok"] and res["keys_checked"] == 44, res


_CHILD = r"""
import json, os, sys
sys.path.insert(0, %(root)r)
import numpy as np
import torch
import schnorr_sig_amd as ssa
rng = np.random.default_rng(19701)
e = ssa.Engine(0)
def sc(k):
    v = rng.integers(0, 256, size=(k, 32), dtype=np.uint8); v[:, 31] &= 0x3f; v[:, 0] |= 1
    return v
sks = sc(70)
def signed(pool_of_lane):
    n = pool_of_lane.shape[0]
    m = rng.integers(0, 256, size=(n, 80), dtype=np.uint8)
    pk, sg = e.keygen_sign_many(sks[pool_of_lane], sc(n), m)
    return sg, pk, m
def grouped(lo, hi, n):
    return lo + (np.arange(n) * (hi - lo)) // n
a, b = signed(grouped(0, 30, 5000)), signed(grouped(30, 50, 5000))
# three slices of 5000: B's keys; B's and 20 new keys (the compaction); B's and the new keys again
idx = np.concatenate([grouped(30, 50, 5000), grouped(30, 70, 5000), grouped(30, 70, 5000)])
sg, pk, m = signed(idx)
bad = [0, 4999, 5000, 5001, 7777, 9999, 10000, 14999]
for i in bad:
    sg[i, 50] ^= 4
n = 15000
co = rng.integers(0, 256, size=(n, 32), dtype=np.uint8); co[:, 31] &= 0x3f
want, wnf = e.verify_many(sg, pk, m, check_torsion=True)
out = {"slice": e.info()["lane_slice"], "bad": [int(want[i]) for i in bad], "wnf": int(wnf), "forms": {}}
dev = torch.device("cuda", 0)
for form in ("host", "device"):
    kc = e.keycache_create(64, evict="recent")
    for warm in (a, b):
        st, nf, _ = e.verify_many_cached(kc, *warm, check_torsion=True)
        assert not st.any()
    if form == "host":
        st, nf, stats = e.verify_many_cached(kc, sg, pk, m, coeffs=co, check_torsion=True)
    else:
        ds, dp, dm, dc = (torch.from_numpy(x).to(dev) for x in (sg, pk, m, co))
        dst = torch.full((n,), 255, dtype=torch.uint8, device=dev)
        dnf = torch.zeros(1, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        stats = e.verify_many_cached_device(kc, ds.data_ptr(), dp.data_ptr(), dm.data_ptr(), n, 80, dc.data_ptr(), 32,
                                            dst.data_ptr(), dnf.data_ptr(), check_torsion=True)
        e.sync()
        st, nf = dst.cpu().numpy(), int(dnf.item())
    out["forms"][form] = {"equal": st.tobytes() == want.tobytes(), "nf": int(nf), "stats": [int(v) for v in stats],
                          "held": kc.info()["held"], "clears": kc.info()["clears"], "ev": kc.eviction_info()}
    kc.close()
print("RESULT " + json.dumps(out))
e.close()
"""


def test_a_compaction_in_the_middle_slice_of_three():
    """SSA_LANE_SLICE = 5000 in a fresh child process.  A cache of 64 holds A (30 keys) and B (20); one call of three slices:
    B's keys (20 hits), B's and 20 new keys (the compaction: K = 20, all 20 move), the same 40 keys (40 hits).  Bad lanes on
    both sides of both boundaries.  Both forms against ssa_verify_many."""
    env = dict(os.environ)
    env["SSA_LANE_SLICE"] = "5000"
    r = subprocess.run([sys.executable, "-c", _CHILD % {"root": ROOT}], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    assert out["slice"] == 5000 and out["bad"] == [2] * 8 and out["wnf"] == 8
    for form, c in out["forms"].items():
        assert c["equal"] and c["nf"] == 8, (form, c)
        s = c["stats"]
        assert s[0] == 100 and (s[HITS], s[INSERTED], s[EVICTIONS], s[BYPASSED]) == (80, 20, 1, 0) and s[5] == 3, (form, c)
        assert c["held"] == 40 and c["clears"] == 0, (form, c)
        ev = c["ev"]
        assert (ev["compactions"], ev["dropped"], ev["last_kept"], ev["last_moved"], ev["epoch"]) == (1, 30, 20, 20, 5), ev


def test_poisoned_workspaces_change_nothing():
    """the third call of scenario 1 after ssa_debug_poison_workspaces(ctx, 0xA5) on a fresh context: the vector and the
    statistics of a fresh context that was not poisoned"""
    import schnorr_sig_amd as ssa
    results = []
    for poison in (False, True):
        eng = ssa.Engine(0)
        try:
            results.append(survivors_at_the_top(eng, "affine", "device",
                                                before_third_call=(lambda: eng.debug_poison_workspaces(0xA5)) if poison else None))
        finally:
            eng.close()
    assert results[0][0].tobytes() == results[1][0].tobytes() and results[0][1] == results[1][1], results


def test_the_default_policy_still_clears(engine):
    """the scenario of test_gpu_keycache.py::test_automatic_clear on a cache that was never switched: the same numbers"""
    rng = np.random.default_rng(16401)
    a, b = KC.honest(engine, rng, 6000, 50), KC.honest(engine, rng, 6000, 50)
    a[1][5, 0:8] = 0xFF
    co = coeffs32(rng, 6000)
    ra, rb = KC.reference(engine, *a, T, co), KC.reference(engine, *b, T, co)
    with engine.keycache_create(64) as cache:
        bytes0 = cache.info()["device_bytes"]
        for k, (batch, ref, clears, form) in enumerate(((a, ra, 0, "host"), (b, rb, 1, "device"), (a, ra, 1, "host"))):
            _, stats = KC.cached(engine, cache, *batch, T, co, ref, form=form)
            assert stats[EVICTIONS] == clears and stats[BYPASSED] == 0, (k, stats)
            assert stats[INSERTED] == ref[2][0] and stats[HITS] == 0, (k, stats)
            assert cache.info()["held"] == ref[2][0]
        assert cache.info()["clears"] == 2 and cache.info()["device_bytes"] == bytes0
        assert cache.eviction_info() == {"policy": "clear", "compactions": 0, "dropped": 0, "last_kept": 0, "last_moved": 0,
                                         "epoch": 0}


@pytest.mark.parametrize("mode", MODES)
def test_switching_the_policy_of_a_warm_cache(engine, mode):
    rng = np.random.default_rng(19901)
    sks = make_scalars(rng, 90)
    a, b = Batch(engine, rng, sks[:40], mode, bad=(9,)), Batch(engine, rng, sks[20:60], mode, bad=(4321,))
    c = Batch(engine, rng, sks[50:90], mode)
    with new_cache(engine, 64, mode, evict="clear") as cache:
        bytes0 = cache.info()["device_bytes"]
        expect(a.run(engine, cache)[1], cache, 0, 40, 0, 40)
        cache.set_eviction("recent")                          # the 40 rows held count as used now
        bytes1 = cache.info()["device_bytes"]
        assert bytes1 >= bytes0 + 64 * 16 and cache.eviction_info()["policy"] == "recent"
        expect(a.run(engine, cache, "device")[1], cache, 40, 0, 0, 40)
        # B: 20 hits, 20 misses, 60 held
        expect(b.run(engine, cache)[1], cache, 20, 20, 0, 60)
        cache.set_eviction("clear")
        cache.set_eviction("clear")
        assert cache.info()["device_bytes"] == bytes1 and cache.eviction_info()["policy"] == "clear"
        expect(b.run(engine, cache, "device")[1], cache, 40, 0, 0, 60)
        cache.set_eviction("recent")                          # all 60 rows count as used now, whatever they were before
        assert cache.info()["device_bytes"] == bytes1
        # C: keys 50..59 hit, 30 misses, 60 + 30 > 64: hist = {0: 10, 1: 50}, budget max(10, 17) = 17, K = 10
        expect(c.run(engine, cache)[1], cache, 10, 30, 1, 40)
        assert cache.eviction_info()["last_kept"] == 10
        cache.set_eviction("clear")
        # A: 40 misses, 40 + 40 > 64: the default policy clears
        expect(a.run(engine, cache)[1], cache, 0, 40, 1, 40)
        info = cache.info()
        assert info["clears"] == 1 and info["device_bytes"] == bytes1 and cache.eviction_info()["compactions"] == 1


def test_a_second_compaction_allocates_nothing():
    """the method of test_workspaces_do_not_grow_from_the_second_call_on: after one compacting call, further ones leave the
    context's workspaces and the cache's footprint as they are"""
    import schnorr_sig_amd as ssa
    eng = ssa.Engine(0)
    try:
        rng = np.random.default_rng(19951)
        v = make_scalars(rng, 30)
        with eng.keycache_create(64, evict="recent") as cache:
            bytes0 = cache.info()["device_bytes"]
            sizes = []
            for call in range(5):
                pool = np.concatenate([v, make_scalars(rng, 30)])
                batch = Batch(eng, rng, pool, "affine", bad=(call,))
                for form in ("host", "device"):
                    batch.run(eng, cache, form)
                sizes.append(eng.info()["workspace_bytes"])
                assert cache.info()["device_bytes"] == bytes0
            assert cache.eviction_info()["compactions"] == 4
            assert sizes[0] > 0 and sizes[4] == sizes[1], sizes
    finally:
        eng.close()
