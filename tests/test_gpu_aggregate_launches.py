"""The enqueue sequence of the half-aggregation family (DESIGN.md sections 20 to 29): which launches every call makes,
under which timing key, what statistics it returns and what the streaming objects and the key cache count.  The other
aggregate tests compare bytes and verdicts; this one pins what a rearrangement of the host code around the kernels could
move without changing a byte.

A fixed, seeded script of calls runs with enable_timing(True); after every step the launch count of every timing key of
the family (read_timing(key)[1]), every statistics array the step returned and the info() of the objects alive are
recorded, and the whole record equals tests/golden/aggregate_launches.json.  The fixture is made by running this file
as a script against the tree of the commit BEFORE the change under test, never against the tree under test:

    python tests/test_gpu_aggregate_launches.py --record tests/golden/aggregate_launches.json

Public Python API only.  The second half runs in a child process under the suite's sliced setting (callscript.SLICE for
SSA_LANE_SLICE and SSA_MSM_SLICE, callscript.SLICED_N = 12345 lanes).  With both knobs at 5000 a push and a filtering
aggregate take one MSM slice at most (agg_check_args refuses more), so there:
  - verify_aggregates_cached takes three aggregates of 4115 lanes: 12345 lanes, THREE slices of the key cache in one
    call (5000, 5000, 2345; agc_expand is launched three times);
  - the verifier's and the aggregator's finish walk 12345 held lanes in pieces of 4096 (the largest power of two
    within the MSM slice): four pieces;
  - the 12345 lanes are pushed in three pushes of one cache slice each, and aggregate_valid_cached takes 5000 lanes, one
    slice: one call of three slices is not reachable for these two under this setting."""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "aggregate_launches.json")
SLICE, SLICED_N = 5000, 12345           # callscript.SLICE, callscript.SLICED_N (asserted equal in the test)
RNG_PIN = bytes(range(100, 144))        # callscript.RNG_PIN
KEYS = ("ag_k_expand", "ag_k_expand_many", "ag_k_lane_map", "ssa_k_hash", "ag_k_leaf", "ag_k_tree", "ag_k_level", "ag_k_coeff",
        "ag_k_fold", "ag_k_fold_finish", "ag_k_finish", "ag_k_pack", "ag_k_gather", "ag_k_fold_seg", "ag_k_fold_finish_seg",
        "ag_k_pack_many", "agx_k_check", "agx_k_append", "agx_k_coeff_fold", "agv_k_append", "agv_k_scalars",
        "agv_k_key_verdict", "agc_expand", "agc_k_key_verdicts", "av_k_keep", "av_k_gather", "av_k_gather_keys")


def _ssa():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import schnorr_sig_amd as ssa
    return ssa


class Lanes:
    """n honest lanes from 64 signers, made once per process: signatures, affine and 49-byte keys, 80-byte messages,
    130-byte keyed records"""

    def __init__(self, eng, n, seed):
        rng = np.random.default_rng(seed)
        sk64 = rng.integers(0, 256, size=(64, 32), dtype=np.uint8)
        sk64[:, 31] &= 0x3F
        sks = sk64[rng.integers(0, 64, size=n)]
        nonces = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
        nonces[:, 31] &= 0x3F
        self.msgs = rng.integers(0, 256, size=(n, 80), dtype=np.uint8)
        self.pks, self.sigs = eng.keygen_sign_many(sks, nonces, self.msgs)
        _, self.keyed = eng.keygen_sign_many(sks, nonces, self.msgs, keyed=True)
        self.wire, st = eng.compress_many(self.pks)
        assert not st.any()

    def bad(self, n, lanes):
        """the signatures of the first n lanes with the scalar of the listed ones spoiled"""
        s = self.sigs[:n].copy()
        for i in lanes:
            s[i, 60] ^= 1
        return s


def _stats(res):
    """every statistics array (uint64[8] or uint64[12]) in what a step returned"""
    out = []
    if isinstance(res, np.ndarray):
        if res.dtype == np.uint64 and res.ndim == 1 and res.size in (8, 12):
            out.append([int(v) for v in res])
    elif isinstance(res, (tuple, list)):
        for r in res:
            out.extend(_stats(r))
    return out


class Recorder:
    def __init__(self, eng):
        self.eng, self.objs, self.steps = eng, {}, []

    def step(self, name, res):
        self.steps.append({"step": name, "launches": {k: self.eng.read_timing(k)[1] for k in KEYS}, "stats": _stats(res),
                           "info": {k: o.info() for k, o in sorted(self.objs.items())}})
        return res


def script_default(ssa):
    """the steps on a default engine"""
    eng = ssa.Engine(0)
    eng.debug_pin_rng(RNG_PIN)
    eng.enable_timing(True)
    L = Lanes(eng, 1300, 0xA661)
    rec = Recorder(eng)
    for n in (0, 1, 600):
        for check in (False, True):
            for name in ("aggregate", "aggregate_sliced"):
                sigs = L.bad(n, [n // 2] if check and n else [])
                res = rec.step("%s n=%d check=%d" % (name, n, check), getattr(eng, name)(sigs, L.pks[:n], L.msgs[:n], check=check))
                rec.step("verify_%s n=%d check=%d" % (name, n, check),
                         getattr(eng, "verify_" + name)(res[1], L.pks[:n], L.msgs[:n]))
    rec.step("aggregate_valid", eng.aggregate_valid(L.bad(600, [0, 299, 599]), L.pks[:600], L.msgs[:600]))
    rec.objs["cache"] = cache = eng.keycache_create(256)
    for heat in ("cold", "warm"):
        rec.step("aggregate_valid_cached " + heat, eng.aggregate_valid_cached(cache, L.bad(600, [7]), L.pks[:600], L.msgs[:600]))
    rec.objs["wcache"] = wcache = eng.keycache_create(256, wire=True)
    rec.step("aggregate_valid_keyed_cached", eng.aggregate_valid_keyed_cached(wcache, L.keyed[:600], L.msgs[:600]))
    counts = np.array([0, 5, 600], dtype=np.uint64)
    aggs, _, _, _ = rec.step("aggregates", eng.aggregates((L.sigs[:605], L.pks[:605], L.msgs[:605]), counts=counts))
    rec.step("aggregates check", eng.aggregates((L.bad(605, [3]), L.pks[:605], L.msgs[:605]), check=True, counts=counts))
    rec.step("verify_aggregates", eng.verify_aggregates(aggs, L.pks[:605], L.msgs[:605]))
    rec.step("verify_aggregates_cached affine", eng.verify_aggregates_cached(cache, aggs, L.pks[:605], L.msgs[:605]))
    rec.step("verify_aggregates_cached wire", eng.verify_aggregates_cached(wcache, aggs, L.wire[:605], L.msgs[:605]))
    for B in (4, 512):
        rec.objs["ag%d" % B] = ag = eng.aggregator(1300, B)
        lo = 0
        for n, screen in ((3, True), (5, False), (600, True), (0, True), (600, False)):
            rec.step("aggregator B=%d push %d screen=%d" % (B, n, screen),
                     ag.push(L.bad(lo + n, [lo] if n == 600 else [])[lo:], L.pks[lo:lo + n], L.msgs[lo:lo + n], screen=screen))
            lo += n
        for take in (None, 6, 0):
            rec.step("aggregator B=%d finish %s" % (B, take), ag.finish_bytes(take))
        del rec.objs["ag%d" % B]
        ag.close()
    e = np.zeros(32, dtype=np.uint8)
    for B in (4, 512):
        rec.objs["av%d" % B] = av = eng.aggregate_verifier(1300, B)
        rs = L.sigs[:, :49]
        rec.step("verifier B=%d plain push" % B, av.push(rs[:3], L.pks[:3], L.msgs[:3]))
        rec.step("verifier B=%d finish unkeyed" % B, av.finish(e))
        rec.step("verifier B=%d finish unkeyed prefix" % B, av.finish(e, 2))
        rec.step("verifier B=%d cached push" % B, av.push(rs[3:603], L.pks[3:603], L.msgs[3:603], cache=cache))
        rec.step("verifier B=%d empty cached push" % B, av.push(rs[:0], L.pks[:0], L.msgs[:0], cache=cache))
        rec.step("verifier B=%d plain push again" % B, av.push(rs[603:608], L.pks[603:608], L.msgs[603:608]))
        rec.step("verifier B=%d empty push" % B, av.push(rs[:0], L.pks[:0], L.msgs[:0]))
        rec.step("verifier B=%d finish keyed" % B, av.finish(e))
        rec.step("verifier B=%d finish keyed prefix" % B, av.finish(e, 6))
        rec.step("verifier B=%d finish none" % B, av.finish(e, 0))
        rec.objs["aw%d" % B] = aw = eng.aggregate_verifier(700, B)
        rec.step("verifier B=%d push_wire" % B, aw.push_wire(rs[:600], L.wire[:600], L.msgs[:600], cache=wcache))
        rec.step("verifier B=%d finish wire" % B, aw.finish(e))
        rec.step("verifier B=%d finish wire prefix" % B, aw.finish(e, 513))
        for k in ("av%d" % B, "aw%d" % B):
            rec.objs.pop(k).close()
    return rec.steps


def script_sliced(ssa):
    """the steps of the child process: SSA_LANE_SLICE = SSA_MSM_SLICE = SLICE, SLICED_N lanes (the module's docstring says
    which steps are three slices or pieces and which can only be one)"""
    eng = ssa.Engine(0)
    assert eng.info()["lane_slice"] == SLICE and eng.info()["msm_slice"] == SLICE
    eng.debug_pin_rng(RNG_PIN)
    eng.enable_timing(True)
    n = SLICED_N
    L = Lanes(eng, n, 0xA662)
    rec = Recorder(eng)
    rec.objs["cache"] = cache = eng.keycache_create(256)
    rec.objs["av"] = av = eng.aggregate_verifier(n)
    e = np.zeros(32, dtype=np.uint8)
    # (a push takes one MSM slice at most: three pushes through the cache, each ONE slice of the key cache)
    for lo in range(0, n, SLICE):
        hi = min(lo + SLICE, n)
        rec.step("cached verifier push [%d, %d)" % (lo, hi),
                 av.push(L.sigs[lo:hi, :49], L.pks[lo:hi], L.msgs[lo:hi], cache=cache))
    rec.step("cached verifier finish", av.finish(e))
    # three aggregates of n / 3 lanes, none over one MSM slice: the n lanes go through the cache in three slices
    third, aggs = n // 3, []
    assert 3 * third == n and third <= SLICE
    for lo in range(0, n, third):
        st, agg, _, _ = eng.aggregate(L.sigs[lo:lo + third], L.pks[lo:lo + third], L.msgs[lo:lo + third])
        assert st == 0
        aggs.append(agg)
    for k in KEYS:
        eng.read_timing(k)      # (the launches of making the aggregates are not the step's)
    verdicts, stats = rec.step("verify_aggregates_cached 3 x %d" % third, eng.verify_aggregates_cached(cache, aggs, L.pks, L.msgs))
    assert not verdicts.any()
    assert rec.steps[-1]["launches"]["agc_expand"] == 3
    # (one slice: a filtering aggregate takes one MSM slice at most)
    rec.step("aggregate_valid_cached", eng.aggregate_valid_cached(cache, L.bad(SLICE, [1, 2]), L.pks[:SLICE], L.msgs[:SLICE]))
    rec.objs["ag"] = ag = eng.aggregator(n)
    for lo in range(0, n, SLICE):
        hi = min(lo + SLICE, n)
        rec.step("aggregator push [%d, %d)" % (lo, hi), ag.push(L.sigs[lo:hi], L.pks[lo:hi], L.msgs[lo:hi], screen=False))
    rec.step("aggregator finish", ag.finish_bytes())
    return rec.steps


def record():
    """{'default': steps, 'sliced': steps}: the first script here, the second in a child process under the sliced setting"""
    env = dict(os.environ, SSA_LANE_SLICE=str(SLICE), SSA_MSM_SLICE=str(SLICE))
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--sliced-child"], env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return {"default": script_default(_ssa()), "sliced": json.loads(r.stdout.strip().splitlines()[-1])}


try:
    import pytest
except ImportError:       # (run as a script on a box without pytest)
    pytest = None

if pytest is not None:
    @pytest.mark.gpu
    def test_the_enqueue_sequence_of_the_aggregate_family_did_not_move():
        import callscript
        assert (callscript.SLICE, callscript.SLICED_N, callscript.RNG_PIN) == (SLICE, SLICED_N, RNG_PIN)
        with open(FIXTURE) as fh:
            want = json.load(fh)
        got = json.loads(json.dumps(record()))
        for part in ("default", "sliced"):
            assert [s["step"] for s in got[part]] == [s["step"] for s in want[part]]
            for g, w in zip(got[part], want[part]):
                assert g == w, "%s: %s" % (part, g["step"])


if __name__ == "__main__":
    if sys.argv[1:2] == ["--sliced-child"]:
        print(json.dumps(script_sliced(_ssa())))
    elif sys.argv[1:2] == ["--record"]:
        with open(sys.argv[2], "w") as fh:
            json.dump(record(), fh, indent=0, sort_keys=True)
            fh.write("\n")
        print("recorded", sys.argv[2])
    else:
        sys.exit("usage: test_gpu_aggregate_launches.py --record FILE")
