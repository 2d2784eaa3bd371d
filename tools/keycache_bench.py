#!/usr/bin/env python3
"""ssa_verify_many_cached against ssa_verify_many_screened, both with SSA_FLAG_CHECK_TORSION.
One engine on cuda:0, device-resident batches of --n signatures with 80-byte messages by u distinct signers (u = 1,
1000, n/16, n/4, n/2, n), each with 0 and 16 bad lanes (a wrong e), library-drawn coefficients, one key cache of
--capacity rows.

Legs, timed in one process and ALTERNATING round by round (each call closed by a synchronise; wall time per call):
  screened_u<U>_b<B>   ssa_verify_many_screened_device                                          (--legs parent)
  cold_u<U>_b<B>       ssa_verify_many_cached_device on a cache cleared just before (not timed)  (--legs new)
  warm_u<U>_b<B>       the same call again: every key is in the cache                            (--legs new)
  plus1_u<U>_b0        the warm call with ONE key the cache has not seen (lane 0 re-signed by a fresh signer before
                       every call, not timed): the latency floor of one lane's key check        (--legs new)
--legs parent uses nothing the parent commit lacks: the same file run from a checkout of the parent measures the
baseline on the parent's library in the same session.  That run, never one on the tree under test, is the baseline of
the bars in DESIGN.md section 16.  After every timed call its status vector and count are checked against
ssa_verify_many's on the same input.  Per-stage times of one extra call per leg come from ssa_ctx_read_timing.  One JSON
line out."""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STAGES = ("dedup", "keycache_lookup", "dedup_gather", "keycache_insert", "ssa_k_keyset_build", "keycache_map",
          "screen_keymask", "ssa_k_hash", "msm_k_prepare", "msm_sort", "msm_k_buckets", "msm_reduce", "msm_k_finish_seg",
          "screen_mark", "screen_list_gather", "ssa_k_verify_keyed", "screen_list_scatter", "ssa_k_verify")
TORSION = dict(check_torsion=True, sig_flag_byte=False)


def _scalars(rng, n):
    v = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    v[:, 31] &= 0x3F
    v[:, 0] |= 1
    return v


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--legs", type=str, default="parent,new")
    ap.add_argument("--us", type=str, default="1,1000,n/16,n/4,n/2,n")
    ap.add_argument("--bad", type=str, default="0,16")
    ap.add_argument("--capacity", type=int, default=1 << 20)
    ap.add_argument("--seed", type=int, default=0x6CAC)
    a = ap.parse_args()
    import torch
    import schnorr_sig_amd as ssa
    dev = torch.device("cuda", 0)
    eng = ssa.Engine(0)
    rng = np.random.default_rng(a.seed)
    n = a.n
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)   # noqa: E731
    size = lambda s: n // int(s[2:]) if s.startswith("n/") else (n if s == "n" else min(int(s), n))   # noqa: E731
    want_legs = [x for x in a.legs.split(",") if x]
    with_new = "new" in want_legs
    cache = eng.keycache_create(a.capacity) if with_new else None
    calls = a.warmup + a.rounds + 1
    inputs, ref, fresh = {}, {}, {}
    d_st = torch.empty(n, dtype=torch.uint8, device=dev)
    d_nf = torch.zeros(1, dtype=torch.int64, device=dev)

    for us in a.us.split(","):
        u = size(us)
        idx = rng.integers(0, u, size=n)
        idx[:u] = np.arange(u)
        rng.shuffle(idx)
        msgs = rng.integers(0, 256, (n, 80), dtype=np.uint8)
        pks, sigs = eng.keygen_sign_many(_scalars(rng, u)[idx], _scalars(rng, n), msgs)
        d_p, d_m = t(pks), t(msgs)
        for bs in a.bad.split(","):
            b = size(bs)
            s2 = sigs.copy()
            if b:
                s2[rng.choice(np.arange(1, n), b, replace=False), 49] ^= 1
            key = "u%s_b%s" % (us, bs)
            inputs[key] = (t(s2), d_p, d_m)
            out = torch.empty(n, dtype=torch.uint8, device=dev)     # what ssa_verify_many says (not timed)
            nf = torch.zeros(1, dtype=torch.int64, device=dev)
            eng.verify_many_device(inputs[key][0].data_ptr(), d_p.data_ptr(), d_m.data_ptr(), n, 80, out.data_ptr(),
                                   nf.data_ptr(), **TORSION)
            eng.sync()
            ref[key] = (out, int(nf.item()))
            if with_new and b == 0:
                # lane 0 by a fresh signer per call (honest: the reference vector stays all zero), in buffers of its own
                fp, fs = eng.keygen_sign_many(_scalars(rng, calls), _scalars(rng, calls), np.repeat(msgs[:1], calls, axis=0))
                fresh[key] = (t(s2), t(pks), t(fs), t(fp), [0])

    def screened(key):
        s, p, m = inputs[key]
        return eng.verify_many_screened_device(s.data_ptr(), p.data_ptr(), m.data_ptr(), n, 80, 0, 0, d_st.data_ptr(),
                                               d_nf.data_ptr(), **TORSION)

    def cached(key):
        s, p, m = inputs[key]
        return eng.verify_many_cached_device(cache, s.data_ptr(), p.data_ptr(), m.data_ptr(), n, 80, 0, 0, d_st.data_ptr(),
                                             d_nf.data_ptr(), **TORSION)

    def plus1(key):
        s, p, _, _, _ = fresh[key]
        return eng.verify_many_cached_device(cache, s.data_ptr(), p.data_ptr(), inputs[key][2].data_ptr(), n, 80, 0, 0,
                                             d_st.data_ptr(), d_nf.data_ptr(), **TORSION)

    def prepare(leg):            # not timed
        if leg[0] == "cold":
            cache.clear()
        elif leg[0] == "plus1":
            s, p, fs, fp, k = fresh[leg[1]]
            s[0].copy_(fs[k[0]])
            p[0].copy_(fp[k[0]])
            k[0] += 1
            torch.cuda.synchronize()

    def wall(fn):
        eng.sync()
        t0 = time.perf_counter()
        fn()
        eng.sync()
        return (time.perf_counter() - t0) * 1e3

    legs = []
    for key in inputs:
        if "parent" in want_legs:
            legs.append(("screened", key))
        if with_new:
            legs += [("cold", key), ("warm", key)]       # in this order: the cold call is what warms the cache
            if key in fresh:
                legs.append(("plus1", key))
    run = {"screened": screened, "cold": cached, "warm": cached, "plus1": plus1}
    name = lambda leg: "%s_%s" % leg   # noqa: E731
    times = {name(leg): [] for leg in legs}
    stats = {}
    res = {"metric": "verify_many_cached", "n": n, "msg_len": 80, "rounds": a.rounds, "warmup": a.warmup, "legs": a.legs,
           "capacity": a.capacity if with_new else 0,
           "library_sha256": hashlib.sha256(open(ssa.LIB_PATH, "rb").read()).hexdigest()[:16],
           "device": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d"), "mismatches": 0}
    for rnd in range(a.warmup + a.rounds):
        for leg in legs:
            prepare(leg)
            got = []
            ms = wall(lambda: got.append(run[leg[0]](leg[1])))
            want, wnf = ref[leg[1]]
            if not bool((d_st == want).all()) or int(d_nf.item()) != wnf:
                res["mismatches"] += 1
            stats[name(leg)] = [int(v) for v in got[0]]
            if rnd >= a.warmup:
                times[name(leg)].append(ms)
    res["ms_median"] = {k: round(float(np.median(v)), 3) for k, v in times.items()}
    res["ms_min"] = {k: round(float(np.min(v)), 3) for k, v in times.items()}
    res["ms_max"] = {k: round(float(np.max(v)), 3) for k, v in times.items()}
    res["stats"] = stats
    stage = {}
    for leg in legs:             # per-stage times of one extra call per leg: [sum of the launches' ms, launches]
        prepare(leg)
        eng.sync()
        eng.enable_timing(True)
        run[leg[0]](leg[1])
        eng.sync()
        stage[name(leg)] = {}
        for k in STAGES:
            avg, cnt = eng.read_timing(k)
            if cnt:
                stage[name(leg)][k] = [round(avg * cnt, 4), int(cnt)]
        eng.enable_timing(False)
    res["stage_ms_total_launches"] = stage
    if cache is not None:
        res["cache_info"] = cache.info()
        cache.close()
    print(json.dumps(res))
    eng.close()
    return 0 if res["mismatches"] == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
