#!/usr/bin/env python3
"""ssa_verify_many_screened with SSA_FLAG_CHECK_TORSION against ssa_verify_many_dedup and ssa_verify_many with the same
flag.  One engine on cuda:0, device-resident batches of --n signatures with 80-byte messages by u
distinct signers (u = 1, 1000, n/16, n/4, n/2, n), each with 0, 16 and n/1024 bad lanes (a wrong e; n/1024 puts one in
every segment), library-drawn coefficients.

Legs, timed in one process and ALTERNATING round by round (each call closed by a synchronise; wall time per call):
  many_u<U>_b<B>       ssa_verify_many_device              (--legs base)
  dedup_u<U>_b<B>      ssa_verify_many_dedup_device        (--legs base)
  new_u<U>_b<B>        ssa_verify_many_screened_device     (--legs new)
  screened_flag        ssa_verify_batch_screened_device on the honest all-distinct batch (--legs new): the screen alone
--legs base uses nothing the parent commit lacks, so the same file run from a checkout of the parent measures the two
baselines on the parent's library in the same session.  After every timed call of the many, dedup and new legs its
status vector and count are checked against ssa_verify_many's on the same input; screened_flag is timed only, its output
is compared with nothing.  Per-stage times of one extra call per leg come from ssa_ctx_read_timing.  One JSON line out."""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STAGES = ("dedup", "dedup_gather", "ssa_k_keyset_build", "screen_keymask", "ssa_k_hash", "msm_k_prepare", "msm_sort",
          "msm_k_buckets", "msm_reduce", "msm_k_finish_seg", "screen_mark", "screen_list_gather", "ssa_k_verify_keyed",
          "screen_list_scatter", "ssa_k_verify")
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
    ap.add_argument("--legs", type=str, default="base,new")
    ap.add_argument("--us", type=str, default="1,1000,n/16,n/4,n/2,n")
    ap.add_argument("--bad", type=str, default="0,16,n/1024")
    ap.add_argument("--seed", type=int, default=0x5C7E)
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
    inputs, ref = {}, {}
    d_st = torch.empty(n, dtype=torch.uint8, device=dev)
    d_nf = torch.zeros(1, dtype=torch.int64, device=dev)

    def many(key, out=None, nf=None):
        s, p, m = inputs[key]
        eng.verify_many_device(s.data_ptr(), p.data_ptr(), m.data_ptr(), n, 80, (out if out is not None else d_st).data_ptr(),
                               (nf if nf is not None else d_nf).data_ptr(), **TORSION)

    def dedup(key):
        s, p, m = inputs[key]
        return eng.verify_many_dedup_device(s.data_ptr(), p.data_ptr(), m.data_ptr(), n, 80, d_st.data_ptr(), d_nf.data_ptr(),
                                            **TORSION)

    def new(key):
        s, p, m = inputs[key]
        return eng.verify_many_screened_device(s.data_ptr(), p.data_ptr(), m.data_ptr(), n, 80, 0, 0, d_st.data_ptr(),
                                               d_nf.data_ptr(), **TORSION)

    def screened_flag(key):
        s, p, m = inputs[key]
        eng.verify_batch_screened_device(s.data_ptr(), p.data_ptr(), m.data_ptr(), n, 80, 0, 0, d_st.data_ptr(),
                                         d_nf.data_ptr())

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
                lanes = np.arange(17, n, n // b)[:b] if bs.startswith("n/") else rng.choice(n, b, replace=False)
                s2[lanes, 49] ^= 1
            key = "u%s_b%s" % (us, bs)
            inputs[key] = (t(s2), d_p, d_m)
            out = torch.empty(n, dtype=torch.uint8, device=dev)     # what ssa_verify_many says (not timed)
            nf = torch.zeros(1, dtype=torch.int64, device=dev)
            many(key, out, nf)
            eng.sync()
            ref[key] = (out, int(nf.item()))

    def wall(fn):
        eng.sync()
        t0 = time.perf_counter()
        fn()
        eng.sync()
        return (time.perf_counter() - t0) * 1e3

    legs = []
    for key in inputs:
        if "base" in want_legs:
            legs += [("many", key), ("dedup", key)]
        if "new" in want_legs:
            legs.append(("new", key))
    honest_all = "u%s_b%s" % (a.us.split(",")[-1], a.bad.split(",")[0])
    if "new" in want_legs:
        legs.append(("screened_flag", honest_all))
    run = {"many": many, "dedup": dedup, "new": new, "screened_flag": screened_flag}
    name = lambda leg: leg[0] if leg[0] == "screened_flag" else "%s_%s" % leg   # noqa: E731
    times = {name(leg): [] for leg in legs}
    stats = {}
    res = {"metric": "verify_many_screened", "n": n, "msg_len": 80, "rounds": a.rounds, "warmup": a.warmup, "legs": a.legs,
           "library_sha256": hashlib.sha256(open(ssa.LIB_PATH, "rb").read()).hexdigest()[:16],
           "device": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d"), "mismatches": 0}
    for rnd in range(a.warmup + a.rounds):
        for leg in legs:
            got = []
            ms = wall(lambda: got.append(run[leg[0]](leg[1])))
            if leg[0] != "screened_flag":
                want, wnf = ref[leg[1]]
                if not bool((d_st == want).all()) or int(d_nf.item()) != wnf:
                    res["mismatches"] += 1
            if got[0] is not None:
                stats[name(leg)] = [int(v) for v in got[0]]
            if rnd >= a.warmup:
                times[name(leg)].append(ms)
    res["ms_median"] = {k: round(float(np.median(v)), 3) for k, v in times.items()}
    res["ms_min"] = {k: round(float(np.min(v)), 3) for k, v in times.items()}
    res["ms_max"] = {k: round(float(np.max(v)), 3) for k, v in times.items()}
    res["stats"] = stats
    stage = {}
    for leg in legs:             # per-stage times of one extra call per leg: [sum of the launches' ms, launches]
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
    print(json.dumps(res))
    eng.close()
    return 0 if res["mismatches"] == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
