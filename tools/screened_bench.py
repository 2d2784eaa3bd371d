#!/usr/bin/env python3
"""Screened batch verification against the two outputs it sits between.  One engine on cuda:0,
device-resident batches of --n signatures with 80-byte messages, library-drawn coefficients.

Legs, timed in one process and ALTERNATING round by round (each call closed by a synchronise; wall time per call):
  screened_0 / _1 / _16 / _1in1024   ssa_verify_batch_screened_device with 0, 1, 16 and one-in-1024 bad lanes
  verify_many_flag                   ssa_verify_many_device with SSA_FLAG_SIG_FLAG_BYTE (the per-lane status vector)
  verify_batch_msm                   ssa_verify_batch_msm_device (one verdict)
After every timed screened call its status vector and count are compared with the per-lane vector of the same input.
--segments K,K,..: the screened legs again under each forced K (ssa_debug_screen_segments; 0 = automatic).
Per-kernel times of one extra screened call per input come from ssa_ctx_read_timing.  One JSON line out."""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
KERNELS = ("ssa_k_hash", "msm_k_prepare", "msm_sort", "msm_k_buckets", "msm_reduce", "msm_k_finish_seg", "screen_gather",
           "ssa_k_verify", "screen_scatter")


def _scalars(rng, n):
    v = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    v[:, 31] &= 0x3F
    v[:, 0] |= 1
    return v


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--segments", type=str, default="0")
    ap.add_argument("--seed", type=int, default=0x5C3E)
    a = ap.parse_args()
    import torch
    import schnorr_sig_amd as ssa
    dev = torch.device("cuda", 0)
    eng = ssa.Engine(0)
    rng = np.random.default_rng(a.seed)
    n = a.n
    msgs = rng.integers(0, 256, (n, 80), dtype=np.uint8)
    pks, sigs = eng.keygen_sign_many(_scalars(rng, n), _scalars(rng, n), msgs)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)   # noqa: E731
    d_pks, d_msgs = t(pks), t(msgs)
    inputs = {}
    for name, bad in (("0", []), ("1", [int(rng.integers(0, n))]), ("16", sorted(rng.choice(n, 16, replace=False))),
                      ("1in1024", list(range(int(rng.integers(0, 1024)), n, 1024)))):
        s = sigs.copy()
        for i in bad:
            s[i, 50] ^= 4
        inputs[name] = (t(s), len(bad))
    d_st = torch.empty(n, dtype=torch.uint8, device=dev)
    d_ref = torch.empty(n, dtype=torch.uint8, device=dev)
    d_nf = torch.zeros(1, dtype=torch.int64, device=dev)
    d_nf2 = torch.zeros(1, dtype=torch.int64, device=dev)
    d_verdict = torch.zeros(1, dtype=torch.int32, device=dev)

    def screened(name):
        eng.verify_batch_screened_device(inputs[name][0].data_ptr(), d_pks.data_ptr(), d_msgs.data_ptr(), n, 80, 0, 0,
                                         d_st.data_ptr(), d_nf.data_ptr())

    def per_lane(name, out, nf):
        eng.verify_many_device(inputs[name][0].data_ptr(), d_pks.data_ptr(), d_msgs.data_ptr(), n, 80, out.data_ptr(),
                               nf.data_ptr(), sig_flag_byte=True)

    def msm():
        eng.verify_batch_msm_device(inputs["0"][0].data_ptr(), d_pks.data_ptr(), d_msgs.data_ptr(), n, 80, None, 0,
                                    d_verdict.data_ptr())

    def wall(fn):
        eng.sync()
        t0 = time.perf_counter()
        fn()
        eng.sync()
        return (time.perf_counter() - t0) * 1e3

    res = {"metric": "screened_batch_verification", "n": n, "msg_len": 80, "rounds": a.rounds, "warmup": a.warmup,
           "library_sha256": hashlib.sha256(open(ssa.LIB_PATH, "rb").read()).hexdigest()[:16],
           "device": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d"),
           "plan": ssa.debug_screen_plan(n), "mismatches": 0}
    ks = [int(k) for k in a.segments.split(",")]
    legs = ["verify_many_flag", "verify_batch_msm"] + ["screened_%s_K%d" % (nm, k) for k in ks for nm in inputs]
    times = {leg: [] for leg in legs}
    for rnd in range(a.warmup + a.rounds):
        for leg in legs:
            if leg == "verify_many_flag":
                ms = wall(lambda: per_lane("0", d_ref, d_nf2))
            elif leg == "verify_batch_msm":
                ms = wall(msm)
            else:
                _, nm, kk = leg.split("_")
                eng.debug_screen_segments(int(kk[1:]))
                ms = wall(lambda: screened(nm))
                per_lane(nm, d_ref, d_nf2)          # every timed screened vector against the per-lane one
                eng.sync()
                if not bool((d_st == d_ref).all()) or int(d_nf.item()) != int(d_nf2.item()):
                    res["mismatches"] += 1
            if rnd >= a.warmup:
                times[leg].append(ms)
    eng.debug_screen_segments(0)
    res["ms_median"] = {leg: round(float(np.median(v)), 3) for leg, v in times.items()}
    res["ms_min"] = {leg: round(float(np.min(v)), 3) for leg, v in times.items()}
    base = res["ms_median"]["verify_many_flag"]
    res["ratio_to_verify_many_flag"] = {leg: round(v / base, 3) for leg, v in res["ms_median"].items()}
    # per-kernel times of one screened call per input (automatic K)
    kern = {}
    for nm in inputs:
        eng.sync()
        eng.enable_timing(True)
        screened(nm)
        eng.sync()
        kern[nm] = {}
        for k in KERNELS:
            avg, cnt = eng.read_timing(k)
            if cnt:
                kern[nm][k] = [round(avg, 4), int(cnt)]
        eng.enable_timing(False)
    res["kernel_ms_avg_launches"] = kern
    print(json.dumps(res))
    eng.close()
    return 0 if res["mismatches"] == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
