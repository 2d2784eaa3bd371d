#!/usr/bin/env python3
"""Half-aggregation against the calls it sits beside.  One engine on cuda:0, device-resident
batches of --n signatures with 80-byte messages.

Legs, timed in one process and ALTERNATING round by round (each call closed by a synchronise; wall time per call):
  verify_aggregate     ssa_verify_aggregate_device on the honest aggregate
  verify_batch_msm     ssa_verify_batch_msm_device on the original signatures, library-drawn coefficients
  aggregate            ssa_aggregate_many_device
  aggregate_checked    ssa_aggregate_many_device with SSA_AGG_CHECK
  hash_message         ssa_hash_message_many_device
Every timed verify_aggregate verdict must be SSA_OK, and every timed aggregate must equal the first one byte for byte.
Per-kernel times of one extra verify_aggregate and one extra aggregate come from ssa_ctx_read_timing; the transcript
kernels' time per Rescue permutation is set beside ssa_k_hash's of the same run (an 80-byte message: four permutations per
lane; leaf, node and coefficient: about one each).  One JSON line out."""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
KERNELS = ("ssa_k_hash", "ag_k_leaf", "ag_k_tree", "ag_k_coeff", "ag_k_fold", "msm_k_prepare", "msm_sort", "msm_k_buckets",
           "msm_reduce", "ag_k_finish")


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
    ap.add_argument("--seed", type=int, default=0xA66)
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
    d_sigs, d_pks, d_msgs = t(sigs), t(pks), t(msgs)
    d_agg = torch.zeros(49 * n + 32, dtype=torch.uint8, device=dev)
    d_agg0 = torch.zeros(49 * n + 32, dtype=torch.uint8, device=dev)
    d_dig = torch.zeros(32 * n, dtype=torch.uint8, device=dev)
    d_verdict = torch.full((1,), 255, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()

    def aggregate(out, check=False):
        return eng.aggregate_device(d_sigs.data_ptr(), d_pks.data_ptr(), d_msgs.data_ptr(), n, 80, out.data_ptr(), check=check)

    def verify_agg():
        eng.verify_aggregate_device(d_agg0.data_ptr(), d_pks.data_ptr(), d_msgs.data_ptr(), n, 80, d_verdict.data_ptr())

    def msm():
        eng.verify_batch_msm_device(d_sigs.data_ptr(), d_pks.data_ptr(), d_msgs.data_ptr(), n, 80, None, 0,
                                    d_verdict.data_ptr())

    def hash_message():
        eng.hash_message_many_device(d_sigs.data_ptr(), d_pks.data_ptr(), d_msgs.data_ptr(), n, 80, d_dig.data_ptr())

    def wall(fn):
        eng.sync()
        t0 = time.perf_counter()
        fn()
        eng.sync()
        return (time.perf_counter() - t0) * 1e3

    res = {"metric": "half_aggregation", "n": n, "msg_len": 80, "rounds": a.rounds, "warmup": a.warmup,
           "library_sha256": hashlib.sha256(open(ssa.LIB_PATH, "rb").read()).hexdigest()[:16],
           "device": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d"), "mismatches": 0,
           "bytes": {"signatures": 81 * n, "aggregate": 49 * n + 32}}
    if aggregate(d_agg0) != 0:
        res["mismatches"] += 1
    eng.sync()
    legs = {"verify_aggregate": verify_agg, "verify_batch_msm": msm, "aggregate": lambda: aggregate(d_agg),
            "aggregate_checked": lambda: aggregate(d_agg, True), "hash_message": hash_message}
    times = {leg: [] for leg in legs}
    for rnd in range(a.warmup + a.rounds):
        for leg, fn in legs.items():
            d_verdict.fill_(255)
            ms = wall(fn)
            if leg == "verify_aggregate" and int(d_verdict.item()) != 0:
                res["mismatches"] += 1
            if leg.startswith("aggregate") and not bool((d_agg == d_agg0).all()):
                res["mismatches"] += 1
            if rnd >= a.warmup:
                times[leg].append(ms)
    res["ms_median"] = {leg: round(float(np.median(v)), 3) for leg, v in times.items()}
    res["ms_min"] = {leg: round(float(np.min(v)), 3) for leg, v in times.items()}
    res["ratio"] = {"verify_aggregate/verify_batch_msm": round(res["ms_median"]["verify_aggregate"] / res["ms_median"]["verify_batch_msm"], 3),
                    "aggregate/hash_message": round(res["ms_median"]["aggregate"] / res["ms_median"]["hash_message"], 3),
                    "aggregate_checked/hash_message": round(res["ms_median"]["aggregate_checked"] / res["ms_median"]["hash_message"], 3)}
    kern = {}
    for name, fn in (("verify_aggregate", verify_agg), ("aggregate", lambda: aggregate(d_agg))):
        eng.sync()
        eng.enable_timing(True)
        fn()
        eng.sync()
        kern[name] = {}
        for k in KERNELS:
            avg, cnt = eng.read_timing(k)
            if cnt:
                kern[name][k] = [round(avg, 4), int(cnt)]
        eng.enable_timing(False)
    res["kernel_ms_avg_launches"] = kern
    # nanoseconds per Rescue permutation: the challenge hash of an 80-byte message is 4 per lane (25 felts), a leaf and a
    # coefficient 1 per lane, the tree n - 1 in all plus the root
    kv = kern["verify_aggregate"]
    perms = {"ssa_k_hash": 4 * n, "ag_k_leaf": n, "ag_k_tree": n, "ag_k_coeff": n}
    res["ns_per_permutation"] = {k: round(kv[k][0] * 1e6 / perms[k], 3) for k in perms if k in kv}
    if all(k in kv for k in perms):
        tr = kv["ag_k_leaf"][0] + kv["ag_k_tree"][0] + kv["ag_k_coeff"][0]
        res["ns_per_permutation"]["transcript"] = round(tr * 1e6 / (3 * n), 3)
    print(json.dumps(res))
    eng.close()
    return 0 if res["mismatches"] == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
