#!/usr/bin/env python3
"""ssa_verify_many_dedup against ssa_verify_many.  One engine on cuda:0, device-resident batches
of --n signatures with 80-byte messages by u distinct signers, sixteen corrupted lanes in each.

Legs, timed in one process and ALTERNATING round by round (each call closed by a synchronise; wall time per call):
  base_torsion / base_flag          ssa_verify_many_device with SSA_FLAG_CHECK_TORSION / with SSA_FLAG_SIG_FLAG_BYTE alone
                                    (the parent's code paths), on the all-distinct batch
  keyed_<flags>_u<U>                ssa_verify_many_dedup_device with the keyed route FORCED (ssa_k_verify_keyed on the
                                    u tables), u = 1, 1000, n/16, n/4, n/2, n
  default_<flags>_u<U>              the call as shipped (the context's own policy): at u = n the price of a wasted dedup
After every timed dedup call its status vector and count are compared with ssa_verify_many's on the same input.
Per-kernel times of one extra call per leg come from ssa_ctx_read_timing.  One JSON line out."""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
KERNELS = ("dedup", "dedup_gather", "ssa_k_keyset_build", "ssa_k_hash", "ssa_k_verify_keyed", "ssa_k_verify")
FLAGS = {"torsion": dict(check_torsion=True, sig_flag_byte=False), "flag": dict(check_torsion=False, sig_flag_byte=True)}


def _scalars(rng, n):
    v = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    v[:, 31] &= 0x3F
    v[:, 0] |= 1
    return v


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--forms", type=str, default="keyed,default")
    ap.add_argument("--seed", type=int, default=0xDED0)
    a = ap.parse_args()
    import torch
    import schnorr_sig_amd as ssa
    dev = torch.device("cuda", 0)
    eng = ssa.Engine(0)
    rng = np.random.default_rng(a.seed)
    n = a.n
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)   # noqa: E731
    us = {"1": 1, "1000": min(1000, n), "n/16": n // 16, "n/4": n // 4, "n/2": n // 2, "n": n}
    inputs = {}
    for name, u in us.items():
        idx = rng.integers(0, u, size=n)
        idx[:u] = np.arange(u)
        rng.shuffle(idx)
        msgs = rng.integers(0, 256, (n, 80), dtype=np.uint8)
        pks, sigs = eng.keygen_sign_many(_scalars(rng, u)[idx], _scalars(rng, n), msgs)
        for i in rng.choice(n, 16, replace=False):
            sigs[i, 50] ^= 4
        inputs[name] = (t(sigs), t(pks), t(msgs))
    d_st = torch.empty(n, dtype=torch.uint8, device=dev)
    d_nf = torch.zeros(1, dtype=torch.int64, device=dev)

    def base(name, fl, out=None, nf=None):
        s, p, m = inputs[name]
        eng.verify_many_device(s.data_ptr(), p.data_ptr(), m.data_ptr(), n, 80, (out if out is not None else d_st).data_ptr(),
                               (nf if nf is not None else d_nf).data_ptr(), **FLAGS[fl])

    def dedup(name, fl):
        s, p, m = inputs[name]
        return eng.verify_many_dedup_device(s.data_ptr(), p.data_ptr(), m.data_ptr(), n, 80, d_st.data_ptr(), d_nf.data_ptr(),
                                            **FLAGS[fl])

    def wall(fn):
        eng.sync()
        t0 = time.perf_counter()
        fn()
        eng.sync()
        return (time.perf_counter() - t0) * 1e3

    # what ssa_verify_many says about every input (not timed)
    ref = {}
    for name in inputs:
        for fl in FLAGS:
            out = torch.empty(n, dtype=torch.uint8, device=dev)
            nf = torch.zeros(1, dtype=torch.int64, device=dev)
            base(name, fl, out, nf)
            eng.sync()
            ref[(name, fl)] = (out, int(nf.item()))
    config = {"keyed": dict(max_distinct_ratio=2.0), "default": {}}
    forms = [f for f in a.forms.split(",") if f]
    legs = [("base", fl, "n") for fl in FLAGS] + [(form, fl, name) for form in forms for fl in FLAGS for name in inputs]
    key = lambda leg: "%s_%s%s" % (leg[0], leg[1], "" if leg[0] == "base" else "_u" + leg[2])   # noqa: E731
    times = {key(leg): [] for leg in legs}
    stats = {}
    res = {"metric": "verify_many_dedup", "n": n, "msg_len": 80, "rounds": a.rounds, "warmup": a.warmup,
           "library_sha256": hashlib.sha256(open(ssa.LIB_PATH, "rb").read()).hexdigest()[:16],
           "device": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d"), "distinct_keys": us, "mismatches": 0}
    for rnd in range(a.warmup + a.rounds):
        for leg in legs:
            form, fl, name = leg
            if form == "base":
                ms = wall(lambda: base(name, fl))
            else:
                eng.debug_dedup_config(**config[form])
                got = []
                ms = wall(lambda: got.append(dedup(name, fl)))
                stats[key(leg)] = [int(v) for v in got[0]]
                want, wnf = ref[(name, fl)]
                if not bool((d_st == want).all()) or int(d_nf.item()) != wnf:
                    res["mismatches"] += 1
            if rnd >= a.warmup:
                times[key(leg)].append(ms)
    res["ms_median"] = {k: round(float(np.median(v)), 3) for k, v in times.items()}
    res["ms_min"] = {k: round(float(np.min(v)), 3) for k, v in times.items()}
    res["ms_max"] = {k: round(float(np.max(v)), 3) for k, v in times.items()}
    res["baseline_spread_ms"] = {fl: round(res["ms_max"]["base_" + fl] - res["ms_min"]["base_" + fl], 3) for fl in FLAGS}
    res["ratio_to_baseline"] = {k: round(v / res["ms_median"]["base_" + k.split("_")[1]], 3) for k, v in res["ms_median"].items()}
    res["stats"] = stats
    # per-kernel times of one extra call per leg
    kern = {}
    for leg in legs:
        form, fl, name = leg
        eng.sync()
        eng.enable_timing(True)
        if form == "base":
            base(name, fl)
        else:
            eng.debug_dedup_config(**config[form])
            dedup(name, fl)
        eng.sync()
        kern[key(leg)] = {}
        for k in KERNELS:
            avg, cnt = eng.read_timing(k)
            if cnt:
                kern[key(leg)][k] = [round(avg, 4), int(cnt)]
        eng.enable_timing(False)
    eng.debug_dedup_config()
    res["kernel_ms_avg_launches"] = kern
    print(json.dumps(res))
    eng.close()
    return 0 if res["mismatches"] == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
