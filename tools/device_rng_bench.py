#!/usr/bin/env python3
"""Cost of drawing the signing nonces on the device (ssa_*_rng).  One engine on cuda:0.

1. Device buffers, n signatures of 80-byte messages by m key pairs of a signer set: ssa_sign_many_indexed_device with
   caller nonces against ssa_sign_many_indexed_rng_device, for the throughput and the constant-time signer.  Per leg:
   `--warmup` untimed calls, then `--steps` calls closed by one synchronise; per-kernel times from ssa_ctx_read_timing
   (ssa_k_draw_scalars_ct is the draw's own kernel).
2. End to end from Python, SignerSet.sign(..., rng=os.urandom) against rng=DEVICE_RNG, for each n in --e2e (each timed
   once after one warm-up call; the os.urandom leg of the largest n is what the host-side draw costs).
One JSON line out, with the library's own sha256."""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
KERNELS = ("ssa_k_draw_scalars_ct", "ssa_k_sign_indexed", "ssa_k_sign_indexed_ct")


def _scalars(rng, n):
    v = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    v[:, 31] &= 0x3F          # below 2^254 < q
    v[:, 0] |= 1              # non-zero
    return v


def _timed(eng, fn, steps, warmup):
    eng.enable_timing(False)
    for _ in range(warmup):
        fn()
    eng.sync()
    eng.enable_timing(True)
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    eng.sync()
    dt = (time.perf_counter() - t0) / steps
    kern = {}
    for k in KERNELS:
        avg, cnt = eng.read_timing(k)
        if cnt:
            kern[k] = round(avg, 4)
    eng.enable_timing(False)
    return dt, kern


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--m", type=int, default=64)
    ap.add_argument("--e2e", type=str, default="65536,1048576")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seed", type=int, default=0x12A)
    a = ap.parse_args()
    import torch
    import schnorr_sig_amd as ssa
    dev = torch.device("cuda", 0)
    eng = ssa.Engine(0)
    rng = np.random.default_rng(a.seed)
    n, m = a.n, a.m
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)   # noqa: E731
    d_nonces = t(_scalars(rng, n))
    d_msgs = t(rng.integers(0, 256, (n, 80), dtype=np.uint8))
    d_idx = t(rng.integers(0, m, n, dtype=np.uint32).view(np.int32))
    d_out = torch.zeros((n, 81), dtype=torch.uint8, device=dev)
    ss = eng.signer_set_create_device(t(_scalars(rng, m)).data_ptr(), m)
    res = {"metric": "device_rng_cost", "n": n, "m": m, "msg_len": 80, "steps": a.steps, "warmup": a.warmup,
           "library_sha256": hashlib.sha256(open(ssa.LIB_PATH, "rb").read()).hexdigest()[:16],
           "device": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d")}
    for ct in (False, True):
        name = "ct" if ct else "throughput"
        caller = lambda: eng.sign_many_indexed_device(ss, d_idx.data_ptr(), d_nonces.data_ptr(), d_msgs.data_ptr(),  # noqa
                                                      n, 80, d_out.data_ptr(), constant_time=ct)
        drawn = lambda: eng.sign_many_indexed_rng_device(ss, d_idx.data_ptr(), d_msgs.data_ptr(), n, 80,  # noqa
                                                         d_out.data_ptr(), constant_time=ct)
        dt_c, k_c = _timed(eng, caller, a.steps, a.warmup)
        dt_r, k_r = _timed(eng, drawn, a.steps, a.warmup)
        sign_k = "ssa_k_sign_indexed_ct" if ct else "ssa_k_sign_indexed"
        draw_ms = k_r.get("ssa_k_draw_scalars_ct", 0.0)
        res[name] = {"caller_nonces_ms": round(dt_c * 1e3, 3), "device_rng_ms": round(dt_r * 1e3, 3),
                     "caller_kernel_ms": k_c, "device_rng_kernel_ms": k_r, "draw_ms": draw_ms,
                     "draw_share_of_signer": round(draw_ms / k_r[sign_k], 4) if k_r.get(sign_k) else None}
    ss.close()
    # end to end from Python
    for ne in (int(x) for x in a.e2e.split(",")):
        ss = ssa.SignerSet.generate(m, eng)
        idx = rng.integers(0, m, ne).tolist()
        msgs = [bytes(rng.integers(0, 256, 80, dtype=np.uint8)) for _ in range(ne)]
        r = {}
        for leg, rg in (("os_urandom", os.urandom), ("device_rng", ssa.DEVICE_RNG)):
            ss.sign(idx[:1024], msgs[:1024], rg)                  # warm-up
            t0 = time.perf_counter()
            ss.sign(idx, msgs, rg)
            r[leg + "_s"] = round(time.perf_counter() - t0, 3)
        r["speedup"] = round(r["os_urandom_s"] / r["device_rng_s"], 2)
        res["e2e_n=%d" % ne] = r
        ss.close()
    print(json.dumps(res))
    eng.close()


if __name__ == "__main__":
    main()
