#!/usr/bin/env python3
"""Rates of batched key derivation (ssa_derive.hpp) at n children, device buffers, one engine on cuda:0:

    xpub       one xpub -> n non-hardened children, with the 96-byte affine keys (derive_normal_public)
    xprv       one xprv -> n children, half of them hardened (derive_private)
    xprv_pub   one xprv -> n xpub children, mixed indices (derive_public)

and, in the same process, ssa_pubkey_many at n as the yardstick (one constant-time base multiplication per key).
Each leg: `--warmup` untimed calls, then `--steps` calls closed by one device synchronise; per-kernel times from
ssa_ctx_read_timing.  One JSON line out, with a sha256 over each leg's outputs (two builds must agree) and the library's
own sha256."""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
KERNELS = ("ssa_k_derive_prep", "ssa_k_xpub_derive", "ssa_k_xprv_derive", "ssa_k_pubkey_ct")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seed", type=int, default=0xD3B)
    a = ap.parse_args()
    import torch
    import schnorr_sig_amd as ssa
    dev = torch.device("cuda", 0)
    eng = ssa.Engine(0)
    rng = np.random.default_rng(a.seed)
    n = a.n
    xprv, st = eng.xprv_master_many(rng.integers(0, 256, (1, 32), dtype=np.uint8))
    assert st[0] == 0
    xpub, st = eng.xprv_derive_many(xprv, [0], derive_public=True)     # any xpub: the child 0 of the master key
    xprv, st2 = eng.xprv_derive_many(xprv, [0])                      # ... and its private side
    assert st[0] == 0 and st2[0] == 0
    soft = rng.integers(0, 1 << 31, n, dtype=np.uint32)
    mixed = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    sks = []
    while len(sks) < n:     # canonical non-zero scalars for the yardstick
        v = rng.integers(0, 256, (n, 32), dtype=np.uint8)
        v[:, 31] &= 0x3F
        sks.extend(v)
    sks = np.stack(sks[:n])
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)   # noqa: E731
    d_prv, d_pub, d_soft, d_mixed, d_sks = t(xprv[0]), t(xpub[0]), t(soft.view(np.int32)), t(mixed.view(np.int32)), t(sks)
    o81, o96, oinf, ost = (torch.zeros(s, dtype=torch.uint8, device=dev) for s in ((n, 81), (n, 96), (n,), (n,)))
    o64 = torch.zeros((n, 64), dtype=torch.uint8, device=dev)
    legs = {
        "xpub": (lambda: eng.xpub_derive_many_device(d_pub.data_ptr(), 1, d_soft.data_ptr(), n, o81.data_ptr(),
                                                     ost.data_ptr(), d_pks=o96.data_ptr(), d_pk_inf=oinf.data_ptr()),
                 (o81, o96, oinf, ost)),
        "xprv": (lambda: eng.xprv_derive_many_device(d_prv.data_ptr(), 1, d_mixed.data_ptr(), n, o64.data_ptr(),
                                                     ost.data_ptr()), (o64, ost)),
        "xprv_pub": (lambda: eng.xprv_derive_many_device(d_prv.data_ptr(), 1, d_mixed.data_ptr(), n, o81.data_ptr(),
                                                         ost.data_ptr(), derive_public=True), (o81, ost)),
        "pubkey_many": (lambda: eng.pubkey_many_device(d_sks.data_ptr(), n, o96.data_ptr()), (o96,)),
    }
    res = {"metric": "derive_rates", "n": n, "steps": a.steps, "warmup": a.warmup,
           "library_sha256": hashlib.sha256(open(ssa.LIB_PATH, "rb").read()).hexdigest()[:16],
           "device": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d")}
    for name, (fn, outs) in legs.items():
        eng.enable_timing(False)
        for _ in range(a.warmup):
            fn()
        eng.sync()
        eng.enable_timing(True)
        t0 = time.perf_counter()
        for _ in range(a.steps):
            fn()
        eng.sync()
        dt = (time.perf_counter() - t0) / a.steps
        kern = {}
        for k in KERNELS:
            avg, cnt = eng.read_timing(k)
            if cnt:
                kern[k] = round(avg, 3)
        eng.enable_timing(False)
        h = hashlib.sha256()
        for o in outs:
            h.update(o.cpu().numpy().tobytes())
        ok = int((ost.cpu().numpy() == 0).sum()) if name != "pubkey_many" else n
        res[name] = {"ms": round(dt * 1e3, 3), "keys_per_s": round(n / dt), "kernel_ms": kern, "ok_lanes": ok,
                     "out_sha256": h.hexdigest()[:16]}
    print(json.dumps(res))
    eng.close()


if __name__ == "__main__":
    main()
