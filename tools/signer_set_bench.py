#!/usr/bin/env python3
"""Rates of signing with a signer set (ssa_sign_many_indexed_device: KeyPair::sign, the key pair read by index) against
ssa_keygen_sign_many_ex_device (PrivateKey::sign) run on the gathered key rows with the same nonces and messages:
n signatures of 80-byte messages, device buffers, one engine on cuda:0, for each m in --keys:

    indexed        ssa_sign_many_indexed_device, throughput signer
    indexed_ct     the same with SSA_FLAG_SIGN_CT
    keygen         ssa_keygen_sign_many_ex_device on sks[key_idx], throughput signer
    keygen_ct      the same with SSA_FLAG_SIGN_CT

Each leg: `--warmup` untimed calls, then `--steps` calls closed by one device synchronise; per-kernel times from
ssa_ctx_read_timing.  Also reported per m: the set's creation time (a warmed-up ssa_signer_set_create_device, which
synchronises) and whether each indexed leg's output is byte-identical to its keygen leg.  One JSON line out, with a
sha256 over each leg's outputs and the library's own sha256."""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
KERNELS = ("ssa_k_sign_indexed", "ssa_k_sign_indexed_ct", "ssa_k_sign", "ssa_k_sign_ct")
CREATE_KERNELS = ("ssa_k_signer_keys", "ssa_k_pubkey_ct", "ssa_k_compress")


def _scalars(rng, n):
    v = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    v[:, 31] &= 0x3F          # below 2^254 < q
    v[:, 0] |= 1              # non-zero
    return v


def _timed(eng, fn, steps, warmup, kernels):
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
    for k in kernels:
        avg, cnt = eng.read_timing(k)
        if cnt:
            kern[k] = round(avg, 3)
    eng.enable_timing(False)
    return dt, kern


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--keys", type=str, default="1,64,65536")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seed", type=int, default=0x5E7)
    a = ap.parse_args()
    import torch
    import schnorr_sig_amd as ssa
    dev = torch.device("cuda", 0)
    eng = ssa.Engine(0)
    rng = np.random.default_rng(a.seed)
    n = a.n
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)   # noqa: E731
    d_nonces = t(_scalars(rng, n))
    d_msgs = t(rng.integers(0, 256, (n, 80), dtype=np.uint8))
    d_pks = torch.zeros((n, 96), dtype=torch.uint8, device=dev)
    res = {"metric": "signer_set_rates", "n": n, "msg_len": 80, "steps": a.steps, "warmup": a.warmup,
           "library_sha256": hashlib.sha256(open(ssa.LIB_PATH, "rb").read()).hexdigest()[:16],
           "device": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d")}
    for m in (int(x) for x in a.keys.split(",")):
        d_sks = t(_scalars(rng, m))
        idx = rng.integers(0, m, n, dtype=np.uint32)
        d_idx = t(idx.view(np.int32))
        d_rows = d_sks[torch.from_numpy(idx.astype(np.int64)).to(dev)].contiguous()     # sks[key_idx]
        eng.signer_set_create_device(d_sks.data_ptr(), m).close()                      # warm-up (tables, allocator)
        eng.enable_timing(True)
        t0 = time.perf_counter()
        ss = eng.signer_set_create_device(d_sks.data_ptr(), m)
        create_ms = (time.perf_counter() - t0) * 1e3
        create_kern = {k: round(avg, 3) for k, (avg, cnt) in ((k, eng.read_timing(k)) for k in CREATE_KERNELS) if cnt}
        eng.enable_timing(False)
        assert (eng.signer_set_status(ss) == 0).all()
        outs = {name: torch.zeros((n, 81), dtype=torch.uint8, device=dev) for name in
                ("indexed", "indexed_ct", "keygen", "keygen_ct")}
        legs = {
            "indexed": lambda o, ct: eng.sign_many_indexed_device(ss, d_idx.data_ptr(), d_nonces.data_ptr(),
                                                                  d_msgs.data_ptr(), n, 80, o.data_ptr(),
                                                                  constant_time=ct),
            "keygen": lambda o, ct: eng.keygen_sign_many_device(d_rows.data_ptr(), d_nonces.data_ptr(),
                                                                d_msgs.data_ptr(), n, 80, d_pks.data_ptr(),
                                                                o.data_ptr(), constant_time=ct),
        }
        r = {"create_ms": round(create_ms, 3), "create_kernel_ms": create_kern}
        for name, fn in legs.items():
            for ct in (False, True):
                leg = name + ("_ct" if ct else "")
                o = outs[leg]
                dt, kern = _timed(eng, lambda: fn(o, ct), a.steps, a.warmup, KERNELS)
                r[leg] = {"ms": round(dt * 1e3, 3), "sigs_per_s": round(n / dt), "kernel_ms": kern,
                          "out_sha256": hashlib.sha256(o.cpu().numpy().tobytes()).hexdigest()[:16]}
        for leg in ("indexed", "indexed_ct"):
            base = leg.replace("indexed", "keygen")
            r[leg]["identical_to_" + base] = bool(torch.equal(outs[leg], outs[base]))
            r[leg]["speedup_vs_" + base] = round(r[base]["ms"] / r[leg]["ms"], 3)
        ss.close()
        res["m=%d" % m] = r
    print(json.dumps(res))
    eng.close()


if __name__ == "__main__":
    main()
