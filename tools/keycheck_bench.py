#!/usr/bin/env python3
"""ssa_keycache_selfcheck and ssa_keyset_selfcheck against the only alternative there was: building the rows again
(DESIGN.md section 17).  One engine on cuda:0.

Per cache size u (--us, default 2^16, 2^20, 2^22): a key cache of u rows is filled by cached calls over u distinct honest
signers (slices of at most 2^20 lanes), then, ALTERNATING round by round, wall time per call (each closed by the call's
own synchronise) and kernel time per call from ssa_ctx_read_timing:
  light_u<U>    ssa_keycache_selfcheck(0)
  deep_u<U>     ssa_keycache_selfcheck(SSA_KEYCHECK_DEEP)
  rebuild_u<U>  ssa_keycache_clear + the cached call(s) that fill the cache again: the remedy before this check.  Its
                kernel time is ssa_k_keyset_build's alone -- the yardstick K of the light check -- and its wall time is
                what a caller paid.
--comb-keys m (default 16): the same two checks on a key set of m keys in comb mode (light_comb / deep_comb).
After the timed rounds every object is checked once more and must be clean.  One JSON line out."""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CHECK_KEYS = ("ssa_k_keytab_check", "ssa_k_keytab_rebuild", "ssa_k_keytab_deep", "ssa_k_keycomb_check")


def _scalars(rng, n):
    v = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    v[:, 31] &= 0x3F
    v[:, 0] |= 1
    return v


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--us", type=str, default="65536,1048576,4194304")
    ap.add_argument("--comb-keys", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seed", type=int, default=0x6CEC)
    a = ap.parse_args()
    import torch
    import schnorr_sig_amd as ssa
    dev = torch.device("cuda", 0)
    eng = ssa.Engine(0)
    rng = np.random.default_rng(a.seed)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)   # noqa: E731
    res = {"metric": "key-table self-check", "rounds": a.rounds, "warmup": a.warmup,
           "library_sha256": hashlib.sha256(open(ssa.LIB_PATH, "rb").read()).hexdigest()[:16],
           "device": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d"), "unclean": 0,
           "wall_ms": {}, "kernel_ms": {}, "out": {}}

    def kernel_ms(keys):
        total = 0.0
        for k in keys:
            avg, cnt = eng.read_timing(k)
            total += avg * cnt
        return total

    def timed(fn, keys):
        """-> (wall ms, kernel ms under ssa_ctx_enable_timing) of one call"""
        eng.sync()
        eng.enable_timing(True)
        kernel_ms(keys)                          # drains the keys
        t0 = time.perf_counter()
        out = fn()
        eng.sync()
        w = (time.perf_counter() - t0) * 1e3
        k = kernel_ms(keys)
        eng.enable_timing(False)
        return w, k, out

    def run_legs(legs, tag):
        wall = {name: [] for name, _, _ in legs}
        kern = {name: [] for name, _, _ in legs}
        for rnd in range(a.warmup + a.rounds):
            for name, fn, keys in legs:
                w, k, out = timed(fn, keys)
                if isinstance(out, dict):
                    res["out"][name + tag] = {f: out[f] for f in ssa.KEYCHECK_FIELDS}
                    res["unclean"] += 0 if out["ok"] else 1
                if rnd >= a.warmup:
                    wall[name].append(w)
                    kern[name].append(k)
        for name, _, _ in legs:
            for dst, src in ((res["wall_ms"], wall), (res["kernel_ms"], kern)):
                v = src[name]
                dst[name + tag] = [round(float(np.median(v)), 4), round(float(np.min(v)), 4), round(float(np.max(v)), 4)]

    for us in [int(x) for x in a.us.split(",") if x]:
        try:
            cache = eng.keycache_create(us)
        except RuntimeError as e:                # no memory for a cache of this size: say so and go on
            res["out"]["skipped_u%d" % us] = str(e)
            continue
        slices = []
        for lo in range(0, us, 1 << 20):
            n = min(1 << 20, us - lo)
            msgs = rng.integers(0, 256, (n, 80), dtype=np.uint8)
            pks, sigs = eng.keygen_sign_many(_scalars(rng, n), _scalars(rng, n), msgs)
            slices.append((t(sigs), t(pks), t(msgs), n))
        d_st = torch.empty(1 << 20, dtype=torch.uint8, device=dev)
        d_nf = torch.zeros(1, dtype=torch.int64, device=dev)

        def fill():
            for s, p, m, n in slices:
                eng.verify_many_cached_device(cache, s.data_ptr(), p.data_ptr(), m.data_ptr(), n, 80, 0, 0,
                                              d_st.data_ptr(), d_nf.data_ptr(), check_torsion=True)

        def rebuild():
            cache.clear()
            fill()

        fill()
        eng.sync()
        assert cache.info()["held"] == us, cache.info()
        run_legs([("light", lambda: cache.selfcheck(), CHECK_KEYS), ("deep", lambda: cache.selfcheck(deep=True), CHECK_KEYS),
                  ("rebuild", rebuild, ("ssa_k_keyset_build",))], "_u%d" % us)
        res["unclean"] += 0 if cache.selfcheck(deep=True)["ok"] else 1
        cache.close()
        del slices
        torch.cuda.empty_cache()

    if a.comb_keys:
        pks = eng.pubkey_many(_scalars(rng, a.comb_keys))
        ks = eng.keyset_create(pks, kind="comb")
        run_legs([("light", lambda: ks.selfcheck(), CHECK_KEYS), ("deep", lambda: ks.selfcheck(deep=True), CHECK_KEYS)],
                 "_comb%d" % a.comb_keys)
        ks.close()
    print(json.dumps(res))
    eng.close()
    return 0 if res["unclean"] == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
