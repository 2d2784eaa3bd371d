#!/usr/bin/env python3
"""ssa_verify_keyed_many_cached_device on 130-byte wire records against what a caller could do without it, all with
SSA_FLAG_CHECK_TORSION.  One engine on cuda:0, device-resident batches of --n records with
80-byte messages by u distinct signers (u = 1000, n/16, n), library-drawn coefficients, key caches of --capacity rows.

Legs, timed in one process and ALTERNATING round by round (each call closed by a synchronise; wall time per call):
  comp_cold_u<U> / comp_warm_u<U>     the composition the parent commit allows: the records split into keys and
                       signatures (two strided device copies), ssa_decompress_many_device on all n keys, then
                       ssa_verify_many_cached_device on an AFFINE cache (cleared just before / warm)    (--legs parent)
  affine_warm_u<U>     ssa_verify_many_cached_device, warm, on keys decompressed beforehand (not timed)   (--legs parent)
  decompress_u<U>      ssa_decompress_many_device alone over the n keys                                  (--legs parent)
  exact_u<U>           ssa_verify_keyed_many, the exact call on HOST buffers (--exact; slow)              (--legs parent)
  wire_cold_u<U> / wire_warm_u<U>     ssa_verify_keyed_many_cached_device on a WIRE cache               (--legs new)
  wire_host_warm_u<U>  ssa_verify_keyed_many_cached on host buffers, warm                                 (--legs new)
--legs parent uses nothing the parent commit lacks: the same file run from a checkout of the parent measures the
baseline on the parent's library in the same session.  After every timed call its status vector and count are checked
against ssa_verify_many's on the unpacked records.  Per-stage times of one extra call per leg come from
ssa_ctx_read_timing.  One JSON line out."""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STAGES = ("keyed_split", "dedup", "keycache_lookup", "dedup_gather", "ssa_k_keyed_decompress", "keycache_insert",
          "ssa_k_keyset_build", "keycache_map", "keyed_expand", "screen_keymask", "ssa_k_hash", "msm_k_prepare", "msm_sort",
          "msm_k_buckets", "msm_reduce", "msm_k_finish_seg", "screen_mark", "screen_list_gather", "ssa_k_verify_keyed",
          "screen_list_scatter", "ssa_k_verify", "ssa_k_unpack_keyed")
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
    ap.add_argument("--us", type=str, default="1000,n/16,n")
    ap.add_argument("--capacity", type=int, default=1 << 21)
    ap.add_argument("--exact", action="store_true")
    ap.add_argument("--seed", type=int, default=0x18CA)
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
    with_parent, with_new = "parent" in want_legs, "new" in want_legs
    affine = eng.keycache_create(a.capacity) if with_parent else None
    wire = eng.keycache_create(a.capacity, wire=True) if with_new else None
    inputs, host, ref = {}, {}, {}
    d_st = torch.empty(n, dtype=torch.uint8, device=dev)
    d_nf = torch.zeros(1, dtype=torch.int64, device=dev)
    # the composition's own buffers: what a caller would hold
    c_keys = torch.empty((n, 49), dtype=torch.uint8, device=dev)
    c_sigs = torch.empty((n, 81), dtype=torch.uint8, device=dev)
    c_pks = torch.empty((n, 96), dtype=torch.uint8, device=dev)
    c_inf = torch.empty(n, dtype=torch.uint8, device=dev)
    c_dst = torch.empty(n, dtype=torch.uint8, device=dev)

    def decompress(d_keys, d_pks, d_inf):
        rc = ssa._lib.ssa_decompress_many_device(eng._ctx, d_keys.data_ptr(), n, d_pks.data_ptr(), d_inf.data_ptr(),
                                                 c_dst.data_ptr())
        assert rc == 0, rc

    for us in a.us.split(","):
        u = size(us)
        idx = rng.integers(0, u, size=n)
        idx[:u] = np.arange(u)
        rng.shuffle(idx)
        msgs = rng.integers(0, 256, (n, 80), dtype=np.uint8)
        pks, keyed = eng.keygen_sign_many(_scalars(rng, u)[idx], _scalars(rng, n), msgs, keyed=True)
        key = "u%s" % us
        d_k, d_m, d_p = t(keyed), t(msgs), t(pks)
        d_s = t(keyed[:, 49:])
        inputs[key] = (d_k, d_m, d_p, d_s)
        host[key] = (keyed, msgs)
        out = torch.empty(n, dtype=torch.uint8, device=dev)     # what ssa_verify_many says (not timed)
        nf = torch.zeros(1, dtype=torch.int64, device=dev)
        eng.verify_many_device(d_s.data_ptr(), d_p.data_ptr(), d_m.data_ptr(), n, 80, out.data_ptr(), nf.data_ptr(),
                               **TORSION)
        eng.sync()
        ref[key] = (out, int(nf.item()))

    def comp(key):
        k, m, _, _ = inputs[key]
        c_keys.copy_(k[:, :49])
        c_sigs.copy_(k[:, 49:])
        torch.cuda.current_stream().synchronize()            # (the engine runs on a stream of its own)
        decompress(c_keys, c_pks, c_inf)
        return eng.verify_many_cached_device(affine, c_sigs.data_ptr(), c_pks.data_ptr(), m.data_ptr(), n, 80, 0, 0,
                                             d_st.data_ptr(), d_nf.data_ptr(), d_pk_inf=c_inf.data_ptr(), **TORSION)

    def affine_warm(key):
        _, m, p, s = inputs[key]
        return eng.verify_many_cached_device(affine, s.data_ptr(), p.data_ptr(), m.data_ptr(), n, 80, 0, 0, d_st.data_ptr(),
                                             d_nf.data_ptr(), **TORSION)

    def decompress_only(key):
        decompress(c_keys, c_pks, c_inf)
        return None

    def exact(key):
        st, nf = eng.verify_keyed_many(*host[key], check_torsion=True)
        d_st.copy_(t(st))
        d_nf.fill_(nf)
        return None

    def wire_dev(key):
        k, m, _, _ = inputs[key]
        return eng.verify_keyed_many_cached_device(wire, k.data_ptr(), m.data_ptr(), n, 80, 0, 0, d_st.data_ptr(),
                                                   d_nf.data_ptr(), **TORSION)

    def wire_host(key):
        st, nf, stats = eng.verify_keyed_many_cached(wire, *host[key], **TORSION)
        d_st.copy_(t(st))
        d_nf.fill_(nf)
        return stats

    def prepare(leg):            # not timed
        if leg[0] == "comp_cold":
            affine.clear()
        elif leg[0] == "wire_cold":
            wire.clear()
        elif leg[0] == "decompress":
            c_keys.copy_(inputs[leg[1]][0][:, :49])
        torch.cuda.synchronize()

    def wall(fn):
        eng.sync()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        eng.sync()
        return (time.perf_counter() - t0) * 1e3

    legs = []
    for key in inputs:
        if with_parent:
            # in this order: the cold call is what warms the cache (the composition's keys and the pre-decompressed
            # ones are the same bytes, so affine_warm finds what comp_cold inserted)
            legs += [("comp_cold", key), ("comp_warm", key), ("affine_warm", key), ("decompress", key)]
            if a.exact:
                legs.append(("exact", key))
        if with_new:
            legs += [("wire_cold", key), ("wire_warm", key), ("wire_host_warm", key)]
    run = {"comp_cold": comp, "comp_warm": comp, "affine_warm": affine_warm, "decompress": decompress_only, "exact": exact,
           "wire_cold": wire_dev, "wire_warm": wire_dev, "wire_host_warm": wire_host}
    name = lambda leg: "%s_%s" % leg   # noqa: E731
    times = {name(leg): [] for leg in legs}
    stats = {}
    res = {"metric": "verify_keyed_many_cached", "n": n, "msg_len": 80, "rounds": a.rounds, "warmup": a.warmup,
           "legs": a.legs, "capacity": a.capacity,
           "library_sha256": hashlib.sha256(open(ssa.LIB_PATH, "rb").read()).hexdigest()[:16],
           "device": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d"), "mismatches": 0}
    for rnd in range(a.warmup + a.rounds):
        for leg in legs:
            prepare(leg)
            got = []
            ms = wall(lambda: got.append(run[leg[0]](leg[1])))
            want, wnf = ref[leg[1]]
            if leg[0] != "decompress" and (not bool((d_st == want).all()) or int(d_nf.item()) != wnf):
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
        if leg[0] in ("exact", "wire_host_warm"):
            continue
        prepare(leg)
        eng.sync()
        eng.enable_timing(True)
        run[leg[0]](leg[1])
        eng.sync()
        stage[name(leg)] = {}
        for k in STAGES + ("ssa_k_decompress",):
            avg, cnt = eng.read_timing(k)
            if cnt:
                stage[name(leg)][k] = [round(avg * cnt, 4), int(cnt)]
        eng.enable_timing(False)
    res["stage_ms_total_launches"] = stage
    res["cache_info"] = {}
    for label, cache in (("affine", affine), ("wire", wire)):
        if cache is not None:
            res["cache_info"][label] = cache.info()
            cache.close()
    print(json.dumps(res))
    eng.close()
    return 0 if res["mismatches"] == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
