#!/usr/bin/env python3
"""A key cache under a flood of never-seen keys: SSA_KEYCACHE_EVICT_RECENT against the clear-only policy (DESIGN.md
section 19), by the protocol of section 16.  One engine on cuda:0, device-resident batches of --n signatures with 80-byte
messages, SSA_FLAG_CHECK_TORSION, library-drawn coefficients.

The workload: --validators keys (2^19) sign every batch; each batch also carries --fresh keys (2^14) that no earlier batch
of the cycle had, one lane each, at the end of the batch.  The cache has --capacity rows (2^19 + 2^16), so it overflows
every fourth batch.  A cycle is --cycle calls (16); the batches of a cycle differ in their last --fresh lanes only, which
are written into the batch before each call (not timed).  By the end of a cycle either policy has dropped every fresh key
of its first batches, so the cycles repeat the same 16 batches; the tool checks that every call inserts exactly --fresh
keys (or, on a clear, all of them).

Legs, timed in one process and ALTERNATING cycle by cycle (each call closed by a synchronise; wall time per call):
  clear    ssa_verify_many_cached_device on a cache with the default policy              (--legs clear)
  recent   the same on a cache switched to SSA_KEYCACHE_EVICT_RECENT                     (--legs recent)
  warm_clear / warm_recent   a batch of the validators alone, all hits, on either cache: what the stamp store in the
           look-up costs
--legs clear uses nothing the parent commit lacks: the same file run from a checkout of the parent measures the baseline
on the parent's library.  That run is the baseline of the bar.  After every timed call its status vector and count are
checked against ssa_verify_many's on the same input.  Per-stage times of one more cycle per leg, call by call, come
from ssa_ctx_read_timing (ssa_k_keyset_build of a call that clears is K_V, the cost of rechecking the validators).  One
JSON line out."""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STAGES = ("dedup", "keycache_lookup", "keycache_compact", "keycache_insert", "ssa_k_keyset_build", "keycache_map")
TORSION = dict(check_torsion=True, sig_flag_byte=False)
HITS, INSERTED, EVICTIONS, BYPASSED = 8, 9, 10, 11


def _scalars(rng, n):
    v = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    v[:, 31] &= 0x3F
    v[:, 0] |= 1
    return v


def move_probe(eng, torch, tails, d_m, nf):
    """A compaction that moves every survivor: a cache of 3 nf - 1 rows; the keys of tail 0 (rows 0 .. nf), those of tail 1
    (rows nf .. 2 nf), then tails 1 and 2 in one batch: nf hits, nf misses, K = nf and every surviving row lies at or
    above row K.  -> the compaction's launches (ms in all, count), the rows and bytes moved, the same call's time on a
    cache with room (no compaction) beside it"""
    s12, p12 = torch.cat([tails[1][0], tails[2][0]]), torch.cat([tails[1][1], tails[2][1]])
    m12 = torch.cat([d_m, d_m])
    st, cnt = torch.empty(2 * nf, dtype=torch.uint8, device=s12.device), torch.zeros(1, dtype=torch.int64, device=s12.device)
    out = {}
    for name, capacity in (("compacting", 3 * nf - 1), ("with_room", 4 * nf)):
        with eng.keycache_create(capacity) as cache:
            cache.set_eviction("recent")
            for k in (0, 1):
                eng.verify_many_cached_device(cache, tails[k][0].data_ptr(), tails[k][1].data_ptr(), d_m.data_ptr(), nf, 80, 0, 0,
                                              st.data_ptr(), cnt.data_ptr(), **TORSION)
            eng.sync()
            eng.enable_timing(True)
            eng.read_timing("keycache_compact")
            t0 = time.perf_counter()
            stats = eng.verify_many_cached_device(cache, s12.data_ptr(), p12.data_ptr(), m12.data_ptr(), 2 * nf, 80, 0, 0,
                                                  st.data_ptr(), cnt.data_ptr(), **TORSION)
            eng.sync()
            ms = (time.perf_counter() - t0) * 1e3
            avg, launches = eng.read_timing("keycache_compact")
            eng.enable_timing(False)
            ev = cache.eviction_info()
            out[name] = {"call_ms": round(ms, 3), "keycache_compact_ms_launches": [round(avg * launches, 4), int(launches)],
                         "rows_moved": ev["last_moved"], "bytes_moved": ev["last_moved"] * (4096 + 96 + 1 + 1 + 4),
                         "stats_8_to_11": [int(v) for v in stats[HITS:]], "rejected": int(cnt.item())}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--validators", type=int, default=1 << 19)
    ap.add_argument("--fresh", type=int, default=1 << 14)
    ap.add_argument("--capacity", type=int, default=(1 << 19) + (1 << 16))
    ap.add_argument("--cycle", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--bad", type=int, default=16)
    ap.add_argument("--legs", type=str, default="clear,recent")
    ap.add_argument("--seed", type=int, default=0xE71C)
    a = ap.parse_args()
    import torch
    import schnorr_sig_amd as ssa
    dev = torch.device("cuda", 0)
    eng = ssa.Engine(0)
    rng = np.random.default_rng(a.seed)
    n, nv, nf = a.n, a.validators, a.fresh
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)   # noqa: E731
    legs = [x for x in a.legs.split(",") if x]

    # the validators on every lane; the last nf lanes are overwritten per call
    idx = rng.integers(0, nv, size=n)
    idx[:nv] = np.arange(nv)
    rng.shuffle(idx[:n - nf])
    msgs = rng.integers(0, 256, (n, 80), dtype=np.uint8)
    pks, sigs = eng.keygen_sign_many(_scalars(rng, nv)[idx], _scalars(rng, n), msgs)
    if a.bad:
        sigs[rng.choice(np.arange(0, n - nf), a.bad, replace=False), 49] ^= 1
    d_s, d_p, d_m = t(sigs), t(pks), t(msgs)
    w_s, w_p = d_s.clone(), d_p.clone()                  # the validators alone (the warm legs)
    tails = []
    for k in range(a.cycle):
        fp, fs = eng.keygen_sign_many(_scalars(rng, nf), _scalars(rng, nf), msgs[n - nf:])
        tails.append((t(fs), t(fp)))
    d_st = torch.empty(n, dtype=torch.uint8, device=dev)
    d_nf = torch.zeros(1, dtype=torch.int64, device=dev)

    def set_tail(k):             # not timed
        d_s[n - nf:].copy_(tails[k][0])
        d_p[n - nf:].copy_(tails[k][1])
        torch.cuda.synchronize()

    def exact(s, p):
        out = torch.empty(n, dtype=torch.uint8, device=dev)
        cnt = torch.zeros(1, dtype=torch.int64, device=dev)
        eng.verify_many_device(s.data_ptr(), p.data_ptr(), d_m.data_ptr(), n, 80, out.data_ptr(), cnt.data_ptr(), **TORSION)
        eng.sync()
        return out, int(cnt.item())

    refs = []
    for k in range(a.cycle):
        set_tail(k)
        refs.append(exact(d_s, d_p))
    ref_warm = exact(w_s, w_p)

    caches = {}
    for leg in legs:
        caches[leg] = eng.keycache_create(a.capacity)
        if leg == "recent":
            caches[leg].set_eviction("recent")

    def call(cache, s, p):
        return eng.verify_many_cached_device(cache, s.data_ptr(), p.data_ptr(), d_m.data_ptr(), n, 80, 0, 0, d_st.data_ptr(),
                                             d_nf.data_ptr(), **TORSION)

    def wall(fn):
        eng.sync()
        t0 = time.perf_counter()
        fn()
        eng.sync()
        return (time.perf_counter() - t0) * 1e3

    res = {"metric": "keycache_eviction", "n": n, "validators": nv, "fresh": nf, "capacity": a.capacity, "cycle": a.cycle,
           "rounds": a.rounds, "warmup": a.warmup, "legs": a.legs, "msg_len": 80,
           "library_sha256": hashlib.sha256(open(ssa.LIB_PATH, "rb").read()).hexdigest()[:16],
           "device": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d"), "mismatches": 0, "unexpected": []}
    per_call = {leg: [[] for _ in range(a.cycle)] for leg in legs}       # ms of call k of the cycle, per round
    evicting = {leg: [[] for _ in range(a.cycle)] for leg in legs}
    warm = {leg: [] for leg in legs}

    def check(ref, leg, what):
        if not bool((d_st == ref[0]).all()) or int(d_nf.item()) != ref[1]:
            res["mismatches"] += 1
            res["unexpected"].append([leg, what, "status vector"])

    for rnd in range(a.warmup + a.rounds):
        for leg in legs:
            for k in range(a.cycle):
                set_tail(k)
                got = []
                ms = wall(lambda: got.append(call(caches[leg], d_s, d_p)))
                st = [int(v) for v in got[0]]
                check(refs[k], leg, k)
                first = rnd == 0 and k == 0                  # the one cold call of the leg
                if st[BYPASSED] or not (first or st[INSERTED] == nf or (st[EVICTIONS] and leg == "clear")):
                    res["unexpected"].append([leg, k, st[HITS:]])
                if rnd >= a.warmup:
                    per_call[leg][k].append(ms)
                    evicting[leg][k].append(st[EVICTIONS])
        for leg in legs:                                     # all hits: the validators alone
            ms = wall(lambda: call(caches[leg], w_s, w_p))
            check(ref_warm, leg, "warm")
            if rnd >= a.warmup:
                warm[leg].append(ms)

    def mmm(v):
        return [round(float(np.median(v)), 3), round(float(np.min(v)), 3), round(float(np.max(v)), 3)]

    for leg in legs:
        cyc = np.array(per_call[leg])                        # cycle x rounds
        ev = np.array(evicting[leg])
        out = {"mean_ms_per_call_median_min_max": mmm(cyc.mean(axis=0)),
               "evictions_per_cycle": [int(v) for v in sorted(set(ev.sum(axis=0).tolist()))],
               "warm_all_hits_ms_median_min_max": mmm(warm[leg])}
        if ev.any():
            out["evicting_call_ms_median_min_max"] = mmm(cyc[ev > 0])
        if (ev == 0).any():
            out["other_call_ms_median_min_max"] = mmm(cyc[ev == 0])
        res[leg] = out

    stage = {}
    for leg in legs:             # per-stage times of one more cycle per leg, call by call: [sum of the launches' ms, launches]
        eng.sync()
        eng.enable_timing(True)
        for k in STAGES:
            eng.read_timing(k)
        stage[leg] = []
        for k in range(a.cycle):
            set_tail(k)
            st = call(caches[leg], d_s, d_p)
            eng.sync()
            one = {"evictions": int(st[EVICTIONS])}
            for name in STAGES:
                avg, cnt = eng.read_timing(name)
                if cnt:
                    one[name] = [round(avg * cnt, 4), int(cnt)]
            stage[leg].append(one)
        eng.enable_timing(False)
    res["stage_ms_total_launches_per_call_of_one_cycle"] = stage
    if "recent" in legs:         # the steady state above moves no row (the validators sit in the front rows): a probe that does
        res["move_probe"] = move_probe(eng, torch, tails, d_m[n - nf:], nf)
    for leg in legs:
        res[leg]["cache_info"] = caches[leg].info()
        if leg == "recent":
            ev = caches[leg].eviction_info()
            res[leg]["eviction_info"] = ev
            row = 4096 + 96 + 1 + 1 + 4
            res[leg]["bytes_moved_last_compaction"] = ev["last_moved"] * row
        caches[leg].close()
    print(json.dumps(res))
    eng.close()
    return 0 if res["mismatches"] == 0 and not res["unexpected"] else 1


if __name__ == "__main__":
    sys.exit(main())
