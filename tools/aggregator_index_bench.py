#!/usr/bin/env python3
"""The leaf index of the streaming aggregator, measured on one GPU.

    python tools/aggregator_index_bench.py --baseline-lib /path/to/parent/libschnorr_sig_amd.so [--n 1048576]
                                           [--signers 65536] [--rounds 3] [--warmup 1] [--unchanged]

--n KeyedSignature records by --signers signers over 80-byte messages are held by a streaming aggregator made with
hold_admission and index (push_keyed_device through a wire cache); a block is a random permutation of them.
--baseline-lib is a build of the parent commit (without it this tree's own library stands in, and the comparison says
nothing).  The legs alternate in one process; each timed call has an untimed call of the same kind in front of it in
every round, starts behind a stream synchronisation and ends with one; medians and all samples are one JSON line.

  sync_stale        index_sync of a table that is stale (the pool filled again in front of the call, outside the clock)
  sync_increment    index_sync behind one more push of --increment lanes onto a synced index of n - increment lanes
  lookup_<share>    lookup_device of n ids of which <share> percent are held (100, 90, 50, 0)
  leaves_select     leaves_select_device of a random permutation
  chain_<share>     lookup_device + push_mixed_wire_device(require = 2) + finish_device from the block's ids (100, 99, 90;
                    the unknown lanes gathered in device memory beforehand, their number known to the caller)
  places_<share>    the same pair with the places handed in: what the lookup adds is chain - places
  parent_cached     reset, push_cached_wire_device + finish_device of the baseline library on the whole body: the
                    parent's only route from ids to a verdict without a map kept on the host

Bar: at shares of 90 and above every sample of chain_<share> lies below every sample of parent_cached.  After every
lookup the places are compared with the places the host knows (`mismatches`), after every chain the verdict with the
parent's.

--unchanged: the calls this tree must not have changed, against the baseline library, on objects created with flags 0
(and, reported beside them, on objects with the index): push_keyed_device of n records, drop_front(n / 2 + 1) and a
random-half remove_device, the pool filled again in front of every call.  The bar: the tree's median lies inside the
range of the baseline's own samples."""
import argparse
import ctypes as C
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from aggverifier_mixed_bench import ParentPool, _scalars, _summary      # noqa: E402

LOOKUP_SHARES, CHAIN_SHARES = (100, 90, 50, 0), (100, 99, 90)
KERNELS = ("agi_k_insert", "agi_k_lookup", "agx_k_leaves_select", "agx_k_select_verdict")


class ParentKeyed(ParentPool):
    """the baseline library's push_keyed_cached_device into its aggregator"""

    def __init__(self, path, capacity):
        super().__init__(path, capacity)
        vp, sz = C.c_void_p, C.c_size_t
        self.lib.ssa_aggregator_push_keyed_cached_device.argtypes = [vp, vp, vp, vp, vp, vp, sz, sz, sz, vp, vp, vp]

    def fill_keyed(self, d_keyed, d_msgs, step):
        n, kept = int(d_keyed.shape[0]), C.c_uint64(0)
        rc = self.lib.ssa_aggregator_reset(self.ag)
        for lo in range(0, n, step):
            cnt = min(step, n - lo)
            rc = rc or self.lib.ssa_aggregator_push_keyed_cached_device(
                self.ctx, self.ag, self.kc, d_keyed[lo:lo + cnt].data_ptr(), d_msgs[lo:lo + cnt].data_ptr(), None, 80, 80, cnt,
                None, C.byref(kept), None)
            if rc != 0 or kept.value != cnt:
                raise RuntimeError("baseline library: ssa_aggregator_push_keyed_cached_device gave %d, kept %d" % (rc, kept.value))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--signers", type=int, default=65536)
    ap.add_argument("--increment", type=int, default=1 << 16)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seed", type=int, default=0x36B)
    ap.add_argument("--baseline-lib", default=None, help="a build of the parent commit's library")
    ap.add_argument("--unchanged", action="store_true", help="the unchanged calls against the baseline, in a run of its own")
    a = ap.parse_args()
    import torch
    import schnorr_sig_amd as ssa
    dev = torch.device("cuda", 0)
    n, signers, inc = a.n, min(a.signers, a.n), min(a.increment, a.n // 2)
    eng = ssa.Engine(0)
    base_path = a.baseline_lib or ssa.LIB_PATH
    par = ParentKeyed(base_path, n)
    rng = np.random.default_rng(a.seed)
    msgs = rng.integers(0, 256, (n, 80), dtype=np.uint8)
    idx = rng.integers(0, signers, size=n)
    idx[:signers] = np.arange(signers)
    rng.shuffle(idx)
    pks, sigs = eng.keygen_sign_many(_scalars(rng, signers)[idx], _scalars(rng, n), msgs)
    wire, st = eng.compress_many(pks)
    assert (st == 0).all()
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)   # noqa: E731
    d_sigs, d_pks, d_msgs, d_wire = t(sigs), t(pks), t(msgs), t(wire)
    d_keyed = torch.cat([d_wire, d_sigs], dim=1).contiguous()
    step = min(n, int(eng.info()["msm_slice"]))
    torch.cuda.synchronize()
    sha = lambda path: hashlib.sha256(open(path, "rb").read()).hexdigest()[:16]   # noqa: E731
    res = {"metric": "aggregator_index_unchanged_paths" if a.unchanged else "aggregator_index", "n": n, "signers": signers,
           "msg_len": 80, "rounds": a.rounds, "warmup": a.warmup, "library_sha256": sha(ssa.LIB_PATH),
           "baseline_sha256": sha(base_path), "baseline_is_this_tree": not a.baseline_lib,
           "device": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d"), "mismatches": 0}
    kc = eng.keycache_create(min(2 * n, 1 << 18), wire=True)

    def fill(ag, hi=n, lo=0, reset=True):
        if reset:
            ag.reset()
        for at in range(lo, hi, step):
            cnt = min(step, hi - at)
            kept, _ = ag.push_keyed_device(kc, d_keyed[at:at + cnt], d_msgs[at:at + cnt], want_stats=False)
            assert kept == cnt

    def syncs():
        eng.sync()
        par.sync()
        torch.cuda.synchronize()

    def run_legs(legs):
        """alternating legs; leg -> (prepare or None, call, sync, check or None): prepare runs outside the clock in front
        of BOTH calls, the untimed and the timed one"""
        times = {leg: [] for leg in legs}
        for rnd in range(a.warmup + a.rounds):
            for leg, (prepare, call, sync, check) in legs.items():
                ms = 0.0
                for _ in (False, True):
                    if prepare:
                        prepare()
                    syncs()
                    t0 = time.perf_counter()
                    call()
                    sync()
                    ms = (time.perf_counter() - t0) * 1e3
                if check and not check():
                    res["mismatches"] += 1
                if rnd >= a.warmup:
                    times[leg].append(ms)
        return times

    if a.unchanged:
        plain, flagged = eng.aggregator(n), eng.aggregator(n, index=True)
        d_mask = t((rng.integers(0, 2, n) == 1).astype(np.uint8))
        torch.cuda.synchronize()
        half = n // 2 + 1
        p_fill = lambda: par.fill_keyed(d_keyed, d_msgs, step)   # noqa: E731
        legs = {
            "parent_push_keyed": (None, p_fill, par.sync, None),
            "push_keyed": (None, lambda: fill(plain), eng.sync, None),
            "push_keyed_with_index": (None, lambda: fill(flagged), eng.sync, None),
            "parent_drop_front": (p_fill, lambda: par.drop_front(half), par.sync, None),
            "drop_front": (lambda: fill(plain), lambda: plain.drop_front(half), eng.sync, None),
            "drop_front_with_index": (lambda: fill(flagged), lambda: flagged.drop_front(half), eng.sync, None),
            "parent_remove": (p_fill, lambda: par.remove(d_mask), par.sync, None),
            "remove": (lambda: fill(plain), lambda: plain.remove_device(d_mask), eng.sync, None),
            "remove_with_index": (lambda: fill(flagged), lambda: flagged.remove_device(d_mask), eng.sync, None)}
        times = run_legs(legs)
        kept = [ag.info()["held"] for ag in (plain, flagged)]
        res["moves_kept"] = kept
        res["moves_bytes_equal"] = bool(kept[0] == kept[1] and (plain.finish_bytes() == flagged.finish_bytes()).all())
        res["mismatches"] += 0 if res["moves_bytes_equal"] else 1
        res.update(_summary(times))
        med = res["ms_median"]
        pairs = (("push_keyed", "parent_push_keyed"), ("drop_front", "parent_drop_front"), ("remove", "parent_remove"))
        res["bar_inside_parent_range"] = {k: bool(min(times[p]) <= med[k] <= max(times[p])) for k, p in pairs}
        res["index_cost_ms"] = {k: round(med[k + "_with_index"] - med[k], 3) for k, _ in pairs}
        handles = (plain, flagged, kc)
    else:
        pool = eng.aggregator(n, hold_admission=True, index=True)
        fill(pool)
        block = rng.permutation(n)                # the block: place of block lane i in the pool
        d_block = t(block.astype(np.int32))
        b_sigs, b_msgs, b_wire = (x[t(block)].contiguous() for x in (d_sigs, d_msgs, d_wire))
        b_rs = b_sigs[:, :49].contiguous()
        d_ids = torch.zeros(32 * n, dtype=torch.uint8, device=dev)
        d_res = torch.zeros(1, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        # the producer's side: the aggregate and the id column of the block, by the pool itself
        d_agg = torch.zeros(49 * n + 32, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        pool.finish_select_device(d_block, d_agg, d_res)
        pool.leaves_select_device(d_block, d_ids, d_res)
        eng.sync()
        assert int(d_res.item()) == 0
        d_e = d_agg[49 * n:].clone()
        random_ids = t(rng.integers(0, 256, 32 * n, dtype=np.uint8)).reshape(n, 32)
        d_places = torch.zeros(n, dtype=torch.int32, device=dev)
        d_count = torch.zeros(1, dtype=torch.int32, device=dev)
        d_v = torch.full((1,), 77, dtype=torch.int32, device=dev)
        d_vp = torch.full((1,), 77, dtype=torch.int32, device=dev)
        inputs = {}
        for share in sorted(set(LOOKUP_SHARES + CHAIN_SHARES)):
            known = np.zeros(n, bool)
            known[rng.choice(n, (n * share) // 100, replace=False)] = True
            d_known = t(known)
            ids = torch.where(d_known[:, None], d_ids.reshape(n, 32), random_ids).contiguous().reshape(-1)
            places = np.where(known, block, 0xFFFFFFFF).astype(np.uint32)
            d_unk = t(np.flatnonzero(~known))
            inputs[share] = (ids, t(places.view(np.int32)), b_rs[d_unk].contiguous(), b_wire[d_unk].contiguous(),
                             b_msgs[d_unk].contiguous(), int((~known).sum()))
        torch.cuda.synchronize()
        pool.index_sync()
        eng.sync()
        res["index_info_after_build"] = pool.index_info()
        av = eng.aggregate_verifier(n)

        def lookup_ok(share):
            ids, want, _, _, _, u = inputs[share]
            return bool((d_places == want).all()) and int(d_count.item()) == u

        def verify(share, with_lookup):
            ids, want, u_rs, u_wire, u_msgs, u = inputs[share]
            if with_lookup:
                pool.lookup_device(ids, d_places, d_count)
            av.reset()
            av.push_mixed_wire_device(pool, d_places if with_lookup else want, d_res, u_rs if u else None,
                                      u_wire if u else None, u_msgs if u else None, cache=kc, require=2, want_stats=False)
            av.finish_device(d_e, d_v)

        par.cached_wire_finish(b_rs, b_wire, b_msgs, d_e, d_vp)
        par.sync()
        want_v = int(d_vp.item())
        res["parent_verdict"] = want_v
        verdict_ok = lambda: int(d_v.item()) == want_v and int(d_res.item()) == 0   # noqa: E731

        def increment_prepare():
            fill(pool, n - inc)
            pool.index_sync()
            fill(pool, n, n - inc, reset=False)

        d_sel = torch.zeros(32 * n, dtype=torch.uint8, device=dev)
        legs = {"sync_stale": (lambda: fill(pool), pool.index_sync, eng.sync, None),
                "sync_increment": (increment_prepare, pool.index_sync, eng.sync, None)}
        for s in LOOKUP_SHARES:
            legs["lookup_%d" % s] = (None, lambda s=s: pool.lookup_device(inputs[s][0], d_places, d_count), eng.sync,
                                     lambda s=s: lookup_ok(s))
        legs["leaves_select"] = (None, lambda: pool.leaves_select_device(d_block, d_sel, d_res), eng.sync,
                                 lambda: bool((d_sel == d_ids).all()) and int(d_res.item()) == 0)
        for s in CHAIN_SHARES:
            legs["chain_%d" % s] = (None, lambda s=s: verify(s, True), eng.sync, lambda s=s: verdict_ok() and lookup_ok(s))
            legs["places_%d" % s] = (None, lambda s=s: verify(s, False), eng.sync, verdict_ok)
        legs["parent_cached"] = (None, lambda: par.cached_wire_finish(b_rs, b_wire, b_msgs, d_e, d_vp), par.sync,
                                 lambda: int(d_vp.item()) == want_v)
        times = run_legs(legs)
        res.update(_summary(times))
        med = res["ms_median"]
        res["lookup_adds_ms"] = {str(s): round(med["chain_%d" % s] - med["places_%d" % s], 3) for s in CHAIN_SHARES}
        res["ratio"] = {"chain_%d/parent_cached" % s: round(med["chain_%d" % s] / med["parent_cached"], 4) for s in CHAIN_SHARES}
        res["bar_high_shares_met"] = all(max(times["chain_%d" % s]) < min(times["parent_cached"]) for s in CHAIN_SHARES if s >= 90)
        # per-kernel times, in a run of its own: a rebuild, an increment, one lookup per share, one gather
        kern = {}
        eng.enable_timing(True)

        def kernel_times(name, prepare, call):
            if prepare:
                prepare()
            eng.sync()
            for kn in KERNELS:
                eng.read_timing(kn)
            call()
            eng.sync()
            kern[name] = {kn: [round(v[0], 4), int(v[1])] for kn in KERNELS for v in [eng.read_timing(kn)] if v[1]}
        kernel_times("sync_stale", lambda: fill(pool), pool.index_sync)
        kernel_times("sync_increment", increment_prepare, pool.index_sync)
        for s in LOOKUP_SHARES:
            kernel_times("lookup_%d" % s, None, lambda s=s: pool.lookup_device(inputs[s][0], d_places, d_count))
        kernel_times("leaves_select", None, lambda: pool.leaves_select_device(d_block, d_sel, d_res))
        eng.enable_timing(False)
        res["kernel_ms_avg_launches"] = kern
        res["index_info_at_end"] = pool.index_info()
        handles = (av, pool, kc)
    print(json.dumps(res))
    for h in handles:
        h.close()
    eng.close()
    par.close()
    return 0 if res["mismatches"] == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
