#!/usr/bin/env python3
"""A block against the pool (push_mixed), measured on one GPU.

    python tools/aggverifier_mixed_bench.py --baseline-lib /path/to/parent/libschnorr_sig_amd.so [--n 1048576]
                                            [--signers 65536] [--rounds 3] [--warmup 1]

--n honest signatures by --signers signers over 80-byte messages are held by a streaming aggregator (screened pushes);
the block is a random permutation of them.  --baseline-lib is a build of the parent commit (without it this tree's own
library stands in, and the comparison says nothing).  The legs alternate in one process; each timed call has an untimed
call of the same kind in front of it in every round, starts behind a stream synchronisation and ends with one; the
medians and all samples are printed as one JSON line.

  mixed_<share>   reset, push_mixed_device + finish_device of this tree with <share> percent of the block's lanes known
                  (100, 99, 90, 50, 0), the unknown lanes' R's, keys and messages gathered in device memory beforehand
  parent          reset, push_device + finish_device of the baseline library on the whole body

Bars, both relative to the parent in the same run:
  shares >= 90    every sample of the new pair is below every sample of the parent's pair
  share 0         the new pair's median lies within the parent's maximum plus the measured time of the classify and rank
                  launches (agv_k_classify, av_k_keep, agv_k_mixed_close; ssa_ctx_read_timing in a run of its own)
The 50 % leg and the crossover share (linear between the measured shares) are reported, not judged.  After every timed
call the verdict is compared with the parent's on the same block and scalar; one untimed pass checks e_agg + 1.

Two more sets of legs, each behind an option of its own (without them the run is the one above):

  --cached      the pool holds its lanes by push_keyed_device through a wire cache and records their admission classes;
                cached_<share>: reset, push_mixed_wire_device(require = 2) + finish_device of this tree, the wire cache
                warm; parent_cached: reset, push_cached_wire_device + finish_device of the baseline library on the whole
                body, its own wire cache warm -- the only way the parent reaches the same verdict.  The bar is an
                ordering: at shares >= 90 every sample of the new pair lies below every sample of the parent's pair.
  --unchanged   the paths this tree must not have changed, against the baseline library: mixed_90 / parent_mixed_90
                (push_mixed_device + finish_device at 90 % known), and on a pool of n lanes filled again in front of
                every call drop_front(n / 2 + 1) and a random-half remove_device -- of the baseline, of this tree
                without the admission column, and of this tree with it.  The bar: the tree's median lies inside the
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
SHARES = (100, 99, 90, 50, 0)
KERNELS = ("agv_k_classify", "av_k_keep", "ag_k_expand", "ssa_k_hash", "agv_k_append_at", "agv_k_append", "agv_k_mixed_close",
           "ag_k_tree", "agv_k_scalars_at", "agv_k_scalars", "agv_k_known_fold", "ag_k_fold_finish", "agv_k_known_close",
           "ag_k_finish")
EXTRA = ("agv_k_classify", "av_k_keep", "agv_k_mixed_close")


def _scalars(rng, n):
    s = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    s[:, 31] &= 0x3F
    s[:, 0] |= 1
    return s


class Parent:
    """the streaming aggregate verifier and the one-shot producer of a build of the library given by its path, on a
    context of its own"""

    def __init__(self, path, capacity):
        vp, sz, i32, u32 = C.c_void_p, C.c_size_t, C.c_int, C.c_uint32
        lib = self.lib = C.CDLL(path)
        lib.ssa_ctx_create_ex.argtypes = [C.POINTER(vp), i32, vp, sz, u32, C.c_uint64]
        lib.ssa_aggregate_many_device.argtypes = [vp, vp, vp, vp, vp, vp, sz, sz, sz, u32, vp, vp, vp]
        lib.ssa_aggverifier_create.argtypes = [vp, sz, sz, u32, C.POINTER(vp)]
        lib.ssa_aggverifier_push_device.argtypes = [vp, vp, vp, vp, vp, vp, vp, sz, sz, sz]
        lib.ssa_aggverifier_finish_device.argtypes = [vp, vp, vp, sz, vp]
        lib.ssa_aggverifier_reset.argtypes = [vp]
        lib.ssa_aggverifier_destroy.argtypes, lib.ssa_aggverifier_destroy.restype = [vp], None
        lib.ssa_ctx_destroy.argtypes, lib.ssa_ctx_destroy.restype = [vp], None
        lib.ssa_ctx_sync.argtypes = [vp]
        self.ctx, self.av = vp(), vp()
        if lib.ssa_ctx_create_ex(C.byref(self.ctx), 0, None, 0, 0, 0) != 0:
            raise RuntimeError("baseline library: ssa_ctx_create_ex failed")
        if lib.ssa_aggverifier_create(self.ctx, capacity, 0, 0, C.byref(self.av)) != 0:
            raise RuntimeError("baseline library: ssa_aggverifier_create failed")

    def aggregate(self, d_sigs, d_pks, d_msgs, d_agg):
        rc = self.lib.ssa_aggregate_many_device(self.ctx, d_sigs.data_ptr(), d_pks.data_ptr(), None, d_msgs.data_ptr(), None,
                                                80, 80, int(d_pks.shape[0]), 0, d_agg.data_ptr(), None, None)
        if rc != 0:
            raise RuntimeError("baseline library: ssa_aggregate_many_device gave %d" % rc)

    def push_finish(self, d_rs, d_pks, d_msgs, d_e, d_verdict):
        n = int(d_pks.shape[0])
        rc = self.lib.ssa_aggverifier_reset(self.av)
        rc = rc or self.lib.ssa_aggverifier_push_device(self.ctx, self.av, d_rs.data_ptr(), d_pks.data_ptr(), None,
                                                        d_msgs.data_ptr(), None, 80, 80, n)
        rc = rc or self.lib.ssa_aggverifier_finish_device(self.ctx, self.av, d_e.data_ptr(), n, d_verdict.data_ptr())
        if rc != 0:
            raise RuntimeError("baseline library: push_device + finish_device gave %d" % rc)

    def sync(self):
        self.lib.ssa_ctx_sync(self.ctx)

    def close(self):
        self.lib.ssa_aggverifier_destroy(self.av)
        self.lib.ssa_ctx_destroy(self.ctx)


class ParentPool(Parent):
    """the rest of the baseline library that the legs of section 35 call: a streaming aggregator, a wire key cache, the
    mixed push and the cached wire push"""

    def __init__(self, path, capacity):
        super().__init__(path, capacity)
        vp, sz, i32, u32, lib = C.c_void_p, C.c_size_t, C.c_int, C.c_uint32, self.lib
        lib.ssa_aggregator_create.argtypes = [vp, sz, sz, u32, C.POINTER(vp)]
        lib.ssa_aggregator_push_device.argtypes = [vp, vp, vp, vp, vp, vp, vp, sz, sz, sz, u32, vp, vp]
        lib.ssa_aggregator_reset.argtypes = [vp]
        lib.ssa_aggregator_drop_front.argtypes = [vp, vp, sz]
        lib.ssa_aggregator_remove_device.argtypes = [vp, vp, vp, sz, vp]
        lib.ssa_aggregator_destroy.argtypes, lib.ssa_aggregator_destroy.restype = [vp], None
        lib.ssa_keycache_create_ex.argtypes = [vp, sz, u32, C.POINTER(vp)]
        lib.ssa_keycache_destroy.argtypes, lib.ssa_keycache_destroy.restype = [vp], None
        lib.ssa_aggverifier_push_mixed_device.argtypes = [vp, vp, vp, vp, sz, vp, vp, vp, vp, vp, sz, sz, sz, vp]
        lib.ssa_aggverifier_push_cached_wire_device.argtypes = [vp, vp, vp, vp, vp, vp, vp, sz, sz, sz, vp]
        self.ag, self.kc, self.capacity = vp(), vp(), capacity
        if lib.ssa_aggregator_create(self.ctx, capacity, 0, 0, C.byref(self.ag)) != 0:
            raise RuntimeError("baseline library: ssa_aggregator_create failed")
        if lib.ssa_keycache_create_ex(self.ctx, min(2 * capacity, 1 << 18), 1, C.byref(self.kc)) != 0:
            raise RuntimeError("baseline library: ssa_keycache_create_ex failed")

    def fill(self, d_sigs, d_pks, d_msgs, step, screen):
        """the pool emptied and filled again with every lane, in pushes of at most `step` lanes"""
        n, kept = int(d_pks.shape[0]), C.c_uint64(0)
        rc = self.lib.ssa_aggregator_reset(self.ag)
        for lo in range(0, n, step):
            cnt = min(step, n - lo)
            rc = rc or self.lib.ssa_aggregator_push_device(self.ctx, self.ag, d_sigs[lo:lo + cnt].data_ptr(),
                                                           d_pks[lo:lo + cnt].data_ptr(), None, d_msgs[lo:lo + cnt].data_ptr(),
                                                           None, 80, 80, cnt, 0 if screen else 1, None, C.byref(kept))
            if rc != 0 or kept.value != cnt:
                raise RuntimeError("baseline library: ssa_aggregator_push_device gave %d, kept %d" % (rc, kept.value))

    def drop_front(self, k):
        if self.lib.ssa_aggregator_drop_front(self.ctx, self.ag, k) != 0:
            raise RuntimeError("baseline library: ssa_aggregator_drop_front failed")

    def remove(self, d_mask):
        kept = C.c_uint64(0)
        if self.lib.ssa_aggregator_remove_device(self.ctx, self.ag, d_mask.data_ptr(), int(d_mask.numel()), C.byref(kept)) != 0:
            raise RuntimeError("baseline library: ssa_aggregator_remove_device failed")
        return int(kept.value)

    def mixed_finish(self, d_places, u_rs, u_pks, u_msgs, d_res, d_e, d_verdict):
        n = int(d_places.numel())
        rc = self.lib.ssa_aggverifier_reset(self.av)
        rc = rc or self.lib.ssa_aggverifier_push_mixed_device(self.ctx, self.av, self.ag, d_places.data_ptr(), n,
                                                              u_rs.data_ptr(), u_pks.data_ptr(), None, u_msgs.data_ptr(), None,
                                                              80, 80, int(u_pks.shape[0]), d_res.data_ptr())
        rc = rc or self.lib.ssa_aggverifier_finish_device(self.ctx, self.av, d_e.data_ptr(), n, d_verdict.data_ptr())
        if rc != 0:
            raise RuntimeError("baseline library: push_mixed_device + finish_device gave %d" % rc)

    def cached_wire_finish(self, d_rs, d_wire, d_msgs, d_e, d_verdict):
        n = int(d_wire.shape[0])
        rc = self.lib.ssa_aggverifier_reset(self.av)
        rc = rc or self.lib.ssa_aggverifier_push_cached_wire_device(self.ctx, self.av, self.kc, d_rs.data_ptr(),
                                                                    d_wire.data_ptr(), d_msgs.data_ptr(), None, 80, 80, n, None)
        rc = rc or self.lib.ssa_aggverifier_finish_device(self.ctx, self.av, d_e.data_ptr(), n, d_verdict.data_ptr())
        if rc != 0:
            raise RuntimeError("baseline library: push_cached_wire_device + finish_device gave %d" % rc)

    def close(self):
        self.lib.ssa_aggregator_destroy(self.ag)
        self.lib.ssa_keycache_destroy(self.kc)
        super().close()


CACHED_KERNELS = KERNELS + ("agv_k_classify_adm", "agv_k_kst_at", "agc_expand", "agv_k_key_verdict", "ssa_k_keyed_decompress",
                            "ssa_k_keyset_build")


def _summary(times):
    return {"ms_median": {k: round(float(np.median(v)), 3) for k, v in times.items()},
            "ms_min": {k: round(float(np.min(v)), 3) for k, v in times.items()},
            "ms_max": {k: round(float(np.max(v)), 3) for k, v in times.items()},
            "ms_all": {k: [round(x, 3) for x in v] for k, v in times.items()}}


def main_section35(a):
    """the legs behind --cached and --unchanged"""
    import torch
    import schnorr_sig_amd as ssa
    dev = torch.device("cuda", 0)
    n, signers = a.n, min(a.signers, a.n)
    eng = ssa.Engine(0)
    base_path = a.baseline_lib or ssa.LIB_PATH
    par = ParentPool(base_path, n)
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
    step = min(n, int(eng.info()["msm_slice"]))
    block = rng.permutation(n)
    d_block = t(block)
    b_sigs, b_pks, b_msgs, b_wire = (x[d_block].contiguous() for x in (d_sigs, d_pks, d_msgs, d_wire))
    b_rs = b_sigs[:, :49].contiguous()
    d_agg = torch.zeros(49 * n + 32, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()      # the gathers ran on torch's stream, the library reads on its own
    par.aggregate(b_sigs, b_pks, b_msgs, d_agg)
    par.sync()
    d_e = d_agg[49 * n:].clone()
    e_bad = d_e.cpu().numpy().copy()
    e_bad[0] ^= 1
    d_e_bad = t(e_bad)
    d_res = torch.zeros(1, dtype=torch.int32, device=dev)
    d_v = torch.full((1,), 77, dtype=torch.int32, device=dev)
    d_vp = torch.full((1,), 77, dtype=torch.int32, device=dev)
    sha = lambda path: hashlib.sha256(open(path, "rb").read()).hexdigest()[:16]   # noqa: E731
    res = {"metric": "aggverifier_mixed_cached" if a.cached else "aggverifier_unchanged_paths", "n": n, "signers": signers,
           "msg_len": 80, "rounds": a.rounds, "warmup": a.warmup, "library_sha256": sha(ssa.LIB_PATH),
           "baseline_sha256": sha(base_path), "baseline_is_this_tree": not a.baseline_lib,
           "device": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d"), "mismatches": 0}

    def share_inputs(share, keys):
        known = np.zeros(n, bool)
        known[rng.choice(n, (n * share) // 100, replace=False)] = True
        places = np.where(known, block, 0xFFFFFFFF).astype(np.uint32)
        d_unk = t(np.flatnonzero(~known))
        return (t(places.view(np.int32)), b_rs[d_unk].contiguous(), keys[d_unk].contiguous(), b_msgs[d_unk].contiguous(),
                int((~known).sum()))

    def run_legs(legs, want):
        """alternating legs, an untimed call in front of every timed one; leg -> (call, sync, verdict word or None)"""
        times = {leg: [] for leg in legs}
        for rnd in range(a.warmup + a.rounds):
            for leg, (call, sync, word) in legs.items():
                ms = 0.0
                for timed in (False, True):
                    if word is not None:
                        word.fill_(77)
                    eng.sync()
                    par.sync()
                    torch.cuda.synchronize()
                    ms = call()
                    if ms is None:
                        t0 = time.perf_counter()
                        sync()
                        ms = (time.perf_counter() - t0) * 1e3
                if word is not None:
                    ok = int(word.item()) == want and (word is d_vp or int(d_res.item()) == 0)
                    res["mismatches"] += 0 if ok else 1
                if rnd >= a.warmup:
                    times[leg].append(ms)
        return times

    def timed(call, sync):
        """a leg whose clock starts in front of the call: the ordinary case"""
        def run():
            t0 = time.perf_counter()
            call()
            sync()
            return (time.perf_counter() - t0) * 1e3
        return run

    if a.cached:
        kc = eng.keycache_create(min(2 * n, 1 << 18), wire=True)
        pool = eng.aggregator(n, hold_admission=True)
        d_keyed = torch.cat([d_wire, d_sigs], dim=1).contiguous()
        torch.cuda.synchronize()
        for lo in range(0, n, step):
            kept, _ = pool.push_keyed_device(kc, d_keyed[lo:lo + step], d_msgs[lo:lo + step], want_stats=False)
            assert kept == min(step, n - lo)
        d_adm = torch.zeros(n, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        pool.admission_device(d_adm)
        eng.sync()
        assert bool((d_adm == 2).all())
        inputs = {share: share_inputs(share, b_wire) for share in SHARES}
        torch.cuda.synchronize()
        av = eng.aggregate_verifier(n)

        def cached(share, e=None):
            d_places, u_rs, u_wire, u_msgs, u = inputs[share]
            av.reset()
            av.push_mixed_wire_device(pool, d_places, d_res, u_rs if u else None, u_wire if u else None, u_msgs if u else None,
                                      cache=kc, require=2, want_stats=False)
            av.finish_device(d_e if e is None else e, d_v)

        want = {}
        for name, e in (("honest", d_e), ("e_agg + 1", d_e_bad)):      # the parent's cached verdicts: the expected values
            par.cached_wire_finish(b_rs, b_wire, b_msgs, e, d_vp)
            par.sync()
            want[name] = int(d_vp.item())
        res["parent_verdicts"] = want
        for share in SHARES:                      # untimed: the refused scalar
            cached(share, d_e_bad)
            eng.sync()
            res["mismatches"] += 0 if int(d_v.item()) == want["e_agg + 1"] and int(d_res.item()) == 0 else 1
        legs = {"cached_%d" % s: (timed(lambda s=s: cached(s), eng.sync), None, d_v) for s in SHARES}
        legs["parent_cached"] = (timed(lambda: par.cached_wire_finish(b_rs, b_wire, b_msgs, d_e, d_vp), par.sync), None, d_vp)
        times = run_legs(legs, want["honest"])
        res.update(_summary(times))
        med = res["ms_median"]
        res["ratio"] = {"cached_%d/parent_cached" % s: round(med["cached_%d" % s] / med["parent_cached"], 4) for s in SHARES}
        kern = {}
        for share in SHARES:                      # per-kernel times of one pair per share, in a run of its own
            eng.sync()
            eng.enable_timing(True)
            for kn in CACHED_KERNELS:
                eng.read_timing(kn)
            cached(share)
            eng.sync()
            kern[share] = {}
            for kn in CACHED_KERNELS:
                avg, cnt = eng.read_timing(kn)
                if cnt:
                    kern[share][kn] = [round(avg, 4), int(cnt)]
            eng.enable_timing(False)
        res["kernel_ms_avg_launches"] = {str(k): v for k, v in kern.items()}
        res["bar_high_shares_met"] = all(max(times["cached_%d" % s]) < min(times["parent_cached"]) for s in SHARES if s >= 90)
        cross = None
        pts = sorted((s, med["cached_%d" % s]) for s in SHARES)
        for (s0, m0), (s1, m1) in zip(pts, pts[1:]):
            if (m0 - med["parent_cached"]) * (m1 - med["parent_cached"]) <= 0 and m0 != m1:
                cross = round(s0 + (s1 - s0) * (m0 - med["parent_cached"]) / (m0 - m1), 1)
        res["crossover_share_percent"] = cross
        handles = (av, pool, kc)
    else:
        plain, flagged = eng.aggregator(n), eng.aggregator(n, hold_admission=True)
        fill = lambda ag: [ag.reset()] + [ag.push_device(d_sigs[lo:lo + step], d_pks[lo:lo + step], d_msgs[lo:lo + step],   # noqa: E731
                                                         screen=False) for lo in range(0, n, step)]
        fill(plain)
        par.fill(d_sigs, d_pks, d_msgs, step, False)
        inp = share_inputs(90, b_pks)
        torch.cuda.synchronize()
        av = eng.aggregate_verifier(n)

        def mixed():
            av.reset()
            av.push_mixed_device(plain, inp[0], d_res, inp[1], inp[2], inp[3])
            av.finish_device(d_e, d_v)

        par.mixed_finish(inp[0], inp[1], inp[2], inp[3], d_res, d_e, d_vp)
        par.sync()
        want = int(d_vp.item())
        res["parent_verdicts"] = {"honest": want}
        legs = {"mixed_90": (timed(mixed, eng.sync), None, d_v),
                "parent_mixed_90": (timed(lambda: par.mixed_finish(inp[0], inp[1], inp[2], inp[3], d_res, d_e, d_vp), par.sync),
                                    None, d_vp)}
        times = run_legs(legs, want)
        # the moves: the pool is filled again in front of every call, outside the clock
        d_mask = t((rng.integers(0, 2, n) == 1).astype(np.uint8))
        torch.cuda.synchronize()
        half = n // 2 + 1

        def move(fill_it, op, sync):
            def run():
                fill_it()
                eng.sync()
                par.sync()
                t0 = time.perf_counter()
                op()
                sync()
                return (time.perf_counter() - t0) * 1e3
            return run
        p_fill = lambda: par.fill(d_sigs, d_pks, d_msgs, step, False)   # noqa: E731
        moves = {"parent_drop_front": (move(p_fill, lambda: par.drop_front(half), par.sync), None, None),
                 "drop_front": (move(lambda: fill(plain), lambda: plain.drop_front(half), eng.sync), None, None),
                 "drop_front_with_column": (move(lambda: fill(flagged), lambda: flagged.drop_front(half), eng.sync), None, None),
                 "parent_remove": (move(p_fill, lambda: par.remove(d_mask), par.sync), None, None),
                 "remove": (move(lambda: fill(plain), lambda: plain.remove_device(d_mask), eng.sync), None, None),
                 "remove_with_column": (move(lambda: fill(flagged), lambda: flagged.remove_device(d_mask), eng.sync), None, None)}
        times.update(run_legs(moves, None))
        # what is left after the moves is the same aggregate, byte for byte, with and without the column
        kept = [ag.info()["held"] for ag in (plain, flagged)]
        res["moves_kept"] = kept
        res["moves_bytes_equal"] = bool(kept[0] == kept[1] and (plain.finish_bytes() == flagged.finish_bytes()).all())
        res["mismatches"] += 0 if res["moves_bytes_equal"] else 1
        res.update(_summary(times))
        med = res["ms_median"]
        pairs = (("mixed_90", "parent_mixed_90"), ("drop_front", "parent_drop_front"), ("remove", "parent_remove"))
        res["bar_inside_parent_range"] = {k: bool(min(times[p]) <= med[k] <= max(times[p])) for k, p in pairs}
        res["column_cost_ms"] = {"drop_front": round(med["drop_front_with_column"] - med["drop_front"], 3),
                                 "remove": round(med["remove_with_column"] - med["remove"], 3)}
        handles = (av, plain, flagged)
    print(json.dumps(res))
    for h in handles:
        h.close()
    eng.close()
    par.close()
    return 0 if res["mismatches"] == 0 else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--signers", type=int, default=65536)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seed", type=int, default=0x34B)
    ap.add_argument("--baseline-lib", default=None, help="a build of the parent commit's library")
    ap.add_argument("--cached", action="store_true", help="the legs through the key cache with require = 2 (section 35)")
    ap.add_argument("--unchanged", action="store_true", help="the unchanged paths against the baseline (section 35)")
    a = ap.parse_args()
    if a.cached and a.unchanged:
        ap.error("--cached and --unchanged are runs of their own")
    if a.cached or a.unchanged:
        return main_section35(a)
    import torch
    import schnorr_sig_amd as ssa
    dev = torch.device("cuda", 0)
    n, signers = a.n, min(a.signers, a.n)
    eng = ssa.Engine(0)
    base_path = a.baseline_lib or ssa.LIB_PATH
    par = Parent(base_path, n)
    rng = np.random.default_rng(a.seed)
    msgs = rng.integers(0, 256, (n, 80), dtype=np.uint8)
    idx = rng.integers(0, signers, size=n)
    idx[:signers] = np.arange(signers)
    rng.shuffle(idx)
    pks, sigs = eng.keygen_sign_many(_scalars(rng, signers)[idx], _scalars(rng, n), msgs)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)   # noqa: E731
    d_sigs, d_pks, d_msgs = t(sigs), t(pks), t(msgs)
    # the pool: every lane, in arrival order, by screened pushes of at most one MSM slice
    pool = eng.aggregator(n)
    step = min(n, int(eng.info()["msm_slice"]))
    for lo in range(0, n, step):
        kept = pool.push_device(d_sigs[lo:lo + step], d_pks[lo:lo + step], d_msgs[lo:lo + step])
        assert kept == min(step, n - lo)
    # the block: a random permutation of the pool's lanes; place of block lane i in the pool: block[i]
    block = rng.permutation(n)
    d_block = t(block)
    b_sigs, b_pks, b_msgs = (x[d_block].contiguous() for x in (d_sigs, d_pks, d_msgs))
    b_rs = b_sigs[:, :49].contiguous()
    d_agg = torch.zeros(49 * n + 32, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()      # the gathers ran on torch's stream, the library reads on its own
    par.aggregate(b_sigs, b_pks, b_msgs, d_agg)
    par.sync()
    d_e = d_agg[49 * n:].clone()
    e_bad = d_e.cpu().numpy().copy()
    e_bad[0] ^= 1
    d_e_bad = t(e_bad)
    inputs = {}
    for share in SHARES:
        known = np.zeros(n, bool)
        known[rng.choice(n, (n * share) // 100, replace=False)] = True
        places = np.where(known, block, 0xFFFFFFFF).astype(np.uint32)
        d_unk = t(np.flatnonzero(~known))
        inputs[share] = (t(places.view(np.int32)), b_rs[d_unk].contiguous(), b_pks[d_unk].contiguous(),
                         b_msgs[d_unk].contiguous(), int((~known).sum()))
    torch.cuda.synchronize()
    av = eng.aggregate_verifier(n)
    d_res = torch.zeros(1, dtype=torch.int32, device=dev)
    d_v = torch.full((1,), 77, dtype=torch.int32, device=dev)
    d_vp = torch.full((1,), 77, dtype=torch.int32, device=dev)

    def mixed(share, e=None):
        d_places, u_rs, u_pks, u_msgs, u = inputs[share]
        av.reset()
        if u:
            av.push_mixed_device(pool, d_places, d_res, u_rs, u_pks, u_msgs)
        else:
            av.push_known_device(pool, d_places, d_res)
        av.finish_device(d_e if e is None else e, d_v)

    sha = lambda path: hashlib.sha256(open(path, "rb").read()).hexdigest()[:16]   # noqa: E731
    res = {"metric": "aggverifier_mixed", "n": n, "signers": signers, "msg_len": 80, "rounds": a.rounds, "warmup": a.warmup,
           "library_sha256": sha(ssa.LIB_PATH), "baseline_sha256": sha(base_path), "baseline_is_this_tree": not a.baseline_lib,
           "device": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d"), "mismatches": 0}
    # the parent's verdicts on the block: the expected values
    want = {}
    for name, e in (("honest", d_e), ("e_agg + 1", d_e_bad)):
        par.push_finish(b_rs, b_pks, b_msgs, e, d_vp)
        par.sync()
        want[name] = int(d_vp.item())
    res["parent_verdicts"] = want
    for share in SHARES:                      # untimed: the refused scalar
        mixed(share, d_e_bad)
        eng.sync()
        res["mismatches"] += 0 if int(d_v.item()) == want["e_agg + 1"] and int(d_res.item()) == 0 else 1
    legs = {"mixed_%d" % s: (lambda s=s: mixed(s), eng.sync, d_v) for s in SHARES}
    legs["parent"] = (lambda: par.push_finish(b_rs, b_pks, b_msgs, d_e, d_vp), par.sync, d_vp)
    times = {leg: [] for leg in legs}
    for rnd in range(a.warmup + a.rounds):
        for leg, (call, sync, word) in legs.items():
            ms = 0.0
            for timed in (False, True):
                word.fill_(77)
                eng.sync()
                par.sync()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                call()
                sync()
                ms = (time.perf_counter() - t0) * 1e3
            ok = int(word.item()) == want["honest"] and (leg == "parent" or int(d_res.item()) == 0)
            res["mismatches"] += 0 if ok else 1
            if rnd >= a.warmup:
                times[leg].append(ms)
    med = res["ms_median"] = {leg: round(float(np.median(v)), 3) for leg, v in times.items()}
    res["ms_min"] = {leg: round(float(np.min(v)), 3) for leg, v in times.items()}
    res["ms_max"] = {leg: round(float(np.max(v)), 3) for leg, v in times.items()}
    res["ms_all"] = {leg: [round(x, 3) for x in v] for leg, v in times.items()}
    res["ratio"] = {"mixed_%d/parent" % s: round(med["mixed_%d" % s] / med["parent"], 4) for s in SHARES}
    # per-kernel times of one pair per share, in a run of its own
    kern = {}
    for share in SHARES:
        eng.sync()
        eng.enable_timing(True)
        for kn in KERNELS:
            eng.read_timing(kn)
        mixed(share)
        eng.sync()
        kern[share] = {}
        for kn in KERNELS:
            avg, cnt = eng.read_timing(kn)
            if cnt:
                kern[share][kn] = [round(avg, 4), int(cnt)]
        eng.enable_timing(False)
    res["kernel_ms_avg_launches"] = {str(k): v for k, v in kern.items()}
    extra = sum(kern[0][kn][0] * kern[0][kn][1] for kn in EXTRA if kn in kern[0])
    res["classify_and_rank_ms_at_share_0"] = round(extra, 4)
    res["bar_high_shares_met"] = all(max(times["mixed_%d" % s]) < min(times["parent"]) for s in SHARES if s >= 90)
    res["bar_share_0_met"] = med["mixed_0"] <= max(times["parent"]) + extra
    # where the new pair costs what the parent's does, linear between the two measured shares around it
    cross = None
    pts = sorted((s, med["mixed_%d" % s]) for s in SHARES)
    for (s0, m0), (s1, m1) in zip(pts, pts[1:]):
        if (m0 - med["parent"]) * (m1 - med["parent"]) <= 0 and m0 != m1:
            cross = round(s0 + (s1 - s0) * (m0 - med["parent"]) / (m0 - m1), 1)
    res["crossover_share_percent"] = cross
    print(json.dumps(res))
    for h in (av, pool):
        h.close()
    eng.close()
    par.close()
    return 0 if res["mismatches"] == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
