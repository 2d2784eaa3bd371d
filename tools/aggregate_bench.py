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
lane; leaf, node and coefficient: about one each).  One JSON line out.

--many KxS (repeatable) measures ssa_verify_aggregates_many_device instead: K aggregates of S
signatures each, cut out of one pool of signatures.  Legs, alternating in the same way, every verdict vector checked:
  many            one call for all K aggregates, the context's own choice of path per group
  many_small      the same call on a context created under SSA_MSM_SMALL_MAX = 2^40 (every group: small path)
  many_bucket     ... under SSA_MSM_SMALL_MAX = 0 (every group: bucket path)
  loop            K calls of ssa_verify_aggregate_device on this tree's library
  loop_baseline   the same K calls through the library given by --baseline-lib (another build, e.g. the parent commit's)
and, once, `single`: the whole pool as ONE aggregate through ssa_verify_aggregate_device.

--valid measures ssa_aggregate_valid_many_device against the only route there was before it, run
through the library given by --baseline-lib (a build of the parent commit; without it, this tree's own library).  Three
workloads of --n signatures: an honest batch, 16 bad lanes, 1 % bad lanes (a flipped bit of e, at random places).  Legs,
alternating in the same way, every timed output checked:
  valid                      the new call: the aggregate of the lanes that verify, and their list
  baseline_checked           ssa_aggregate_many_device with SSA_AGG_CHECK on the whole batch: the aggregate of an honest
                             batch, a refusal of any other
  baseline_filtered          ssa_aggregate_many_device without the check on arrays filtered beforehand (bad lanes only;
                             the time the caller needs to filter is NOT counted)
The bar: valid < baseline_checked on the honest batch, valid < baseline_checked + baseline_filtered on the others.

--cached measures ssa_verify_aggregates_many_cached(_wire)_device on section 21's first workload,
--many's first KxS (default 1024x1024), signed by --signers distinct signers (0: every lane its own).  The validator's keys
arrive as 49 wire bytes.  Legs, alternating in the same way, every verdict vector checked:
  wire_cold                 the wire call on a cache cleared in front of it (the clear is not timed)
  wire_warm                 the wire call on a cache that holds every key
  affine_warm               the affine call on affine keys, a warm affine cache
  baseline                  the route there was before, through --baseline-lib (a build of the parent commit; without it
                            this tree's own library): ssa_decompress_many_device + ssa_verify_aggregates_many_device.  No
                            subgroup guarantee.
  baseline_keyset           the same plus ssa_keyset_create_device (ladder tables) over the distinct keys, which gives
                            the statuses of the subgroup check.  The HOST time a caller needs to find the distinct keys
                            and to map the statuses back onto aggregates is NOT counted.

--valid-cached measures ssa_aggregate_valid_many_cached_device and ssa_aggregate_valid_keyed_many_cached_device (DESIGN.md
section 24): --n signatures by --signers distinct signers (0: every lane its own), three workloads -- an honest batch, 16
bad lanes (a flipped bit of e), 1 % bad lanes of which every second one has a key outside the prime-order subgroup.  Legs,
alternating in the same way, every timed output checked (kept count and list, aggregate, kept keys):
  affine_cold, affine_warm   the affine form on a cache cleared in front of it (the clear is not timed) / that holds every key
  keyed_cold, keyed_warm     the keyed form (130-byte records) through a wire cache, likewise
  baseline_valid             ssa_aggregate_valid_many_device through --baseline-lib (a build of the parent commit; without it
                             this tree's own library): NO guarantee about the keys
  baseline_guarded           the guarded route there was before, through the same library: ssa_verify_many_cached_device
                             (warm affine cache, subgroup check and flag byte), then ssa_aggregate_many_device on arrays
                             filtered beforehand.  The HOST time a caller needs to filter four arrays and upload them again
                             is NOT counted.

--sharded measures the sliced calls against the single calls of --baseline-lib at --n signatures,
device buffers, legs alternating: verify_sliced / verify_baseline, aggregate_sliced / aggregate_baseline, and this tree's own
single calls.  Up to one MSM slice the routes differ in the tree alone (flat ag_k_level launches against ag_k_tree); above
it (n a multiple of 2^20, 2^20 distinct lanes repeated) only the sliced legs run.  --multi adds MultiEngine([0, 0]) from
host buffers beside this tree's host forms: two contexts on ONE device, which says nothing about scaling.

--produce-many [KxS] measures the producer of many aggregates (ssa_aggregates_many_device): K batches
of S signatures (4096 x 256) with 80-byte messages, device buffers, legs alternating in one process:
  many            ONE ssa_aggregates_many_device call over the K x S lanes
  loop_baseline   K ssa_aggregate_many_device calls through --baseline-lib (a build of the parent commit, which has no other
                  way; without it, this tree's own library)
  single          the same lanes as ONE aggregate through this tree's ssa_aggregate_many_device (recorded, no bar)
Every timed output is compared with the aggregates of the single call, batch by batch, made once before the rounds.

--accumulator measures the streaming aggregator: --n honest signatures pushed in --pushes equal
pushes, then ssa_aggregator_finish_device against ssa_aggregate_many_sliced_device of --baseline-lib over the same
signatures, legs alternating; the pushes' own times and ssa_aggregate_valid_many_device at --n are recorded beside it.

--accumulator --remove measures removing lanes in place on an object of --n lanes: drop_front of
half, of half plus one, and remove_device of a random half, against reset + unscreened pushes of the remaining half
through the aggregator of --baseline-lib (accumulator_remove_main).

--verifier measures the streaming aggregate verifier: the R's, keys and messages of --n honest
signatures pushed in --pushes equal pushes, then ssa_aggverifier_finish_device against
ssa_verify_aggregate_sliced_device of --baseline-lib over the same lanes, legs alternating; the pushes' own times, the
kernels of one push and of finish, and finish at 256 and 2048 lanes beside ssa_verify_aggregate_device are recorded.

--verifier --cached measures the same object through the key cache: the lanes by --signers
signers pushed with 49-byte wire keys through a wire cache, the keyed finish against the plain verifier's finish of
--baseline-lib over the same lanes, and the sum of the pushes (cold, warm) beside ssa_decompress_many_device + the plain
push of --baseline-lib (verifier_cached_main).
"""
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


MANY_KERNELS = ("ag_k_expand_many", "ssa_k_hash", "ag_k_leaf", "ag_k_tree", "ag_k_coeff", "msm_k_small",
                "msm_k_sum_records_seg", "ag_k_gather", "msm_k_prepare", "msm_sort", "msm_k_buckets", "msm_reduce",
                "msm_k_finish_seg", "ag_k_finish")


class BaselineLoop:
    """ssa_verify_aggregate_device of ANOTHER build of the library, loaded beside this tree's in the same process"""

    def __init__(self, path):
        import ctypes as C
        self.C, self.lib = C, C.CDLL(path)
        vp, sz, i32 = C.c_void_p, C.c_size_t, C.c_int
        self.lib.ssa_ctx_create_ex.argtypes = [C.POINTER(vp), i32, vp, sz, C.c_uint32, C.c_uint64]
        self.lib.ssa_verify_aggregate_device.argtypes = [vp, vp, vp, vp, vp, vp, sz, sz, sz, vp]
        self.lib.ssa_ctx_sync.argtypes = [vp]
        self.lib.ssa_ctx_destroy.argtypes = [vp]
        self.lib.ssa_ctx_destroy.restype = None
        self.ctx = vp()
        if self.lib.ssa_ctx_create_ex(C.byref(self.ctx), 0, None, 0, 0, 0) != 0:
            raise RuntimeError("baseline library: ssa_ctx_create_ex failed")

    def verify(self, d_agg, d_pks, d_msgs, n, d_verdict):
        if self.lib.ssa_verify_aggregate_device(self.ctx, d_agg, d_pks, None, d_msgs, None, 80, 80, n, d_verdict) != 0:
            raise RuntimeError("baseline library: ssa_verify_aggregate_device failed")

    def sync(self):
        self.lib.ssa_ctx_sync(self.ctx)

    def close(self):
        self.lib.ssa_ctx_destroy(self.ctx)


def engine_under(small_max):
    import schnorr_sig_amd as ssa
    old = os.environ.get("SSA_MSM_SMALL_MAX")
    os.environ["SSA_MSM_SMALL_MAX"] = str(small_max)
    try:
        return ssa.Engine(0)
    finally:
        if old is None:
            del os.environ["SSA_MSM_SMALL_MAX"]
        else:
            os.environ["SSA_MSM_SMALL_MAX"] = old


def many_main(a):
    import torch
    import schnorr_sig_amd as ssa
    dev = torch.device("cuda", 0)
    shapes = [tuple(int(v) for v in w.lower().split("x")) for w in a.many]
    n = max(k * s for k, s in shapes)
    eng = ssa.Engine(0)
    engs = {"many": eng, "many_small": engine_under(1 << 40), "many_bucket": engine_under(0)}
    base = BaselineLoop(a.baseline_lib) if a.baseline_lib else None
    rng = np.random.default_rng(a.seed)
    msgs = rng.integers(0, 256, (n, 80), dtype=np.uint8)
    pks, sigs = eng.keygen_sign_many(_scalars(rng, n), _scalars(rng, n), msgs)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)   # noqa: E731
    d_sigs, d_pks, d_msgs = t(sigs), t(pks), t(msgs)
    torch.cuda.synchronize()
    res = {"metric": "aggregates_many", "msg_len": 80, "rounds": a.rounds, "warmup": a.warmup,
           "library_sha256": hashlib.sha256(open(ssa.LIB_PATH, "rb").read()).hexdigest()[:16],
           "baseline_sha256": hashlib.sha256(open(a.baseline_lib, "rb").read()).hexdigest()[:16] if base else None,
           "device": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d"), "mismatches": 0, "workloads": []}

    def wall(fn, sync):
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        return (time.perf_counter() - t0) * 1e3

    for k, s in shapes:
        lanes = k * s
        d_wire = torch.zeros(49 * lanes + 32 * k, dtype=torch.uint8, device=dev)
        for j in range(k):        # the honest aggregates, in their wire form end to end
            lo = j * s
            if eng.aggregate_device(d_sigs.data_ptr() + 81 * lo, d_pks.data_ptr() + 96 * lo, d_msgs.data_ptr() + 80 * lo, s, 80,
                                    d_wire.data_ptr() + 49 * lo + 32 * j) != 0:
                res["mismatches"] += 1
        eng.sync()
        counts = [s] * k
        d_v = torch.full((k,), 255, dtype=torch.int32, device=dev)

        def many(e):
            return lambda: e.verify_aggregates_device(d_wire, counts, d_pks[:lanes], d_msgs[:lanes], d_verdicts=d_v)

        def loop(verify):
            def run():
                for j in range(k):
                    lo = j * s
                    verify(d_wire.data_ptr() + 49 * lo + 32 * j, d_pks.data_ptr() + 96 * lo, d_msgs.data_ptr() + 80 * lo, s,
                           d_v.data_ptr() + 4 * j)
            return run

        legs = {name: (many(e), e.sync) for name, e in engs.items()}
        legs["loop"] = (loop(lambda ag, pk, ms, cnt, v: eng.verify_aggregate_device(ag, pk, ms, cnt, 80, v)), eng.sync)
        if base:
            legs["loop_baseline"] = (loop(base.verify), base.sync)
        times = {leg: [] for leg in legs}
        for rnd in range(a.warmup + a.rounds):
            for leg, (fn, sync) in legs.items():
                d_v.fill_(255)
                torch.cuda.synchronize()
                ms = wall(fn, sync)
                if bool((d_v != 0).any()):
                    res["mismatches"] += 1
                if rnd >= a.warmup:
                    times[leg].append(ms)
        w = {"aggregates": k, "signatures_each": s, "plan": {}, "ms_median": {leg: round(float(np.median(v)), 3) for leg, v in times.items()},
             "ms_min": {leg: round(float(np.min(v)), 3) for leg, v in times.items()}}
        pl = ssa.debug_aggregates_plan(counts)
        w["plan"] = {"groups": len(pl["groups"]), "bucket_groups": sum(g["bucket"] for g in pl["groups"]),
                     "tree_passes": len(pl["passes"]),
                     "padded_lanes": sum(g["aggregates"] * g["segment_lanes"] for g in pl["groups"]), "lanes": lanes}
        med = w["ms_median"]
        w["ratio"] = {"loop/many": round(med["loop"] / med["many"], 3)}
        if base:
            w["ratio"]["loop_baseline/many"] = round(med["loop_baseline"] / med["many"], 3)
        w["msigs_per_s"] = {leg: round(lanes / v / 1e3, 3) for leg, v in med.items()}
        kern = {}
        for name in ("many", "many_small", "many_bucket"):
            e = engs[name]
            e.sync()
            e.enable_timing(True)
            many(e)()
            e.sync()
            kern[name] = {}
            for kn in MANY_KERNELS:
                avg, cnt = e.read_timing(kn)
                if cnt:
                    kern[name][kn] = [round(avg, 4), int(cnt)]
            e.enable_timing(False)
        w["kernel_ms_avg_launches"] = kern
        res["workloads"].append(w)
    # the floor: the whole pool as ONE aggregate
    d_one = torch.zeros(49 * n + 32, dtype=torch.uint8, device=dev)
    d_v1 = torch.full((1,), 255, dtype=torch.int32, device=dev)
    if eng.aggregate_device(d_sigs.data_ptr(), d_pks.data_ptr(), d_msgs.data_ptr(), n, 80, d_one.data_ptr()) != 0:
        res["mismatches"] += 1
    one = []
    for rnd in range(a.warmup + a.rounds):
        d_v1.fill_(255)
        torch.cuda.synchronize()
        ms = wall(lambda: eng.verify_aggregate_device(d_one.data_ptr(), d_pks.data_ptr(), d_msgs.data_ptr(), n, 80,
                                                      d_v1.data_ptr()), eng.sync)
        if int(d_v1.item()) != 0:
            res["mismatches"] += 1
        if rnd >= a.warmup:
            one.append(ms)
    res["single"] = {"n": n, "ms_median": round(float(np.median(one)), 3), "ms_min": round(float(np.min(one)), 3)}
    print(json.dumps(res))
    for e in engs.values():
        e.close()
    if base:
        base.close()
    return 0 if res["mismatches"] == 0 else 1


PRODUCE_KERNELS = ("ag_k_lane_map", "ssa_k_hash", "ag_k_leaf", "ag_k_tree", "ag_k_coeff", "ag_k_fold_seg",
                   "ag_k_fold_finish_seg", "ag_k_pack_many", "ag_k_fold")


def produce_many_main(a):
    import torch
    import schnorr_sig_amd as ssa
    dev = torch.device("cuda", 0)
    k, s = (int(v) for v in a.produce_many.lower().split("x"))
    n = k * s
    sha = lambda path: hashlib.sha256(open(path, "rb").read()).hexdigest()[:16]   # noqa: E731
    base_path = a.baseline_lib or ssa.LIB_PATH
    eng = ssa.Engine(0)
    base = BaselineAggregate(base_path)
    rng = np.random.default_rng(a.seed)
    msgs = rng.integers(0, 256, (n, 80), dtype=np.uint8)
    pks, sigs = eng.keygen_sign_many(_scalars(rng, n), _scalars(rng, n), msgs)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)   # noqa: E731
    d_sigs, d_pks, d_msgs = t(sigs), t(pks), t(msgs)
    counts = [s] * k
    wire = 49 * n + 32 * k
    d_ref, d_out = (torch.zeros(wire, dtype=torch.uint8, device=dev) for _ in range(2))
    d_one, d_one0 = (torch.zeros(49 * n + 32, dtype=torch.uint8, device=dev) for _ in range(2))
    d_res = torch.full((k,), 255, dtype=torch.int32, device=dev)
    d_status = torch.zeros(n, dtype=torch.uint8, device=dev)
    d_nfail = torch.zeros(1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    res = {"metric": "aggregates_produce_many", "aggregates": k, "signatures_each": s, "lanes": n, "msg_len": 80,
           "rounds": a.rounds, "warmup": a.warmup, "library_sha256": sha(ssa.LIB_PATH), "baseline_sha256": sha(base_path),
           "baseline_is_this_tree": not a.baseline_lib, "device": torch.cuda.get_device_name(0),
           "date": time.strftime("%Y-%m-%d"), "mismatches": 0}

    def loop(aggregate, out):
        def run():
            for j in range(k):
                lo = j * s
                if aggregate(d_sigs.data_ptr() + 81 * lo, d_pks.data_ptr() + 96 * lo, d_msgs.data_ptr() + 80 * lo, s,
                             out.data_ptr() + 49 * lo + 32 * j) != 0:
                    res["mismatches"] += 1
        return run

    def many():
        eng.aggregates_device(d_sigs, counts, d_pks, d_msgs, d_aggs=d_out, d_results=d_res, d_status=d_status, d_nfail=d_nfail)

    def single(out):
        return lambda: eng.aggregate_device(d_sigs.data_ptr(), d_pks.data_ptr(), d_msgs.data_ptr(), n, 80, out.data_ptr())

    # the reference of every check: this tree's single call, batch by batch; and the N lanes as one aggregate
    loop(lambda sg, pk, ms, cnt, out: eng.aggregate_device(sg, pk, ms, cnt, 80, out), d_ref)()
    single_ok = n <= eng.info()["msm_slice"]
    if single_ok and single(d_one0)() != 0:
        res["mismatches"] += 1
    eng.sync()

    def wall(fn, sync):
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        return (time.perf_counter() - t0) * 1e3

    legs = {"many": (many, eng.sync, d_out, d_ref),
            "loop_baseline": (loop(lambda sg, pk, ms, cnt, out: base.aggregate(sg, pk, ms, cnt, out, False), d_out), base.sync,
                              d_out, d_ref)}
    if single_ok:
        legs["single"] = (single(d_one), eng.sync, d_one, d_one0)
    times = {leg: [] for leg in legs}
    for rnd in range(a.warmup + a.rounds):
        for leg, (fn, sync, out, want) in legs.items():
            out.fill_(255)
            d_res.fill_(255)
            torch.cuda.synchronize()
            ms = wall(fn, sync)
            if not bool((out == want).all()) or (leg == "many" and (bool((d_res != 0).any()) or int(d_nfail.item()) != 0)):
                res["mismatches"] += 1
            if rnd >= a.warmup:
                times[leg].append(ms)
    res["ms_rounds"] = {leg: [round(v, 3) for v in vs] for leg, vs in times.items()}
    res["ms_median"] = {leg: round(float(np.median(v)), 3) for leg, v in times.items()}
    res["ms_min"] = {leg: round(float(np.min(v)), 3) for leg, v in times.items()}
    med = res["ms_median"]
    res["ratio"] = {"loop_baseline/many": round(med["loop_baseline"] / med["many"], 3)}
    if single_ok:
        res["ratio"]["many/single"] = round(med["many"] / med["single"], 3)
    res["msigs_per_s"] = {leg: round(n / v / 1e3, 3) for leg, v in med.items()}
    kern = {}
    for name, fn in (("many", many),) + ((("single", single(d_one)),) if single_ok else ()):
        eng.sync()
        eng.enable_timing(True)
        fn()
        eng.sync()
        kern[name] = {}
        for kn in PRODUCE_KERNELS:
            avg, cnt = eng.read_timing(kn)
            if cnt:
                kern[name][kn] = [round(avg, 4), int(cnt)]
        eng.enable_timing(False)
    res["kernel_ms_avg_launches"] = kern
    total, _ = ssa.debug_aggregates_fold_plan(counts)
    res["plan"] = {"partials": total, "tree_passes": len(ssa.debug_aggregates_plan(counts)["passes"])}
    print(json.dumps(res))
    eng.close()
    base.close()
    return 0 if res["mismatches"] == 0 else 1


VALID_KERNELS = ("ssa_k_hash", "msm_k_prepare", "msm_sort", "msm_k_buckets", "msm_reduce", "msm_k_finish_seg",
                 "screen_gather", "ssa_k_verify", "screen_scatter", "av_k_keep", "av_k_gather", "ag_k_leaf", "ag_k_tree",
                 "ag_k_coeff", "ag_k_fold", "ag_k_pack")


class BaselineAggregate:
    """ssa_aggregate_many_device of a build of the library given by its path, on a context of its own"""

    def __init__(self, path):
        import ctypes as C
        self.lib = C.CDLL(path)
        vp, sz, i32 = C.c_void_p, C.c_size_t, C.c_int
        self.lib.ssa_ctx_create_ex.argtypes = [C.POINTER(vp), i32, vp, sz, C.c_uint32, C.c_uint64]
        self.lib.ssa_aggregate_many_device.argtypes = [vp, vp, vp, vp, vp, vp, sz, sz, sz, C.c_uint32, vp, vp, vp]
        self.lib.ssa_ctx_sync.argtypes = [vp]
        self.lib.ssa_ctx_destroy.argtypes = [vp]
        self.lib.ssa_ctx_destroy.restype = None
        self.ctx = vp()
        if self.lib.ssa_ctx_create_ex(C.byref(self.ctx), 0, None, 0, 0, 0) != 0:
            raise RuntimeError("baseline library: ssa_ctx_create_ex failed")

    def aggregate(self, d_sigs, d_pks, d_msgs, n, d_agg, check):
        rc = self.lib.ssa_aggregate_many_device(self.ctx, d_sigs, d_pks, None, d_msgs, None, 80, 80, n, 1 if check else 0,
                                                d_agg, None, None)
        if rc < 0:
            raise RuntimeError("baseline library: ssa_aggregate_many_device failed (%d)" % rc)
        return rc

    def sync(self):
        self.lib.ssa_ctx_sync(self.ctx)

    def close(self):
        self.lib.ssa_ctx_destroy(self.ctx)


def valid_main(a):
    import torch
    import schnorr_sig_amd as ssa
    dev = torch.device("cuda", 0)
    eng = ssa.Engine(0)
    base_path = a.baseline_lib or ssa.LIB_PATH
    base = BaselineAggregate(base_path)
    rng = np.random.default_rng(a.seed)
    n = a.n
    msgs = rng.integers(0, 256, (n, 80), dtype=np.uint8)
    pks, honest = eng.keygen_sign_many(_scalars(rng, n), _scalars(rng, n), msgs)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)   # noqa: E731
    d_pks, d_msgs = t(pks), t(msgs)
    sha = lambda path: hashlib.sha256(open(path, "rb").read()).hexdigest()[:16]   # noqa: E731
    res = {"metric": "aggregate_valid", "n": n, "msg_len": 80, "rounds": a.rounds, "warmup": a.warmup,
           "library_sha256": sha(ssa.LIB_PATH), "baseline_sha256": sha(base_path), "baseline_is_this_tree": not a.baseline_lib,
           "device": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d"), "mismatches": 0, "workloads": []}

    def wall(fn, sync):
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        return (time.perf_counter() - t0) * 1e3

    for name, n_bad in (("honest", 0), ("16 bad", 16), ("1 % bad", n // 100)):
        bad = np.sort(rng.choice(n, size=min(n_bad, n), replace=False))
        sigs = honest.copy()
        sigs[bad, 49] ^= 1
        keep = np.setdiff1d(np.arange(n), bad)
        m = keep.size
        d_sigs = t(sigs)
        d_fs, d_fp, d_fm = t(sigs[keep]), t(pks[keep]), t(msgs[keep])
        d_want = torch.zeros(49 * n + 32, dtype=torch.uint8, device=dev)          # the aggregate of the kept lanes, zeros behind
        d_keep = torch.zeros(n, dtype=torch.int32, device=dev)
        d_keep[:m] = t(keep.astype(np.int32))
        if m and eng.aggregate_device(d_fs.data_ptr(), d_fp.data_ptr(), d_fm.data_ptr(), m, 80, d_want.data_ptr()) != 0:
            res["mismatches"] += 1
        eng.sync()
        d_agg = torch.zeros(49 * n + 32, dtype=torch.uint8, device=dev)
        d_kept = torch.zeros(n, dtype=torch.int32, device=dev)
        got = {}

        def valid():
            got["m"] = eng.aggregate_valid_device(d_sigs.data_ptr(), d_pks.data_ptr(), d_msgs.data_ptr(), n, 80,
                                                  d_agg.data_ptr(), d_kept.data_ptr())

        def checked():
            got["rc"] = base.aggregate(d_sigs.data_ptr(), d_pks.data_ptr(), d_msgs.data_ptr(), n, d_agg.data_ptr(), True)

        def filtered():
            got["rc"] = base.aggregate(d_fs.data_ptr(), d_fp.data_ptr(), d_fm.data_ptr(), m, d_agg.data_ptr(), False)

        legs = {"valid": (valid, eng.sync), "baseline_checked": (checked, base.sync)}
        if n_bad and m:
            legs["baseline_filtered"] = (filtered, base.sync)
        times = {leg: [] for leg in legs}
        for rnd in range(a.warmup + a.rounds):
            for leg, (fn, sync) in legs.items():
                d_agg.fill_(0xEE)
                d_kept.fill_(-1)
                torch.cuda.synchronize()
                ms = wall(fn, sync)
                if leg == "valid":
                    good = got["m"] == m and bool((d_agg == d_want).all()) and bool((d_kept == d_keep).all())
                elif leg == "baseline_checked" and n_bad:
                    good = got["rc"] != 0 and not bool(d_agg.any())                # refused: a zeroed aggregate
                else:
                    good = got["rc"] == 0 and bool((d_agg[:49 * m + 32] == d_want[:49 * m + 32]).all())
                res["mismatches"] += 0 if good else 1
                if rnd >= a.warmup:
                    times[leg].append(ms)
        med = {leg: round(float(np.median(v)), 3) for leg, v in times.items()}
        route = round(med["baseline_checked"] + med.get("baseline_filtered", 0.0), 3)
        w = {"workload": name, "bad_lanes": int(bad.size), "kept": int(m), "ms_median": med,
             "ms_min": {leg: round(float(np.min(v)), 3) for leg, v in times.items()},
             "ms_all": {leg: [round(x, 3) for x in v] for leg, v in times.items()},
             "baseline_route_ms": route, "valid/baseline_route": round(med["valid"] / route, 3),
             "faster_than_baseline_route": bool(med["valid"] < route)}
        eng.sync()
        eng.enable_timing(True)
        valid()
        eng.sync()
        w["kernel_ms_avg_launches"] = {}
        for k in VALID_KERNELS:
            avg, cnt = eng.read_timing(k)
            if cnt:
                w["kernel_ms_avg_launches"][k] = [round(avg, 4), int(cnt)]
        eng.enable_timing(False)
        res["workloads"].append(w)
    print(json.dumps(res))
    eng.close()
    base.close()
    return 0 if res["mismatches"] == 0 else 1


VALID_CACHED_KERNELS = ("keyed_split", "dedup", "keycache_lookup", "keycache_insert", "ssa_k_keyed_decompress",
                        "ssa_k_keyset_build", "keycache_map", "keyed_expand", "ssa_k_hash", "screen_keymask", "msm_k_prepare",
                        "msm_sort", "msm_k_buckets", "msm_reduce", "msm_k_finish_seg", "screen_mark", "screen_list_gather",
                        "ssa_k_verify_keyed", "screen_list_scatter", "av_k_keep", "av_k_gather_keys", "av_k_gather",
                        "ag_k_leaf", "ag_k_tree", "ag_k_coeff", "ag_k_fold", "ag_k_pack")


class BaselineGuarded:
    """ssa_aggregate_valid_many_device, and ssa_verify_many_cached_device + ssa_aggregate_many_device, of a build of the
    library given by its path, on a context and an affine key cache of its own"""

    def __init__(self, path, capacity):
        import ctypes as C
        self.C, self.lib = C, C.CDLL(path)
        vp, sz, i32, u32 = C.c_void_p, C.c_size_t, C.c_int, C.c_uint32
        self.lib.ssa_ctx_create_ex.argtypes = [C.POINTER(vp), i32, vp, sz, u32, C.c_uint64]
        self.lib.ssa_keycache_create.argtypes = [vp, sz, C.POINTER(vp)]
        self.lib.ssa_keycache_destroy.argtypes = [vp]
        self.lib.ssa_keycache_destroy.restype = None
        self.lib.ssa_verify_many_cached_device.argtypes = [vp, vp, vp, vp, vp, vp, vp, sz, sz, sz, u32, vp, u32, vp, vp, vp]
        self.lib.ssa_aggregate_many_device.argtypes = [vp, vp, vp, vp, vp, vp, sz, sz, sz, u32, vp, vp, vp]
        self.lib.ssa_aggregate_valid_many_device.argtypes = [vp, vp, vp, vp, vp, vp, sz, sz, sz, vp, vp,
                                                             C.POINTER(C.c_uint64), vp]
        self.lib.ssa_ctx_sync.argtypes = [vp]
        self.lib.ssa_ctx_destroy.argtypes = [vp]
        self.lib.ssa_ctx_destroy.restype = None
        self.ctx, self.kc = vp(), vp()
        if self.lib.ssa_ctx_create_ex(C.byref(self.ctx), 0, None, 0, 0, 0) != 0:
            raise RuntimeError("baseline library: ssa_ctx_create_ex failed")
        if self.lib.ssa_keycache_create(self.ctx, capacity, C.byref(self.kc)) != 0:
            raise RuntimeError("baseline library: ssa_keycache_create failed")

    def valid(self, d_sigs, d_pks, d_msgs, n, d_agg, d_kept):
        nk = self.C.c_uint64(0)
        if self.lib.ssa_aggregate_valid_many_device(self.ctx, d_sigs, d_pks, None, d_msgs, None, 80, 80, n, d_agg, d_kept,
                                                    self.C.byref(nk), None) != 0:
            raise RuntimeError("baseline library: ssa_aggregate_valid_many_device failed")
        return int(nk.value)

    def statuses(self, d_sigs, d_pks, d_msgs, n, d_status):
        if self.lib.ssa_verify_many_cached_device(self.ctx, self.kc, d_sigs, d_pks, None, d_msgs, None, 80, 80, n, 1 | 8, None,
                                                  32, d_status, None, None) != 0:
            raise RuntimeError("baseline library: ssa_verify_many_cached_device failed")

    def aggregate(self, d_sigs, d_pks, d_msgs, n, d_agg):
        if self.lib.ssa_aggregate_many_device(self.ctx, d_sigs, d_pks, None, d_msgs, None, 80, 80, n, 0, d_agg, None, None) != 0:
            raise RuntimeError("baseline library: ssa_aggregate_many_device failed")

    def sync(self):
        self.lib.ssa_ctx_sync(self.ctx)

    def close(self):
        self.lib.ssa_keycache_destroy(self.kc)
        self.lib.ssa_ctx_destroy(self.ctx)


def valid_cached_main(a):
    import torch
    import schnorr_sig_amd as ssa
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import pymodel as pm
    dev = torch.device("cuda", 0)
    n = a.n
    if a.signers < 0 or a.signers > n:
        raise SystemExit("--signers must lie in [0, n = %d]" % n)
    signers = a.signers or n
    eng = ssa.Engine(0)
    base_path = a.baseline_lib or ssa.LIB_PATH
    base = BaselineGuarded(base_path, signers + 16)
    rng = np.random.default_rng(a.seed)
    msgs = rng.integers(0, 256, (n, 80), dtype=np.uint8)
    idx = rng.integers(0, signers, size=n)
    idx[:signers] = np.arange(signers)
    rng.shuffle(idx)
    pks, honest = eng.keygen_sign_many(_scalars(rng, signers)[idx], _scalars(rng, n), msgs)
    # a key on the curve and outside the prime-order subgroup: the point of order 2
    t2 = np.frombuffer(pm.fp6_to_bytes48(pm.SMALL_ORDER_POINTS[2][0]) + pm.fp6_to_bytes48(pm.SMALL_ORDER_POINTS[2][1]), np.uint8)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)   # noqa: E731
    d_msgs = t(msgs)
    sha = lambda path: hashlib.sha256(open(path, "rb").read()).hexdigest()[:16]   # noqa: E731
    res = {"metric": "aggregate_valid_cached", "n": n, "signers": signers, "msg_len": 80, "rounds": a.rounds,
           "warmup": a.warmup, "library_sha256": sha(ssa.LIB_PATH), "baseline_sha256": sha(base_path),
           "baseline_is_this_tree": not a.baseline_lib, "device": torch.cuda.get_device_name(0),
           "date": time.strftime("%Y-%m-%d"), "mismatches": 0, "workloads": []}
    ac, wc = eng.keycache_create(signers + 16), eng.keycache_create(signers + 16, wire=True)

    for name, n_bad in (("honest", 0), ("16 bad", 16), ("1 % bad, half of them keys", n // 100)):
        bad = np.sort(rng.choice(n, size=min(n_bad, n), replace=False))
        sigs, keys = honest.copy(), pks.copy()
        sigs[bad[0::2], 49] ^= 1
        if name.startswith("1 %"):
            keys[bad[1::2]] = t2
        else:
            sigs[bad[1::2], 49] ^= 1
        wire, st = eng.compress_many(keys)
        assert (st == 0).all()
        keep = np.setdiff1d(np.arange(n), bad)
        m = keep.size
        rec = np.concatenate([wire, sigs], axis=1)
        d_sigs, d_pks, d_rec = t(sigs), t(keys), t(rec)
        d_fs, d_fp, d_fm = t(sigs[keep]), t(keys[keep]), t(msgs[keep])
        d_want = torch.zeros(49 * n + 32, dtype=torch.uint8, device=dev)          # the aggregate of the kept lanes, zeros behind
        d_keep = torch.zeros(n, dtype=torch.int32, device=dev)
        d_keep[:m] = t(keep.astype(np.int32))
        d_want_pks, d_want_w = torch.zeros(n, 96, dtype=torch.uint8, device=dev), torch.zeros(n, 49, dtype=torch.uint8, device=dev)
        d_want_pks[:m], d_want_w[:m] = d_fp, t(wire[keep])
        if m and eng.aggregate_device(d_fs.data_ptr(), d_fp.data_ptr(), d_fm.data_ptr(), m, 80, d_want.data_ptr()) != 0:
            res["mismatches"] += 1
        eng.sync()
        d_agg = torch.zeros(49 * n + 32, dtype=torch.uint8, device=dev)
        d_kept = torch.zeros(n, dtype=torch.int32, device=dev)
        d_ko, d_io = torch.zeros(n, 96, dtype=torch.uint8, device=dev), torch.zeros(n, dtype=torch.uint8, device=dev)
        d_wo = torch.zeros(n, 49, dtype=torch.uint8, device=dev)
        d_status = torch.zeros(n, dtype=torch.uint8, device=dev)
        got = {}

        def affine():
            got["m"], got["stats"] = eng.aggregate_valid_cached_device(
                ac, d_sigs.data_ptr(), d_pks.data_ptr(), d_msgs.data_ptr(), n, 80, d_agg.data_ptr(), d_kept.data_ptr(),
                d_pks_out=d_ko.data_ptr(), d_pk_inf_out=d_io.data_ptr())

        def keyed():
            got["m"], got["stats"] = eng.aggregate_valid_keyed_cached_device(
                wc, d_rec.data_ptr(), d_msgs.data_ptr(), n, 80, d_agg.data_ptr(), d_kept.data_ptr(), d_keys49_out=d_wo.data_ptr())

        def base_valid():
            got["m"] = base.valid(d_sigs.data_ptr(), d_pks.data_ptr(), d_msgs.data_ptr(), n, d_agg.data_ptr(), d_kept.data_ptr())

        def base_guarded():
            base.statuses(d_sigs.data_ptr(), d_pks.data_ptr(), d_msgs.data_ptr(), n, d_status.data_ptr())
            base.aggregate(d_fs.data_ptr(), d_fp.data_ptr(), d_fm.data_ptr(), m, d_agg.data_ptr())

        legs = {"affine_cold": (affine, eng.sync), "affine_warm": (affine, eng.sync), "keyed_cold": (keyed, eng.sync),
                "keyed_warm": (keyed, eng.sync), "baseline_valid": (base_valid, base.sync),
                "baseline_guarded": (base_guarded, base.sync)}
        base_guarded()          # the baseline's cache is warm from here on
        base.sync()
        times = {leg: [] for leg in legs}
        for rnd in range(a.warmup + a.rounds):
            for leg, (fn, sync) in legs.items():
                for buf in (d_agg, d_ko, d_io, d_wo, d_status):
                    buf.fill_(0xEE)
                d_kept.fill_(-1)
                if leg == "affine_cold":
                    ac.clear()
                if leg == "keyed_cold":
                    wc.clear()
                eng.sync()
                torch.cuda.synchronize()
                sync()
                t0 = time.perf_counter()
                fn()
                sync()
                ms = (time.perf_counter() - t0) * 1e3
                if leg == "baseline_guarded":
                    good = bool((d_agg[:49 * m + 32] == d_want[:49 * m + 32]).all()) and \
                        np.flatnonzero(d_status.cpu().numpy()).tolist() == bad.tolist()
                else:
                    good = got["m"] == m and bool((d_agg == d_want).all()) and bool((d_kept == d_keep).all())
                if leg.startswith("affine"):
                    good = good and bool((d_ko == d_want_pks).all()) and not bool(d_io.any())
                if leg.startswith("keyed"):
                    good = good and bool((d_wo == d_want_w).all())
                if leg.endswith("_cold"):
                    good = good and int(got["stats"][8]) == 0
                if leg.endswith("_warm"):
                    good = good and int(got["stats"][9]) == 0
                res["mismatches"] += 0 if good else 1
                if rnd >= a.warmup:
                    times[leg].append(ms)
        med = {leg: round(float(np.median(v)), 3) for leg, v in times.items()}
        w = {"workload": name, "bad_lanes": int(bad.size), "kept": int(m), "ms_median": med,
             "ms_min": {leg: round(float(np.min(v)), 3) for leg, v in times.items()},
             "ms_all": {leg: [round(x, 3) for x in v] for leg, v in times.items()},
             "ratio": {leg + "/" + b: round(med[leg] / med[b], 3) for leg in ("affine_cold", "affine_warm", "keyed_cold", "keyed_warm")
                       for b in ("baseline_valid", "baseline_guarded")}}
        if n_bad == 0:
            kern = {}
            for leg in ("affine_warm", "keyed_warm"):
                eng.sync()
                eng.enable_timing(True)
                legs[leg][0]()
                eng.sync()
                kern[leg] = {}
                for kn in VALID_CACHED_KERNELS:
                    avg, cnt = eng.read_timing(kn)
                    if cnt:
                        kern[leg][kn] = [round(avg, 4), int(cnt)]
                eng.enable_timing(False)
            w["kernel_ms_avg_launches"] = kern
        res["workloads"].append(w)
    print(json.dumps(res))
    ac.close()
    wc.close()
    eng.close()
    base.close()
    return 0 if res["mismatches"] == 0 else 1


CACHED_KERNELS = ("dedup", "keycache_lookup", "keycache_insert", "ssa_k_keyed_decompress", "ssa_k_keyset_build",
                  "keycache_map", "agc_expand") + MANY_KERNELS + ("agc_k_key_verdicts",)


class BaselineRoute:
    """decompress + verify_aggregates_many (+ a key set over the distinct keys) of a build of the library given by its
    path, on a context of its own"""

    def __init__(self, path):
        import ctypes as C
        self.C, self.lib = C, C.CDLL(path)
        vp, sz, i32, u64p = C.c_void_p, C.c_size_t, C.c_int, C.POINTER(C.c_uint64)
        self.lib.ssa_ctx_create_ex.argtypes = [C.POINTER(vp), i32, vp, sz, C.c_uint32, C.c_uint64]
        self.lib.ssa_decompress_many_device.argtypes = [vp, vp, sz, vp, vp, vp]
        self.lib.ssa_verify_aggregates_many_device.argtypes = [vp, vp, u64p, sz, vp, vp, vp, vp, sz, sz, vp]
        self.lib.ssa_keyset_create_device.argtypes = [vp, vp, vp, sz, C.c_uint32, C.POINTER(vp)]
        self.lib.ssa_keyset_destroy.argtypes = [vp]
        self.lib.ssa_keyset_destroy.restype = None
        self.lib.ssa_ctx_sync.argtypes = [vp]
        self.lib.ssa_ctx_destroy.argtypes = [vp]
        self.lib.ssa_ctx_destroy.restype = None
        self.ctx = vp()
        self.keysets = []
        if self.lib.ssa_ctx_create_ex(C.byref(self.ctx), 0, None, 0, 0, 0) != 0:
            raise RuntimeError("baseline library: ssa_ctx_create_ex failed")

    def route(self, d_wire_keys, d_pks, d_inf, d_st, n, d_aggs, counts, d_msgs, d_v, d_distinct=0, m=0):
        if m:       # the statuses of the subgroup check: ladder tables (4 KB per key) over the distinct keys
            ks = self.C.c_void_p()
            if self.lib.ssa_keyset_create_device(self.ctx, d_distinct, None, m, 2, self.C.byref(ks)) != 0:
                raise RuntimeError("baseline library: ssa_keyset_create_device failed")
            self.keysets.append(ks)
        if self.lib.ssa_decompress_many_device(self.ctx, d_wire_keys, n, d_pks, d_inf, d_st) != 0:
            raise RuntimeError("baseline library: ssa_decompress_many_device failed")
        cp = counts.ctypes.data_as(self.C.POINTER(self.C.c_uint64))
        if self.lib.ssa_verify_aggregates_many_device(self.ctx, d_aggs, cp, counts.size, d_pks, d_inf, d_msgs, None, 80, 80,
                                                      d_v) != 0:
            raise RuntimeError("baseline library: ssa_verify_aggregates_many_device failed")

    def drop_keysets(self):         # (outside the timed region)
        for ks in self.keysets:
            self.lib.ssa_keyset_destroy(ks)
        self.keysets = []

    def sync(self):
        self.lib.ssa_ctx_sync(self.ctx)

    def close(self):
        self.drop_keysets()
        self.lib.ssa_ctx_destroy(self.ctx)


def cached_main(a):
    import torch
    import schnorr_sig_amd as ssa
    dev = torch.device("cuda", 0)
    k, s = tuple(int(v) for v in (a.many[0] if a.many else "1024x1024").lower().split("x"))
    n = k * s
    if a.signers < 0 or a.signers > n:
        raise SystemExit("--signers must lie in [0, K * S = %d]" % n)
    signers = a.signers or n
    eng = ssa.Engine(0)
    base_path = a.baseline_lib or ssa.LIB_PATH
    base = BaselineRoute(base_path)
    rng = np.random.default_rng(a.seed)
    msgs = rng.integers(0, 256, (n, 80), dtype=np.uint8)
    idx = rng.integers(0, signers, size=n)
    idx[:signers] = np.arange(signers)
    rng.shuffle(idx)
    sks = _scalars(rng, signers)
    pks, sigs = eng.keygen_sign_many(sks[idx], _scalars(rng, n), msgs)
    wire_keys, st = eng.compress_many(pks)
    distinct = eng.pubkey_many(sks)
    assert (st == 0).all()
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)   # noqa: E731
    d_sigs, d_pks, d_msgs, d_wk, d_distinct = t(sigs), t(pks), t(msgs), t(wire_keys), t(distinct)
    d_upks = torch.zeros(96 * n, dtype=torch.uint8, device=dev)       # what the baseline's decompression writes
    d_uinf = torch.zeros(n, dtype=torch.uint8, device=dev)
    d_ust = torch.zeros(n, dtype=torch.uint8, device=dev)
    d_wire = torch.zeros(49 * n + 32 * k, dtype=torch.uint8, device=dev)
    sha = lambda path: hashlib.sha256(open(path, "rb").read()).hexdigest()[:16]   # noqa: E731
    res = {"metric": "aggregates_cached", "aggregates": k, "signatures_each": s, "signers": signers, "msg_len": 80,
           "rounds": a.rounds, "warmup": a.warmup, "library_sha256": sha(ssa.LIB_PATH), "baseline_sha256": sha(base_path),
           "baseline_is_this_tree": not a.baseline_lib, "device": torch.cuda.get_device_name(0),
           "date": time.strftime("%Y-%m-%d"), "mismatches": 0}
    for j in range(k):        # the honest aggregates, in their wire form end to end
        lo = j * s
        if eng.aggregate_device(d_sigs.data_ptr() + 81 * lo, d_pks.data_ptr() + 96 * lo, d_msgs.data_ptr() + 80 * lo, s, 80,
                                d_wire.data_ptr() + 49 * lo + 32 * j) != 0:
            res["mismatches"] += 1
    eng.sync()
    counts = np.full(k, s, dtype=np.uint64)
    d_v = torch.full((k,), 255, dtype=torch.int32, device=dev)
    wc, ac = eng.keycache_create(signers, wire=True), eng.keycache_create(signers)
    stats = {}

    def cached(cache, d_keys, leg):
        def run():
            stats[leg] = eng.verify_aggregates_cached_device(cache, d_wire, counts, d_keys, d_msgs, d_verdicts=d_v)[1]
        return run

    def baseline(with_keyset):
        return lambda: base.route(d_wk.data_ptr(), d_upks.data_ptr(), d_uinf.data_ptr(), d_ust.data_ptr(), n,
                                  d_wire.data_ptr(), counts, d_msgs.data_ptr(), d_v.data_ptr(),
                                  d_distinct.data_ptr() if with_keyset else 0, signers if with_keyset else 0)

    legs = {"wire_cold": (cached(wc, d_wk, "wire_cold"), eng.sync), "wire_warm": (cached(wc, d_wk, "wire_warm"), eng.sync),
            "affine_warm": (cached(ac, d_pks, "affine_warm"), eng.sync), "baseline": (baseline(False), base.sync),
            "baseline_keyset": (baseline(True), base.sync)}
    cached(ac, d_pks, "affine_warm")()        # the affine cache is warm from here on
    eng.sync()
    times = {leg: [] for leg in legs}
    for rnd in range(a.warmup + a.rounds):
        for leg, (fn, sync) in legs.items():
            d_v.fill_(255)
            if leg == "wire_cold":
                wc.clear()
            eng.sync()
            torch.cuda.synchronize()
            sync()
            t0 = time.perf_counter()
            fn()
            sync()
            ms = (time.perf_counter() - t0) * 1e3
            base.drop_keysets()
            good = not bool((d_v != 0).any())
            if leg in stats:      # cold: every key inserted; warm: every key found; nothing refused
                st = [int(x) for x in stats[leg]]
                good = good and st[0] == signers and st[6] == 0 and \
                    (st[2] == signers and st[1] == 0 if leg == "wire_cold" else st[1] == signers and st[2] == 0)
            elif bool((d_upks.view(-1, 96) != d_pks).any()):
                good = False
            res["mismatches"] += 0 if good else 1
            if rnd >= a.warmup:
                times[leg].append(ms)
    med = {leg: round(float(np.median(v)), 3) for leg, v in times.items()}
    res["ms_median"] = med
    res["ms_min"] = {leg: round(float(np.min(v)), 3) for leg, v in times.items()}
    res["ms_all"] = {leg: [round(x, 3) for x in v] for leg, v in times.items()}
    res["ratio"] = {"wire_warm/baseline": round(med["wire_warm"] / med["baseline"], 3),
                    "wire_warm/baseline_keyset": round(med["wire_warm"] / med["baseline_keyset"], 3),
                    "wire_cold/baseline_keyset": round(med["wire_cold"] / med["baseline_keyset"], 3),
                    "affine_warm/wire_warm": round(med["affine_warm"] / med["wire_warm"], 3)}
    res["stats"] = {leg: [int(x) for x in v] for leg, v in stats.items()}
    kern = {}
    for leg in ("wire_warm", "wire_cold"):
        if leg == "wire_cold":
            wc.clear()
        eng.sync()
        eng.enable_timing(True)
        legs[leg][0]()
        eng.sync()
        kern[leg] = {}
        for kn in CACHED_KERNELS:
            avg, cnt = eng.read_timing(kn)
            if cnt:
                kern[leg][kn] = [round(avg, 4), int(cnt)]
        eng.enable_timing(False)
    res["kernel_ms_avg_launches"] = kern
    print(json.dumps(res))
    wc.close()
    ac.close()
    eng.close()
    base.close()
    return 0 if res["mismatches"] == 0 else 1


SHARDED_KERNELS = KERNELS[:3] + ("ag_k_level",) + KERNELS[3:] + ("ag_k_expand", "msm_k_sum_records")


def sharded_main(a):
    """--sharded: the sliced calls of DESIGN.md section 25 against the single calls of --baseline-lib (a build of the parent
    commit; without it, this tree's own library), device buffers, the legs alternating in one process.  Up to one MSM slice
    the two routes differ in the tree alone: flat ag_k_level launches against ag_k_tree.  Above it only this tree's legs
    run (the single calls refuse the size); the batch is then 2^20 distinct lanes repeated.  With --multi also
    MultiEngine([0, 0]) from host buffers against this tree's host forms: TWO CONTEXTS ON ONE DEVICE, not scaling."""
    import torch
    import schnorr_sig_amd as ssa
    dev = torch.device("cuda", 0)
    eng = ssa.Engine(0)
    base_path = a.baseline_lib or ssa.LIB_PATH
    n, n0 = a.n, min(a.n, 1 << 20)
    if n % n0:
        raise SystemExit("--sharded: n above 2^20 must be a multiple of it")
    with_base = n <= 1 << 23
    base_a, base_v = (BaselineAggregate(base_path), BaselineLoop(base_path)) if with_base else (None, None)
    rng = np.random.default_rng(a.seed)
    msgs = rng.integers(0, 256, (n0, 80), dtype=np.uint8)
    pks, sigs = eng.keygen_sign_many(_scalars(rng, n0), _scalars(rng, n0), msgs)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev).repeat(n // n0, 1)   # noqa: E731
    d_sigs, d_pks, d_msgs = t(sigs), t(pks), t(msgs)
    d_agg = torch.zeros(49 * n + 32, dtype=torch.uint8, device=dev)
    d_agg0 = torch.zeros(49 * n + 32, dtype=torch.uint8, device=dev)
    d_verdict = torch.full((1,), 255, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    sha = lambda path: hashlib.sha256(open(path, "rb").read()).hexdigest()[:16]   # noqa: E731
    res = {"metric": "aggregate_sharded", "n": n, "distinct_lanes": n0, "msg_len": 80, "rounds": a.rounds, "warmup": a.warmup,
           "library_sha256": sha(ssa.LIB_PATH), "baseline_sha256": sha(base_path), "baseline_is_this_tree": not a.baseline_lib,
           "device": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d"), "mismatches": 0}
    ptrs = (d_sigs.data_ptr(), d_pks.data_ptr(), d_msgs.data_ptr())

    def wall(fn, sync):
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        return (time.perf_counter() - t0) * 1e3

    if eng.aggregate_sliced_device(*ptrs, n, 80, d_agg0.data_ptr()) != 0:
        res["mismatches"] += 1
    eng.sync()
    verify_ptrs = (d_agg0.data_ptr(), d_pks.data_ptr(), d_msgs.data_ptr())
    legs = {"verify_sliced": (lambda: eng.verify_aggregate_sliced_device(*verify_ptrs, n, 80, d_verdict.data_ptr()), eng.sync),
            "aggregate_sliced": (lambda: eng.aggregate_sliced_device(*ptrs, n, 80, d_agg.data_ptr()), eng.sync)}
    if with_base:
        legs.update({
            "verify_baseline": (lambda: base_v.verify(*verify_ptrs, n, d_verdict.data_ptr()), base_v.sync),
            "aggregate_baseline": (lambda: base_a.aggregate(*ptrs, n, d_agg.data_ptr(), False), base_a.sync),
            "verify_single": (lambda: eng.verify_aggregate_device(*verify_ptrs, n, 80, d_verdict.data_ptr()), eng.sync),
            "aggregate_single": (lambda: eng.aggregate_device(*ptrs, n, 80, d_agg.data_ptr()), eng.sync)})
    times = {leg: [] for leg in legs}
    for rnd in range(a.warmup + a.rounds):
        for leg, (fn, sync) in legs.items():
            d_verdict.fill_(255)
            d_agg.fill_(0xEE)
            torch.cuda.synchronize()
            ms = wall(fn, sync)
            good = int(d_verdict.item()) == 0 if leg.startswith("verify") else bool((d_agg == d_agg0).all())
            res["mismatches"] += 0 if good else 1
            if rnd >= a.warmup:
                times[leg].append(ms)
    med = res["ms_median"] = {leg: round(float(np.median(v)), 3) for leg, v in times.items()}
    res["ms_all"] = {leg: [round(x, 3) for x in v] for leg, v in times.items()}
    if with_base:
        res["ratio"] = {"verify_sliced/verify_baseline": round(med["verify_sliced"] / med["verify_baseline"], 4),
                        "aggregate_sliced/aggregate_baseline": round(med["aggregate_sliced"] / med["aggregate_baseline"], 4)}
    kern = {}
    for leg in ("verify_sliced", "aggregate_sliced") + (("verify_single",) if with_base else ()):
        eng.sync()
        eng.enable_timing(True)
        legs[leg][0]()
        eng.sync()
        kern[leg] = {}
        for k in SHARDED_KERNELS:
            avg, cnt = eng.read_timing(k)
            if cnt:
                kern[leg][k] = [round(avg, 4), int(cnt)]
        eng.enable_timing(False)
    res["kernel_ms_avg_regions"] = kern
    # nanoseconds per Rescue permutation: a leaf is one per lane; the flat levels of a slice of m lanes hash m - 1 pairs
    # when the block is the slice, ag_k_tree over n leaves n - 1 and the root
    kv, slices = kern["verify_sliced"], -(-n // (1 << 23))
    if "ag_k_level" in kv and "ag_k_leaf" in kv:
        res["ns_per_permutation"] = {"ag_k_leaf": round(kv["ag_k_leaf"][0] * kv["ag_k_leaf"][1] * 1e6 / n, 3),
                                     "ag_k_level": round(kv["ag_k_level"][0] * kv["ag_k_level"][1] * 1e6 / (n - slices), 3)}
        if with_base and "ag_k_tree" in kern["verify_single"]:
            res["ns_per_permutation"]["ag_k_tree"] = round(kern["verify_single"]["ag_k_tree"][0] * 1e6 / n, 3)
    if a.multi:
        old = os.environ.get("SSA_AGG_BLOCK")
        os.environ["SSA_AGG_BLOCK"] = str(n // 2)          # two blocks: one per context
        try:
            multi = ssa.MultiEngine([0, 0])
        finally:
            if old is None:
                del os.environ["SSA_AGG_BLOCK"]
            else:
                os.environ["SSA_AGG_BLOCK"] = old
        h_sigs, h_pks, h_msgs = (x.cpu().numpy() for x in (d_sigs, d_pks, d_msgs))
        h_agg = d_agg0.cpu().numpy()
        mlegs = {"multi_aggregate": lambda: multi.aggregate(h_sigs, h_pks, h_msgs)[1],
                 "host_aggregate": lambda: eng.aggregate_sliced(h_sigs, h_pks, h_msgs)[1],
                 "multi_verify": lambda: multi.verify_aggregate(h_agg, h_pks, h_msgs),
                 "host_verify": lambda: eng.verify_aggregate_sliced(h_agg, h_pks, h_msgs)}
        mt = {leg: [] for leg in mlegs}
        for rnd in range(a.warmup + a.rounds):
            for leg, fn in mlegs.items():
                t0 = time.perf_counter()
                out = fn()
                ms = (time.perf_counter() - t0) * 1e3
                good = out == 0 if leg.endswith("verify") else bool((out == h_agg).all())
                res["mismatches"] += 0 if good else 1
                if rnd >= a.warmup:
                    mt[leg].append(ms)
        res["two_contexts_on_one_device_host_buffers_ms_median"] = {leg: round(float(np.median(v)), 3) for leg, v in mt.items()}
        multi.close()
    print(json.dumps(res))
    eng.close()
    for b in (base_a, base_v):
        if b:
            b.close()
    return 0 if res["mismatches"] == 0 else 1


ACCUMULATOR_KERNELS = ("ssa_k_hash", "msm_k_prepare", "msm_sort", "msm_k_buckets", "msm_reduce", "msm_k_finish_seg",
                       "screen_gather", "ssa_k_verify", "screen_scatter", "agx_k_check", "av_k_keep", "agx_k_append",
                       "ag_k_level", "ag_k_tree", "agx_k_coeff_fold", "ag_k_fold_finish")


class BaselineProducer:
    """ssa_aggregate_many_sliced_device and ssa_aggregate_valid_many_device of a build of the library given by its path,
    on a context of its own"""

    def __init__(self, path):
        import ctypes as C
        self.C, self.lib = C, C.CDLL(path)
        vp, sz, i32 = C.c_void_p, C.c_size_t, C.c_int
        self.lib.ssa_ctx_create_ex.argtypes = [C.POINTER(vp), i32, vp, sz, C.c_uint32, C.c_uint64]
        self.lib.ssa_aggregate_many_sliced_device.argtypes = [vp, vp, vp, vp, vp, vp, sz, sz, sz, C.c_uint32, vp, vp, vp]
        self.lib.ssa_aggregate_valid_many_device.argtypes = [vp, vp, vp, vp, vp, vp, sz, sz, sz, vp, vp,
                                                             C.POINTER(C.c_uint64), vp]
        self.lib.ssa_ctx_sync.argtypes = [vp]
        self.lib.ssa_ctx_destroy.argtypes = [vp]
        self.lib.ssa_ctx_destroy.restype = None
        self.ctx = vp()
        if self.lib.ssa_ctx_create_ex(C.byref(self.ctx), 0, None, 0, 0, 0) != 0:
            raise RuntimeError("baseline library: ssa_ctx_create_ex failed")

    def sliced(self, d_sigs, d_pks, d_msgs, n, d_agg):
        rc = self.lib.ssa_aggregate_many_sliced_device(self.ctx, d_sigs, d_pks, None, d_msgs, None, 80, 80, n, 0, d_agg, None,
                                                       None)
        if rc != 0:
            raise RuntimeError("baseline library: ssa_aggregate_many_sliced_device failed (%d)" % rc)

    def valid(self, d_sigs, d_pks, d_msgs, n, d_agg, d_kept):
        kept = self.C.c_uint64(0)
        if self.lib.ssa_aggregate_valid_many_device(self.ctx, d_sigs, d_pks, None, d_msgs, None, 80, 80, n, d_agg, d_kept,
                                                    self.C.byref(kept), None) != 0:
            raise RuntimeError("baseline library: ssa_aggregate_valid_many_device failed")
        return int(kept.value)

    def sync(self):
        self.lib.ssa_ctx_sync(self.ctx)

    def close(self):
        self.lib.ssa_ctx_destroy(self.ctx)


def accumulator_main(a):
    """--accumulator: the streaming aggregator.  --n honest signatures over 80-byte messages in
    device buffers are pushed in --pushes equal pushes; then the legs alternate in one process:
      finish            ssa_aggregator_finish_device and a stream synchronisation: what is left for block time
      baseline_sliced   ssa_aggregate_many_sliced_device through --baseline-lib (a build of the parent commit; without
                        it, this tree's own library) over the same signatures: the fastest one-shot producer call
      pushes            reset and all the pushes again, each one timed: their sum (recorded only)
      baseline_valid    ssa_aggregate_valid_many_device through the same library at --n (recorded only)
    The bar: finish < baseline_sliced, by more than baseline_sliced differs between two processes."""
    import torch
    import schnorr_sig_amd as ssa
    dev = torch.device("cuda", 0)
    eng = ssa.Engine(0)
    base_path = a.baseline_lib or ssa.LIB_PATH
    base = BaselineProducer(base_path)
    n, k = a.n, a.pushes
    if n % k:
        raise SystemExit("--accumulator: --n must be a multiple of --pushes")
    per = n // k
    rng = np.random.default_rng(a.seed)
    msgs = rng.integers(0, 256, (n, 80), dtype=np.uint8)
    pks, sigs = eng.keygen_sign_many(_scalars(rng, n), _scalars(rng, n), msgs)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)   # noqa: E731
    d_sigs, d_pks, d_msgs = t(sigs), t(pks), t(msgs)
    d_agg = torch.zeros(49 * n + 32, dtype=torch.uint8, device=dev)
    d_agg0 = torch.zeros(49 * n + 32, dtype=torch.uint8, device=dev)
    d_kept = torch.zeros(n, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    sha = lambda path: hashlib.sha256(open(path, "rb").read()).hexdigest()[:16]   # noqa: E731
    res = {"metric": "aggregator", "n": n, "pushes": k, "msg_len": 80, "rounds": a.rounds, "warmup": a.warmup,
           "library_sha256": sha(ssa.LIB_PATH), "baseline_sha256": sha(base_path), "baseline_is_this_tree": not a.baseline_lib,
           "device": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d"), "mismatches": 0}
    ptrs = (d_sigs.data_ptr(), d_pks.data_ptr(), d_msgs.data_ptr())
    base.sliced(*ptrs, n, d_agg0.data_ptr())
    base.sync()
    ag = eng.aggregator(n)

    def wall(fn, sync):
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        return (time.perf_counter() - t0) * 1e3

    def push_all():
        """reset, then every push timed on its own -> their times"""
        ag.reset()
        out = []
        for j in range(k):
            sl = slice(j * per, (j + 1) * per)
            out.append(wall(lambda: ag.push_device(d_sigs[sl], d_pks[sl], d_msgs[sl]), eng.sync))
        if ag.info()["held"] != n:
            res["mismatches"] += 1
        return out

    push_all()
    push_ms, times = [], {"finish": [], "baseline_sliced": [], "pushes": [], "baseline_valid": []}
    for rnd in range(a.warmup + a.rounds):
        for leg in times:
            d_agg.fill_(0xEE)
            torch.cuda.synchronize()
            if leg == "finish":
                ms = wall(lambda: ag.finish_device(d_agg), eng.sync)
            elif leg == "baseline_sliced":
                ms = wall(lambda: base.sliced(*ptrs, n, d_agg.data_ptr()), base.sync)
            elif leg == "pushes":
                each = push_all()
                ms = float(np.sum(each))
                if rnd >= a.warmup:
                    push_ms.append(each)
                ag.finish_device(d_agg)
                eng.sync()
            else:
                kept = []
                ms = wall(lambda: kept.append(base.valid(*ptrs, n, d_agg.data_ptr(), d_kept.data_ptr())), base.sync)
                res["mismatches"] += 0 if kept == [n] else 1
            res["mismatches"] += 0 if bool((d_agg == d_agg0).all()) else 1
            if rnd >= a.warmup:
                times[leg].append(ms)
    med = res["ms_median"] = {leg: round(float(np.median(v)), 3) for leg, v in times.items()}
    res["ms_all"] = {leg: [round(x, 3) for x in v] for leg, v in times.items()}
    res["push_ms_median_by_position"] = [round(float(x), 3) for x in np.median(np.array(push_ms), axis=0)]
    res["ratio"] = {"finish/baseline_sliced": round(med["finish"] / med["baseline_sliced"], 4),
                    "pushes/baseline_valid": round(med["pushes"] / med["baseline_valid"], 4)}
    res["finish_faster_than_baseline_sliced"] = bool(med["finish"] < med["baseline_sliced"])

    def timed(fn):
        eng.sync()
        eng.enable_timing(True)
        fn()
        eng.sync()
        out = {}
        for kn in ACCUMULATOR_KERNELS:
            avg, cnt = eng.read_timing(kn)
            if cnt:
                out[kn] = [round(avg, 4), int(cnt)]
        eng.enable_timing(False)
        return out

    kern = {"finish": timed(lambda: ag.finish_device(d_agg))}
    ag.reset()
    kern["push"] = timed(lambda: ag.push_device(d_sigs[:per], d_pks[:per], d_msgs[:per]))
    kern["push_no_screen"] = timed(lambda: ag.push_device(d_sigs[per:2 * per], d_pks[per:2 * per], d_msgs[per:2 * per],
                                                          screen=False))
    res["kernel_ms_avg_launches"] = kern
    print(json.dumps(res))
    ag.close()
    eng.close()
    base.close()
    return 0 if res["mismatches"] == 0 else 1


REMOVE_KERNELS = ("av_k_keep", "agx_k_first_changed", "agx_k_move", "ag_k_level", "ag_k_tree")


class BaselineAggregator:
    """the streaming aggregator of a build of the library given by its path, on a context of its own: reset, unscreened
    ssa_aggregator_push_device, ssa_aggregator_finish_device"""

    def __init__(self, path, capacity):
        import ctypes as C
        self.C, self.lib = C, C.CDLL(path)
        vp, sz, i32, u32 = C.c_void_p, C.c_size_t, C.c_int, C.c_uint32
        self.lib.ssa_ctx_create_ex.argtypes = [C.POINTER(vp), i32, vp, sz, u32, C.c_uint64]
        self.lib.ssa_aggregator_create.argtypes = [vp, sz, sz, u32, C.POINTER(vp)]
        self.lib.ssa_aggregator_reset.argtypes = [vp]
        self.lib.ssa_aggregator_push_device.argtypes = [vp, vp, vp, vp, vp, vp, vp, sz, sz, sz, u32, vp,
                                                        C.POINTER(C.c_uint64)]
        self.lib.ssa_aggregator_finish_device.argtypes = [vp, vp, sz, vp]
        self.lib.ssa_aggregator_destroy.argtypes = [vp]
        self.lib.ssa_aggregator_destroy.restype = None
        self.lib.ssa_ctx_sync.argtypes = [vp]
        self.lib.ssa_ctx_destroy.argtypes = [vp]
        self.lib.ssa_ctx_destroy.restype = None
        self.ctx, self.ag = vp(), vp()
        if self.lib.ssa_ctx_create_ex(C.byref(self.ctx), 0, None, 0, 0, 0) != 0:
            raise RuntimeError("baseline library: ssa_ctx_create_ex failed")
        if self.lib.ssa_aggregator_create(self.ctx, capacity, 0, 0, C.byref(self.ag)) != 0:
            raise RuntimeError("baseline library: ssa_aggregator_create failed")

    def repush(self, d_sigs, d_pks, d_msgs, per):
        """reset, then the lanes of the three tensors in unscreened pushes of `per`"""
        if self.lib.ssa_aggregator_reset(self.ag) != 0:
            raise RuntimeError("baseline library: ssa_aggregator_reset failed")
        kept, n = self.C.c_uint64(0), int(d_pks.shape[0])
        for lo in range(0, n, per):
            cnt = min(per, n - lo)
            rc = self.lib.ssa_aggregator_push_device(self.ctx, self.ag, d_sigs[lo:].data_ptr(), d_pks[lo:].data_ptr(), None,
                                                     d_msgs[lo:].data_ptr(), None, 80, 80, cnt, 1, None, self.C.byref(kept))
            if rc != 0 or kept.value != cnt:
                raise RuntimeError("baseline library: ssa_aggregator_push_device failed (%d)" % rc)

    def finish(self, d_agg):
        if self.lib.ssa_aggregator_finish_device(self.ctx, self.ag, (1 << 64) - 1, d_agg.data_ptr()) != 0:
            raise RuntimeError("baseline library: ssa_aggregator_finish_device failed")

    def sync(self):
        self.lib.ssa_ctx_sync(self.ctx)

    def close(self):
        self.lib.ssa_aggregator_destroy(self.ag)
        self.lib.ssa_ctx_destroy(self.ctx)


def accumulator_remove_main(a):
    """--accumulator --remove: removing lanes in place.  An object holds --n honest signatures
    over 80-byte messages (device buffers); the legs alternate in one process, each timed call with a stream
    synchronisation, an untimed call of the same kind in front of it, and the object reloaded before both:
      drop_front_aligned   drop_front(n / 2): the tops are moved
      drop_front_odd       drop_front(n / 2 + 1): every block is reduced again
      remove_half          remove_device of a random half
      baseline_repush      the cheapest route --baseline-lib (a build of the parent commit; without it, this tree's own
                           library) has to the state of drop_front_aligned: reset, then unscreened push_device of the
                           remaining n / 2 lanes in pushes of 2^16
    After every timed call the object's finish is compared with the aggregate the baseline library's aggregator gives
    the kept lanes.  The bar: each removal leg below baseline_repush by more than baseline_repush differs between two
    processes."""
    import torch
    import schnorr_sig_amd as ssa
    dev = torch.device("cuda", 0)
    eng = ssa.Engine(0)
    base_path = a.baseline_lib or ssa.LIB_PATH
    n, per = a.n, 1 << 16
    if n % (2 * per):
        raise SystemExit("--accumulator --remove: --n must be a multiple of 2^17")
    half = n // 2
    base = BaselineAggregator(base_path, n)
    rng = np.random.default_rng(a.seed)
    msgs = rng.integers(0, 256, (n, 80), dtype=np.uint8)
    pks, sigs = eng.keygen_sign_many(_scalars(rng, n), _scalars(rng, n), msgs)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)   # noqa: E731
    d_sigs, d_pks, d_msgs = t(sigs), t(pks), t(msgs)
    drop = np.zeros(n, np.uint8)
    drop[rng.choice(n, half, replace=False)] = 1
    d_drop, d_keep = t(drop), t(np.flatnonzero(drop == 0))
    d_agg = torch.zeros(49 * n + 32, dtype=torch.uint8, device=dev)
    sha = lambda path: hashlib.sha256(open(path, "rb").read()).hexdigest()[:16]   # noqa: E731
    res = {"metric": "aggregator_remove", "n": n, "msg_len": 80, "rounds": a.rounds, "warmup": a.warmup,
           "library_sha256": sha(ssa.LIB_PATH), "baseline_sha256": sha(base_path), "baseline_is_this_tree": not a.baseline_lib,
           "device": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d"), "mismatches": 0}
    # the kept lanes of each leg, and the baseline library's aggregate of them handed to its aggregator alone
    lanes = {"drop_front_aligned": (d_sigs[half:], d_pks[half:], d_msgs[half:]),
             "drop_front_odd": (d_sigs[half + 1:], d_pks[half + 1:], d_msgs[half + 1:]),
             "remove_half": (d_sigs[d_keep].contiguous(), d_pks[d_keep].contiguous(), d_msgs[d_keep].contiguous())}
    want = {}
    for leg, (s, p, m) in lanes.items():
        base.repush(s, p, m, per)
        want[leg] = torch.zeros(49 * int(p.shape[0]) + 32, dtype=torch.uint8, device=dev)
        base.finish(want[leg])
        base.sync()
    want["baseline_repush"] = want["drop_front_aligned"]
    ag = eng.aggregator(n)

    def wall(fn, sync):
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        return (time.perf_counter() - t0) * 1e3

    def reload():
        ag.reset()
        for lo in range(0, n, per):
            ag.push_device(d_sigs[lo:lo + per], d_pks[lo:lo + per], d_msgs[lo:lo + per], screen=False)
        eng.sync()

    calls = {"drop_front_aligned": lambda: ag.drop_front(half), "drop_front_odd": lambda: ag.drop_front(half + 1),
             "remove_half": lambda: ag.remove_device(d_drop),
             "baseline_repush": lambda: base.repush(*lanes["drop_front_aligned"], per)}
    times = {leg: [] for leg in calls}
    for rnd in range(a.warmup + a.rounds):
        for leg, call in calls.items():
            mine = leg != "baseline_repush"
            sync = eng.sync if mine else base.sync
            for timed_call in (False, True):
                if mine:
                    reload()
                ms = wall(call, sync)
            out = d_agg[:want[leg].numel()]
            out.fill_(0xEE)
            torch.cuda.synchronize()
            if mine:
                ag.finish_device(out, int((want[leg].numel() - 32) // 49))
                eng.sync()
            else:
                base.finish(out)
                base.sync()
            res["mismatches"] += 0 if bool((out == want[leg]).all()) else 1
            if rnd >= a.warmup:
                times[leg].append(ms)
    med = res["ms_median"] = {leg: round(float(np.median(v)), 3) for leg, v in times.items()}
    res["ms_all"] = {leg: [round(x, 3) for x in v] for leg, v in times.items()}
    res["ratio_to_baseline_repush"] = {leg: round(med[leg] / med["baseline_repush"], 4) for leg in calls}
    kern = {}
    for leg in ("drop_front_aligned", "drop_front_odd", "remove_half"):
        reload()
        eng.enable_timing(True)
        calls[leg]()
        eng.sync()
        kern[leg] = {}
        for kn in REMOVE_KERNELS:
            avg, cnt = eng.read_timing(kn)
            if cnt:
                kern[leg][kn] = [round(avg, 4), int(cnt)]
        eng.enable_timing(False)
    res["kernel_ms_avg_launches"] = kern
    print(json.dumps(res))
    ag.close()
    eng.close()
    base.close()
    return 0 if res["mismatches"] == 0 else 1


VERIFIER_KERNELS = ("ag_k_expand", "ssa_k_hash", "agv_k_append", "ag_k_level", "ag_k_tree", "agv_k_scalars", "msm_sort",
                    "msm_k_buckets", "msm_reduce", "msm_k_sum_records", "ag_k_finish")


class BaselineValidator:
    """ssa_verify_aggregate_sliced_device and ssa_verify_aggregate_device of a build of the library given by its path, on a
    context of its own"""

    def __init__(self, path):
        import ctypes as C
        self.C, self.lib = C, C.CDLL(path)
        vp, sz, i32 = C.c_void_p, C.c_size_t, C.c_int
        self.lib.ssa_ctx_create_ex.argtypes = [C.POINTER(vp), i32, vp, sz, C.c_uint32, C.c_uint64]
        for name in ("ssa_verify_aggregate_sliced_device", "ssa_verify_aggregate_device"):
            getattr(self.lib, name).argtypes = [vp, vp, vp, vp, vp, vp, sz, sz, sz, vp]
        self.lib.ssa_ctx_sync.argtypes = [vp]
        self.lib.ssa_ctx_destroy.argtypes = [vp]
        self.lib.ssa_ctx_destroy.restype = None
        self.ctx = vp()
        if self.lib.ssa_ctx_create_ex(C.byref(self.ctx), 0, None, 0, 0, 0) != 0:
            raise RuntimeError("baseline library: ssa_ctx_create_ex failed")

    def sliced(self, d_agg, d_pks, d_msgs, n, d_verdict):
        if self.lib.ssa_verify_aggregate_sliced_device(self.ctx, d_agg, d_pks, None, d_msgs, None, 80, 80, n, d_verdict) != 0:
            raise RuntimeError("baseline library: ssa_verify_aggregate_sliced_device failed")

    def single(self, d_agg, d_pks, d_msgs, n, d_verdict):
        if self.lib.ssa_verify_aggregate_device(self.ctx, d_agg, d_pks, None, d_msgs, None, 80, 80, n, d_verdict) != 0:
            raise RuntimeError("baseline library: ssa_verify_aggregate_device failed")

    def sync(self):
        self.lib.ssa_ctx_sync(self.ctx)

    def close(self):
        self.lib.ssa_ctx_destroy(self.ctx)


def verifier_main(a):
    """--verifier: the streaming aggregate verifier.  The block body of --n honest signatures over
    80-byte messages (R's, keys, messages: device buffers) is pushed in --pushes equal pushes; then the legs alternate in
    one process:
      finish            ssa_aggverifier_finish_device and a stream synchronisation: what is left once e_agg is known
      baseline_sliced   ssa_verify_aggregate_sliced_device through --baseline-lib (a build of the parent commit; without
                        it, this tree's own library) over the same lanes: the fastest one-shot validator call
      pushes            reset and all the pushes again, each one timed: their sum (recorded only)
    Every timed verdict is checked.  The bar: finish < baseline_sliced, by more than baseline_sliced differs between two
    processes.  Recorded beside it: the kernels of finish and of one push, and finish at 256 and 2048 lanes against
    ssa_verify_aggregate_device of the same library (the price of always taking the bucket path)."""
    import torch
    import schnorr_sig_amd as ssa
    dev = torch.device("cuda", 0)
    eng = ssa.Engine(0)
    base_path = a.baseline_lib or ssa.LIB_PATH
    base = BaselineValidator(base_path)
    n, k = a.n, a.pushes
    if n % k:
        raise SystemExit("--verifier: --n must be a multiple of --pushes")
    per = n // k
    rng = np.random.default_rng(a.seed)
    msgs = rng.integers(0, 256, (n, 80), dtype=np.uint8)
    pks, sigs = eng.keygen_sign_many(_scalars(rng, n), _scalars(rng, n), msgs)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)   # noqa: E731
    d_sigs, d_pks, d_msgs = t(sigs), t(pks), t(msgs)
    d_agg = torch.zeros(49 * n + 32, dtype=torch.uint8, device=dev)
    d_verdict = torch.full((1,), 255, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    if eng.aggregate_sliced_device(d_sigs.data_ptr(), d_pks.data_ptr(), d_msgs.data_ptr(), n, 80, d_agg.data_ptr()) != 0:
        raise SystemExit("--verifier: the honest batch did not aggregate")
    eng.sync()
    d_rs = d_agg[:49 * n].view(n, 49)
    d_e = d_agg[49 * n:]
    del d_sigs
    sha = lambda path: hashlib.sha256(open(path, "rb").read()).hexdigest()[:16]   # noqa: E731
    res = {"metric": "aggregate_verifier", "n": n, "pushes": k, "msg_len": 80, "rounds": a.rounds, "warmup": a.warmup,
           "library_sha256": sha(ssa.LIB_PATH), "baseline_sha256": sha(base_path), "baseline_is_this_tree": not a.baseline_lib,
           "device": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d"), "mismatches": 0}
    ptrs = (d_agg.data_ptr(), d_pks.data_ptr(), d_msgs.data_ptr())
    av = eng.aggregate_verifier(n)

    def wall(fn, sync):
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        return (time.perf_counter() - t0) * 1e3

    def push_all(obj=av, count=n, each=per):
        """reset, then every push timed on its own -> their times"""
        obj.reset()
        out = []
        for lo in range(0, count, each):
            sl = slice(lo, min(lo + each, count))
            out.append(wall(lambda: obj.push_device(d_rs[sl], d_pks[sl], d_msgs[sl]), eng.sync))
        if obj.info()["held"] != count:
            res["mismatches"] += 1
        return out

    def checked(ms):
        res["mismatches"] += 0 if int(d_verdict.item()) == 0 else 1
        return ms

    push_all()
    push_ms, times = [], {"finish": [], "baseline_sliced": [], "pushes": []}
    for rnd in range(a.warmup + a.rounds):
        for leg in times:
            d_verdict.fill_(255)
            torch.cuda.synchronize()
            if leg == "finish":
                ms = checked(wall(lambda: av.finish_device(d_e, d_verdict), eng.sync))
            elif leg == "baseline_sliced":
                ms = checked(wall(lambda: base.sliced(*ptrs, n, d_verdict.data_ptr()), base.sync))
            else:
                each = push_all()
                ms = float(np.sum(each))
                if rnd >= a.warmup:
                    push_ms.append(each)
                av.finish_device(d_e, d_verdict)
                eng.sync()
                checked(ms)
            if rnd >= a.warmup:
                times[leg].append(ms)
    med = res["ms_median"] = {leg: round(float(np.median(v)), 3) for leg, v in times.items()}
    res["ms_all"] = {leg: [round(x, 3) for x in v] for leg, v in times.items()}
    res["push_ms_median_by_position"] = [round(float(x), 3) for x in np.median(np.array(push_ms), axis=0)]
    res["ratio"] = {"finish/baseline_sliced": round(med["finish"] / med["baseline_sliced"], 4),
                    "(pushes+finish)/baseline_sliced": round((med["pushes"] + med["finish"]) / med["baseline_sliced"], 4)}
    res["finish_faster_than_baseline_sliced"] = bool(med["finish"] < med["baseline_sliced"])

    def timed(fn):
        eng.sync()
        eng.enable_timing(True)
        fn()
        eng.sync()
        out = {}
        for kn in VERIFIER_KERNELS:
            avg, cnt = eng.read_timing(kn)
            if cnt:
                out[kn] = [round(avg, 4), int(cnt)]
        eng.enable_timing(False)
        return out

    kern = {"finish": timed(lambda: av.finish_device(d_e, d_verdict))}
    av.reset()
    kern["push"] = timed(lambda: av.push_device(d_rs[:per], d_pks[:per], d_msgs[:per]))
    res["kernel_ms_avg_launches"] = kern
    av.close()

    # small aggregates: finish always takes the bucket path, the one-shot call takes msm_k_small up to 3072 lanes
    small = {}
    for m in (256, 2048):
        if m > n:
            continue
        d_small = torch.zeros(49 * m + 32, dtype=torch.uint8, device=dev)
        d_sg = t(sigs[:m])
        if eng.aggregate_device(d_sg.data_ptr(), d_pks.data_ptr(), d_msgs.data_ptr(), m, 80, d_small.data_ptr()) != 0:
            res["mismatches"] += 1
        eng.sync()
        sv = eng.aggregate_verifier(m)
        sv.push_device(d_small[:49 * m].view(m, 49), d_pks[:m], d_msgs[:m])
        eng.sync()
        st = {"finish": [], "baseline_single": []}
        for rnd in range(a.warmup + a.rounds):
            for leg in st:
                d_verdict.fill_(255)
                torch.cuda.synchronize()
                if leg == "finish":
                    ms = checked(wall(lambda: sv.finish_device(d_small[49 * m:], d_verdict), eng.sync))
                else:
                    ms = checked(wall(lambda: base.single(d_small.data_ptr(), d_pks.data_ptr(), d_msgs.data_ptr(), m,
                                                          d_verdict.data_ptr()), base.sync))
                if rnd >= a.warmup:
                    st[leg].append(ms)
        small[str(m)] = {leg: round(float(np.median(v)), 4) for leg, v in st.items()}
        sv.close()
    res["small_ms_median"] = small
    print(json.dumps(res))
    eng.close()
    base.close()
    return 0 if res["mismatches"] == 0 else 1


CACHED_PUSH_KERNELS = ("dedup", "keycache_lookup", "keycache_insert", "keycache_map", "ssa_k_keyset_build",
                       "ssa_k_keyed_decompress", "agc_expand", "ag_k_expand", "ssa_k_hash", "agv_k_append", "ag_k_level", "ag_k_tree")


class BaselineStream:
    """the streaming verifier and ssa_decompress_many_device of a build of the library given by its path (the parent
    commit's: plain pushes only), on a context of its own"""

    def __init__(self, path, capacity):
        import ctypes as C
        self.C, self.lib = C, C.CDLL(path)
        vp, sz, i32 = C.c_void_p, C.c_size_t, C.c_int
        self.lib.ssa_ctx_create_ex.argtypes = [C.POINTER(vp), i32, vp, sz, C.c_uint32, C.c_uint64]
        self.lib.ssa_aggverifier_create.argtypes = [vp, sz, sz, C.c_uint32, C.POINTER(vp)]
        self.lib.ssa_aggverifier_push_device.argtypes = [vp, vp, vp, vp, vp, vp, vp, sz, sz, sz]
        self.lib.ssa_aggverifier_finish_device.argtypes = [vp, vp, vp, sz, vp]
        self.lib.ssa_aggverifier_reset.argtypes = [vp]
        self.lib.ssa_aggverifier_destroy.argtypes = [vp]
        self.lib.ssa_aggverifier_destroy.restype = None
        self.lib.ssa_decompress_many_device.argtypes = [vp, vp, sz, vp, vp, vp]
        self.lib.ssa_ctx_enable_timing.argtypes = [vp, i32]
        self.lib.ssa_ctx_read_timing.argtypes = [vp, C.c_char_p, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]
        self.lib.ssa_ctx_sync.argtypes = [vp]
        self.lib.ssa_ctx_destroy.argtypes = [vp]
        self.lib.ssa_ctx_destroy.restype = None
        self.ctx, self.av = vp(), vp()
        if self.lib.ssa_ctx_create_ex(C.byref(self.ctx), 0, None, 0, 0, 0) != 0:
            raise RuntimeError("baseline library: ssa_ctx_create_ex failed")
        if self.lib.ssa_aggverifier_create(self.ctx, capacity, 0, 0, C.byref(self.av)) != 0:
            raise RuntimeError("baseline library: ssa_aggverifier_create failed")

    def reset(self):
        self.lib.ssa_aggverifier_reset(self.av)

    def decompress_push(self, d_rs, d_wk, d_msgs, n, d_upks, d_uinf, d_ust):
        """the parent's route for a block body with wire keys: ssa_decompress_many_device, then the plain push"""
        if self.lib.ssa_decompress_many_device(self.ctx, d_wk, n, d_upks, d_uinf, d_ust) != 0:
            raise RuntimeError("baseline library: ssa_decompress_many_device failed")
        if self.lib.ssa_aggverifier_push_device(self.ctx, self.av, d_rs, d_upks, d_uinf, d_msgs, None, 80, 80, n) != 0:
            raise RuntimeError("baseline library: ssa_aggverifier_push_device failed")

    def finish(self, d_e, d_verdict):
        if self.lib.ssa_aggverifier_finish_device(self.ctx, self.av, d_e, self.C.c_size_t(-1).value, d_verdict) != 0:
            raise RuntimeError("baseline library: ssa_aggverifier_finish_device failed")

    def timed_finish(self, d_e, d_verdict, names):
        """one finish under ssa_ctx_enable_timing -> {kernel: [ms per timed region, regions]}"""
        C = self.C
        self.sync()
        self.lib.ssa_ctx_enable_timing(self.ctx, 1)
        self.finish(d_e, d_verdict)
        self.sync()
        out = {}
        for kn in names:
            avg, cnt = C.c_double(0), C.c_uint64(0)
            self.lib.ssa_ctx_read_timing(self.ctx, kn.encode(), C.byref(avg), C.byref(cnt))
            if cnt.value:
                out[kn] = [round(avg.value, 4), int(cnt.value)]
        self.lib.ssa_ctx_enable_timing(self.ctx, 0)
        return out

    def sync(self):
        self.lib.ssa_ctx_sync(self.ctx)

    def close(self):
        self.lib.ssa_aggverifier_destroy(self.av)
        self.lib.ssa_ctx_destroy(self.ctx)


def verifier_cached_main(a):
    """--verifier --cached: the streaming verifier through the key cache.  --n honest lanes by
    --signers signers (0: every lane its own) over 80-byte messages, device buffers, pushed in --pushes equal pushes with
    49-byte wire keys.  Legs alternating in one process:
      finish_keyed      ssa_aggverifier_finish_device of the keyed object (the fold of the key statuses included)
      finish_plain      ssa_aggverifier_finish_device of a second object of THIS library on the same context, the same
                        lanes pushed plainly: keyed against plain with everything else equal
      finish_baseline   ssa_aggverifier_finish_device of --baseline-lib (a build of the parent commit; without it, this
                        tree's own library) over the same lanes, pushed plainly behind ssa_decompress_many_device
      push_wire_warm    reset, all the pushes through the warm wire cache: their sum
      push_baseline     reset, per push ssa_decompress_many_device + the plain push of --baseline-lib: their sum
    and once, in front, push_wire_cold (the same pushes into the empty cache).  Every timed verdict is checked.  The bar:
    finish_keyed exceeds finish_baseline by no more than the larger of that leg's spread between two processes and the
    timed duration of agv_k_key_verdict.  The pushes are recorded and have no bar."""
    import torch
    import schnorr_sig_amd as ssa
    dev = torch.device("cuda", 0)
    n, k = a.n, a.pushes
    if n % k:
        raise SystemExit("--verifier: --n must be a multiple of --pushes")
    if a.signers < 0 or a.signers > n:
        raise SystemExit("--signers must lie in [0, --n = %d]" % n)
    per, signers = n // k, a.signers or n
    # the lanes are made on a context of their own, which is closed before anything is timed: the timed object lives on a
    # context that has done nothing else, as the baseline's does (a context that has signed and aggregated 2^20 lanes
    # holds MSM workspaces of another history, and msm_k_buckets of its finish runs 0.1 ms slower: profiles/r25/)
    gen = ssa.Engine(0)
    base_path = a.baseline_lib or ssa.LIB_PATH
    base = BaselineStream(base_path, n)
    rng = np.random.default_rng(a.seed)
    msgs = rng.integers(0, 256, (n, 80), dtype=np.uint8)
    idx = rng.integers(0, signers, size=n)
    idx[:signers] = np.arange(signers)
    rng.shuffle(idx)
    pks, sigs = gen.keygen_sign_many(_scalars(rng, signers)[idx], _scalars(rng, n), msgs)
    wire_keys, st = gen.compress_many(pks)
    assert (st == 0).all()
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)   # noqa: E731
    d_sigs, d_pks, d_msgs, d_wk = t(sigs), t(pks), t(msgs), t(wire_keys)
    d_agg = torch.zeros(49 * n + 32, dtype=torch.uint8, device=dev)
    d_upks = torch.zeros(96 * per, dtype=torch.uint8, device=dev)      # what the baseline's decompression writes, per push
    d_uinf = torch.zeros(per, dtype=torch.uint8, device=dev)
    d_ust = torch.zeros(per, dtype=torch.uint8, device=dev)
    d_verdict = torch.full((1,), 255, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    if gen.aggregate_sliced_device(d_sigs.data_ptr(), d_pks.data_ptr(), d_msgs.data_ptr(), n, 80, d_agg.data_ptr()) != 0:
        raise SystemExit("--verifier --cached: the honest batch did not aggregate")
    gen.sync()
    gen.close()
    eng = ssa.Engine(0)
    d_rs, d_e = d_agg[:49 * n].view(n, 49), d_agg[49 * n:]
    del d_sigs, d_pks
    sha = lambda path: hashlib.sha256(open(path, "rb").read()).hexdigest()[:16]   # noqa: E731
    res = {"metric": "aggregate_verifier_cached", "n": n, "pushes": k, "signers": signers, "msg_len": 80, "rounds": a.rounds,
           "warmup": a.warmup, "library_sha256": sha(ssa.LIB_PATH), "baseline_sha256": sha(base_path),
           "baseline_is_this_tree": not a.baseline_lib, "device": torch.cuda.get_device_name(0),
           "date": time.strftime("%Y-%m-%d"), "mismatches": 0}
    av, cache = eng.aggregate_verifier(n), eng.keycache_create(signers, wire=True)
    stats = np.zeros(8, dtype=np.uint64)
    # finish_plain: a second object of THIS library on the keyed object's context, the same lanes pushed plainly (keys
    # decompressed once, outside the timed region): keyed against plain with everything else equal
    av_plain = eng.aggregate_verifier(n)
    d_upks_all = torch.zeros((n, 96), dtype=torch.uint8, device=dev)
    d_uinf_all = torch.zeros(n, dtype=torch.uint8, device=dev)
    d_ust_all = torch.zeros(n, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    if ssa._lib.ssa_decompress_many_device(eng._ctx, d_wk.data_ptr(), n, d_upks_all.data_ptr(), d_uinf_all.data_ptr(),
                                           d_ust_all.data_ptr()) != 0:
        raise SystemExit("--verifier --cached: ssa_decompress_many_device failed")
    for lo in range(0, n, per):
        av_plain.push_device(d_rs[lo:lo + per], d_upks_all[lo:lo + per], d_msgs[lo:lo + per], d_pk_inf=d_uinf_all[lo:lo + per])
    eng.sync()
    if av_plain.info()["held"] != n or av_plain.info()["reserved"] != 0:
        raise SystemExit("--verifier --cached: the plain object did not take the lanes")

    def wall(fn, sync):
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        return (time.perf_counter() - t0) * 1e3

    def push_keyed():
        av.reset()
        stats[:] = 0
        out = []
        for lo in range(0, n, per):
            sl = slice(lo, lo + per)
            got = []
            out.append(wall(lambda: got.append(av.push_wire_device(d_rs[sl], d_wk[sl], d_msgs[sl], cache=cache)[1]), eng.sync))
            stats[:] += got[0]
        if av.info()["held"] != n or av.info()["reserved"] != n:
            res["mismatches"] += 1
        return out

    def push_base():
        base.reset()
        out = []
        for lo in range(0, n, per):
            out.append(wall(lambda: base.decompress_push(d_rs.data_ptr() + 49 * lo, d_wk.data_ptr() + 49 * lo,
                                                         d_msgs.data_ptr() + 80 * lo, per, d_upks.data_ptr(), d_uinf.data_ptr(),
                                                         d_ust.data_ptr()), base.sync))
        return out

    def checked(ms):
        res["mismatches"] += 0 if int(d_verdict.item()) == 0 else 1
        return ms

    cold = push_keyed()
    res["push_wire_cold_ms"] = round(float(np.sum(cold)), 3)
    res["stats_cold"] = [int(x) for x in stats]
    push_base()
    times = {"finish_keyed": [], "finish_plain": [], "finish_baseline": [], "push_wire_warm": [], "push_baseline": []}
    # --rotate-legs (a diagnostic): the two finish legs and the two push legs swap places every other round, and the times
    # are also recorded by the order of the round (0: as listed, 1: swapped)
    by_place = {leg: [[], []] for leg in times}
    orders = [list(times), ["finish_baseline", "finish_plain", "finish_keyed", "push_baseline", "push_wire_warm"]]
    for rnd in range(a.warmup + a.rounds):
        order = orders[rnd % 2] if a.rotate_legs else orders[0]
        for leg in order:
            d_verdict.fill_(255)
            torch.cuda.synchronize()
            if leg.startswith("finish"):
                # every timed finish follows one untimed finish of the same object: whichever finish is the first heavy
                # work behind the push legs runs msm_k_buckets about 0.1 ms slower (profiles/r25/: runs 1 to 4), and
                # without this the first leg of the round would carry that
                fn, sync = {"finish_keyed": (lambda: av.finish_device(d_e, d_verdict), eng.sync),
                            "finish_plain": (lambda: av_plain.finish_device(d_e, d_verdict), eng.sync),
                            "finish_baseline": (lambda: base.finish(d_e.data_ptr(), d_verdict.data_ptr()), base.sync)}[leg]
                fn()
                sync()
                d_verdict.fill_(255)
                torch.cuda.synchronize()
                ms = checked(wall(fn, sync))
            elif leg == "push_wire_warm":
                ms = float(np.sum(push_keyed()))
                av.finish_device(d_e, d_verdict)
                eng.sync()
                checked(ms)
            else:
                ms = float(np.sum(push_base()))
                base.finish(d_e.data_ptr(), d_verdict.data_ptr())
                base.sync()
                checked(ms)
            if rnd >= a.warmup:
                times[leg].append(ms)
                by_place[leg][0 if order is orders[0] else 1].append(round(ms, 3))
    if a.rotate_legs:
        res["rotated_ms_by_place"] = by_place
    res["stats_warm"] = [int(x) for x in stats]
    med = res["ms_median"] = {leg: round(float(np.median(v)), 3) for leg, v in times.items()}
    res["ms_all"] = {leg: [round(x, 3) for x in v] for leg, v in times.items()}
    res["ratio"] = {"finish_keyed/finish_baseline": round(med["finish_keyed"] / med["finish_baseline"], 4),
                    "push_wire_warm/push_baseline": round(med["push_wire_warm"] / med["push_baseline"], 4)}
    res["finish_keyed_minus_baseline_ms"] = round(med["finish_keyed"] - med["finish_baseline"], 4)
    res["finish_keyed_minus_plain_ms"] = round(med["finish_keyed"] - med["finish_plain"], 4)

    def timed(fn, names):
        eng.sync()
        eng.enable_timing(True)
        fn()
        eng.sync()
        out = {}
        for kn in names:
            avg, cnt = eng.read_timing(kn)
            if cnt:
                out[kn] = [round(avg, 4), int(cnt)]
        eng.enable_timing(False)
        return out

    kern = {"finish": timed(lambda: av.finish_device(d_e, d_verdict), VERIFIER_KERNELS + ("agv_k_key_verdict",)),
            "finish_plain": timed(lambda: av_plain.finish_device(d_e, d_verdict), VERIFIER_KERNELS + ("agv_k_key_verdict",)),
            "finish_baseline": base.timed_finish(d_e.data_ptr(), d_verdict.data_ptr(), VERIFIER_KERNELS)}
    av.reset()
    kern["push_warm"] = timed(lambda: av.push_wire_device(d_rs[:per], d_wk[:per], d_msgs[:per], cache=cache), CACHED_PUSH_KERNELS)
    res["kernel_ms_avg_launches"] = kern
    print(json.dumps(res))
    av.close()
    av_plain.close()
    cache.close()
    eng.close()
    base.close()
    return 0 if res["mismatches"] == 0 else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seed", type=int, default=0xA66)
    ap.add_argument("--many", action="append", default=[], metavar="KxS",
                    help="K aggregates of S signatures in one ssa_verify_aggregates_many call (repeatable)")
    ap.add_argument("--baseline-lib", default=None,
                    help="another build of the library for the loop_baseline leg (--many) or the baseline legs (--valid, "
                         "--cached)")
    ap.add_argument("--valid", action="store_true",
                    help="ssa_aggregate_valid_many_device against the checked call (and the unchecked one on filtered arrays)")
    ap.add_argument("--cached", action="store_true",
                    help="ssa_verify_aggregates_many_cached(_wire)_device against decompress + ssa_verify_aggregates_many; "
                         "with --verifier: the pushes through a wire key cache and the keyed finish against the plain "
                         "verifier of --baseline-lib")
    ap.add_argument("--valid-cached", action="store_true",
                    help="ssa_aggregate_valid_(keyed_)many_cached_device against ssa_aggregate_valid_many_device and against "
                         "ssa_verify_many_cached_device + ssa_aggregate_many_device on filtered arrays")
    ap.add_argument("--signers", type=int, default=65536,
                    help="--cached, --valid-cached, --verifier --cached: distinct signers (0: every lane its own)")
    ap.add_argument("--sharded", action="store_true",
                    help="ssa_aggregate_many_sliced_device / ssa_verify_aggregate_sliced_device against the single calls of "
                         "--baseline-lib")
    ap.add_argument("--multi", action="store_true", help="--sharded: also MultiEngine([0, 0]) from host buffers")
    ap.add_argument("--produce-many", nargs="?", const="4096x256", default=None, metavar="KxS",
                    help="ssa_aggregates_many_device over K batches of S signatures against K ssa_aggregate_many_device "
                         "calls of --baseline-lib")
    ap.add_argument("--accumulator", action="store_true",
                    help="ssa_aggregator_finish_device after --pushes pushes against ssa_aggregate_many_sliced_device of "
                         "--baseline-lib over the same --n signatures")
    ap.add_argument("--verifier", action="store_true",
                    help="ssa_aggverifier_finish_device after --pushes pushes against ssa_verify_aggregate_sliced_device of "
                         "--baseline-lib over the same --n lanes")
    ap.add_argument("--pushes", type=int, default=16,
                    help="--accumulator, --verifier: equal pushes the --n signatures arrive in")
    ap.add_argument("--rotate-legs", action="store_true",
                    help="--verifier --cached: a diagnostic -- swap each leg with its counterpart every other round and "
                         "record the times by place as well")
    ap.add_argument("--remove", action="store_true",
                    help="--accumulator: drop_front and remove_device on an object of --n lanes (DESIGN.md section 30) "
                         "against reset + unscreened pushes of the remaining half through --baseline-lib")
    a = ap.parse_args()
    if a.verifier:
        return verifier_cached_main(a) if a.cached else verifier_main(a)
    if a.accumulator:
        return accumulator_remove_main(a) if a.remove else accumulator_main(a)
    if a.produce_many:
        return produce_many_main(a)
    if a.sharded:
        return sharded_main(a)
    if a.valid_cached:
        return valid_cached_main(a)
    if a.cached:
        return cached_main(a)
    if a.many:
        return many_main(a)
    if a.valid:
        return valid_main(a)
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
