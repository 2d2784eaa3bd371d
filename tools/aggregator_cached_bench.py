#!/usr/bin/env python3
"""The streaming aggregator through the key cache, and its key column, measured on one GPU.

    python tools/aggregator_cached_bench.py --baseline-lib /path/to/parent/libschnorr_sig_amd.so [--n 1048576]
                                            [--signers 65536] [--rounds 7] [--warmup 2]

--n honest KeyedSignature records by --signers signers over 80-byte messages, in device buffers.  --baseline-lib is a
build of the parent commit (without it this tree's own library stands in, and the comparison says nothing).  The legs
alternate in one process; each timed call has an untimed call of the same kind in front of it in every round, starts
behind a stream synchronisation and ends with one; the medians and all samples are printed as one JSON line.

  (a) push_keyed_warm        reset, then ONE ssa_aggregator_push_keyed_cached_device of all n records, cache warm
      parent_one_shot_warm   the parent's ssa_aggregate_valid_keyed_many_cached_device on the same input, cache warm
  (b) finish_and_keys        ssa_aggregator_finish_device + ssa_aggregator_keys_device of all n lanes (a key column)
      finish                 ssa_aggregator_finish_device alone on the same object
  (c) drop_front_odd_keys    drop_front(n / 2 + 1) on the object with a key column
      remove_half_keys       remove_device of a random half on it
  (d) the object made with flags 0, this tree against the parent, both driven through the same ctypes calls (class
      Parent below, once on each library: a push synchronises, so the host's part of a call is on the timed path):
      plain_push / parent_plain_push     reset, then unscreened ssa_aggregator_push_device in pushes of 2^16
      plain_finish / parent_plain_finish
      plain_remove / parent_plain_remove remove_device of the same random half

After every timed call the outputs are compared: the push's finish and keys with the parent's one-shot aggregate and the
records' first 49 bytes, the removals' with the parent's aggregator over the kept lanes."""
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
PER = 1 << 16
KERNELS = ("ssa_k_hash", "ssa_k_keyed_decompress", "ssa_k_keyset_build", "av_k_keep", "agx_k_append", "ag_k_tree",
           "agx_k_move", "agx_k_coeff_fold", "ag_k_fold_finish")


def _scalars(rng, n):
    s = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    s[:, 31] &= 0x3F
    s[:, 0] |= 1
    return s


class Parent:
    """the calls of a build of the library given by its path, on a context, a wire key cache (cache_rows != 0) and an
    aggregator (flags 0) of its own"""

    def __init__(self, path, n, cache_rows):
        vp, sz, i32, u32, u64p = C.c_void_p, C.c_size_t, C.c_int, C.c_uint32, C.POINTER(C.c_uint64)
        lib = self.lib = C.CDLL(path)
        lib.ssa_ctx_create_ex.argtypes = [C.POINTER(vp), i32, vp, sz, u32, C.c_uint64]
        lib.ssa_keycache_create_ex.argtypes = [vp, sz, u32, C.POINTER(vp)]
        lib.ssa_aggregate_valid_keyed_many_cached_device.argtypes = [vp, vp, vp, vp, vp, sz, sz, sz, vp, vp, u64p, vp, vp, vp]
        lib.ssa_aggregator_create.argtypes = [vp, sz, sz, u32, C.POINTER(vp)]
        lib.ssa_aggregator_reset.argtypes = [vp]
        lib.ssa_aggregator_push_device.argtypes = [vp, vp, vp, vp, vp, vp, vp, sz, sz, sz, u32, vp, u64p]
        lib.ssa_aggregator_finish_device.argtypes = [vp, vp, sz, vp]
        lib.ssa_aggregator_remove_device.argtypes = [vp, vp, vp, sz, u64p]
        for name in ("ssa_aggregator_destroy", "ssa_keycache_destroy", "ssa_ctx_destroy"):
            getattr(lib, name).argtypes, getattr(lib, name).restype = [vp], None
        lib.ssa_ctx_sync.argtypes = [vp]
        self.ctx, self.kc, self.ag = vp(), vp(), vp()
        if lib.ssa_ctx_create_ex(C.byref(self.ctx), 0, None, 0, 0, 0) != 0:
            raise RuntimeError("baseline library: ssa_ctx_create_ex failed")
        if cache_rows and lib.ssa_keycache_create_ex(self.ctx, cache_rows, 1, C.byref(self.kc)) != 0:    # SSA_KEYCACHE_WIRE
            raise RuntimeError("baseline library: ssa_keycache_create_ex failed")
        if lib.ssa_aggregator_create(self.ctx, n, 0, 0, C.byref(self.ag)) != 0:
            raise RuntimeError("baseline library: ssa_aggregator_create failed")

    def one_shot(self, d_rec, d_msgs, n, d_agg, d_kept, d_keys):
        m = C.c_uint64(0)
        rc = self.lib.ssa_aggregate_valid_keyed_many_cached_device(self.ctx, self.kc, d_rec.data_ptr(), d_msgs.data_ptr(), None,
                                                                   80, 80, n, d_agg.data_ptr(), d_kept.data_ptr(), C.byref(m),
                                                                   None, d_keys.data_ptr(), None)
        if rc != 0:
            raise RuntimeError("baseline library: ssa_aggregate_valid_keyed_many_cached_device failed (%d)" % rc)
        return int(m.value)

    def repush(self, d_sigs, d_pks, d_msgs):
        if self.lib.ssa_aggregator_reset(self.ag) != 0:
            raise RuntimeError("baseline library: ssa_aggregator_reset failed")
        kept, n = C.c_uint64(0), int(d_pks.shape[0])
        for lo in range(0, n, PER):
            cnt = min(PER, n - lo)
            rc = self.lib.ssa_aggregator_push_device(self.ctx, self.ag, d_sigs[lo:].data_ptr(), d_pks[lo:].data_ptr(), None,
                                                     d_msgs[lo:].data_ptr(), None, 80, 80, cnt, 1, None, C.byref(kept))
            if rc != 0 or kept.value != cnt:
                raise RuntimeError("baseline library: ssa_aggregator_push_device failed (%d)" % rc)

    def finish(self, d_agg):
        if self.lib.ssa_aggregator_finish_device(self.ctx, self.ag, (1 << 64) - 1, d_agg.data_ptr()) != 0:
            raise RuntimeError("baseline library: ssa_aggregator_finish_device failed")

    def remove(self, d_drop):
        kept = C.c_uint64(0)
        if self.lib.ssa_aggregator_remove_device(self.ctx, self.ag, d_drop.data_ptr(), int(d_drop.numel()), C.byref(kept)) != 0:
            raise RuntimeError("baseline library: ssa_aggregator_remove_device failed")
        return int(kept.value)

    def sync(self):
        self.lib.ssa_ctx_sync(self.ctx)

    def close(self):
        self.lib.ssa_aggregator_destroy(self.ag)
        if self.kc:
            self.lib.ssa_keycache_destroy(self.kc)
        self.lib.ssa_ctx_destroy(self.ctx)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--signers", type=int, default=65536)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=0xA66)
    ap.add_argument("--baseline-lib", default=None, help="a build of the parent commit's library")
    a = ap.parse_args()
    import torch
    import schnorr_sig_amd as ssa
    dev = torch.device("cuda", 0)
    n, signers = a.n, min(a.signers, a.n)
    if n % (2 * PER):
        raise SystemExit("--n must be a multiple of 2^17")
    half = n // 2
    eng = ssa.Engine(0)
    base_path = a.baseline_lib or ssa.LIB_PATH
    par, mine = Parent(base_path, n, signers + 16), Parent(ssa.LIB_PATH, n, 0)
    rng = np.random.default_rng(a.seed)
    msgs = rng.integers(0, 256, (n, 80), dtype=np.uint8)
    idx = rng.integers(0, signers, size=n)
    idx[:signers] = np.arange(signers)
    rng.shuffle(idx)
    pks, sigs = eng.keygen_sign_many(_scalars(rng, signers)[idx], _scalars(rng, n), msgs)
    wire, st = eng.compress_many(pks)
    assert (np.asarray(st) == 0).all()
    rec = np.concatenate([np.asarray(wire, np.uint8).reshape(n, 49), sigs], axis=1)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)   # noqa: E731
    d_sigs, d_pks, d_msgs, d_rec = t(sigs), t(pks), t(msgs), t(rec)
    d_wire = d_rec[:, :49].contiguous()
    drop = np.zeros(n, np.uint8)
    drop[rng.choice(n, half, replace=False)] = 1
    keep = np.flatnonzero(drop == 0)
    d_drop, d_keep = t(drop), t(keep)
    buf = lambda size: torch.zeros(size, dtype=torch.uint8, device=dev)   # noqa: E731
    d_agg, d_agg2, d_keys, d_keys2 = buf(49 * n + 32), buf(49 * n + 32), buf(49 * n), buf(49 * n)
    d_kept = torch.zeros(n, dtype=torch.int32, device=dev)
    sha = lambda path: hashlib.sha256(open(path, "rb").read()).hexdigest()[:16]   # noqa: E731
    res = {"metric": "aggregator_cached", "n": n, "signers": signers, "msg_len": 80, "rounds": a.rounds, "warmup": a.warmup,
           "library_sha256": sha(ssa.LIB_PATH), "baseline_sha256": sha(base_path), "baseline_is_this_tree": not a.baseline_lib,
           "device": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d"), "mismatches": 0}
    # expected values, from the parent alone: the one-shot aggregate of all lanes, and its aggregator's over the kept ones
    d_want = buf(49 * n + 32)
    assert par.one_shot(d_rec, d_msgs, n, d_want, d_kept, d_keys2) == n          # (and the parent's cache is warm)
    want_lanes = {"odd": (d_sigs[half + 1:], d_pks[half + 1:], d_msgs[half + 1:], d_wire[half + 1:]),
                  "half": tuple(x[d_keep].contiguous() for x in (d_sigs, d_pks, d_msgs, d_wire))}
    want = {}
    for k, (s, p, m, w) in want_lanes.items():
        par.repush(s, p, m)
        want[k] = buf(49 * int(p.shape[0]) + 32)
        par.finish(want[k])
    par.sync()
    cache = eng.keycache_create(signers + 16, wire=True)
    held = eng.aggregator(n, hold_keys=True)
    stats = {}

    def push_keyed():
        stats["m"], stats["stats"] = held.push_keyed_device(cache, d_rec, d_msgs)

    def reload_held():
        held.reset()
        push_keyed()
        eng.sync()

    def plain_result(lib, key):
        """the finish of everything the library's flags-0 object holds, against the expectation"""
        w = d_want if key == "all" else want[key]
        d_agg2.fill_(0xEE)
        torch.cuda.synchronize()
        lib.finish(d_agg2[:w.numel()])
        lib.sync()
        return bool((d_agg2[:w.numel()] == w).all())

    def finish_and_keys():
        held.finish_device(d_agg)
        held.keys_device(d_keys)

    def check_object(ag, key, keys):
        """finish (and keys) of everything the object holds against want[key] / the kept keys"""
        m = len(ag)
        d_agg2.fill_(0xEE)
        d_keys2.fill_(0xEE)
        torch.cuda.synchronize()
        ag.finish_device(d_agg2[:49 * m + 32])
        good = True
        if keys is not None:
            ag.keys_device(d_keys2[:49 * m])
            eng.sync()
            good = bool((d_keys2[:49 * m] == keys.reshape(-1)).all())
        eng.sync()
        w = d_want if key == "all" else want[key]
        return good and w.numel() == 49 * m + 32 and bool((d_agg2[:49 * m + 32] == w).all())

    # leg: (prepare, timed call, its sync, check)
    legs = {
        "push_keyed_warm": (held.reset, push_keyed, eng.sync, lambda: stats["m"] == n and int(stats["stats"][9]) == 0 and check_object(held, "all", d_wire)),
        "parent_one_shot_warm": (lambda: None, lambda: par.one_shot(d_rec, d_msgs, n, d_agg, d_kept, d_keys), par.sync,
                                 lambda: bool((d_agg == d_want).all()) and bool((d_keys == d_wire.reshape(-1)).all())),
        "finish_and_keys": (reload_held, finish_and_keys, eng.sync,
                            lambda: bool((d_agg == d_want).all()) and bool((d_keys == d_wire.reshape(-1)).all())),
        "finish": (lambda: None, lambda: held.finish_device(d_agg), eng.sync, lambda: bool((d_agg == d_want).all())),
        "drop_front_odd_keys": (reload_held, lambda: held.drop_front(half + 1), eng.sync,
                                lambda: check_object(held, "odd", want_lanes["odd"][3])),
        "remove_half_keys": (reload_held, lambda: held.remove_device(d_drop), eng.sync,
                             lambda: check_object(held, "half", want_lanes["half"][3])),
    }
    for name, lib in (("plain", mine), ("parent_plain", par)):
        legs[name + "_push"] = (lambda: None, lambda lib=lib: lib.repush(d_sigs, d_pks, d_msgs), lib.sync,
                                lambda lib=lib: plain_result(lib, "all"))
        legs[name + "_finish"] = (lambda: None, lambda lib=lib: lib.finish(d_agg), lib.sync, lambda: bool((d_agg == d_want).all()))
        legs[name + "_remove"] = (lambda lib=lib: lib.repush(d_sigs, d_pks, d_msgs), lambda lib=lib: lib.remove(d_drop), lib.sync,
                                  lambda lib=lib: plain_result(lib, "half"))
    reload_held()
    times = {leg: [] for leg in legs}
    for rnd in range(a.warmup + a.rounds):
        for leg, (prepare, call, sync, check) in legs.items():
            ms = 0.0
            for timed in (False, True):
                prepare()
                d_agg.fill_(0xEE)
                d_keys.fill_(0xEE)
                eng.sync()
                par.sync()
                mine.sync()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                call()
                sync()
                ms = (time.perf_counter() - t0) * 1e3
            res["mismatches"] += 0 if check() else 1
            if leg in ("drop_front_odd_keys", "remove_half_keys"):
                reload_held()
            if rnd >= a.warmup:
                times[leg].append(ms)
    med = res["ms_median"] = {leg: round(float(np.median(v)), 3) for leg, v in times.items()}
    res["ms_min"] = {leg: round(float(np.min(v)), 3) for leg, v in times.items()}
    res["ms_max"] = {leg: round(float(np.max(v)), 3) for leg, v in times.items()}
    res["ms_all"] = {leg: [round(x, 3) for x in v] for leg, v in times.items()}
    res["ratio"] = {"push_keyed_warm/parent_one_shot_warm": round(med["push_keyed_warm"] / med["parent_one_shot_warm"], 4),
                    "plain_push/parent": round(med["plain_push"] / med["parent_plain_push"], 4),
                    "plain_finish/parent": round(med["plain_finish"] / med["parent_plain_finish"], 4),
                    "plain_remove/parent": round(med["plain_remove"] / med["parent_plain_remove"], 4)}
    kern = {}
    for leg in ("push_keyed_warm", "finish_and_keys", "drop_front_odd_keys", "remove_half_keys"):
        prepare, call, sync, _ = legs[leg]
        prepare()
        eng.sync()
        eng.enable_timing(True)
        for kn in KERNELS:
            eng.read_timing(kn)
        call()
        sync()
        kern[leg] = {}
        for kn in KERNELS:
            avg, cnt = eng.read_timing(kn)
            if cnt:
                kern[leg][kn] = [round(avg, 4), int(cnt)]
        eng.enable_timing(False)
        reload_held()
    res["kernel_ms_avg_launches"] = kern
    print(json.dumps(res))
    for h in (held, cache):
        h.close()
    eng.close()
    par.close()
    mine.close()
    return 0 if res["mismatches"] == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
