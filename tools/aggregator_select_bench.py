#!/usr/bin/env python3
"""Selections of held lanes (finish_select, remove_indices), measured on one GPU.

    python tools/aggregator_select_bench.py --baseline-lib /path/to/parent/libschnorr_sig_amd.so [--n 1048576]
                                            [--signers 65536] [--rounds 3] [--warmup 1]

--n honest KeyedSignature records by --signers signers over 80-byte messages are held by an aggregator with a key column,
admitted through a warm wire key cache.  --baseline-lib is a build of the parent commit (without it this tree's own
library stands in, and the comparison says nothing).  The legs alternate in one process; each timed call has an untimed
call of the same kind in front of it in every round, starts behind a stream synchronisation and ends with one; the
medians and all samples are printed as one JSON line.

  (a) select_all             finish_select_device with keys for a random permutation of all n lanes
      parent_many_all        the parent's ssa_aggregate_many_device on the same lanes, whose signatures, keys and messages
      parent_sliced_all      are already gathered in device memory in that order; ssa_aggregate_many_sliced_device
  (b) select_half / parent_many_half / parent_sliced_half     the same for a random n / 2 lanes in random order
  (c) finish_and_keys        finish_device + keys_device of all n lanes: the arrival-order block, for scale
  (d) remove_indices_half    remove_indices_device of a random n / 2 lanes
      remove_mask_half       remove_device with the equivalent mask, on the same object and the same run

The comparison for finish_select is, per round, the faster of the parent's two calls ("pairings").  After every timed call
the outputs are compared: the selection's aggregate with the parent's one-shot aggregate of the selected lanes, its keys
with the records' first 49 bytes in the list's order, the removals' finish and keys with those of the kept lanes."""
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
KERNELS = ("agx_k_select", "ag_k_tree", "agx_k_coeff_fold", "ag_k_fold_finish", "agx_k_select_verdict", "agx_k_mark",
           "agx_k_bits_to_mask", "av_k_keep", "agx_k_first_changed", "agx_k_move")


def _scalars(rng, n):
    s = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    s[:, 31] &= 0x3F
    s[:, 0] |= 1
    return s


class Parent:
    """the one-shot producer calls of a build of the library given by its path, on a context of its own"""

    def __init__(self, path):
        vp, sz, i32, u32 = C.c_void_p, C.c_size_t, C.c_int, C.c_uint32
        lib = self.lib = C.CDLL(path)
        lib.ssa_ctx_create_ex.argtypes = [C.POINTER(vp), i32, vp, sz, u32, C.c_uint64]
        for name in ("ssa_aggregate_many_device", "ssa_aggregate_many_sliced_device"):
            getattr(lib, name).argtypes = [vp, vp, vp, vp, vp, vp, sz, sz, sz, u32, vp, vp, vp]
        lib.ssa_ctx_destroy.argtypes, lib.ssa_ctx_destroy.restype = [vp], None
        lib.ssa_ctx_sync.argtypes = [vp]
        self.ctx = vp()
        if lib.ssa_ctx_create_ex(C.byref(self.ctx), 0, None, 0, 0, 0) != 0:
            raise RuntimeError("baseline library: ssa_ctx_create_ex failed")

    def aggregate(self, lanes, d_agg, sliced=False):
        d_sigs, d_pks, d_msgs = lanes
        fn = self.lib.ssa_aggregate_many_sliced_device if sliced else self.lib.ssa_aggregate_many_device
        rc = fn(self.ctx, d_sigs.data_ptr(), d_pks.data_ptr(), None, d_msgs.data_ptr(), None, 80, 80, int(d_pks.shape[0]), 0,
                d_agg.data_ptr(), None, None)
        if rc != 0:
            raise RuntimeError("baseline library: ssa_aggregate_many%s_device gave %d" % ("_sliced" if sliced else "", rc))

    def sync(self):
        self.lib.ssa_ctx_sync(self.ctx)

    def close(self):
        self.lib.ssa_ctx_destroy(self.ctx)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--signers", type=int, default=65536)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seed", type=int, default=0x5E1)
    ap.add_argument("--baseline-lib", default=None, help="a build of the parent commit's library")
    a = ap.parse_args()
    import torch
    import schnorr_sig_amd as ssa
    dev = torch.device("cuda", 0)
    n, signers = a.n, min(a.signers, a.n)
    half = n // 2
    eng = ssa.Engine(0)
    base_path = a.baseline_lib or ssa.LIB_PATH
    par = Parent(base_path)
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
    lists = {"all": rng.permutation(n), "half": rng.permutation(n)[:half]}
    gone = rng.choice(n, half, replace=False)
    mask = np.zeros(n, np.uint8)
    mask[gone] = 1
    kept = np.flatnonzero(mask == 0)
    d_list = {k: t(v.astype(np.int32)) for k, v in lists.items()}
    d_gone, d_mask = t(gone.astype(np.int32)), t(mask)
    buf = lambda size: torch.zeros(size, dtype=torch.uint8, device=dev)   # noqa: E731
    d_agg, d_agg2, d_keys, d_keys2 = buf(49 * n + 32), buf(49 * n + 32), buf(49 * n), buf(49 * n)
    d_res = torch.zeros(1, dtype=torch.int32, device=dev)
    sha = lambda path: hashlib.sha256(open(path, "rb").read()).hexdigest()[:16]   # noqa: E731
    res = {"metric": "aggregator_select", "n": n, "signers": signers, "msg_len": 80, "rounds": a.rounds, "warmup": a.warmup,
           "library_sha256": sha(ssa.LIB_PATH), "baseline_sha256": sha(base_path), "baseline_is_this_tree": not a.baseline_lib,
           "device": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d"), "mismatches": 0}
    # the parent's inputs, gathered in the chosen order beforehand, and its answers: the expected values
    gathered, want, want_keys = {}, {}, {}
    for k, v in list(lists.items()) + [("kept", kept), ("arrival", None)]:
        if v is None:
            gathered[k], want_keys[k] = (d_sigs, d_pks, d_msgs), d_wire
        else:
            d_v = t(v)
            gathered[k], want_keys[k] = tuple(x[d_v].contiguous() for x in (d_sigs, d_pks, d_msgs)), d_wire[d_v].contiguous()
        want[k] = buf(49 * int(gathered[k][1].shape[0]) + 32)
        torch.cuda.synchronize()      # the gathers ran on torch's stream, the library reads on its own
        par.aggregate(gathered[k], want[k])
    par.sync()
    cache = eng.keycache_create(signers + 16, wire=True)
    held = eng.aggregator(n, hold_keys=True)

    def reload_held():
        held.reset()
        m, _ = held.push_keyed_device(cache, d_rec, d_msgs, want_stats=False)
        assert m == n
        eng.sync()

    def select(k):
        held.finish_select_device(d_list[k], d_agg, d_res, d_keys)

    def selected(k):
        m = int(d_list[k].numel())
        return (int(d_res.item()) == 0 and bool((d_agg[:49 * m + 32] == want[k]).all())
                and bool((d_keys[:49 * m] == want_keys[k].reshape(-1)).all()))

    def parent_ok(k):
        return bool((d_agg[:want[k].numel()] == want[k]).all())

    def finish_and_keys():
        held.finish_device(d_agg)
        held.keys_device(d_keys)

    def removed():
        """finish and keys of what the object holds against the kept lanes"""
        m = len(held)
        d_agg2.fill_(0xEE)
        d_keys2.fill_(0xEE)
        torch.cuda.synchronize()
        held.finish_device(d_agg2[:49 * m + 32])
        held.keys_device(d_keys2[:49 * m])
        eng.sync()
        return (m == kept.size and bool((d_agg2[:49 * m + 32] == want["kept"]).all())
                and bool((d_keys2[:49 * m] == want_keys["kept"].reshape(-1)).all()))

    nothing = lambda: None   # noqa: E731
    # leg: (prepare, timed call, its sync, check)
    legs = {}
    for k in ("all", "half"):
        legs["select_" + k] = (nothing, lambda k=k: select(k), eng.sync, lambda k=k: selected(k))
        legs["parent_many_" + k] = (nothing, lambda k=k: par.aggregate(gathered[k], d_agg), par.sync, lambda k=k: parent_ok(k))
        legs["parent_sliced_" + k] = (nothing, lambda k=k: par.aggregate(gathered[k], d_agg, sliced=True), par.sync,
                                      lambda k=k: parent_ok(k))
    legs["finish_and_keys"] = (nothing, finish_and_keys, eng.sync,
                               lambda: parent_ok("arrival") and bool((d_keys == d_wire.reshape(-1)).all()))
    legs["remove_indices_half"] = (reload_held, lambda: held.remove_indices_device(d_gone), eng.sync, removed)
    legs["remove_mask_half"] = (reload_held, lambda: held.remove_device(d_mask), eng.sync, removed)
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
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                call()
                sync()
                ms = (time.perf_counter() - t0) * 1e3
            res["mismatches"] += 0 if check() else 1
            if leg.startswith("remove_"):
                reload_held()
            if rnd >= a.warmup:
                times[leg].append(ms)
    med = res["ms_median"] = {leg: round(float(np.median(v)), 3) for leg, v in times.items()}
    res["ms_min"] = {leg: round(float(np.min(v)), 3) for leg, v in times.items()}
    res["ms_max"] = {leg: round(float(np.max(v)), 3) for leg, v in times.items()}
    res["ms_all"] = {leg: [round(x, 3) for x in v] for leg, v in times.items()}
    res["pairings"], res["ratio"] = {}, {}
    for k in ("all", "half"):
        best = [min(m_, s_) for m_, s_ in zip(times["parent_many_" + k], times["parent_sliced_" + k])]
        res["pairings"][k] = [[round(x, 3), round(b, 3)] for x, b in zip(times["select_" + k], best)]
        res["ratio"]["select_%s/parent_best" % k] = round(
            med["select_" + k] / min(med["parent_many_" + k], med["parent_sliced_" + k]), 4)
        res["ratio"]["select_%s/finish_and_keys" % k] = round(med["select_" + k] / med["finish_and_keys"], 4)
    res["select_faster_in_every_pairing"] = all(x < b for k in res["pairings"] for x, b in res["pairings"][k])
    res["ratio"]["remove_indices_half/remove_mask_half"] = round(med["remove_indices_half"] / med["remove_mask_half"], 4)
    kern = {}
    for leg in ("select_all", "select_half", "remove_indices_half", "remove_mask_half"):
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
        if leg.startswith("remove_"):
            reload_held()
    res["kernel_ms_avg_launches"] = kern
    print(json.dumps(res))
    for h in (held, cache):
        h.close()
    eng.close()
    par.close()
    return 0 if res["mismatches"] == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
