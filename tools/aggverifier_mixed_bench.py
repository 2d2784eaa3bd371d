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
call the verdict is compared with the parent's on the same block and scalar; one untimed pass checks e_agg + 1."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--signers", type=int, default=65536)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seed", type=int, default=0x34B)
    ap.add_argument("--baseline-lib", default=None, help="a build of the parent commit's library")
    a = ap.parse_args()
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
