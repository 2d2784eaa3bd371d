#!/usr/bin/env python3
"""The one-slice split against the unsplit call, on ONE context whose knobs the debug setter
changes between the legs: ms per call of ssa_verify_many_device (verify_batch flags or the subgroup check, bench.py's
batch) for the short part at each share in 1/16ths, with and without an end game of its own, at each batch size.  The
legs alternate round by round; every leg's status vector and count are compared with the unsplit call's.  Prints one
JSON line.

  split_sweep.py [--sizes 131072,262144,524288,1048576] [--fracs 2,4,6,8] [--reps 5] [--rounds 3] [--check-torsion]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import bench  # noqa: E402
import schnorr_sig_amd as ssa  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="131072,262144,524288,1048576")
    ap.add_argument("--fracs", default="2,4,6,8")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--check-torsion", action="store_true", help="SSA_FLAG_CHECK_TORSION instead of verify_batch flags")
    args = ap.parse_args()
    sizes = [int(v) for v in args.sizes.split(",")]
    fracs = [int(v) for v in args.fracs.split(",")]
    dev = torch.device("cuda", 0)
    eng = ssa.Engine(0)
    n_max = max(sizes)
    sigs, pks, msgs, g = bench.gen_batch(torch, eng, dev, n_max, 0x5C4E0222)
    status = torch.empty(n_max, dtype=torch.uint8, device=dev)
    nfail = torch.zeros(1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()

    def call(n):
        eng.verify_many_device(sigs.data_ptr(), pks.data_ptr(), msgs.data_ptr(), n, 80, status.data_ptr(), nfail.data_ptr(),
                               check_torsion=args.check_torsion, sig_flag_byte=not args.check_torsion)

    def timed(n):
        call(n)
        eng.sync()
        t0 = time.perf_counter()
        for _ in range(args.reps):
            call(n)
        eng.sync()
        return (time.perf_counter() - t0) / args.reps * 1e3

    legs = [(0, 0)] + [(f, t) for f in fracs for t in (0, 1)]
    out = {"check_torsion": args.check_torsion, "reps": args.reps, "rounds": args.rounds, "sizes": {}, "mismatches": 0}
    for n in sizes:
        ms = {leg: [] for leg in legs}
        ref = None
        for rnd in range(args.rounds):
            for frac, tail_b in legs:
                eng.debug_split_config(split_min=0, split_frac=frac, tail_b=tail_b)
                ms[frac, tail_b].append(timed(n))
                got = (status[:n].clone(), int(nfail.item()))
                if ref is None:
                    ref = got
                elif got[1] != ref[1] or not torch.equal(got[0], ref[0]):
                    out["mismatches"] += 1
        out["sizes"][str(n)] = {"rejected": ref[1], "legs": [
            {"frac16": f, "tail_b": t, "plan": ssa.debug_split_plan(n, f), "ms_median": round(statistics.median(ms[f, t]), 4),
             "ms_min": round(min(ms[f, t]), 4), "ms_max": round(max(ms[f, t]), 4)} for f, t in legs]}
        for leg in out["sizes"][str(n)]["legs"]:
            sys.stderr.write("n=%d %s\n" % (n, json.dumps(leg)))
    eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
