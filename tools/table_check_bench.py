"""Cost of the exact table self-check per comb width.

For each width (16 / 20 / 22 / 24 bits) a fresh child process times context creation -- the comb build and its check
-- and then runs ssa_ctx_selfcheck five times with kernel timing on.  One JSON line per width: the ssa_k_gtab_check
time, rows/s, and the bytes it reads per second next to the ~6.3 TB/s HBM read floor.

    python tools/table_check_bench.py [--widths 16,20,22,24] [--reps 5]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_FLOOR_TBS = 6.3

CHILD = r"""
import json, sys, time
import schnorr_sig_amd as ssa
bits, reps = int(sys.argv[1]), int(sys.argv[2])
budget = 64 << 30
t0 = time.perf_counter()
eng = ssa.Engine(0, gtab_bits=bits, hbm_budget_bytes=budget)
create_ms = (time.perf_counter() - t0) * 1e3
info = eng.info()
eng.enable_timing(True)
walls = []
for _ in range(reps):
    t1 = time.perf_counter()
    r = eng.selfcheck()
    walls.append((time.perf_counter() - t1) * 1e3)
    assert r["ok"], r
avg, cnt = eng.read_timing("ssa_k_gtab_check")
print(json.dumps({"bits": info["gtab_bits"], "rows": r["rows"], "table_bytes": info["gtab_bytes"], "builds": r["builds"],
                  "create_ms": create_ms, "check_ms": avg, "check_launches": cnt, "selfcheck_wall_ms": min(walls)}))
eng.close()
"""


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--widths", default="16,20,22,24")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=600)
    a = ap.parse_args()
    for bits in [int(b) for b in a.widths.split(",")]:
        r = subprocess.run([sys.executable, "-c", CHILD, str(bits), str(a.reps)], capture_output=True, text=True,
                           timeout=a.timeout, cwd=ROOT)
        if r.returncode != 0:
            print(json.dumps({"bits": bits, "error": r.returncode, "stderr": r.stderr[-2000:]}))
            sys.exit(1)
        d = json.loads(r.stdout.strip().splitlines()[-1])
        s = d["check_ms"] / 1e3
        d["rows_per_s"] = d["rows"] / s if s else None
        d["read_gbs"] = d["table_bytes"] / s / 1e9 if s else None
        d["hbm_floor_ms"] = d["table_bytes"] / (HBM_FLOOR_TBS * 1e12) * 1e3
        d["build_ms_est"] = d["create_ms"] - d["check_ms"]      # creation = build + check + context set-up
        print(json.dumps(d), flush=True)


if __name__ == "__main__":
    main()
