"""bench.py without --full: the headline alone (set-up, warm-up, the timed steps, the line), and --dump-outputs writes
what the last timed step computed.  The default batch carries one seeded forgery per 1024 lanes, so the status vector
is not all zero: the dump is a fingerprint of the run, the same from run to run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(args, env_extra=None, timeout=900):
    """bench.py as a FRESH child process (never an exec of this process, which has touched the GPU)"""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT",
                                                            "MASTER_ADDR", "GROUP_RANK", "LOCAL_WORLD_SIZE")}
    env["HSA_ENABLE_IPC_MODE_LEGACY"] = "0"
    env.update(env_extra or {})
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, capture_output=True,
                       text=True, timeout=timeout)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1 and r.stdout.strip() == lines[0], r.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_is_the_headline_and_dumps_its_last_step(tmp_path):
    n, steps = 65536, 3
    args = ["--gpus", "1", "--batch", str(n), "--steps", str(steps), "--warmup", "1"]
    runs = [_bench(args + ["--dump-outputs", str(tmp_path / d)]) for d in ("a", "b")]
    for out in runs:
        assert out["full"] is False and out["steps"] == steps and out["n_gpus"] == 1
        assert out["unit"] == "verifications/s" and out["higher_is_better"] is True and out["dtype"] == "u64"
        assert out["value"] > 0 and abs(out["value"] - n / (out["ms_per_step"] * 1e-3)) < 1e-6 * out["value"]
        assert out["config"]["forged_per_gpu"] == n >> 10 and "64 forged per GPU" in out["config"]["workload"]
        assert out["rejected"] == n >> 10 and out["all_verdicts_as_expected"] is True     # lane by lane
        assert out["kernels_ms"]["launches"] > 0
        for leg in ("with_torsion_check_verifications_per_sec", "verify_batch_msm_form", "host_path", "keyed_context",
                    "signing", "pipelined_two_contexts", "config4_strong"):
            assert out[leg] is None, leg
        assert "cpu_baseline" not in out and "measured_fpmul_peak" not in out
    a, b = tmp_path / "a", tmp_path / "b"
    assert sorted(os.listdir(a)) == sorted(os.listdir(b)) == ["rejected.npy", "status.npy"]
    st = np.load(a / "status.npy")
    assert st.dtype == np.float32 and st.shape == (n,)
    assert int((st != 0).sum()) == n >> 10 and set(np.unique(st).tolist()) == {0.0, 2.0}   # SSA_INVALID_SIGNATURE
    assert np.load(a / "rejected.npy").tolist() == [float(n >> 10)]
    for f in ("status.npy", "rejected.npy"):
        assert (np.load(a / f) == np.load(b / f)).all(), f


def test_two_ranks_dump_one_status_file_each(tmp_path):
    """gloo rendezvous, both ranks on the one GPU: every rank forges its own seeded lanes and writes its own shard"""
    n = 16384
    out = _bench(["--gpus", "2", "--batch", str(n), "--steps", "1", "--warmup", "1", "--dump-outputs", str(tmp_path)],
                 env_extra={"SSA_BENCH_BACKEND": "gloo"})
    assert out["n_gpus"] == 2 and out["rejected"] == 2 * (n >> 10) and out["all_verdicts_as_expected"] is True
    assert sorted(os.listdir(tmp_path)) == ["rejected.npy", "status_rank0.npy", "status_rank1.npy"]
    st = [np.load(tmp_path / ("status_rank%d.npy" % r)) for r in (0, 1)]
    assert all(s.shape == (n,) and int((s != 0).sum()) == n >> 10 for s in st)
    assert not (st[0] == st[1]).all()                     # the ranks' forgeries sit on different lanes
    assert np.load(tmp_path / "rejected.npy").tolist() == [float(2 * (n >> 10))]
