"""CPU tests of bench.py's options: a plain run leaves every leg beside the headline to --full, and --dump-outputs writes
the last timed step's outputs as float .npy files, within the size cap and reproducibly."""
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_full_is_off_by_default():
    a = bench.parse_args(["--gpus", "1", "--steps", "3", "--warmup", "1"])
    assert a.full is False and a.dump_outputs is None and a.steps == 3 and a.warmup == 1
    a = bench.parse_args(["--full", "--dump-outputs", "out"])
    assert a.full is True and a.dump_outputs == "out"
    assert bench.parse_args([]).forged is None and bench.parse_args(["--forged", "0"]).forged == 0


def _batch(n, seed=1):
    g = torch.Generator()
    g.manual_seed(seed)
    return tuple(torch.randint(0, 256, (n, w), dtype=torch.uint8, generator=g) for w in (81, 96, 80))


def test_forgeries_touch_exactly_the_seeded_lanes():
    n, count = 4096, 37
    sigs, pks, msgs = _batch(n)
    s0, p0, m0 = sigs.clone(), pks.clone(), msgs.clone()
    idx = bench.forge(torch, sigs, pks, msgs, n, count, bench.FORGE_SEED)
    assert idx.shape == (count,) and len(set(idx.tolist())) == count
    changed = (sigs != s0).any(1) | (pks != p0).any(1) | (msgs != m0).any(1)
    assert sorted(changed.nonzero().flatten().tolist()) == sorted(idx.tolist())
    # each lane gets one kind: e (byte 50), message, key or R -- never the bytes the --corrupt kinds change
    assert (sigs[:, 49] == s0[:, 49]).all() and (msgs[:, 40] == m0[:, 40]).all()
    kinds = [(sigs[:, 50] != s0[:, 50]), (msgs != m0).any(1), (pks != p0).any(1), (sigs[:, :49] != s0[:, :49]).any(1)]
    assert sum(int(k.sum()) for k in kinds) == count
    # seeded: the same lanes and bytes every run
    s1, p1, m1 = _batch(n)
    bench.forge(torch, s1, p1, m1, n, count, bench.FORGE_SEED)
    assert (s1 == sigs).all() and (p1 == pks).all() and (m1 == msgs).all()


def test_zero_steps_are_refused():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode != 0 and "--steps" in r.stderr
    assert not any(ln.startswith("{") for ln in r.stdout.splitlines())


def test_dump_writes_status_and_count(tmp_path):
    status = torch.zeros(1000, dtype=torch.uint8)
    status[[3, 500, 999]] = torch.tensor([1, 2, 3], dtype=torch.uint8)
    bench.dump_outputs(str(tmp_path), status, 3, 0, 1)
    assert sorted(os.listdir(tmp_path)) == ["rejected.npy", "status.npy"]
    st = np.load(tmp_path / "status.npy")
    assert st.dtype == np.float32 and st.shape == (1000,)
    assert (st == status.numpy().astype(np.float32)).all()
    rej = np.load(tmp_path / "rejected.npy")
    assert rej.dtype == np.float64 and rej.tolist() == [3.0]


def test_dump_of_a_large_batch_is_a_fixed_sample_under_the_cap(tmp_path):
    n = bench.DUMP_BYTES_MAX // 4 + 12345
    status = torch.from_numpy((np.arange(n) % 7).astype(np.uint8))
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), status, 0, 0, 1)
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert total < 64 << 20
    idx = np.load(tmp_path / "a" / "status_index.npy")
    st = np.load(tmp_path / "a" / "status.npy")
    assert idx.dtype == np.float64 and st.shape == idx.shape == (bench.DUMP_BYTES_MAX // 12,)
    assert (np.diff(idx) > 0).all() and (st == idx.astype(np.int64) % 7).all()
    for f in ("status.npy", "status_index.npy", "rejected.npy"):       # the same sample every run
        assert (np.load(tmp_path / "a" / f) == np.load(tmp_path / "b" / f)).all()


def test_dump_of_several_ranks_names_each_shard(tmp_path):
    for rank in (0, 1):
        bench.dump_outputs(str(tmp_path), torch.full((10,), rank, dtype=torch.uint8), 7, rank, 2)
    assert sorted(os.listdir(tmp_path)) == ["rejected.npy", "status_rank0.npy", "status_rank1.npy"]
    assert (np.load(tmp_path / "status_rank1.npy") == 1).all()
