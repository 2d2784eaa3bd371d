"""The C++ mirror of the leaf column and the leaf index (schnorr_sig::Aggregator with HoldIndex: leaves, leaves_select,
index_sync, lookup, index_info) gives the Python mirror's bytes on one scenario, through
tests/csrc/aggregator_index_driver.cpp."""
import os
import struct
import subprocess

import numpy as np
import pytest

from test_gpu_aggregator_index import POOL_B, UNKNOWN, world      # noqa: F401  (the fixture: the signed lanes and their leaves)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = (1 << 64) - 1


def build_driver(tmp_path):
    libdir = os.path.join(ROOT, "schnorr-sig_amd", "csrc")
    exe = str(tmp_path / "aggregator_index_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                           os.path.join(ROOT, "tests", "csrc", "aggregator_index_driver.cpp"), "-L" + libdir,
                           "-lschnorr_sig_amd", "-Wl,-rpath," + libdir, "-L/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    return exe


@pytest.mark.parametrize("index", [True, False])
def test_cxx_mirror_gives_the_python_mirrors_bytes(engine, world, tmp_path, index):      # noqa: F811
    import schnorr_sig_amd as ssa
    exe = build_driver(tmp_path)
    rng = np.random.default_rng(3690)
    first, second = np.concatenate([np.arange(300)[::-1], np.arange(10)]), np.arange(300, 420)
    ids = np.concatenate([world.leaves[rng.permutation(500)[:200]], world.absent[:20], world.leaves[:10]])
    flags = ssa.AGGR_HOLD_ADMISSION | (ssa.AGGR_HOLD_INDEX if index else 0)
    blob, want = struct.pack("<3Q", 512, POOL_B, flags), b""
    ops = 0

    def guarded(call):
        try:
            return 0, call()
        except (RuntimeError, ValueError):
            return 1, None
    with engine.aggregator(512, POOL_B, hold_admission=True, index=index) as ag:
        def push(lanes, screen):
            nonlocal blob, want, ops
            blob += struct.pack("<3Q", 1, int(screen), len(lanes)) + world.sigs[lanes].tobytes() + world.pks[lanes].tobytes()
            blob += struct.pack("<%dQ" % len(lanes), *([80] * len(lanes))) + world.msgs[lanes].tobytes()
            status, kept = ag.push(world.sigs[lanes], world.pks[lanes], world.msgs[lanes], screen=screen)
            assert kept == len(lanes)
            want += status.tobytes()
            ops += 1

        def lookup(x):
            nonlocal blob, want, ops
            blob += struct.pack("<2Q", 2, len(x)) + np.ascontiguousarray(x).tobytes()
            threw, out = guarded(lambda: ag.lookup(x))
            assert threw == (0 if index else 1)
            want += bytes([threw]) + (b"" if threw else out[0].tobytes() + struct.pack("<Q", out[1]))
            ops += 1
            return out

        def leaves(n_take):
            nonlocal blob, want, ops
            blob += struct.pack("<2Q", 3, ALL if n_take is None else n_take)
            threw, out = guarded(lambda: ag.leaves(n_take))
            want += bytes([threw]) + (b"" if threw else out.tobytes())
            ops += 1
            return threw

        def leaves_select(order):
            nonlocal blob, want, ops
            order = np.asarray(order, dtype=np.uint32)
            blob += struct.pack("<2Q", 4, len(order)) + order.tobytes()
            threw, out = guarded(lambda: ag.leaves_select(order))
            want += bytes([threw]) + (b"" if threw else out.tobytes())
            ops += 1
            return threw

        def drop_front(n):
            nonlocal blob, ops
            blob += struct.pack("<2Q", 5, n)
            ag.drop_front(n)
            ops += 1

        def index_sync():
            nonlocal blob, want, ops
            blob += struct.pack("<Q", 6)
            threw, _ = guarded(ag.index_sync)
            assert threw == (0 if index else 1)
            want += bytes([threw])
            ops += 1

        def index_info():
            nonlocal blob, want, ops
            blob += struct.pack("<Q", 7)
            threw, out = guarded(ag.index_info)
            want += bytes([threw]) + (b"" if threw else struct.pack("<8Q", *out.values()))
            ops += 1
            return out

        push(first, True)
        assert leaves(None) == 0 and leaves(7) == 0 and leaves(0) == 0 and leaves(311) == 1
        out = lookup(ids)
        if index:
            assert (out[0][-10:] == 299 - np.arange(10)).all() and out[1] >= 20      # the doubled lanes: the lower place
        index_info()
        assert leaves_select(np.arange(310)[::-1]) == 0 and leaves_select([0, 0, 309]) == 0 and leaves_select([]) == 0
        assert leaves_select([3, 310]) == 1
        push(second, False)
        lookup(ids)
        info = index_info()
        if index:
            assert info["rebuilds"] == 1 and info["indexed"] == 430 and info["overflowed"] == 0
        drop_front(POOL_B + 1)
        index_sync()
        index_info()
        out = lookup(ids)
        if index:
            assert (out[0] != UNKNOWN).sum() > 100
        lookup(np.zeros((0, 32), np.uint8))
        info = index_info()
        if index:
            assert info["rebuilds"] == 2 and info["lookups"] == 3 and info["ids"] == 3 * len(ids)
    path, outp = str(tmp_path / "cases.bin"), str(tmp_path / "out.bin")
    with open(path, "wb") as f:
        f.write(blob[:24] + struct.pack("<Q", ops) + blob[24:])
    r = subprocess.run([exe, path, outp], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    got = open(outp, "rb").read()
    assert len(got) == len(want) and got == want
