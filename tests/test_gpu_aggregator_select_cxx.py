"""finish_select, remove_indices and take_select of schnorr_sig::Aggregator of the C++ mirror
(schnorr-sig_amd/host/schnorr_sig.hpp) on the GPU: one scenario replayed by
tests/csrc/aggregator_select_driver.cpp in a child process.  Every output is byte for byte that of the Python mirror
(Engine.aggregator) on the same bytes, whose aggregates are the one-shot aggregates of the selected lanes."""
import os
import struct
import subprocess

import numpy as np
import pytest

from test_gpu_aggregate_valid_cached import Case, Honest
from test_gpu_aggregates_cached import new_cache

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, B = 700, 8


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    libdir = os.path.join(ROOT, "schnorr-sig_amd", "csrc")
    exe = str(tmp_path_factory.mktemp("aggregator_select_cxx") / "aggregator_select_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                           os.path.join(ROOT, "tests", "csrc", "aggregator_select_driver.cpp"), "-L" + libdir,
                           "-lschnorr_sig_amd", "-Wl,-rpath," + libdir, "-L/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    return exe


def test_cxx_mirror_gives_the_python_mirrors_bytes(engine, driver, tmp_path):
    c = Case(Honest(engine, N, seed=0x5E1C))
    c.sigs[100, 49] ^= 1                             # one lane is dropped: places and lanes differ from there on
    rec = np.ascontiguousarray(np.concatenate([c.wire, c.sigs], axis=1))
    K = np.delete(np.arange(N), 100)

    def one_shot(idx):
        st, agg, _, nf = engine.aggregate(c.sigs[idx], c.pks[idx], c.msgs[idx])
        assert st == 0 and nf == 0
        return agg.tobytes()
    rng = np.random.default_rng(0x5E1D)
    l1 = rng.choice(K.size, 513, replace=False).astype(np.uint32)
    l2 = rng.choice(K.size, 300, replace=False).astype(np.uint32)
    l3 = l2.copy()
    l3[299] = l3[3]                                  # an index twice
    rest = np.delete(K, l2)
    want = b""
    with new_cache(engine, "wire") as cw, engine.aggregator(N, B, hold_keys=True) as a, engine.aggregator(N, B) as b:
        st, kept, _ = a.push_keyed(cw, rec, c.msgs)
        assert np.flatnonzero(st).tolist() == [100] and kept == K.size
        want += st.tobytes() + struct.pack("<Q", kept)
        agg, keys = a.finish_select_bytes(l1, keys=True)
        assert agg.tobytes() == one_shot(K[l1]) and (keys == c.wire[K[l1]]).all()
        want += keys.tobytes() + agg.tobytes()
        agg, keys = a.take_select(l2)
        assert agg.to_bytes() == one_shot(K[l2]) and (keys == c.wire[K[l2]]).all()
        want += keys.tobytes() + agg.to_bytes()
        left = a.finish_bytes().tobytes()            # (once: the driver's `finishes` must agree)
        assert (a.keys() == c.wire[rest]).all() and left == one_shot(rest)
        want += a.keys().tobytes() + left
        assert b.push_keyed(cw, rec, c.msgs)[1] == K.size
        want += b.finish_select_bytes(l1).tobytes() + struct.pack("<Q", b.remove_indices(l2)) + b.finish_bytes().tobytes()
        # what the driver is refused, so that the counters agree
        for obj, lst, keys in ((a, l3, True), (b, [0], True)):
            with pytest.raises(RuntimeError):
                obj.finish_select(lst, keys=keys)
        with pytest.raises(RuntimeError):
            a.remove_indices(l3)
        for obj in (a, b):
            info = obj.info()
            want += struct.pack("<8Q", info["held"], info["capacity"], info["block_lanes"], info["pushes"], info["offered"],
                                info["dropped"], info["blocks"], info["finishes"])
    path, outp = str(tmp_path / "case.bin"), str(tmp_path / "out.bin")
    with open(path, "wb") as f:
        f.write(struct.pack("<5Q", N, B, l1.size, l2.size, l3.size))
        f.write(c.sigs.tobytes() + c.wire.tobytes())
        f.write(struct.pack("<%dQ" % N, *([c.msgs.shape[1]] * N)) + c.msgs.tobytes())
        f.write(l1.tobytes() + l2.tobytes() + l3.tobytes())
    r = subprocess.run([driver, path, outp], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    got = open(outp, "rb").read()
    assert len(got) == len(want) and got == want
