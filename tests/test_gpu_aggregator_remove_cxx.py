"""drop_front, remove and take of schnorr_sig::Aggregator of the C++ mirror (schnorr-sig_amd/host/schnorr_sig.hpp) on the
GPU: one front drop, one mask and one take replayed by tests/csrc/aggregator_remove_driver.cpp in a child process.  Its
aggregates, kept count and counters are byte for byte those of the Python mirror (Engine.aggregator) on the same bytes,
which are the one-shot aggregates of the kept lanes."""
import os
import struct
import subprocess

import numpy as np
import pytest

import test_gpu_aggregator as tga

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, FRONT, TAKE = 1100, 513, 300


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    libdir = os.path.join(ROOT, "schnorr-sig_amd", "csrc")
    exe = str(tmp_path_factory.mktemp("aggregator_remove_cxx") / "aggregator_remove_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                           os.path.join(ROOT, "tests", "csrc", "aggregator_remove_driver.cpp"), "-L" + libdir,
                           "-lschnorr_sig_amd", "-Wl,-rpath," + libdir, "-L/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    return exe


def test_cxx_mirror_gives_the_python_mirrors_bytes(engine, driver, tmp_path):
    rng = np.random.default_rng(0xC5AD)
    msgs = rng.integers(0, 256, size=(N, 80), dtype=np.uint8)
    pks, sigs = engine.keygen_sign_many(tga.make_scalars(rng, N), tga.make_scalars(rng, N), msgs)
    inf = np.zeros(N, np.uint8)
    mask = np.zeros(N - FRONT, np.uint8)
    mask[rng.choice(N - FRONT, (N - FRONT) // 3, replace=False)] = 3
    mask[0] = 1
    K = FRONT + np.flatnonzero(mask == 0)
    one_shot = lambda idx: tga.one_shot(engine, sigs[idx], pks[idx], msgs[idx]).tobytes()
    with engine.aggregator(N) as ag:
        assert ag.push(sigs, pks, msgs, screen=False)[1] == N
        ag.drop_front(FRONT)
        want = ag.finish_bytes().tobytes()
        assert want == one_shot(np.arange(FRONT, N))
        kept = ag.remove(mask)
        assert kept == K.size
        after = ag.finish_bytes().tobytes()
        assert after == one_shot(K)
        taken = ag.take(TAKE).to_bytes()
        assert taken == one_shot(K[:TAKE])
        rest = ag.finish_bytes().tobytes()
        assert rest == one_shot(K[TAKE:])
        info = ag.info()
        want += struct.pack("<Q", kept) + after + taken + rest
        want += struct.pack("<8Q", info["held"], info["capacity"], info["block_lanes"], info["pushes"], info["offered"],
                            info["dropped"], info["blocks"], info["finishes"])
    path, outp = str(tmp_path / "case.bin"), str(tmp_path / "out.bin")
    with open(path, "wb") as f:
        f.write(struct.pack("<4Q", N, 0, FRONT, TAKE))
        f.write(sigs.tobytes() + pks.tobytes() + inf.tobytes())
        f.write(struct.pack("<%dQ" % N, *([msgs.shape[1]] * N)) + msgs.tobytes() + mask.tobytes())
    r = subprocess.run([driver, path, outp], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    got = open(outp, "rb").read()
    assert len(got) == len(want) and got == want
