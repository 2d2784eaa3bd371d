"""schnorr_sig::Aggregator of the C++ mirror (schnorr-sig_amd/host/schnorr_sig.hpp) on the GPU: the bad-lane scenario of
tests/test_gpu_aggregator.py -- one lane of every class, three pushes cut at block edges -- replayed by
tests/csrc/aggregator_driver.cpp in a child process, screened and unscreened.  Its statuses, kept counts, counters and
aggregates are byte for byte those of the Python mirror (Engine.aggregator) on the same bytes."""
import os
import struct
import subprocess

import numpy as np
import pytest

import test_gpu_aggregator as tga

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    libdir = os.path.join(ROOT, "schnorr-sig_amd", "csrc")
    exe = str(tmp_path_factory.mktemp("aggregator_cxx") / "aggregator_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                           os.path.join(ROOT, "tests", "csrc", "aggregator_driver.cpp"), "-L" + libdir,
                           "-lschnorr_sig_amd", "-Wl,-rpath," + libdir, "-L/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    return exe


@pytest.fixture(scope="module")
def case(engine):
    rng = np.random.default_rng(0xC5AB)
    n = tga.TOTAL
    msgs = rng.integers(0, 256, size=(n, 80), dtype=np.uint8)
    pks, sigs = engine.keygen_sign_many(tga.make_scalars(rng, n), tga.make_scalars(rng, n), msgs)
    return tga.spoil(engine, sigs, pks, msgs)


@pytest.mark.parametrize("screen", [True, False], ids=["screened", "no screen"])
def test_cxx_mirror_gives_the_python_mirrors_bytes(engine, driver, case, tmp_path, screen):
    sigs, pks, msgs, inf = case
    n, cuts = tga.TOTAL, tga.BAD_PUSHES
    want = b""
    with engine.aggregator(n) as ag:
        lo = 0
        for cnt in cuts:
            sl = slice(lo, lo + cnt)
            status, kept = ag.push(sigs[sl], pks[sl], msgs[sl], pk_inf=inf[sl], screen=screen)
            want += status.tobytes() + struct.pack("<Q", kept)
            lo += cnt
        info = ag.info()
        held = info["held"]
        assert held == n - sum(1 for v in tga.BAD.values() if not v[1 if screen else 2])
        want += struct.pack("<8Q", held, info["capacity"], info["block_lanes"], info["pushes"], info["offered"],
                            info["dropped"], info["blocks"], info["finishes"])
        want += ag.finish_bytes().tobytes() + ag.finish_bytes(held // 2).tobytes()
    path, outp = str(tmp_path / "case.bin"), str(tmp_path / "out.bin")
    with open(path, "wb") as f:
        f.write(struct.pack("<4Q", n, int(screen), 0, len(cuts)) + struct.pack("<%dQ" % len(cuts), *cuts))
        f.write(sigs.tobytes() + pks.tobytes() + inf.tobytes())
        f.write(struct.pack("<%dQ" % n, *([msgs.shape[1]] * n)) + msgs.tobytes())
    r = subprocess.run([driver, path, outp], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    got = open(outp, "rb").read()
    assert len(got) == len(want) and got == want
