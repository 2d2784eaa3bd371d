"""schnorr_sig::AggregateVerifier of the C++ mirror (schnorr-sig_amd/host/schnorr_sig.hpp) on the GPU: the bad-lane
scenario of tests/test_gpu_aggverifier.py -- one lane of every class, three pushes cut at block edges -- replayed by
tests/csrc/aggverifier_driver.cpp in one child process.  Its verdicts and counters are those of the Python mirror
(Engine.aggregate_verifier) on the same bytes, which in turn are the one-shot Engine.verify_aggregate's."""
import os
import struct
import subprocess

import numpy as np
import pytest

import test_gpu_aggverifier as tgv

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = (1 << 64) - 1


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    libdir = os.path.join(ROOT, "schnorr-sig_amd", "csrc")
    exe = str(tmp_path_factory.mktemp("aggverifier_cxx") / "aggverifier_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                           os.path.join(ROOT, "tests", "csrc", "aggverifier_driver.cpp"), "-L" + libdir,
                           "-lschnorr_sig_amd", "-Wl,-rpath," + libdir, "-L/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    return exe


def test_cxx_mirror_gives_the_python_mirrors_verdicts(engine, driver, tmp_path):
    pool = tgv.Pool(engine)
    n, cuts = tgv.TOTAL, tgv.BAD_PUSHES
    blob, want = struct.pack("<Q", len(tgv.BAD)), b""
    for what, (k, verdict) in tgv.BAD.items():
        rs, pks, msgs, inf, e_agg = tgv.spoil(engine, pool, what)
        e_agg, e_front = np.array(e_agg), np.array(pool.e(0, k))
        finishes = [(ALL, e_agg), (n, e_agg), (k, e_front), (k + 1, e_agg), (0, np.zeros(32, np.uint8))]
        with engine.aggregate_verifier(n) as av:
            lo = 0
            for cnt in cuts:
                sl = slice(lo, lo + cnt)
                av.push(rs[sl], pks[sl], msgs[sl], pk_inf=inf[sl])
                lo += cnt
            got = [av.finish(e, None if take == ALL else take) for take, e in finishes]
            assert got[0] == verdict == engine.verify_aggregate(np.concatenate([rs.reshape(-1), e_agg]), pks, msgs, pk_inf=inf)
            assert got[2] == tgv.OK and got[4] == tgv.OK
            info = av.info()
        want += struct.pack("<%di" % len(got), *got)
        want += struct.pack("<8Q", info["held"], info["capacity"], info["block_lanes"], info["pushes"], info["pushed"],
                            info["reserved"], info["blocks"], info["finishes"])
        blob += struct.pack("<3Q", n, 0, len(cuts)) + struct.pack("<%dQ" % len(cuts), *cuts)
        blob += rs.tobytes() + pks.tobytes() + inf.tobytes()
        blob += struct.pack("<%dQ" % n, *([msgs.shape[1]] * n)) + msgs.tobytes()
        blob += struct.pack("<Q", len(finishes)) + b"".join(struct.pack("<Q", take) + e.tobytes() for take, e in finishes)
    path, outp = str(tmp_path / "cases.bin"), str(tmp_path / "out.bin")
    with open(path, "wb") as f:
        f.write(blob)
    r = subprocess.run([driver, path, outp], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    got = open(outp, "rb").read()
    assert len(got) == len(want) and got == want
