"""AggregateSignature::aggregate_sliced / verify_sliced of the C++ mirror (schnorr-sig_amd/host/schnorr_sig.hpp) on the
GPU: one case of three slices and a ragged last one, replayed by tests/csrc/aggregate_sliced_driver.cpp in a child process
whose context has an MSM slice of 512 lanes.  Its aggregate is byte for byte Engine.aggregate of a default context."""
import os
import struct
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID = 0, 2


def test_cxx_mirror_slices_to_the_single_calls_bytes(engine, tmp_path):
    import schnorr_sig_amd as ssa
    rng = np.random.default_rng(0xC5A25)
    n = 3 * 512 + 5

    def scalars(m):
        s = rng.integers(0, 256, size=(m, 32), dtype=np.uint8)
        s[:, 31] &= 0x3F
        s[:, 0] |= 1
        return s
    rows = [rng.bytes(int(rng.integers(0, 100))) for _ in range(n)]
    flat, off = ssa.pack_messages(rows)
    pks, sigs = engine.keygen_sign_many(scalars(n), scalars(n), flat, offsets=off)
    inf = np.zeros(n, np.uint8)
    st, want, _, _ = engine.aggregate(sigs, pks, flat, offsets=off, pk_inf=inf)
    assert st == OK

    libdir = os.path.join(ROOT, "schnorr-sig_amd", "csrc")
    exe = str(tmp_path / "aggregate_sliced_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                           os.path.join(ROOT, "tests", "csrc", "aggregate_sliced_driver.cpp"), "-L" + libdir,
                           "-lschnorr_sig_amd", "-Wl,-rpath," + libdir, "-L/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    case, outp = str(tmp_path / "case.bin"), str(tmp_path / "out.bin")
    with open(case, "wb") as f:
        f.write(struct.pack("<Q", n) + sigs.tobytes() + pks.tobytes() + inf.tobytes())
        f.write(struct.pack("<%dQ" % n, *[len(r) for r in rows]) + b"".join(rows))
    r = subprocess.run([exe, case, outp], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, SSA_MSM_SLICE="512"))
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    got = open(outp, "rb").read()
    assert got[:-8] == want.tobytes()
    assert struct.unpack("<2I", got[-8:]) == (OK, INVALID)
