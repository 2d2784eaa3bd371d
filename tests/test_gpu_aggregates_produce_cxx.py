"""AggregateSignature::aggregate_many of the C++ mirror (schnorr-sig_amd/host/schnorr_sig.hpp) on the GPU: the boundary
counts of tests/test_gpu_aggregates_produce.py replayed by tests/csrc/aggregates_produce_driver.cpp in a child process, its
results and aggregates byte for byte those of the Python mirror (Engine.aggregates_wire) on the same bytes."""
import os
import struct
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, MALFORMED = 0, 3
COUNTS = [1, 0, 2, 255, 256, 257, 0, 513, 3, 1, 0]


def test_cxx_mirror_gives_the_python_mirrors_bytes(engine, tmp_path):
    import schnorr_sig_amd as ssa
    rng = np.random.default_rng(0xC5A26)
    n = sum(COUNTS)

    def scalars(m):
        s = rng.integers(0, 256, size=(m, 32), dtype=np.uint8)
        s[:, 31] &= 0x3F
        s[:, 0] |= 1
        return s
    rows = [rng.bytes(int(rng.integers(0, 100))) for _ in range(n)]
    flat, off = ssa.pack_messages(rows)
    pks, sigs = engine.keygen_sign_many(scalars(n), scalars(n), flat, offsets=off)
    sigs = sigs.copy()
    sigs[2, 48] |= 0x01                      # aggregate 2 is refused: an undecodable R
    inf = np.zeros(n, np.uint8)
    _, wire, results, _, nfail = engine.aggregates_wire((sigs, pks, flat), check=True, counts=COUNTS, pk_inf=inf, offsets=off)
    assert results.tolist() == [MALFORMED if j == 2 else OK for j in range(len(COUNTS))] and nfail == 1

    libdir = os.path.join(ROOT, "schnorr-sig_amd", "csrc")
    exe = str(tmp_path / "aggregates_produce_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                           os.path.join(ROOT, "tests", "csrc", "aggregates_produce_driver.cpp"), "-L" + libdir,
                           "-lschnorr_sig_amd", "-Wl,-rpath," + libdir, "-L/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    case, outp = str(tmp_path / "case.bin"), str(tmp_path / "out.bin")
    with open(case, "wb") as f:
        f.write(struct.pack("<Q", len(COUNTS)) + struct.pack("<%dQ" % len(COUNTS), *COUNTS) + struct.pack("<Q", 1))
        f.write(sigs.tobytes() + pks.tobytes() + inf.tobytes())
        f.write(struct.pack("<%dQ" % n, *[len(r) for r in rows]) + b"".join(rows))
    r = subprocess.run([exe, case, outp], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    assert open(outp, "rb").read() == results.astype("<u4").tobytes() + wire.tobytes()
