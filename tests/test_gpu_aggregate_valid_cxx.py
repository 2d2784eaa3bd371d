"""AggregateSignature::aggregate_valid of the C++ mirror (schnorr-sig_amd/host/schnorr_sig.hpp) on the GPU: one case of 300
lanes with five bad ones replayed by tests/csrc/aggregate_valid_driver.cpp in a child process, its aggregate and kept list
byte for byte those of the Python mirror (Engine.aggregate_valid) on the same bytes."""
import os
import struct
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cxx_mirror_gives_the_python_mirrors_bytes(engine, tmp_path):
    import schnorr_sig_amd as ssa
    rng = np.random.default_rng(0xC5AA)
    n = 300

    def scalars(m):
        s = rng.integers(0, 256, size=(m, 32), dtype=np.uint8)
        s[:, 31] &= 0x3F
        s[:, 0] |= 1
        return s
    rows = [rng.bytes(int(rng.integers(0, 100))) for _ in range(n)]
    flat, off = ssa.pack_messages(rows)
    pks, sigs = engine.keygen_sign_many(scalars(n), scalars(n), flat, offsets=off)
    sigs, pks = sigs.copy(), pks.copy()
    bad = [0, 64, 131, 256, n - 1]
    sigs[bad[0], 49] ^= 1                   # a bit of e
    sigs[bad[1], 48] ^= 0x40                # the sort bit of R
    sigs[bad[2], 49:81] = 0xFF              # e >= q
    pks[bad[3], 48] ^= 1                    # a key off the curve
    sigs[bad[4]] = sigs[bad[4] - 1]         # another lane's signature
    inf = np.zeros(n, np.uint8)
    agg, kept, status = engine.aggregate_valid(sigs, pks, flat, offsets=off, pk_inf=inf)
    assert kept.tolist() == [i for i in range(n) if i not in bad] and agg.size == 49 * (n - 5) + 32

    libdir = os.path.join(ROOT, "schnorr-sig_amd", "csrc")
    exe = str(tmp_path / "aggregate_valid_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                           os.path.join(ROOT, "tests", "csrc", "aggregate_valid_driver.cpp"), "-L" + libdir,
                           "-lschnorr_sig_amd", "-Wl,-rpath," + libdir, "-L/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    case, outp = str(tmp_path / "case.bin"), str(tmp_path / "out.bin")
    with open(case, "wb") as f:
        f.write(struct.pack("<Q", n) + sigs.tobytes() + pks.tobytes() + inf.tobytes())
        f.write(struct.pack("<%dQ" % n, *[len(r) for r in rows]) + b"".join(rows))
    r = subprocess.run([exe, case, outp], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    assert open(outp, "rb").read() == struct.pack("<Q", kept.size) + kept.astype("<u4").tobytes() + agg.tobytes()
