"""AggregateSignature::verify_many of the C++ mirror (schnorr-sig_amd/host/schnorr_sig.hpp) on the GPU: one five-aggregate
case replayed by tests/csrc/aggregates_many_driver.cpp in a child process, its verdicts byte for byte those of the Python
mirror (Engine.verify_aggregates) on the same bytes."""
import os
import struct
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID, MALFORMED = 0, 2, 3


def test_cxx_mirror_gives_the_python_mirrors_bytes(engine, tmp_path):
    import schnorr_sig_amd as ssa
    rng = np.random.default_rng(0xC5A9)
    counts = [3, 0, 260, 1, 4]
    n = sum(counts)

    def scalars(m):
        s = rng.integers(0, 256, size=(m, 32), dtype=np.uint8)
        s[:, 31] &= 0x3F
        s[:, 0] |= 1
        return s
    rows = [rng.bytes(int(rng.integers(0, 100))) for _ in range(n)]
    flat, off = ssa.pack_messages(rows)
    pks, sigs = engine.keygen_sign_many(scalars(n), scalars(n), flat, offsets=off)
    aggs, lo = [], 0
    for c in counts:
        f, o = ssa.pack_messages(rows[lo:lo + c])
        st, agg, _, _ = engine.aggregate(sigs[lo:lo + c], pks[lo:lo + c], f, offsets=o)
        assert st == OK
        aggs.append(agg)
        lo += c
    aggs[2][49 * 259 + 48] ^= 0x40          # the last R's sort bit
    aggs[4][-32:] = 0xFF                    # e_agg >= q
    inf = np.zeros(n, np.uint8)
    want = engine.verify_aggregates(aggs, pks, flat, pk_inf=inf, offsets=off)
    assert want.tolist() == [OK, OK, INVALID, OK, MALFORMED]

    libdir = os.path.join(ROOT, "schnorr-sig_amd", "csrc")
    exe = str(tmp_path / "aggregates_many_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                           os.path.join(ROOT, "tests", "csrc", "aggregates_many_driver.cpp"), "-L" + libdir,
                           "-lschnorr_sig_amd", "-Wl,-rpath," + libdir, "-L/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    case, outp = str(tmp_path / "case.bin"), str(tmp_path / "verdicts.bin")
    with open(case, "wb") as f:
        f.write(struct.pack("<Q", len(counts)) + struct.pack("<%dQ" % len(counts), *counts))
        f.write(b"".join(a.tobytes() for a in aggs) + pks.tobytes() + inf.tobytes())
        f.write(struct.pack("<%dQ" % n, *[len(r) for r in rows]) + b"".join(rows))
    r = subprocess.run([exe, case, outp], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    assert open(outp, "rb").read() == want.astype("<u4").tobytes()
