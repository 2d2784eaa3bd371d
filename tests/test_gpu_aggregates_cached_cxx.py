"""The key-cache overloads of AggregateSignature::verify_many of the C++ mirror (schnorr-sig_amd/host/schnorr_sig.hpp,
DESIGN.md section 23) on the GPU: one five-aggregate case with one subgroup-bad key, replayed by
tests/csrc/aggregates_cached_driver.cpp in a child process through an Affine and a Wire cache, its verdicts byte for byte
those of the Python mirror (Engine.verify_aggregates_cached) on the same bytes."""
import os
import struct
import subprocess

import numpy as np
import pytest

from test_gpu_screened_torsion import special_key_lanes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, BAD_KEY, INVALID, MALFORMED = 0, 1, 2, 3


def test_cxx_overloads_give_the_python_mirrors_bytes(engine, tmp_path):
    import schnorr_sig_amd as ssa
    rng = np.random.default_rng(0xC5AA)
    counts = [3, 0, 260, 1, 4]
    n = sum(counts)

    def scalars(m):
        s = rng.integers(0, 256, size=(m, 32), dtype=np.uint8)
        s[:, 31] &= 0x3F
        s[:, 0] |= 1
        return s
    rows = [rng.bytes(80) for _ in range(n)]
    flat, off = ssa.pack_messages(rows)
    signers = scalars(9)[rng.integers(0, 9, size=n)]
    pks, sigs = engine.keygen_sign_many(signers, scalars(n), flat, offsets=off)
    # lane 100 of the 260-lane aggregate: a signature made for a key P + T2 (on the curve, outside the subgroup)
    pkb, s1, m1 = special_key_lanes(rng, 1, True)
    i = 3 + 100
    pks[i], sigs[i], rows[i] = pkb, s1[0], m1[0].tobytes()
    flat, off = ssa.pack_messages(rows)
    aggs, lo = [], 0
    for c in counts:
        f, o = ssa.pack_messages(rows[lo:lo + c])
        st, agg, _, _ = engine.aggregate(sigs[lo:lo + c], pks[lo:lo + c], f, offsets=o)
        assert st == OK
        aggs.append(agg)
        lo += c
    aggs[4][-32:] = 0xFF                    # e_agg >= q
    inf = np.zeros(n, np.uint8)
    wire, st = engine.compress_many(pks)
    assert (st == 0).all()
    with engine.keycache_create(256) as ca, engine.keycache_create(256, wire=True) as cw:
        want_a, stats_a = engine.verify_aggregates_cached(ca, aggs, pks, flat, pk_inf=inf, offsets=off)
        want_w, stats_w = engine.verify_aggregates_cached(cw, aggs, wire, flat, offsets=off)
    assert want_a.tolist() == want_w.tolist() == [OK, OK, BAD_KEY, OK, MALFORMED]

    libdir = os.path.join(ROOT, "schnorr-sig_amd", "csrc")
    exe = str(tmp_path / "aggregates_cached_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                           os.path.join(ROOT, "tests", "csrc", "aggregates_cached_driver.cpp"), "-L" + libdir,
                           "-lschnorr_sig_amd", "-Wl,-rpath," + libdir, "-L/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    case, outp = str(tmp_path / "case.bin"), str(tmp_path / "verdicts.bin")
    with open(case, "wb") as f:
        f.write(struct.pack("<Q", len(counts)) + struct.pack("<%dQ" % len(counts), *counts))
        f.write(b"".join(a.tobytes() for a in aggs) + pks.tobytes() + inf.tobytes() + wire.tobytes())
        f.write(struct.pack("<%dQ" % n, *[len(r) for r in rows]) + b"".join(rows))
    r = subprocess.run([exe, case, outp], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    got = open(outp, "rb").read()
    k = len(counts)
    assert got[:4 * k] == want_a.astype("<u4").tobytes()
    assert got[4 * k:8 * k] == want_w.astype("<u4").tobytes()
    # both calls met a cold cache, as the Python mirror's did: the same statistics
    assert got[8 * k:8 * k + 64] == stats_a.astype("<u8").tobytes()
    assert got[8 * k + 64:] == stats_w.astype("<u8").tobytes()
