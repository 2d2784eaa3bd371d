"""The KeyCache overloads of schnorr_sig::AggregateVerifier (schnorr-sig_amd/host/schnorr_sig.hpp) on the GPU: the
bad-key scenario of tests/test_gpu_aggverifier_cached.py -- one key P + T2, three pushes cut at block edges, all through
the cache or mixed with plain pushes, affine and wire keys -- replayed by tests/csrc/aggverifier_cached_driver.cpp in one
child process.  Its verdicts, statistics and counters are those of the Python mirror on the same bytes, and the verdicts
are in turn the one-shot Engine.verify_aggregates_cached's (rhs) wherever the whole prefix came through the cache."""
import os
import struct
import subprocess

import numpy as np
import pytest

import test_gpu_aggverifier_cached as tc
from test_gpu_aggverifier_cached import world      # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = (1 << 64) - 1
CUTS = {"all cached": [(512, 1), (513, 1), (263, 1)], "plain, cached, plain": [(512, 0), (513, 1), (263, 0)],
        "the key in a plain push": [(512, 1), (513, 0), (263, 1)]}


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    libdir = os.path.join(ROOT, "schnorr-sig_amd", "csrc")
    exe = str(tmp_path_factory.mktemp("aggverifier_cached_cxx") / "aggverifier_cached_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                           os.path.join(ROOT, "tests", "csrc", "aggverifier_cached_driver.cpp"), "-L" + libdir,
                           "-lschnorr_sig_amd", "-Wl,-rpath," + libdir, "-L/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    return exe


def test_cxx_overloads_give_the_python_mirrors_verdicts_statistics_and_counters(engine, world, driver, tmp_path):
    n, p = tc.TOTAL, tc.PLACES["left_of_a_block_edge"]              # lane 1023: in the second push
    lanes = np.arange(n)
    cases = [(mode, name) for mode in tc.MODES for name in CUTS]
    blob, want = struct.pack("<Q", len(cases)), b""
    for mode, name in cases:
        cuts = CUTS[name]
        body = tc.world_body(world, lanes, tc.spoil_classes(engine, mode)["p_plus_t2"], [p])
        keys = body.keys(engine, mode)
        e = lambda t: tc.e_honest(engine, world, lanes, t)      # noqa: E731
        finishes = [(ALL, e(n)), (n, tc.neg(e(n))), (p, e(p)), (p + 1, e(p + 1)), (0, np.zeros(32, np.uint8))]
        run = tc.Run(engine, mode, "host")
        with engine.aggregate_verifier(n) as av, tc.new_cache(engine, mode, capacity=256) as cache:
            lo, stats = 0, []
            for cnt, through in cuts:
                st = run.push(av, body, lo, lo + cnt, cache if through else None)
                stats.append(st if st is not None else [0] * 8)
                lo += cnt
            got = [av.finish(s, None if take == ALL else take) for take, s in finishes]
            info = av.info()
        key_checked = cuts[1][1] == 1
        assert got[0] == got[1] == got[3] == (tc.BAD_KEY if key_checked else tc.INVALID), (mode, name, got)
        assert got[2] == tc.OK and got[4] == tc.OK
        if name == "all cached":
            assert got == [tc.rhs(engine, body, mode, s, n if take == ALL else take) for take, s in finishes]
        assert info["reserved"] == sum(c for c, through in cuts if through)
        for st in stats:
            want += struct.pack("<8Q", *st)
        want += struct.pack("<%di" % len(got), *got)
        want += struct.pack("<8Q", info["held"], info["capacity"], info["block_lanes"], info["pushes"], info["pushed"],
                            info["reserved"], info["blocks"], info["finishes"])
        blob += struct.pack("<3Q", n, int(mode == "wire"), len(cuts)) + b"".join(struct.pack("<2Q", c, t) for c, t in cuts)
        blob += body.rs.tobytes() + keys.u_pks.tobytes() + keys.u_inf.astype(np.uint8).tobytes() + body.wire.tobytes()
        blob += struct.pack("<%dQ" % n, *([body.msgs.shape[1]] * n)) + body.msgs.tobytes()
        blob += struct.pack("<Q", len(finishes)) + b"".join(struct.pack("<Q", take) + np.asarray(s).tobytes()
                                                            for take, s in finishes)
    path, outp = str(tmp_path / "cases.bin"), str(tmp_path / "out.bin")
    with open(path, "wb") as f:
        f.write(blob)
    r = subprocess.run([driver, path, outp], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    got = open(outp, "rb").read()
    assert len(got) == len(want) and got == want
