"""The KeyCache overloads of AggregateSignature::aggregate_valid of the C++ mirror (schnorr-sig_amd/host/schnorr_sig.hpp) on
the GPU: one case of 3 300 lanes with bad lanes of every kind replayed by tests/csrc/aggregate_valid_cached_driver.cpp in a
child process, once with objects and an Affine cache and once with records and a Wire cache.  Kept list, aggregate, kept
keys and statistics are byte for byte those of the array call on the same bytes, and the mirror's verify_many accepts what
came out on the same cache."""
import os
import struct
import subprocess

import numpy as np
import pytest

from test_gpu_aggregate_valid_cached import MODES, call, cases_of
from test_gpu_aggregates_cached import new_cache

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_EXE = {}


def driver(tmp_path_factory):
    if "exe" not in _EXE:
        libdir = os.path.join(ROOT, "schnorr-sig_amd", "csrc")
        exe = str(tmp_path_factory.mktemp("avc") / "aggregate_valid_cached_driver")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                               os.path.join(ROOT, "tests", "csrc", "aggregate_valid_cached_driver.cpp"), "-L" + libdir,
                               "-lschnorr_sig_amd", "-Wl,-rpath," + libdir, "-L/opt/rocm/lib", "-lamdhip64",
                               "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
        _EXE["exe"] = exe
    return _EXE["exe"]


@pytest.mark.parametrize("mode", MODES)
def test_cxx_overloads_give_the_array_calls_bytes(engine, tmp_path, tmp_path_factory, mode):
    n = 3300
    cname, c = cases_of(engine, n, mode)[0]
    keys = c.keys(engine, mode)
    with new_cache(engine, mode) as cache:
        g = call(engine, cache, mode, "host", c.sigs, keys, c.msgs)
    assert g.rc == 0 and 0 < g.m < n and cname == "p_plus_t2"
    want = struct.pack("<Q", g.m) + g.kept[:g.m].astype("<u4").tobytes() + g.agg[:49 * g.m + 32].tobytes()
    if mode == "wire":
        want += g.keys[:g.m].tobytes()
    else:
        want += np.concatenate([g.keys[:g.m], g.inf[:g.m, None]], axis=1).tobytes()
    want += struct.pack("<12Q", *g.stats) + struct.pack("<I", 0)
    case, outp = str(tmp_path / "case.bin"), str(tmp_path / "out.bin")
    with open(case, "wb") as f:
        f.write(struct.pack("<QQ", 1 if mode == "wire" else 0, n) + c.sigs.tobytes() + c.pks.tobytes() + c.inf.tobytes())
        f.write(c.wire.tobytes() + struct.pack("<%dQ" % n, *([80] * n)) + c.msgs.tobytes())
    r = subprocess.run([driver(tmp_path_factory), case, outp], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    assert open(outp, "rb").read() == want
