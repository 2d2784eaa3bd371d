"""The KeyCache overloads of schnorr_sig::Aggregator of the C++ mirror (schnorr-sig_amd/host/schnorr_sig.hpp) on the GPU:
a push through an affine cache, push_keyed through a wire cache (record bytes and KeyedSignature objects), keys, remove and
finish replayed by tests/csrc/aggregator_cached_driver.cpp in a child process.  Every output is byte for byte that of the
Python mirror (Engine.aggregator) on the same bytes, whose aggregates are the one-shot aggregates of the kept lanes."""
import os
import struct
import subprocess

import numpy as np
import pytest

from test_gpu_aggregate_valid_cached import BAD_KEY, INVALID, Case, Honest
from test_gpu_aggregates_cached import new_cache, spoil_classes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, N_AFFINE, N_OBJECTS = 3300, 3100, 8               # both pushes above the small-batch bound: the caches are used


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    libdir = os.path.join(ROOT, "schnorr-sig_amd", "csrc")
    exe = str(tmp_path_factory.mktemp("aggregator_cached_cxx") / "aggregator_cached_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                           os.path.join(ROOT, "tests", "csrc", "aggregator_cached_driver.cpp"), "-L" + libdir,
                           "-lschnorr_sig_amd", "-Wl,-rpath," + libdir, "-L/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    return exe


def test_cxx_mirror_gives_the_python_mirrors_bytes(engine, driver, tmp_path):
    c = Case(Honest(engine, N, seed=0xC5AE))
    spoil_classes(engine, "affine")["p_plus_t2"](c.pks, c.inf, c.wire, 7)
    c.sigs[100, 49] ^= 1
    rec = np.ascontiguousarray(np.concatenate([c.wire, c.sigs], axis=1))
    want_status = np.zeros(N, np.uint8)
    want_status[7], want_status[100] = BAD_KEY, INVALID
    K = np.flatnonzero(want_status == 0)
    KA = np.concatenate([K[K < N_AFFINE], K])

    def one_shot(idx):
        st, agg, _, nf = engine.aggregate(c.sigs[idx], c.pks[idx], c.msgs[idx])
        assert st == 0 and nf == 0
        return agg.tobytes()
    rng = np.random.default_rng(0xC5AF)
    mask_a, mask_b = np.zeros(KA.size, np.uint8), np.zeros(K.size, np.uint8)
    mask_a[rng.choice(KA.size, KA.size // 3, replace=False)] = 3
    mask_b[rng.choice(K.size, K.size // 5, replace=False)] = 1
    mask_b[0] = 1
    want = b""

    def pushed(out):
        st, kept, stats = out
        return st.tobytes() + struct.pack("<Q", kept) + struct.pack("<12Q", *(int(x) for x in stats))
    with new_cache(engine, "affine") as ca, new_cache(engine, "wire") as cw, engine.aggregator(N_AFFINE + N) as a, \
            engine.aggregator(N, hold_keys=True) as b, engine.aggregator(N_OBJECTS + 1, hold_keys=True) as o:
        out = a.push(c.sigs[:N_AFFINE], c.pks[:N_AFFINE], c.msgs[:N_AFFINE], pk_inf=c.inf[:N_AFFINE], cache=ca)
        assert (out[0] == want_status[:N_AFFINE]).all() and int(out[2][5]) == 1
        want += pushed(out)
        out = a.push_keyed(cw, rec, c.msgs)
        assert (out[0] == want_status).all() and int(out[2][5]) == 1
        want += pushed(out)
        agg = a.finish_bytes().tobytes()
        assert agg == one_shot(KA)
        kept = a.remove(mask_a)
        after = a.finish_bytes().tobytes()
        assert after == one_shot(KA[mask_a == 0])
        want += agg + struct.pack("<Q", kept) + after
        want += pushed(b.push_keyed(cw, rec, c.msgs))
        keys, agg = b.keys(), b.finish_bytes().tobytes()
        assert (keys == c.wire[K]).all() and agg == one_shot(K)
        kept = b.remove(mask_b)
        keys2, after = b.keys(), b.finish_bytes().tobytes()
        assert (keys2 == c.wire[K[mask_b == 0]]).all() and after == one_shot(K[mask_b == 0])
        want += keys.tobytes() + agg + struct.pack("<Q", kept) + keys2.tobytes() + after
        out = o.push_keyed(cw, rec[:N_OBJECTS], c.msgs[:N_OBJECTS])
        assert out[1] == N_OBJECTS - 1 and out[0][7] == BAD_KEY
        want += pushed(out) + o.keys().tobytes() + o.finish_bytes().tobytes()
        assert (o.keys() == c.wire[:7]).all()
        for obj in (a, b, o):
            info = obj.info()
            want += struct.pack("<8Q", info["held"], info["capacity"], info["block_lanes"], info["pushes"], info["offered"],
                                info["dropped"], info["blocks"], info["finishes"])
    path, outp = str(tmp_path / "case.bin"), str(tmp_path / "out.bin")
    with open(path, "wb") as f:
        f.write(struct.pack("<6Q", N, N_AFFINE, 0, N_OBJECTS, mask_a.size, mask_b.size))
        f.write(c.sigs.tobytes() + c.pks.tobytes() + c.inf.tobytes() + c.wire.tobytes())
        f.write(struct.pack("<%dQ" % N, *([c.msgs.shape[1]] * N)) + c.msgs.tobytes() + mask_a.tobytes() + mask_b.tobytes())
    r = subprocess.run([driver, path, outp], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    got = open(outp, "rb").read()
    assert len(got) == len(want) and got == want
