"""The C++ mirror (schnorr-sig_amd/host/schnorr_sig.hpp) executed class by class on the GPU.  tests/csrc/mirror_driver.cpp
replays a scenario written here -- keys, byte streams for its Rng, messages, records, indices, seeds -- through the mirror's
classes and writes back every output; everything is compared byte for byte with the CPU oracle where it defines the
answer, with tests/derive_model.py, tests/device_rng_model.py and tests/aggregate_model.py for the rest, and with the Python
mirror on the same inputs and coefficients as a second witness.  There is no tolerance anywhere.

The screened and cached paths are only reached above msm_small_max: every driver child, and the Python engine of this file,
run with SSA_MSM_SMALL_MAX=256, and the status vectors have 600 lanes by 40 signers (three 256-lane blocks, the last
ragged).  One child per test function; when one dies on a signal or runs out of time, the rest of the file skips."""
import os
import struct
import subprocess

import numpy as np
import pytest

import aggregate_model as am
import derive_model as dm
import device_rng_model as drm
import pymodel as pm
from test_gpu_screened import per_lane

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q = pm.Q
N, SIGNERS, MSG_LEN, SMALL_MAX = 600, 40, 80, "256"
HITS, INSERTED, EVICTIONS, BYPASSED = 8, 9, 10, 11
OK_, PANIC, INVALID_ARGUMENT, RUNTIME_ERROR = 0, 1, 2, 3
THREADS = 16


# ---- the scenario format: records of  u32 name length, name, u32 blob count, per blob u64 length and bytes ---------------
def _blob(x):
    if isinstance(x, np.ndarray):
        return x.tobytes()
    if isinstance(x, int):
        return struct.pack("<Q", x)
    if isinstance(x, str):
        return x.encode()
    return bytes(x)


def write_records(path, steps):
    with open(path, "wb") as f:
        for name, *blobs in steps:
            f.write(struct.pack("<I", len(name)) + name.encode() + struct.pack("<I", len(blobs)))
            for b in blobs:
                b = _blob(b)
                f.write(struct.pack("<Q", len(b)) + b)


def read_records(path):
    data, pos, out = open(path, "rb").read(), 0, []
    while pos < len(data):
        (ln,) = struct.unpack_from("<I", data, pos)
        name = data[pos + 4: pos + 4 + ln].decode()
        (nb,) = struct.unpack_from("<I", data, pos + 4 + ln)
        pos += 8 + ln
        blobs = []
        for _ in range(nb):
            (bl,) = struct.unpack_from("<Q", data, pos)
            blobs.append(data[pos + 8: pos + 8 + bl])
            pos += 8 + bl
        out.append(Step(name, blobs))
    return out


class Step:
    """one answer of the driver: how the step ended, the exception's text, the bytes its Rng handed out, the results"""

    def __init__(self, name, blobs):
        self.name, self.outcome, self.what = name, blobs[0][0], blobs[1].decode()
        self.rng_used = struct.unpack("<Q", blobs[2])[0]
        self.out = blobs[3:]

    def words(self, k=0):
        return [int(v) for v in np.frombuffer(self.out[k], "<u8")]

    def u8(self, k=0):
        return np.frombuffer(self.out[k], np.uint8)

    def __repr__(self):
        return "Step(%s, outcome=%d, %r, rng=%d, %s)" % (self.name, self.outcome, self.what, self.rng_used,
                                                         [len(b) for b in self.out])


class Driver:
    def __init__(self, exe):
        self.exe, self.dead = exe, None

    def run(self, tmp_path, steps, timeout=120):
        if self.dead:
            pytest.skip("an earlier driver child ended badly (%s): no further GPU work from this file" % self.dead)
        scen, outp = str(tmp_path / "scenario.bin"), str(tmp_path / "output.bin")
        write_records(scen, steps)
        env = dict(os.environ)
        env["SSA_MSM_SMALL_MAX"] = SMALL_MAX
        try:
            r = subprocess.run([self.exe, scen, outp], env=env, capture_output=True, text=True, timeout=timeout)
        except subprocess.TimeoutExpired:
            self.dead = "time limit"
            pytest.fail("the driver ran into its time limit")
        if r.returncode < 0 or r.returncode in (124, 134, 137, 139):
            self.dead = "exit status %d" % r.returncode
        assert r.returncode == 0 and "mirror_driver done" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
        res = read_records(outp)
        assert [s.name for s in res] == [st[0] for st in steps]
        return res


@pytest.fixture(scope="session")
def driver(tmp_path_factory):
    libdir = os.path.join(ROOT, "schnorr-sig_amd", "csrc")
    exe = str(tmp_path_factory.mktemp("mirror_driver") / "mirror_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                           os.path.join(ROOT, "tests", "csrc", "mirror_driver.cpp"), "-L" + libdir, "-lschnorr_sig_amd",
                           "-Wl,-rpath," + libdir, "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    return Driver(exe)


@pytest.fixture(scope="module")
def eng():
    """the Python mirror's engine under the same small-batch bound as the driver's contexts; the variable is gone again
    before anything else creates a context"""
    import schnorr_sig_amd as ssa
    os.environ["SSA_MSM_SMALL_MAX"] = SMALL_MAX
    try:
        e = ssa.Engine(0)
    finally:
        del os.environ["SSA_MSM_SMALL_MAX"]
    yield e
    e.close()


# ---- inputs ---------------------------------------------------------------------------------------------------------------
def le32(v):
    return int(v).to_bytes(32, "little")


def blocks_of(rng, n):
    """n 64-byte Rng blocks and the scalars Scalar::random makes of them"""
    b = rng.integers(0, 256, size=(n, 64), dtype=np.uint8)
    sc = np.frombuffer(b"".join(le32(int.from_bytes(r.tobytes(), "little") % Q) for r in b), np.uint8).reshape(n, 32)
    return b, sc


def scalars(rng, n):
    return blocks_of(rng, n)[1]


def msg_args(msgs):
    off = np.zeros(len(msgs) + 1, np.uint64)
    if len(msgs):
        off[1:] = np.cumsum([len(m) for m in msgs])
    return off, b"".join(bytes(m) for m in msgs)


def triple_steps(sigs, pks, inf, msgs):
    return [("sigs", sigs), ("pks", pks, inf), ("msgs",) + msg_args(list(msgs))]


def key97(pk96, inf=0):
    return bytes(pk96) + bytes([inf])


def distinct_keys(pks, inf):
    return len({bytes(p) + bytes([i]) for p, i in zip(pks, inf)})


def off_curve_x(oracle, rng):
    while True:
        c = bytes(rng.integers(0, 256, 48, dtype=np.uint8))
        c = c[:7] + b"\0" + c[8:15] + b"\0" + c[16:23] + b"\0" + c[24:31] + b"\0" + c[32:39] + b"\0" + c[40:47] + b"\0\0"
        if oracle.decompress(c) is None:
            return c


class Lanes:
    """600 signatures by 40 signers with one lane (or more) of every class of bad input, the oracle's two status vectors
    for them, and a second, honest batch by 40 other signers.  Computed once on the CPU and never changed."""

    def __init__(self, oracle):
        rng = np.random.default_rng(77001)
        self.sks = scalars(rng, SIGNERS)
        self.signer = rng.integers(0, SIGNERS, N)
        self.signer[:SIGNERS] = np.arange(SIGNERS)                      # every signer signs
        nonces = scalars(rng, N)
        self.msgs = rng.integers(0, 256, size=(N, MSG_LEN), dtype=np.uint8)
        pks, sigs = oracle.keygen_sign_many(self.sks[self.signer], nonces, self.msgs, threads=THREADS)
        self.honest = (sigs.copy(), pks.copy(), self.msgs.copy())
        inf = np.zeros(N, np.uint8)
        msgs = self.msgs.copy()
        bad = {}
        sigs[0, 49] ^= 1;                       bad["e"] = [0]
        sigs[255, 60] ^= 0x80;                  bad["e"].append(255)
        msgs[256, 79] ^= 0x10;                  bad["msg"] = [256]
        msgs[599, 0] ^= 1;                      bad["msg"].append(599)
        for i in (100, 511):                                             # the key of another signer
            j = next(j for j in range(N) if self.signer[j] != self.signer[i])
            pks[i] = self.honest[1][j]
        bad["swap"] = [100, 511]
        sigs[512, 48] ^= 0x40;                  bad["neg_r"] = [512]
        sigs[300, 48] ^= 0x40;                  bad["neg_r"].append(300)
        pks[200] = 0; inf[200] = 1;             bad["identity"] = [200]
        # an identity key under which a signature does verify: R = [r]G, e = r
        r = scalars(rng, 1)[0]
        rp, _ = oracle.keygen(r.tobytes())
        pks[201] = 0; inf[201] = 1
        sigs[201] = np.frombuffer(oracle.compress(rp) + r.tobytes(), np.uint8)
        self.identity_ok = 201
        f = pm.FIXTURE_SMALL_ORDER_PK
        small = np.frombuffer(pm.fp6_to_bytes48(f[0]) + pm.fp6_to_bytes48(f[1]), np.uint8)
        pks[257] = small; pks[400] = small;     bad["small_order"] = [257, 400]
        pks[450, 0:8] = 0xFF;                   bad["limb_ge_p"] = [450]
        pks[598, 88:96] = 0xFF;                 bad["limb_ge_p"].append(598)
        sigs[520, 49:81] = 0xFF;                bad["e_ge_q"] = [520]
        sigs[10, 49:81] = np.frombuffer(le32(Q), np.uint8); bad["e_ge_q"].append(10)
        sigs[530, 48] |= 0x01;                  bad["flag"] = [530]
        sigs[254, 48] = 0xFF;                   bad["flag"].append(254)
        self.bad, self.sigs, self.pks, self.inf, self.msgs = bad, sigs, pks, inf, msgs
        self.bad_lanes = sorted(i for v in bad.values() for i in v)
        self.u = distinct_keys(pks, inf)
        # Signature::verify and verify_batch semantics, lane by lane, from the oracle
        self.want_verify = oracle.verify_many(sigs, pks, msgs, check_torsion=True, pk_inf=inf, threads=THREADS)
        self.want_batch = oracle.verify_many(sigs, pks, msgs, check_torsion=False, pk_inf=inf, sig_flag_byte=True,
                                             threads=THREADS)
        # 130-byte wire records of the same lanes; a key that does not encode keeps its x
        recs = np.zeros((N, 130), np.uint8)
        for i in range(N):
            if i in bad["limb_ge_p"]:
                comp = pks[i, :48].tobytes() + b"\0"
            else:
                comp = oracle.compress(pks[i].tobytes(), bool(inf[i]))
            recs[i] = np.frombuffer(comp + sigs[i].tobytes(), np.uint8)
        self.undecodable = [33, 577]                                     # honest lanes whose record's key has no y / a bad flag
        recs[33, :49] = np.frombuffer(off_curve_x(oracle, rng), np.uint8)
        recs[577, 48] = 0xFF
        # KeyedSignature::verify of a record: 3 where the key does not decode, Signature::verify under the decoded key
        # elsewhere -- the vector above but for the keys whose bad limb is in y, which the wire form does not carry
        dec = [oracle.decompress(r[:49].tobytes()) for r in recs]
        ok = np.array([d is not None for d in dec])
        self.want_keyed = np.full(N, 3, np.uint8)
        self.want_keyed[ok] = oracle.verify_many(
            sigs[ok], np.array([np.frombuffer(d[0], np.uint8) for d in dec if d is not None]), msgs[ok], check_torsion=True,
            pk_inf=np.array([d[1] for d in dec if d is not None], np.uint8), threads=THREADS)
        assert not ok[self.undecodable].any() and not ok[450]
        differ = np.nonzero(self.want_keyed != self.want_verify)[0]
        assert set(differ) <= set(self.undecodable + [598]), differ
        self.recs = recs
        self.u_wire = len({r[:49].tobytes() for r in recs})
        # the second batch: honest, 40 other signers, lanes of one signer spread out
        self.sks2 = scalars(rng, SIGNERS)
        self.signer2 = np.arange(N) % SIGNERS
        self.msgs2 = rng.integers(0, 256, size=(N, MSG_LEN), dtype=np.uint8)
        self.pks2, self.sigs2 = oracle.keygen_sign_many(self.sks2[self.signer2], scalars(rng, N), self.msgs2, threads=THREADS)
        self.inf2 = np.zeros(N, np.uint8)
        self.recs2 = np.concatenate([np.frombuffer(b"".join(oracle.compress(p.tobytes()) for p in self.pks2),
                                                   np.uint8).reshape(N, 49), self.sigs2], axis=1)


@pytest.fixture(scope="module")
def lanes(oracle):
    ln = Lanes(oracle)
    assert set(int(v) for v in ln.want_verify) == {0, 1, 2, 3} and set(int(v) for v in ln.want_batch) == {0, 2, 3}
    # Signature::verify reads x(R) alone: R -> -R and the flag byte matter to verify_batch only
    x_only = ln.bad["neg_r"] + ln.bad["flag"]
    strict = [i for i in ln.bad_lanes if i not in x_only]
    assert (ln.want_verify[strict] != 0).all() and (np.delete(ln.want_verify, strict) == 0).all()
    assert (ln.want_batch[ln.bad_lanes] != 0).all() and (np.delete(ln.want_batch, ln.bad_lanes) == 0).all()
    assert (ln.want_batch[ln.bad["flag"]] == 3).all() and (ln.want_batch[ln.bad["neg_r"]] == 2).all()
    assert (ln.want_verify[ln.bad["small_order"]] == 1).all() and (ln.want_batch[ln.bad["small_order"]] != 1).all()
    assert ln.want_verify[ln.identity_ok] == 0 and ln.want_verify[200] == 2
    return ln


def _rechecked_as_the_segments_say(stats):
    """a slice all of whose segments fail is handed to the exact kernel whole (600 lanes may well be one segment)"""
    if stats[2] == stats[1]:
        assert stats[6] == 1 and stats[3] == N, stats
    else:
        assert stats[6] == 0 and 1 <= stats[3] < N, stats


def all_returned(res):
    bad = [s for s in res if s.outcome != OK_]
    assert not bad, bad


# ---- a. signing with a replayed Rng --------------------------------------------------------------------------------------
def test_key_pairs_sign_with_a_replayed_rng(driver, oracle, tmp_path):
    rng = np.random.default_rng(77101)
    lens = (0, 1, 7, 8, 80, 161)
    forms = ("kp_sign", "kp_sign_bind", "sk_sign", "sk_sign_bind")
    blk, sc = blocks_of(rng, 2 + len(lens) * len(forms))
    blk[0] = 0                                                            # the first draw is 0: KeyPair::create draws again
    msgs = [bytes(rng.integers(0, 256, k, dtype=np.uint8)) for k in lens]
    steps = [("rng", blk), ("kp_create",)]
    for m in msgs:
        steps += [(f, m) for f in forms]
    res = driver.run(tmp_path, steps)
    all_returned(res)
    sk = sc[1].tobytes()
    pk, _ = oracle.keygen(sk)
    comp = oracle.compress(pk)
    assert res[1].out == [sk, key97(pk)] and res[1].rng_used == 128
    k, recs = 2, []
    for m in msgs:
        for f in forms:
            s = res[k]
            want = oracle.sign(sk, sc[k].tobytes(), pk, m)
            assert s.rng_used == 64, s
            if f.endswith("bind"):
                assert s.out == [key97(pk), want, comp + want], (f, len(m))
                recs.append((comp + want, m))
            else:
                assert s.out == [want], (f, len(m))
            assert oracle.verify(want, pk, m) == 0
            k += 1
    # KeyedSignature::from_bytes: round trip, and what it refuses
    rec = recs[-1][0]
    e_at = 49 + 49
    cases = [(rec, True), (rec[:e_at] + le32(Q - 1), True), (rec[:e_at] + le32(Q), False), (rec[:e_at] + le32(Q + 1), False),
             (rec[:e_at] + b"\xff" * 32, False), (rec[:48] + b"\xff" + rec[49:], False),
             (off_curve_x(oracle, rng) + rec[49:], False), (recs[0][0], True)]
    # a scalar that differs from q only below its top byte, either way (the comparison runs from the top)
    cases += [(rec[:e_at] + le32(Q - 256), True), (rec[:e_at] + le32(Q + (1 << 200)), False)]
    res = driver.run(tmp_path, [("keyed_from_bytes", c) for c, _ in cases])
    all_returned(res)
    for (c, ok), s in zip(cases, res):
        if ok:
            assert s.out == [b"\1", key97(oracle.decompress(c[:49])[0]), c[49:], c], s
        else:
            assert s.out == [b"\0"], s


# ---- b. SignerSet from key pairs -----------------------------------------------------------------------------------------
def _py_outcome(call):
    import schnorr_sig_amd as ssa
    try:
        return OK_, call()
    except ssa.MalformedInput as e:
        return PANIC, e
    except ValueError as e:
        return INVALID_ARGUMENT, e
    except RuntimeError as e:
        return RUNTIME_ERROR, e


def test_signer_set_from_key_pairs(driver, oracle, eng, tmp_path):
    import schnorr_sig_amd as ssa
    rng = np.random.default_rng(77201)
    m, n = 7, 65
    sks = scalars(rng, m)
    idx = rng.integers(0, m, n).astype(np.uint32)
    idx[:4] = [6, 6, 0, 6]
    msgs = [bytes(rng.integers(0, 256, int(k), dtype=np.uint8)) for k in rng.integers(0, 120, n)]
    msgs[0], msgs[1] = b"", msgs[1][:1] or b"x"
    blk, sc = blocks_of(rng, 2 * n)
    over = idx.copy()
    over[n - 1] = m
    steps = [("ss_pairs", sks), ("ss_public_keys",), ("ss_secret_keys",), ("idx", idx), ("msgs",) + msg_args(msgs),
             ("rng", blk), ("ss_sign",), ("ss_sign_bind",),
             ("idx", over), ("ss_sign",), ("ss_sign_bind",),                       # an index == m
             ("idx", idx[:n - 1]), ("ss_sign",), ("ss_sign_bind",),                # one message too many
             ("idx", b""), ("msgs",) + msg_args([]), ("ss_sign",), ("ss_sign_bind",),   # n = 0
             ("ss_pairs", b"")]                                                   # m = 0
    res = driver.run(tmp_path, steps)
    pks = [oracle.keygen(s.tobytes())[0] for s in sks]
    assert res[0].outcome == OK_ and res[0].words() == [m]
    assert res[1].out == [b"".join(key97(p) for p in pks)] and res[2].out == [sks.tobytes()]
    want = [oracle.sign(sks[idx[i]].tobytes(), sc[i].tobytes(), pks[idx[i]], msgs[i]) for i in range(n)]
    want2 = [oracle.sign(sks[idx[i]].tobytes(), sc[n + i].tobytes(), pks[idx[i]], msgs[i]) for i in range(n)]
    assert res[6].outcome == OK_ and res[6].out == [b"".join(want)] and res[6].rng_used == 64 * n
    assert res[7].outcome == OK_ and res[7].rng_used == 64 * n
    assert res[7].out == [b"".join(key97(pks[k]) for k in idx), b"".join(want2)]
    for k in (9, 10, 12, 13):
        assert res[k].outcome == PANIC and res[k].rng_used == 0, res[k]
    # the Python mirror on the same keys, indices and byte stream
    feed = iter(blk)
    replay = lambda k: next(feed).tobytes()
    pairs = [ssa.KeyPair.from_bytes(s.tobytes(), eng) for s in sks]
    ss = ssa.SignerSet.from_key_pairs(pairs, eng)
    try:
        assert b"".join(s.to_bytes() for s in ss.sign(idx, msgs, replay)) == res[6].out[0]
        ks = ss.sign(idx, msgs, replay, keyed=True)
        assert b"".join(k.signature.to_bytes() for k in ks) == res[7].out[1]
        assert b"".join(key97(k.public_key.affine, k.public_key.is_identity) for k in ks) == res[7].out[0]
        for keyed, k in ((False, 16), (True, 17)):                                 # n = 0 as the Python mirror has it
            oc, val = _py_outcome(lambda: ss.sign([], [], replay, keyed=keyed))
            assert res[k].outcome == oc, (res[k], val)
            if oc == OK_:
                assert val == [] and all(b == b"" for b in res[k].out)
    finally:
        ss.close()
    oc, val = _py_outcome(lambda: ssa.SignerSet.from_key_pairs([], eng))           # m = 0
    assert res[18].outcome == oc, (res[18], val)
    if oc == OK_:
        val.close()


# ---- c. DeviceRng under a pinned seed ------------------------------------------------------------------------------------
def test_device_rng_pinned_equals_the_model_and_unpinned_differs(driver, oracle, tmp_path):
    rng = np.random.default_rng(77301)
    seed = bytes(rng.integers(0, 256, 44, dtype=np.uint8))
    sk = scalars(rng, 1)[0].tobytes()
    pk, _ = oracle.keygen(sk)
    msg, n = b"nonce drawn on the device", 33
    idx = rng.integers(0, 5, n).astype(np.uint32)
    msgs = [bytes(rng.integers(0, 256, int(k), dtype=np.uint8)) for k in rng.integers(0, 90, n)]
    single = ("kp_sign_dev", "kp_sign_bind_dev", "sk_sign_dev", "sk_sign_bind_dev")
    steps = [("pin", seed), ("kp_from_bytes", sk)] + [(f, msg) for f in single] + \
            [("ss_generate", 5), ("ss_secret_keys",), ("ss_public_keys",), ("idx", idx), ("msgs",) + msg_args(msgs),
             ("ss_sign_dev",), ("ss_sign_bind_dev",), ("pin", b"")] + [(f, msg) for f in single + single] + \
            [("ss_sign_dev",), ("ss_sign_dev",), ("ss_generate", 5), ("ss_secret_keys",)]
    res = driver.run(tmp_path, steps)
    all_returned(res)
    assert all(s.rng_used == 0 for s in res)
    assert res[1].out == [b"\1", key97(pk)]
    draws = drm.draw(seed, range(n))
    want = oracle.sign(sk, draws[0].tobytes(), pk, msg)
    comp = oracle.compress(pk)
    for k, f in enumerate(single):
        assert res[2 + k].out == ([key97(pk), want, comp + want] if "bind" in f else [want]), f
    keys = draws[:5]
    gpk = [oracle.keygen(s.tobytes())[0] for s in keys]
    assert res[6].words() == [5] and res[7].out == [keys.tobytes()] and res[8].out == [b"".join(key97(p) for p in gpk)]
    wsig = b"".join(oracle.sign(keys[idx[i]].tobytes(), draws[i].tobytes(), gpk[idx[i]], msgs[i]) for i in range(n))
    assert res[11].out == [wsig]
    assert res[12].out == [b"".join(key97(gpk[k]) for k in idx), wsig]
    # unpinned: every signature verifies under the oracle, no two calls agree
    seen = set()
    for k, f in enumerate(single + single):
        s = res[14 + k]
        sig = s.out[1] if "bind" in f else s.out[0]
        assert oracle.verify(sig, pk, msg) == 0 and sig not in seen and sig != want, f
        seen.add(sig)
    a, b = res[22].out[0], res[23].out[0]
    assert a != b and a != wsig and len(a) == 81 * n
    flat_off = msg_args(msgs)
    for sg in (a, b):
        st = oracle.verify_many(np.frombuffer(sg, np.uint8), np.array([np.frombuffer(gpk[k], np.uint8) for k in idx]),
                                np.frombuffer(flat_off[1] + b"\0", np.uint8), offsets=flat_off[0], threads=THREADS)
        assert (st == 0).all()
    assert res[24].words() == [5] and res[25].out[0] != keys.tobytes() and len(set(
        res[25].out[0][32 * k: 32 * k + 32] for k in range(5))) == 5


# ---- d. status vectors ----------------------------------------------------------------------------------------------------
def test_status_vectors_of_600_lanes(driver, oracle, eng, lanes, tmp_path):
    ln = lanes
    rng = np.random.default_rng(77401)
    blk, co = blocks_of(rng, 2 * N)
    steps = triple_steps(ln.sigs, ln.pks, ln.inf, ln.msgs) + [
        ("rng", blk), ("verify_many_statuses",), ("verify_many_screened_statuses", b"\1"),
        ("verify_many_screened_statuses", b"\0"), ("verify_batch_statuses", b"\1"), ("verify_batch_statuses", b"\0"),
        ("verify_batch", b"\0", b"\0"), ("verify_batch", b"\0", b"\1")] + \
        triple_steps(*ln.honest[:2], np.zeros(N, np.uint8), ln.honest[2]) + [
        ("verify_many_screened_statuses", b"\0"), ("verify_batch", b"\0", b"\1")] + \
        triple_steps(b"", b"", b"", []) + [
        ("verify_many_statuses",), ("verify_many_screened_statuses", b"\1"), ("verify_many_screened_statuses", b"\0"),
        ("verify_batch_statuses", b"\1"), ("verify_batch_statuses", b"\0")]
    res = driver.run(tmp_path, steps)
    dedup, scr, scr0, bat, bat0, vb, vbm = res[4:11]
    # Signature::verify semantics: the oracle's vector
    assert dedup.outcome == OK_ and (dedup.u8() == ln.want_verify).all() and dedup.rng_used == 0
    py_st, py_nf, py_stats = eng.verify_many_dedup(ln.sigs, ln.pks, ln.msgs, pk_inf=ln.inf)
    assert (py_st == ln.want_verify).all() and dedup.words(1) == [int(v) for v in py_stats]
    assert dedup.words(1)[0] == ln.u and dedup.words(1)[1] + dedup.words(1)[2] >= 1 and dedup.words(1)[3] == 0
    print("dedup stats", dedup.words(1))
    for s, c in ((scr, co[:N]), (scr0, None)):
        assert s.outcome == OK_ and (s.u8() == ln.want_verify).all() and s.rng_used == (64 * N if c is not None else 0), s
        stats = s.words(1)
        print("screened stats", stats)
        # the screened route: distinct keys found, the slice screened, the failing segments' lanes re-checked
        assert stats[0] == ln.u and stats[5] == 1 and stats[7] == 0 and 1 <= stats[2] <= stats[1], stats
        _rechecked_as_the_segments_say(stats)
    py_st, py_nf, py_stats = eng.verify_many_screened(ln.sigs, ln.pks, ln.msgs, pk_inf=ln.inf, coeffs=co[:N])
    assert py_st.tobytes() == scr.out[0] and [int(v) for v in py_stats] == scr.words(1)
    # verify_batch semantics: the oracle's per-lane vector, which is also what the per-lane kernel gives
    assert (per_lane(eng, ln.sigs, ln.pks, ln.msgs, ln.inf)[0] == ln.want_batch).all()
    for s, c in ((bat, co[N:]), (bat0, None)):
        assert s.outcome == OK_ and (s.u8() == ln.want_batch).all() and s.rng_used == (64 * N if c is not None else 0), s
    py_st, _ = eng.verify_batch_screened(ln.sigs, ln.pks, ln.msgs, coeffs=co[N:], pk_inf=ln.inf)
    assert py_st.tobytes() == bat.out[0]
    # verify_batch on the same slice, both algorithms: malformed lanes, so the reference panics; the Python mirror agrees
    assert eng.verify_batch_status(ln.sigs, ln.pks, ln.msgs, pk_inf=ln.inf) == 3
    assert eng.verify_batch_msm(ln.sigs, ln.pks, ln.msgs, pk_inf=ln.inf) == 3
    assert oracle.verify_batch_msm(ln.sigs, ln.pks, ln.msgs, co[:N], pk_inf=ln.inf, threads=THREADS) == 3
    assert vb.outcome == PANIC and vbm.outcome == PANIC
    # the honest lanes: nothing re-checked, Ok
    hon, hvb = res[14], res[15]
    assert (hon.u8() == 0).all() and hon.words(1)[0] == SIGNERS and hon.words(1)[2:5] == [0, 0, 0] and hon.words(1)[5] == 1
    assert hvb.out == [b"\0"]
    # n = 0
    for s in res[19:24]:
        assert s.outcome == OK_ and s.out[0] == b"" and s.rng_used == 0, s


# ---- e. key caches --------------------------------------------------------------------------------------------------------
def _cache_sequence(call, call2, cache_ops):
    """cold, warm, clear, cold again; then recent-first eviction and the second batch, which overflows the cache"""
    seq = [call(), cache_ops("info"), call(), cache_ops("info"), cache_ops("clear"), cache_ops("info"), call(),
           cache_ops("info"), cache_ops("recent"), cache_ops("eviction_info"), cache_ops("info"), call2(),
           cache_ops("eviction_info"), cache_ops("info"), call(), cache_ops("eviction_info"),
           cache_ops("selfcheck", 0, 0), cache_ops("selfcheck", 1, 0), cache_ops("selfcheck", 1, 1)]
    return seq


_CACHE_STEP = {"info": ("kc_info",), "clear": ("kc_clear",), "recent": ("kc_set_eviction", "Recent"),
               "eviction_info": ("kc_eviction_info",)}


def _cxx_cache_ops(op, *args):
    return [("kc_selfcheck", bytes([args[0]]), bytes([args[1]]))] if op == "selfcheck" else [_CACHE_STEP[op]]


def _compare_cache_runs(res, py, want1, want2, u1):
    """res: the driver's answers to _cache_sequence's steps, py: the Python mirror's results of the same sequence"""
    import schnorr_sig_amd as ssa
    assert len(res) == len(py)
    calls = []
    for s, p in zip(res, py):
        assert s.outcome == OK_, s
        if s.name.startswith("verify_"):
            st, nf, stats = p
            assert s.out[0] == st.tobytes() and s.words(1) == [int(v) for v in stats], (s, stats)
            calls.append(s)
        elif s.name == "kc_info":
            assert s.words() == [p[k] for k in ("capacity", "held", "clears", "device_bytes")], (s.words(), p)
        elif s.name == "kc_eviction_info":
            assert s.words() == [ssa.KEYCACHE_EVICT[p["policy"]]] + [p[k] for k in (
                "compactions", "dropped", "last_kept", "last_moved", "epoch")], (s.words(), p)
        elif s.name == "kc_selfcheck":
            assert s.words() == [p[k] for k in ssa.KEYCHECK_FIELDS] and s.out[1] == bytes([p["ok"]]) and s.out[2] == b"", (s, p)
            assert p["ok"] and p["keys_checked"] > 0 and p["keys_bad"] == 0
    cold, warm, again, second, third = calls
    for s in (cold, warm, again, third):
        assert (s.u8() == want1).all()
    assert (second.u8() == want2).all()
    for s in calls:
        assert s.words(1)[5] == 1 and s.words(1)[BYPASSED] == 0, s.words(1)
        if s is second:                                                   # honest: screened, nothing re-checked
            assert s.words(1)[2:5] == [0, 0, 0] and s.words(1)[6] == 0, s.words(1)
        else:
            assert 1 <= s.words(1)[2] <= s.words(1)[1], s.words(1)
            _rechecked_as_the_segments_say(s.words(1))
    assert (cold.words(1)[0], cold.words(1)[HITS], cold.words(1)[INSERTED]) == (u1, 0, u1)
    assert (warm.words(1)[HITS], warm.words(1)[INSERTED]) == (u1, 0)
    assert (again.words(1)[HITS], again.words(1)[INSERTED]) == (0, u1)
    assert second.words(1)[INSERTED] == SIGNERS and second.words(1)[HITS] == 0 and second.words(1)[EVICTIONS] == 1
    infos = [s.words() for s in res if s.name == "kc_info"]
    assert [i[1] for i in infos[:4]] == [u1, u1, 0, u1] and infos[0][0] == 64
    ev = [s.words() for s in res if s.name == "kc_eviction_info"]
    assert ev[0][:3] == [1, 0, 0] and ev[1][0] == 1 and ev[1][1] == 1 and ev[1][2] >= u1 + SIGNERS - 64, ev


def test_key_cache_affine(driver, eng, lanes, tmp_path):
    ln = lanes
    rng = np.random.default_rng(77501)
    blk, co = blocks_of(rng, N)
    first, second = triple_steps(ln.sigs, ln.pks, ln.inf, ln.msgs), triple_steps(ln.sigs2, ln.pks2, ln.inf2, ln.msgs2)
    call = lambda: first + [("rng", blk), ("verify_many_cached_statuses", b"\1")]
    call2 = lambda: second + [("rng", blk), ("verify_many_cached_statuses", b"\1")]
    steps = [("kc_create", 64, b"\0")] + [s for part in _cache_sequence(call, call2, _cxx_cache_ops) for s in part]
    steps += first + [("verify_many_cached_statuses", b"\0")]                       # coefficients drawn by the library
    steps += [("kc_create", 64, b"\1"), ("verify_many_cached_statuses", b"\0")]     # a wire cache is not for this call
    res = driver.run(tmp_path, steps)
    assert res[0].out == [b"\0"]
    cache = eng.keycache_create(64)
    try:
        ops = {"info": cache.info, "clear": cache.clear, "recent": lambda: cache.set_eviction("recent"),
               "eviction_info": cache.eviction_info, "selfcheck": lambda d, r: cache.selfcheck(bool(d), bool(r))}
        py = _cache_sequence(
            lambda: eng.verify_many_cached(cache, ln.sigs, ln.pks, ln.msgs, pk_inf=ln.inf, coeffs=co),
            lambda: eng.verify_many_cached(cache, ln.sigs2, ln.pks2, ln.msgs2, pk_inf=ln.inf2, coeffs=co),
            lambda op, *a: ops[op](*a))
    finally:
        cache.close()
    keep = [s for s in res[1:-6] if s.name.startswith(("verify_", "kc_"))]
    _compare_cache_runs(keep, [p for p in py], ln.want_verify, np.zeros(N, np.uint8), ln.u)
    drawn = res[-3]
    assert drawn.outcome == OK_ and (drawn.u8() == ln.want_verify).all() and drawn.rng_used == 0
    wire = eng.keycache_create(64, wire=True)
    try:
        with pytest.raises(RuntimeError) as err:
            eng.verify_many_cached(wire, ln.sigs, ln.pks, ln.msgs, pk_inf=ln.inf)
    finally:
        wire.close()
    text = str(err.value)                                                          # "<call> failed: <text> (<code>)"
    assert res[-2].out == [b"\1"] and res[-1].outcome == RUNTIME_ERROR
    assert res[-1].what == "ssa_verify_many_cached: " + text[text.index("failed: ") + 8: text.rindex(" (")], (res[-1], text)


def test_key_cache_wire_records_and_device_forms(driver, eng, lanes, tmp_path):
    ln = lanes
    rng = np.random.default_rng(77601)
    blk, co = blocks_of(rng, N)
    msgs1, msgs2 = ("msgs",) + msg_args(list(ln.msgs)), ("msgs",) + msg_args(list(ln.msgs2))
    call = lambda: [("keyed", ln.recs), msgs1, ("rng", blk), ("verify_keyed_many_cached_statuses", b"\1")]
    call2 = lambda: [("keyed", ln.recs2), msgs2, ("rng", blk), ("verify_keyed_many_cached_statuses", b"\1")]
    steps = [("kc_create", 64, b"\1")] + [s for part in _cache_sequence(call, call2, _cxx_cache_ops) for s in part]
    tail = [("keyed", ln.recs), msgs1, ("verify_keyed_many_cached_statuses", b"\0"),
            ("keyed", ln.recs[:N - 1]), ("verify_keyed_many_cached_statuses", b"\0"),        # one message too many
            ("keyed", ln.recs.tobytes()[:-1]), ("verify_keyed_many_cached_statuses", b"\0"),  # a cut record
            ("keyed", ln.recs), ("kc_clear",),
            ("verify_keyed_many_cached_device", ln.msgs, MSG_LEN, 1), ("verify_keyed_many_cached_device", ln.msgs, MSG_LEN, 1),
            ("verify_keyed_many_device", ln.msgs, MSG_LEN, 1), ("verify_keyed_many_device", ln.msgs, MSG_LEN, 0),
            ("kc_info",)]
    res = driver.run(tmp_path, steps + tail)
    assert res[0].out == [b"\1"]
    cache = eng.keycache_create(64, wire=True)
    try:
        ops = {"info": cache.info, "clear": cache.clear, "recent": lambda: cache.set_eviction("recent"),
               "eviction_info": cache.eviction_info, "selfcheck": lambda d, r: cache.selfcheck(bool(d), bool(r))}
        py = _cache_sequence(lambda: eng.verify_keyed_many_cached(cache, ln.recs, ln.msgs, coeffs=co),
                             lambda: eng.verify_keyed_many_cached(cache, ln.recs2, ln.msgs2, coeffs=co),
                             lambda op, *a: ops[op](*a))
    finally:
        cache.close()
    keep = [s for s in res[1:len(steps)] if s.name.startswith(("verify_", "kc_"))]
    _compare_cache_runs(keep, py, ln.want_keyed, np.zeros(N, np.uint8), ln.u_wire)
    t = res[len(steps):]
    assert t[2].outcome == OK_ and (t[2].u8() == ln.want_keyed).all() and t[2].rng_used == 0
    assert t[4].outcome == INVALID_ARGUMENT and t[6].outcome == INVALID_ARGUMENT
    assert t[4].what == "We should have the same number of messages than keyed signatures"
    # the device pass-throughs: return code, n_fail, statuses, and the cache seen filling and then hitting
    nf = int((ln.want_keyed != 0).sum())
    cold, warm, plain, plain_no_torsion = t[9:13]
    for s in (cold, warm, plain):
        assert s.outcome == OK_ and s.words() == [0, nf] and (s.u8(1) == ln.want_keyed).all(), s
    assert (cold.words(2)[0], cold.words(2)[HITS], cold.words(2)[INSERTED]) == (ln.u_wire, 0, ln.u_wire)
    assert (warm.words(2)[HITS], warm.words(2)[INSERTED]) == (ln.u_wire, 0) and warm.words(2)[5] == 1
    want_nt = ln.want_keyed.copy()
    want_nt[ln.bad["small_order"]] = ln.want_batch[ln.bad["small_order"]]          # flags = 0: no subgroup check
    assert plain_no_torsion.words()[0] == 0 and (plain_no_torsion.u8(1) == want_nt).all()
    assert t[13].words()[1] == ln.u_wire


# ---- f. AggregateSignature -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [3, N])
def test_aggregate_signature(driver, oracle, eng, lanes, tmp_path, n):
    ln = lanes
    sigs, pks, msgs = ln.sigs2[:n], ln.pks2[:n], ln.msgs2[:n]
    inf = np.zeros(n, np.uint8)
    want = am.aggregate(am.oracle_backend(oracle, threads=THREADS), list(sigs), list(pks), list(msgs))
    e_agg = int.from_bytes(want[-32:], "little")
    bit = next(b for b in range(256) if (e_agg ^ (1 << b)) < Q)
    flipped = want[:-32] + le32(e_agg ^ (1 << bit))
    bad_msgs = msgs.copy()
    bad_msgs[n - 1, 5] ^= 4
    swapped = pks.copy()
    swapped[[0, 1]] = swapped[[1, 0]]
    assert ln.signer2[0] != ln.signer2[1]
    noncanon = want[:-32] + le32(Q)
    bad_sig = sigs.copy()
    bad_sig[n // 2, 70] ^= 1
    undec = sigs.copy()
    undec[n - 1, 49:81] = 0xFF
    T = lambda s=sigs, p=pks, m=msgs: triple_steps(s, p, inf, m)
    steps = T() + [("aggregate", b"\0"), ("agg_verify",), ("aggregate", b"\1"), ("agg_verify",),
                   ("agg_from_bytes", want), ("agg_verify",),
                   ("agg_set_bytes", flipped), ("agg_verify",), ("agg_from_bytes", flipped), ("agg_verify",),
                   ("agg_from_bytes", noncanon), ("agg_set_bytes", noncanon), ("agg_verify",),
                   ("agg_set_bytes", want)] + \
        T(m=bad_msgs) + [("agg_verify",)] + T(p=swapped) + [("agg_verify",)] + \
        [("pks", pks[:n - 1], inf[:n - 1]), ("agg_verify",)] + T() + [("msgs",) + msg_args(list(msgs[:n - 1])), ("agg_verify",)] + \
        T(s=bad_sig) + [("aggregate", b"\1"), ("aggregate", b"\0")] + T(s=undec) + [("aggregate", b"\1"), ("aggregate", b"\0")]
    res = driver.run(tmp_path, steps)
    r = [s for s in res if s.name.startswith("agg")]
    assert r[0].out == [b"\1", want, struct.pack("<Q", n)] and r[1].out == [b"\0"]          # check = false; verify is Ok
    assert r[2].out == r[0].out and r[3].out == [b"\0"]                                     # check = true
    assert r[4].out == [b"\1"] and r[5].out == [b"\0"]
    assert r[6].outcome == OK_ and r[7].out == [b"\2"] and r[8].out == [b"\1"] and r[9].out == [b"\2"]   # one bit of e_agg
    assert r[10].out == [b"\0"] and r[11].outcome == OK_ and r[12].outcome == PANIC, r[10:13]  # e_agg = q
    assert r[14].out == [b"\2"] and r[15].out == [b"\2"]                                    # one message bit; two keys swapped
    assert r[16].outcome == PANIC and r[17].outcome == PANIC                                # a key / a message short
    assert r[16].what == r[17].what == "We should have the same number of messages than public keys"
    assert r[18].out == [b"\0"]                                                             # a bad signature, checked: none
    assert r[19].outcome == OK_ and r[19].out[0] == b"\1" and r[19].out[1] != want          # unchecked: an aggregate all the same
    assert r[20].outcome == PANIC and r[21].outcome == PANIC                                # an undecodable signature
    # second witness: the Python mirror's engine
    st, agg = eng.aggregate(sigs, pks, msgs, check=False)[:2]
    assert st == 0 and agg.tobytes() == want
    assert eng.verify_aggregate(np.frombuffer(flipped, np.uint8), pks, msgs) == 2


# ---- g. self-checks -------------------------------------------------------------------------------------------------------
def test_selfchecks_name_the_eight_words_in_order(driver, oracle, eng, lanes, tmp_path):
    import schnorr_sig_amd as ssa
    ln = lanes
    f = pm.FIXTURE_SMALL_ORDER_PK
    small = np.frombuffer(pm.fp6_to_bytes48(f[0]) + pm.fp6_to_bytes48(f[1]), np.uint8)
    pks = np.stack([ln.pks2[0], ln.pks2[1], small, ln.pks2[2], ln.pks2[3]])
    inf = np.zeros(5, np.uint8)
    sk = ln.sks2[0].tobytes()
    steps = [("ctx_selfcheck",), ("kp_from_bytes", sk), ("rng", bytes(range(64))), ("kp_sign", b"builds the constant-time table"),
             ("ctx_selfcheck",), ("pks", pks, inf)]
    for kind in ("Ladder", "Comb"):
        steps += [("keyset_create", kind), ("keyset_selfcheck", b"\0"), ("keyset_selfcheck", b"\1")]
    res = driver.run(tmp_path, steps)
    all_returned(res)
    fresh = ssa.Engine(0)
    try:
        first = fresh.selfcheck()
        ssa.KeyPair.from_bytes(sk, fresh).sign(b"builds the constant-time table", lambda k: bytes(range(64)), fresh)
        second = fresh.selfcheck()
    finally:
        fresh.close()
    for s, p in ((res[0], first), (res[4], second)):
        assert s.words() == [p[k] for k in ssa.SELFCHECK_FIELDS] and s.out[1] == bytes([p["ok"]]) and p["ok"], (s.words(), p)
    assert second["ctab_rows"] > first["ctab_rows"] == 0 and first["rows"] > 0 and first["bits"] > 0
    k = 6
    for kind in ("ladder", "comb"):
        assert res[k].words() == [5]
        ks = eng.keyset_create(pks, pk_inf=inf, kind=kind)
        try:
            for deep in (False, True):
                p, s = ks.selfcheck(deep=deep), res[k + 1 + deep]
                assert s.words() == [p[f] for f in ssa.KEYCHECK_FIELDS], (kind, deep, s.words(), p)
                assert s.out[1] == bytes([p["ok"]]) and s.out[2] == p["bad"].tobytes() and len(s.out[2]) == 5
                assert p["keys_checked"] == 5 and (p["comb_rows_checked"] > 0) == (kind == "comb")
        finally:
            ks.close()
        k += 3


# ---- h. derivation --------------------------------------------------------------------------------------------------------
def test_hierarchical_derivation_equals_the_model(driver, oracle, tmp_path):
    rng = np.random.default_rng(77801)
    seeds = [bytes(32), bytes(rng.integers(0, 256, 32, dtype=np.uint8)), b"\xff" * 32,
             bytes(rng.integers(0, 256, 32, dtype=np.uint8))]
    chain = [bytes([5, 0, 0, 0]), bytes([0, 0, 0, 0x80]), bytes([1, 2, 3, 4])]
    pub = lambda sk: pm.pt_decompress(oracle.compress(oracle.keygen(le32(sk))[0]))[1]   # [sk]G as a model point
    steps, want = [], []
    for seed in seeds:
        sk, cc = dm.master(seed)
        steps.append(("xprv_master", seed)); want.append([b"\1", dm.xprv_bytes(sk, cc)])
        steps.append(("xpub_from_xprv",)); want.append([b"\1", dm.xpub_bytes(pub(sk), cc)])
        for i in chain:
            iv = int.from_bytes(i, "little")
            child = dm.derive_private(sk, cc, iv, pk49=oracle.compress(oracle.keygen(le32(sk))[0]))
            cpub = dm.xpub_bytes(pub(child[0]), child[1])
            # xprv -> public child; for a normal index the same child from the xpub, by the method and the free function
            steps.append(("xprv_derive_public", i)); want.append([b"\1", cpub])
            steps.append(("xpub_from_xprv",)); want.append([b"\1", dm.xpub_bytes(pub(sk), cc)])
            if dm.is_hardened(iv):
                steps.append(("xpub_derive_normal_public", i)); want.append([b"\0"])
                steps.append(("free_derive_public", i)); want.append(PANIC)
            else:
                via = dm.derive_normal_public(pub(sk), cc, iv)
                assert dm.xpub_bytes(*via) == cpub
                steps.append(("free_derive_public", i)); want.append([cpub[:49], cpub[49:]])
                steps.append(("xpub_derive_normal_public", i)); want.append([b"\1", cpub])
            steps.append(("free_derive_private", i)); want.append([le32(child[0]), child[1]])
            steps.append(("xprv_derive_private", i)); want.append([b"\1", dm.xprv_bytes(*child)])
            sk, cc = child
    # ExtendedPublicKey::from_bytes, ExtendedPrivateKey::from_bytes
    good = dm.xpub_bytes(pub(sk), cc)
    ident = oracle.compress(bytes(96), True) + cc
    steps += [("xpub_from_bytes", good), ("xpub_from_bytes", ident), ("xpub_from_bytes", off_curve_x(oracle, rng) + cc),
              ("xpub_from_bytes", good[:48] + b"\xff" + cc), ("xprv_from_bytes", le32(Q) + cc), ("xprv_from_bytes", le32(Q - 1) + cc)]
    want += [[b"\1", good, key97(oracle.decompress(good[:49])[0]), b"\1"], [b"\0"], [b"\0"], [b"\0"], [b"\0"], [b"\1", le32(Q - 1) + cc]]
    res = driver.run(tmp_path, steps)
    assert len({w[1] for w in want if isinstance(w, list) and len(w) > 1}) > 4 * 6
    for s, w in zip(res, want):
        if w == PANIC:
            assert s.outcome == PANIC, s
        else:
            assert s.outcome == OK_ and s.out == w and s.rng_used == 0, (s, [x.hex() for x in s.out], [x.hex() for x in w])
