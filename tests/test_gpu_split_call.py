"""One-slice calls of the lane kernels as two unequal parts on the context's two streams.

The split is forced by the debug setter at sizes just above the cooperative crossovers (7680 lanes, 10496 with the
subgroup check), where a launch is a few ms: n = limit + 1 + 256 k + r.  Part A = lanes [0, nA) runs on the caller's
stream, part B = [nA, n) on the twin's, into disjoint ranges of the same workspaces, status array and counter -- so the
status bytes and the count must be those of the same context with the split off, and those of the oracle, whatever
sits on either side of the cut; the call must keep the stream order of an unsplit call; and with timing on it records
one entry per key."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COOP = {False: 7680, True: 10496}          # the cooperative kernel's crossovers without / with the subgroup check
N_MAX = 10497 + 256 * 3 + 255              # the largest n of any case below
FRAC = 4                                   # the forced share of part B, in 1/16ths


def _scalars(rng, n):
    s = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    s[:, 31] &= 0x3F
    s[:, 0] |= 1
    return s


def _small_order_key():
    """the reference's non-subgroup point (src/signature.rs:387-404) as 96 affine bytes"""
    with open(os.path.join(ROOT, "tests", "golden", "vectors.json")) as fh:
        f = json.load(fh)["fixture_small_order_pk"]
    return np.frombuffer(b"".join(int(x).to_bytes(8, "little") for x in (f["x"] + f["y"])), dtype=np.uint8)


@pytest.fixture(scope="module")
def data(engine, oracle):
    """N_MAX honest lanes, signed once over 80-byte rows and once over ragged messages (offset table), and the oracle's
    statuses of all of them for both flag words: computed once, shared by every case, never modified"""
    rng = np.random.default_rng(0x5B117)
    sks, nonces = _scalars(rng, N_MAX), _scalars(rng, N_MAX)
    msgs = rng.integers(0, 256, size=(N_MAX, 80), dtype=np.uint8)
    pks, sigs = engine.keygen_sign_many(sks, nonces, msgs)
    lens = rng.integers(0, 120, size=N_MAX)
    lens[:3] = [0, 1, 119]
    off = np.zeros(N_MAX + 1, np.uint64)
    off[1:] = np.cumsum(lens)
    flat = rng.integers(0, 256, size=int(off[-1]) + 1, dtype=np.uint8)
    pks_r, sigs_r = engine.keygen_sign_many(sks, nonces, flat, offsets=off)
    assert (pks_r == pks).all()
    d = {"sigs": sigs, "pks": pks, "msgs": msgs, "sigs_r": sigs_r, "flat": flat, "off": off}
    for torsion in (False, True):
        d["oracle", torsion] = oracle.verify_many(sigs, pks, msgs, check_torsion=torsion, sig_flag_byte=not torsion)
        assert (d["oracle", torsion] == 0).all()
    d["oracle_r"] = oracle.verify_many(sigs_r, pks, flat, offsets=off, check_torsion=False, sig_flag_byte=True)
    assert (d["oracle_r"] == 0).all()
    for v in d.values():
        v.setflags(write=False)
    return d


@pytest.fixture(scope="module")
def eng():
    """the context under test: its split is switched on and off by the debug setter.  A test process holds other contexts
    on the device (the session's engine), beside which no call is split unless told to: alone=0"""
    import schnorr_sig_amd as ssa
    e = ssa.Engine(0)
    e.debug_split_config(alone=0)
    e.enable_timing(True)             # (_run tells from the timing entries whether a call was split)
    yield e
    e.close()


def _shape(ssa, torsion, kind):
    """n = limit + 1 + 256 k + r and its plan at FRAC/16: r chosen so that B ends in a ragged block behind whole ones,
    B is a single ragged block, or n is a multiple of 256.  Returns (n, share, nA, nB, mode of the call)."""
    base = COOP[torsion] + 1
    mode = None
    if kind == "multiple":
        n = base + 256 * 2 + 255
        assert n % 256 == 0
        frac = FRAC
    elif kind == "ragged":
        n = base + 256 * 3 + 100
        frac = FRAC
    else:
        # one ragged block: the smallest share, and the r that leaves B under 256 lanes.  Above 10496 lanes a sixteenth is
        # more than 400 lanes whatever r is, so with the subgroup check this shape runs at n = 3841 + r with the lane
        # kernels forced (SSA_FLAG_FORCE_LANE)
        frac = 1
        if torsion:
            base, mode = 3841, "lane"
        n = next(m for m in range(base, base + 512)
                 if 64 < ssa.debug_split_plan(m, 1, check_torsion=torsion, force_lane=torsion)[1] < 256)
    nA, nB = ssa.debug_split_plan(n, frac, check_torsion=torsion, force_lane=mode == "lane")
    assert nA + nB == n and nA % 256 == 0 and 0 < nB <= nA
    if kind == "ragged":
        assert nB > 512 and nB % 256 != 0
    elif kind == "single":
        assert 64 < nB < 256
    return n, frac, nA, nB, mode


def _device(torch, *arrays):
    dev = torch.device("cuda", 0)
    return [torch.from_numpy(np.array(a)).to(dev) for a in arrays]          # (a copy: the shared arrays are read-only)


def _run(torch, e, d_sigs, d_pks, d_msgs, n, torsion, d_inf=None, d_off=None, mode=None, split=None):
    """one device call on e; returns (status bytes, count).  split True / False: e has timing on, and the call must /
    must not have run as two parts (a split call leaves an entry of two launches under each key)"""
    dev = d_sigs.device
    dst = torch.full((n,), 255, dtype=torch.uint8, device=dev)
    dnf = torch.full((1,), -1, dtype=torch.int64, device=dev)
    if split is not None:
        for key in ("ssa_k_hash", "ssa_k_verify"):
            e.read_timing(key)              # (whatever earlier calls left)
    e.verify_many_device(d_sigs.data_ptr(), d_pks.data_ptr(), d_msgs.data_ptr(), n, 80, dst.data_ptr(), dnf.data_ptr(),
                         d_offsets=d_off.data_ptr() if d_off is not None else 0,
                         d_pk_inf=d_inf.data_ptr() if d_inf is not None else 0,
                         check_torsion=torsion, sig_flag_byte=not torsion, mode=mode)
    e.sync()
    if split is not None:
        for key in ("ssa_k_hash", "ssa_k_verify"):
            assert (e.debug_split_timing(key) is not None) == split, (key, split)
            assert e.read_timing(key)[1] == 1
    return dst.cpu().numpy(), int(dnf.item())


BAD_KINDS = ("e", "x", "key", "small")


def _spoil(sigs, pks, lane, kind, n):
    if kind == "e":                 # a bit of e: InvalidSignature
        sigs[lane, 49] ^= 1
    elif kind == "x":               # a non-canonical limb of the signature's x: malformed
        sigs[lane, 0:8] = 0xFF
    elif kind == "key":             # someone else's key: InvalidSignature
        pks[lane] = pks[(lane + 7) % n]
    else:                           # the reference's small-order point: InvalidPublicKey with the subgroup check
        pks[lane] = _small_order_key()


@pytest.mark.parametrize("kind", ["ragged", "single", "multiple"])
@pytest.mark.parametrize("torsion", [False, True])
def test_split_call_equals_unsplit_call_and_oracle(data, eng, oracle, torsion, kind):
    """both flag words (SSA_FLAG_SIG_FLAG_BYTE alone, SSA_FLAG_CHECK_TORSION), the three shapes of part B; bad lanes of
    every kind at lanes 0, nA - 1, nA and n - 1 (the kinds rotate over the four lanes: four rounds put each kind on each),
    pk_inf set on both sides of the cut.  Split and unsplit calls alternate on the one context: split, unsplit, split."""
    import torch
    import schnorr_sig_amd as ssa
    n, frac, nA, nB, mode = _shape(ssa, torsion, kind)
    edge = [0, nA - 1, nA, n - 1]
    for rnd in range(4):
        sigs, pks = data["sigs"][:n].copy(), data["pks"][:n].copy()
        for j, lane in enumerate(edge):
            _spoil(sigs, pks, lane, BAD_KINDS[(j + rnd) % 4], n)
        inf = np.zeros(n, np.uint8)
        inf[[nA - 2, nA + 1]] = 1
        touched = np.array(sorted(set(edge + [nA - 2, nA + 1])))
        want = data["oracle", torsion][:n].copy()
        want[touched] = oracle.verify_many(sigs[touched], pks[touched], data["msgs"][touched], check_torsion=torsion,
                                           pk_inf=inf[touched], sig_flag_byte=not torsion)
        assert (want[edge] != 0).all()
        ds, dp, dm, di = _device(torch, sigs, pks, data["msgs"][:n], inf)
        runs = []
        for f in (frac, 0, frac):
            eng.debug_split_config(split_min=0, split_frac=f)
            runs.append(_run(torch, eng, ds, dp, dm, n, torsion, d_inf=di, mode=mode, split=f != 0))
        eng.debug_split_config(split_frac=0)
        for st, nf in runs:
            assert nf == int((want != 0).sum())
            bad = np.nonzero(st != want)[0]
            assert bad.size == 0, (bad[:8], st[bad[:8]], want[bad[:8]], nA, n)


def test_split_call_offset_table_unequal_lengths(data, eng):
    """the offsets-table form: part B's offsets are the table moved by nA entries (the message bytes stay put), lengths
    from 0 to 119 bytes, bad lanes on both sides of the cut"""
    import torch
    import schnorr_sig_amd as ssa
    n, frac, nA, nB, _ = _shape(ssa, False, "ragged")
    sigs, pks = data["sigs_r"][:n].copy(), data["pks"][:n].copy()
    flat = data["flat"].copy()
    off = data["off"][:n + 1]
    want = data["oracle_r"][:n].copy()
    for lane in (0, nA - 1, nA, n - 1):
        sigs[lane, 49] ^= 1
        want[lane] = 2
    lane = next(i for i in range(nA + 1, n) if off[i + 1] > off[i])       # a message byte of part B
    flat[int(off[lane])] ^= 0x10
    want[lane] = 2
    ds, dp, dm, do = _device(torch, sigs, pks, flat, off.astype(np.int64))
    for f in (0, frac, 0):
        eng.debug_split_config(split_min=0, split_frac=f)
        st, nf = _run(torch, eng, ds, dp, dm, n, False, d_off=do, split=f != 0)
        assert nf == 5 and (st == want).all(), (f, np.nonzero(st != want)[0][:8])
    eng.debug_split_config(split_frac=0)


def test_split_call_keeps_the_stream_order(data, eng):
    """on a stream of the caller's: the inputs are written on that stream immediately before the call (over zeros),
    overwritten on it immediately after, and the status and the count are consumed on it -- no host synchronisation in
    between.  Part B runs on another stream: it must not start before the inputs exist, and the caller's stream must
    not go on before it has ended."""
    import torch
    import schnorr_sig_amd as ssa
    n, frac, nA, nB, _ = _shape(ssa, False, "ragged")
    sigs, pks = data["sigs"][:n].copy(), data["pks"][:n]
    want = np.zeros(n, np.uint8)
    for lane in (1, nA - 1, nA, nA + 300, n - 1):
        sigs[lane, 49] ^= 1
        want[lane] = 2
    src_s, src_p, src_m = _device(torch, sigs, pks, data["msgs"][:n])
    dev = src_s.device
    ds, dp, dm = (torch.zeros_like(t) for t in (src_s, src_p, src_m))
    dst = torch.full((n,), 255, dtype=torch.uint8, device=dev)
    dnf = torch.full((1,), -1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device=dev)
    eng.debug_split_config(split_min=0, split_frac=frac)
    eng.set_stream(s.cuda_stream)
    try:
        got = []
        for rep in range(3):
            with torch.cuda.stream(s):
                ds.copy_(src_s, non_blocking=True)
                dp.copy_(src_p, non_blocking=True)
                dm.copy_(src_m, non_blocking=True)
                eng.verify_many_device(ds.data_ptr(), dp.data_ptr(), dm.data_ptr(), n, 80, dst.data_ptr(), dnf.data_ptr(),
                                       check_torsion=False, sig_flag_byte=True)
                for t in (ds, dp, dm):
                    t.zero_()
                got.append((dst.clone(), dnf.clone()))
                dst.fill_(255)
                dnf.fill_(-1)
        s.synchronize()
        for st, nf in got:
            assert int(nf.item()) == 5 and (st.cpu().numpy() == want).all()
        assert eng.debug_split_timing("ssa_k_verify") is not None          # (the calls were split)
    finally:
        eng.set_stream(None)
        eng.debug_split_config(split_frac=0)


def test_part_b_with_an_end_game_of_its_own(data):
    """SSA_SPLIT_TAIL_B: with a "generation" of 8 waves both parts are long enough for an end game, part A's in the
    context's buffers and part B's in the twin's; same results as the unsplit call of the same context"""
    import torch
    import schnorr_sig_amd as ssa
    os.environ["SSA_TAIL_WAVES"] = "8"
    try:
        e = ssa.Engine(0)
    finally:
        del os.environ["SSA_TAIL_WAVES"]
    try:
        n, frac, nA, nB, _ = _shape(ssa, True, "ragged")
        sigs, pks = data["sigs"][:n].copy(), data["pks"][:n].copy()
        for j, lane in enumerate((0, nA - 1, nA, n - 1)):
            _spoil(sigs, pks, lane, BAD_KINDS[j], n)
        ds, dp, dm = _device(torch, sigs, pks, data["msgs"][:n])
        ref = _run(torch, e, ds, dp, dm, n, True)
        assert ref[1] == 4 and sorted(np.nonzero(ref[0])[0]) == [0, nA - 1, nA, n - 1]
        for tail_b in (1, 0, 1):
            e.debug_split_config(split_min=0, split_frac=frac, tail_b=tail_b, alone=0)
            e.enable_timing(True)
            st, nf = _run(torch, e, ds, dp, dm, n, True, split=True)
            assert nf == ref[1] and (st == ref[0]).all()
    finally:
        e.close()


def test_context_without_a_twin_never_splits(data):
    """SSA_TWO_STREAMS=0: the knobs ask for a split, the call runs as one pair of launches on the one stream"""
    import torch
    import schnorr_sig_amd as ssa
    os.environ["SSA_TWO_STREAMS"] = "0"
    try:
        e = ssa.Engine(0)
    finally:
        del os.environ["SSA_TWO_STREAMS"]
    try:
        assert not e.info()["two_streams"]
        n, frac, nA, nB, _ = _shape(ssa, False, "ragged")
        sigs = data["sigs"][:n].copy()
        sigs[nA, 49] ^= 1
        ds, dp, dm = _device(torch, sigs, data["pks"][:n], data["msgs"][:n])
        e.debug_split_config(split_min=0, split_frac=frac, alone=0)
        e.enable_timing(True)
        before = e.info()["workspace_bytes"]
        st, nf = _run(torch, e, ds, dp, dm, n, False)
        assert nf == 1 and st[nA] == 2 and int((st != 0).sum()) == 1
        assert e.debug_split_timing("ssa_k_hash") is None and e.debug_split_timing("ssa_k_verify") is None
        assert e.read_timing("ssa_k_hash")[1] == 1 and e.read_timing("ssa_k_verify")[1] == 1
        assert e.info()["workspace_bytes"] >= before
    finally:
        e.close()


def test_split_call_records_one_timing_entry_per_key(data):
    """after ONE split call each key reports count 1, and its time -- from the earlier start to the later end of the two
    launches -- is at least each part's own; the twin keeps no entry; the workspaces are those of the unsplit call plus
    the twin's few hundred bytes"""
    import torch
    import schnorr_sig_amd as ssa
    n, frac, nA, nB, _ = _shape(ssa, False, "ragged")
    ds, dp, dm = _device(torch, data["sigs"][:n], data["pks"][:n], data["msgs"][:n])
    one, two = ssa.Engine(0), ssa.Engine(0)
    try:
        _run(torch, one, ds, dp, dm, n, False)
        two.debug_split_config(split_min=0, split_frac=frac, alone=0)
        two.enable_timing(True)
        st, nf = _run(torch, two, ds, dp, dm, n, False)
        assert nf == 0 and (st == 0).all()
        for key in ("ssa_k_hash", "ssa_k_verify"):
            span, a, b = two.debug_split_timing(key)
            print("%s: span %.3f ms, part A %.3f ms, part B %.3f ms" % (key, span, a, b))
            assert a > 0 and b > 0 and span >= a and span >= b
            avg, count = two.read_timing(key)
            assert count == 1 and avg == pytest.approx(span, rel=1e-6)
            assert two.read_timing(key)[1] == 0             # (read and gone, the twin's list included)
        extra = two.info()["workspace_bytes"] - one.info()["workspace_bytes"]
        assert 0 <= extra < 4096, extra
    finally:
        one.close()
        two.close()


def test_context_beside_another_on_the_device_does_not_split(data, engine):
    """a call is split only while its context is the one context of the process on its device: two contexts that each
    split their half of a batch get in each other's way.  Beside the session's engine the knobs alone split nothing;
    SSA_SPLIT_ALONE=0 (here: the setter) does; results are the same either way"""
    import torch
    import schnorr_sig_amd as ssa
    n, frac, nA, nB, _ = _shape(ssa, False, "ragged")
    sigs = data["sigs"][:n].copy()
    sigs[[nA - 1, nA], 49] ^= 1
    ds, dp, dm = _device(torch, sigs, data["pks"][:n], data["msgs"][:n])
    e = ssa.Engine(0)
    try:
        e.enable_timing(True)
        e.debug_split_config(split_min=0, split_frac=frac)
        ref = _run(torch, e, ds, dp, dm, n, False)
        assert ref[1] == 2 and sorted(np.nonzero(ref[0])[0]) == [nA - 1, nA]
        assert e.debug_split_timing("ssa_k_verify") is None and e.read_timing("ssa_k_verify")[1] == 1
        e.debug_split_config(alone=0)
        st, nf = _run(torch, e, ds, dp, dm, n, False)
        assert nf == 2 and (st == ref[0]).all()
        assert e.debug_split_timing("ssa_k_verify") is not None and e.read_timing("ssa_k_verify")[1] == 1
    finally:
        e.close()


def test_host_forms_are_never_split(data):
    """only the exported ssa_verify_many_device splits, not the library's own uses of it: a host batch of more than one
    slice drives the context and its twin from two threads, where a split on one would reach into the twin under the other.
    A staged host slice (SSA_PIPELINE_CHUNKS=1: no upload pipeline, so the call goes through verify_launch) with every
    knob asking for a split runs as one pair of launches; so do the two slices of a larger host batch, one on the context and one on its twin; the same context
    splits its device calls"""
    import torch
    import schnorr_sig_amd as ssa
    n, frac, nA, nB, _ = _shape(ssa, False, "ragged")
    sigs = data["sigs"][:n].copy()
    sigs[[0, nA - 1, nA, n - 1], 49] ^= 1
    pks, msgs = np.array(data["pks"][:n]), np.array(data["msgs"][:n])
    env = {"SSA_PIPELINE_CHUNKS": "1", "SSA_LANE_SLICE": "8192"}
    os.environ.update(env)
    try:
        e = ssa.Engine(0)
    finally:
        for k in env:
            del os.environ[k]
    try:
        e.debug_split_config(split_min=0, split_frac=frac, alone=0)
        e.enable_timing(True)
        for m, launches in ((8192, 1), (n, 2)):        # one slice; two slices, the second on the twin
            st, nf = e.verify_many(sigs[:m], pks[:m], msgs[:m], check_torsion=False, mode="lane", sig_flag_byte=True)
            want = np.zeros(m, np.uint8)
            want[[i for i in (0, nA - 1, nA, n - 1) if i < m]] = 2
            assert nf == int((want != 0).sum()) and (st == want).all()
            assert e.debug_split_timing("ssa_k_hash") is None and e.debug_split_timing("ssa_k_verify") is None
            assert e.read_timing("ssa_k_hash")[1] == launches and e.read_timing("ssa_k_verify")[1] == launches
        # the keyed records (KeyedSignature::verify) reach the same launches through the library's own use of
        # ssa_verify_many_device: host form at one slice and at two (8192 lanes on the context, the rest on its twin,
        # where it takes the cooperative kernel), and the device form
        comp, stc = e.compress_many(pks)
        assert (stc == 0).all()
        keyed = np.concatenate([comp, sigs], axis=1)
        for m in (8192, n):
            st, nf = e.verify_keyed_many(keyed[:m], msgs[:m], check_torsion=False)
            want = np.zeros(m, np.uint8)
            want[[i for i in (0, nA - 1, nA, n - 1) if i < m]] = 2
            assert nf == int((want != 0).sum()) and (st == want).all()
            assert e.debug_split_timing("ssa_k_hash") is None and e.debug_split_timing("ssa_k_verify") is None
            assert e.read_timing("ssa_k_hash")[1] == 1 and e.read_timing("ssa_k_verify")[1] == 1
        dk, dm = _device(torch, keyed[:8192], msgs[:8192])
        dst = torch.full((8192,), 255, dtype=torch.uint8, device=dk.device)
        dnf = torch.full((1,), -1, dtype=torch.int64, device=dk.device)
        e.verify_keyed_many_device(dk.data_ptr(), dm.data_ptr(), 8192, 80, dst.data_ptr(), dnf.data_ptr(),
                                   check_torsion=False)
        e.sync()
        assert int(dnf.item()) == int((dst != 0).sum().item()) == sum(1 for i in (0, nA - 1, nA, n - 1) if i < 8192)
        assert e.debug_split_timing("ssa_k_hash") is None and e.debug_split_timing("ssa_k_verify") is None
        assert e.read_timing("ssa_k_hash")[1] == 1 and e.read_timing("ssa_k_verify")[1] == 1
        ds, dp, dm = _device(torch, sigs[:8192], pks[:8192], msgs[:8192])
        st, nf = _run(torch, e, ds, dp, dm, 8192, False, split=True)
        assert nf == int((st != 0).sum()) == sum(1 for i in (0, nA - 1, nA, n - 1) if i < 8192)
    finally:
        e.close()
