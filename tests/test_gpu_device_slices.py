"""Device-buffer entry points over a batch cut into slices (ssa_ctx.hpp: DevBatch::slice, the one rule for cutting a
device batch): on a context with small slices every sliced device form gives what the one-slice engine gives.  The
messages come by offset table (the table moves with a slice, the message bytes stay put), identity-key flags ride
along, and the rejected lanes sit in every slice, next to its boundaries:
 * lane slices of 4096: four slices, alternating between the context's stream and its twin's;
 * MSM slices of 5000: 5000 / 5000 / 2345, the last on the small-batch cooperative path (and, screened, the exact
   per-lane path)."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 12345
LANE_SLICE, MSM_SLICE = 4096, 5000
BAD = [4095, 4096, 4999, 5000, 8191, 9999, 10000, 12344]
INF_BAD = [4095, 9999]      # spoiled lanes that also carry an identity-key flag


def _scalars(rng, n):
    s = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    s[:, 31] &= 0x3F
    s[:, 0] |= 1
    return s


@pytest.fixture(scope="module")
def sliced():
    """an engine whose per-lane kernels and MSM pipeline run in slices of LANE_SLICE / MSM_SLICE (read at creation)"""
    import schnorr_sig_amd as ssa
    os.environ["SSA_LANE_SLICE"], os.environ["SSA_MSM_SLICE"] = str(LANE_SLICE), str(MSM_SLICE)
    try:
        eng = ssa.Engine(0)
    finally:
        del os.environ["SSA_LANE_SLICE"], os.environ["SSA_MSM_SLICE"]
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def batches(engine):
    """{"honest": ..., "spoiled": ...}: (sigs, pks, message bytes, pk_inf) with ONE offset table (lengths 0-40), and
    32-byte coefficients below 2^128 (one value for every path: a narrower width may be read as signed)"""
    rng = np.random.default_rng(0xD5C1)
    lens = rng.integers(0, 41, size=N)
    lens[BAD] = np.maximum(lens[BAD], 1)
    off = np.zeros(N + 1, np.uint64)
    off[1:] = np.cumsum(lens)
    flat = rng.integers(0, 256, size=int(off[-1]), dtype=np.uint8)
    pks, sigs = engine.keygen_sign_many(_scalars(rng, N), _scalars(rng, N), flat, offsets=off)
    bsigs, bpks, bflat = sigs.copy(), pks.copy(), flat.copy()
    for k, i in enumerate(BAD):
        if k % 4 == 0:
            bsigs[i, 49] ^= 1                       # e bit flip
        elif k % 4 == 1:
            bflat[int(off[i])] ^= 0x20              # message bit flip
        elif k % 4 == 2:
            bpks[i] = pks[i - 1]                    # someone else's key
        else:
            bsigs[i, :49] = sigs[i - 1, :49]        # someone else's R
    inf = np.zeros(N, np.uint8)
    binf = inf.copy()
    binf[INF_BAD] = 1
    coeffs = rng.integers(0, 256, size=(N, 32), dtype=np.uint8)
    coeffs[:, 16:] = 0
    return {"honest": (sigs, pks, flat, inf), "spoiled": (bsigs, bpks, bflat, binf)}, off, coeffs


def _dev(*arrays):
    import torch
    out = [torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0") for a in arrays]
    torch.cuda.synchronize()
    return out


def _ptrs(batch, off, coeffs):
    """device copies (kept alive by the caller) and their addresses: sigs, pks, messages, offsets, pk_inf, coeffs"""
    sigs, pks, flat, inf = batch
    bufs = _dev(sigs, pks, flat, off.view(np.int64), inf, coeffs)
    return bufs, [b.data_ptr() for b in bufs]


def _verify_many_device(eng, batch, off, **kw):
    import torch
    bufs, (ds, dp, dm, do, di, _) = _ptrs(batch, off, np.zeros(32, np.uint8))
    st = torch.full((N,), 255, dtype=torch.uint8, device="cuda:0")
    nf = torch.full((1,), -1, dtype=torch.int64, device="cuda:0")
    eng.verify_many_device(ds, dp, dm, N, 0, st.data_ptr(), nf.data_ptr(), d_offsets=do, d_pk_inf=di, mode="lane", **kw)
    eng.sync()
    return st.cpu().numpy(), int(nf.item())


def _sample_matches_oracle(oracle, batch, off, status, **kw):
    """the oracle on the spoiled lanes, the slice boundaries and every 97th lane"""
    sigs, pks, flat, inf = batch
    samp = np.unique(np.concatenate([BAD, np.arange(0, N, 97), [0, 4097, 8192, 12287, 12288, N - 1]]))
    lens = (off[samp + 1] - off[samp]).astype(np.int64)
    sub_off = np.zeros(samp.size + 1, np.uint64)
    sub_off[1:] = np.cumsum(lens)
    sub_flat = np.concatenate([flat[int(off[i]):int(off[i + 1])] for i in samp])
    exp = oracle.verify_many(sigs[samp], pks[samp], sub_flat, offsets=sub_off, pk_inf=inf[samp], **kw)
    return (status[samp] == exp).all()


@pytest.mark.parametrize("torsion", [False, True])
def test_verify_many_device_in_lane_slices(engine, sliced, batches, oracle, torsion):
    data, off, _ = batches
    for name, batch in data.items():
        ref, nf_ref = _verify_many_device(engine, batch, off, check_torsion=torsion)
        got, nf = _verify_many_device(sliced, batch, off, check_torsion=torsion)
        assert (got == ref).all() and nf == nf_ref == int((ref != 0).sum()), name
        assert sorted(np.flatnonzero(ref)) == (BAD if name == "spoiled" else []), name
        assert _sample_matches_oracle(oracle, batch, off, got, check_torsion=torsion), name


def test_msm_device_forms_in_slices(engine, sliced, batches, oracle):
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import msm_records as mr
    data, off, coeffs = batches
    for name, want in (("honest", 0), ("spoiled", 2)):
        bufs, (ds, dp, dm, do, di, dc) = _ptrs(data[name], off, coeffs)
        verdicts, records = [], []
        for eng in (engine, sliced):
            v = torch.full((1,), 255, dtype=torch.int32, device="cuda:0")
            rec = torch.zeros(24, dtype=torch.int64, device="cuda:0")
            eng.verify_batch_msm_device(ds, dp, dm, N, 0, dc, 32, v.data_ptr(), d_offsets=do, d_pk_inf=di)
            eng.verify_batch_msm_partial_device(ds, dp, dm, N, 0, dc, 32, rec.data_ptr(), d_offsets=do, d_pk_inf=di)
            eng.sync()
            verdicts.append(int(v.item()))
            records.append(rec.cpu().numpy().view(np.uint64))
        assert verdicts == [want, want], name
        r1, r2 = records
        assert mr.record_is_wellformed(oracle, r1) and mr.record_is_wellformed(oracle, r2), name
        assert mr.record_point(oracle, r1) == mr.record_point(oracle, r2), name
        assert mr.record_lin(r1) == mr.record_lin(r2), name


def test_screened_device_in_slices(engine, sliced, batches, oracle):
    import torch
    data, off, coeffs = batches
    for name, batch in data.items():
        ref, nf_ref = _verify_many_device(engine, batch, off, check_torsion=False, sig_flag_byte=True)
        bufs, (ds, dp, dm, do, di, dc) = _ptrs(batch, off, coeffs)
        st = torch.full((N,), 255, dtype=torch.uint8, device="cuda:0")
        nf = torch.full((1,), -1, dtype=torch.int64, device="cuda:0")
        sliced.verify_batch_screened_device(ds, dp, dm, N, 0, dc, 32, st.data_ptr(), nf.data_ptr(), d_offsets=do,
                                            d_pk_inf=di)
        sliced.sync()
        got = st.cpu().numpy()
        assert (got == ref).all() and int(nf.item()) == nf_ref == int((ref != 0).sum()), name
        assert sorted(np.flatnonzero(got)) == (BAD if name == "spoiled" else []), name
        assert _sample_matches_oracle(oracle, batch, off, got, check_torsion=False, sig_flag_byte=True), name
