"""A table of calls for the call-order and concurrency tests (test_gpu_call_order.py, test_gpu_concurrent_contexts.py).

A step is (family, variant, n, seed).  inputs(step, maker) builds its inputs, which depend on the seed alone: the honest
signatures come from maker.keygen_sign_many (any engine gives the same bytes) and a known set of bad lanes is put on
top.  expected(step, inp) gives what must come out BY CONSTRUCTION, for every lane; check_oracle compares the touched lanes
and a strided sample of clean ones with the CPU oracle.  run(step, eng, objs, maker) makes the call on engine `eng`
(objs: the key set, caches and signer set that live on it) and returns a dict of results; same(a, b, orc) compares two
such dicts exactly -- MSM shard records through tests/msm_records.py (affine point and lin: the Jacobian representative
is not a contract).

What the oracle does NOT cover, within its budget of about 300 lanes a step: the verdict of verify_batch_msm is computed
by the oracle only for n <= 300 with caller coefficients, the record of msm_partial only for n <= 100.  At 3072 .. 20 000
(window width 8 | 16, the tile of the bucket method) and for library-drawn coefficients the MSM verdicts rest on the
verdict known by construction (0, 2 or 3) alone; the lanes that make a batch bad are not checked one by one there.

The sizes are the smallest that straddle every dispatch boundary of the library, not the workload's own."""
import hashlib
from collections import namedtuple

import numpy as np

import derive_model as dm
import device_rng_model as rng_model
import msm_records as mr

Step = namedtuple("Step", "family variant n seed")

Q = mr.Q
P = mr.P
FL = {"T": dict(check_torsion=True, sig_flag_byte=False), "TF": dict(check_torsion=True, sig_flag_byte=True),
      "N": dict(check_torsion=False, sig_flag_byte=False), "F": dict(check_torsion=False, sig_flag_byte=True)}
ALL_KINDS = ("e_bit", "e_ge_q", "msg_bit", "noncanon_pk", "offsub", "identity")
RNG_PIN = bytes(range(100, 144))        # debug_pin_rng of the _rng signers (44 bytes)
H = dm.HARDENED
DIRTY_N = 20000
SLICE, SLICED_N = 5000, 12345           # SSA_LANE_SLICE / SSA_MSM_SLICE of the sliced engines and their batch


def make_scalars(rng, n):
    """the suite's one definition (imported at the first call, after pytest has collected that module itself)"""
    from test_gpu_screened_torsion import make_scalars as f
    return f(rng, n)


def coeffs32(rng, n):
    from test_gpu_screened_torsion import coeffs32 as f
    return f(rng, n)


def fixture_key():
    """the reference's key outside the prime-order subgroup (src/signature.rs:385-406)"""
    import pymodel as m
    f = m.FIXTURE_SMALL_ORDER_PK
    return np.frombuffer(m.fp6_to_bytes48(f[0]) + m.fp6_to_bytes48(f[1]), np.uint8)


def kind_status(kind, fl):
    """the status of a lane whose one defect is `kind`, under the flags fl"""
    return {"e_bit": 2, "e_ge_q": 3, "msg_bit": 2, "noncanon_pk": 3, "offsub": 1 if fl["check_torsion"] else 2,
            "identity": 0, "noncanon_rec": 3}[kind]


def make_batch(maker, seed, n, kinds=ALL_KINDS, msg_len=80, dirty=False):
    """n honest signatures by min(n, 37) signers, then min(12, n // 2) lanes (the first and the last among them) with one
    defect each, cycling over `kinds`.  dirty: every lane bad or malformed, pk_inf on every tenth."""
    rng = np.random.default_rng(seed)
    u = min(n, 37)
    idx = rng.integers(0, u, size=n)
    idx[:u] = np.arange(u)
    sks = make_scalars(rng, u)[idx]
    msgs = rng.integers(0, 256, size=(n, msg_len), dtype=np.uint8)
    pks, sigs = maker.keygen_sign_many(sks, make_scalars(rng, n), msgs)
    inf = np.zeros(n, np.uint8)
    lane_kind = {}
    if dirty:
        k = np.arange(n) % 5
        sigs[k == 0, 49] ^= 1
        sigs[k == 1, 49:] = 0xFF
        msgs[k == 2, 0] ^= 1
        pks[k == 3, 0:8] = 0xFF
        pks[k == 4] = fixture_key()
        inf[::10] = 1
    else:
        nb = min(12, n // 2) if kinds else 0
        lanes = []
        if nb:
            lanes = sorted({0, n - 1} | {int(v) for v in 1 + rng.choice(n - 2, nb - 2, replace=False)}) if nb > 2 else [0, n - 1][:nb]
        ident = []
        for j, i in enumerate(lanes):
            kind = kinds[j % len(kinds)]
            lane_kind[i] = kind
            if kind == "e_bit":
                sigs[i, 49] ^= 1
            elif kind == "e_ge_q":
                sigs[i, 49:81] = 0xFF
            elif kind == "msg_bit":
                msgs[i, int(rng.integers(0, msg_len))] ^= 0x10
            elif kind == "noncanon_pk":
                pks[i, 0:8] = 0xFF
            elif kind == "offsub":
                pks[i] = fixture_key()
            elif kind == "identity":
                ident.append(i)
        if ident:           # an identity key (pk_inf) with e = r and R = [r]G: the key contributes nothing
            r = make_scalars(rng, len(ident))
            rp, _ = maker.keygen_sign_many(r, r, msgs[ident])
            rc, _ = maker.compress_many(rp)
            pks[ident] = 0
            inf[ident] = 1
            sigs[ident, :49] = rc
            sigs[ident, 49:] = r
    return {"sigs": sigs, "pks": pks, "msgs": msgs, "inf": inf, "kinds": lane_kind, "n": n}


def keyed_records(maker, b):
    """pk(49) || sig(81) of a batch without identity or non-canonical keys, then a key that does not decode on two lanes"""
    n = b["n"]
    cpk, st = maker.compress_many(b["pks"])
    assert not st.any()
    rec = np.concatenate([cpk, b["sigs"]], axis=1)
    for i in ([n // 3, n // 2] if n >= 24 else []):
        if i not in b["kinds"]:
            rec[i, 0:8] = 0xFF
            b["kinds"][i] = "noncanon_rec"
    return np.ascontiguousarray(rec)


_KEYSET_KEYS = []


def keyset_keys(maker):
    """keys of the key sets, the same on every context: two honest ones, the fixture key, a non-canonical one (made once:
    afterwards no maker is needed)"""
    if not _KEYSET_KEYS:
        sks = make_scalars(np.random.default_rng(777001), 4)
        pks = maker.pubkey_many(sks)
        pks[2] = fixture_key()
        pks[3, 0:8] = 0xFF
        _KEYSET_KEYS.extend([sks, pks])
    return _KEYSET_KEYS[0], _KEYSET_KEYS[1].copy()


def signer_keys():
    return make_scalars(np.random.default_rng(777002), 5)


_INPUTS = {}


def inputs(step, maker):
    """the inputs of a step (built once, then shared and read-only)"""
    if step not in _INPUTS:
        inp = _build_inputs(step, maker)
        for v in inp.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _INPUTS[step] = inp
    return _INPUTS[step]


def _coeffs(rng, tag, n, dirty):
    if tag == "lib":
        return None
    if dirty:
        return np.full((n, 32), 0xFF, np.uint8)
    c = coeffs32(rng, n)
    if tag == "c16":
        c[:, 16:] = 0
    return c


def _build_inputs(step, maker):
    fam, var, n, seed = step
    v = var.split(".")
    dirty = v[-1] == "dirty"
    rng = np.random.default_rng(seed + 1)
    ml = 160 if dirty else 80
    if fam == "verify_many":
        return make_batch(maker, seed, n, msg_len=ml, dirty=dirty)
    if fam in ("verify_batch_msm", "msm_partial"):
        flavour = {"honest": (), "bad": ("e_bit", "msg_bit"), "malformed": ("e_bit", "e_ge_q")}[v[2] if fam == "verify_batch_msm" and not dirty else "bad"]
        b = make_batch(maker, seed, n, kinds=flavour, msg_len=ml, dirty=dirty)
        b["coeffs"] = _coeffs(rng, v[0], n, dirty)
        return b
    if fam in ("verify_batch_screened", "verify_many_dedup"):
        b = make_batch(maker, seed, n, msg_len=ml, dirty=dirty)
        if fam == "verify_batch_screened":
            b["coeffs"] = _coeffs(rng, v[0], n, dirty)
        return b
    if fam in ("verify_many_screened", "verify_many_cached"):
        b = make_batch(maker, seed, n, msg_len=ml, dirty=dirty)
        b["coeffs"] = _coeffs(rng, v[1], n, dirty)
        return b
    if fam in ("verify_keyed_many", "verify_keyed_many_cached"):
        b = make_batch(maker, seed, n, kinds=() if dirty else ("e_bit", "e_ge_q", "msg_bit", "offsub"), msg_len=ml)
        b["keyed"] = keyed_records(maker, b)
        if dirty:
            k = np.arange(n) % 4
            b["keyed"][k == 0, 49 + 49] ^= 1
            b["keyed"][k == 1, 49 + 49:] = 0xFF
            b["msgs"][k == 2, 0] ^= 1
            b["keyed"][k == 3, 0:8] = 0xFF
        if fam == "verify_keyed_many_cached":
            b["coeffs"] = _coeffs(rng, v[1], n, dirty)
        return b
    if fam == "verify_many_indexed":
        sks, keys = keyset_keys(maker)
        kidx = rng.integers(0, 2, size=n).astype(np.uint32)
        msgs = rng.integers(0, 256, size=(n, 80), dtype=np.uint8)
        _, sigs = maker.keygen_sign_many(sks[kidx], make_scalars(rng, n), msgs)
        kinds = {}
        nb = min(10, n // 2)
        lanes = sorted({0, n - 1} | {int(x) for x in 1 + rng.choice(n - 2, nb - 2, replace=False)})
        for j, i in enumerate(lanes):
            kind = ("e_bit", "e_ge_q", "msg_bit", "offsub", "noncanon_pk")[j % 5]
            kinds[i] = kind
            if kind == "e_bit":
                sigs[i, 49] ^= 1
            elif kind == "e_ge_q":
                sigs[i, 49:81] = 0xFF
            elif kind == "msg_bit":
                msgs[i, 5] ^= 0x10
            elif kind == "offsub":
                kidx[i] = 2
            else:
                kidx[i] = 3
        return {"sigs": sigs, "pks": keys[kidx], "msgs": msgs, "kidx": kidx, "kinds": kinds, "n": n,
                "inf": np.zeros(n, np.uint8)}
    if fam in ("keygen_sign_many", "pubkey_many", "rng_signers", "sign_many_indexed"):
        m = signer_keys()
        kidx = rng.integers(0, 5, size=n).astype(np.uint32)
        sks = make_scalars(rng, n) if fam in ("keygen_sign_many", "pubkey_many") else m[kidx]
        return {"sks": sks, "nonces": make_scalars(rng, n), "kidx": kidx, "n": n,
                "msgs": rng.integers(0, 256, size=(n, 37), dtype=np.uint8)}
    if fam == "hash_message_many":
        b = make_batch(maker, seed, n, kinds=())
        if v[0] == "offsets":
            lens = np.array([(0, 7, 8, 80, 160, 33)[i % 6] for i in range(n)])
            off = np.zeros(n + 1, np.uint64)
            off[1:] = np.cumsum(lens)
            b["off"] = off
            b["flat"] = rng.integers(0, 256, size=int(off[-1]) + 1, dtype=np.uint8)
        else:
            b["msgs"] = rng.integers(0, 256, size=(n, int(v[0][3:])), dtype=np.uint8)
        return b
    if fam == "rescue_hash_many":
        return {"felts": rng.integers(0, P, size=(n, int(v[0][1:])), dtype=np.uint64), "n": n}
    if fam == "compress_many":
        b = make_batch(maker, seed, n, kinds=("offsub", "identity"))
        return {"pks": b["pks"], "inf": b["inf"], "n": n}
    if fam == "decompress_many":
        b = make_batch(maker, seed, n, kinds=("offsub", "identity"))
        c, st = maker.compress_many(b["pks"], b["inf"])
        assert not st.any()
        bad = [n // 2, n // 3] if n >= 24 else []
        if bad:
            c[bad[0], 0:8] = 0xFF
            c[bad[1], 48] |= 0x03
        return {"comp": c, "bad": np.array(bad, np.int64), "n": n}
    if fam == "xprv_master_many":
        return {"seeds": rng.integers(0, 256, size=(n, 32), dtype=np.uint8), "n": n}
    if fam in ("xprv_derive_many", "xpub_derive_many"):
        par = [dm.master(rng.integers(0, 256, size=32, dtype=np.uint8).tobytes()) for _ in range(5)]
        sk = np.stack([np.frombuffer(p[0].to_bytes(32, "little"), np.uint8) for p in par])
        pk49, _ = maker.compress_many(maker.pubkey_many(sk))
        idx = rng.integers(0, 1 << 31, size=n).astype(np.uint32)
        idx[::3] |= np.uint32(H)
        return {"par": par, "pk49": pk49, "idx": idx, "pidx": rng.integers(0, 5, size=n).astype(np.uint32), "n": n,
                "xprv": np.stack([np.frombuffer(dm.xprv_bytes(*p), np.uint8) for p in par]),
                "xpub": np.stack([np.frombuffer(bytes(pk49[k]) + par[k][1], np.uint8) for k in range(5)])}
    if fam == "selfcheck":
        return {"n": 0}
    raise KeyError(fam)


# ------------------------------------------------------------------------------------------------ persistent objects
class Objs:
    """the key sets, key caches and signer set of one engine, made at their first use and alive until close()"""

    def __init__(self, eng, maker):
        self.eng, self.maker, self.made = eng, maker, {}

    def get(self, name):
        if name not in self.made:
            eng = self.eng
            if name in ("ladder", "comb"):
                obj = eng.keyset_create(keyset_keys(self.maker)[1], kind=name)
            elif name == "cache":
                obj = eng.keycache_create(4096)
            elif name == "wire":
                obj = eng.keycache_create(4096, wire=True)
            else:
                obj = eng.signer_set_create(signer_keys())
            self.made[name] = obj
        return self.made[name]

    def close(self):
        for obj in self.made.values():
            obj.close()
        self.made = {}


# ------------------------------------------------------------------------------------------------ the calls
def _dev(*arrays):
    import torch
    out = [None if a is None else torch.from_numpy(np.array(a)).to("cuda:0") for a in arrays]      # (the inputs are read-only)
    torch.cuda.synchronize()
    return out


def _dev_out(n):
    import torch
    st = torch.full((max(n, 1),), 255, dtype=torch.uint8, device="cuda:0")
    nf = torch.full((1,), -1, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    return st, nf


def _p(t):
    return t.data_ptr() if t is not None else 0


def _status_result(eng, st, nf, n, **more):
    eng.sync()
    return dict(status=st.cpu().numpy()[:n].copy(), nfail=int(nf.item()), **more)


def run(step, eng, objs, maker):
    """the call of `step` on `eng` -> a dict of its results (numpy arrays and ints)"""
    fam, var, n, _ = step
    inp = inputs(step, maker)
    v = [t for t in var.split(".") if t != "dirty"]
    sigs, pks, msgs, inf = (inp.get(k) for k in ("sigs", "pks", "msgs", "inf"))
    ml = msgs.shape[1] if msgs is not None and msgs.ndim == 2 else 0
    if fam == "verify_many":
        mode = None if v[0] == "auto" else v[0]
        if v[2] == "host":
            st, nf = eng.verify_many(sigs, pks, msgs, pk_inf=inf, mode=mode, **FL[v[1]])
            return dict(status=st, nfail=nf)
        ds, dp, dmsg, di = _dev(sigs, pks, msgs, inf)
        st, nf = _dev_out(n)
        eng.verify_many_device(_p(ds), _p(dp), _p(dmsg), n, ml, _p(st), _p(nf), d_pk_inf=_p(di), mode=mode, **FL[v[1]])
        return _status_result(eng, st, nf, n)
    if fam in ("verify_batch_msm", "msm_partial"):
        co, cb = inp["coeffs"], 16 if v[0] == "c16" else 32
        if v[1] == "host":
            if fam == "msm_partial":
                rec = eng.verify_batch_msm_partial(sigs, pks, msgs, coeffs=co, pk_inf=inf)
                return dict(record=rec, verdict=eng.msm_combine(rec))
            return dict(verdict=eng.verify_batch_msm(sigs, pks, msgs, coeffs=co, pk_inf=inf))
        import torch
        ds, dp, dmsg, di = _dev(sigs, pks, msgs, inf)
        dc = _dev(np.ascontiguousarray(co[:, :cb]))[0] if co is not None else None
        if fam == "msm_partial":
            out = torch.zeros(24, dtype=torch.int64, device="cuda:0")
            torch.cuda.synchronize()
            eng.verify_batch_msm_partial_device(_p(ds), _p(dp), _p(dmsg), n, ml, _p(dc), cb, _p(out), d_pk_inf=_p(di))
            eng.sync()
            rec = out.cpu().numpy().view(np.uint64).copy()
            return dict(record=rec, verdict=eng.msm_combine(rec))
        out = torch.full((1,), 255, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        eng.verify_batch_msm_device(_p(ds), _p(dp), _p(dmsg), n, ml, _p(dc), cb, _p(out), d_pk_inf=_p(di))
        eng.sync()
        return dict(verdict=int(out.item()))
    if fam == "verify_batch_screened":
        co = inp["coeffs"]
        if v[1] == "host":
            st, nf = eng.verify_batch_screened(sigs, pks, msgs, coeffs=co, pk_inf=inf)
            return dict(status=st, nfail=nf)
        ds, dp, dmsg, di, dc = _dev(sigs, pks, msgs, inf, co)
        st, nf = _dev_out(n)
        eng.verify_batch_screened_device(_p(ds), _p(dp), _p(dmsg), n, ml, _p(dc), 32, _p(st), _p(nf), d_pk_inf=_p(di))
        return _status_result(eng, st, nf, n)
    if fam == "verify_many_dedup":
        if v[1] == "host":
            st, nf, stats = eng.verify_many_dedup(sigs, pks, msgs, pk_inf=inf, **FL[v[0]])
            return dict(status=st, nfail=nf, distinct=int(stats[0]), bound_hits=int(stats[3]))
        ds, dp, dmsg, di = _dev(sigs, pks, msgs, inf)
        st, nf = _dev_out(n)
        stats = eng.verify_many_dedup_device(_p(ds), _p(dp), _p(dmsg), n, ml, _p(st), _p(nf), d_pk_inf=_p(di), **FL[v[0]])
        return _status_result(eng, st, nf, n, distinct=int(stats[0]), bound_hits=int(stats[3]))
    if fam in ("verify_many_screened", "verify_many_cached"):
        co = inp["coeffs"]
        cache = (objs.get("cache"),) if fam == "verify_many_cached" else ()
        res = {}
        for rep in (("", "_warm") if cache else ("",)):      # a cache: the same call again, served from its rows
            if v[2] == "host":
                fn = eng.verify_many_cached if cache else eng.verify_many_screened
                st, nf, stats = fn(*cache, sigs, pks, msgs, coeffs=co, pk_inf=inf, **FL[v[0]])
            else:
                ds, dp, dmsg, di, dc = _dev(sigs, pks, msgs, inf, co)
                dst, dnf = _dev_out(n)
                fn = eng.verify_many_cached_device if cache else eng.verify_many_screened_device
                stats = fn(*cache, _p(ds), _p(dp), _p(dmsg), n, ml, _p(dc), 32, _p(dst), _p(dnf), d_pk_inf=_p(di), **FL[v[0]])
                r = _status_result(eng, dst, dnf, n)
                st, nf = r["status"], r["nfail"]
            res["status" + rep], res["nfail" + rep] = st, nf
            if co is not None:          # caller coefficients: the screen's own counts are a function of the inputs
                res["stats" + rep] = np.array(stats[:7], np.uint64)
        return res
    if fam == "verify_keyed_many":
        kd = inp["keyed"]
        if v[1] == "host":
            st, nf = eng.verify_keyed_many(kd, msgs, check_torsion=FL[v[0]]["check_torsion"])
            return dict(status=st, nfail=nf)
        dk, dmsg = _dev(kd, msgs)
        st, nf = _dev_out(n)
        eng.verify_keyed_many_device(_p(dk), _p(dmsg), n, ml, _p(st), _p(nf), check_torsion=FL[v[0]]["check_torsion"])
        return _status_result(eng, st, nf, n)
    if fam == "verify_keyed_many_cached":
        kd, co, cache = inp["keyed"], inp["coeffs"], objs.get("wire")
        res = {}
        for rep in ("", "_warm"):
            if v[2] == "host":
                st, nf, stats = eng.verify_keyed_many_cached(cache, kd, msgs, coeffs=co, **FL[v[0]])
            else:
                dk, dmsg, dc = _dev(kd, msgs, co)
                dst, dnf = _dev_out(n)
                stats = eng.verify_keyed_many_cached_device(cache, _p(dk), _p(dmsg), n, ml, _p(dc), 32, _p(dst), _p(dnf),
                                                            **FL[v[0]])
                r = _status_result(eng, dst, dnf, n)
                st, nf = r["status"], r["nfail"]
            res["status" + rep], res["nfail" + rep] = st, nf
            if co is not None:
                res["stats" + rep] = np.array(stats[:7], np.uint64)
        return res
    if fam == "verify_many_indexed":
        ks = objs.get(v[0])
        if v[2] == "host":
            st, nf = eng.verify_many_indexed(ks, inp["kidx"], sigs, msgs, **FL[v[1]])
            return dict(status=st, nfail=nf)
        di, ds, dmsg = _dev(inp["kidx"], sigs, msgs)
        st, nf = _dev_out(n)
        eng.verify_many_indexed_device(ks, _p(di), _p(ds), _p(dmsg), n, ml, _p(st), _p(nf),
                                       check_torsion=FL[v[1]]["check_torsion"])
        return _status_result(eng, st, nf, n)
    kw = dict(constant_time="ct" in v, keyed="keyed" in v)
    if fam == "keygen_sign_many":
        pk, sg = eng.keygen_sign_many(inp["sks"], inp["nonces"], msgs, **kw)
        return dict(pks=pk, sigs=sg)
    if fam == "pubkey_many":
        return dict(pks=eng.pubkey_many(inp["sks"]))
    if fam == "sign_many_indexed":
        return dict(sigs=eng.sign_many_indexed(objs.get("signers"), inp["kidx"], inp["nonces"], msgs, **kw))
    if fam == "rng_signers":
        eng.debug_pin_rng(RNG_PIN)
        try:
            if v[0] == "keygen":
                pk, sg = eng.keygen_sign_many_rng(inp["sks"], msgs, **kw)
                return dict(pks=pk, sigs=sg)
            return dict(sigs=eng.sign_many_indexed_rng(objs.get("signers"), inp["kidx"], msgs, **kw))
        finally:
            eng.debug_pin_rng(None)
    if fam == "hash_message_many":
        if v[0] == "offsets":
            return dict(digests=eng.hash_message_many(sigs, pks, inp["flat"], offsets=inp["off"]))
        if v[-1] == "dev":
            import torch
            ds, dp, dmsg = _dev(sigs, pks, msgs if ml else np.zeros(1, np.uint8))
            out = torch.zeros((n, 32), dtype=torch.uint8, device="cuda:0")
            torch.cuda.synchronize()
            eng.hash_message_many_device(_p(ds), _p(dp), _p(dmsg), n, ml, _p(out))
            eng.sync()
            return dict(digests=out.cpu().numpy().copy())
        return dict(digests=eng.hash_message_many(sigs, pks, msgs))
    if fam == "rescue_hash_many":
        return dict(digests=eng.rescue_hash_many(inp["felts"]))
    if fam == "compress_many":
        out, st = eng.compress_many(pks, inf)
        return dict(comp=out, status=st)
    if fam == "decompress_many":
        pk, pinf, st = eng.decompress_many(inp["comp"])
        return dict(pks=pk, inf=pinf, status=st)
    if fam == "xprv_master_many":
        out, st = eng.xprv_master_many(inp["seeds"])
        return dict(children=out, status=st)
    if fam == "xprv_derive_many":
        out, st = eng.xprv_derive_many(inp["xprv"], inp["idx"], parent_idx=inp["pidx"], derive_public=v[0] == "pub")
        return dict(children=out, status=st)
    if fam == "xpub_derive_many":
        out, pk, pinf, st = eng.xpub_derive_many(inp["xpub"], inp["idx"], parent_idx=inp["pidx"])
        return dict(children=out, pks=pk, inf=pinf, status=st)
    if fam == "selfcheck":
        if v[0] == "ctx":
            r = eng.selfcheck()
            return {k: r[k] for k in ("ok", "rows", "bad", "ctab_bad", "bits")}
        r = (objs.get("ladder") if v[0] == "keyset" else objs.get("cache")).selfcheck(deep=True)
        return {k: r[k] for k in ("ok", "keys_bad")}
    raise KeyError(fam)


def same(a, b, orc):
    """None when the two result dicts are exactly equal, else what differs"""
    if set(a) != set(b):
        return "results %s / %s" % (sorted(a), sorted(b))
    for k in a:
        x, y = a[k], b[k]
        if k == "record":
            if (mr.record_point(orc, x), mr.record_lin(x), int(x[22]), int(x[23])) != \
                    (mr.record_point(orc, y), mr.record_lin(y), int(y[22]), int(y[23])):
                return "record"
        elif isinstance(x, np.ndarray):
            if x.shape != y.shape or not np.array_equal(x, y):
                d = np.nonzero((x != y).reshape(x.shape[0], -1).any(axis=1))[0] if x.shape == y.shape and x.ndim else []
                return "%s: %d rows differ, first %s" % (k, len(d), list(d[:8]))
        elif x != y:
            return "%s: %r != %r" % (k, x, y)
    return None


# ------------------------------------------------------------------------------------------------ expectations
def _flags_of(step):
    fam, var = step.family, step.variant.split(".")
    if fam == "verify_many":
        return FL[var[1]]
    if fam == "verify_batch_screened":
        return FL["F"]
    if fam == "verify_many_indexed":
        return FL[var[1]] if var[2] == "host" else dict(FL[var[1]], sig_flag_byte=False)
    if fam in ("verify_keyed_many",):
        return dict(FL[var[0]], sig_flag_byte=False)
    return FL[var[0]]


STATUS_FAMILIES = ("verify_many", "verify_batch_screened", "verify_many_dedup", "verify_many_screened", "verify_many_cached",
                   "verify_keyed_many", "verify_keyed_many_cached", "verify_many_indexed")


def expected(step, inp):
    """what the step must return BY CONSTRUCTION, every lane of it: {result name: value}"""
    fam, var, n, _ = step
    v = var.split(".")
    if fam in STATUS_FAMILIES:
        fl = _flags_of(step)
        st = np.zeros(n, np.uint8)
        for i, kind in inp["kinds"].items():
            st[i] = kind_status(kind, fl)
        exp = {"status": st, "nfail": int((st != 0).sum())}
        if fam == "verify_many_dedup":      # 128 probes in a table loaded to a quarter: no lane reaches the bound
            exp["bound_hits"] = 0
        if fam in ("verify_many_cached", "verify_keyed_many_cached"):
            exp.update(status_warm=st, nfail_warm=exp["nfail"])
        return exp
    if fam in ("verify_batch_msm", "msm_partial"):
        kinds = set(inp["kinds"].values())
        return {"verdict": 3 if "e_ge_q" in kinds else 2 if kinds else 0}
    if fam == "compress_many":
        return {"status": np.zeros(n, np.uint8)}
    if fam == "xprv_master_many":
        return {"status": np.zeros(n, np.uint8)}
    if fam == "xpub_derive_many":
        return {"status": (inp["idx"] >= H).astype(np.uint8)}
    if fam == "selfcheck":
        return {"ok": True, "bad": 0, "ctab_bad": 0} if v[0] == "ctx" else {"ok": True, "keys_bad": 0}
    return {}


def sample_lanes(inp, clean=40):
    n = inp["n"]
    touched = list(inp.get("kinds", {})) + [int(i) for i in inp.get("bad", [])]
    return np.unique(np.array(touched + list(range(0, n, max(1, n // clean))) + [n - 1], np.int64))


def check_oracle(step, inp, res, orc):
    """the touched lanes and a strided sample of clean ones against the CPU oracle (about 50 lanes a step)"""
    fam, var, n, _ = step
    v = var.split(".")
    s = sample_lanes(inp) if n else np.zeros(0, np.int64)
    if fam in STATUS_FAMILIES:
        fl = _flags_of(step)
        spks, sinf, ssigs, undecodable = inp["pks"][s], inp["inf"][s], inp["sigs"][s], np.zeros(s.size, bool)
        if "keyed" in inp:          # the oracle decompresses the record's key itself
            spks, sinf, ssigs = np.zeros((s.size, 96), np.uint8), np.zeros(s.size, np.uint8), inp["keyed"][s, 49:]
            for j, i in enumerate(s):
                dec = orc.decompress(inp["keyed"][i, :49].tobytes())
                undecodable[j] = dec is None
                if dec is not None:
                    spks[j], sinf[j] = np.frombuffer(dec[0], np.uint8), dec[1]
        want = orc.verify_many(ssigs, spks, inp["msgs"][s], pk_inf=sinf, **fl)
        want[undecodable] = 3
        for key in ("status", "status_warm"):
            if key in res:
                assert (res[key][s] == want).all(), (step, key, s[res[key][s] != want][:8])
    elif fam == "verify_batch_msm" and n <= 300 and inp["coeffs"] is not None:
        assert res["verdict"] == orc.verify_batch_msm(inp["sigs"], inp["pks"], inp["msgs"], inp["coeffs"], pk_inf=inp["inf"])
    elif fam == "msm_partial" and n <= 100:
        left, lin, bad = mr.cpu_partial(orc, inp["sigs"], inp["pks"], inp["msgs"], inp["coeffs"], pk_inf=inp["inf"])
        rec = res["record"]
        assert mr.record_is_wellformed(orc, rec) and not bad and int(rec[22]) == 0
        assert mr.record_point(orc, rec) == left and mr.record_lin(rec) == lin
        assert res["verdict"] == mr.cpu_combine(orc, rec)
    elif fam in ("keygen_sign_many", "pubkey_many", "sign_many_indexed", "rng_signers"):
        s = s[:24]
        nonces = rng_model.draw(RNG_PIN, [int(i) for i in s]) if fam == "rng_signers" else inp["nonces"][s]
        pk, sg = orc.keygen_sign_many(inp["sks"][s], nonces, inp["msgs"][s])
        if "pks" in res:
            assert (res["pks"][s] == pk).all(), step
        if "sigs" in res:
            assert (res["sigs"][s][:, -81:] == sg).all(), step
            if "keyed" in v:
                for j, i in enumerate(s):
                    assert res["sigs"][i, :49].tobytes() == orc.compress(pk[j].tobytes()), step
    elif fam == "hash_message_many":
        for i in s:
            msg = inp["flat"][int(inp["off"][i]):int(inp["off"][i + 1])] if v[0] == "offsets" else inp["msgs"][i]
            assert res["digests"][i].tobytes() == orc.hash_message(inp["sigs"][i, :48].tobytes(), inp["pks"][i].tobytes(),
                                                                   msg.tobytes()), (step, i)
    elif fam == "rescue_hash_many":
        f = inp["felts"][s]
        want = orc.hash_field_many(f) if f.shape[1] else np.stack([orc.hash_field(np.zeros(0, np.uint64))] * s.size)
        assert (res["digests"][s] == want).all(), step
    elif fam == "compress_many":
        for i in s:
            assert res["comp"][i].tobytes() == orc.compress(inp["pks"][i].tobytes(), bool(inp["inf"][i])), (step, i)
    elif fam == "decompress_many":
        for i in s:
            dec = orc.decompress(inp["comp"][i].tobytes())
            if dec is None:
                assert res["status"][i] == 1 and i in inp["bad"], (step, i)
            else:
                assert res["status"][i] == 0 and bool(res["inf"][i]) == dec[1], (step, i)
                assert dec[1] or res["pks"][i].tobytes() == dec[0], (step, i)
        assert set(np.nonzero(res["status"])[0]) == set(int(i) for i in inp["bad"]), step
    elif fam == "xprv_master_many":
        for i in s:
            assert res["children"][i].tobytes() == dm.xprv_bytes(*dm.master(inp["seeds"][i].tobytes())), (step, i)
    elif fam in ("xprv_derive_many", "xpub_derive_many"):
        for i in s[:16]:
            k, ix = int(inp["pidx"][i]), int(inp["idx"][i])
            sk, cc = inp["par"][k]
            pk49 = inp["pk49"][k].tobytes()
            if fam == "xpub_derive_many" and ix >= H:
                assert res["status"][i] == 1 and not res["children"][i].any(), (step, i)
                continue
            child, ccc = dm.derive_private(sk, cc, ix, pk49)      # (the child of the public derivation is [child]G too)
            assert res["status"][i] == 0, (step, i)
            if fam == "xprv_derive_many" and v[0] == "priv":
                assert res["children"][i].tobytes() == dm.xprv_bytes(child, ccc), (step, i)
            else:
                cpk = orc.keygen(child.to_bytes(32, "little"))[0]
                assert res["children"][i].tobytes() == orc.compress(cpk) + ccc, (step, i)
                if "pks" in res:
                    assert res["pks"][i].tobytes() == cpk and not res["inf"][i], (step, i)


def check_expected(step, inp, res):
    for k, want in expected(step, inp).items():
        got = res[k]
        if isinstance(want, np.ndarray):
            assert np.array_equal(got, want), (step, k, np.nonzero(got != want)[0][:8])
        else:
            assert got == want, (step, k, got, want)


# ------------------------------------------------------------------------------------------------ the script
def _steps(family, rows, base):
    return [Step(family, var, n, base + 17 * j) for j, (var, n) in enumerate(rows)]


# sizes: 1, 63, 257; 3072 | 3073 (the small-batch bound of the MSM forms); 4095 | 4096 (window width 8 | 16 and the tile
# of the bucket method); 7680 | 7681 and 10496 | 10497 (cooperative | lane kernels, without | with the subgroup check);
# 20 000 (several screened segments, the last one ragged)
FAMILIES = {
    "verify_many": _steps("verify_many", [
        ("lane.T.host", 1), ("coop.T.host", 1), ("lane.N.host", 63), ("coop.F.dev", 63), ("lane.TF.dev", 257),
        ("coop.N.host", 257), ("coop.TF.host", 1000), ("lane.F.host", 4097), ("auto.N.host", 7680), ("auto.N.dev", 7681),
        ("auto.T.host", 10496), ("auto.T.dev", 10497)], 1000),
    "verify_batch_msm": _steps("verify_batch_msm", [
        ("c32.host.honest", 1), ("c32.dev.bad", 63), ("lib.host.honest", 257), ("c32.host.honest", 3072),
        ("c32.host.bad", 3073), ("c16.dev.bad", 4095), ("c16.dev.honest", 4096), ("lib.host.malformed", 4096),
        ("lib.dev.bad", 20000)], 2000),
    "msm_partial": _steps("msm_partial", [
        ("c32.host", 63), ("c16.dev", 3073), ("c32.host", 4095), ("c32.dev", 4096), ("c32.host", 20000)], 3000),
    "verify_batch_screened": _steps("verify_batch_screened", [
        ("c32.host", 3072), ("c32.dev", 3073), ("lib.host", 4095), ("c32.host", 4096), ("lib.dev", 20000),
        ("c32.host", 20000)], 4000),
    "verify_many_dedup": _steps("verify_many_dedup", [
        ("N.dev", 1), ("TF.host", 63), ("T.host", 257), ("T.dev", 7681), ("N.host", 10497)], 5000),
    "verify_many_screened": _steps("verify_many_screened", [
        ("T.c32.host", 3072), ("T.lib.dev", 3073), ("N.c32.host", 4095), ("TF.c32.dev", 4096), ("N.lib.host", 10497),
        ("T.c32.host", 20000)], 6000),
    "verify_many_cached": _steps("verify_many_cached", [
        ("N.c32.host", 257), ("T.c32.host", 3073), ("TF.lib.dev", 4096), ("T.c32.dev", 20000)], 7000),
    "verify_keyed_many": _steps("verify_keyed_many", [
        ("T.host", 1), ("N.dev", 257), ("T.dev", 7681), ("T.host", 10497)], 8000),
    "verify_keyed_many_cached": _steps("verify_keyed_many_cached", [
        ("T.c32.host", 3073), ("TF.lib.dev", 4096), ("T.c32.dev", 20000)], 9000),
    "verify_many_indexed": _steps("verify_many_indexed", [
        ("ladder.T.host", 63), ("ladder.N.dev", 257), ("comb.T.host", 257), ("comb.TF.host", 4097),
        ("ladder.T.host", 10497)], 10000),
    "keygen_sign_many": _steps("keygen_sign_many", [("tp", 1), ("ct", 63), ("tp.keyed", 257), ("ct.keyed", 1000)], 11000),
    "pubkey_many": _steps("pubkey_many", [("ct", 1), ("ct", 257)], 12000),
    "sign_many_indexed": _steps("sign_many_indexed", [("tp", 63), ("ct.keyed", 257)], 13000),
    "rng_signers": _steps("rng_signers", [("keygen.tp", 63), ("indexed.ct", 257), ("keygen.ct.keyed", 257)], 14000),
    "hash_message_many": _steps("hash_message_many", [
        ("len8", 1), ("len0", 63), ("len7", 257), ("offsets", 257), ("len160", 257), ("len80.dev", 1000)], 15000),
    "rescue_hash_many": _steps("rescue_hash_many", [("w0", 63), ("w8", 257), ("w13", 1000)], 16000),
    "compress_many": _steps("compress_many", [("aff", 1), ("aff", 257)], 17000),
    "decompress_many": _steps("decompress_many", [("wire", 1), ("wire", 257)], 18000),
    "xprv_master_many": _steps("xprv_master_many", [("seed", 257)], 19000),
    "xprv_derive_many": _steps("xprv_derive_many", [("pub", 63), ("priv", 257)], 20000),
    "xpub_derive_many": _steps("xpub_derive_many", [("normal", 257)], 21000),
    "selfcheck": _steps("selfcheck", [("ctx", 0), ("keyset", 0), ("cache", 0)], 22000),
}
SCRIPT = [s for steps in FAMILIES.values() for s in steps]

# the families whose calls run over more than one slice on an engine with 5000-lane slices, at n = 12 345
SLICED = [
    Step("verify_many", "lane.T.host", SLICED_N, 30000), Step("verify_many", "lane.F.dev", SLICED_N, 30001),
    Step("verify_batch_msm", "c32.host.bad", SLICED_N, 30002), Step("msm_partial", "c32.host", SLICED_N, 30003),
    Step("verify_batch_screened", "c32.host", SLICED_N, 30004), Step("verify_many_dedup", "T.host", SLICED_N, 30005),
    Step("verify_many_screened", "T.c32.host", SLICED_N, 30006), Step("verify_many_cached", "T.c32.host", SLICED_N, 30007),
    Step("verify_keyed_many", "T.host", SLICED_N, 30008), Step("verify_keyed_many_cached", "T.c32.host", SLICED_N, 30009),
    Step("verify_many_indexed", "ladder.T.host", SLICED_N, 30010), Step("keygen_sign_many", "ct", SLICED_N, 30011),
    Step("sign_many_indexed", "tp", SLICED_N, 30012), Step("hash_message_many", "len80", SLICED_N, 30013),
]

# the families that share ws_h, ws_tab, the msm_*, scr_*, dd_*, kc_*, ky_* and staging buffers, and the "dirty" step of
# each: the largest n, every lane bad or malformed, all-0xFF coefficients, pk_inf on a tenth of the lanes, 160-byte messages
DIRTY = {
    "verify_many": Step("verify_many", "lane.T.host.dirty", DIRTY_N, 40000),
    "verify_batch_msm": Step("verify_batch_msm", "c32.host.dirty", DIRTY_N, 40001),
    "msm_partial": Step("msm_partial", "c32.host.dirty", DIRTY_N, 40002),
    "verify_batch_screened": Step("verify_batch_screened", "c32.host.dirty", DIRTY_N, 40003),
    "verify_many_dedup": Step("verify_many_dedup", "T.host.dirty", DIRTY_N, 40004),
    "verify_many_screened": Step("verify_many_screened", "T.c32.host.dirty", DIRTY_N, 40005),
    "verify_many_cached": Step("verify_many_cached", "T.c32.host.dirty", DIRTY_N, 40006),
    "verify_keyed_many": Step("verify_keyed_many", "T.host.dirty", DIRTY_N, 40007),
    "verify_keyed_many_cached": Step("verify_keyed_many_cached", "T.c32.host.dirty", DIRTY_N, 40008),
}
SCREENED = ("verify_batch_screened", "verify_many_screened", "verify_many_cached", "verify_keyed_many_cached")


def step_id(step):
    return "%s-%s-%d" % (step.family, step.variant, step.n)


def digest(res):
    """a short fingerprint of a result dict (messages)"""
    h = hashlib.sha256()
    for k in sorted(res):
        h.update(k.encode() + (res[k].tobytes() if isinstance(res[k], np.ndarray) else repr(res[k]).encode()))
    return h.hexdigest()[:12]
