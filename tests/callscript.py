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

The sizes are the smallest that straddle every dispatch boundary of the library, not the workload's own.

The aggregate side (half-aggregation, DESIGN.md sections 20 .. 36).  One-shot steps are calls; a streaming step is a
SCENARIO on an object made and closed inside the step (aggregator_scenario, _run_aggverifier), so that its result depends
on the step's inputs alone; the key caches stay the shared ones of Objs ("in every state of the cache").  Every aggregate,
key column, leaf column and coefficient-dependent output is compared with tests/aggregate_model.py over the C oracle at
EVERY size (class Transcript: the leaves are hashed once per step), the streaming ones with the aggregate of exactly the
kept lanes in their order; known_sum with aggverifier_mixed_model, the admission bytes with aggverifier_admission_model's
piecewise move, the look-ups with aggregator_index_model's dictionary.  Statuses and verdicts are known by construction
for every lane and every aggregate.  What the models do NOT cover: am.verify, the point-exact verification, runs at the
smallest sizes only (verify_aggregate at 1 and 2 lanes, the aggregates of at most three lanes of the list "edges"); at
every other size an accepting or rejecting verdict of the MSM rests on construction alone -- honest lanes and the honest
scalar accept, one flipped bit rejects.  The honest scalars the validators are handed come from the maker's own
Engine.aggregate and are themselves compared with the model.  Statistics of the key caches (hits, inserts, clears) depend on
what ran before and are not results; `bad_key_aggregates` and `cached_lanes` are functions of the inputs and are.

Exported entry point (include/schnorr_sig_amd.h from ssa_aggregate_many on) -> steps; f(_device) stands for both forms:
    ssa_aggregate_many(_device)                          aggregate *.host.* / *.dev.*
    ssa_verify_aggregate(_device)                        verify_aggregate *.host / *.dev
    ssa_aggregate_many_sliced(_device)                   aggregate_sliced; SLICED: three slices
    ssa_verify_aggregate_sliced(_device)                 verify_aggregate_sliced; SLICED
    ssa_aggregate_shard_tops_device, ssa_aggregate_root_device, ssa_aggregate_shard_fold_device,
    ssa_aggregate_combine_device, ssa_verify_aggregate_shard_device, ssa_verify_aggregate_combine_device
                                                         aggregate_shards (one shard that is the whole aggregate, through
                                                         schnorr_sig_amd.sharding as a rank of a sharded aggregate calls them)
    ssa_verify_aggregates_many(_device)                  verify_aggregates edges | many | paths . host | dev
    ssa_aggregates_many(_device)                         aggregates *.host / *.dev
    ssa_verify_aggregates_many_cached(_device)           verify_aggregates_cached *.affine.host / *.affine.dev
    ssa_verify_aggregates_many_cached_wire(_device)      verify_aggregates_cached *.wire.host / *.wire.dev; SLICED
    ssa_aggregate_valid_many(_device)                    aggregate_valid host / dev; SLICED (lane slices)
    ssa_aggregate_valid_many_cached(_device)             aggregate_valid_cached host / dev
    ssa_aggregate_valid_keyed_many_cached(_device)       aggregate_valid_keyed_cached host / dev; SLICED (lane slices)
    ssa_aggregator_create, _destroy, _info, _reset       every aggregator step
    ssa_aggregator_push(_device)                         aggregator screened | noscreen | index.admission [.dev]
    ssa_aggregator_push_cached(_device)                  aggregator cached | index.admission [.dev]
    ssa_aggregator_push_keyed_cached(_device)            aggregator keyed.holdkeys [.dev]; SLICED
    ssa_aggregator_finish(_device), _leaves(_device), _leaves_select(_device), _finish_select(_device),
    _drop_front, _remove(_device), _remove_indices(_device)      every aggregator step [.dev: the device forms]
    ssa_aggregator_keys(_device)                         aggregator keyed.holdkeys [.dev]
    ssa_aggregator_admission(_device), _index_sync, _lookup(_device), _index_info     aggregator index.admission [.dev]
    ssa_aggverifier_create, _destroy, _info, _reset      every aggverifier step
    ssa_aggverifier_push(_device), _finish(_device)      aggverifier plain [.dev] (finish: every aggverifier step)
    ssa_aggverifier_push_cached(_device)                 aggverifier cached [.dev]
    ssa_aggverifier_push_cached_wire(_device)            aggverifier wire [.dev]
    ssa_aggverifier_push_mixed(_device), _push_known(_device)    aggverifier mixed [.dev] (the pool: ssa_aggregator_lookup(_device);
                                                         S is read through the debug hook ssa_debug_aggverifier_known_sum)
    ssa_aggverifier_push_mixed_cached(_device)           aggverifier mixed.cached [.dev]
    ssa_aggverifier_push_mixed_cached_wire(_device)      aggverifier mixed.wire.require2 [.dev]; SLICED
Left out on purpose: ssa_multi_aggregate_many and ssa_multi_verify_aggregate (several devices: not one context's
workspaces; tests/test_gpu_aggregate_sharded.py); ssa_abi_version (no context)."""
import hashlib
from collections import namedtuple

import numpy as np

import aggregate_model as am
import aggregator_index_model as index_model
import aggverifier_admission_model as adm_model
import aggverifier_mixed_model as mixed_model
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
    if fam in AGG_FAMILIES:
        return _build_agg_inputs(step, maker, v, dirty, ml)
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
    if fam in AGG_FAMILIES:
        return _run_agg(step, eng, objs, inp, v, ml)
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
    if fam in AGG_FAMILIES:
        return _expected_agg(step, inp, v)
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
    if fam in AGG_FAMILIES:
        return _check_agg_models(step, inp, res, orc, v)
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


# ------------------------------------------------------------------------------------------------ the aggregate families
AGG_FAMILIES = ("aggregate", "aggregate_sliced", "aggregates", "aggregate_valid", "aggregate_valid_cached",
                "aggregate_valid_keyed_cached", "verify_aggregate", "verify_aggregate_sliced", "verify_aggregates",
                "verify_aggregates_cached", "aggregate_shards", "aggregator", "aggverifier")
UNKNOWN = 0xFFFFFFFF                    # SSA_AGGV_UNKNOWN
MALFORMED_KINDS = ("e_ge_q", "noncanon_pk", "noncanon_rec")      # what the producer refuses without a screen
ADM_CLASS = {"noscreen": 0, "screened": 1, "cached": 2, "keyed": 2}
PUSH_RULE = {"noscreen": "nocheck", "screened": "F", "cached": "TF", "keyed": "TF"}
# lists of counts of the many-calls: empty aggregates, neighbours that share a 256-lane workgroup (100 | 156, and the
# small ones of "many"), a group on each path (<= 3072: the small path, above: the bucket path), 300 aggregates
# (AG_GROUP_MAX = 256: more than one group), aggregates that straddle the 5000-lane slice boundaries, and the list of the dirty steps
COUNTS = {
    "edges": [0, 1, 63, 0, 100, 156, 257, 3, 513, 0],
    "paths": [3072, 0, 3073, 5, 4096, 3500],
    "many": [3000] + [(5 * j + 1) % 9 for j in range(299)],      # its first 256 take the bucket path, the other 44 the small
    "sliced": [4990, 20, 0, 4985, 15, 2335],
    "allbad": [3073, 0, 4096, 5000, 257, 7574],
}
N_OF = {name: sum(c) for name, c in COUNTS.items()}
assert N_OF["sliced"] == SLICED_N and N_OF["allbad"] == DIRTY_N
FINISH_PREFIXES = (1, 512, 513, 8192, 8193)     # both sides of AG_TREE_SPAN / the block, and of AGV_KST_SPAN


def lane_status(inp, rule):
    """the status of every lane BY CONSTRUCTION under the flags FL[rule], or ("nocheck") under the producer's own checks"""
    st = np.zeros(inp["n"], np.uint8)
    for i, kind in inp["kinds"].items():
        st[i] = (3 if kind in MALFORMED_KINDS else 0) if rule == "nocheck" else kind_status(kind, FL[rule])
    return st


def lane_starts(counts):
    """(first lane of every aggregate, and one more; first byte of every aggregate in the wire form)"""
    start = np.concatenate([[0], np.cumsum(np.asarray(counts, np.int64))])
    return start, 49 * start[:-1] + 32 * np.arange(len(counts))


def cuts(n, piece=None):
    """ragged pushes: 1, 511, 1, 700 lanes, then the rest (piece: in pieces of at most that many lanes)"""
    out, lo = [], 0
    for c in (1, 511, 1, 700):
        if lo + c >= n:
            break
        out.append((lo, lo + c))
        lo += c
    piece = piece or n
    return out + [(a, min(a + piece, n)) for a in range(lo, n, piece)]


def verifier_cuts(n):
    """the pushes of the aggverifier scenario: on the engines with a 5000-lane MSM slice a push above it is refused"""
    return cuts(n, 4000 if n == SLICED_N else None)


def _spoil_aggregates(b, counts, wire, cached):
    """a known set of bad aggregates -> the verdict of every aggregate BY CONSTRUCTION: every second empty one gets a
    non-zero scalar (2); of the others every fourth a flipped message bit in its middle lane (2), two in sixteen a scalar
    >= q or an R that does not decode (3), and (cached) one in eight the key outside the subgroup on its last lane (1)"""
    start, off = lane_starts(counts)
    verdict = np.zeros(len(counts), np.uint32)
    empties = [j for j, c in enumerate(counts) if c == 0]
    for j in empties[1::2]:
        wire[off[j]] = 1
        verdict[j] = 2
    for t, j in enumerate(j for j, c in enumerate(counts) if c):
        c = int(counts[j])
        if t % 4 == 1:
            b["msgs"][start[j] + c // 2, 3] ^= 0x20
            verdict[j] = 2
        elif t % 16 == 2:
            wire[off[j] + 49 * c: off[j] + 49 * c + 32] = 0xFF
            verdict[j] = 3
        elif t % 16 == 6:
            wire[off[j] + 49 * (c - 1): off[j] + 49 * (c - 1) + 8] = 0xFF
            verdict[j] = 3
        elif cached and t % 8 == 3:
            b["pks"][start[j] + c - 1] = fixture_key()
            verdict[j] = 1
    return verdict


def _build_agg_inputs(step, maker, v, dirty, ml):
    fam, var, n, seed = step
    rng = np.random.default_rng(seed + 1)
    if fam in ("aggregate", "aggregate_sliced"):                    # check|nocheck . host|dev . honest|bad
        return make_batch(maker, seed, n, kinds=ALL_KINDS if v[2] == "bad" else (), msg_len=ml, dirty=dirty)
    if fam == "aggregate_shards":                                   # b<block lanes> . honest|bad
        return make_batch(maker, seed, n, kinds=("e_ge_q", "noncanon_pk") if v[1] == "bad" else (), msg_len=ml)
    if fam == "aggregates":                                         # list . check|nocheck . host|dev
        b = make_batch(maker, seed, n, msg_len=ml, dirty=dirty)
        b["counts"] = np.array(COUNTS[v[0]], np.uint64)
        return b
    if fam in ("aggregate_valid", "aggregate_valid_cached"):        # host|dev
        return make_batch(maker, seed, n, msg_len=ml, dirty=dirty)
    if fam == "aggregate_valid_keyed_cached":
        b = make_batch(maker, seed, n, kinds=("e_bit", "e_ge_q", "msg_bit", "offsub"), msg_len=ml)
        b["keyed"] = keyed_records(maker, b)
        return b
    if fam in ("verify_aggregate", "verify_aggregate_sliced"):      # case . host|dev
        b = make_batch(maker, seed, n, kinds=(), msg_len=ml, dirty=dirty)
        if dirty:
            b["agg"] = np.concatenate([b["sigs"][:, :49].reshape(-1), np.full(32, 0xFF, np.uint8)])
            return b
        rc, agg, _, nf = maker.aggregate(b["sigs"], b["pks"], b["msgs"], pk_inf=b["inf"])
        assert rc == 0 and nf == 0
        b["honest_agg"], b["flip"] = agg.copy(), -1
        lane = {"first": 0, "mid": n // 2, "last": n - 1}
        if v[0] in lane:
            b["flip"] = lane[v[0]]
            b["msgs"][b["flip"], 1] ^= 0x04
        elif v[0] == "e_ge_q":
            agg[49 * n:] = 0xFF
        elif v[0] == "bad_r":
            agg[49 * (n // 2): 49 * (n // 2) + 8] = 0xFF
        b["agg"] = agg
        return b
    if fam in ("verify_aggregates", "verify_aggregates_cached"):    # list . [affine|wire .] host|dev
        counts = np.array(COUNTS[v[0]], np.uint64)
        b = make_batch(maker, seed, n, kinds=(), msg_len=ml, dirty=dirty)
        b["counts"] = counts
        if dirty:                                                   # every aggregate bad: scalars >= q, an empty one's 1
            start, off = lane_starts(counts)
            wire = np.zeros(49 * n + 32 * counts.size, np.uint8)
            for j, c in enumerate(int(c) for c in counts):
                wire[off[j]: off[j] + 49 * c] = b["sigs"][start[j]: start[j] + c, :49].reshape(-1)
                wire[off[j] + 49 * c: off[j] + 49 * c + 32] = 0xFF if c else 0
                wire[off[j] + 49 * c] = 0xFF if c else 1
            b["wire"], b["verdicts"] = wire, np.where(counts > 0, 3, 2).astype(np.uint32)
            return b
        _, wire, results, _, nf = maker.aggregates_wire((b["sigs"], b["pks"], b["msgs"]), counts=counts, pk_inf=b["inf"])
        assert not results.any() and nf == 0
        wire = wire.copy()
        b["honest_wire"], b["honest_msgs"], b["honest_pks"] = wire.copy(), b["msgs"].copy(), b["pks"].copy()
        b["verdicts"] = _spoil_aggregates(b, counts, wire, fam == "verify_aggregates_cached")
        b["wire"] = wire
        if "wire" in v[1:]:
            b["keys49"], st = maker.compress_many(b["pks"])
            assert not st.any()
        return b
    if fam == "aggregator":       # screened | noscreen | cached | keyed.holdkeys | index.admission [. dev]
        keyed = v[0] == "keyed"
        b = make_batch(maker, seed, n, kinds=("e_bit", "e_ge_q", "msg_bit", "offsub") if keyed else ALL_KINDS, msg_len=ml,
                       dirty=dirty)
        if v[0] == "index":       # one lane twice in the pool: a look-up answers the LOWEST place
            clean = [i for i in range(2, n - 2) if i not in b["kinds"]]
            a, d = clean[0], clean[-1]
            for k in ("sigs", "pks", "msgs", "inf"):
                b[k][d] = b[k][a]
            b["dup"] = (a, d)
        if keyed:
            b["keyed"] = keyed_records(maker, b)
        return b
    if fam == "aggverifier":      # plain | cached | wire | mixed | mixed.cached | mixed.wire.require2 [. dev]
        b = make_batch(maker, seed, n, kinds=(), msg_len=ml, dirty=dirty)
        if dirty:
            return b
        b["off"] = -1
        if v[0] in ("cached", "wire"):          # a key outside the subgroup: in some prefixes, not in others
            b["off"] = min(n - 1, 520)
            b["pks"][b["off"]] = fixture_key()
        lanes = np.arange(n)
        if v[0] == "mixed":       # about 5 % leave the pool before the push, 5 % more are held but not named: 90 % known
            r = rng.random(n)
            b["drop"], b["unnamed"] = (r < 0.05).astype(np.uint8), ((r >= 0.05) & (r < 0.10)).astype(np.uint8)
            known = np.nonzero(r >= 0.10)[0]
            b["again"] = known[:5]               # pushed once more, by push_known, behind the block
            lanes = np.concatenate([lanes, b["again"]])
        if "wire" in v:
            b["keys49"], st = maker.compress_many(b["pks"])
            assert not st.any()
        b["lanes"] = lanes
        b["e"] = {}
        for t in sorted({t for t in FINISH_PREFIXES + (n, lanes.size) if t <= lanes.size}):
            ix = lanes[:t]
            rc, agg, _, nf = maker.aggregate(b["sigs"][ix], b["pks"][ix], b["msgs"][ix])
            assert rc == 0 and nf == 0
            b["e"][t] = agg[49 * t:].copy()
        return b
    raise KeyError(fam)


def _tensor(shape, dtype_name, fill=255):
    """an output on the device, filled with what no call writes"""
    import torch
    return torch.full(shape if isinstance(shape, tuple) else (max(int(shape), 1),), fill, dtype=getattr(torch, dtype_name),
                      device="cuda:0")


def _host(eng, t, n=None, dtype=None):
    """a device output as a numpy array (the engine's stream has finished)"""
    a = t.cpu().numpy().copy()
    if dtype is not None:
        a = a.view(dtype)
    return a if n is None else a[:n]


def _sync():
    import torch
    torch.cuda.synchronize()


def _run_agg(step, eng, objs, inp, v, ml):
    fam, var, n, _ = step
    sigs, pks, msgs, inf = (inp.get(k) for k in ("sigs", "pks", "msgs", "inf"))
    dev = v[-1] == "dev"
    if fam in ("aggregate", "aggregate_sliced"):
        check, sliced = v[0] == "check", fam == "aggregate_sliced"
        if v[1] == "host":
            rc, agg, st, nf = (eng.aggregate_sliced if sliced else eng.aggregate)(sigs, pks, msgs, pk_inf=inf, check=check)
            return dict(rc=rc, agg=agg, status=st, nfail=nf)
        ds, dp, dmsg, di = _dev(sigs, pks, msgs, inf)
        dagg = _tensor(49 * n + 32, "uint8")
        st, nf = _dev_out(n)
        rc = (eng.aggregate_sliced_device if sliced else eng.aggregate_device)(
            _p(ds), _p(dp), _p(dmsg), n, ml, _p(dagg), _p(st), _p(nf), d_pk_inf=_p(di), check=check)
        return _status_result(eng, st, nf, n, rc=rc, agg=_host(eng, dagg, 49 * n + 32))
    if fam == "aggregate_shards":
        # the shard primitives as a process of a sharded aggregate calls them (tops, root, fold, combine; tops with the
        # challenge scalars, root, shard record, combine), here one shard that is the whole aggregate: device tensors
        from schnorr_sig_amd.sharding import aggregate_sharded, verify_aggregate_sharded
        B = int(v[0][1:])
        ds, dp, dmsg = _dev(sigs, pks, msgs)
        rc, e_agg, rs, st = aggregate_sharded(eng, ds, dp, dmsg, n, B)
        eng.sync()
        res = dict(rc=rc, agg=np.concatenate([_host(eng, rs), _host(eng, e_agg)]), status=_host(eng, st))
        if rc == 0:
            forged = np.array(msgs)
            forged[n // 2, 3] ^= 1
            res["verdict"] = verify_aggregate_sharded(eng, rs.reshape(-1, 49), dp, dmsg, e_agg, n, B)
            res["verdict_forged"] = verify_aggregate_sharded(eng, rs.reshape(-1, 49), dp, _dev(forged)[0], e_agg, n, B)
        return res
    if fam == "aggregates":
        check, counts = v[1] == "check", inp["counts"]
        k = counts.size
        if not dev:
            _, wire, results, st, nf = eng.aggregates_wire((sigs, pks, msgs), check=check, counts=counts, pk_inf=inf)
            return dict(wire=wire.copy(), results=results, status=st, nfail=nf)
        ds, dp, dmsg, di = _dev(sigs, pks, msgs, inf)
        dagg, dres = _tensor(49 * n + 32 * k, "uint8"), _tensor(k, "int32")
        st, nf = _dev_out(n)
        eng.aggregates_device(ds, counts, dp, dmsg, d_aggs=dagg, d_results=dres, d_status=st, d_nfail=nf, d_pk_inf=di,
                              check=check)
        eng.sync()
        return _status_result(eng, st, nf, n, wire=_host(eng, dagg, 49 * n + 32 * k), results=_host(eng, dres, k, np.uint32))
    if fam in ("aggregate_valid", "aggregate_valid_cached", "aggregate_valid_keyed_cached"):
        cache = {"aggregate_valid": None, "aggregate_valid_cached": "cache", "aggregate_valid_keyed_cached": "wire"}[fam]
        res = {}
        for rep in (("", "_warm") if cache else ("",)):          # a cache: the same call again, served from its rows
            if not dev:
                if fam == "aggregate_valid":
                    out = eng.aggregate_valid(sigs, pks, msgs, pk_inf=inf)
                elif fam == "aggregate_valid_cached":
                    out = eng.aggregate_valid_cached(objs.get(cache), sigs, pks, msgs, pk_inf=inf)
                    res["pks_out" + rep], res["inf_out" + rep] = out[3], out[4]
                else:
                    out = eng.aggregate_valid_keyed_cached(objs.get(cache), inp["keyed"], msgs)
                    res["keys_out" + rep] = out[3]
                res["agg" + rep], res["kept" + rep], res["status" + rep] = out[0], out[1], out[2]
                continue
            dagg, dkept, dst = _tensor(49 * n + 32, "uint8"), _tensor(n, "int32", -1), _tensor(n, "uint8")
            if fam == "aggregate_valid":
                ds, dp, dmsg, di = _dev(sigs, pks, msgs, inf)
                m = eng.aggregate_valid_device(_p(ds), _p(dp), _p(dmsg), n, ml, _p(dagg), _p(dkept), _p(dst), d_pk_inf=_p(di))
                tails = []
            elif fam == "aggregate_valid_cached":
                ds, dp, dmsg, di = _dev(sigs, pks, msgs, inf)
                dpo, dio = _tensor(96 * n, "uint8"), _tensor(n, "uint8")
                _sync()
                m, _ = eng.aggregate_valid_cached_device(objs.get(cache), _p(ds), _p(dp), _p(dmsg), n, ml, _p(dagg), _p(dkept),
                                                         _p(dst), _p(dpo), _p(dio), d_pk_inf=_p(di))
                eng.sync()
                po, io = _host(eng, dpo, 96 * n), _host(eng, dio, n)
                res["pks_out" + rep], res["inf_out" + rep] = po[:96 * m].reshape(m, 96), io[:m]
                tails = [po[96 * m:], io[m:]]
            else:
                dk, dmsg = _dev(inp["keyed"], msgs)
                dko = _tensor(49 * n, "uint8")
                _sync()
                m, _ = eng.aggregate_valid_keyed_cached_device(objs.get(cache), _p(dk), _p(dmsg), n, ml, _p(dagg), _p(dkept),
                                                               _p(dst), _p(dko))
                eng.sync()
                ko = _host(eng, dko, 49 * n)
                res["keys_out" + rep] = ko[:49 * m].reshape(m, 49)
                tails = [ko[49 * m:]]
            eng.sync()
            agg, kept = _host(eng, dagg, 49 * n + 32), _host(eng, dkept, n, np.uint32)
            res["agg" + rep], res["kept" + rep], res["status" + rep] = agg[:49 * m + 32], kept[:m], _host(eng, dst, n)
            # "zero behind the kept lanes": the device forms clear their outputs up to the capacity
            res["tail_is_zero" + rep] = int(not any(t.any() for t in tails + [agg[49 * m + 32:], kept[m:]]))
        return res
    if fam in ("verify_aggregate", "verify_aggregate_sliced"):
        sliced = fam == "verify_aggregate_sliced"
        if v[1] == "host":
            return dict(verdict=(eng.verify_aggregate_sliced if sliced else eng.verify_aggregate)(inp["agg"], pks, msgs,
                                                                                                  pk_inf=inf))
        da, dp, dmsg, di = _dev(inp["agg"], pks, msgs, inf)
        out = _tensor(1, "int32")
        _sync()
        (eng.verify_aggregate_sliced_device if sliced else eng.verify_aggregate_device)(
            _p(da), _p(dp), _p(dmsg), n, ml, _p(out), d_pk_inf=_p(di))
        eng.sync()
        return dict(verdict=int(out.item()))
    if fam == "verify_aggregates":
        counts = inp["counts"]
        if not dev:
            import schnorr_sig_amd as ssa
            return dict(verdicts=eng.verify_aggregates(ssa.split_aggregates(counts, inp["wire"]), pks, msgs, pk_inf=inf))
        dw, dp, dmsg, di = _dev(inp["wire"], pks, msgs, inf)
        dv = _tensor(counts.size, "int32")
        _sync()
        eng.verify_aggregates_device(dw, counts, dp, dmsg, d_verdicts=dv, d_pk_inf=di)
        eng.sync()
        return dict(verdicts=_host(eng, dv, counts.size, np.uint32))
    if fam == "verify_aggregates_cached":
        counts, wire_keys = inp["counts"], v[1] == "wire"
        cache = objs.get("wire" if wire_keys else "cache")
        keys, kinf = (inp["keys49"], None) if wire_keys else (pks, inf)
        res = {}
        for rep in ("", "_warm"):
            if not dev:
                import schnorr_sig_amd as ssa
                out, stats = eng.verify_aggregates_cached(cache, ssa.split_aggregates(counts, inp["wire"]), keys, msgs,
                                                          pk_inf=kinf)
            else:
                dw, dk, dmsg, di = _dev(inp["wire"], keys, msgs, kinf)
                dv = _tensor(counts.size, "int32")
                _sync()
                _, stats = eng.verify_aggregates_cached_device(cache, dw, counts, dk, dmsg, d_verdicts=dv, d_pk_inf=di)
                eng.sync()
                out = _host(eng, dv, counts.size, np.uint32)
            res["verdicts" + rep], res["bad_key_aggregates" + rep] = out, int(stats[6])
        return res
    if fam == "aggregator":
        return _run_aggregator(step, eng, objs, inp, v)
    if fam == "aggverifier":
        return _run_aggverifier(step, eng, objs, inp, v)
    raise KeyError(fam)


# ---- the streaming aggregator: one scenario, planned from the inputs alone
def aggregator_scenario(step, inp):
    """what the scenario does and which lanes the object holds after each of its stages, BY CONSTRUCTION"""
    fam, var, n, seed = step
    v = var.split(".")
    rng = np.random.default_rng(seed + 7)
    how = {"screened": ["screened"], "noscreen": ["noscreen"], "cached": ["cached"], "keyed": ["keyed"],
           "index": ["noscreen", "screened", "cached"]}[v[0]]
    chunks = [(lo, hi, how[c % len(how)]) for c, (lo, hi) in enumerate(cuts(n))]
    status, cls = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    for lo, hi, h in chunks:
        status[lo:hi], cls[lo:hi] = lane_status(inp, "F" if v[-1] == "dirty" else PUSH_RULE[h])[lo:hi], ADM_CLASS[h]
    if v[-1] == "dirty":
        status = np.ones(n, np.uint8)           # (which nonzero value is not part of the dirty step's check)
    k0 = np.nonzero(status == 0)[0]
    held = k0.size
    s = dict(chunks=chunks, status=status, cls=cls, k0=k0, held=held)
    if not held:
        return s
    s["takes"] = sorted({t for t in (1, 512, 513, held) if t <= held})
    s["select"] = rng.permutation(held)[:held // 2].astype(np.uint32)
    s["mask"] = (rng.random(held) < 1.0 / 3).astype(np.uint8)
    k1 = k0[s["mask"] == 0]
    s["drops"] = [min(512, k1.size), min(1, max(0, k1.size - 512))]
    k3 = k1[sum(s["drops"]):]
    s["indices"] = rng.permutation(k3.size)[:k3.size // 10].astype(np.uint32)
    s["k1"], s["k3"], s["k4"] = k1, k3, np.delete(k3, s["indices"])
    s["absent"] = rng.integers(0, 256, size=(2, 32), dtype=np.uint8)
    # look-ups: ids of held places (one of them twice), of the doubled lane, and ids no lane has
    dup = inp.get("dup")
    q1 = list(range(0, held, 7)) + ([int(np.searchsorted(k0, dup[1]))] if dup else []) + [0]
    s["query1"], s["query2"] = np.array(q1), np.array(list(range(0, held, 5)) + q1[-2:])

    def places(query, kept):
        out, there = [], set(kept.tolist())
        for p in query:
            lane = int(k0[p])
            at = [int(np.searchsorted(kept, x)) for x in (dup if dup and lane in dup else (lane,)) if x in there]
            out.append(min(at) if at else UNKNOWN)
        return np.array(out + [UNKNOWN, UNKNOWN], np.uint32)
    s["places1"], s["places2"] = places(s["query1"], k0), places(s["query2"], s["k4"])
    return s


def _run_aggregator(step, eng, objs, inp, v):
    n, dev = step.n, v[-1] == "dev"
    sc = aggregator_scenario(step, inp)
    keyed, adm, index = v[0] == "keyed", "admission" in v, v[0] == "index"
    sigs, pks, msgs, inf = (inp[k] for k in ("sigs", "pks", "msgs", "inf"))
    ag = eng.aggregator(n, hold_keys=keyed, hold_admission=adm, index=index)
    res = {}

    def push(lo, hi, how):
        cache = objs.get("cache") if how == "cached" else objs.get("wire") if how == "keyed" else None
        if not dev:
            if how == "keyed":
                return ag.push_keyed(cache, inp["keyed"][lo:hi], msgs[lo:hi])[:2]
            return ag.push(sigs[lo:hi], pks[lo:hi], msgs[lo:hi], pk_inf=inf[lo:hi], screen=how != "noscreen", cache=cache)[:2]
        dst = _tensor(hi - lo, "uint8")
        if how == "keyed":
            dk, dmsg = _dev(inp["keyed"][lo:hi], msgs[lo:hi])
            kept = ag.push_keyed_device(cache, dk, dmsg, d_status=dst)[0]
        else:
            ds, dp, dmsg, di = _dev(sigs[lo:hi], pks[lo:hi], msgs[lo:hi], inf[lo:hi])
            if how == "cached":
                kept = ag.push_cached_device(cache, ds, dp, dmsg, d_status=dst, d_pk_inf=di)[0]
            else:
                kept = ag.push_device(ds, dp, dmsg, d_status=dst, d_pk_inf=di, screen=how != "noscreen")
        eng.sync()
        return _host(eng, dst, hi - lo), kept

    def out_bytes(call, size, shape=None):
        """a device form that lands `size` bytes in a uint8 tensor"""
        d = _tensor(size, "uint8")
        _sync()
        call(d)
        eng.sync()
        a = _host(eng, d, size)
        return a.reshape(shape) if shape else a

    def finish(t=None):
        t = ag.info()["held"] if t is None else t
        return out_bytes(lambda d: ag.finish_device(d, t), 49 * t + 32) if dev else ag.finish_bytes(t)

    def leaves():
        h = ag.info()["held"]
        return out_bytes(lambda d: ag.leaves_device(d), 32 * h, (h, 32)) if dev else ag.leaves()

    def keys():
        h = ag.info()["held"]
        return out_bytes(lambda d: ag.keys_device(d), 49 * h, (h, 49)) if dev else ag.keys()

    def admission():
        h = ag.info()["held"]
        return out_bytes(lambda d: ag.admission_device(d), h) if dev else ag.admission()

    def lookup(ids):
        if not dev:
            return ag.lookup(ids)
        dids, dpl, dcnt = _dev(ids.reshape(-1))[0], _tensor(ids.shape[0], "int32"), _tensor(1, "int32")
        _sync()
        ag.lookup_device(dids, dpl, dcnt)
        eng.sync()
        return _host(eng, dpl, ids.shape[0], np.uint32), int(dcnt.item())

    def info():
        i = ag.info()
        return np.array([i[k] for k in ("held", "pushes", "offered", "dropped")], np.uint64)

    try:
        status, kept = np.full(n, 255, np.uint8), []
        for lo, hi, how in sc["chunks"]:
            st, m = push(lo, hi, how)
            status[lo:hi] = st
            kept.append(m)
        res.update(status=status, kept=np.array(kept, np.uint64), info=info())
        if not sc["held"]:
            res["finish"] = finish()
            return res
        for t in sc["takes"]:
            res["finish_%d" % t] = finish(t)
        res["leaves"] = leaves()
        if keyed:
            res["keys"] = keys()
        if adm:
            res["admission"] = admission()
        if index:
            ids = np.concatenate([res["leaves"][sc["query1"]], sc["absent"]])
            res["places"], res["unknown"] = lookup(ids)
        # ---- a chosen subset in a chosen order
        order = sc["select"]
        m = order.size
        if not dev:
            out = ag.finish_select_bytes(order, keys=keyed)
            res["select"], res["select_leaves"] = (out[0] if keyed else out), ag.leaves_select(order)
            if keyed:
                res["select_keys"] = out[1]
        else:
            dord = _dev(order.view(np.int32))[0]
            dagg, dk, dl, dr = _tensor(49 * m + 32, "uint8"), _tensor(49 * m, "uint8"), _tensor(32 * m, "uint8"), _tensor(2, "int32")
            _sync()
            ag.finish_select_device(dord, dagg, dr[0:1], dk if keyed else None)
            ag.leaves_select_device(dord, dl, dr[1:2])
            eng.sync()
            res["select"], res["select_leaves"] = _host(eng, dagg, 49 * m + 32), _host(eng, dl, 32 * m).reshape(m, 32)
            res["select_results"] = _host(eng, dr, 2, np.uint32)
            if keyed:
                res["select_keys"] = _host(eng, dk, 49 * m).reshape(m, 49)
        # ---- refused lists change nothing
        before, refused = (finish(), info()), 0
        for bad in (lambda: ag.remove_indices([0, sc["held"]]), lambda: ag.remove_indices([1, 1]),
                    lambda: ag.finish_bytes(sc["held"] + 1), lambda: ag.finish_select_bytes([0, 0]),
                    lambda: ag.drop_front(sc["held"] + 1), lambda: ag.remove(np.zeros(sc["held"] + 1, np.uint8))):
            try:
                bad()
            except RuntimeError:
                refused += 1
        after = (finish(), info())
        res["refused"] = refused
        res["refusals_changed_nothing"] = int(all(np.array_equal(a, b) for a, b in zip(before, after)))
        # ---- removals in place
        res["kept_after_remove"] = ag.remove_device(_dev(sc["mask"])[0]) if dev else ag.remove(sc["mask"])
        if index:
            ag.index_sync()             # takes the rebuild off the next look-up; changes no answer
        res["finish_after_remove"] = finish()
        for d in sc["drops"]:
            ag.drop_front(d)
        res["finish_after_drops"] = finish()
        idx = sc["indices"]
        res["kept_after_indices"] = ag.remove_indices_device(_dev(idx.view(np.int32))[0]) if dev else ag.remove_indices(idx)
        res["finish_after_indices"], res["leaves_after"], res["info_after"] = finish(), leaves(), info()
        if keyed:
            res["keys_after"] = keys()
        if adm:
            res["admission_after"] = admission()
        if index:
            ids = np.concatenate([res["leaves"][sc["query2"]], sc["absent"]])
            res["places_after"], res["unknown_after"] = lookup(ids)
            ii = ag.index_info()        # (compared with the reference run: how many rebuilds a scenario costs is not stated)
            res["index_info"] = np.array([ii[k] for k in ("indexed", "stale", "rebuilds", "overflowed", "lookups", "ids")],
                                         np.uint64)
        ag.reset()
        res["held_after_reset"] = ag.info()["held"]
        return res
    finally:
        ag.close()


# ---- the streaming aggregate verifier
def aggverifier_scenario(step, inp):
    """the finishes of the scenario and their verdicts BY CONSTRUCTION: {n_take: (honest scalar's, wrong scalar's)}"""
    v = step.variant.split(".")
    if v[-1] == "dirty":
        return {}
    off = inp["off"]
    return {t: (1, 1) if 0 <= off < t else (0, 2) for t in inp["e"]}


def mixed_places(inp):
    """(the pool's place of every lane of the block after the removal, UNKNOWN for a lane that left the pool or is not
    named; the same before the names are withheld)"""
    n = inp["n"]
    held = np.cumsum(1 - inp["drop"].astype(np.int64)) - 1
    looked_up = np.where(inp["drop"] == 0, held, UNKNOWN).astype(np.uint32)
    return np.where(inp["unnamed"] == 0, looked_up, UNKNOWN).astype(np.uint32), looked_up


def _run_aggverifier(step, eng, objs, inp, v):
    n, dev = step.n, v[-1] == "dev"
    sigs, pks, msgs, inf = (inp[k] for k in ("sigs", "pks", "msgs", "inf"))
    rs = np.ascontiguousarray(sigs[:, :49])
    mixed, wire = v[0] == "mixed", "wire" in v
    cache = objs.get("wire") if wire else objs.get("cache") if (v[0] == "cached" or "cached" in v) else None
    keys = inp["keys49"] if wire else pks
    require = 2 if "require2" in v else 0
    av = eng.aggregate_verifier(n + 8)
    pool, res = None, {}

    def push_all(pieces):
        """the pushes of the scenario, one after the other.  The plain device forms only enqueue, so the inputs of every
        piece are uploaded first and kept until the stream has run: the pushes stand in the stream back to back"""
        if not dev:
            for lo, hi in pieces:
                if wire:
                    av.push_wire(rs[lo:hi], keys[lo:hi], msgs[lo:hi], cache=cache)
                else:
                    av.push(rs[lo:hi], pks[lo:hi], msgs[lo:hi], pk_inf=inf[lo:hi], cache=cache)
            return
        uploads = [_dev(rs[lo:hi], keys[lo:hi], msgs[lo:hi], inf[lo:hi]) for lo, hi in pieces]
        for dr, dk, dmsg, di in uploads:
            if wire:
                av.push_wire_device(dr, dk, dmsg, cache=cache)
            else:
                av.push_device(dr, dk, dmsg, d_pk_inf=di, cache=cache)
        eng.sync()

    def finish(e, t):
        if not dev:
            return av.finish(e, t)
        de, dv = _dev(e)[0], _tensor(1, "int32")
        _sync()
        av.finish_device(de, dv, t)
        eng.sync()
        return int(dv.item())

    try:
        if "dirty" in step.variant.split("."):
            push_all(verifier_cuts(n))
            ff = np.full(32, 0xFF, np.uint8)
            res.update(held=av.info()["held"], few=finish(np.zeros(32, np.uint8), 3), all=finish(np.zeros(32, np.uint8), n),
                       noncanonical=finish(ff, 3))
            return res
        if not mixed:
            push_all(verifier_cuts(n))
        else:
            # the pool: an aggregator that admits every lane of the block, then loses about 5 % of them
            pool = eng.aggregator(n, hold_keys=require == 2, hold_admission=require == 2, index=True)
            for lo, hi in verifier_cuts(n):
                if require == 2:
                    st, m = pool.push_keyed(cache, np.concatenate([keys[lo:hi], sigs[lo:hi]], axis=1), msgs[lo:hi])[:2]
                else:
                    st, m = pool.push(sigs[lo:hi], pks[lo:hi], msgs[lo:hi], pk_inf=inf[lo:hi])[:2]
                assert m == hi - lo and not st.any()
            want, _ = mixed_places(inp)
            pieces = [(lo, hi, np.nonzero(want[lo:hi] == UNKNOWN)[0] + lo) for lo, hi in verifier_cuts(n)]     # (.., its unknown lanes)
            if not dev:
                ids = pool.leaves()
                res["pool_kept"] = pool.remove(inp["drop"])
                places, res["looked_up_unknown"] = pool.lookup(ids)
                res["looked_up"] = places.copy()
                places[inp["unnamed"] != 0] = UNKNOWN
                for lo, hi, u in pieces:
                    if wire:
                        av.push_mixed_wire(pool, places[lo:hi], rs[u], keys[u], msgs[u], cache=cache, require=require)
                    else:
                        av.push_mixed(pool, places[lo:hi], rs[u], pks[u], msgs[u], pk_inf=inf[u], cache=cache, require=require)
                av.push_known(pool, places[inp["again"]], cache=cache if require else None, require=require)
                res["places"] = places
            else:       # the places never leave the device: leaves -> look-up -> mixed pushes
                dids, dpl, dw = _tensor(32 * n, "uint8"), _tensor(n, "int32"), _tensor(len(pieces) + 2, "int32")
                dagain, dunnamed = _dev(inp["again"].astype(np.int64), inp["unnamed"])
                pool.leaves_device(dids)
                eng.sync()
                dids.view(n, 32)[dunnamed != 0] = 0xEE          # an id no lane has: the look-up answers UNKNOWN
                _sync()
                res["pool_kept"] = pool.remove_device(_dev(inp["drop"])[0])
                pool.lookup_device(dids, dpl, dw[0:1])
                uploads = [_dev(rs[u], keys[u], msgs[u], inf[u]) if u.size else (None,) * 4 for _, _, u in pieces]
                for k, ((lo, hi, u), (dr, dk, dmsg, di)) in enumerate(zip(pieces, uploads)):     # back to back, as above
                    word = dw[k + 1:k + 2]
                    if wire:
                        av.push_mixed_wire_device(pool, dpl[lo:hi], word, dr, dk, dmsg, cache=cache, require=require)
                    elif cache is not None:
                        av.push_mixed_device(pool, dpl[lo:hi], word, dr, dk, dmsg, d_pk_inf=di, cache=cache, require=require)
                    else:
                        av.push_mixed_device(pool, dpl[lo:hi], word, dr, dk, dmsg, d_pk_inf=di)
                eng.sync()
                dpl2 = dpl[dagain].contiguous()
                _sync()
                if require:
                    av.push_mixed_wire_device(pool, dpl2, dw[-1:], None, None, None, cache=cache, require=require)
                else:
                    av.push_known_device(pool, dpl2, dw[-1:])
                eng.sync()
                res["places"], res["result_words"] = _host(eng, dpl, n, np.uint32), _host(eng, dw, None, np.uint32)
        info = av.info()
        res["held"], res["cached_lanes"] = info["held"], info["reserved"]
        for t, e in inp["e"].items():
            wrong = e.copy()
            wrong[0] ^= 1
            res["honest_%d" % t], res["wrong_%d" % t] = finish(e, t), finish(wrong, t)
            if mixed:
                res["known_sum_%d" % t] = av.known_sum(t)
        av.reset()
        res["held_after_reset"] = av.info()["held"]
        return res
    finally:
        av.close()
        if pool is not None:
            pool.close()


# ---- what must come out by construction
def _expected_agg(step, inp, v):
    fam, var, n, _ = step
    if v[-1] == "dirty":
        return {}           # the dirty steps carry a check of their own: dirty_check
    if fam in ("aggregate", "aggregate_sliced"):
        st = lane_status(inp, "F" if v[0] == "check" else "nocheck")
        exp = {"status": st, "nfail": int((st != 0).sum()), "rc": int(st[st != 0].min()) if st.any() else 0}
        if st.any():
            exp["agg"] = np.zeros(49 * n + 32, np.uint8)
        return exp
    if fam == "aggregate_shards":
        st = lane_status(inp, "nocheck")
        if st.any():
            return {"rc": 3, "status": st, "agg": np.zeros(49 * n + 32, np.uint8)}
        return {"rc": 0, "status": st, "verdict": 0, "verdict_forged": 2}
    if fam == "aggregates":
        st = lane_status(inp, "F" if v[1] == "check" else "nocheck")
        start, _ = lane_starts(inp["counts"])
        results = np.array([int(st[a:b][st[a:b] != 0].min()) if st[a:b].any() else 0 for a, b in zip(start, start[1:])],
                           np.uint32)
        return {"status": st, "nfail": int((st != 0).sum()), "results": results}
    if fam in ("aggregate_valid", "aggregate_valid_cached", "aggregate_valid_keyed_cached"):
        st = lane_status(inp, "F" if fam == "aggregate_valid" else "TF")
        kept = np.nonzero(st == 0)[0].astype(np.uint32)
        exp = {}
        for rep in ("", "_warm") if fam != "aggregate_valid" else ("",):
            exp.update({"status" + rep: st, "kept" + rep: kept})
            if fam == "aggregate_valid_cached":
                exp.update({"pks_out" + rep: inp["pks"][kept], "inf_out" + rep: inp["inf"][kept]})
            if fam == "aggregate_valid_keyed_cached":
                exp["keys_out" + rep] = inp["keyed"][kept, :49]
            if v[-1] == "dev":
                exp["tail_is_zero" + rep] = 1
        return exp
    if fam in ("verify_aggregate", "verify_aggregate_sliced"):
        return {"verdict": {"honest": 0, "first": 2, "mid": 2, "last": 2, "e_ge_q": 3, "bad_r": 3}[v[0]]}
    if fam == "verify_aggregates":
        return {"verdicts": inp["verdicts"]}
    if fam == "verify_aggregates_cached":
        bad = int((inp["verdicts"] == 1).sum())
        return {"verdicts": inp["verdicts"], "verdicts_warm": inp["verdicts"], "bad_key_aggregates": bad,
                "bad_key_aggregates_warm": bad}
    if fam == "aggregator":
        sc = aggregator_scenario(step, inp)
        k0, k4, chunks = sc["k0"], sc["k4"], sc["chunks"]
        exp = {"status": sc["status"], "kept": np.array([(sc["status"][lo:hi] == 0).sum() for lo, hi, _ in chunks], np.uint64),
               "info": np.array([sc["held"], len(chunks), n, n - sc["held"]], np.uint64), "refused": 6,
               "refusals_changed_nothing": 1, "held_after_reset": 0, "kept_after_remove": int(sc["k1"].size), "kept_after_indices": int(k4.size),
               "info_after": np.array([k4.size, len(chunks), n, n - sc["held"]], np.uint64)}
        if v[0] == "keyed":
            exp.update(keys=inp["keyed"][k0, :49], keys_after=inp["keyed"][k4, :49],
                       select_keys=inp["keyed"][k0[sc["select"]], :49])
        if "admission" in v:
            exp.update(admission=sc["cls"][k0], admission_after=sc["cls"][k4])
        if v[0] == "index":
            exp.update(places=sc["places1"], unknown=2, places_after=sc["places2"],
                       unknown_after=int((sc["places2"] == UNKNOWN).sum()))
        if v[-1] == "dev":
            exp["select_results"] = np.zeros(2, np.uint32)
        return exp
    if fam == "aggverifier":
        exp = {"held": int(inp["lanes"].size), "cached_lanes": 0, "held_after_reset": 0}
        for t, (honest, wrong) in aggverifier_scenario(step, inp).items():
            exp["honest_%d" % t], exp["wrong_%d" % t] = honest, wrong
        if v[0] in ("cached", "wire"):
            exp["cached_lanes"] = n
        if v[0] == "mixed":
            places, looked_up = mixed_places(inp)
            exp.update(places=places, pool_kept=int((inp["drop"] == 0).sum()))
            if v[-1] == "dev":       # the look-up's count of unknown ids, then the result words of the two pushes
                exp["result_words"] = np.array([(places == UNKNOWN).sum()] + [0] * (len(verifier_cuts(n)) + 1), np.uint32)
            else:
                exp.update(looked_up=looked_up, looked_up_unknown=int((looked_up == UNKNOWN).sum()))
            del exp["cached_lanes"]     # (a function of the unknown lanes and of how the known ones were pushed: compared
        return exp                      #  with the reference run, not stated here)
    raise KeyError(fam)


def dirty_check(step, res):
    """the by-construction check of a dirty step: every lane was bad or malformed, nothing was kept or accepted"""
    fam, n = step.family, step.n
    if fam in ("aggregate", "aggregate_sliced"):       # lanes with one flipped bit and no pk_inf: the smallest status is 2
        assert res["rc"] == 2 and not res["agg"].any() and res["status"].all() and res["nfail"] == n, step
    elif fam == "aggregates":
        filled = np.array(COUNTS["allbad"]) > 0
        assert (res["results"][filled] == 2).all() and not res["results"][~filled].any(), (step, res["results"])
        assert not res["wire"].any() and res["status"].all() and res["nfail"] == n, (step, res["nfail"])
    elif fam in ("aggregate_valid", "aggregate_valid_cached"):
        for rep in ("", "_warm") if fam == "aggregate_valid_cached" else ("",):
            assert res["status" + rep].all() and res["kept" + rep].size == 0 and res["agg" + rep].size == 32, step
            assert not res["agg" + rep].any(), step
    elif fam == "verify_aggregate":
        assert res["verdict"] == 3, step
    elif fam == "verify_aggregates":
        assert (res["verdicts"] == np.where(np.array(COUNTS["allbad"]) > 0, 3, 2)).all(), step
    elif fam == "aggregator":
        assert res["status"].all() and not res["kept"].any() and res["info"][0] == 0 and res["info"][3] == n, step
        assert res["finish"].size == 32 and not res["finish"].any(), step
    elif fam == "aggverifier":
        # The verifier sees R's, keys and messages, no scalars.  make_batch(dirty): lane i has defect i % 5, and the
        # lanes 0, 10, 20, .. carry pk_inf.  Lanes 0 .. 2: R decodes, the key is on the curve (lane 0: pk_inf set, the
        # identity, its key bytes are not read) -- nothing is malformed, so a prefix of three is decided by the equation:
        # the zero scalar does not satisfy it (INVALID_SIGNATURE, 2), and a scalar >= q is MALFORMED (3) before anything
        # else ("e_agg >= q", ssa_verify_aggregate).  Lane 3's key has a non-canonical limb (the lane fails its check: every
        # finish that takes it would be MALFORMED), lane 4's key is the fixture outside the subgroup -- and after pushes
        # through a key cache finish answers "SSA_INVALID_PUBLIC_KEY if some lane i < n has key status
        # SSA_INVALID_PUBLIC_KEY ... The key decides, also over a malformed R or a wrong e_agg in the same prefix"
        # (include/schnorr_sig_amd.h, the cached pushes of the aggregate verifier): the whole pool answers 1, not 3.
        assert (res["held"], res["few"], res["all"], res["noncanonical"]) == (n, 2, 1, 3), (step, res)
    elif "status" in res:
        assert res["status"].all() and res["nfail"] == n, step
    else:
        assert res["verdict"] == 3, step


# ---- the models
class Transcript:
    """the leaves of some lanes of a step's inputs, hashed once by tests/aggregate_model.py; from them the aggregate of
    any list of those lanes in any order -- "what ssa_aggregate_many returns for those lanes handed in alone" """

    def __init__(self, be, inp, lanes, msgs=None, pks=None):
        self.be, self.inp = be, inp
        lanes = [int(i) for i in lanes]
        msgs, pks = inp["msgs"] if msgs is None else msgs, inp["pks"] if pks is None else pks
        felts = am.leaves(be, list(inp["sigs"][lanes, :49]), list(pks[lanes]), list(msgs[lanes])) if lanes else []
        self.felts = {i: [int(x) for x in f] for i, f in zip(lanes, felts)}

    def leaf_bytes(self, lanes):
        return np.array([self.felts[int(i)] for i in lanes], dtype=np.uint64).reshape(-1, 4).view(np.uint8).reshape(-1, 32)

    def coeffs(self, lanes):
        m = len(lanes)
        if not m:
            return []
        top = am.tree_top(self.be, [self.felts[int(i)] for i in lanes])
        return am.coeffs_of_root(self.be, am.root_of(self.be, top, m), m)

    def scalar(self, lanes):
        return am.fold(self.coeffs(lanes), self.inp["sigs"][np.asarray(lanes, np.int64)]) if len(lanes) else 0

    def aggregate(self, lanes):
        lanes = np.asarray(lanes, np.int64)
        return np.concatenate([self.inp["sigs"][lanes, :49].reshape(-1),
                               np.frombuffer(self.scalar(lanes).to_bytes(32, "little"), np.uint8)])


def _eq(got, want, what):
    assert got.shape == want.shape and np.array_equal(got, want), what


def _check_agg_models(step, inp, res, orc, v):
    """bytes against tests/aggregate_model.py over the oracle, at every size; am.verify at the smallest sizes"""
    fam, var, n, _ = step
    be = am.oracle_backend(orc)
    if v[-1] == "dirty":
        return
    reps = ("", "_warm") if fam in ("aggregate_valid_cached", "aggregate_valid_keyed_cached") else ("",)
    if fam in ("aggregate", "aggregate_sliced", "aggregate_shards"):
        if not res["rc"]:
            _eq(res["agg"], Transcript(be, inp, range(n)).aggregate(np.arange(n)), step)
    elif fam == "aggregates":
        start, off = lane_starts(inp["counts"])
        ok = [j for j in range(len(off)) if not res["results"][j]]
        tr = Transcript(be, inp, [i for j in ok for i in range(start[j], start[j + 1])])
        want = np.zeros(res["wire"].size, np.uint8)
        for j in ok:
            want[off[j]: off[j] + 49 * int(inp["counts"][j]) + 32] = tr.aggregate(np.arange(start[j], start[j + 1]))
        _eq(res["wire"], want, step)
    elif fam in ("aggregate_valid", "aggregate_valid_cached", "aggregate_valid_keyed_cached"):
        kept = res["kept"].astype(np.int64)
        want = Transcript(be, inp, kept).aggregate(kept)
        for rep in reps:
            _eq(res["agg" + rep], want, (step, rep))
    elif fam in ("verify_aggregate", "verify_aggregate_sliced"):
        msgs = inp["msgs"].copy()
        if inp["flip"] >= 0:
            msgs[inp["flip"], 1] ^= 0x04
        _eq(inp["honest_agg"], Transcript(be, inp, range(n), msgs).aggregate(np.arange(n)), step)     # what the maker made
        if n <= 2:
            assert res["verdict"] == am.verify(be, inp["agg"], inp["pks"], inp["msgs"], pk_inf=inp["inf"]), step
    elif fam in ("verify_aggregates", "verify_aggregates_cached"):
        start, off = lane_starts(inp["counts"])
        tr = Transcript(be, inp, range(n), inp["honest_msgs"], inp["honest_pks"])
        want = np.concatenate([tr.aggregate(np.arange(a, b)) for a, b in zip(start, start[1:])])
        _eq(inp["honest_wire"], want, step)
        if v[0] == "edges":                 # the point-exact verification: the aggregates of at most three lanes
            for j, c in enumerate(int(c) for c in inp["counts"]):
                if c <= 3 and inp["verdicts"][j] != 1:
                    lanes = slice(start[j], start[j + 1])
                    got = am.verify(be, inp["wire"][off[j]: off[j] + 49 * c + 32], inp["pks"][lanes], inp["msgs"][lanes])
                    assert got == res["verdicts"][j], (step, j)
    elif fam == "aggregator":
        sc = aggregator_scenario(step, inp)
        k0, k1, k3, k4 = sc["k0"], sc["k1"], sc["k3"], sc["k4"]
        tr = Transcript(be, inp, k0)
        for t in sc["takes"]:
            _eq(res["finish_%d" % t], tr.aggregate(k0[:t]), (step, "finish", t))
        _eq(res["leaves"], tr.leaf_bytes(k0), (step, "leaves"))
        _eq(res["select"], tr.aggregate(k0[sc["select"]]), (step, "select"))
        _eq(res["select_leaves"], tr.leaf_bytes(k0[sc["select"]]), (step, "select_leaves"))
        _eq(res["finish_after_remove"], tr.aggregate(k1), (step, "remove"))
        _eq(res["finish_after_drops"], tr.aggregate(k3), (step, "drop_front"))
        _eq(res["finish_after_indices"], tr.aggregate(k4), (step, "remove_indices"))
        _eq(res["leaves_after"], tr.leaf_bytes(k4), (step, "leaves_after"))
        if "admission" in v:                # the column moves with its lanes: the model's piecewise move
            pool = adm_model.ClassPool()
            for lo, hi, how in sc["chunks"]:
                lanes = k0[(k0 >= lo) & (k0 < hi)]
                pool.push([tr.felts[int(i)] for i in lanes], [0] * lanes.size, ADM_CLASS[how])
            _eq(res["admission"], np.array(pool.adm, np.uint8), (step, "admission"))
            pool.remove(np.nonzero(sc["mask"] == 0)[0], piece=512)
            pool.drop_front(sum(sc["drops"]), piece=512)
            pool.remove(np.delete(np.arange(k3.size), sc["indices"]), piece=512)
            _eq(res["admission_after"], np.array(pool.adm, np.uint8), (step, "admission_after"))
            assert pool.leaves == [tr.felts[int(i)] for i in k4], step
        if v[0] == "index":                 # the model's dictionary: id -> the lowest place that holds it
            for held, query, got in ((k0, sc["query1"], res["places"]), (k4, sc["query2"], res["places_after"])):
                d = index_model.lowest_places(tr.leaf_bytes(held))
                ids = np.concatenate([tr.leaf_bytes(k0[query]), sc["absent"]])
                _eq(got, np.array([d.get(bytes(x), UNKNOWN) for x in ids], np.uint32), (step, "lookup"))
    elif fam == "aggverifier":
        lanes = inp["lanes"]
        tr = Transcript(be, inp, range(n))
        for t, e in inp["e"].items():       # the honest scalars the maker made
            assert int.from_bytes(e.tobytes(), "little") == tr.scalar(lanes[:t]), (step, "e_agg", t)
        if v[0] == "mixed":
            places, _ = mixed_places(inp)
            held = np.nonzero(inp["drop"] == 0)[0]
            pool = mixed_model.ModelPool([tr.felts[int(i)] for i in held],
                                         [int.from_bytes(inp["sigs"][i, 49:].tobytes(), "little") for i in held])
            mv = mixed_model.MixedModelVerifier(be, 512, None, lambda r, pk: ("not decoded", None, None, None, False))
            u = np.nonzero(places == UNKNOWN)[0]
            mv.push_mixed(pool, [int(p) for p in places], list(inp["sigs"][u, :49]), list(inp["pks"][u]), list(inp["msgs"][u]))
            mv.push_mixed(pool, [int(p) for p in places[inp["again"]]], [], [], [])
            for t in inp["e"]:
                assert res["known_sum_%d" % t] == mv.known_sum(t), (step, "known_sum", t)


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
    # the aggregate families: 512 | 513 (AG_TREE_SPAN and the aggregator's block) and 8192 | 8193 cached lanes
    # (AGV_KST_SPAN) on top of the sizes above; the many-calls take the lists of COUNTS
    "aggregate": _steps("aggregate", [
        ("check.host.honest", 1), ("nocheck.dev.honest", 63), ("check.dev.bad", 257), ("nocheck.host.honest", 512),
        ("check.host.honest", 513), ("nocheck.host.bad", 3072), ("check.dev.honest", 3073), ("nocheck.dev.honest", 4095),
        ("check.host.honest", 4096), ("check.host.bad", 20000), ("nocheck.host.honest", 20000)], 23000),
    "aggregate_sliced": _steps("aggregate_sliced", [
        ("check.host.honest", 257), ("nocheck.dev.honest", 513), ("check.dev.bad", 3073), ("nocheck.host.honest", 20000)],
        24000),
    "aggregate_shards": _steps("aggregate_shards", [
        ("b4.honest", 63), ("b512.honest", 513), ("b256.bad", 3073), ("b2048.honest", 4096), ("b512.honest", 20000)], 24500),
    "aggregates": _steps("aggregates", [
        ("edges.check.host", N_OF["edges"]), ("edges.nocheck.dev", N_OF["edges"]), ("many.check.dev", N_OF["many"]),
        ("many.nocheck.host", N_OF["many"]), ("paths.check.host", N_OF["paths"]), ("paths.nocheck.dev", N_OF["paths"])], 25000),
    "aggregate_valid": _steps("aggregate_valid", [
        ("host", 1), ("dev", 63), ("host", 257), ("host", 512), ("dev", 513), ("host", 3072), ("dev", 3073), ("host", 4095),
        ("dev", 4096), ("host", 20000)], 26000),
    "aggregate_valid_cached": _steps("aggregate_valid_cached", [
        ("host", 257), ("dev", 3073), ("host", 4096), ("host", 20000)], 27000),
    "aggregate_valid_keyed_cached": _steps("aggregate_valid_keyed_cached", [
        ("host", 257), ("host", 3072), ("dev", 4095), ("dev", 20000)], 28000),
    "verify_aggregate": _steps("verify_aggregate", [
        ("honest.host", 1), ("honest.dev", 2), ("first.host", 63), ("mid.dev", 257), ("last.host", 512), ("honest.dev", 513),
        ("e_ge_q.host", 3072), ("bad_r.dev", 3072), ("honest.host", 3073), ("mid.host", 4095), ("first.dev", 4096),
        ("last.dev", 20000), ("honest.host", 20000)], 29000),
    "verify_aggregate_sliced": _steps("verify_aggregate_sliced", [
        ("honest.host", 257), ("mid.dev", 513), ("honest.dev", 3073), ("last.host", 20000)], 29500),
    "verify_aggregates": _steps("verify_aggregates", [
        ("edges.host", N_OF["edges"]), ("edges.dev", N_OF["edges"]), ("many.host", N_OF["many"]), ("many.dev", N_OF["many"]),
        ("paths.host", N_OF["paths"]), ("paths.dev", N_OF["paths"])], 31000),
    "verify_aggregates_cached": _steps("verify_aggregates_cached", [
        ("edges.affine.host", N_OF["edges"]), ("edges.wire.dev", N_OF["edges"]), ("many.affine.dev", N_OF["many"]),
        ("many.wire.host", N_OF["many"]), ("paths.wire.host", N_OF["paths"]), ("paths.affine.dev", N_OF["paths"])], 32000),
    "aggregator": _steps("aggregator", [
        ("screened", 257), ("noscreen", 257), ("keyed.holdkeys.dev", 257), ("cached", 1500), ("keyed.holdkeys", 1500),
        ("index.admission", 1500), ("screened.dev", 1500), ("noscreen.dev", 5000), ("cached.dev", 5000),
        ("keyed.holdkeys", 5000), ("index.admission.dev", 5000), ("screened", 20000)], 33000),
    "aggverifier": _steps("aggverifier", [
        ("plain", 257), ("cached", 257), ("mixed.wire.require2", 257), ("plain.dev", 1500), ("wire", 1500), ("mixed", 1500),
        ("mixed.cached", 1500), ("mixed.dev", 5000), ("mixed.cached.dev", 5000), ("cached.dev", 8500),
        ("mixed.wire.require2.dev", 8500), ("wire.dev", 20000)], 34000),
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
    # the aggregate families whose calls take any n: three slices, aggregates that straddle both slice boundaries,
    # finish prefixes on both sides of 512 and 8192
    Step("aggregate_sliced", "check.host.honest", SLICED_N, 30014), Step("verify_aggregate_sliced", "honest.host", SLICED_N, 30015),
    Step("verify_aggregate_sliced", "mid.dev", SLICED_N, 30016), Step("aggregate_valid", "host", SLICED_N, 30017),
    Step("aggregate_valid_keyed_cached", "host", SLICED_N, 30018),
    Step("verify_aggregates_cached", "sliced.wire.host", SLICED_N, 30019), Step("aggregator", "keyed.holdkeys", SLICED_N, 30020),
    Step("aggverifier", "mixed.wire.require2", SLICED_N, 30021),
]

# The sliced steps run on an engine whose lane slice AND MSM slice are 5000 lanes -- but for these families: their calls
# refuse n above the context's MSM slice (include/schnorr_sig_amd.h: the filtering producers, the aggregator's pushes and
# selections) and cut their key work by the lane slice alone, so their steps run on an engine whose LANE slice alone is
# 5000: 12 345 lanes are three slices of the key dedup and the key cache, inside one MSM slice
LANE_SLICED = ("aggregate_valid", "aggregate_valid_keyed_cached", "aggregator")


def slicing(step):
    """how the engine of a sliced step is cut: "lanes" (SSA_LANE_SLICE alone) or True (SSA_MSM_SLICE too)"""
    return "lanes" if step.family in LANE_SLICED else True


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
    # the aggregate families share ws_h, st_*, msm_*, scr_*, dd_*, kc_* with the ones above and the ag_* .. agv_* buffers
    # among themselves; each dirty step is checked by dirty_check
    "aggregate": Step("aggregate", "check.host.dirty", DIRTY_N, 40009),
    "verify_aggregate": Step("verify_aggregate", "honest.host.dirty", DIRTY_N, 40010),
    "verify_aggregates": Step("verify_aggregates", "allbad.host.dirty", DIRTY_N, 40011),
    "aggregates": Step("aggregates", "allbad.check.host.dirty", DIRTY_N, 40012),
    "aggregate_valid": Step("aggregate_valid", "host.dirty", DIRTY_N, 40013),
    "aggregate_valid_cached": Step("aggregate_valid_cached", "host.dirty", DIRTY_N, 40014),
    "aggregator": Step("aggregator", "screened.dirty", DIRTY_N, 40015),
    "aggverifier": Step("aggverifier", "cached.dirty", DIRTY_N, 40016),
}
OLD_DIRTY = list(DIRTY)[:9]             # the families of the verify side; the others are the aggregate side
SCREENED = ("verify_batch_screened", "verify_many_screened", "verify_many_cached", "verify_keyed_many_cached",
            "aggregate", "aggregates", "aggregate_valid", "aggregate_valid_cached", "aggregator")


def step_id(step):
    return "%s-%s-%d" % (step.family, step.variant, step.n)


def digest(res):
    """a short fingerprint of a result dict (messages)"""
    h = hashlib.sha256()
    for k in sorted(res):
        h.update(k.encode() + (res[k].tobytes() if isinstance(res[k], np.ndarray) else repr(res[k]).encode()))
    return h.hexdigest()[:12]
