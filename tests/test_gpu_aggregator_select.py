"""Selections of held lanes (ssa_aggregator_finish_select, ssa_aggregator_remove_indices):
finish_select(order) is, byte for byte, what ssa_aggregate_many (flags 0) returns for the named lanes handed in alone in
the list's order, its key column the pushed records' first 49 bytes in that order, and the object is not changed by it;
remove_indices leaves what remove leaves for the equivalent mask; a list with an index out of range or named twice is
refused on the device, its outputs zeroed, and no lane outside [0, held) is read.

Expected values come from Engine.aggregate on the selected lanes of the caller's arrays and from numpy indexing, never
from an aggregator; for one three-lane case also from tests/aggregate_model.py over the pymodel backend.  Objects:
  mixed4   flags 0, block_lanes 4: a screened plain push, a NO_SCREEN push and a keyed-cached push, each dropping a lane
  keyed8   key column, block_lanes 8: three keyed-cached pushes that drop four lanes
  keyed512 key column, the default block of 512."""
import ctypes as C
import os

import numpy as np
import pytest

import aggregate_model as am
from test_gpu_aggregate_valid_cached import Case, Honest, dev
from test_gpu_aggregates_cached import new_cache, spoil_classes

pytestmark = pytest.mark.gpu

OK = 0
N = 1160                                             # lanes offered; four are dropped
CAP = 2048
FILL = 0xEE
OBJECTS = {"mixed4": (4, False), "keyed8": (8, True), "keyed512": (0, True)}
BAD_SIG, BAD_E, BAD_KEY_AT, BAD_SIG2 = 100, 400, 700, 900
CUTS = [(0, 300), (300, 600), (600, N)]
_STATE = {}


# ------------------------------------------------------------------ the pool
def batch(engine):
    """N lanes by 40 repeating signers with a bad signature, a scalar e >= q, a key under P + T2 and another bad
    signature, one in each push"""
    if "batch" not in _STATE:
        c = Case(Honest(engine, N, seed=0x5E1EC7))
        c.sigs[BAD_SIG, 49] ^= 1
        c.sigs[BAD_E, 49:81] = 0xFF
        spoil_classes(engine, "affine")["p_plus_t2"](c.pks, c.inf, c.wire, BAD_KEY_AT)
        c.sigs[BAD_SIG2, 49] ^= 1
        c.rec = np.ascontiguousarray(np.concatenate([c.wire, c.sigs], axis=1))
        for a in (c.sigs, c.pks, c.inf, c.wire, c.msgs, c.rec):
            a.setflags(write=False)
        _STATE["batch"] = c
    return _STATE["batch"]


def load(engine, name, cache, capacity=CAP, lanes=None):
    """a new object of the kind `name` with the pool pushed -> (object, K: the lanes of the batch it holds, in order).
    lanes: an index array pushed in one keyed push instead (honest lanes)"""
    b = batch(engine)
    B, hold = OBJECTS[name]
    ag = engine.aggregator(capacity, B, hold_keys=hold)
    if lanes is not None:
        st, m, _ = ag.push_keyed(cache, b.rec[lanes], b.msgs[lanes])
        assert m == len(lanes) and not st.any()
        return ag, np.asarray(lanes, dtype=np.int64)
    kept = []
    for j, (lo, hi) in enumerate(CUTS):
        if hold or j == 2:
            st, m, _ = ag.push_keyed(cache, b.rec[lo:hi], b.msgs[lo:hi])
        else:
            st, m = ag.push(b.sigs[lo:hi], b.pks[lo:hi], b.msgs[lo:hi], pk_inf=b.inf[lo:hi], screen=(j == 0))
        assert m == int((st == 0).sum()) == hi - lo - (2 if j == 2 else 1), (name, j, np.flatnonzero(st))
        kept.append(lo + np.flatnonzero(st == 0))
    K = np.concatenate(kept)
    assert K.tolist() == [i for i in range(N) if i not in (BAD_SIG, BAD_E, BAD_KEY_AT, BAD_SIG2)]
    return ag, K


@pytest.fixture(scope="module")
def objs(engine):
    """the three objects, loaded once: no test may change them (finish_select does not)"""
    cache = new_cache(engine, "wire")
    made = {name: load(engine, name, cache) for name in OBJECTS}
    yield {"cache": cache, **made}
    for ag, _ in made.values():
        ag.close()
    cache.close()


def ref(engine, lanes):
    """Engine.aggregate of the lanes `lanes` of the batch handed in alone, computed once each and never changed"""
    b = batch(engine)
    lanes = np.asarray(lanes, dtype=np.int64)
    key = ("ref", lanes.tobytes())
    if key not in _STATE:
        if lanes.size == 0:
            agg = np.zeros(32, np.uint8)
        else:
            st, agg, _, nf = engine.aggregate(b.sigs[lanes], b.pks[lanes], b.msgs[lanes], pk_inf=b.inf[lanes])
            assert st == OK and nf == 0
        agg.setflags(write=False)
        _STATE[key] = agg
    return _STATE[key]


def select(ag, order, keys=None):
    """finish_select on buffers filled with FILL, with the keys where the object holds them -> (agg, keys or None)"""
    keys = ag.hold_keys if keys is None else keys
    out = ag.finish_select_bytes(order, keys=keys)
    return out if keys else (out, None)


def check_select(engine, ag, K, order):
    """the selection `order` of the object against Engine.aggregate and the caller's arrays"""
    b = batch(engine)
    order = np.asarray(order, dtype=np.int64)
    agg, keys = select(ag, order)
    lanes = K[order] if order.size else np.zeros(0, np.int64)
    assert agg.size == 49 * order.size + 32
    assert (agg[:49 * order.size].reshape(-1, 49) == b.sigs[lanes, :49]).all()            # every byte of every R
    assert (agg == ref(engine, lanes)).all()
    if ag.hold_keys:
        assert keys.shape == (order.size, 49) and (keys == b.wire[lanes]).all()
    return agg, keys


def state(ag, ns):
    """what a selection must leave alone: info but the finishes, finish(n) for the ns, keys(n)"""
    info = dict(ag.info(), finishes=0)
    return info, [ag.finish_bytes(n).tobytes() for n in ns], [ag.keys(n).tobytes() for n in ns] if ag.hold_keys else None


# ------------------------------------------------------------------ 1. shapes
def shapes(B, held):
    B = B or 512
    return sorted({0, 1, 2, B - 1, B, B + 1, 255, 256, 257, 511, 512, 513, held})


@pytest.mark.parametrize("name", list(OBJECTS))
def test_shapes(engine, objs, name):
    ag, K = objs[name]
    held = K.size
    assert ag.info()["held"] == held == N - 4
    rng = np.random.default_rng(0x5E1 + held)
    for m in shapes(OBJECTS[name][0], held):
        check_select(engine, ag, K, rng.choice(held, m, replace=False))


def test_three_lanes_against_the_model(engine, objs):
    b = batch(engine)
    ag, K = objs["mixed4"]
    order = [K.size - 1, 0, 517]
    lanes = K[order]
    agg, _ = select(ag, order)
    assert agg.tobytes() == am.aggregate(am.pymodel_backend(), b.sigs[lanes], b.pks[lanes], b.msgs[lanes])


# ------------------------------------------------------------------ 2. orders
def far_apart(held, m):
    """neighbours in the list from opposite ends of the object: 0, held - 1, 1, held - 2, ..."""
    lo, hi = np.arange(m // 2 + 1), held - 1 - np.arange(m // 2 + 1)
    return np.stack([lo, hi], axis=1).reshape(-1)[:m]


@pytest.mark.parametrize("name", list(OBJECTS))
def test_orders(engine, objs, name):
    ag, K = objs[name]
    held = K.size
    for m in (1, 5, 513, held):                      # the identity prefix is finish(m)
        agg, _ = check_select(engine, ag, K, np.arange(m))
        assert (agg == ag.finish_bytes(m)).all()
    check_select(engine, ag, K, np.arange(held)[::-1])
    check_select(engine, ag, K, np.random.default_rng(0x0DE2).permutation(held))
    check_select(engine, ag, K, np.arange(0, held, 2))
    # the shared dword of two lanes whose sources are far apart, at every alignment of 49 t mod 4: check_select compares
    # all 49 bytes of every R and key
    for m in (4, 5, 6, 7, 600):
        order = far_apart(held, m)
        assert {49 * t % 4 for t in range(m)} == {0, 1, 2, 3} and abs(int(order[1]) - int(order[0])) > held - 2
        check_select(engine, ag, K, order)


# ------------------------------------------------------------------ 3. the key column
def test_the_selection_is_what_the_validator_takes(engine, objs):
    import schnorr_sig_amd as ssa
    b = batch(engine)
    ag, K = objs["keyed8"]
    order = np.random.default_rng(0xB10C).choice(K.size, 700, replace=False)
    agg, keys = check_select(engine, ag, K, order)
    msgs = b.msgs[K[order]].copy()
    with new_cache(engine, "wire") as cache:
        v, _ = engine.verify_aggregates_cached(cache, [agg], keys, msgs)
        assert v.tolist() == [OK]
        msgs[350, 3] ^= 1
        v, _ = engine.verify_aggregates_cached(cache, [agg], keys, msgs)
        assert v.tolist() != [OK]
    # the keys of an object that holds none
    plain, _ = objs["mixed4"]
    lst = np.arange(5, dtype=np.uint32)
    out, k49 = np.full(49 * 5 + 32, FILL, np.uint8), np.full(49 * 5, FILL, np.uint8)
    before = state(plain, [5])
    assert ssa._lib.ssa_aggregator_finish_select(engine._ctx, plain.handle, ssa._ptr(lst), 5, ssa._ptr(out),
                                                 ssa._ptr(k49)) == ssa.ERR_ARG
    assert (out == FILL).all() and (k49 == FILL).all() and state(plain, [5]) == before
    with pytest.raises(RuntimeError):
        plain.finish_select(lst, keys=True)


# ------------------------------------------------------------------ 4. nothing moves
@pytest.mark.parametrize("name", ["mixed4", "keyed512"])
def test_a_selection_leaves_the_object_alone(engine, name):
    b = batch(engine)
    extra = np.arange(N - 200, N)                    # honest lanes, pushed once more behind the selection
    ns = [3, 512, N - 4]
    with new_cache(engine, "wire") as cache:
        ag, K = load(engine, name, cache)
        twin, _ = load(engine, name, cache)
        try:
            before, finishes = state(ag, ns), ag.info()["finishes"]
            check_select(engine, ag, K, np.random.default_rng(4).permutation(K.size)[:900])
            assert ag.info()["finishes"] == finishes + 1
            assert state(ag, ns) == before == state(twin, ns)
            drop = np.zeros(K.size + extra.size, np.uint8)
            drop[1::3] = 1
            for o in (ag, twin):
                st, m, _ = o.push_keyed(cache, b.rec[extra], b.msgs[extra])
                assert m == extra.size and not st.any()
                assert o.remove(drop) == int((drop == 0).sum())
            rest = np.concatenate([K, extra])[drop == 0]
            ns2 = [1, 513, rest.size]
            assert state(ag, ns2) == state(twin, ns2)
            assert (ag.finish_bytes() == ref(engine, rest)).all()
            check_select(engine, ag, rest, np.arange(rest.size)[::-1][:300])
        finally:
            ag.close()
            twin.close()


# ------------------------------------------------------------------ 5. refusals
def refused_lists(held, capacity):
    """name -> a list the device refuses.  `held` and `capacity - 1` name places behind the lanes held that hold stale
    lanes: each stands first, last, and directly behind a valid index (so that it is somebody's next source)"""
    rng = np.random.default_rng(0xBAD)
    base = rng.choice(held, 620, replace=False)
    out = {}
    adj = base.copy()
    adj[11] = adj[10]
    out["duplicate, adjacent"] = adj
    far = base.copy()
    far[400] = far[100]                              # 300 positions apart: other workgroups
    out["duplicate, 300 apart"] = far
    tri = base.copy()
    tri[[7, 300, 619]] = tri[50]
    out["three times"] = tri
    for what, idx in (("held", held), ("capacity - 1", capacity - 1)):
        for where, at in (("first", 0), ("last", base.size - 1), ("behind a valid index", 258)):
            lst = base.copy()
            lst[at] = idx
            out["%s, %s" % (what, where)] = lst
    out["one index, out of range"] = np.array([held])
    out["two lanes, the same"] = np.array([5, 5])
    return out


def test_refused_lists_zero_the_outputs_and_change_nothing(engine):
    """an object filled to its capacity and thinned by a remove: the places [held, capacity) hold stale lanes, inside
    the object's allocations, so a list that names them is safe to run.  What this test can see of such a list is the
    refusal: SSA_ERR_ARG / result word 1, every output byte zero, the object unchanged, and a valid call right afterwards
    correct.  It cannot see whether the stale lane was READ -- the outputs are zeroed either way --: that no thread forms
    an address from an unchecked index rests on the code of agx_k_select (every address comes from `src` or `nsrc`, both
    compared with `held` first; the comment above the kernel gives the argument), not on this test."""
    import schnorr_sig_amd as ssa
    import torch
    lib, p = ssa._lib, ssa._ptr
    b = batch(engine)
    lanes = np.setdiff1d(np.arange(N), [BAD_SIG, BAD_E, BAD_KEY_AT, BAD_SIG2])[:800]       # honest lanes
    capacity = lanes.size
    with new_cache(engine, "wire") as cache:
        ag, _ = load(engine, "keyed8", cache, capacity=capacity, lanes=lanes)
        try:
            drop = np.zeros(capacity, np.uint8)
            drop[5::6] = 1
            K = lanes[drop == 0]
            assert ag.remove(drop) == K.size
            held = K.size
            assert held < capacity - 1 and ag.info()["capacity"] == capacity
            ns = [1, 100, held]
            before = state(ag, ns)
            good = np.random.default_rng(77).permutation(held)[:620]
            for round_ in ("plain", "poisoned"):
                for name, lst in refused_lists(held, capacity).items():
                    lst = np.ascontiguousarray(lst, dtype=np.uint32)
                    m = lst.size
                    # the host form
                    agg, k49 = np.full(49 * m + 32, FILL, np.uint8), np.full(49 * m, FILL, np.uint8)
                    assert lib.ssa_aggregator_finish_select(engine._ctx, ag.handle, p(lst), m, p(agg), p(k49)) == ssa.ERR_ARG, name
                    assert not agg.any() and not k49.any(), name
                    with pytest.raises(RuntimeError):
                        ag.finish_select(lst)
                    # the device form
                    d_lst = torch.from_numpy(lst.astype(np.int32)).to("cuda:0")
                    d_agg = torch.full((49 * m + 32 + 8,), FILL, dtype=torch.uint8, device="cuda:0")
                    d_k49 = torch.full((49 * m + 8,), FILL, dtype=torch.uint8, device="cuda:0")
                    d_res = torch.full((1,), 0x55, dtype=torch.int32, device="cuda:0")
                    assert ag.finish_select_device(d_lst, d_agg[3:], d_res, d_k49[1:]) == m
                    engine.sync()
                    ga, gk = d_agg.cpu().numpy(), d_k49.cpu().numpy()
                    assert int(d_res.item()) == 1, name
                    assert not ga[3:3 + 49 * m + 32].any() and (ga[:3] == FILL).all() and (ga[3 + 49 * m + 32:] == FILL).all(), name
                    assert not gk[1:1 + 49 * m].any() and (gk[:1] == FILL).all() and (gk[1 + 49 * m:] == FILL).all(), name
                    # the removal by the same list
                    nk = C.c_uint64(0)
                    assert lib.ssa_aggregator_remove_indices(engine._ctx, ag.handle, p(lst), m, C.byref(nk)) == ssa.ERR_ARG, name
                    with pytest.raises(RuntimeError):
                        ag.remove_indices_device(d_lst)
                    assert dict(ag.info(), finishes=0) == before[0], name
                    # bitmap and flag are cleared per call: a valid list directly afterwards
                    check_select(engine, ag, K, good)
                assert state(ag, ns) == before
                engine.debug_poison_workspaces(0xA5 if round_ == "plain" else 0x00)
            check_select(engine, ag, K, good)
            assert state(ag, ns) == before
        finally:
            ag.close()


def test_argument_errors(engine, objs):
    import schnorr_sig_amd as ssa
    import torch
    lib, p = ssa._lib, ssa._ptr
    ag, K = objs["keyed8"]
    held = K.size
    before = state(ag, [held])
    lst = np.arange(held + 1, dtype=np.uint32)
    agg, k49, nk = np.full(49 * (held + 1) + 32, FILL, np.uint8), np.full(49 * (held + 1), FILL, np.uint8), C.c_uint64(7)
    ctx = engine._ctx
    d_lst = torch.arange(64, dtype=torch.int32, device="cuda:0")
    d_out = torch.full((49 * 64 + 32,), FILL, dtype=torch.uint8, device="cuda:0")
    d_res = torch.full((1,), 0x55, dtype=torch.int32, device="cuda:0")
    other = ssa.Engine(0)
    try:
        sel, rem = lib.ssa_aggregator_finish_select, lib.ssa_aggregator_remove_indices
        seld, remd = lib.ssa_aggregator_finish_select_device, lib.ssa_aggregator_remove_indices_device
        assert sel(ctx, ag.handle, p(lst), held + 1, p(agg), None) == ssa.ERR_ARG              # m > held
        assert rem(ctx, ag.handle, p(lst), held + 1, C.byref(nk)) == ssa.ERR_ARG
        assert sel(ctx, ag.handle, None, 3, p(agg), None) == ssa.ERR_ARG                       # no list
        assert rem(ctx, ag.handle, None, 3, C.byref(nk)) == ssa.ERR_ARG
        assert sel(ctx, ag.handle, p(lst), 3, None, None) == ssa.ERR_ARG                       # no output
        assert rem(ctx, ag.handle, p(lst), 3, None) == ssa.ERR_ARG
        assert sel(other._ctx, ag.handle, p(lst), 3, p(agg), None) == ssa.ERR_ARG              # not the object's context
        assert rem(other._ctx, ag.handle, p(lst), 3, C.byref(nk)) == ssa.ERR_ARG
        # the device forms: a list that is not 4-byte aligned, no result word
        for off in (1, 2, 3):
            assert seld(ctx, ag.handle, d_lst.data_ptr() + off, 8, d_out.data_ptr(), None, d_res.data_ptr()) == ssa.ERR_ARG
            assert remd(ctx, ag.handle, d_lst.data_ptr() + off, 8, C.byref(nk)) == ssa.ERR_ARG
        assert seld(ctx, ag.handle, d_lst.data_ptr(), 8, d_out.data_ptr(), None, None) == ssa.ERR_ARG
        engine.sync()
        assert (agg == FILL).all() and (k49 == FILL).all() and nk.value == 7
        assert int(d_res.item()) == 0x55 and (d_out.cpu().numpy() == FILL).all()
        assert state(ag, [held]) == before
        # an orphaned object
        with new_cache(other, "wire") as cache:
            b = batch(engine)
            orphan = other.aggregator(16, 4, hold_keys=True)
            assert orphan.push_keyed(cache, b.rec[:8], b.msgs[:8])[1] == 8
            handle = orphan.handle
    finally:
        other.close()
    try:
        assert sel(ctx, handle, p(lst), 3, p(agg), None) == ssa.ERR_ARG
        assert rem(ctx, handle, p(lst), 3, C.byref(nk)) == ssa.ERR_ARG
    finally:
        orphan.close()


def test_the_slice_bounds_a_selection_and_the_fold_walks_its_pieces():
    """a context whose MSM slice is 600 lanes: pieces of 512, so a selection of 600 lanes folds in two pieces, and one of
    601 is refused before anything is launched"""
    import schnorr_sig_amd as ssa
    old = os.environ.get("SSA_MSM_SLICE")
    os.environ["SSA_MSM_SLICE"] = "600"
    try:
        tight = ssa.Engine(0)
    finally:
        if old is None:
            del os.environ["SSA_MSM_SLICE"]
        else:
            os.environ["SSA_MSM_SLICE"] = old
    try:
        assert tight.info()["msm_slice"] == 600
        lanes = np.concatenate([np.arange(1, 97), np.arange(101, 101 + 299), np.arange(401, 401 + 299)])      # 694 honest
        with new_cache(tight, "wire") as cache:
            ag, K = load(tight, "keyed8", cache, lanes=lanes[:400])
            try:
                st, m, _ = ag.push_keyed(cache, batch(tight).rec[lanes[400:]], batch(tight).msgs[lanes[400:]])
                assert m == lanes.size - 400 and not st.any()
                perm = np.random.default_rng(600).permutation(lanes.size)
                for m in (512, 513, 600):
                    check_select(tight, ag, lanes, perm[:m])
                with pytest.raises(RuntimeError):
                    ag.finish_select(perm[:601])
                assert ag.remove_indices(perm[:601]) == lanes.size - 601       # a removal knows no slice limit
                rest = np.setdiff1d(np.arange(lanes.size), perm[:601])
                check_select(tight, ag, lanes[rest], np.arange(rest.size)[::-1])
            finally:
                ag.close()
    finally:
        tight.close()


# ------------------------------------------------------------------ 6. remove_indices
def remove_lists(B, held):
    B = B or 512
    rng = np.random.default_rng(0x2E0)
    return {"random": rng.choice(held, held // 3, replace=False),
            "with lane 0": np.array([700, 0, 13, held - 1]),
            "a front run of two blocks": rng.permutation(2 * B),
            "empty": np.zeros(0, np.int64),
            "everything": rng.permutation(held)}


@pytest.mark.parametrize("form", ["host", "device"])
@pytest.mark.parametrize("name", list(OBJECTS))
def test_remove_indices_is_remove_with_the_equivalent_mask(engine, name, form):
    import torch
    with new_cache(engine, "wire") as cache:
        for lname, lst in remove_lists(OBJECTS[name][0], N - 4).items():
            ag, K = load(engine, name, cache)
            twin, _ = load(engine, name, cache)
            try:
                mask = np.zeros(K.size, np.uint8)
                mask[lst] = 1
                rest = K[mask == 0]
                if form == "host":
                    got = ag.remove_indices(lst)
                else:
                    got = ag.remove_indices_device(torch.from_numpy(lst.astype(np.int32)).to("cuda:0"))
                assert got == twin.remove(mask) == rest.size, lname
                ns = sorted({0, min(1, rest.size), min(513, rest.size), rest.size})
                assert state(ag, ns) == state(twin, ns), lname
                assert (ag.finish_bytes() == ref(engine, rest)).all(), lname
            finally:
                ag.close()
                twin.close()


@pytest.mark.parametrize("name", ["mixed4", "keyed512"])
def test_take_select_leaves_the_complement_in_arrival_order(engine, name):
    import schnorr_sig_amd as ssa
    b = batch(engine)
    with new_cache(engine, "wire") as cache:
        ag, K = load(engine, name, cache)
        try:
            rng = np.random.default_rng(0x7A4E)
            first = rng.choice(K.size, 500, replace=False)
            out = ag.take_select(first)
            agg, keys = out if ag.hold_keys else (out, None)
            assert isinstance(agg, ssa.AggregateSignature) and agg.to_bytes() == ref(engine, K[first]).tobytes()
            rest = np.delete(K, first)
            assert ag.info()["held"] == rest.size and (ag.finish_bytes() == ref(engine, rest)).all()
            if ag.hold_keys:
                assert (keys == b.wire[K[first]]).all() and (ag.keys() == b.wire[rest]).all()
            second = rng.choice(rest.size, 400, replace=False)
            out = ag.take_select(second)
            agg = out[0] if ag.hold_keys else out
            assert agg.to_bytes() == ref(engine, rest[second]).tobytes()
            last = np.delete(rest, second)
            assert ag.info()["held"] == last.size and (ag.finish_bytes() == ref(engine, last)).all()
        finally:
            ag.close()


# ------------------------------------------------------------------ 7. the device forms
@pytest.mark.parametrize("name", list(OBJECTS))
def test_the_device_forms_give_the_bytes_of_the_host_forms(engine, objs, name):
    import torch
    b = batch(engine)
    ag, K = objs[name]
    held = K.size
    rng = np.random.default_rng(0xDE71CE)
    for m in (0, 1, 257, held):
        order = rng.choice(held, m, replace=False)
        want, want_keys = select(ag, order)
        d_order = torch.from_numpy(order.astype(np.int32)).to("cuda:0")
        d_agg = torch.full((49 * m + 32 + 8,), FILL, dtype=torch.uint8, device="cuda:0")
        d_k49 = torch.full((49 * m + 8,), FILL, dtype=torch.uint8, device="cuda:0") if ag.hold_keys else None
        d_res = torch.full((1,), 0x55, dtype=torch.int32, device="cuda:0")
        assert ag.finish_select_device(d_order, d_agg[5:], d_res, None if d_k49 is None else d_k49[3:]) == m
        engine.sync()
        got = d_agg.cpu().numpy()
        assert int(d_res.item()) == 0
        assert (got[5:5 + 49 * m + 32] == want).all() and (got[:5] == FILL).all() and (got[5 + 49 * m + 32:] == FILL).all()
        assert (want == ref(engine, K[order] if m else [])).all()
        if ag.hold_keys:
            gk = d_k49.cpu().numpy()
            assert (gk[3:3 + 49 * m].reshape(-1, 49) == want_keys).all() and (gk[:3] == FILL).all() and (gk[3 + 49 * m:] == FILL).all()
            assert (want_keys == b.wire[K[order]]).all() if m else want_keys.shape == (0, 49)
