"""Removing lanes from the streaming aggregator (ssa_aggregator_drop_front, ssa_aggregator_remove) on
the CPU: the plan of a removal -- which stored tops stay, which are moved, which are reduced again -- against brute force
over lane numbers, and the algorithm itself restated over the model of tests/aggregate_model.py: leaves compacted, tops
treated as the plan says, finish from the stored tops plus the ragged block, held against the one-shot aggregate of the
kept lanes for every mask, every prefix and one more push."""
import itertools

import numpy as np
import pytest

import aggregate_model as am
from test_aggregator_host import ModelAggregator, cached


# ---------------------------------------------------------------------------------------------- the plan of a removal
def removals(held, f, m):
    """sets of removed lanes that (held, first_changed, new_held) stands for: none; the front drop for f == 0; for a
    mask whose first removed lane is f, the run behind f and the set spread as far as it goes"""
    n = held - m
    if n == 0:
        return [[]]
    if f == 0:
        return [list(range(n))]
    return [list(range(f, f + n)), [f] + list(range(held - (n - 1), held))]


def brute_plan(held, f, m, B):
    """by lane numbers alone: a top STAYS when its block holds the same lanes as before under every removal the three
    numbers stand for; tops are MOVED only when every surviving block is an old block (then all of them by one shift);
    every other complete block is reduced again"""
    old = [tuple(range(B * b, B * b + B)) for b in range(held // B)]
    stays, shifts = [], []
    for gone in removals(held, f, m):
        gone = set(gone)
        lanes = [i for i in range(held) if i not in gone]
        assert len(lanes) == m
        new = [tuple(lanes[B * b: B * b + B]) for b in range(m // B)]
        stays.append(next((b for b, blk in enumerate(new) if blk != old[b]), len(new)))
        shifts.append({old.index(blk) - b if blk in old else None for b, blk in enumerate(new)})
    unchanged = min(stays)
    if unchanged == m // B and held == m:
        return (unchanged, 0, unchanged, 0)
    if all(len(s) <= 1 and None not in s for s in shifts) and held != m and f == 0:
        return (0, m // B, m // B, 0)
    return (unchanged, 0, unchanged, m // B - unchanged)


def check_plan(held, f, m, B):
    import schnorr_sig_amd as ssa
    got = ssa.aggregator_remove_plan(held, f, m, B)
    assert got == brute_plan(held, f, m, B), (held, f, m, B, got)
    unchanged, moved, first, count = got
    # every complete block of the new object in exactly one class
    assert (moved == 0 or unchanged == 0 == count) and first == max(unchanged, moved) and first + count == m // B
    if moved:
        assert (held - m) % B == 0 and (held - m) // B + moved <= held // B


@pytest.mark.parametrize("B", [2, 4, 8, 64])
def test_remove_plan_against_brute_force(B):
    for held in range(71):
        for m in range(held + 1):
            for f in range(m + 1):
                check_plan(held, f, m, B)


def test_remove_plan_around_the_default_block():
    import schnorr_sig_amd as ssa
    edges = [0, 1, 511, 512, 513, 1023, 1024, 1025, 1536, 1537]
    for held in edges:
        for m in (e for e in edges if e <= held):
            for f in (e for e in edges if e <= m):
                check_plan(held, f, m, 512)
                assert ssa.aggregator_remove_plan(held, f, m, 0) == ssa.aggregator_remove_plan(held, f, m, 512)
    assert ssa.aggregator_remove_plan(1536, 0, 1024, 512) == (0, 2, 2, 0)          # drop_front(512): two tops moved
    assert ssa.aggregator_remove_plan(1536, 0, 1023, 512) == (0, 0, 0, 1)          # drop_front(513): one block again
    assert ssa.aggregator_remove_plan(1536, 1000, 1535, 512) == (1, 0, 1, 1)       # lane 1000: block 0 stays


def test_remove_plan_refusals():
    import schnorr_sig_amd as ssa
    for B in (1, 3, 6, 1024, 513):
        with pytest.raises(RuntimeError):
            ssa.aggregator_remove_plan(8, 0, 4, B)
    for held, f, m in ((8, 0, 9), (8, 5, 4), (8, 9, 8), ((1 << 30) + 1, 0, 0)):
        with pytest.raises(RuntimeError):
            ssa.aggregator_remove_plan(held, f, m, 4)
    assert ssa._lib.ssa_debug_aggregator_remove_plan(8, 0, 4, 4, None) == ssa.ERR_ARG


def test_symbols_are_declared_and_exported():
    import os
    import schnorr_sig_amd as ssa
    names = ["ssa_aggregator_drop_front", "ssa_aggregator_remove", "ssa_aggregator_remove_device",
             "ssa_debug_aggregator_remove_plan"]
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include",
                               "schnorr_sig_amd.h")).read()
    assert all(n in ssa.ABI_SYMBOLS and ("int %s(" % n) in header for n in names)
    assert ssa.ABI_VERSION == ssa._lib.ssa_abi_version() == 5                      # additive: the version stays


def test_null_handles_are_argument_errors():
    """what the entry points refuse before they touch a device"""
    import ctypes as C
    import schnorr_sig_amd as ssa
    lib, nk, mask = ssa._lib, C.c_uint64(7), (C.c_uint8 * 4)()
    assert lib.ssa_aggregator_drop_front(None, None, 0) == ssa.ERR_ARG
    assert lib.ssa_aggregator_remove(None, None, mask, 4, C.byref(nk)) == ssa.ERR_ARG
    assert lib.ssa_aggregator_remove_device(None, None, mask, 4, C.byref(nk)) == ssa.ERR_ARG
    assert nk.value == 7


# ---------------------------------------------------------------------------------------------- the algorithm over the model
N = 8


def model_apply(ag, kept, plan):
    """the kept lanes (ascending old places) move to the front of a ModelAggregator; its tops as the plan says"""
    held, B = len(ag.leaves), ag.B
    unchanged, moved, first, count = plan
    ag.rs, ag.es, ag.leaves = ([a[i] for i in kept] for a in (ag.rs, ag.es, ag.leaves))
    shift = (held - len(kept)) // B
    tops = ag.tops[shift: shift + moved] if moved else ag.tops[:unchanged]
    assert len(tops) == first
    tops += [am.tree_top(ag.be, ag.leaves[B * b: B * (b + 1)]) for b in range(first, first + count)]
    assert len(tops) == len(kept) // B
    ag.tops = tops


def model_drop_front(ag, n):
    import schnorr_sig_amd as ssa
    held = len(ag.leaves)
    model_apply(ag, list(range(n, held)), ssa.aggregator_remove_plan(held, 0, held - n, ag.B))


def model_remove(ag, drop):
    import schnorr_sig_amd as ssa
    held = len(ag.leaves)
    kept = [i for i in range(held) if not drop[i]]
    f = next((i for i in range(held) if drop[i]), len(kept))
    # (a mask that removes lane 0 is no front drop to the library: every block is reduced again)
    plan = ssa.aggregator_remove_plan(held, f, len(kept), ag.B) if f else (0, 0, 0, len(kept) // ag.B)
    model_apply(ag, kept, plan)
    return kept


@pytest.fixture(scope="module")
def lanes(oracle):
    """N + 1 honest signatures, the caching pymodel back-end, and ref(lanes) -> the one-shot (root, aggregate) of those
    lanes handed in alone, each computed once"""
    rng = np.random.default_rng(0xD80F)
    s = rng.integers(0, 256, size=(2, N + 1, 32), dtype=np.uint8)
    s[:, :, 31] &= 0x3F
    s[:, :, 0] |= 1
    msgs = rng.integers(0, 256, size=(N + 1, 80), dtype=np.uint8)
    pks, sigs = oracle.keygen_sign_many(s[0], s[1], msgs)
    be = cached(am.pymodel_backend())
    refs = {(): (None, bytes(32))}

    def ref(idx):
        idx = tuple(idx)
        if idx not in refs:
            k = list(idx)
            rs = [bytes(x)[:49] for x in sigs[k]]
            root = am.root_of(be, am.tree_top(be, am.leaves(be, rs, pks[k], msgs[k])), len(k))
            refs[idx] = (root, am.aggregate(be, sigs[k], pks[k], msgs[k]))
        return refs[idx]
    return be, sigs, pks, msgs, ref


def loaded_model(be, sigs, pks, msgs, n, B):
    ag = ModelAggregator(be, B)
    ag.push(sigs[:n], pks[:n], msgs[:n])
    return ag


def check_prefixes_then_push(ag, kept, lanes):
    be, sigs, pks, msgs, ref = lanes
    for take in itertools.chain(range(len(kept), -1, -1), range(len(kept) + 1)):
        assert ag.finish(take) == ref(kept[:take]), (ag.B, kept, take)
    ag.push(sigs[N:], pks[N:], msgs[N:])                  # later pushes append behind lane |K|
    assert len(ag.tops) == (len(kept) + 1) // ag.B
    assert ag.finish(len(kept) + 1) == ref(list(kept) + [N]), (ag.B, kept)


@pytest.mark.parametrize("B", [2, 4, 8])
def test_model_of_remove_equals_the_one_shot_aggregate_of_the_kept_lanes(lanes, B):
    be, sigs, pks, msgs, ref = lanes
    for n in range(1, N + 1):
        for drop in itertools.product((0, 1), repeat=n):
            ag = loaded_model(be, sigs, pks, msgs, n, B)
            kept = model_remove(ag, drop)
            check_prefixes_then_push(ag, kept, lanes)


@pytest.mark.parametrize("B", [2, 4, 8])
def test_model_of_drop_front_equals_the_one_shot_aggregate_of_the_rest(lanes, B):
    be, sigs, pks, msgs, ref = lanes
    for n in range(1, N + 1):
        for k in range(n + 1):
            ag = loaded_model(be, sigs, pks, msgs, n, B)
            model_drop_front(ag, k)
            check_prefixes_then_push(ag, list(range(k, n)), lanes)
            if k < n:                                     # and a second block taken from what is left
                ag2 = loaded_model(be, sigs, pks, msgs, n, B)
                model_drop_front(ag2, k)
                model_drop_front(ag2, 1)
                assert ag2.finish(n - k - 1) == ref(list(range(k + 1, n))), (B, n, k)
