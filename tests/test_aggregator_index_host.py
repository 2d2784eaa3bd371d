"""The leaf column and the leaf index of the streaming aggregator on the CPU: the entry points as
declared, what they refuse without a device, the create flag and the bytes it allocates, the Python mirror's
ValueErrors, and the two models of tests/aggregator_index_model.py -- the table under every insertion order, and the lazy
state machine against a dictionary rebuilt from scratch."""
import ctypes as C
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import aggregator_index_model as aim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"ssa_aggregator_index_sync": 2, "ssa_aggregator_lookup": 6, "ssa_aggregator_lookup_device": 6,
       "ssa_aggregator_leaves": 4, "ssa_aggregator_leaves_device": 4, "ssa_aggregator_leaves_select": 5,
       "ssa_aggregator_leaves_select_device": 6, "ssa_aggregator_index_info": 3}
DECLARED = [
    "int ssa_aggregator_index_sync(ssa_ctx *ctx, ssa_aggregator *ag);",
    "int ssa_aggregator_lookup(ssa_ctx *ctx, ssa_aggregator *ag, const uint8_t *ids32, size_t n, uint32_t *places_out, "
    "uint64_t *n_unknown_out);",
    "int ssa_aggregator_lookup_device(ssa_ctx *ctx, ssa_aggregator *ag, const uint8_t *d_ids32, size_t n, "
    "uint32_t *d_places_out, uint32_t *d_n_unknown_out);",
    "int ssa_aggregator_leaves(ssa_ctx *ctx, ssa_aggregator *ag, size_t n_take, uint8_t *ids32_out);",
    "int ssa_aggregator_leaves_device(ssa_ctx *ctx, ssa_aggregator *ag, size_t n_take, uint8_t *d_ids32_out);",
    "int ssa_aggregator_leaves_select(ssa_ctx *ctx, ssa_aggregator *ag, const uint32_t *order, size_t m, uint8_t *ids32_out);",
    "int ssa_aggregator_leaves_select_device(ssa_ctx *ctx, ssa_aggregator *ag, const uint32_t *d_order, size_t m, "
    "uint8_t *d_ids32_out, uint32_t *d_result_out);",
    "int ssa_aggregator_index_info(ssa_ctx *ctx, ssa_aggregator *ag, uint64_t out[8]);",
]


# ---------------------------------------------------------------------------------------------- symbols
def test_symbols_are_declared_exported_and_bound():
    import schnorr_sig_amd as ssa
    header = open(os.path.join(ROOT, "include", "schnorr_sig_amd.h")).read()
    flat = re.sub(r"\s+", " ", header)
    lib = os.path.join(ROOT, "schnorr-sig_amd", "csrc", "libschnorr_sig_amd.so")
    exported = set(subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout.split())
    for name, n_args in NEW.items():
        assert name in exported, name
        assert name in ssa.ABI_SYMBOLS and len(getattr(ssa._lib, name).argtypes) == n_args, name
    for decl in DECLARED:
        assert decl in flat, decl
    assert "#define SSA_AGGR_HOLD_INDEX 32u" in header and ssa.AGGR_HOLD_INDEX == 32
    assert ssa.ABI_VERSION == ssa._lib.ssa_abi_version() == 5                     # additive: the version stays
    assert ssa.AGGV_UNKNOWN == aim.UNKNOWN
    for method in ("index_sync", "lookup", "lookup_device", "leaves", "leaves_device", "leaves_select",
                   "leaves_select_device", "index_info"):
        assert callable(getattr(ssa.Aggregator, method)), method
    assert len(ssa.AGGREGATOR_INDEX_FIELDS) == 8
    with open(os.path.join(ROOT, "schnorr-sig_amd", "host", "schnorr_sig.hpp")) as fh:
        mirror = fh.read()
    for text in ("HoldIndex = SSA_AGGR_HOLD_INDEX", "void index_sync()", "Lookup lookup(const std::vector<uint8_t> &ids32)",
                 "std::vector<uint8_t> leaves(size_t n_take = All) const",
                 "std::vector<uint8_t> leaves_select(const std::vector<uint32_t> &order) const", "IndexInfo index_info() const"):
        assert text in mirror, text
    # the fail-open rule and the synchronisation of index_info are stated where a caller reads them
    assert "FAIL-OPEN" in header and "THE INDEX IS LAZY" in header and "SYNCHRONISES" in header


def test_null_objects_and_buffers_are_argument_errors():
    """what the entry points refuse before they touch a device, and write nothing"""
    import schnorr_sig_amd as ssa
    lib = ssa._lib
    ids = (C.c_uint8 * 64)(*([5] * 64))
    places = (C.c_uint32 * 4)(7, 7, 7, 7)
    count, words = C.c_uint64(9), (C.c_uint64 * 8)(*([9] * 8))
    order = (C.c_uint32 * 2)(0, 1)
    fake = C.c_void_p(0x1000)                       # never dereferenced: the context is NULL
    for n in (0, 2):
        assert lib.ssa_aggregator_lookup(None, None, ids, n, places, C.byref(count)) == ssa.ERR_ARG
        assert lib.ssa_aggregator_lookup(None, fake, ids, n, places, C.byref(count)) == ssa.ERR_ARG
        assert lib.ssa_aggregator_lookup_device(None, None, ids, n, places, places) == ssa.ERR_ARG
        assert lib.ssa_aggregator_leaves(None, None, n, ids) == ssa.ERR_ARG
        assert lib.ssa_aggregator_leaves_device(None, None, n, ids) == ssa.ERR_ARG
        assert lib.ssa_aggregator_leaves_select(None, None, order, n, ids) == ssa.ERR_ARG
        assert lib.ssa_aggregator_leaves_select_device(None, None, order, n, ids, places) == ssa.ERR_ARG
    assert lib.ssa_aggregator_index_sync(None, None) == ssa.ERR_ARG
    assert lib.ssa_aggregator_index_sync(None, fake) == ssa.ERR_ARG
    assert lib.ssa_aggregator_index_info(None, None, words) == ssa.ERR_ARG
    assert lib.ssa_aggregator_index_info(None, fake, None) == ssa.ERR_ARG
    assert list(ids) == [5] * 64 and list(places) == [7] * 4 and count.value == 9 and list(words) == [9] * 8


# ---------------------------------------------------------------------------------------------- create flags and bytes
def test_create_flags():
    """32 alone and with the key column and the admission column; 1 stays a push flag, 4, 16 and 64 nobody's.  Without a
    context create refuses everything, so the flags are read off the two byte reports, which refuse what create
    refuses"""
    import schnorr_sig_amd as ssa
    five, eight = (C.c_uint64 * 5)(), (C.c_uint64 * 8)()
    for flags in (32, 34, 40, 42, 0, 2, 8, 10):
        assert ssa._lib.ssa_debug_aggregator_bytes(16, 0, flags, five) == 0, flags
        assert ssa._lib.ssa_debug_aggregator_bytes_ex(16, 0, flags, eight) == 0, flags
    for flags in (33, 36, 48, 64, 0x80000020):
        assert ssa._lib.ssa_debug_aggregator_bytes(16, 0, flags, five) == ssa.ERR_ARG, flags
        assert ssa._lib.ssa_debug_aggregator_bytes_ex(16, 0, flags, eight) == ssa.ERR_ARG, flags
    accepted = [f for f in range(128) if ssa._lib.ssa_debug_aggregator_bytes_ex(16, 0, f, eight) == 0]
    assert accepted == [0, 2, 8, 10, 32, 34, 40, 42]
    h = C.c_void_p()
    assert ssa._lib.ssa_aggregator_create(None, 16, 0, ssa.AGGR_HOLD_INDEX, C.byref(h)) == ssa.ERR_ARG and not h.value


@pytest.mark.parametrize("capacity", [1, 255, 256, 257, 1000, 1 << 20])
def test_bytes_ex_reports_the_table_and_nothing_else_moves(capacity):
    import schnorr_sig_amd as ssa
    for hold_keys, hold_admission in itertools.product((False, True), repeat=2):
        plain = ssa.aggregator_bytes_ex(capacity, 0, hold_keys=hold_keys, hold_admission=hold_admission)
        with_index = ssa.aggregator_bytes_ex(capacity, 0, hold_keys=hold_keys, hold_admission=hold_admission, index=True)
        assert plain[6:] == (0, 0) and with_index[:6] == plain[:6] and with_index[7] == 0
        table = with_index[6]
        counter = 8
        assert (table - counter) % 8 == 0
        slots = (table - counter) // 8
        assert slots & (slots - 1) == 0 and slots >= 4 * capacity and slots >= 1024
        assert slots < 8 * capacity or slots == 1024                       # the smallest such power of two
        # the five-word report accepts the flag and reports what it reported
        five = (C.c_uint64 * 6)(*([0xEE] * 6))
        flags = ssa.AGGR_HOLD_INDEX | (ssa.AGGR_HOLD_KEYS49 if hold_keys else 0) | (ssa.AGGR_HOLD_ADMISSION if hold_admission else 0)
        assert ssa._lib.ssa_debug_aggregator_bytes(capacity, 0, flags, five) == 0
        assert tuple(five[:5]) == ssa.aggregator_bytes(capacity, 0, hold_keys=hold_keys) and five[5] == 0xEE


# ---------------------------------------------------------------------------------------------- the mirror
class FakeEngine:
    _ctx, device = None, 0


def fake_pool(index):
    import schnorr_sig_amd as ssa
    ag = object.__new__(ssa.Aggregator)             # no engine, no handle: a call into the library would fail differently
    ag.engine, ag.handle, ag.index, ag.hold_keys, ag.hold_admission = FakeEngine(), None, index, False, False
    return ag


def test_the_mirror_refuses_what_the_host_can_see():
    ag = fake_pool(False)
    ids = np.zeros((2, 32), np.uint8)
    with pytest.raises(ValueError, match="index=True"):
        ag.lookup(ids)
    with pytest.raises(ValueError, match="index=True"):
        ag.lookup_device(None, None, None)
    with pytest.raises(ValueError, match="index=True"):
        ag.index_sync()
    with pytest.raises(ValueError, match="index=True"):
        ag.index_info()
    ag = fake_pool(True)
    for size in (1, 31, 33, 63):
        with pytest.raises(ValueError, match="32 bytes"):
            ag.lookup(np.zeros(size, np.uint8))
        with pytest.raises(ValueError, match="32 bytes"):
            ag.lookup(bytes(size))
    with pytest.raises(ValueError):
        ag.lookup_device(np.zeros(64, np.uint8), None, None)               # no tensor on the engine's device
    with pytest.raises(ValueError):
        ag.leaves_select([2 ** 32])
    with pytest.raises(ValueError):
        ag.leaves_select([-1])
    with pytest.raises(ValueError):
        ag.leaves_select([0.5])


# ---------------------------------------------------------------------------------------------- the model: SipHash
def test_the_models_siphash_is_siphash_2_4():
    """the test vectors of the reference implementation (Aumasson, Bernstein): key 00 01 .. 0f, input 00 01 .. (len - 1)"""
    key = bytes(range(16))
    assert aim.siphash24(key, b"") == 0x726fdb47dd0e0e31
    assert aim.siphash24(key, bytes(range(1))) == 0x74f839c593dc67fd
    assert aim.siphash24(key, bytes(range(8))) == 0x93f5f5799a932462
    assert aim.siphash24(key, bytes(range(15))) == 0xa129ca6149be45e5      # the worked example of the paper
    # a fingerprint is the hash of 33 bytes: the leaf and the tag
    leaf = bytes(range(100, 132))
    assert aim.fingerprint(key, leaf) == aim.siphash24(key, leaf + bytes([aim.TAG]))


# ---------------------------------------------------------------------------------------------- the model: the table
VALUES = [bytes([v]) * 32 for v in range(8)]         # eight distinct leaves: duplicates are common


def pool_of(rng, n):
    return [VALUES[int(v)] for v in rng.integers(0, 8, n)]


def orders_of(n, rng):
    if n <= 6:
        return [list(p) for p in itertools.permutations(range(n))]
    return [list(range(n)), list(range(n - 1, -1, -1))] + [[int(v) for v in rng.permutation(n)] for _ in range(200)]


def answers(table, leaves, ids):
    return [table.lookup(leaves, len(leaves), x) for x in ids]


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 6, 9, 16, 33, 64])
def test_every_insertion_order_gives_the_lowest_place(n):
    """16 slots so that chains are long (the bound is the table: nothing overflows while 8 values fit 16 slots): the
    answer to every query is the lowest place under every order tried, and never depends on the order"""
    rng = np.random.default_rng(3600 + n)
    for trial in range(2 if n <= 6 else 1):
        leaves = pool_of(rng, n)
        want = aim.lowest_places(leaves)
        ids = VALUES + [bytes([200]) * 32]
        expect = [want.get(x, aim.UNKNOWN) for x in ids]
        for order in orders_of(n, rng):
            t = aim.Table(16, 16, key16=bytes(rng.integers(0, 256, 16, dtype=np.uint8)))
            t.insert_range(leaves, 0, n, order)
            assert t.overflowed == 0
            assert answers(t, leaves, ids) == expect, (leaves, order)
            assert sum(1 for w in t.words if w != aim.EMPTY) == len(want)      # one slot per distinct leaf


@pytest.mark.parametrize("n", [2, 5, 17, 64])
def test_an_incremental_insert_equals_a_rebuild(n):
    rng = np.random.default_rng(3700 + n)
    leaves = pool_of(rng, n)
    key = bytes(rng.integers(0, 256, 16, dtype=np.uint8))
    whole = aim.Table(16, 16, key)
    whole.insert_range(leaves, 0, n)
    for cut in sorted({1, n // 2, n - 1}):
        for _ in range(20):
            t = aim.Table(16, 16, key)
            t.insert_range(leaves, 0, cut, [int(v) for v in rng.permutation(cut)])
            t.insert_range(leaves, cut, n, [cut + int(v) for v in rng.permutation(n - cut)])
            # the owners are the same; WHICH slot a leaf took may differ with the order of two leaves in one chain
            assert sorted(w & 0xFFFFFFFF for w in t.words if w != aim.EMPTY) == \
                sorted(w & 0xFFFFFFFF for w in whole.words if w != aim.EMPTY)
            assert answers(t, leaves, VALUES) == answers(whole, leaves, VALUES)


@pytest.mark.parametrize("bound", [1, 2])
def test_a_short_bound_fails_open(bound):
    """with walks of one and two slots: no query returns a place whose leaf differs, a returned place is the lowest one,
    and the held ids answered unknown are exactly those whose every lane the model counted as overflowed"""
    rng = np.random.default_rng(3800 + bound)
    seen_overflow = 0
    for trial in range(300):
        n = int(rng.integers(1, 65))
        distinct = trial % 2 == 0
        leaves = [bytes(rng.integers(0, 256, 32, dtype=np.uint8)) for _ in range(n)] if distinct else pool_of(rng, n)
        t = aim.Table(16, bound, key16=bytes(rng.integers(0, 256, 16, dtype=np.uint8)))
        t.insert_range(leaves, 0, n, [int(v) for v in rng.permutation(n)])
        want = aim.lowest_places(leaves)
        unknown_held = 0
        for ident, lowest in want.items():
            got = t.lookup(leaves, n, ident)
            lanes = {p for p in range(n) if leaves[p] == ident}
            if got == aim.UNKNOWN:
                assert lanes <= t.lost, "an id is unknown only if every lane that holds it overflowed"
                unknown_held += len(lanes)
            else:
                assert leaves[got] == ident and got == min(lanes - t.lost)
                assert got == lowest or lowest in t.lost
        absent = bytes([201]) * 32
        assert t.lookup(leaves, n, absent) == aim.UNKNOWN
        assert t.overflowed == len(t.lost)
        if distinct:
            assert unknown_held == t.overflowed                             # distinct ids: the counter is the number of unknowns
        seen_overflow += t.overflowed
    assert seen_overflow > 0


# ---------------------------------------------------------------------------------------------- the model: the state machine
def test_the_lazy_state_machine_against_a_dictionary():
    """any sequence of push, remove, reset, sync and lookup over pools of up to 10 lanes: indexed, stale and the answers
    are those of a dictionary rebuilt from scratch, and only sync and lookup touch the table"""
    rng = np.random.default_rng(3636)
    for trial in range(300):
        pool = aim.IndexedPool(slots=64, bound=64, key16=bytes(rng.integers(0, 256, 16, dtype=np.uint8)))
        rebuilds, must_clear = 0, True
        for step in range(30):
            op = ("push", "remove", "reset", "sync", "lookup")[int(rng.integers(0, 5))]
            work = pool.index_work
            if op == "push":
                room = 10 - len(pool.leaves)
                pool.push(pool_of(rng, int(rng.integers(0, room + 1))))
                assert pool.index_work == work
            elif op == "remove":
                before = list(pool.leaves)
                kept = [i for i in range(len(before)) if rng.integers(0, 3)]
                pool.remove(kept)
                assert pool.index_work == work
                if len(kept) != len(before):
                    must_clear = True
                    assert pool.stale and pool.indexed == 0
            elif op == "reset":
                pool.reset()
                assert pool.index_work == work and pool.stale and pool.indexed == 0
                must_clear = True
            elif op == "sync":
                pool.sync()
                rebuilds += must_clear
                must_clear = False
                assert not pool.stale and pool.indexed == len(pool.leaves) and pool.rebuilds == rebuilds
            else:
                want = aim.lowest_places(pool.leaves)
                ids = VALUES + [bytes([200]) * 32] + pool.leaves[:2]
                places, unknown = pool.lookup(ids)
                rebuilds += must_clear
                must_clear = False
                expect = [want.get(x, aim.UNKNOWN) for x in ids]
                assert places == expect and unknown == expect.count(aim.UNKNOWN)
                assert not pool.stale and pool.indexed == len(pool.leaves) and pool.rebuilds == rebuilds
        assert pool.table.overflowed == 0
