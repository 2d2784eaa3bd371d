"""The admission column and the mixed push through the key cache on the CPU: the entry points as
declared, what they refuse without a device, the create flags, the bytes an object allocates, the Python mirror's
ValueErrors, and the two models of tests/aggverifier_admission_model.py -- the class column under every removal, and the
refusal rule and verdict of a push that requires a class -- with a byte-level model of the column's move."""
import ctypes as C
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import aggregate_model as am
import aggverifier_admission_model as adm
from aggverifier_mixed_model import UNKNOWN
from test_aggverifier_mixed_host import world      # noqa: F401  (the fixture: ten honest lanes, a pool in reverse order)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PUSHES = ["ssa_aggverifier_push_mixed_cached", "ssa_aggverifier_push_mixed_cached_device",
          "ssa_aggverifier_push_mixed_cached_wire", "ssa_aggverifier_push_mixed_cached_wire_device"]
NEW = PUSHES + ["ssa_aggregator_admission", "ssa_aggregator_admission_device", "ssa_debug_aggregator_bytes_ex"]


# ---------------------------------------------------------------------------------------------- symbols
def test_symbols_are_declared_exported_and_bound():
    import schnorr_sig_amd as ssa
    header = open(os.path.join(ROOT, "include", "schnorr_sig_amd.h")).read()
    lib = os.path.join(ROOT, "schnorr-sig_amd", "csrc", "libschnorr_sig_amd.so")
    exported = set(subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout.split())
    for name in NEW:
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in exported, name
        assert name in ssa.ABI_SYMBOLS and getattr(ssa._lib, name).argtypes is not None, name
    # the documented argument lists: ctx, av, ag, kc, places, n, the u compact lanes, u, require, [result], stats
    args = {n: len(getattr(ssa._lib, n).argtypes) for n in NEW}
    assert args == {PUSHES[0]: 16, PUSHES[1]: 17, PUSHES[2]: 15, PUSHES[3]: 16, NEW[4]: 4, NEW[5]: 4, NEW[6]: 4}
    for name in PUSHES:
        assert ("int %s(ssa_ctx *ctx, ssa_aggverifier *av, ssa_aggregator *ag, ssa_keycache *kc," % name) in header
        decl = header[header.index("int %s(" % name):]
        assert re.search(r"size_t u, uint32_t require,\s+(uint32_t \*d_result_out,\s+)?uint64_t stats_out\[8\]\);",
                         decl[:decl.index(";") + 1]), name
    assert "#define SSA_AGGR_HOLD_ADMISSION 8u" in header and ssa.AGGR_HOLD_ADMISSION == 8
    for value, name in enumerate(("UNSCREENED", "SCREENED", "KEY_CHECKED")):
        assert ("#define SSA_ADM_%s %du" % (name, value)) in header and getattr(ssa, "ADM_" + name) == value
        assert getattr(adm, name) == value
    assert ssa.ABI_VERSION == ssa._lib.ssa_abi_version() == 5                     # additive: the version stays
    for method in ("admission", "admission_device"):
        assert callable(getattr(ssa.Aggregator, method))
    for method in ("push_mixed", "push_mixed_wire", "push_mixed_device", "push_mixed_wire_device", "push_known"):
        assert callable(getattr(ssa.AggregateVerifier, method))
    assert callable(ssa.aggregator_bytes_ex)
    with open(os.path.join(ROOT, "schnorr-sig_amd", "host", "schnorr_sig.hpp")) as fh:
        mirror = fh.read()
    for text in ("HoldAdmission = SSA_AGGR_HOLD_ADMISSION", "std::vector<uint8_t> admission(", "enum class Require",
                 "void push_mixed(Aggregator &pool, KeyCache &cache", "void push_mixed_wire(Aggregator &pool, KeyCache &cache"):
        assert text in mirror, text


def test_null_objects_and_lists_are_argument_errors():
    """what the entry points refuse before they touch a device, and write nothing"""
    import schnorr_sig_amd as ssa
    lib, word = ssa._lib, (C.c_uint32 * 3)(7, 7, 7)
    stats = (C.c_uint64 * 8)(*([9] * 8))
    places = (C.c_uint32 * 2)(0, UNKNOWN)
    buf = (C.c_uint8 * 16)(*([5] * 16))
    for require in (0, 1, 2, 3):
        assert lib.ssa_aggverifier_push_mixed_cached(None, None, None, None, places, 2, None, None, None, None, None, 0, 0, 0,
                                                     require, stats) == ssa.ERR_ARG
        assert lib.ssa_aggverifier_push_mixed_cached(None, None, None, None, None, 0, None, None, None, None, None, 0, 0, 0,
                                                     require, stats) == ssa.ERR_ARG
        assert lib.ssa_aggverifier_push_mixed_cached_device(None, None, None, None, None, 2, None, None, None, None, None, 0, 0,
                                                            0, require, C.byref(word, 4), stats) == ssa.ERR_ARG
        assert lib.ssa_aggverifier_push_mixed_cached_wire(None, None, None, None, places, 2, None, None, None, None, 0, 0, 0,
                                                          require, stats) == ssa.ERR_ARG
        assert lib.ssa_aggverifier_push_mixed_cached_wire_device(None, None, None, None, None, 2, None, None, None, None, 0, 0,
                                                                 0, require, C.byref(word, 4), stats) == ssa.ERR_ARG
    assert lib.ssa_aggregator_admission(None, None, 0, buf) == ssa.ERR_ARG
    assert lib.ssa_aggregator_admission_device(None, None, 0, buf) == ssa.ERR_ARG
    assert list(word) == [7, 7, 7] and list(stats) == [9] * 8 and list(buf) == [5] * 16


# ---------------------------------------------------------------------------------------------- create flags and bytes
def test_create_flags():
    """1 is a push flag, 4 is nobody's, 3 holds 1: refused as before; 8 and 8 | 2 are the new flag alone and with the
    key column.  Without a context create refuses everything, so the flags are read off the two byte reports, which
    refuse what create refuses"""
    import schnorr_sig_amd as ssa
    five, eight = (C.c_uint64 * 5)(), (C.c_uint64 * 8)()
    for flags in (1, 3, 4, 0x80000000, 9, 12, 16):
        assert ssa._lib.ssa_debug_aggregator_bytes(16, 0, flags, five) == ssa.ERR_ARG, flags
        assert ssa._lib.ssa_debug_aggregator_bytes_ex(16, 0, flags, eight) == ssa.ERR_ARG, flags
    for flags in (0, 2, 8, 10):
        assert ssa._lib.ssa_debug_aggregator_bytes(16, 0, flags, five) == 0, flags
        assert ssa._lib.ssa_debug_aggregator_bytes_ex(16, 0, flags, eight) == 0, flags
    assert ssa._lib.ssa_debug_aggregator_bytes_ex(16, 0, 8, None) == ssa.ERR_ARG
    assert ssa._lib.ssa_debug_aggregator_bytes_ex(0, 0, 8, eight) == ssa.ERR_ARG
    assert ssa._lib.ssa_debug_aggregator_bytes_ex(16, 3, 8, eight) == ssa.ERR_ARG
    h = C.c_void_p()
    assert ssa._lib.ssa_aggregator_create(None, 16, 0, ssa.AGGR_HOLD_ADMISSION, C.byref(h)) == ssa.ERR_ARG and not h.value


@pytest.mark.parametrize("capacity,B", [(1, 0), (511, 0), (512, 0), (513, 0), (1000, 64), (1 << 20, 0), (7, 2)])
def test_bytes_ex_against_bytes(capacity, B):
    import schnorr_sig_amd as ssa
    for hold_keys in (False, True):
        five = ssa.aggregator_bytes(capacity, B, hold_keys=hold_keys)
        plain = ssa.aggregator_bytes_ex(capacity, B, hold_keys=hold_keys)
        with_adm = ssa.aggregator_bytes_ex(capacity, B, hold_keys=hold_keys, hold_admission=True)
        assert plain == five + (0, 0, 0)                                   # without the flag: what it allocated before
        assert with_adm[:5] == five and with_adm[6:] == (0, 0)             # the column changes no other array
        assert capacity <= with_adm[5] <= capacity + 16
    # the five-word report takes the flag and writes five words: the word behind them stays
    out = (C.c_uint64 * 6)(*([0xEE] * 6))
    assert ssa._lib.ssa_debug_aggregator_bytes(capacity, B, ssa.AGGR_HOLD_ADMISSION | ssa.AGGR_HOLD_KEYS49, out) == 0
    assert tuple(out[:5]) == ssa.aggregator_bytes(capacity, B, hold_keys=True) and out[5] == 0xEE
    assert ssa._lib.ssa_debug_aggregator_bytes(capacity, B, ssa.AGGR_HOLD_ADMISSION, out) == 0
    assert tuple(out[:5]) == ssa.aggregator_bytes(capacity, B) and out[4] == 0 and out[5] == 0xEE


# ---------------------------------------------------------------------------------------------- the mirror
class FakeCache:
    def __init__(self, wire):
        self.wire, self.handle = wire, None


class FakePool:
    def __init__(self, hold_admission):
        self.hold_admission, self.handle = hold_admission, None


@pytest.mark.parametrize("require", [3, -1, 1.0, "2", None, True, 2 ** 32])
def test_the_mirror_refuses_a_require_that_is_no_class(require):
    import schnorr_sig_amd as ssa
    av = object.__new__(ssa.AggregateVerifier)            # no engine, no handle: a call would fail differently
    pool, cache, wcache = FakePool(True), FakeCache(False), FakeCache(True)
    with pytest.raises(ValueError):
        av.push_mixed(pool, [0], None, None, None, cache=cache, require=require)
    with pytest.raises(ValueError):
        av.push_mixed_wire(pool, [0], None, None, None, cache=wcache, require=require)
    with pytest.raises(ValueError):
        av.push_known(pool, [0], cache=cache, require=require)
    with pytest.raises(ValueError):
        av.push_mixed_device(pool, None, None, None, None, None, cache=cache, require=require)
    with pytest.raises(ValueError):
        av.push_mixed_wire_device(pool, None, None, None, None, None, cache=wcache, require=require)


def test_the_mirror_refuses_what_the_host_can_see():
    import schnorr_sig_amd as ssa
    av = object.__new__(ssa.AggregateVerifier)
    with_adm, without = FakePool(True), FakePool(False)
    affine, wire = FakeCache(False), FakeCache(True)
    for require in (1, 2):
        with pytest.raises(ValueError, match="hold_admission"):
            av.push_mixed(without, [0], None, None, None, cache=affine, require=require)
        with pytest.raises(ValueError, match="hold_admission"):
            av.push_mixed_wire(without, [0], None, None, None, cache=wire, require=require)
        with pytest.raises(ValueError, match="key cache"):
            av.push_mixed(with_adm, [0], None, None, None, require=require)        # a class without a cache
        with pytest.raises(ValueError, match="key cache"):
            av.push_known(with_adm, [0], require=require)
    with pytest.raises(ValueError, match="wire"):
        av.push_mixed(with_adm, [0], None, None, None, cache=wire)                 # the other mode, either way
    with pytest.raises(ValueError, match="wire"):
        av.push_mixed_wire(with_adm, [0], None, None, None, cache=affine)
    with pytest.raises(ValueError, match="wire"):
        av.push_mixed_wire(with_adm, [0], None, None, None, cache=None)
    with pytest.raises(ValueError, match="wire"):
        av.push_mixed_wire_device(with_adm, None, None, None, None, None, cache=None)
    with pytest.raises(ValueError):
        av.push_mixed(with_adm, [2 ** 32], None, None, None, cache=affine, require=2)      # places, as before


# ---------------------------------------------------------------------------------------------- the model, part one: the column moves
@pytest.mark.parametrize("n", range(1, 11))
def test_the_class_column_under_every_removal_and_front_drop(n):
    """a pool of n lanes, EVERY assignment of classes (the rows of one array: a move treats every row alike), every
    mask and every front drop, whole and in pieces of one and three lanes: the classes are those of the kept lanes, in
    order, and nothing in front of the first removed lane is written"""
    all_classes = np.array(list(itertools.product((0, 1, 2), repeat=n)), dtype=np.uint8)
    assert all_classes.shape == (3 ** n, n)
    masks = [[i for i in range(n) if not drop >> i & 1] for drop in range(1 << n)]
    fronts = [list(range(k, n)) for k in range(n + 1)]
    for kept in masks + fronts:
        for piece in (1, 3, n):
            col = all_classes.copy()
            m = adm.move(col, kept, piece)
            assert m == len(kept)
            assert (col[:, :m] == all_classes[:, kept]).all(), (kept, piece)
            first = next((c for c, s in enumerate(kept) if s != c), m)
            assert (col[:, :first] == all_classes[:, :first]).all()
    # the same through the pool's own calls, with pushes of three kinds behind a removal
    pool = adm.ClassPool()
    classes = [int(c) for c in all_classes[len(all_classes) // 2]]
    for c in classes:
        pool.push([[c, 0, 0, 0]], [c + 10], c)
    assert pool.adm == classes
    pool.drop_front(n // 2, piece=2)
    assert pool.adm == classes[n // 2:] and [v[0] for v in pool.leaves] == pool.adm
    pool.push([[9, 9, 9, 9]] * 2, [1, 2], adm.KEY_CHECKED)
    kept = list(range(0, len(pool.adm), 2))
    want = [pool.adm[i] for i in kept]
    pool.remove(kept, piece=3)
    assert pool.adm == want and len(pool.es) == len(want) == len(pool.leaves)
    pool.reset()
    assert pool.adm == [] and adm.below(pool, [0], 2) == []


# ---------------------------------------------------------------------------------------------- the model, part two: the push
def class_pool(pool, classes):
    return adm.ClassPool(pool.leaves, pool.es, classes)


@pytest.mark.parametrize("n", range(1, 9))
def test_a_push_is_refused_iff_a_named_lane_is_below_the_class(world, n):      # noqa: F811
    """every subset of known lanes, every require, EVERY assignment of classes to the block's lanes: refused iff some
    named lane is below `require` -- a lane that is not named never decides -- and a refusal changes nothing"""
    be, mul, pool, place, rs, pks, msgs, want = world
    av = adm.AdmissionVerifier(be, 4, *mul)
    empty = av.state()
    classes = [0] * len(pool.es)
    cpool = class_pool(pool, classes)
    checked = 0
    for assignment in itertools.product((0, 1, 2), repeat=n):
        for i, c in enumerate(assignment):
            cpool.adm[place[i]] = c
        for mask in range(1 << n):
            named = [i for i in range(n) if mask >> i & 1]
            places = [place[i] if mask >> i & 1 else UNKNOWN for i in range(n)]
            lowest = min((assignment[i] for i in named), default=2)
            for require in (0, 1, 2):
                refused = bool(adm.below(cpool, places, require))
                assert refused == (lowest < require), (assignment, mask, require)
                checked += 1
                if refused and (mask + require + sum(assignment)) % 61 == 0:       # the push itself, thinned out: it is the same rule
                    unk = [i for i in range(n) if not mask >> i & 1]
                    with pytest.raises(ValueError):
                        av.push_mixed_cached(cpool, places, [rs[i] for i in unk], [pks[i] for i in unk],
                                             [msgs[i] for i in unk], require)
                    assert av.state() == empty
    assert checked == 3 ** n * 2 ** n * 3


@pytest.mark.parametrize("n", range(1, 9))
def test_an_accepted_push_gives_the_one_shot_verdict(world, n):                # noqa: F811
    """every subset of known lanes and every require, under the class assignments that just pass (every named lane at
    exactly `require`, the others at 0) and that pass with room (all at 2): the verdict is am.verify's on the block, for
    the honest scalar and the negated one"""
    be, mul, pool, place, rs, pks, msgs, want = world
    root, e, v_honest, neg, v_neg = want[n]
    for mask in range(1 << n):
        unk = [i for i in range(n) if not mask >> i & 1]
        places = [place[i] if mask >> i & 1 else UNKNOWN for i in range(n)]
        verdicts = set()
        for require in (0, 1, 2):
            for classes in ([require if mask >> i & 1 else 0 for i in range(n)], [2] * n):
                cpool = class_pool(pool, [0] * len(pool.es))
                for i, c in enumerate(classes):
                    cpool.adm[place[i]] = c
                av = adm.AdmissionVerifier(be, 4, *mul)
                av.push_mixed_cached(cpool, places, [rs[i] for i in unk], [pks[i] for i in unk], [msgs[i] for i in unk],
                                     require)
                assert av.known == [bool(mask >> i & 1) for i in range(n)] and av.kst == [0] * n
                got = (av.finish(n, e), av.finish(n, neg))
                assert got == ((root, v_honest), (root, v_neg)), (n, mask, require)
                verdicts.add(got[0][1])
        assert verdicts == {am.OK}


def test_model_refusals_and_the_key_status_at_its_true_place(world):           # noqa: F811
    be, mul, pool, place, rs, pks, msgs, want = world
    cpool = class_pool(pool, [2] * len(pool.es))
    plain = adm.AdmissionVerifier(be, 2, *mul)
    for require in (3, -1):
        with pytest.raises(ValueError):
            plain.push_mixed_cached(cpool, [place[0]], [], [], [], require)
    with pytest.raises(ValueError):
        plain.push_mixed_cached(pool, [place[0]], [], [], [], 1)            # a pool without the column
    plain.push_mixed_cached(pool, [place[0]], [], [], [], 0)                # ... which require == 0 takes
    assert plain.finish(1, want[1][1])[1] == am.OK
    # lanes 0 .. 5, unknown at 1, 3 and 5; the key of lane 5 -- the LAST compact lane, j = 2 -- is outside the subgroup:
    # exactly the prefixes that reach place 5 say so.  A status written at held + j would refuse from place 2 on.
    bad_key = bytes(pks[5])
    av = adm.AdmissionVerifier(be, 2, *mul, key_status=lambda pk: adm.INVALID_PUBLIC_KEY if pk == bad_key else 0)
    known = {0, 2, 4}
    unk = [1, 3, 5]
    av.push_mixed_cached(cpool, [place[i] if i in known else UNKNOWN for i in range(6)], [rs[i] for i in unk],
                         [pks[i] for i in unk], [msgs[i] for i in unk], 2)
    assert av.kst == [0, 0, 0, 0, 0, adm.INVALID_PUBLIC_KEY]
    for n in range(1, 7):
        assert av.finish(n, want[n][1])[1] == (adm.INVALID_PUBLIC_KEY if n == 6 else am.OK), n
    assert av.finish(6, want[6][3])[1] == adm.INVALID_PUBLIC_KEY              # the key decides over a wrong scalar


# ---------------------------------------------------------------------------------------------- the bytes of the move
class ByteColumn:
    """a byte array that records who wrote what: the admission column and its staging are read and written as bytes"""

    def __init__(self, data):
        self.data = np.array(data, dtype=np.uint8)
        self.writes = np.zeros(self.data.size, np.int64)
        self.owner = {}

    def store8(self, lane, addr, v):
        assert 0 <= addr < self.data.size
        self.data[addr] = v
        self.writes[addr] += 1
        assert self.owner.setdefault(addr, lane) == lane, "two lanes write one byte"


def move_bytes(column, kept, first, piece, rng):
    """agx_k_move's fifth column and the copy behind it, piece by piece: thread t of a piece stores the one byte
    st_adm[t] = adm[src(c0 + t)]; the copy puts staging [0, cnt) onto places [c0, c0 + cnt).  -> the bytes written into
    the column, per place"""
    m, written = len(kept), np.zeros(column.size, np.int64)
    for c0 in range(first, m, piece):
        cnt = min(piece, m - c0)
        stage = ByteColumn(np.full(piece + 16, 0xEE))                     # the staging: poisoned, with room behind
        for t in rng.permutation(cnt):                                    # the threads of a launch run in no order
            stage.store8(int(t), int(t), column[kept[c0 + t]])
        assert (stage.writes[:cnt] == 1).all() and not stage.writes[cnt:].any()
        assert (stage.data[cnt:] == 0xEE).all()                           # nothing outside the piece
        column[c0:c0 + cnt] = stage.data[:cnt]                            # the stream-ordered copy back
        written[c0:c0 + cnt] += 1
    return written


@pytest.mark.parametrize("piece", [1, 2, 3, 5, 64])
@pytest.mark.parametrize("held", [1, 2, 7, 8, 9, 33])
def test_the_move_writes_every_staging_byte_once_and_the_column_where_it_must(held, piece):
    rng = np.random.default_rng(1000 * held + piece)
    for trial in range(12):
        column = rng.integers(0, 3, size=held + 16, dtype=np.uint8)
        column[held:] = 0xDD                                              # what lies behind `held`: stale bytes
        before = column.copy()
        if trial % 3 == 0:
            kept = list(range(int(rng.integers(0, held + 1)), held))      # a front drop
        else:
            kept = [i for i in range(held) if rng.integers(0, 3)]
        first = next((c for c, s in enumerate(kept) if s != c), len(kept))
        written = move_bytes(column, kept, first, piece, rng)
        m = len(kept)
        assert (column[:m] == before[kept]).all() if m else True
        assert (written[first:m] == 1).all() and not written[:first].any() and not written[m:].any()
        assert (column[m:] == before[m:]).all()                           # places behind the kept lanes keep their bytes
