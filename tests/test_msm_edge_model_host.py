"""The case table of tests/msm_edge_model.py is what tests/test_gpu_msm_edges.py runs on the GPU; here the model alone
decides, on the CPU, that every case reaches the branches it names -- under every order of a bucket's items and every
tree group -- and that the walk's result is the oracle's (tests/msm_records.py::cpu_partial on the built lanes).  No case
is skipped or excused: a case that does not produce its events fails this file."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import msm_edge_model as em      # noqa: E402
import msm_records as mr         # noqa: E402

Q = em.Q


@pytest.fixture(scope="module")
def builder(oracle):
    return em.Builder(oracle)


_BUILT = {}


def built(builder, case, n=None):
    key = (case.name, n)
    if key not in _BUILT:
        _BUILT[key] = builder.build_case(case, n)
    return _BUILT[key]


def test_signed_digits_mirror_and_shape():
    """the recoding against its definition (digits in range, the value they stand for) and the two shapes"""
    assert em.shape(4095) == em.Shape(8, 32, 128, 16) and em.shape(4096) == em.Shape(16, 16, 32768, 4096)
    import random
    rnd = random.Random(0x5D)
    for c in (8, 16):
        sh = em.shape_of_c(c)
        for k in [0, 1, Q - 1, (1 << 255) - 1, (1 << (c - 1)), (1 << (c - 1)) - 1] + [rnd.randrange(Q) for _ in range(300)]:
            digs, carry = em.signed_digits(k, c, sh.windows)
            assert all(-(1 << (c - 1)) <= d < (1 << (c - 1)) for d in digs)
            assert em.digits_value(digs, c) == k - (carry << (c * sh.windows))
            assert carry == 0 or k >= Q
    # a coefficient of 2^256 - 1 is reduced before it is recoded; unreduced it carries out of the last window
    assert em.signed_digits((1 << 256) - 1, 8, 32)[1] == 1


def test_every_digit_table_round_trips():
    """a digit vector with 0 < value < q is recoded to itself (the builder works from digit tables)"""
    seen = 0
    for case in em.CASES:
        sh = em.shape_of_c(case.c)
        for _, _, spec in case.entries:
            v = em.case_digits(case, spec)
            t = em.digits_value(v, case.c)
            assert 0 < t < Q, case.name
            assert em.signed_digits(t, case.c, sh.windows) == (v, 0), case.name
            seen += 1
    assert seen > 150


def test_case_table_is_complete():
    """every case names at least one event, in known words; the names are unique; both window widths are there"""
    names = [c.name for c in em.CASES]
    assert len(set(names)) == len(names) and len(names) >= 90
    for case in em.CASES:
        assert case.require, case.name
        for stage, kind in case.require | case.may:
            assert kind in em.KINDS and (stage in em.STAGES or stage == "tree"), (case.name, stage, kind)
    assert {c.c for c in em.CASES} == {8, 16}
    # every case at both window widths, but the six that need tree levels 2 and 3: 46 + 52
    c8 = {c.name[:-3] for c in em.CASES if c.c == 8}
    c16 = {c.name[:-4] for c in em.CASES if c.c == 16}
    assert len(c8) == 46 and c8 < c16 and all(n.startswith("tree_level") for n in c16 - c8) and len(c16 - c8) == 6
    # every (stage, branch) of DESIGN.md's table is required by some case
    req = {e for c in em.CASES for e in c.require}
    for want in [("bucket", k) for k in ("same", "opposite", "acc_identity", "addend_identity", "dbl_to_identity")] + \
                [("chunk_running", k) for k in ("same", "opposite", "acc_identity", "addend_identity")] + \
                [("chunk_total", k) for k in ("same", "opposite", "acc_identity", "addend_identity")] + \
                [("chunk_k0", k) for k in ("opposite", "dbl_of_identity", "dbl_to_identity")] + \
                [("tree", k) for k in ("same", "opposite", "acc_identity", "addend_identity", "dbl_to_identity")] + \
                [("tree2", k) for k in ("same", "opposite", "acc_identity")] + \
                [("tree3", k) for k in ("same", "opposite", "acc_identity", "dbl_to_identity")] + \
                [("horner", k) for k in em.KINDS]:
        assert want in req, want


@pytest.mark.parametrize("case", em.CASES, ids=lambda c: c.name)
def test_case_meets_its_events_and_the_oracle(builder, oracle, case):
    """every tree group: the walk produces every event the case names under every bucket order; its final element, as
    a point, is cpu_partial's, lin is the sum in Python integers; the small path's walk and the c = 16 walk of c = 8
    lanes give the same element"""
    b = built(builder, case)
    assert b.n == (em.PAD_C16 if case.c == 16 else em.PAD_C8) and em.shape(b.n).c == case.c
    final = None
    for tg in em.TREE_GROUPS:
        elem, events, may = em.walk_buckets(b.lanes, b.n, tg, b.r)
        assert em.required_events(case, tg, events) == [], (case.name, tg)
        assert case.may <= may, (case.name, tg)
        assert final is None or final == elem
        final = elem
    assert em.walk_small(b.lanes, b.r) == final
    if case.c == 8:
        assert em.walk_buckets(b.lanes, em.PAD_C16, 16, b.r)[0] == final
    pt, lin, mal = mr.cpu_partial(oracle, *em.active(b))
    assert not mal
    assert builder.element_point(final, b.r) == pt
    assert lin == b.lin == sum(ln.s * int.from_bytes(bytes(b.sigs[i, 49:]), "little") for ln, i in zip(b.lanes, b.active)) % Q
    if "nothing_below" in case.name or "all_coefficients_zero" in case.name:
        assert pt is None and (lin != 0) == ("nothing_below" in case.name)
    # the padding adds nothing: all of its coefficients are zero, and the whole call is the same sum
    assert not b.coeffs[[i for i in range(b.n) if i not in set(b.active)]].any()


def test_padding_lane_is_honest(builder, oracle):
    assert oracle.verify(builder.pad_sig, builder.pad_pk, builder.pad_msg) == 0


def test_scalar_instances(builder, oracle):
    """the lin-only instances: every (coefficient, e) pair on every one of the four lanes' neighbours, lin by Python
    integers and by cpu_partial"""
    inst = em.scalar_instances()
    assert len(inst) == 15 and {p for row in inst for p in row} == set(em.SCALAR_COMBOS)
    for combos in inst[:3]:
        b = builder.build_scalars(combos)
        assert b.n == 600 and tuple(b.active) == (0, 255, 256, 599)
        want = sum((co % Q) * e for co, e in combos) % Q
        pt, lin, mal = mr.cpu_partial(oracle, *em.active(b))
        assert not mal and lin == want == b.lin
        assert builder.element_point(em.walk_small(b.lanes), 1) == pt
        assert [int.from_bytes(bytes(b.coeffs[i]), "little") for i in b.active] == [co for co, _ in combos]


def test_no_case_is_met_by_emptiness(builder):
    """an instance without any active lane meets one event only, the identity doubled in Horner's chain -- chunks and
    tree groups without a non-identity input record nothing -- and so every case but all_coefficients_zero, which IS
    that instance, names at least one event (one per tree group where it names tree levels) that emptiness cannot meet"""
    empty = builder.build([], 8)
    for c, n in ((8, em.PAD_C8), (16, em.PAD_C16)):
        for tg in em.TREE_GROUPS:
            _, events, _ = em.walk_buckets(empty.lanes, n, tg)
            assert events == {("horner", "dbl_of_identity")}
            for case in em.CASES:
                if case.c == c and not case.name.startswith("all_coefficients_zero"):
                    named_levels_only = all(e[0] in ("tree2", "tree3") for e in case.require)
                    assert em.required_events(case, tg, events) or (named_levels_only and tg != 16), case.name


def test_tree_single_first_never_takes_the_copy_path(builder):
    """what sets tree_single_first apart from tree_single_middle and _last: its one chunk sum opens its group at every
    level and under every tree group, so the accumulator of the tree is never the identity when an addend is not"""
    for case in em.CASES:
        if case.name.startswith("tree_single_first"):
            b = built(builder, case)
            for tg in em.TREE_GROUPS:
                events = em.walk_buckets(b.lanes, b.n, tg, b.r)[1]
                assert not [e for e in events if e[0].startswith("tree") and e[1] != "addend_identity"], (case.name, tg)
