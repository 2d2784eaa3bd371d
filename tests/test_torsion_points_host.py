"""The torsion keys of tests/torsion_points.py and the ladder event model (tests/ladder_event_model.py), on the CPU.

Part one proves the fixtures: every point has exactly the order it is filed under, lies outside the prime subgroup, and
the C oracle multiplies it as the Python model does.  Part two proves the model: its digits recompose the scalar, and
the accumulator it predicts window by window is the point the textbook sequence of doublings and additions reaches."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import ladder_event_model as lem
import pymodel as m
import torsion_points as tp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q = m.Q
EDGE_SCALARS = [0, 1, 2, 15, 16, 17, 31, 32, 33, Q - 1, Q, Q + 1, 2**255 - 1, 2**250, 2**250 - 1, 2**250 - lem.OFFSET5,
                2**250 - lem.OFFSET5 - 1, lem.OFFSET5, 2**255 - lem.OFFSET5, int("7" + "8" * 63, 16)]


@pytest.mark.parametrize("o", sorted(tp.ALL_POINTS))
def test_exact_order(o, oracle):
    t = tp.ALL_POINTS[o]
    assert m.on_curve(t) and oracle.on_curve(t)
    assert m.pt_mul(o, t) is None
    primes = tp.PRIME_FACTORS[o]
    prod = 1
    for p in primes:
        prod *= p
        assert m.pt_mul(o // p, t) is not None, p
    assert prod == o
    assert not m.is_torsion_free(t) and not oracle.is_torsion_free(t)
    assert (m.Q * m.COFACTOR) % o == 0
    if o >= 29:     # no identity among 1T..16T: the affine table builder takes the key; and the table has opposite entries
        assert all(m.pt_mul(i, t) is not None for i in range(1, 17))
    if o == 29:
        assert m.pt_mul(16, t) == m.pt_neg(m.pt_mul(13, t)) and m.pt_mul(15, t) == m.pt_neg(m.pt_mul(14, t))


@pytest.mark.parametrize("o", sorted(tp.ALL_POINTS))
def test_oracle_point_mul_agrees_with_the_model(o, oracle):
    t = tp.ALL_POINTS[o]
    rng = random.Random(o)
    acc = None
    for k in range(o + 1):                                   # acc = [k]T by repeated addition
        assert oracle.point_mul(k, t) == acc, k
        if k in (0, 1, 2, o // 2, o - 1, o):
            assert m.pt_mul(k, t) == acc, k
        acc = m.pt_add(acc, t)
    for k in [Q, Q - 1, 2**255 - 1] + [rng.getrandbits(255) for _ in range(5)]:
        assert oracle.point_mul(k, t) == m.pt_mul(k, t) == m.pt_mul(k % o, t)


def test_derivation_script_reproduces_the_literals():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "golden", "make_torsion_points.py")],
                         check=True, capture_output=True, text=True).stdout
    ns = {}
    exec(out, ns)
    assert ns["POINTS"] == tp.POINTS


# ---------------------------------------------------------------- the event model
def test_digits_recompose_the_scalar():
    rng = random.Random(1)
    ks = EDGE_SCALARS + [rng.getrandbits(255) for _ in range(500)] + [rng.getrandbits(b) for b in range(1, 255, 7)]
    for k in ks:
        top, digits = lem.recode(k)
        assert 0 <= top <= 32 and len(digits) == 50 and all(-16 <= d <= 15 for d in digits)
        assert lem.recompose(top, digits) == k and lem.scalar_of(top, digits) == k
        if k < Q:
            assert top <= 31
    assert lem.recode(2**255 - 1)[0] == 32
    assert lem.qnaf_value() == Q
    digits, gaps = lem.qnaf()
    assert len(digits) == 44 and sum(gaps) == 255 and all(d % 2 and abs(d) <= 15 for d in digits)


_SUMS = {}


def _add(a, b):
    """pymodel.pt_add, each distinct pair of operands computed once (the walks of one key repeat their doublings)"""
    if (a, b) not in _SUMS:
        _SUMS[a, b] = m.pt_add(a, b)
    return _SUMS[a, b]


def _textbook(top, schedule, table):
    """the ladder as written: entry or 16P + (top - 16)P, then `gap` doublings and one addition per window"""
    acc = None
    if top:
        acc = table[min(top, 16)]
        if top > 16:
            acc = _add(acc, table[top - 16])
    out = [acc]
    for d, gap in schedule:
        for _ in range(gap):
            acc = _add(acc, acc)
        if d:
            e = table[abs(d)]
            acc = _add(acc, m.pt_neg(e) if d < 0 else e)
        out.append(acc)
    return out


def _check_walk(w, o, multiples, table):
    """the model's accumulators are the textbook ladder's, and every class is what the points say"""
    pts = _textbook(w.top, [(s.digit, s.gap) for s in w.steps], table)
    assert pts[0] == multiples[w.top_m]
    if w.top > 16:
        a, b = table[16], table[w.top - 16]
        want = (lem.IDENTITY_ENTRY if b is None else lem.FROM_IDENTITY if a is None else lem.EQUAL if a == b else
                lem.OPPOSITE if a == m.pt_neg(b) else lem.GENERIC)
        assert w.top_cls == want
    for it, s in enumerate(w.steps):
        assert pts[it] == multiples[s.m_in] and pts[it + 1] == multiples[s.m_out], it
        acc = multiples[(s.m_in << s.gap) % o]
        if s.digit == 0:
            want = lem.ZERO
        else:
            e = table[abs(s.digit)]
            e = m.pt_neg(e) if s.digit < 0 else e
            want = (lem.IDENTITY_ENTRY if e is None else lem.FROM_IDENTITY if acc is None else lem.EQUAL if acc == e else
                    lem.OPPOSITE if acc == m.pt_neg(e) else lem.GENERIC)
        assert s.cls == want, (it, s)


@pytest.mark.parametrize("o", sorted(tp.ALL_POINTS))
def test_model_follows_the_textbook_ladder(o):
    _SUMS.clear()
    t = tp.ALL_POINTS[o]
    multiples = [None]
    for _ in range(o - 1):
        multiples.append(m.pt_add(multiples[-1], t))
    table = [multiples[i % o] for i in range(17)]
    rng = random.Random(100 + o)
    ks = EDGE_SCALARS + [o, o - 1, o + 1] + [rng.getrandbits(255) for _ in range(200 - len(EDGE_SCALARS) - 3)]
    assert len(ks) == 200
    seen = set()
    for k in ks:
        w = lem.walk(k, o)
        _check_walk(w, o, multiples, table)
        assert multiples[w.steps[-1].m_out] == multiples[k % o]
        seen.update(cls for _, cls in lem.events(w))
    assert m.pt_mul(ks[-1], t) == multiples[ks[-1] % o] and m.pt_mul(Q, t) == multiples[Q % o]
    if o != 2:                                          # (order 2: every window starts from the identity)
        assert seen == set(lem.EVENTS)                  # 200 scalars meet every kind of collision
    wq = lem.walk_q(o)                                  # the subgroup check's schedule
    _check_walk(wq, o, multiples, table)
    assert multiples[wq.steps[-1].m_out] == multiples[Q % o] and Q % o != 0


def test_engineered_scalars_meet_their_event():
    rng = random.Random(7)
    for o in tp.ORDERS:
        for cls in lem.EVENTS:
            for at in (0, 1, 24, 48, 49):
                k = lem.scalar_with_event(o, cls, at, rng)
                assert lem.walk(k, o).steps[at].cls == cls
        k = lem.scalar_with_event(o, lem.EQUAL, "top", rng)
        assert lem.recode(k)[0] == 32 and lem.walk(k, o).top_cls == lem.EQUAL
    k = lem.scalar_with_event(29, lem.OPPOSITE, "top", rng)
    w = lem.walk(k, 29)
    assert w.top == 29 and w.top_cls == lem.OPPOSITE and w.top_m == 0
    with pytest.raises(ValueError):
        lem.scalar_with_event(58, lem.OPPOSITE, "top", rng)
    # an honest key: nothing ever happens unless the top digit is zero
    assert lem.event_free(Q - 1) and lem.event_free(2**250) and not lem.event_free(5) and not lem.event_free(0)


def test_subgroup_check_meets_collisions_at_order_29_and_58():
    """[q]T for T of order 29 runs into its own opposite twice (and resumes from the identity): the subgroup check of a
    hostile key depends on the exceptional exits of the window statement as well"""
    assert [c for _, c in lem.events(lem.walk_q(29))] == [lem.OPPOSITE, lem.FROM_IDENTITY] * 2
    assert [c for _, c in lem.events(lem.walk_q(58))] == [lem.FROM_IDENTITY] * 2


# ---------------------------------------------------------------- the device headers compiled for the host
from test_host_arith import ha, arr, p_, _pt, _unpt    # noqa: E402,F401  (ha is that module's fixture)


@pytest.mark.parametrize("o", tp.ORDERS)
def test_host_compiled_table_and_ladder_on_torsion_keys(ha, oracle, o):
    """build_ptab and mul_ptab as the kernels compile them, on the host (the compiled additions, not the generated
    statements): a key of order >= 29 goes through the affine table builder -- none of its denominators vanishes --, the
    table it leaves is 1T..16T limb for limb with the stored opposites, and the ladder is exact on scalars that meet
    every class of collision at the first, a middle and the last window and at the top digit"""
    rnd = random.Random(o)
    t = tp.POINTS[o]
    ks = [lem.scalar_with_event(o, cls, at, rnd) for cls in lem.EVENTS for at in (0, 25, 49)]
    ks += [lem.scalar_with_event(o, lem.EQUAL, "top", rnd), 0, o, o - 1, o + 1, Q, Q - 1, 2**255 - 1]
    if o <= 32:
        ks.append(lem.scalar_with_event(o, lem.OPPOSITE, "top", rnd))
    ks += [rnd.getrandbits(255) for _ in range(8)]
    tab = np.zeros(ha.ha_ptab_words(), np.uint64)
    pv, pi = _pt(t)
    for k in ks:
        out = np.zeros(12, np.uint64)
        inf = ha.ha_mul_ptab(p_(arr([(k >> (64 * i)) & (2**64 - 1) for i in range(4)])), p_(pv), pi, p_(tab), p_(out))
        assert _unpt(out, inf) == oracle.point_mul(k, t) == m.pt_mul(k % o, t), k
    rows = tab.reshape(16, 32)
    for i in range(1, 17):
        x, y = m.pt_mul(i, t)
        assert tuple(int(v) for v in rows[i - 1, 0:6]) == x and tuple(int(v) for v in rows[i - 1, 6:12]) == y, i
        assert tuple(int(v) for v in rows[i - 1, 16:22]) == x and tuple(int(v) for v in rows[i - 1, 22:28]) == m.f6_neg(y), i
    if o == 29:
        assert (rows[15, 0:6] == rows[12, 0:6]).all() and (rows[15, 6:12] == rows[12, 22:28]).all()     # 16T = -13T
