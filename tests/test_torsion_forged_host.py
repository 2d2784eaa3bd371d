"""tests/golden/torsion_forged.json (made by tests/golden/make_torsion_forged.py) on the CPU: every record is a forged
acceptance under a key outside the prime subgroup, the event lists are the model's, and the set as a whole meets the
conditions that make the GPU tests of tests/test_gpu_torsion_ladder.py prove something."""
import collections

import numpy as np
import pytest

import ladder_event_model as lem
import pymodel as m
import torsion_fixture as tf
import torsion_points as tp

COUNTS = {29: 8, 5: 4, 10: 4, 58: 4, 145: 4, 181: 4, 290: 2}


@pytest.fixture(scope="module")
def records():
    return tf.load()


def test_counts_and_layout(records):
    assert collections.Counter(r.order for r in records) == COUNTS
    for r in records:
        assert len(r.sig) == 81 and len(r.pk) == 96 and len(r.msg) == tf.MSG_LEN
        assert r.pk == tp.pk96(r.order)
        assert int.from_bytes(r.sig[49:], "little") == r.e and 0 < r.e < m.Q - 1
        assert r.h % r.order == r.c and r.c != 0
        assert len({(x.sig, x.msg) for x in records}) == len(records)


def test_events_are_the_models(records):
    for r in records:
        t = tp.ALL_POINTS[r.order]
        x = m.fp6_from_bytes48(r.sig[:48])
        assert m.scalar_from_digest(m.hash_message(x, t, r.msg)) == r.h
        assert r.events == lem.events(lem.walk(r.h, r.order))
        # R is the point the record says, flag byte included
        rp = m.pt_add(m.pt_mul(r.e, m.default_params().generator()), m.pt_mul(r.c, t))
        assert m.pt_compress(rp) == r.sig[:49]


def test_fixture_conditions(records):
    """conditions on the fixture, not measurements (the fixture script chooses its candidates to meet them)"""
    big = [r for r in records if r.order >= 29]
    for cls in lem.EVENTS:
        for reg in ("first", "middle", "last"):
            assert any(c == cls and at != "top" and lem.region(at) == reg for r in big for at, c in r.events), (cls, reg)
    assert any(at == "top" for r in big for at, _ in r.events)
    top = [r for r in big if r.events[0][0] == "top"]
    assert any(r.order == 29 and lem.recode(r.h)[0] == 29 and r.events[0][1] == lem.OPPOSITE for r in top)
    for r in records:
        assert any(at != "top" for at, _ in r.events), r.order
    # an identity accumulator at a piece boundary of both end-game plans of the GPU test (pass 1 = the ladder of [h]P)
    import schnorr_sig_amd as ssa
    for pieces, gens in tf.TAIL_CONFIGS:
        n = tf.tail_batch(gens)
        for torsion in (False, True):
            plan = ssa.debug_tail_plan(tf.TAIL_WAVES, n, check_torsion=torsion, pieces=pieces, gens=gens)
            cuts = tf.ladder_cuts(plan)
            assert cuts, plan
            assert tf.parked_identity_records(records, cuts), (pieces, gens, torsion, cuts)


def test_records_verify_with_the_model_and_the_oracle(records, oracle):
    sigs, pks, msgs = tf.arrays(records)
    twins = tf.twins(sigs)
    assert (oracle.verify_many(sigs, pks, msgs, check_torsion=False) == 0).all()
    assert (oracle.verify_many(sigs, pks, msgs, check_torsion=False, sig_flag_byte=True) == 0).all()
    assert (oracle.verify_many(sigs, pks, msgs, check_torsion=True) == 1).all()
    assert (oracle.verify_many(twins, pks, msgs, check_torsion=False) == 2).all()
    assert (oracle.verify_many(twins, pks, msgs, check_torsion=False, sig_flag_byte=True) == 2).all()
    assert (oracle.verify_many(twins, pks, msgs, check_torsion=True) == 1).all()
    assert (oracle.verify_many_fast(sigs, pks, msgs, check_torsion=False) == 0).all()
    for i, r in enumerate(records):
        t = tp.ALL_POINTS[r.order]
        assert m.verify(r.sig, t, r.msg, check_torsion=False) == m.OK
        assert m.verify(r.sig, t, r.msg, check_torsion=True) == m.INVALID_PUBLIC_KEY
        assert m.verify(twins[i].tobytes(), t, r.msg, check_torsion=False) == m.INVALID_SIGNATURE
        assert (np.frombuffer(r.sig, np.uint8) != twins[i]).sum() == 1


def _generic_madd(p, q):
    """the mixed addition's generic formulas and nothing else: no test for Z = 0, for an identity entry, for H = 0"""
    X, Y, Z = p
    zz = m.f6_sqr(Z)
    H = m.f6_sub(m.f6_mul(q[0], zz), X)
    R = m.f6_sub(m.f6_mul(m.f6_mul(q[1], Z), zz), Y)
    hh = m.f6_sqr(H)
    hhh, v = m.f6_mul(H, hh), m.f6_mul(X, hh)
    x3 = m.f6_sub(m.f6_sub(m.f6_sqr(R), hhh), m.f6_scale(v, 2))
    return x3, m.f6_sub(m.f6_mul(R, m.f6_sub(v, x3)), m.f6_mul(Y, hhh)), m.f6_mul(Z, H)


def _jac_dbl(p):
    X, Y, Z = p
    xx, yy, zz = m.f6_sqr(X), m.f6_sqr(Y), m.f6_sqr(Z)
    s = m.f6_scale(m.f6_mul(X, yy), 4)
    mm = m.f6_add(m.f6_scale(xx, 3), m.f6_sqr(zz))
    x3 = m.f6_sub(m.f6_sqr(mm), m.f6_scale(s, 2))
    return x3, m.f6_sub(m.f6_mul(mm, m.f6_sub(s, x3)), m.f6_scale(m.f6_sqr(yy), 8)), m.f6_scale(m.f6_mul(Y, Z), 2)


def _ladder(h, t, madd):
    """the schedule of the model over Jacobian points with the given mixed addition -> affine point or None"""
    table = [None] + [m.pt_mul(i, t) for i in range(1, 17)]
    top, digits = lem.recode(h)
    acc = (m.F6_ONE, m.F6_ONE, m.F6_ZERO)
    if top:
        e = table[min(top, 16)]
        acc = (e[0], e[1], m.F6_ONE)
        if top > 16:
            acc = madd(acc, table[top - 16])
    for it in range(lem.WINDOWS):
        for _ in range(5):
            acc = _jac_dbl(acc)
        d = digits[lem.WINDOWS - 1 - it]
        if d:
            e = table[abs(d)]
            acc = madd(acc, m.pt_neg(e) if d < 0 else e)
    if acc[2] == m.F6_ZERO:
        return None
    zi = m.f6_inv(acc[2])
    zi2 = m.f6_sqr(zi)
    return m.f6_mul(acc[0], zi2), m.f6_mul(acc[1], m.f6_mul(zi2, zi))


def _exact_madd(p, q):
    """jac_madd of csrc/curve.hpp: the generic formulas behind the three exits"""
    if p[2] == m.F6_ZERO:
        return q[0], q[1], m.F6_ONE
    r = _generic_madd(p, q)
    if r[2] == m.F6_ZERO:                                     # H = 0
        zz = m.f6_sqr(p[2])
        if m.f6_mul(m.f6_mul(q[1], p[2]), zz) == p[1]:        # R = 0 as well: the same point
            return _jac_dbl(p)
    return r


def test_a_ladder_without_the_exceptional_exits_loses_every_record(records):
    """what the records are for: the schedule of the kernels over Jacobian points gives [h]T with the exact mixed addition
    and a different point, for EVERY record of order >= 29, once the addition is the generic formulas alone -- so a lane
    that is accepted on the GPU has taken the exits.  (The keys of order 5 and 10 need the identity-entry exit too.)"""
    for r in records:
        if r.order < 29:
            continue
        t = tp.ALL_POINTS[r.order]
        want = m.pt_mul(r.c, t)
        assert _ladder(r.h, t, _exact_madd) == want
        assert _ladder(r.h, t, _generic_madd) != want, r.order
