"""The collision paths of the per-lane ladder on keys of order 29 .. 362 (tests/torsion_points.py), on the GPU.

A key outside the prime subgroup whose order is at least 29 goes through the affine table builder like an honest key,
and its ladder then meets what an honest ladder never meets: an accumulator equal to the table entry it adds, opposite
to it, or the identity (tests/ladder_event_model.py says at which window).  Under verify_batch semantics -- no subgroup
check -- the result must still be exact.  Every comparison here is exact (bytes, limbs, statuses) against the C oracle.

The wave layout decides whether a test proves anything (tests/torsion_fixture.py): every batch holds its special lanes
twice, SOLITARY -- one per wave, at lane 0, 31, 32 or 63, among honest lanes whose ladders meet nothing -- and as a
CROWD of special lanes in the same wave.

The forged records of tests/golden/torsion_forged.json are the only inputs of the suite that are ACCEPTED after the
ladder went through a collision; tests/test_torsion_forged_host.py proves them on the CPU."""
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ladder_event_model as lem     # noqa: E402
import torsion_fixture as tf         # noqa: E402
import torsion_points as tp          # noqa: E402

pytestmark = pytest.mark.gpu

Q = lem.Q
FLAGS = [(torsion, fb) for torsion in (False, True) for fb in (False, True)]
N_HONEST = 252                        # four waves' worth of filler, cycled


def _make_scalars(rng, n):
    s = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    s[:, 31] &= 0x3F
    s[:, 0] |= 1
    return s


def _h_of(engine, sigs, pks, msgs):
    import pymodel as m
    dig = engine.hash_message_many(sigs, pks, msgs)
    return [m.scalar_from_digest(d.tobytes()) for d in dig]


class Lanes:
    """the special lanes (forged records, then their twins), the honest pool, and the oracle's status of each under
    every flag combination -- computed once, never changed"""

    def __init__(self, engine, oracle):
        self.records = tf.load()
        sigs, pks, msgs = tf.arrays(self.records)
        self.n_rec = len(self.records)
        self.sigs = np.concatenate([sigs, tf.twins(sigs)])
        self.pks = np.concatenate([pks, pks])
        self.msgs = np.concatenate([msgs, msgs])
        self.order = np.array([r.order for r in self.records] * 2)
        rng = np.random.default_rng(0x7029)
        n = 2 * N_HONEST
        sks, nonces = _make_scalars(rng, n), _make_scalars(rng, n)
        hm = rng.integers(0, 256, size=(n, tf.MSG_LEN), dtype=np.uint8)
        hp, hs = oracle.keygen_sign_many(sks, nonces, hm)
        # honest lanes whose ladder meets nothing: the top digit of h is not zero (one lane in about 31 is dropped)
        keep = np.array([lem.event_free(h) for h in _h_of(engine, hs, hp, hm)])
        assert keep.sum() >= N_HONEST
        keep = np.flatnonzero(keep)[:N_HONEST]
        self.h_sigs, self.h_pks, self.h_msgs = hs[keep], hp[keep], hm[keep]
        self.want, self.h_want = {}, {}
        for torsion, fb in FLAGS:
            self.want[torsion, fb] = oracle.verify_many(self.sigs, self.pks, self.msgs, check_torsion=torsion,
                                                        sig_flag_byte=fb)
            self.h_want[torsion, fb] = oracle.verify_many(self.h_sigs, self.h_pks, self.h_msgs, check_torsion=torsion,
                                                          sig_flag_byte=fb)
            assert not self.h_want[torsion, fb].any()
            # forged lanes: exactly 0 without the subgroup check and 1 with it; their twins 2 or 1
            assert (self.want[torsion, fb][:self.n_rec] == (1 if torsion else 0)).all()
            assert (self.want[torsion, fb][self.n_rec:] == (1 if torsion else 2)).all()

    def batch(self, pick=None):
        """the two layouts over the special lanes `pick` (default: all) -> dict of the batch and what it must answer"""
        pick = np.arange(len(self.sigs)) if pick is None else np.asarray(pick)
        special, honest = tf.layouts(len(pick), N_HONEST)
        b = {"special": special, "pick": pick,
             "sigs": tf.lay_out(self.sigs[pick], self.h_sigs, special, honest),
             "pks": tf.lay_out(self.pks[pick], self.h_pks, special, honest),
             "msgs": tf.lay_out(self.msgs[pick], self.h_msgs, special, honest)}
        b["want"] = {f: tf.lay_out(self.want[f][pick], self.h_want[f], special, honest) for f in FLAGS}
        return b


_STATE = {}


@pytest.fixture(scope="module")
def lanes(engine, oracle):
    if "lanes" not in _STATE:
        _STATE["lanes"] = Lanes(engine, oracle)
    return _STATE["lanes"]


def _assert_status(got, nf, want, what):
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (what, bad[:10], got[bad[:10]], want[bad[:10]])
    assert nf == int((want != 0).sum()), what


def test_layouts_are_what_they_claim(lanes):
    """the test of the layouts: every special lane stands once alone in a wave of event-free honest lanes, at the four
    places in turn, and once in a wave of special lanes only"""
    b = lanes.batch()
    sp = b["special"].reshape(-1, tf.WAVE)
    n = len(b["pick"])
    for i in range(n):
        assert (sp[i] >= 0).sum() == 1 and sp[i, tf.SOLITARY_PLACES[i % 4]] == i
    assert (sp[n:] >= 0).all() and set(sp[n:].ravel()) == set(range(n))
    assert {tf.SOLITARY_PLACES[i % 4] for i in range(n) if lanes.order[i] == 29} == set(tf.SOLITARY_PLACES)


# ---------------------------------------------------------------- a. mul_ptab alone
def _mul_cases():
    """(scalar, order) rows chosen by the model, for every order >= 29"""
    rnd = random.Random(0x3A)
    rows = []
    for o in tp.ORDERS:
        ks = []
        for cls in lem.EVENTS:
            for at in (0, 25, 49):
                k = lem.scalar_with_event(o, cls, at, rnd)
                assert lem.walk(k, o).steps[at].cls == cls
                ks.append(k)
        ks.append(lem.scalar_with_event(o, lem.EQUAL, "top", rnd))          # top = 32: 16P + 16P
        if o <= 32:
            ks.append(lem.scalar_with_event(o, lem.OPPOSITE, "top", rnd))   # top = o:  16P + (o - 16)P = O
        top0 = rnd.getrandbits(249)                                          # top = 0: the ladder starts from the identity
        assert lem.recode(top0)[0] == 0
        ks += [top0, 0, o, o - 1, o + 1, Q, Q - 1, 2**255 - 1]
        ks += [rnd.getrandbits(255) for _ in range(32)]
        rows += [(k, o) for k in ks]
    return rows


def test_mul_ptab_on_torsion_keys(engine, oracle):
    """[k]T through the production table and ladder (debug op 4) against the oracle's point, for scalars that meet every
    class of collision at the first, a middle and the last window, the top-digit collisions, the edge scalars and random
    ones.  The honest filler lanes are checked as well: in a solitary wave they run the compiled addition behind the
    special lane's exit, on a point the statement has already doubled."""
    import pymodel as m
    rows = _mul_cases()
    assert 250 <= len(rows) <= 400
    seen = set()
    for k, o in rows:
        w = lem.walk(k, o)
        seen.update((o, cls, "top" if at == "top" else lem.region(at)) for at, cls in lem.events(w))
    for o in tp.ORDERS:
        for cls in lem.EVENTS:
            assert {(o, cls, r) for r in ("first", "middle", "last")} <= seen
        assert (o, lem.EQUAL, "top") in seen
    assert (29, lem.OPPOSITE, "top") in seen
    # honest filler: [k]([j]G) with event-free k
    rnd = random.Random(0x3B)
    g = m.default_params().generator()
    hpts = [oracle.point_mul(rnd.getrandbits(200) | 1, g) for _ in range(12)]
    hrows = []
    while len(hrows) < N_HONEST:
        k = rnd.getrandbits(255)
        if lem.event_free(k):
            hrows.append((k, hpts[len(hrows) % len(hpts)]))
    want_special = [oracle.point_mul(k, tp.POINTS[o]) for k, o in rows]
    for (k, o), w in zip(rows, want_special):
        assert (w is None) == (k % o == 0)
    want_honest = [oracle.point_mul(k, p) for k, p in hrows]

    def encode(pairs):
        a = np.zeros((len(pairs), 4), dtype=np.uint64)
        b = np.zeros((len(pairs), 13), dtype=np.uint64)
        for i, (k, p) in enumerate(pairs):
            a[i] = np.frombuffer(int(k).to_bytes(32, "little"), dtype=np.uint64)
            b[i, :6], b[i, 6:12] = p[0], p[1]
        return a, b

    def expect(points):
        e = np.zeros((len(points), 13), dtype=np.uint64)
        for i, p in enumerate(points):
            if p is None:
                e[i, 12] = 1
            else:
                e[i, :6], e[i, 6:12] = p[0], p[1]
        return e

    sa, sb = encode([(k, tp.POINTS[o]) for k, o in rows])
    ha, hb = encode(hrows)
    special, honest = tf.layouts(len(rows), N_HONEST)
    a, b = tf.lay_out(sa, ha, special, honest), tf.lay_out(sb, hb, special, honest)
    want = tf.lay_out(expect(want_special), expect(want_honest), special, honest)
    got = engine.debug_arith(4, a, b, 13)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, [(int(i), int(special[i]), rows[special[i]] if special[i] >= 0 else "honest") for i in bad[:8]]


# ---------------------------------------------------------------- b. per-lane verification
@pytest.mark.parametrize("mode", ["lane", "coop"])
def test_forged_acceptances_per_lane(engine, lanes, mode):
    """the forged records, their twins and honest filler through both kernel families, subgroup check and flag byte on
    and off: the oracle's status vector, with the forged lanes at exactly 0 (1 with the check)"""
    b = lanes.batch()
    for torsion, fb in FLAGS:
        got, nf = engine.verify_many(b["sigs"], b["pks"], b["msgs"], check_torsion=torsion, mode=mode, sig_flag_byte=fb)
        _assert_status(got, nf, b["want"][torsion, fb], (mode, torsion, fb))
        forged = (b["special"] >= 0) & (b["special"] < lanes.n_rec)
        assert (got[forged] == (1 if torsion else 0)).all()
        twin = b["special"] >= lanes.n_rec
        assert (got[twin] == (1 if torsion else 2)).all()
        assert (got[b["special"] < 0] == 0).all()


# ---------------------------------------------------------------- c. the end game
def _tail_engine(pieces, gens, reversed_grid):
    import schnorr_sig_amd as ssa
    env = {"SSA_TAIL_WAVES": str(tf.TAIL_WAVES), "SSA_TAIL_PIECES": str(pieces), "SSA_TAIL_GENS": str(gens),
           "SSA_TAIL_UNIFORM": "0", "SSA_TAIL_REVERSED": "1" if reversed_grid else "0"}
    os.environ.update(env)
    try:
        return ssa.Engine(0)
    finally:
        for k in env:
            del os.environ[k]


@pytest.mark.parametrize("pieces,gens,reversed_grid", [(8, 1, False), (5, 2, True)])
def test_end_game_parks_and_resumes_collisions(engine, lanes, pieces, gens, reversed_grid):
    """the forged records of order 29 and 58 (and their twins) INSIDE the tail groups of a launch whose last generation
    runs in pieces: the accumulator is parked between windows, and for some records it is parked as the identity (Z = 0)
    and resumed -- the model names them.  The result is the plain engine's and the oracle's."""
    import schnorr_sig_amd as ssa
    assert (pieces, gens) in tf.TAIL_CONFIGS
    n = tf.tail_batch(gens)
    pick = np.flatnonzero(np.isin(lanes.order, (29, 58)))
    for torsion in (False, True):
        plan = ssa.debug_tail_plan(tf.TAIL_WAVES, n, check_torsion=torsion, pieces=pieces, gens=gens)
        assert plan["n_pieces"] >= 2
        parked = tf.parked_identity_records(lanes.records, tf.ladder_cuts(plan))
        assert parked and set(parked) <= set(pick.tolist())
    part = lanes.batch(pick)                                # solitary waves, then the crowd
    m = len(part["special"])
    assert m % tf.WAVE == 0 and m <= gens * tf.TAIL_WAVES * tf.WAVE
    # the tail groups hold the lanes from 256 * main_blocks on: the layouts start one wave into them
    assert plan["main_blocks"] == ssa.debug_tail_plan(tf.TAIL_WAVES, n, pieces=pieces, gens=gens)["main_blocks"]
    at = plan["main_blocks"] * 256 + tf.WAVE
    assert at + m <= n
    idx = np.arange(n) % N_HONEST
    sigs, pks, msgs = lanes.h_sigs[idx].copy(), lanes.h_pks[idx].copy(), lanes.h_msgs[idx].copy()
    sigs[at:at + m], pks[at:at + m], msgs[at:at + m] = part["sigs"], part["pks"], part["msgs"]
    eng = _tail_engine(pieces, gens, reversed_grid)
    try:
        for torsion, fb in FLAGS:
            want = np.zeros(n, dtype=np.uint8)
            want[at:at + m] = part["want"][torsion, fb]
            got, nf = eng.verify_many(sigs, pks, msgs, check_torsion=torsion, mode="lane", sig_flag_byte=fb)
            _assert_status(got, nf, want, ("tail", torsion, fb))
            ref, nf_ref = engine.verify_many(sigs, pks, msgs, check_torsion=torsion, mode="lane", sig_flag_byte=fb)
            _assert_status(ref, nf_ref, want, ("plain", torsion, fb))
    finally:
        eng.close()


# ---------------------------------------------------------------- d. keyed kernels
KEYSET_ORDERS = (29, 58, 181, 10)


@pytest.mark.parametrize("kind", ["ladder", "comb"])
def test_key_sets_with_torsion_keys(engine, oracle, lanes, kind):
    """a key set of four honest keys and T29, T58, T181, T10: status, self-check (plain and deep), the forged records
    through verify_many_indexed against the oracle, and for the ladder tables the sixteen multiples of T29 limb for limb"""
    import pymodel as m
    import schnorr_sig_amd as ssa
    rng = np.random.default_rng(0x7D)
    hsk = _make_scalars(rng, 4)
    n = 2 * N_HONEST                                        # honest filler by four signers, event-free lanes only
    hm = rng.integers(0, 256, size=(n, tf.MSG_LEN), dtype=np.uint8)
    hidx = (np.arange(n) % 4).astype(np.uint32)
    hp, hs = oracle.keygen_sign_many(hsk[hidx], _make_scalars(rng, n), hm)
    keep = np.flatnonzero([lem.event_free(h) for h in _h_of(engine, hs, hp, hm)])[:N_HONEST]
    assert len(keep) == N_HONEST
    hs, hm, hidx = hs[keep], hm[keep], hidx[keep]
    keys = np.concatenate([hp[:4], np.stack([np.frombuffer(tp.pk96(o), np.uint8) for o in KEYSET_ORDERS])])
    ks = engine.keyset_create(keys, kind=kind)
    try:
        assert list(engine.keyset_status(ks)) == [0, 0, 0, 0, 1, 1, 1, 1]
        for deep in (False, True):
            res = ks.selfcheck(deep=deep)
            assert res["ok"] and res["keys_checked"] == 8 and res["keys_bad"] == 0 and not res["bad"].any(), res
        pick = np.flatnonzero(np.isin(lanes.order, KEYSET_ORDERS))
        special, honest = tf.layouts(len(pick), N_HONEST)
        sigs = tf.lay_out(lanes.sigs[pick], hs, special, honest)
        msgs = tf.lay_out(lanes.msgs[pick], hm, special, honest)
        sidx = np.array([4 + KEYSET_ORDERS.index(o) for o in lanes.order[pick]], dtype=np.uint32)
        key_idx = tf.lay_out(sidx, hidx, special, honest)
        zeros = np.zeros(N_HONEST, dtype=np.uint8)
        assert not oracle.verify_many(hs, keys[hidx], hm, check_torsion=True, sig_flag_byte=True).any()
        for torsion, fb in FLAGS:
            want = tf.lay_out(lanes.want[torsion, fb][pick], zeros, special, honest)
            got, nf = engine.verify_many_indexed(ks, key_idx, sigs, msgs, check_torsion=torsion, sig_flag_byte=fb)
            _assert_status(got, nf, want, (kind, torsion, fb))
            assert (got[(special >= 0) & (pick[special] < lanes.n_rec)] == (1 if torsion else 0)).all()
        if kind == "ladder":
            t = tp.POINTS[29]
            tab = ks.debug_keytab_read(ssa.KEYTAB_LADDER, 4).reshape(16, 32)
            for i in range(1, 17):
                x, y = m.pt_mul(i, t)
                assert tuple(int(v) for v in tab[i - 1, 0:6]) == x and tuple(int(v) for v in tab[i - 1, 6:12]) == y, i
                assert tuple(int(v) for v in tab[i - 1, 16:22]) == x, i
                assert tuple(int(v) for v in tab[i - 1, 22:28]) == m.f6_neg(y), i
            assert (tab[15, 0:6] == tab[12, 0:6]).all() and (tab[15, 6:12] == tab[12, 22:28]).all()     # 16T = -13T
    finally:
        ks.close()


# ---------------------------------------------------------------- e. the callers in front of the exact kernel
def test_callers_in_front_of_the_exact_kernel(engine, oracle, lanes):
    """dedup, screening and the key caches hand their doubtful lanes to the exact keyed kernel: the same batch through
    each of them gives the oracle's statuses, the forged lanes at 0 (1 with the subgroup check)"""
    b = lanes.batch()
    sigs, pks, msgs = b["sigs"], b["pks"], b["msgs"]
    forged = (b["special"] >= 0) & (b["special"] < lanes.n_rec)

    def check(got, nf, torsion, fb, what):
        _assert_status(got, nf, b["want"][torsion, fb], what)
        assert (got[forged] == (1 if torsion else 0)).all(), what

    for torsion in (False, True):
        got, nf, _ = engine.verify_many_dedup(sigs, pks, msgs, check_torsion=torsion)
        check(got, nf, torsion, False, ("dedup", torsion))
        got, nf, _ = engine.verify_many_screened(sigs, pks, msgs, check_torsion=torsion)
        check(got, nf, torsion, False, ("screened", torsion))
    got, nf = engine.verify_batch_screened(sigs, pks, msgs)
    check(got, nf, False, True, "batch screened")
    cache = engine.keycache_create(1024)
    try:
        for state in ("cold", "warm"):
            for torsion in (False, True):
                got, nf, _ = engine.verify_many_cached(cache, sigs, pks, msgs, check_torsion=torsion)
                check(got, nf, torsion, False, ("cached", state, torsion))
    finally:
        cache.close()
    # the compressed records: the 49-byte torsion keys decompress on the device
    comp = {}
    for row in np.unique(pks, axis=0):
        comp[row.tobytes()] = np.frombuffer(oracle.compress(row.tobytes()), np.uint8)
    keyed = np.concatenate([np.stack([comp[r.tobytes()] for r in pks]), sigs], axis=1)
    wire = engine.keycache_create(1024, wire=True)
    try:
        for state in ("cold", "warm"):
            for torsion in (False, True):
                got, nf, _ = engine.verify_keyed_many_cached(wire, keyed, msgs, check_torsion=torsion)
                check(got, nf, torsion, False, ("keyed cached", state, torsion))
    finally:
        wire.close()


# ---------------------------------------------------------------- f. the MSM verdict
def test_msm_verdict_with_torsion_lanes(engine, oracle, lanes):
    """256 lanes: honest ones, every forged record, the order-29 records four times over so that 32 lanes share T29.
    The batch equation multiplies a key by s h mod q, which for a key outside the subgroup is [s h]P only while
    s h < q: with the coefficient 1 on the torsion lanes every lane's equation holds exactly and the verdict is an
    accept; with random coefficients it is whatever the oracle's verify_batch says for them (a reject).  One twin
    swapped in must reject under either."""
    n = 256
    spec = list(range(lanes.n_rec)) + [i for i in range(lanes.n_rec) if lanes.order[i] == 29] * 3
    assert sum(lanes.order[i] == 29 for i in spec) == 32
    rng = np.random.default_rng(0xF5)
    place = np.sort(rng.permutation(n)[:len(spec)])
    idx = np.arange(n) % N_HONEST
    sigs, pks, msgs = lanes.h_sigs[idx].copy(), lanes.h_pks[idx].copy(), lanes.h_msgs[idx].copy()
    sigs[place], pks[place], msgs[place] = lanes.sigs[spec], lanes.pks[spec], lanes.msgs[spec]
    rand = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    rand[:, 31] &= 0x3F
    ones = rand.copy()
    ones[place] = 0
    ones[place, 0] = 1
    want_ones = oracle.verify_batch_msm(sigs, pks, msgs, ones)
    want_rand = oracle.verify_batch_msm(sigs, pks, msgs, rand)
    assert want_ones == 0 and want_rand == oracle.verify_batch_msm_fast(sigs, pks, msgs, rand)
    assert engine.verify_batch_msm(sigs, pks, msgs, coeffs=ones) == want_ones
    assert engine.verify_batch_msm(sigs, pks, msgs, coeffs=rand) == want_rand
    bad = sigs.copy()
    bad[place[5]] = lanes.sigs[lanes.n_rec + spec[5]]        # the twin of that record
    assert oracle.verify_batch_msm(bad, pks, msgs, ones) == 2
    assert engine.verify_batch_msm(bad, pks, msgs, coeffs=ones) == 2


# ---------------------------------------------------------------- g. the final identity through the comb
def test_result_at_infinity_is_accepted_like_the_oracle(engine, oracle):
    """pk = [k]G, sig.x = 0 and e = -h k: [h]P + [e]G = O, the last addition of the generator's comb meets its opposite,
    and the x of the identity is taken to be 0 -- whatever the oracle answers (an accept; with the flag byte only under
    the identity's encoding 0x80) is the expected status, on the default comb and on a 16-bit one, both kernel families.
    (tests/test_gpu_screened.py meets the identity R through verify_batch_screened only, with random keys.)"""
    import pymodel as m
    import schnorr_sig_amd as ssa
    g = m.default_params().generator()
    msg = b"the result is the identity"[:tf.MSG_LEN]
    sigs, pks = [], []
    for k in (1, 2, 65536, Q - 1):
        pk = m.pt_mul(k, g)
        h = m.scalar_from_digest(m.hash_message(m.F6_ZERO, pk, msg))
        e = (-h * k) % Q
        for flag in (0x80, 0):
            sigs.append(bytes(48) + bytes([flag]) + e.to_bytes(32, "little"))
            pks.append(m.fp6_to_bytes48(pk[0]) + m.fp6_to_bytes48(pk[1]))
    sigs = np.frombuffer(b"".join(sigs), np.uint8).reshape(-1, 81)
    pks = np.frombuffer(b"".join(pks), np.uint8).reshape(-1, 96)
    msgs = np.tile(np.frombuffer(msg, np.uint8), (len(sigs), 1))
    small = ssa.Engine(0, gtab_bits=16)
    try:
        for torsion, fb in FLAGS:
            want = oracle.verify_many(sigs, pks, msgs, check_torsion=torsion, sig_flag_byte=fb)
            assert (want[0::2] == 0).all()                  # the identity's own encoding is accepted
            for eng in (engine, small):
                for mode in ("lane", "coop"):
                    got, nf = eng.verify_many(sigs, pks, msgs, check_torsion=torsion, mode=mode, sig_flag_byte=fb)
                    _assert_status(got, nf, want, (torsion, fb, mode, eng is small))
    finally:
        small.close()
