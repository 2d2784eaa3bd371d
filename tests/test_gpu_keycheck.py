"""Self-check of key-set and key-cache tables (ssa_keyset_selfcheck, ssa_keycache_selfcheck) on
the GPU: clean objects are clean with and without DEEP and their counts add up, a check changes no verification
result, every kind of poke is reported at the poked key, and a repaired cache is a correct cache.

Discipline: after a poke only selfcheck, repair and destroy run on the object.  A poke is an XOR, so the same XOR puts
the word back; where a test goes on using an object it has un-poked it and seen a clean check first."""
import ctypes as C

import numpy as np
import pytest

import schnorr_sig_amd as ssa
from test_gpu_keycache import HITS, INSERTED, CLEARS
from test_gpu_screened_torsion import coeffs32, key_choice, make_scalars

pytestmark = pytest.mark.gpu

NONE = 2 ** 64 - 1
COMB_ROWS = 16 << 16
LADDER, STATUS, KEY, PK_INF, COMB = ssa.KEYTAB_LADDER, ssa.KEYTAB_STATUS, ssa.KEYTAB_KEY, ssa.KEYTAB_PK_INF, ssa.KEYTAB_COMB
ST0, ST1, ST3 = "status0", "status1", "status3"


def point_bytes(pt):
    import pymodel as m
    return np.frombuffer(m.fp6_to_bytes48(pt[0]) + m.fp6_to_bytes48(pt[1]), np.uint8)


def key_material(engine, rng, m, specials=True):
    """m keys: secret scalars (specials: unused), key bytes, pk_inf flags and the status each must get.  With specials,
    from m = 8 on: key 1 is the identity (pk_inf), 2 a non-canonical key, 3 P + T2 (outside the subgroup), 4 the point of
    order 2 itself (a table with sentinel entries), 5 a key off the curve -- the keys of tests/test_gpu_screened_torsion.py."""
    import pymodel as pm
    sks = make_scalars(rng, m)
    pks = engine.pubkey_many(sks).copy()
    inf = np.zeros(m, np.uint8)
    kinds = [ST0] * m
    if specials and m >= 8:
        pks[1] = 0
        inf[1] = 1
        pks[2, 0:8] = 0xFF
        kinds[2] = ST3
        t2 = pm.SMALL_ORDER_POINTS[2]
        p3 = (pm.fp6_from_bytes48(pks[3, :48].tobytes()), pm.fp6_from_bytes48(pks[3, 48:].tobytes()))
        pks[3] = point_bytes(pm.pt_add(p3, t2))
        kinds[3] = ST1
        pks[4] = point_bytes(t2)
        kinds[4] = ST1
        pks[5, 48] ^= 1
        kinds[5] = ST3
    return sks, pks, inf, kinds


def expect_clean(res, kinds, comb=False):
    n0, n1 = kinds.count(ST0), kinds.count(ST1)
    m = len(kinds)
    assert res["ok"], res
    assert res["keys_checked"] == m and res["keys_bad"] == 0 and res["first_bad_key"] == NONE, res
    assert res["ladder_entries_checked"] == 16 * n0, res
    assert res["keys_rebuilt_and_compared"] == n1, res
    assert res["comb_rows_checked"] == (n0 * COMB_ROWS if comb else 0), res
    assert res["combs_skipped"] == (m - n0 if comb else 0), res
    assert res["rows_repaired"] == 0, res
    if "bad" in res:
        assert res["bad"].shape == (m,) and not res["bad"].any()


def expect_one_bad(res, key, m):
    assert not res["ok"], res
    assert res["keys_checked"] == m and res["keys_bad"] == 1 and res["first_bad_key"] == key, res
    if "bad" in res:
        assert list(np.nonzero(res["bad"])[0]) == [key] and res["bad"][key] == 1


def signed_lanes(engine, rng, sks, pks, inf, n):
    """n lanes over the keys: honest signatures under the scalars (lanes of special keys carry a signature that is not
    theirs), and each lane's key bytes and flag for the per-lane entry points"""
    idx = key_choice(rng, n, sks.shape[0]).astype(np.uint32)
    msgs = rng.integers(0, 256, size=(n, 80), dtype=np.uint8)
    _, sigs = engine.keygen_sign_many(sks[idx], make_scalars(rng, n), msgs)
    return idx, sigs, msgs, pks[idx], inf[idx]


def fill_cache(engine, cache, rng, sks, pks, inf, n=None):
    """one cached call that puts every key into the cache -> what is needed to repeat it"""
    n = n or max(4096, 2 * sks.shape[0])
    idx, sigs, msgs, lane_pks, lane_inf = signed_lanes(engine, rng, sks, pks, inf, n)
    co = coeffs32(rng, n)
    st, nf, stats = engine.verify_many_cached(cache, sigs, lane_pks, msgs, coeffs=co, pk_inf=lane_inf)
    return (sigs, lane_pks, msgs, co, lane_inf), st, [int(v) for v in stats]


def cache_rows(cache, pks, inf):
    """cache row of each key (rows are handed out in the order of first appearance: read the stored bytes back)"""
    held = cache.info()["held"]
    stored = {}
    for r in range(held):
        kb = cache.debug_keytab_read(KEY, r).view(np.uint8).tobytes()
        stored[(kb, int(cache.debug_keytab_read(PK_INF, r)[0]) != 0)] = r
    return [stored[(pks[i].tobytes(), bool(inf[i]))] for i in range(pks.shape[0])]


# ---- clean objects ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 1000, 65536])
def test_ladder_key_sets_are_clean(engine, m):
    rng = np.random.default_rng(17100 + m % 1000)
    sks, pks, inf, kinds = key_material(engine, rng, m)
    ks = engine.keyset_create(pks, pk_inf=inf, kind="ladder")
    try:
        status = engine.keyset_status(ks)
        assert [{0: ST0, 1: ST1, 3: ST3}[int(s)] for s in status] == kinds
        ws = None
        for deep in (False, True, False, True):
            expect_clean(ks.selfcheck(deep=deep), kinds)
            if ws is not None:
                assert engine.info()["workspace_bytes"] == ws, "nothing is allocated from the second call on"
            if deep:
                ws = engine.info()["workspace_bytes"]
    finally:
        ks.close()


def test_comb_key_set_is_clean(engine):
    rng = np.random.default_rng(17150)
    sks, pks, inf, kinds = key_material(engine, rng, 2)
    ks = engine.keyset_create(pks, pk_inf=inf, kind="comb")
    try:
        for deep in (False, True):
            expect_clean(ks.selfcheck(deep=deep), kinds, comb=True)
    finally:
        ks.close()


def test_comb_key_set_with_an_identity_key_and_a_key_outside_the_subgroup(engine):
    rng = np.random.default_rng(17151)
    sks, pks, inf, kinds = key_material(engine, rng, 8)
    keep = [0, 1, 3]                              # an honest key, the identity, P + T2
    pks, inf, kinds = pks[keep], inf[keep], [kinds[i] for i in keep]
    ks = engine.keyset_create(pks, pk_inf=inf, kind="comb")
    try:
        for deep in (False, True):
            res = ks.selfcheck(deep=deep)
            expect_clean(res, kinds, comb=True)
            assert res["combs_skipped"] == 1 and res["comb_rows_checked"] == 2 * COMB_ROWS
    finally:
        ks.close()


def test_cache_is_clean_cold_partly_warm_and_after_an_automatic_clear(engine):
    rng = np.random.default_rng(17200)
    u = 400
    sks, pks, inf, kinds = key_material(engine, rng, u + u // 2)
    with engine.keycache_create(640) as cache:
        res = cache.selfcheck()
        assert res == dict(zip(ssa.KEYCHECK_FIELDS, [0, 0, NONE, 0, 0, 0, 0, 0]), ok=True)      # empty
        assert cache.selfcheck(deep=True, repair=True)["ok"]
        _, _, stats = fill_cache(engine, cache, rng, sks[:u], pks[:u], inf[:u])
        assert stats[INSERTED] == u and cache.info()["held"] == u
        for deep in (False, True):
            expect_clean(cache.selfcheck(deep=deep), kinds[:u])
        # partly warm: the second half of those keys and u / 2 new ones
        _, _, stats = fill_cache(engine, cache, rng, sks[u // 2:], pks[u // 2:], inf[u // 2:])
        assert stats[HITS] == u // 2 and stats[INSERTED] == u // 2 and cache.info()["held"] == u + u // 2
        for deep in (False, True):
            expect_clean(cache.selfcheck(deep=deep, repair=deep), kinds)
        # more new keys than there is room for: the cache clears itself and holds the new slice's keys only
        sks2, pks2, inf2, kinds2 = key_material(engine, rng, 300)
        _, _, stats = fill_cache(engine, cache, rng, sks2, pks2, inf2)
        assert stats[CLEARS] == 1 and cache.info()["held"] == 300
        for deep in (False, True):
            expect_clean(cache.selfcheck(deep=deep), kinds2)


# ---- a check changes no result ------------------------------------------------------------------------------------
def test_selfcheck_changes_no_verification_result(engine):
    rng = np.random.default_rng(17300)
    m, n = 200, 6000
    sks, pks, inf, kinds = key_material(engine, rng, m)
    idx, sigs, msgs, lane_pks, lane_inf = signed_lanes(engine, rng, sks, pks, inf, n)
    co = coeffs32(rng, n)
    want, wnf = engine.verify_many(sigs, lane_pks, msgs, pk_inf=lane_inf, check_torsion=True)
    assert 0 < wnf < n
    ks = engine.keyset_create(pks, pk_inf=inf, kind="ladder")
    try:
        with engine.keycache_create(1024) as cache:
            def both():
                a = engine.verify_many_indexed(ks, idx, sigs, msgs, check_torsion=True)
                b = engine.verify_many_cached(cache, sigs, lane_pks, msgs, coeffs=co, pk_inf=lane_inf)
                return a[0].tobytes(), a[1], b[0].tobytes(), b[1]

            before = both()
            assert before == (want.tobytes(), wnf, want.tobytes(), wnf)
            for deep in (False, True):
                expect_clean(ks.selfcheck(deep=deep), kinds)
                expect_clean(cache.selfcheck(deep=deep, repair=True), kinds)
                assert both() == before
            # without the subgroup check the tables of status-1 keys are what the indexed form reads
            w2, w2nf = engine.verify_many(sigs, lane_pks, msgs, pk_inf=lane_inf, check_torsion=False)
            a = engine.verify_many_indexed(ks, idx, sigs, msgs, check_torsion=False)
            assert a[0].tobytes() == w2.tobytes() and a[1] == w2nf
    finally:
        ks.close()


# ---- pokes --------------------------------------------------------------------------------------------------------
class Ladder:
    """a ladder key set and a warm cache over the same keys; rows[i]: key i's number in the object"""

    def __init__(self, engine, rng, m=64):
        self.sks, self.pks, self.inf, self.kinds = key_material(engine, rng, m)
        self.m = m
        self.ks = engine.keyset_create(self.pks, pk_inf=self.inf, kind="ladder")
        self.cache = engine.keycache_create(2 * m)
        fill_cache(engine, self.cache, rng, self.sks, self.pks, self.inf)
        assert self.cache.info()["held"] == m
        self.objects = {"keyset": (self.ks, list(range(m))), "cache": (self.cache, cache_rows(self.cache, self.pks, self.inf))}

    def close(self):
        self.ks.close()
        self.cache.close()


@pytest.fixture(scope="module")
def ladder(engine):
    lad = Ladder(engine, np.random.default_rng(17400))
    yield lad
    lad.close()


def poke_and_restore(obj, what, row, word, mask, m, light_sees, deep_sees=True):
    obj.debug_keytab_xor(what, row, word, mask)
    try:
        for deep, sees in ((False, light_sees), (True, deep_sees)):
            res = obj.selfcheck(deep=deep)
            if sees:
                expect_one_bad(res, row, m)
            else:
                assert res["ok"] and res["keys_bad"] == 0 and res["first_bad_key"] == NONE, (deep, res)
    finally:
        obj.debug_keytab_xor(what, row, word, mask)          # the same XOR puts the word back
    res = obj.selfcheck(deep=True)
    assert res["ok"] and res["keys_bad"] == 0, res


@pytest.mark.parametrize("which", ["keyset", "cache"])
@pytest.mark.parametrize("name,what,key,word,mask", [
    ("positive half", LADDER, 7, 5 * 32 + 3, 1 << 40),
    ("positive half, entry 1", LADDER, 9, 0 * 32 + 11, 1),
    ("negative half x", LADDER, 11, 9 * 32 + 16 + 2, 1 << 63),
    ("negative half y", LADDER, 13, 15 * 32 + 16 + 7, 1 << 5),
    ("status-1 key table", LADDER, 3, 2 * 32 + 6, 1 << 20),
    ("order-2 key table (sentinel entry)", LADDER, 4, 1 * 32 + 0, 1),
    ("identity key table", LADDER, 1, 4 * 32 + 23, 1 << 9),
    ("key byte", KEY, 17, 4, 1 << 17),
    ("key byte of a status-1 key", KEY, 3, 9, 1 << 33),
    ("pk_inf byte 0 -> 1", PK_INF, 19, 0, 1),
    ("pk_inf byte 1 -> 0", PK_INF, 1, 0, 1),
    ("status 0 -> 3", STATUS, 21, 0, 3),
    ("status 3 -> 0", STATUS, 2, 0, 3),
    ("status 3 -> 1", STATUS, 5, 0, 2),
    ("status 0 -> 2", STATUS, 23, 0, 2),
    ("status 1 -> 3", STATUS, 3, 0, 2),
    # the point of order 2 under status 0: its 2P is a sentinel, which no chain of a prime-order key has
    ("status 1 -> 0 of the order-2 key", STATUS, 4, 0, 1),
])
def test_pokes_fail_at_the_poked_key(ladder, which, name, what, key, word, mask):
    obj, rows = ladder.objects[which]
    poke_and_restore(obj, what, rows[key], word, mask, ladder.m, light_sees=True)


@pytest.mark.parametrize("which", ["keyset", "cache"])
@pytest.mark.parametrize("key,kind", [(25, "0 -> 1"), (3, "1 -> 0"), (1, "0 -> 1, identity")])
def test_status_flips_between_0_and_1_need_deep(ladder, which, key, kind):
    obj, rows = ladder.objects[which]
    poke_and_restore(obj, STATUS, rows[key], 0, 1, ladder.m, light_sees=False, deep_sees=True)


@pytest.mark.parametrize("which", ["keyset", "cache"])
def test_padding_word_pokes_stay_clean(ladder, which):
    obj, rows = ladder.objects[which]
    for key, word in ((27, 5 * 32 + 13), (27, 0 * 32 + 31), (3, 7 * 32 + 28), (2, 100)):     # key 2: status 3, table unread
        poke_and_restore(obj, LADDER, rows[key], word, 0xFFFF0000FFFF, ladder.m, light_sees=False, deep_sees=False)


def test_two_pokes_report_the_first_and_count_both(ladder):
    obj, rows = ladder.objects["keyset"]
    a, b = sorted((rows[30], rows[41]))
    obj.debug_keytab_xor(LADDER, a, 3 * 32 + 1, 2)
    obj.debug_keytab_xor(LADDER, b, 8 * 32 + 20, 4)
    try:
        res = obj.selfcheck()
        assert not res["ok"] and res["keys_bad"] == 2 and res["first_bad_key"] == a
        assert list(np.nonzero(res["bad"])[0]) == [a, b]
    finally:
        obj.debug_keytab_xor(LADDER, a, 3 * 32 + 1, 2)
        obj.debug_keytab_xor(LADDER, b, 8 * 32 + 20, 4)
    assert obj.selfcheck(deep=True)["ok"]


def test_comb_row_pokes_fail_at_the_poked_key(engine):
    rng = np.random.default_rng(17500)
    sks, pks, inf, kinds = key_material(engine, rng, 2)
    ks = engine.keyset_create(pks, pk_inf=inf, kind="comb")
    try:
        expect_clean(ks.selfcheck(), kinds, comb=True)
        base = ks.debug_keytab_read(COMB, 1)
        assert not base[:12].any() and base[12:].view(np.uint8).tobytes() == pks[1].tobytes()     # rows (0, 0), (0, 1)
        for key, row, word, mask in ((1, (7 << 16) + 12345, 4, 1 << 30), (0, 1, 0, 1), (1, 0, 11, 1 << 63),
                                     (0, COMB_ROWS - 1, 6, 1 << 2)):
            poke_and_restore(ks, COMB, key, 12 * row + word, mask, 2, light_sees=True)
    finally:
        ks.close()


# ---- repair -------------------------------------------------------------------------------------------------------
def test_repair_rebuilds_the_poked_rows_and_the_cache_stays_exact(engine):
    rng = np.random.default_rng(17600)
    m = 300
    sks, pks, inf, kinds = key_material(engine, rng, m)
    with engine.keycache_create(512) as cache:
        batch, st0, stats = fill_cache(engine, cache, rng, sks, pks, inf, n=8000)
        sigs, lane_pks, msgs, co, lane_inf = batch
        assert stats[INSERTED] == m
        rows = cache_rows(cache, pks, inf)
        pokes = [(LADDER, rows[10], 6 * 32 + 2, 1 << 11), (LADDER, rows[20], 12 * 32 + 16 + 9, 1 << 50),
                 (STATUS, rows[30], 0, 3), (LADDER, rows[3], 3 * 32 + 1, 1 << 7), (PK_INF, rows[40], 0, 1),
                 (KEY, rows[50], 2, 1 << 21)]
        for what, row, word, mask in pokes:
            cache.debug_keytab_xor(what, row, word, mask)
        k = len(pokes)
        res = cache.selfcheck()
        assert not res["ok"] and res["keys_bad"] == k and res["first_bad_key"] == min(p[1] for p in pokes)
        assert res["rows_repaired"] == 0
        res = cache.selfcheck(repair=True)
        assert res["ok"] and res["keys_bad"] == k and res["rows_repaired"] == k, res
        assert res["first_bad_key"] == min(p[1] for p in pokes)
        for deep in (False, True):
            res = cache.selfcheck(deep=deep, repair=deep)
            assert res["ok"] and res["keys_bad"] == 0 and res["rows_repaired"] == 0 and res["keys_checked"] == m, res
        # the repaired cache is a correct cache: byte for byte the screened form's vector under the same coefficients;
        # the two rows whose 97 bytes changed answer for other keys now, so the original keys miss and are inserted again
        want, wnf, _ = engine.verify_many_screened(sigs, lane_pks, msgs, coeffs=co, pk_inf=lane_inf)
        st, nf, stats = engine.verify_many_cached(cache, sigs, lane_pks, msgs, coeffs=co, pk_inf=lane_inf)
        assert st.tobytes() == want.tobytes() == st0.tobytes() and nf == wnf
        assert int(stats[INSERTED]) == 2 and int(stats[HITS]) == m - 2, stats
        assert cache.info()["held"] == m + 2
        assert cache.selfcheck(deep=True)["ok"]


def test_repair_with_deep_fixes_a_flipped_status(engine):
    rng = np.random.default_rng(17601)
    m = 64
    sks, pks, inf, kinds = key_material(engine, rng, m)
    with engine.keycache_create(128) as cache:
        fill_cache(engine, cache, rng, sks, pks, inf)
        rows = cache_rows(cache, pks, inf)
        cache.debug_keytab_xor(STATUS, rows[3], 0, 1)           # 1 -> 0: a key outside the subgroup would be accepted
        assert cache.selfcheck(repair=True)["rows_repaired"] == 0
        res = cache.selfcheck(deep=True, repair=True)
        assert res["ok"] and res["keys_bad"] == 1 and res["first_bad_key"] == rows[3] and res["rows_repaired"] == 1
        assert int(cache.debug_keytab_read(STATUS, rows[3])[0]) == 1
        expect_clean(cache.selfcheck(deep=True), kinds)


# ---- edge cases ---------------------------------------------------------------------------------------------------
def test_arguments_on_live_objects(ladder):
    lib = ssa._lib
    out = (C.c_uint64 * 8)()
    bad = (C.c_uint8 * ladder.m)()
    ks, kc = ladder.ks.handle, ladder.cache.handle
    for flags in (2, 3, 4, 1 << 31):
        assert lib.ssa_keyset_selfcheck(ks, flags, bad, out) == ssa.ERR_ARG, flags
    for flags in (4, 8, 1 << 31):
        assert lib.ssa_keycache_selfcheck(kc, flags, out) == ssa.ERR_ARG, flags
    assert lib.ssa_keyset_selfcheck(ks, 0, bad, None) == ssa.ERR_ARG
    assert lib.ssa_keycache_selfcheck(kc, 0, None) == ssa.ERR_ARG
    assert lib.ssa_keyset_selfcheck(ks, 1, None, out) == ssa.OK            # bad_out is optional
    m = ladder.m
    words = (C.c_uint64 * 512)()
    for h in ((ks, None), (None, kc)):
        for args in ((LADDER, m, 0, 1), (LADDER, 0, 512, 1), (LADDER, 2 ** 40, 0, 1), (STATUS, 0, 1, 1), (STATUS, 0, 0, 256),
                     (KEY, 0, 12, 1), (PK_INF, m, 0, 1), (PK_INF, 0, 0, 1 << 8), (COMB, 0, 0, 1), (5, 0, 0, 1), (-1, 0, 0, 1)):
            assert lib.ssa_debug_keytab_xor(*h, *args) == ssa.ERR_ARG, args
        assert lib.ssa_debug_keytab_read(*h, LADDER, m, words) == ssa.ERR_ARG
        assert lib.ssa_debug_keytab_read(*h, COMB, 0, words) == ssa.ERR_ARG
        assert lib.ssa_debug_keytab_read(*h, LADDER, 0, None) == ssa.ERR_ARG
    assert lib.ssa_debug_keytab_xor(ks, kc, LADDER, 0, 0, 1) == ssa.ERR_ARG
    assert ladder.ks.selfcheck(deep=True)["ok"] and ladder.cache.selfcheck(deep=True)["ok"]     # nothing was written


def test_orphaned_objects_are_refused():
    eng = ssa.Engine(0)
    rng = np.random.default_rng(17700)
    sks, pks, inf, _ = key_material(eng, rng, 4)
    ks = eng.keyset_create(pks, kind="ladder")
    cache = eng.keycache_create(16)
    assert ks.selfcheck()["ok"] and cache.selfcheck()["ok"]
    eng.close()
    out = (C.c_uint64 * 8)()
    assert ssa._lib.ssa_keyset_selfcheck(ks.handle, 0, None, out) == ssa.ERR_ARG
    assert ssa._lib.ssa_keycache_selfcheck(cache.handle, 0, out) == ssa.ERR_ARG
    assert ssa._lib.ssa_debug_keytab_xor(ks.handle, None, LADDER, 0, 0, 1) == ssa.ERR_ARG
    assert ssa._lib.ssa_debug_keytab_xor(None, cache.handle, LADDER, 0, 0, 1) == ssa.ERR_ARG
    ks.close()
    cache.close()


def test_key_set_made_without_flags_keeps_zero_flags(engine):
    rng = np.random.default_rng(17701)
    sks, pks, inf, kinds = key_material(engine, rng, 16, specials=False)
    ks = engine.keyset_create(pks, kind="ladder")
    try:
        assert all(int(ks.debug_keytab_read(PK_INF, i)[0]) == 0 for i in range(16))
        expect_clean(ks.selfcheck(deep=True), kinds)
        tab = ks.debug_keytab_read(LADDER, 5)
        assert tab[:12].view(np.uint8).tobytes() == pks[5].tobytes()          # entry 1P is the key, bit for bit
        assert ks.debug_keytab_read(KEY, 5).view(np.uint8).tobytes() == pks[5].tobytes()
    finally:
        ks.close()
