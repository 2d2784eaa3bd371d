"""GPU tests of the exact table self-check (ssa_ctx_selfcheck): clean tables at every width, rows
against the oracle, the constant-time table, read-only behaviour, and failures found at the poked row -- on demand and
at build time.  Tables are poked only in child processes, which run no verification or signing after a poke."""
import os
import subprocess
import sys

import numpy as np
import pytest

import schnorr_sig_amd as ssa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = 2 ** 64 - 1
pytestmark = pytest.mark.gpu


def _windows(bits):
    return (255 + bits) // bits


def _scalars(rng, n):
    s = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    s[:, 31] &= 0x3F
    s[:, 0] |= 1
    return s


def _child(code, timeout=600):
    r = subprocess.run([sys.executable, "-c", "import schnorr_sig_amd as ssa\nimport numpy as np\n" + code],
                       capture_output=True, text=True, timeout=timeout, cwd=ROOT)
    assert r.returncode == 0, "child exit %d:\n%s" % (r.returncode, r.stderr[-4000:])
    assert "DONE" in r.stdout, r.stdout[-2000:]
    return r.stdout


def _generator():
    blob = ssa.Engine.default_params()
    w = np.frombuffer(blob[2720:2816], dtype="<u8")
    return tuple(int(v) for v in w[:6]), tuple(int(v) for v in w[6:])


# ---- 1. healthy tables are clean --------------------------------------------------------------------------------
def test_session_engine_tables_are_clean(engine):
    r = engine.selfcheck()
    bits = engine.info()["gtab_bits"]
    assert r["ok"], r
    assert r["bits"] == bits
    assert r["rows"] == _windows(bits) << bits
    assert r["bad"] == 0 and r["first_bad"] == NONE
    assert r["builds"] == 1


@pytest.mark.parametrize("bits", [16, 20, 22])
def test_fresh_engines_are_clean(bits):
    eng = ssa.Engine(0, gtab_bits=bits)
    try:
        r = eng.selfcheck()
        assert r["ok"] and r["bits"] == bits and r["rows"] == _windows(bits) << bits, r
        assert r["bad"] == 0 and r["first_bad"] == NONE and r["builds"] >= 1
    finally:
        eng.close()


# ---- 2. independent ground truth --------------------------------------------------------------------------------
def test_comb_rows_equal_the_oracle(oracle):
    bits, q = 16, ssa.Q
    g = _generator()
    rng = np.random.default_rng(7100)
    picks = [(w, d) for w in range(_windows(bits)) for d in (1, 2, (1 << bits) - 1)]
    picks += [(int(rng.integers(0, _windows(bits))), int(rng.integers(1, 1 << bits))) for _ in range(150)]
    eng = ssa.Engine(0, gtab_bits=bits)
    try:
        assert eng.selfcheck()["ok"]
        for w, d in picks:
            row = eng.debug_table_read(ssa.TABLE_COMB, (w << bits) + d, 1)[0]
            x, y = oracle.point_mul(d * pow(2, bits * w, q) % q, g)
            assert [int(v) for v in row] == list(x) + list(y), (w, d)
        zero = eng.debug_table_read(ssa.TABLE_COMB, 3 << bits, 1)[0]
        assert not zero.any()
    finally:
        eng.close()


# ---- 3. the constant-time table ---------------------------------------------------------------------------------
def test_ct_table_is_checked_once_built():
    rng = np.random.default_rng(7200)
    eng = ssa.Engine(0, gtab_bits=16)
    try:
        r = eng.selfcheck()
        assert r["ok"] and r["ctab_rows"] == 0 and r["ctab_bad"] == 0 and r["ctab_first_bad"] == NONE, r
        eng.keygen_sign_many(_scalars(rng, 4), _scalars(rng, 4), np.zeros((4, 16), np.uint8), constant_time=True)
        r = eng.selfcheck()
        assert r["ok"] and r["ctab_rows"] == 1026 and r["ctab_bad"] == 0 and r["ctab_first_bad"] == NONE, r
    finally:
        eng.close()


# ---- 4. the check only reads --------------------------------------------------------------------------------------
def test_selfcheck_changes_no_result(engine):
    rng = np.random.default_rng(7300)
    n = 3000
    sks, nonces = _scalars(rng, n), _scalars(rng, n)
    msgs = rng.integers(0, 256, size=(n, 40), dtype=np.uint8)

    def run():
        out = []
        for ct in (False, True):
            pks, sigs = engine.keygen_sign_many(sks, nonces, msgs, constant_time=ct)
            bad = sigs.copy()
            bad[::7, 60] ^= 1
            st, nf = engine.verify_many(bad, pks, msgs, check_torsion=True)
            out += [pks.tobytes(), sigs.tobytes(), st.tobytes(), nf]
        return out

    before = run()
    r = engine.selfcheck()
    assert r["ok"] and r["ctab_rows"] == 1026, r
    after = run()
    assert before == after
    assert before[3] == (n + 6) // 7


# ---- 5. on-demand failures point at the poked row -----------------------------------------------------------------
def test_pokes_fail_at_the_poked_row():
    code = r"""
B = 16
M = (1 << B) - 1
rng = np.random.default_rng(7400)
s = rng.integers(1, 200, size=(2, 32), dtype=np.uint8)
s[:, 31] = 0
eng = ssa.Engine(0, gtab_bits=B)
eng.keygen_sign_many(s, s, np.zeros((2, 8), np.uint8), constant_time=True)   # the only signature: before any poke
r = eng.selfcheck()
assert r["ok"] and r["ctab_rows"] == 1026 and r["builds"] == 1, r
cases = [((0, 1), 0, 1), ((0, 1), 6, 1 << 40), ((0, 2), 3, 1), ((0, 2), 9, 1 << 63),
         ((3, 12345), 0, 1 << 5), ((3, 12345), 11, 1 << 17), ((5, M), 4, 1), ((7, 1), 7, 1 << 33),
         ((2, 0), 5, 1), ((0, 0), 0, 1 << 1)]
for (w, d), word, mask in cases:
    row = (w << B) + d
    eng.debug_table_xor(ssa.TABLE_COMB, row, word, mask)
    r = eng.selfcheck()
    assert not r["ok"] and r["first_bad"] == row, ((w, d), word, r)
    if (w, d) == (5, M):
        assert r["bad"] >= 2, r
    if (w, d) == (7, 1):
        assert r["bad"] >= M, r
    eng.debug_table_xor(ssa.TABLE_COMB, row, word, mask)                      # restored
    r = eng.selfcheck()
    assert r["ok"] and r["bad"] == 0 and r["ctab_rows"] == 1026, r
# the constant-time table (built by the signature above, before any poke)
eng.debug_table_xor(ssa.TABLE_CT, 16 * 5 + 7, 3, 1 << 9)
r = eng.selfcheck()
assert not r["ok"] and r["bad"] == 0 and r["ctab_first_bad"] == 16 * 5 + 7 and r["ctab_bad"] >= 1, r
r = eng.selfcheck()
assert r["ok"] and r["ctab_rows"] == 0, r      # no longer used: the next constant-time call rebuilds it
try:
    eng.debug_table_read(ssa.TABLE_CT, 0, 1)
    raise SystemExit("a failed constant-time table is still readable")
except RuntimeError:
    pass
# restoring a comb word did not un-retire the table: with one row left wrong, a new engine gets a new table
eng.debug_table_xor(ssa.TABLE_COMB, (3 << B) + 12345, 2, 1)
eng2 = ssa.Engine(0, gtab_bits=B)
r2 = eng2.selfcheck()
assert r2["ok"] and r2["builds"] == 1, r2
r = eng.selfcheck()
assert not r["ok"] and r["first_bad"] == (3 << B) + 12345, r
for bad in ((-1, 0), (16 << B, 0), (0, 12)):
    try:
        eng.debug_table_xor(ssa.TABLE_COMB, bad[0] & (2 ** 64 - 1), bad[1], 1)
        raise SystemExit("out of bounds poke accepted: %r" % (bad,))
    except RuntimeError:
        pass
eng2.close()
eng.close()
print("DONE")
"""
    _child(code)


# ---- 6. failures at build time ------------------------------------------------------------------------------------
def test_build_failure_once_is_rebuilt():
    _child("""
ssa.debug_corrupt_table_builds(1)
eng = ssa.Engine(0, gtab_bits=16)
r = eng.selfcheck()
assert r["ok"] and r["builds"] == 2 and r["bits"] == 16, r
eng.close()
print("DONE")
""")


def test_build_failure_twice_falls_back_a_width():
    _child("""
ssa.debug_corrupt_table_builds(2)
eng = ssa.Engine(0, gtab_bits=20)
assert eng.info()["gtab_bits"] == 16, eng.info()
r = eng.selfcheck()
assert r["ok"] and r["builds"] == 1 and r["bits"] == 16, r
eng.close()
print("DONE")
""")


def test_build_failure_everywhere_is_err_table():
    _child("""
ssa.debug_corrupt_table_builds(1000)
try:
    ssa.Engine(0, gtab_bits=16)
    raise SystemExit("created")
except RuntimeError as e:
    assert "(-5)" in str(e), str(e)
ssa.debug_corrupt_table_builds(0)
eng = ssa.Engine(0, gtab_bits=16)
assert eng.selfcheck()["ok"]
eng.close()
print("DONE")
""")
