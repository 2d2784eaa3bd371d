"""CPU tests of the table self-check (ssa_ctx_selfcheck): the ABI it adds, and a big-integer model
of the relations the kernel checks (oracle/pymodel.py arithmetic) -- true chains pass, every single-word flip is found
at the flipped row, and the degenerate chord / tangent inputs are refused."""
import ctypes
import os
import re

import pytest

import pymodel as m

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "schnorr_sig_amd.h")
NEW = ("ssa_ctx_selfcheck", "ssa_debug_table_read", "ssa_debug_table_xor", "ssa_debug_corrupt_table_builds")
NONE = 2 ** 64 - 1


def test_header_declares_the_selfcheck_abi():
    hdr = open(HDR).read()
    for name in NEW:
        assert re.search(r"\bint %s\s*\(" % name, hdr), name
    assert re.search(r"#define SSA_ERR_TABLE \(-5\)", hdr)
    assert re.search(r"#define SSA_ABI_VERSION 5\b", hdr)


def test_library_exports_the_selfcheck_abi():
    import schnorr_sig_amd as ssa
    lib = ctypes.CDLL(ssa.LIB_PATH)
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in ssa.ABI_SYMBOLS
    assert ssa.ERR_TABLE == -5
    assert hasattr(ssa.Engine, "selfcheck") and hasattr(ssa, "debug_corrupt_table_builds")


def test_strerror_of_err_table_is_its_own():
    import schnorr_sig_amd as ssa
    msgs = {rc: ssa._lib.ssa_strerror(rc).decode() for rc in (0, 1, 2, 3, -1, -2, -3, -4, -5, -99)}
    assert msgs[-5] != msgs[-99]                        # not "unknown"
    assert list(msgs.values()).count(msgs[-5]) == 1
    assert "table" in msgs[-5]


def test_selfcheck_refuses_bad_arguments_without_a_device():
    import schnorr_sig_amd as ssa
    out = (ctypes.c_uint64 * 8)()
    assert ssa._lib.ssa_ctx_selfcheck(None, 0, out) == ssa.ERR_ARG
    assert ssa._lib.ssa_debug_table_read(None, 0, 0, 1, None) == ssa.ERR_ARG
    assert ssa._lib.ssa_debug_table_xor(None, 0, 0, 0, 1) == ssa.ERR_ARG
    assert ssa._lib.ssa_debug_corrupt_table_builds(-1) == ssa.ERR_ARG
    assert ssa._lib.ssa_debug_corrupt_table_builds(0) == 0


# ---- the model ------------------------------------------------------------------------------------------------------
def windows(bits):
    return (255 + bits) // bits


def header(bits):
    return bits | windows(bits) << 8


def rows_checked(bits):
    return windows(bits) << bits


def chain_rel(R, P, Q, tangent):
    """R == P + Q (chord) or R == 2P (tangent) without an inversion; False on the degenerate den == 0"""
    (xr, yr), (xp, yp) = R, P
    if tangent:
        num = m.f6_add(m.f6_scale(m.f6_sqr(xp), 3), m.F6_ONE)
        den = m.f6_scale(yp, 2)
        xs = m.f6_scale(xp, 2)
    else:
        xq, yq = Q
        num, den, xs = m.f6_sub(yq, yp), m.f6_sub(xq, xp), m.f6_add(xp, xq)
    if den == m.F6_ZERO:
        return False
    ex = m.f6_mul(m.f6_add(xr, xs), m.f6_sqr(den)) == m.f6_sqr(num)
    ey = m.f6_mul(m.f6_add(yr, yp), den) == m.f6_mul(num, m.f6_sub(xp, xr))
    return ex and ey


def check_table(rows, bits, nwin, head, g):
    """the kernel's verdict on a table of 12-word rows: (failing rows, first failing row)"""
    nbad, first = 0, NONE
    pt = lambda r: (tuple(r[:6]), tuple(r[6:]))          # noqa: E731
    for w in range(nwin):
        base = w << bits
        B = pt(rows[base + 1])
        prev = pt(rows[base - 1]) if w else None
        for d in range(1 << bits):
            r = rows[base + d]
            ok = all(v < m.P for v in r)
            if d == 0:
                ok = ok and list(r) == [head if w == 0 else 0] + [0] * 11
            elif d == 1 and w == 0:
                ok = ok and pt(r) == g
            else:
                Q = pt(rows[base - (1 << bits) + 1]) if d == 1 else B
                ok = ok and chain_rel(pt(r), B if d == 2 else prev, Q, d == 2)
                prev = pt(r)
            if not ok:
                nbad += 1
                first = min(first, base + d)
    return nbad, first


def build_table(bits, nwin, g, head):
    rows = []
    for w in range(nwin):
        b = m.pt_mul(1 << (bits * w), g)
        acc = None
        for d in range(1 << bits):
            rows.append([head if (w, d) == (0, 0) else 0] + [0] * 11 if acc is None else list(acc[0]) + list(acc[1]))
            acc = m.pt_add(acc, b)
    return rows


@pytest.fixture(scope="module")
def toy():
    g = m.default_params().generator()
    bits, nwin = 4, 2
    return bits, nwin, g, build_table(bits, nwin, g, header(bits))


def test_model_accepts_true_chains(toy):
    bits, nwin, g, rows = toy
    assert check_table(rows, bits, nwin, header(bits), g) == (0, NONE)
    # the first rows of a window, a tangent row and the window hop, as the relations say
    pt = lambda r: (tuple(r[:6]), tuple(r[6:]))          # noqa: E731
    B1 = pt(rows[16 + 1])
    assert chain_rel(pt(rows[16 + 2]), B1, None, True)                         # (1, 2) = 2 B_1
    assert chain_rel(pt(rows[16 + 3]), pt(rows[16 + 2]), B1, False)            # (1, 3) = (1, 2) + B_1
    assert chain_rel(pt(rows[16 + 1]), pt(rows[15]), pt(rows[1]), False)       # (1, 1) = (0, 15) + B_0
    assert chain_rel(pt(rows[2]), pt(rows[1]), None, True)
    assert pt(rows[16 + 1]) == m.pt_mul(16, g)


def test_model_finds_every_single_word_flip_at_the_flipped_row(toy):
    bits, nwin, g, rows = toy
    for k in range(len(rows)):
        for word in range(12):
            bad = [list(r) for r in rows]
            bad[k][word] ^= 1 << (5 * word % 64)
            nbad, first = check_table(bad, bits, nwin, header(bits), g)
            assert first == k and nbad >= 1, (k, word)


def test_model_refuses_degenerate_inputs(toy):
    bits, nwin, g, rows = toy
    pt = lambda r: (tuple(r[:6]), tuple(r[6:]))          # noqa: E731
    P = pt(rows[3])
    # dx == 0: a chord through P and P (the tangent's answer is the only R that fits, yet it is refused), and P, -P
    assert not chain_rel(m.pt_add(P, P), P, P, False)
    assert not chain_rel(pt(rows[1]), P, m.pt_neg(P), False)
    # y_P == 0: a tangent at a point of order 2 (the relation would accept any R with the right x otherwise)
    two_torsion = (P[0], m.F6_ZERO)
    assert not chain_rel(P, two_torsion, None, True)


def test_model_geometry_matches_the_host_formula():
    assert [(b, windows(b), rows_checked(b)) for b in (16, 20, 22, 24)] == [
        (16, 16, 16 << 16), (20, 13, 13 << 20), (22, 12, 12 << 22), (24, 11, 11 << 24)]
    for b in (16, 20, 22, 24):
        assert b * windows(b) >= 256 > b * (windows(b) - 1)
        assert header(b) == b | windows(b) << 8 and header(b) < m.P
    assert rows_checked(24) == 184549376                # 1.85e8 rows, 17.7 GB at 96 bytes per row
