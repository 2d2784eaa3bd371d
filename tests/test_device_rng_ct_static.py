"""Static check of the device-side draw of nonces and keys (schnorr-sig_amd/csrc/ssa_rng.hpp):
Scalar::random(rng) runs on the GPU, so the ChaCha20 rounds on the secret seed, the 512-bit reduction mod q and the
zero-fallback select are secret work.  They live in the out-of-line ct_draw_scalar (the pre-pass ssa_k_draw_scalars_ct)
and ct_draw_wide (the test hook's kernel), which get the rules of tests/test_signer_set_ct_static.py:
  * no branch on EXEC or VCC, no EXEC narrowing, no v_readfirstlane, v_readlane only to reload a spilled SGPR;
  * every remaining conditional branch follows an s_cmp of an SGPR with an immediate (the ChaCha20 round counter);
  * every call is direct and goes to a checked body;
  * no vector memory access takes its address from a loaded value (the taint pass of tests/test_derive_ct_static.py).
The helpers are those of tests/test_signer_set_ct_static.py and tests/test_derive_ct_static.py, imported."""
import re

import pytest

import test_derive_ct_static as dct
import test_signer_set_ct_static as sct

DRAW_FUNCS = ("ct_draw_scalar", "ct_draw_wide")


@pytest.fixture(scope="module")
def fns():
    return dct._functions(dct._asm())


def test_draw_functions_have_no_data_dependent_control_flow(fns, monkeypatch):
    # the signer-set test's rule set, pointed at the draw functions (its checked closure plus these)
    monkeypatch.setattr(sct, "NEW_FUNCS", DRAW_FUNCS)
    sct.test_new_secret_functions_have_no_data_dependent_control_flow(fns)


def test_draw_functions_call_nothing(fns):
    """the whole draw is inline in the two checked bodies: nothing secret escapes into an unchecked callee"""
    for name in DRAW_FUNCS:
        assert sct._calls(fns[name]) == [], name


def test_draw_is_two_chacha_blocks_reduced_and_selected(fns):
    """both blocks are always computed: the round loop runs twice (two counted loops with the round bound 10), and the
    result is chosen with selects, not branches"""
    lines = dct._lines(fns["ct_draw_scalar"])
    loops = [ln for ln in lines if re.match(r"s_cbranch_scc[01] \.LBB\d+_\d+$", ln)]
    assert len(loops) == 2, loops
    assert sum(1 for ln in lines if ln.startswith("v_cndmask_b32")) >= 8 or \
        sum(1 for ln in lines if ln.startswith(("v_and_b32", "v_and_or_b32", "v_bfi_b32"))) >= 8


def test_prepass_kernels_call_only_the_checked_draw(fns):
    assert sct._calls(fns["ssa_k_draw_scalars_ct"]) == ["ct_draw_scalar"]
    assert sct._calls(fns["ssa_k_draw_wide"]) == ["ct_draw_wide"]


def test_existing_signing_kernels_are_untouched_consumers(fns):
    """the signers read the drawn scalars as their nonces through the same checked functions as before"""
    for kern in ("ssa_k_sign_ct", "ssa_k_sign_indexed_ct"):
        calls = sct._calls(fns[kern])
        assert "ct_draw_scalar" not in calls and "ct_draw_wide" not in calls
        assert set(calls) <= set(sct.CHECKED), calls
