"""Host logic of the one-slice split, on the CPU (no device): the two parts ssa_api.hip cuts a one-slice call into.

Part A, lanes [0, nA), stays on the caller's stream; part B, the nB lanes behind it, runs on the second stream into the
lane range [nA, n) of the same workspaces.  So the parts must cover every lane exactly once, B must start at a workgroup
of its own (nA a multiple of 256: ssa_k_hash and ssa_k_verify run 256 lanes per workgroup), A must be the longer part
(it ends alone, with the end game), and a call that is short, cooperative or without a second stream is not split."""
import pytest

SPLIT_MIN = 1 << 17
COOP, COOP_TORSION = 7680, 10496          # the cooperative kernel's crossovers (CtxKnobs)
SIZES = [0, 1, 255, 256, 257, SPLIT_MIN - 1, SPLIT_MIN, 1 << 20, (1 << 20) - 1]
FRACS = list(range(0, 9))                 # SSA_SPLIT_FRAC in 1/16ths; 0 = off


@pytest.fixture(scope="module")
def ssa():
    import schnorr_sig_amd as m
    return m


@pytest.mark.parametrize("frac", FRACS)
@pytest.mark.parametrize("n", SIZES)
def test_parts_cover_every_lane_once(ssa, n, frac):
    for torsion in (False, True):
        for split_min in (0, SPLIT_MIN):
            nA, nB = ssa.debug_split_plan(n, frac, split_min=split_min, check_torsion=torsion)
            # A = [0, nA), B = [nA, nA + nB): every lane once
            assert nA + nB == n and nA >= 0 and nB >= 0
            assert nB <= nA
            if nB:
                assert nA % 256 == 0 and nA > 0
                # the short part is the share asked for, to within the one workgroup nA is rounded up by
                assert n * frac // 16 - 256 < nB <= n * frac // 16
            else:
                assert nA == n


@pytest.mark.parametrize("frac", FRACS[1:])
def test_large_calls_are_split_when_everything_allows_it(ssa, frac):
    for n in (SPLIT_MIN, (1 << 20) - 1, 1 << 20):
        nA, nB = ssa.debug_split_plan(n, frac, split_min=SPLIT_MIN)
        assert nB > 0 and nA % 256 == 0 and nA + nB == n
    # forced lane kernels at a size of the tests: n = 7681 + 256 k + r
    nA, nB = ssa.debug_split_plan(7681 + 256 * 3 + 100, frac, split_min=0)
    assert nB > 0 and nA % 256 == 0


@pytest.mark.parametrize("frac", FRACS)
@pytest.mark.parametrize("n", SIZES)
def test_no_split_when_off_short_cooperative_or_without_twin(ssa, n, frac):
    # the twin is off (SSA_TWO_STREAMS=0, no memory for it, or the context is itself a twin)
    assert ssa.debug_split_plan(n, frac, twin=False) == (n, 0)
    # under the minimum
    assert ssa.debug_split_plan(n, frac, split_min=n + 1) == (n, 0)
    if n < SPLIT_MIN:
        assert ssa.debug_split_plan(n, frac, split_min=SPLIT_MIN) == (n, 0)
    # the split is off
    assert ssa.debug_split_plan(n, 0) == (n, 0)
    # the cooperative path: at and below the crossover of the flag word, and above it only when forced to lanes
    for torsion, lim in ((False, COOP), (True, COOP_TORSION)):
        if n <= lim:
            assert ssa.debug_split_plan(n, frac, check_torsion=torsion) == (n, 0)
    assert ssa.debug_split_plan(COOP, 8) == (COOP, 0) and ssa.debug_split_plan(COOP + 1, 8)[1] > 0
    assert ssa.debug_split_plan(COOP_TORSION, 8, check_torsion=True) == (COOP_TORSION, 0)
    assert ssa.debug_split_plan(COOP_TORSION + 1, 8, check_torsion=True)[1] > 0
    assert ssa.debug_split_plan(1 << 20, 8, coop_max_n=1 << 20) == (1 << 20, 0)
    assert ssa.debug_split_plan(4096, 8, force_lane=True)[1] > 0


def test_a_share_above_one_half_is_refused(ssa):
    """B is never the longer part: the knob stops at 8/16, and a plan asked for more does not split"""
    assert ssa.debug_split_plan(1 << 20, 9) == (1 << 20, 0)
    nA, nB = ssa.debug_split_plan(1 << 20, 8)
    assert nA == nB == 1 << 19
    nA, nB = ssa.debug_split_plan((1 << 20) - 1, 8)
    assert nA == 1 << 19 and nB == (1 << 19) - 1
