"""The streaming aggregator (ssa_aggregator_*) on the CPU: the plan of a push against brute force,
and the algorithm itself -- leaves appended push by push, the tops of completed blocks stored, finish from the stored tops
plus the ragged block -- restated over the model of tests/aggregate_model.py and held against the one-shot aggregate of
the concatenation, for every split into pushes and every prefix."""
import itertools

import numpy as np
import pytest

import aggregate_model as am


# ---------------------------------------------------------------------------------------------- the plan of a push
def brute_plan(held, m, B):
    """blocks of B lanes that hold no lane >= held + m and at least one lane >= held; then the lanes behind the last
    complete block"""
    total = held + m
    done = [b for b in range(total // B + 1) if B * (b + 1) <= total and B * (b + 1) > held]
    tail_first = max((B * (b + 1) for b in range(total // B + 1) if B * (b + 1) <= total), default=0)
    return (done[0] if done else held // B, len(done), tail_first, total - tail_first)


@pytest.mark.parametrize("B", [2, 4, 8, 64])
def test_plan_against_brute_force(B):
    import schnorr_sig_amd as ssa
    for held in range(71):
        for m in range(71):
            got = ssa.aggregator_plan(held, m, B)
            assert got == brute_plan(held, m, B), (held, m, B, got)
            first, count, tail_first, tail_len = got
            assert first == held // B and tail_first == B * (first + count) and 0 <= tail_len < B


def test_plan_around_the_default_block():
    import schnorr_sig_amd as ssa
    edges = [0, 1, 511, 512, 513, 1023, 1024, 1025]
    for held in edges:
        for m in edges:
            assert ssa.aggregator_plan(held, m, 512) == brute_plan(held, m, 512), (held, m)
            assert ssa.aggregator_plan(held, m, 0) == ssa.aggregator_plan(held, m, 512)       # 0: the default


def test_plan_refuses_what_create_refuses():
    import schnorr_sig_amd as ssa
    for B in (1, 3, 6, 1024, 513):
        with pytest.raises(RuntimeError):
            ssa.aggregator_plan(0, 1, B)
    with pytest.raises(RuntimeError):
        ssa.aggregator_plan(1 << 30, 1, 512)                                                  # above SSA_MAX_BATCH


def test_symbols_are_declared_and_exported():
    import schnorr_sig_amd as ssa
    names = ["ssa_aggregator_create", "ssa_aggregator_destroy", "ssa_aggregator_reset", "ssa_aggregator_info",
             "ssa_aggregator_push", "ssa_aggregator_push_device", "ssa_aggregator_finish", "ssa_aggregator_finish_device",
             "ssa_debug_aggregator_plan"]
    assert all(n in ssa.ABI_SYMBOLS for n in names)
    assert ssa.ABI_VERSION == ssa._lib.ssa_abi_version() == 5


def test_null_handles_are_argument_errors():
    """what the entry points refuse before they touch a device"""
    import ctypes as C
    import schnorr_sig_amd as ssa
    lib, h, out8, nk, buf = ssa._lib, C.c_void_p(), (C.c_uint64 * 8)(), C.c_uint64(7), (C.c_uint8 * 32)()
    assert lib.ssa_aggregator_create(None, 16, 0, 0, C.byref(h)) == ssa.ERR_ARG and not h.value
    assert lib.ssa_aggregator_reset(None) == ssa.ERR_ARG
    assert lib.ssa_aggregator_info(None, out8) == ssa.ERR_ARG
    assert lib.ssa_aggregator_push(None, None, None, None, None, None, None, 0, 0, 0, 0, None, C.byref(nk)) == ssa.ERR_ARG
    assert lib.ssa_aggregator_push_device(None, None, None, None, None, None, None, 0, 0, 0, 0, None,
                                          C.byref(nk)) == ssa.ERR_ARG
    assert lib.ssa_aggregator_finish(None, None, 0, buf) == ssa.ERR_ARG
    assert lib.ssa_aggregator_finish_device(None, None, 0, buf) == ssa.ERR_ARG
    assert nk.value == 7
    lib.ssa_aggregator_destroy(None)


# ---------------------------------------------------------------------------------------------- the algorithm over the model
N_MAX = 20


def cached(backend):
    """the pymodel back-end with every hash computed once: the splits below ask for the same nodes again and again"""
    hfm, hmsg = backend[0], backend[1]
    seen_f, seen_m = {}, {}

    def hash_field_many(rows):
        out = []
        for r in rows:
            key = tuple(int(v) for v in r)
            if key not in seen_f:
                seen_f[key] = [int(v) for v in hfm([list(key)])[0]]
            out.append(list(seen_f[key]))
        return out

    def hash_message(rx48, pk96, msg):
        key = (bytes(rx48), bytes(pk96), bytes(msg))
        if key not in seen_m:
            seen_m[key] = hmsg(*key)
        return seen_m[key]
    return hash_field_many, hash_message


class ModelAggregator:
    """what ssa_aggregator holds and does, in the model's terms"""

    def __init__(self, backend, B):
        self.be, self.B = backend, B
        self.rs, self.es, self.leaves, self.tops = [], [], [], []

    def push(self, sigs, pks, msgs):
        held, B = len(self.leaves), self.B
        rs = [bytes(s)[:49] for s in sigs]
        self.rs += rs
        self.es += [int.from_bytes(bytes(s)[49:81], "little") for s in sigs]
        self.leaves += am.leaves(self.be, rs, pks, msgs) if rs else []
        for b in range(held // B, len(self.leaves) // B):                 # the blocks this push completed
            assert len(self.tops) == b
            self.tops.append(am.tree_top(self.be, self.leaves[B * b: B * (b + 1)]))

    def finish(self, n):
        """-> (root, aggregate bytes) of the first n lanes; reads the state, writes none of it"""
        if n == 0:
            return None, bytes(32)
        B = self.B
        tops = [list(t) for t in self.tops[:n // B]]                      # a copy: the workspace of the call
        if n % B:
            tops.append(am.tree_top(self.be, self.leaves[B * (n // B): n]))
        root = am.root_of(self.be, am.tree_top(self.be, tops), n)
        a = am.coeffs_of_root(self.be, root, n)
        e_agg = sum(x * y for x, y in zip(a, self.es[:n])) % am.Q
        return root, b"".join(self.rs[:n]) + e_agg.to_bytes(32, "little")


@pytest.fixture(scope="module")
def model(oracle):
    """N_MAX honest signatures (the C oracle signs: byte-identical to pymodel.sign), the caching pymodel back-end, and
    the one-shot root and aggregate of every prefix"""
    rng = np.random.default_rng(0xA66A)
    s = rng.integers(0, 256, size=(2, N_MAX, 32), dtype=np.uint8)
    s[:, :, 31] &= 0x3F
    s[:, :, 0] |= 1
    msgs = rng.integers(0, 256, size=(N_MAX, 80), dtype=np.uint8)
    pks, sigs = oracle.keygen_sign_many(s[0], s[1], msgs)
    be = cached(am.pymodel_backend())
    want = {0: (None, bytes(32))}
    for n in range(1, N_MAX + 1):
        rs = [bytes(x)[:49] for x in sigs[:n]]
        root = am.root_of(be, am.tree_top(be, am.leaves(be, rs, pks[:n], msgs[:n])), n)
        want[n] = (root, am.aggregate(be, sigs[:n], pks[:n], msgs[:n]))
    return be, sigs, pks, msgs, want


def splits(n):
    """every way to cut n lanes into at most three pushes, empty pushes included"""
    return [(a, b - a, n - b) for a in range(n + 1) for b in range(a, n + 1)]


@pytest.mark.parametrize("B", [2, 4, 8])
def test_model_of_the_aggregator_equals_the_one_shot_aggregate(model, B):
    be, sigs, pks, msgs, want = model
    seen = {}                                    # the state after a sequence of pushes depends on their sum alone
    for n in range(1, N_MAX + 1):
        for cut in splits(n):
            ag, lo = ModelAggregator(be, B), 0
            for cnt in cut:
                ag.push(sigs[lo:lo + cnt], pks[lo:lo + cnt], msgs[lo:lo + cnt])
                lo += cnt
            assert len(ag.tops) == n // B
            state = (tuple(map(tuple, ag.leaves)), tuple(map(tuple, ag.tops)), tuple(ag.rs), tuple(ag.es))
            if n in seen:                        # ... so every prefix is finished once per n, and every split lands there
                assert state == seen[n], (n, cut)
                continue
            seen[n] = state
            for take in itertools.chain(range(n, -1, -1), range(n + 1)):          # descending, then ascending
                assert ag.finish(take) == want[take], (B, n, cut, take)
            assert (tuple(map(tuple, ag.leaves)), tuple(map(tuple, ag.tops)), tuple(ag.rs), tuple(ag.es)) == state


def test_model_blocks_are_subtrees(model):
    """the fact the object rests on: the tree over the tops of aligned blocks of 2^t leaves, the
    ragged last one by the same odd-node rule, is the level-by-level tree"""
    be, sigs, pks, msgs, want = model
    lv = am.leaves(be, [bytes(x)[:49] for x in sigs], pks, msgs)
    for n in range(1, N_MAX + 1):
        top = am.tree_top(be, lv[:n])
        for B in (2, 4, 8, 16):
            tops = [am.tree_top(be, lv[lo:min(lo + B, n)]) for lo in range(0, n, B)]
            assert am.tree_top(be, tops) == top, (n, B)
