""""Several contexts may be used concurrently" (include/schnorr_sig_amd.h): four threads, each with its own engine, run
steps of tests/callscript.py side by side -- a cold key-cache insert, key-set builds, the constant-time table build, a
self-check of the shared comb and calls of several slices beside plain verifications -- and every result must equal the
one the same step gave when its script ran alone.  tools/soak_threads.py is the long soak; this is the suite's quick
version."""
import ctypes as C
import os
import struct
import threading
import time

import numpy as np
import pytest

import callscript as cs

pytestmark = pytest.mark.gpu

THREADS = 4
ALT_SEED = 500000       # the steps of the engine with another parameter blob have seeds of their own


def _step(family, variant, n, seed_shift=0):
    s = next(s for s in cs.FAMILIES[family] if s.variant == variant and s.n == n)
    return cs.Step(s.family, s.variant, s.n, s.seed + seed_shift)


def _plans():
    """per thread, three rounds of steps; every round of every thread mixes families, the aggregate side among them"""
    sl = cs.SLICED
    new = [s for s in sl[14:] if cs.slicing(s) is True]
    lanes = [s for s in sl[14:] if cs.slicing(s) == "lanes"]
    assert len(new) == 5 and len(lanes) == 3
    alt = cs.N_OF
    return [
        # 0: a 16-bit comb for G; a cold cache insert, the constant-time table build, a key-set build, self-checks; the
        #    aggregate validator and the streaming aggregator walk that comb
        [[_step("verify_many_cached", "T.c32.host", 3073), _step("verify_many", "auto.T.host", 10496),
          _step("selfcheck", "ctx", 0), _step("verify_aggregate", "honest.host", 3073), _step("aggregator", "screened", 257)],
         [_step("verify_many_indexed", "ladder.T.host", 63), _step("keygen_sign_many", "ct", 63),
          _step("verify_batch_screened", "c32.host", 20000), _step("verify_aggregate", "mid.dev", 257),
          _step("aggregator", "index.admission", 1500)],
         [_step("selfcheck", "keyset", 0), _step("verify_batch_msm", "c32.host.bad", 3073),
          _step("verify_many_screened", "T.c32.host", 20000), _step("verify_aggregate", "last.dev", 20000),
          _step("aggregator", "cached", 1500)]],
        # 1: 5000-lane slices: every call runs over three of them, on the context and its twin (the new sliced steps but
        #    those of callscript.LANE_SLICED, which this engine refuses: thread 3 has them)
        [sl[0:5] + new[0:2], sl[5:10] + new[2:4], sl[10:14] + new[4:5]],
        # 2: another parameter blob (its own sponge layout): nothing of it may leak into the other contexts
        [[_step("verify_many", "auto.N.host", 7680, ALT_SEED), _step("hash_message_many", "len7", 257, ALT_SEED),
          _step("keygen_sign_many", "ct.keyed", 1000, ALT_SEED), _step("aggregate", "check.host.honest", 513, ALT_SEED),
          _step("aggregate", "check.dev.bad", 257, ALT_SEED)],
         [_step("verify_many_dedup", "T.host", 257, ALT_SEED), _step("verify_keyed_many", "T.host", 10497, ALT_SEED),
          _step("selfcheck", "ctx", 0, ALT_SEED), _step("verify_aggregates", "edges.host", alt["edges"], ALT_SEED),
          _step("verify_aggregates", "many.dev", alt["many"], ALT_SEED)],
         [_step("verify_many_cached", "T.c32.host", 3073, ALT_SEED), _step("rescue_hash_many", "w8", 257, ALT_SEED),
          _step("sign_many_indexed", "ct.keyed", 257, ALT_SEED), _step("aggverifier", "wire", 1500, ALT_SEED)]],
        # 3: its engine, key cache and signer set are closed and made again between the rounds; the first engine has
        #    5000-lane lane slices, and the first round holds the sliced steps that need them
        [[_step("verify_keyed_many_cached", "T.c32.host", 3073), _step("sign_many_indexed", "tp", 63),
          _step("xprv_derive_many", "priv", 257), _step("aggregate_valid_keyed_cached", "host", 257)] + lanes,
         [_step("verify_many_cached", "N.c32.host", 257), _step("rng_signers", "indexed.ct", 257),
          _step("verify_many", "coop.TF.host", 1000), _step("selfcheck", "cache", 0),
          _step("aggregator", "index.admission", 1500)],
         [_step("verify_many", "auto.T.dev", 10497), _step("msm_partial", "c32.host", 4095),
          _step("verify_many_indexed", "ladder.N.dev", 257), _step("aggverifier", "mixed.wire.require2", 257)]],
    ]


def _alt_blob():
    """capacity-first sponge, padded, digest from state[4..8] (variant 2 of test_alternative_parameter_blobs)"""
    import schnorr_sig_amd as ssa
    b = bytearray(ssa.Engine.default_params())
    struct.pack_into("<IIiIII", b, 8, 7, 4, -1, 1, 4, 0)
    return bytes(b)


def _engines(blob):
    """the four engines of one phase, made by the main thread: the environment is changed and restored here, before any
    thread runs (the library reads it with getenv when a context is created)"""
    import schnorr_sig_amd as ssa

    def cut(*names):
        old = {k: os.environ.get(k) for k in names}
        os.environ.update({k: str(cs.SLICE) for k in old})
        try:
            return ssa.Engine(0)
        finally:
            for k, v in old.items():
                if v is None:
                    del os.environ[k]
                else:
                    os.environ[k] = v
    # (3: the engine of its first round has 5000-lane LANE slices, for the steps of callscript.LANE_SLICED; the engines
    #  the thread makes for its later rounds are plain ones)
    return [ssa.Engine(0, gtab_bits=16), cut("SSA_LANE_SLICE", "SSA_MSM_SLICE"), ssa.Engine(0, params=blob),
            cut("SSA_LANE_SLICE")]


def _orphans_are_refused():
    """a context destroyed while it still owns a key set, a key cache and a signer set: the handles are refused, not
    dangling, and can still be closed"""
    import schnorr_sig_amd as ssa
    lib = ssa._lib
    eng = ssa.Engine(0)
    ks = eng.keyset_create(cs.keyset_keys(None)[1], kind="ladder")
    kc = eng.keycache_create(64)
    ss = eng.signer_set_create(cs.signer_keys())
    eng.close()
    out, st = (C.c_uint64 * 4)(), np.zeros(8, np.uint8)
    assert lib.ssa_keycache_info(kc.handle, out) == ssa.ERR_ARG and lib.ssa_keycache_clear(kc.handle) == ssa.ERR_ARG
    assert lib.ssa_keyset_status(ks.handle, C.c_void_p(st.ctypes.data)) == ssa.ERR_ARG
    assert lib.ssa_signer_set_status(ss.handle, C.c_void_p(st.ctypes.data)) == ssa.ERR_ARG
    for h in (ks, kc, ss):
        h.close()


class Worker(threading.Thread):
    def __init__(self, tid, eng, rounds, barrier, wait_s):
        super().__init__(daemon=True)
        self.tid, self.eng, self.rounds, self.barrier, self.wait_s = tid, eng, rounds, barrier, wait_s
        self.objs = cs.Objs(eng, None)
        self.calls, self.results, self.current, self.error = [], {}, "start", None

    def run(self):
        import schnorr_sig_amd as ssa
        try:
            for r, steps in enumerate(self.rounds):
                if r and self.tid == 3:                      # a new engine, key cache and signer set for this round
                    self.objs.close()
                    self.eng.close()
                    self.eng = ssa.Engine(0)
                    self.objs = cs.Objs(self.eng, None)
                if r == 1 and self.tid == 0:
                    self.current = "orphans"
                    _orphans_are_refused()
                self.barrier.wait(self.wait_s)
                k = self.tid % len(steps)                    # every thread starts its round somewhere else
                for step in steps[k:] + steps[:k]:
                    self.current = "round %d %s" % (r, cs.step_id(step))
                    t0 = time.perf_counter()
                    res = cs.run(step, self.eng, self.objs, None)
                    self.calls.append((t0, time.perf_counter()))
                    self.results[(r, step)] = res
        except Exception as exc:        # noqa: BLE001  (reported by the main thread)
            self.error = "thread %d at %s: %r" % (self.tid, self.current, exc)
            self.barrier.abort()


def test_four_contexts_side_by_side_equal_their_serial_runs(engine, oracle):
    from oracle import Oracle
    blob, plans = _alt_blob(), _plans()
    serial_engs, engs, workers = _engines(blob), _engines(blob), []
    try:
        # ---- the serial reference: each script alone, in its own order, timed
        cs.keyset_keys(engine)
        serial, t0 = {}, time.perf_counter()
        for tid, rounds in enumerate(plans):
            maker = serial_engs[2] if tid == 2 else engine       # honest signatures under the blob they are verified with
            objs = cs.Objs(serial_engs[tid], maker)
            try:
                for r, steps in enumerate(rounds):
                    for step in steps:
                        serial[(tid, r, step)] = cs.run(step, serial_engs[tid], objs, maker)
            finally:
                objs.close()
        serial_s = time.perf_counter() - t0
        alt = Oracle(blob=blob)                              # (the oracle's parameters are process-wide: put back below)
        try:
            for (tid, r, step), res in serial.items():
                cs.check_expected(step, cs.inputs(step, None), res)
                if tid == 2:
                    cs.check_oracle(step, cs.inputs(step, None), res, alt)
        finally:
            Oracle()
        # ---- the same scripts side by side
        wait_s = max(60.0, 20.0 * serial_s)     # 4 threads on one device (<= 4x) and a shared machine's noise: ends trouble,
        barrier = threading.Barrier(THREADS)    # asserts no speed
        workers = [Worker(tid, engs[tid], plans[tid], barrier, wait_s) for tid in range(THREADS)]
        deadline = time.perf_counter() + wait_s
        for w in workers:
            w.start()
        for w in workers:
            w.join(max(0.0, deadline - time.perf_counter()))
        stuck = [w for w in workers if w.is_alive()]
        if stuck:
            pytest.exit("concurrent contexts: thread %d did not finish within %.0f s (at %s); nothing more is run on the GPU"
                        % (stuck[0].tid, wait_s, stuck[0].current), returncode=3)
        errors = [w.error for w in workers if w.error]
        if any("(-2)" in e for e in errors):
            pytest.exit("concurrent contexts: SSA_ERR_HIP -- %s; nothing more is run on the GPU" % errors, returncode=3)
        errors = [e for e in errors if "BrokenBarrierError" not in e] or errors
        assert not errors, errors
        # ---- exact equality, and the proof that the calls did overlap
        for w in workers:
            assert len(w.results) == sum(len(r) for r in plans[w.tid])
            for (r, step), res in w.results.items():
                diff = cs.same(res, serial[(w.tid, r, step)], oracle)
                assert diff is None, "thread %d round %d %s: %s" % (w.tid, r, cs.step_id(step), diff)
        overlaps = [sum(1 for a in w.calls if any(a[0] < b[1] and b[0] < a[1] for o in workers if o is not w for b in o.calls))
                    for w in workers]
        assert all(overlaps), "vacuous: calls that overlapped a call of another thread, per thread: %s" % overlaps
        print("calls that overlapped another thread's, per thread: %s; serial %.2f s" % (overlaps, serial_s))
    finally:
        if not any(w.is_alive() for w in workers):
            for w in workers:
                w.objs.close()
                w.eng.close()
            for e in serial_engs + (engs if not workers else []):
                e.close()
