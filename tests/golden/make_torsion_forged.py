"""Forged acceptances under keys outside the prime subgroup -> tests/golden/torsion_forged.json (Python model only).

    python tests/golden/make_torsion_forged.py        # about two minutes

For pk = T of order o, a chosen c in [1, o) and a random e, the signature (R = [e]G + [c]T, e) verifies under batch
semantics (no subgroup check) iff h(R.x, T, msg) = c mod o: then [h]T + [e]G = [c]T + [e]G = R.  R is kept and the
message's counter runs until the hash agrees, about o tries.  Such a lane is the only kind of input that is ACCEPTED after
the per-lane ladder met an exceptional addition -- every other torsion-key lane of the suite answers 2, which is also what
a ladder answers that went wrong at the collision.

Which candidates are kept is decided by tests/ladder_event_model.py on h: a candidate without an event in a window is
dropped; for orders 29 and 58 a pool of candidates is drawn and a greedy cover keeps those that meet most missing GOALS
  * every event class in the first 10, the middle 30 and the last 10 windows (orders >= 29 only),
  * a top-digit event (order 29: top = 29 is 16T + 13T = O),
  * for orders 29 and 58: an identity accumulator at the end of windows 25, 26, 39, 46, 49 -- the piece boundaries of the
    end-game plans the GPU test runs (ssa.debug_tail_plan with SSA_TAIL_WAVES = 32; any of them is enough for the test),
every other order keeps its first candidates.  tests/test_torsion_forged_host.py asserts the conditions on the
committed file and verifies every record with the model and the C oracle."""
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import pymodel as m                 # noqa: E402
import ladder_event_model as lem    # noqa: E402
import torsion_points as tp         # noqa: E402

COUNTS = [(29, 8), (58, 4), (5, 4), (10, 4), (145, 4), (181, 4), (290, 2)]
MSG_LEN = 24
BOUNDARIES = (25, 26, 39, 46, 49)
POOL = {29: 240, 58: 60}          # candidates to choose from; every other order keeps its first `count`


def candidate(rng, o, serial):
    """one forged record: (record dict, walk of h)"""
    prm = m.default_params()
    t = tp.ALL_POINTS[o]
    c = rng.randrange(1, o)
    e = rng.randrange(2, 1 << 250)
    r = m.pt_add(m.pt_mul(e, prm.generator()), m.pt_mul(c, t))
    counter = 0
    while True:
        msg = (b"tors %03d %05d %07d" % (o, serial, counter)).ljust(MSG_LEN, b".")
        assert len(msg) == MSG_LEN
        h = m.scalar_from_digest(m.hash_message(r[0], t, msg, prm))
        if h % o == c:
            break
        counter += 1
    w = lem.walk(h, o)
    rec = {"order": o, "c": c, "sig": (m.pt_compress(r) + e.to_bytes(32, "little")).hex(), "pk": tp.pk96(o).hex(),
           "msg": msg.hex(), "h": "%x" % h, "e": "%x" % e,
           "events": [[str(at), cls] for at, cls in lem.events(w)]}
    return rec, w


def goals_of(o, w):
    g = set()
    if o < 29:
        return g
    for at, cls in lem.events(w):
        g.add(("top",) if at == "top" else (cls, lem.region(at)))
    if o in (29, 58):
        g.update(("park", b) for b in BOUNDARIES if w.steps[b - 1].m_out == 0)
    return g


def main():
    rng = random.Random(0x70F5)
    want = {(cls, reg) for cls in lem.EVENTS for reg in ("first", "middle", "last")}
    want |= {("top",)} | {("park", b) for b in BOUNDARIES}
    records, serial = [], 0
    for o, count in COUNTS:
        pool = []
        while len(pool) < (POOL.get(o, count)):
            serial += 1
            rec, w = candidate(rng, o, serial)
            if any(at != "top" for at, _ in lem.events(w)):          # every record has an event in a window
                pool.append((rec, goals_of(o, w)))
        kept = []
        while len(kept) < count:                                    # greedy cover: the candidate with most missing goals
            best = max(pool, key=lambda rg: len(rg[1] & want))
            pool.remove(best)
            want -= best[1]
            kept.append(best[0])
        records += kept
    # A top-digit event needs top = 29 at order 29 (one h in about 31 among those that fit c); the pool holds several.
    assert not want, "goals not met: %r" % sorted(want)
    with open(os.path.join(HERE, "torsion_forged.json"), "w") as f:
        json.dump({"records": records}, f, indent=1)
        f.write("\n")
    print("%d records, %d candidates" % (len(records), serial))


if __name__ == "__main__":
    main()
