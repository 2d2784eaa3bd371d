"""What the host and GPU tests of the torsion-key ladder share (test infrastructure): the forged records of
tests/golden/torsion_forged.json, their bit-flipped twins, the end-game configurations, and the two wave layouts.

Why a layout: the window statement of the per-lane kernels reports an exceptional addition PER WAVE -- one such lane
sends every lane of its wave to the compiled jac_madd.  In a wave full of torsion keys some lane leaves the statement at
almost every window for the cheap reasons (identity entries, Z = 0), so a lane whose accumulator equals a real table
entry is never the ONLY reason its wave leaves.  The solitary layout puts each special lane alone among 63 honest lanes
whose ladders meet nothing (ladder_event_model.event_free), at lane 0, 31, 32 or 63 of its wave; the crowd layout fills
waves with special lanes, the situation the suite had before."""
import collections
import json
import os

import numpy as np

import ladder_event_model as lem

HERE = os.path.dirname(os.path.abspath(__file__))
MSG_LEN = 24
WAVE = 64
SOLITARY_PLACES = (0, 31, 32, 63)

TAIL_WAVES = 32
TAIL_CONFIGS = ((8, 1), (5, 2))             # (pieces, gens); the second one runs with the grid reversed


def tail_batch(gens):
    """the smallest batch test_end_game_pieces_equal_whole_lanes uses"""
    return (2 + gens) * TAIL_WAVES * WAVE + 1037


Record = collections.namedtuple("Record", "order c sig pk msg h e events")


def load():
    with open(os.path.join(HERE, "golden", "torsion_forged.json")) as f:
        raw = json.load(f)["records"]
    return [Record(r["order"], r["c"], bytes.fromhex(r["sig"]), bytes.fromhex(r["pk"]), bytes.fromhex(r["msg"]),
                   int(r["h"], 16), int(r["e"], 16), [(at if at == "top" else int(at), cls) for at, cls in r["events"]])
            for r in raw]


def arrays(records):
    """(sigs n x 81, pks n x 96, msgs n x MSG_LEN)"""
    def stack(field, w):
        return np.frombuffer(b"".join(getattr(r, field) for r in records), dtype=np.uint8).reshape(-1, w).copy()
    return stack("sig", 81), stack("pk", 96), stack("msg", MSG_LEN)


def twins(sigs):
    """the same signatures with bit 0 of e flipped (e stays below q: the records' e is below 2^250)"""
    t = sigs.copy()
    t[:, 49] ^= 1
    return t


def ladder_cuts(plan):
    """the windows of the ladder of [h]P (pass 1) in front of which a piece of the plan resumes a parked accumulator"""
    return sorted(lo for pas, first, last, lo, hi in plan["pieces"] if pas == 1 and lo > 0)


def parked_identity_records(records, cuts):
    """indices of the records of order 29 / 58 whose accumulator is the identity when a piece parks it"""
    out = []
    for i, r in enumerate(records):
        if r.order in (29, 58):
            steps = lem.walk(r.h, r.order).steps
            if any(steps[c - 1].m_out == 0 for c in cuts):
                out.append(i)
    return out


def layouts(n_special, n_honest):
    """-> (special, honest): for every lane of the batch the index of the special lane it holds, or -1, and the index of
    the honest lane, or -1.  Solitary part: one wave per special lane, the lane at SOLITARY_PLACES[i % 4], 63 honest
    lanes around it (the honest pool is cycled).  Crowd part: whole waves of special lanes in order, the last one filled
    up by starting over."""
    assert n_special > 0 and n_honest >= WAVE - 1
    special, honest, h = [], [], 0
    for i in range(n_special):
        place = SOLITARY_PLACES[i % len(SOLITARY_PLACES)]
        for lane in range(WAVE):
            if lane == place:
                special.append(i)
                honest.append(-1)
            else:
                special.append(-1)
                honest.append(h % n_honest)
                h += 1
    crowd = -(-n_special // WAVE) * WAVE
    special += [i % n_special for i in range(crowd)]
    honest += [-1] * crowd
    return np.array(special), np.array(honest)


def lay_out(special_rows, honest_rows, special, honest):
    """the batch array of a layout: row i is special_rows[special[i]] or honest_rows[honest[i]]"""
    out = np.empty((len(special),) + special_rows.shape[1:], dtype=special_rows.dtype)
    s = special >= 0
    out[s] = special_rows[special[s]]
    out[~s] = honest_rows[honest[~s]]
    return out
