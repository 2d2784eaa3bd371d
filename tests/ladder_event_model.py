"""CPU model (test infrastructure, Python integers, no GPU) of the per-lane ladder [k]P of csrc/ssa_kernels.hpp
(ladder_init / ladder_steps over the lane's table 1P..16P) for a key P of known order o: which addition of the schedule
meets which exceptional case.

The schedule, restated from csrc/curve.hpp (sc_recode_offset5, sc_win5, sc_top5):
    k' = k + sum_{w < 50} 16 * 32^w                      (k < 2^255)
    digit_w = bits [5w, 5w + 5) of k'  -  16   in [-16, 15]          w = 0..49
    top     = k' >> 250                        in [0, 32]
    [k]P = (..((top P) * 32 + digit_49 P) * 32 + ...) * 32 + digit_0 P
ladder_init forms top P as the table's entry for top <= 16 and as 16P + (top - 16)P -- one mixed addition -- above; then
every window is `gap` = 5 doublings and one mixed addition of the entry |digit| (or its stored opposite).  The subgroup
check [q]P runs the same loop over the width-5 NAF of q (csrc/qnaf.inc: QNAF_DIGIT / QNAF_GAP, parsed here).

With P of order o the accumulator is [m mod o]P, so the class of every addition follows from integers alone:
    ZERO          the digit is 0: the window is its doublings, nothing is added
    GENERIC       acc != O, entry != O, acc != +-entry
    EQUAL         acc == entry:  the addition is a doubling            (H == 0 and R == 0)
    OPPOSITE      acc == -entry: the result is the identity            (H == 0, R != 0)
    FROM_IDENTITY acc == O and the entry is a point                    (Z == 0)
    IDENTITY_ENTRY the entry is the table's (0, 0): digit = 0 mod o    (x2 == 0); the accumulator may be O as well
For o = 2 an entry is its own opposite; the model reports EQUAL, which is the branch jac_madd takes (H == R == 0).
The three classes EQUAL, OPPOSITE and FROM_IDENTITY are the EVENTS: the cases in which the generated window statement
must report 0 and the compiled jac_madd must take over.

walk() returns, for the top digit and for each window, (class, m before the doublings, m after the addition) -- the
host test multiplies those out with pymodel and compares with the textbook sequence."""
import os
import re
from collections import namedtuple

Q = 0x7AF2599B3B3F22D0563FBF0F990A37B5327AA72330157722D443623EAED4ACCF
WINDOWS = 50
OFFSET5 = sum(16 << (5 * w) for w in range(WINDOWS))

ZERO, GENERIC, EQUAL, OPPOSITE, FROM_IDENTITY, IDENTITY_ENTRY = (
    "zero", "generic", "equal", "opposite", "from_identity", "identity_entry")
EVENTS = (EQUAL, OPPOSITE, FROM_IDENTITY)

Step = namedtuple("Step", "cls digit gap m_in m_out")        # m_in: before the doublings; m_out: after the addition
Walk = namedtuple("Walk", "top top_cls top_m steps")         # top_m: the accumulator ladder_init returns


def recode(k):
    """(top, digits) with digits[w] the signed digit of window w (w = 0 is the LAST window of the ladder)"""
    assert 0 <= k < 1 << 255
    kr = k + OFFSET5
    return kr >> 250, [((kr >> (5 * w)) & 31) - 16 for w in range(WINDOWS)]


def recompose(top, digits):
    return (top << 250) + sum(d << (5 * w) for w, d in enumerate(digits))


def scalar_of(top, digits):
    """the k whose recoding is (top, digits); asserts that it is one"""
    k = recompose(top, digits)
    assert 0 <= k < 1 << 255 and recode(k) == (top, list(digits))
    return k


def classify(m, d, o):
    """the class of acc + [d]P for acc = [m]P, P of order o, d a non-zero integer"""
    if d % o == 0:
        return IDENTITY_ENTRY
    if m % o == 0:
        return FROM_IDENTITY
    if (m - d) % o == 0:
        return EQUAL
    if (m + d) % o == 0:
        return OPPOSITE
    return GENERIC


def init_class(top, o):
    """(class, m) of ladder_init: the class is ZERO for top = 0, GENERIC / IDENTITY_ENTRY for a plain table entry
    (top <= 16, no addition), and the class of the addition 16P + (top - 16)P above 16"""
    if top == 0:
        return ZERO, 0
    if top <= 16:
        return (IDENTITY_ENTRY if top % o == 0 else GENERIC), top % o
    return classify(16, top - 16, o), top % o


def _walk(top, schedule, o):
    top_cls, m = init_class(top, o)
    steps = []
    for d, gap in schedule:
        m_in = m
        md = (m << gap) % o
        cls = ZERO if d == 0 else classify(md, d, o)
        m = (md + d) % o
        steps.append(Step(cls, d, gap, m_in, m))
    return Walk(top, top_cls, init_class(top, o)[1], steps)


def walk(k, o):
    """the ladder of [k]P, P of order o: steps[it] is window it of ladder_steps (digit_{49 - it})"""
    top, digits = recode(k)
    return _walk(top, [(digits[WINDOWS - 1 - it], 5) for it in range(WINDOWS)], o)


def qnaf():
    """(digits, gaps) of csrc/qnaf.inc, top digit first"""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "schnorr-sig_amd", "csrc", "qnaf.inc")
    text = open(path).read()
    out = []
    for name in ("QNAF_DIGIT", "QNAF_GAP"):
        body = re.search(name + r"\[QNAF_LEN\] = \{([^}]*)\}", text).group(1)
        out.append([int(v) for v in body.split(",")])
    assert len(out[0]) == len(out[1]) == int(re.search(r"QNAF_LEN = (\d+)", text).group(1))
    return out[0], out[1]


def qnaf_value():
    digits, gaps = qnaf()
    v = 0
    for d, g in zip(digits, gaps):
        v = (v << g) + d
    return v


def walk_q(o):
    """the ladder of the subgroup check [q]P: top = QNAF_DIGIT[0], then one window per further digit"""
    digits, gaps = qnaf()
    assert gaps[0] == 0 and 0 < digits[0] <= 16
    return _walk(digits[0], list(zip(digits[1:], gaps[1:])), o)


def events(w):
    """[(window index or 'top', class)] of the EVENTS of a walk"""
    out = [("top", w.top_cls)] if w.top_cls in EVENTS else []
    return out + [(it, s.cls) for it, s in enumerate(w.steps) if s.cls in EVENTS]


def event_free(k, o=Q):
    """no addition of [k]P is exceptional and no window starts from the identity -- what the honest filler lanes of the
    GPU tests must satisfy (for a prime-order key that is: the top digit is not zero)"""
    w = walk(k, o)
    return w.top_cls == GENERIC and all(s.cls in (GENERIC, ZERO) for s in w.steps) \
        and all(s.m_in != 0 for s in w.steps)


def region(it):
    """'first' (windows 0..9), 'middle' (10..39) or 'last' (40..49)"""
    return "first" if it < 10 else ("last" if it >= 40 else "middle")


def scalar_with_event(o, cls, at, rng):
    """a scalar k whose walk on a key of order o meets `cls` at `at` (a window index, or 'top'); the other digits come
    from rng (a random.Random).  The digits in front of the window are random and the window's digit is solved for;
    FROM_IDENTITY first needs the identity: a zero top digit for window 0, an OPPOSITE one window earlier otherwise.
    At 'top': EQUAL is top = 32, OPPOSITE is top = o (o <= 32); FROM_IDENTITY would need o | 16."""
    def solve(m, want_cls):
        md = m * 32 % o
        return [d for d in range(-16, 16) if d != 0 and classify(md, d, o) == want_cls]

    if at == "top" and (cls == FROM_IDENTITY or (cls == OPPOSITE and o > 32)):
        raise ValueError("no top-digit %s for order %d" % (cls, o))
    for _ in range(100000):
        digits = [rng.randrange(-16, 16) for _ in range(WINDOWS)]
        t = rng.randrange(1, 31)
        if at == "top":
            t = 32 if cls == EQUAL else o
            if t == 32:
                digits[WINDOWS - 1] = rng.randrange(-16, -12)     # keeps k below 2^255
        else:
            fixed = [(at, cls)]
            if cls == FROM_IDENTITY:
                if at == 0:
                    t = 0
                else:
                    fixed.insert(0, (at - 1, OPPOSITE))
            m, ok = init_class(t, o)[1], True
            for it in range(at + 1):
                for fit, fcls in fixed:
                    if fit == it:
                        want = solve(m, fcls)
                        ok = ok and bool(want)
                        if want:
                            digits[WINDOWS - 1 - it] = rng.choice(want)
                m = (m * 32 + digits[WINDOWS - 1 - it]) % o
            if not ok:
                continue
        k = recompose(t, digits)
        if not (0 <= k < 1 << 255) or recode(k) != (t, digits):
            continue
        w = walk(k, o)
        if (at == "top" and w.top_cls == cls) or (at != "top" and w.steps[at].cls == cls):
            return k
    raise ValueError("no scalar for order %d, %s at %s" % (o, cls, at))
