"""CPU model (test infrastructure, Python integers, no GPU) of the bucket path of the MSM form (csrc/ssa_msm.hip): which
addition meets which exceptional case, and where.

Three parts:
  * the recoding (signed_digits, shape) and a builder that turns a CASE -- a list of (side, point, digit vector) entries
    -- into the sigs / pks / msgs / coeffs32 / pk_inf of the public call ("Exceptional additions");
  * a scalar walk: every point of a case is  k G + u T  for the generator G and at most one small-order point T of order r,
    so it is the pair (k mod q, u mod r), and the walk follows the kernels' order of additions exactly -- the items of a
    bucket (every order: the GPU ranks them by LDS atomics), chunk_sum as written, the tree in groups of tree_group, Horner
    with c doublings per step -- and returns the final pair and the set of events (stage, kind) it met;
  * the case table: every case names the events it must produce.

The walk needs no curve arithmetic; tests/test_msm_edge_model_host.py maps its result to a point with the oracle and
compares with tests/msm_records.py::cpu_partial on the built lanes."""
import itertools
from collections import namedtuple

import numpy as np

Q = 0x7AF2599B3B3F22D0563FBF0F990A37B5327AA72330157722D443623EAED4ACCF
MSM_CHUNK = 8
MSG_LEN = 24
PAD_C8 = 40                # lanes of a c = 8 instance (the engineered ones first, then padding)
PAD_C16 = 4096             # the smallest n at which msm_shape picks 16-bit windows
MAX_BUCKET_ITEMS = 6       # every order of a bucket is walked: 6! = 720 at the most

KINDS = ("same", "opposite", "acc_identity", "addend_identity", "dbl_of_identity", "dbl_to_identity")
STAGES = ("bucket", "chunk_running", "chunk_total", "chunk_k0", "tree1", "tree2", "tree3", "horner")

Shape = namedtuple("Shape", "c windows buckets chunks")


def shape(n):
    """msm_shape"""
    c = 16 if n >= 4096 else 8
    buckets = 1 << (c - 1)
    return Shape(c, (255 + c - 1) // c, buckets, 1 if buckets <= MSM_CHUNK else buckets // MSM_CHUNK)


def shape_of_c(c):
    return shape(PAD_C16 if c == 16 else PAD_C8)


def signed_digits(k, c, windows):
    """write_signed_digits: (digits, carry out of the last window) of the 256-bit integer k"""
    half = 1 << (c - 1)
    carry, out = 0, []
    for j in range(windows):
        raw = ((k >> (j * c)) & ((1 << c) - 1)) + carry
        carry = 0
        if raw >= half:
            raw -= 2 * half
            carry = 1
        out.append(raw)
    return out, carry


def digits_value(digits, c):
    return sum(d << (c * j) for j, d in enumerate(digits))


# ---- elements: (k mod q, u mod r) stands for k G + u T --------------------------------------------------------------
class Group:
    def __init__(self, r=1):
        self.r = r
        self.zero = (0, 0)

    def add(self, a, b):
        return (a[0] + b[0]) % Q, (a[1] + b[1]) % self.r

    def neg(self, a):
        return (-a[0]) % Q, (-a[1]) % self.r

    def mul(self, k, a):
        return k * a[0] % Q, k * a[1] % self.r


class Walk:
    """the additions of the kernels on elements, with the events they meet"""

    def __init__(self, grp):
        self.g = grp
        self.events = set()

    def add(self, stage, acc, q, events=None):
        """jac_madd / jac_add / coop_jac_add: q is None (the (0, 0) sentinel) or an element"""
        ev = self.events if events is None else events
        g = self.g
        if q is None or q == g.zero:
            if acc != g.zero or q is None:    # identity + identity past the buckets happens in every empty chunk and
                ev.add((stage, "addend_identity"))   # group: it is no event, so that no requirement is met by emptiness
            return acc
        if acc == g.zero:
            ev.add((stage, "acc_identity"))
            return q
        if acc == q:                      # H = 0 and R = 0 (a point of order 2 is its own opposite: the code doubles)
            ev.add((stage, "same"))
            res = g.add(acc, acc)
            if res == g.zero:
                ev.add((stage, "dbl_to_identity"))
            return res
        if acc == g.neg(q):
            ev.add((stage, "opposite"))
            return g.zero
        return g.add(acc, q)

    def dbl(self, stage, acc):
        g = self.g
        if acc == g.zero:
            self.events.add((stage, "dbl_of_identity"))
            return acc
        res = g.add(acc, acc)
        if res == g.zero:
            self.events.add((stage, "dbl_to_identity"))
        return res

    def bucket(self, items):
        """the sum of a bucket's items; an event counts only if it occurs under EVERY order of the items (`may`: under
        some order)"""
        if len(items) > MAX_BUCKET_ITEMS:
            raise ValueError("a bucket of %d items: the walk tries every order" % len(items))
        always, may, result = None, set(), None
        for order in set(itertools.permutations(items)):
            ev, acc = set(), self.g.zero
            for q in order:
                acc = self.add("bucket", acc, q, ev)
            assert result is None or result == acc
            result = acc
            always = ev if always is None else always & ev
            may |= ev
        return result, always, may


Lane = namedtuple("Lane", "r_elem p_elem s h")      # r_elem / p_elem: the element of R_i / of -P_i, None = sentinel


def walk_buckets(lanes, n, tree_group=16, r=1):
    """the bucket path on `lanes` (zero-coefficient padding lanes left out: they have no items) of an n-lane call
    -> (final element, events under every bucket order, events under some order)"""
    sh = shape(n)
    grp = Group(r)
    w = Walk(grp)
    may = set()
    # items by (window, bucket): window j holds R's digit of s and -P's digit of s h
    items = {}
    for ln in lanes:
        for elem, k in ((ln.r_elem, ln.s % Q), (ln.p_elem, ln.s * ln.h % Q)):
            digs, carry = signed_digits(k, sh.c, sh.windows)
            assert carry == 0
            for j, d in enumerate(digs):
                if d:
                    q = None if elem is None else (elem if d > 0 else grp.neg(elem))
                    items.setdefault((j, abs(d) - 1), []).append(q)
    bsum = {}
    for key, its in items.items():
        res, always, some = w.bucket(its)
        w.events |= always
        may |= some
        if res != grp.zero:
            bsum[key] = res
    # chunk_sum on every chunk that holds a non-identity bucket; all the others give the identity, with these events
    # (events are recorded only there and in tree groups with a non-identity input: what an empty chunk or group does
    # -- the identity added to and doubled -- every instance does thousands of times, and it proves nothing about a case)
    filled = {(j, b // MSM_CHUNK) for (j, b) in bsum}
    csum = {}
    for (j, ch) in filled:
        k0 = ch * MSM_CHUNK
        running = total = bsum.get((j, k0 + MSM_CHUNK - 1), grp.zero)
        for k in range(k0 + MSM_CHUNK - 2, k0 - 1, -1):
            running = w.add("chunk_running", running, bsum.get((j, k), grp.zero))
            total = w.add("chunk_total", total, running)
        if k0 > 0:
            acc = running
            for bit in range(k0.bit_length() - 2, -1, -1):
                acc = w.dbl("chunk_k0", acc)
                if (k0 >> bit) & 1:
                    acc = w.add("chunk_k0", acc, running)
            total = w.add("chunk_total", total, acc)
        assert total == _chunk_value(grp, bsum, j, k0)
        if total != grp.zero:
            csum[(j, ch)] = total
    # the tree: groups of tree_group, left to right, one level after another
    count, level = sh.chunks, 1
    cur = csum
    while count > 1:
        groups = (count + tree_group - 1) // tree_group
        stage = "tree%d" % level
        nxt = {}
        live = {(j, idx // tree_group) for (j, idx) in cur}
        for (j, gi) in live:
            lo, hi = gi * tree_group, min(gi * tree_group + tree_group, count)
            acc = cur.get((j, lo), grp.zero)
            for idx in range(lo + 1, hi):
                acc = w.add(stage, acc, cur.get((j, idx), grp.zero))
            if acc != grp.zero:
                nxt[(j, gi)] = acc
        cur, count, level = nxt, groups, level + 1
    # Horner from the top window
    acc = cur.get((sh.windows - 1, 0), grp.zero)
    for j in range(sh.windows - 2, -1, -1):
        for _ in range(sh.c):
            acc = w.dbl("horner", acc)
        acc = w.add("horner", acc, cur.get((j, 0), grp.zero))
    return acc, w.events, may | w.events


def _chunk_value(grp, bsum, j, k0):
    tot = grp.zero
    for k in range(k0, k0 + MSM_CHUNK):
        tot = grp.add(tot, grp.mul(k + 1, bsum.get((j, k), grp.zero)))
    return tot


def walk_small(lanes, r=1):
    """the small path: the per-lane records s R_i - s h P_i summed left to right"""
    grp = Group(r)
    acc = grp.zero
    for ln in lanes:
        for elem, k in ((ln.r_elem, ln.s % Q), (ln.p_elem, ln.s * ln.h % Q)):
            if elem is not None:
                acc = grp.add(acc, grp.mul(k, elem))
    return acc


# ---- cases ------------------------------------------------------------------------------------------------------------
# An entry is (side, point, digits):
#   side "R": the lane has an identity key (pk_inf = 1), its R is `point` and its coefficient is the digits' value
#   side "P": the lane's R is the infinity encoding, its key is `point` and its coefficient is t / h mod q for the digits'
#             value t: the digits on -P are exactly `digits`
#   point: ("G", m) = [m]G; ("G", m, "flip") = R with bit 0x40 of its flag byte flipped = -[m]G (side R only);
#          ("T", o) = the point of order o of pymodel.SMALL_ORDER_POINTS (side P only); ("INF",) = the sentinel: the
#          infinity encoding as R, an identity key as P
#   digits: {window: digit}
# An entry may carry ("raw", coefficient bytes as an int, e) instead of digits (side R): the scalar cases.
Case = namedtuple("Case", "name c entries require may r")


def _case(name, c, entries, require, may=(), r=1):
    return Case(name, c, tuple(entries), frozenset(require), frozenset(may), r)


def G(m, digs, flip=False):
    return ("R", ("G", m, "flip") if flip else ("G", m), digs)


def K(k, digs):
    return ("P", ("G", k), digs)


def T(o, digs):
    return ("P", ("T", o), digs)


def SR(digs):
    return ("R", ("INF",), digs)


def SP(digs):
    return ("P", ("INF",), digs)


def _cases_for(c):
    sh = shape_of_c(c)
    top = sh.windows - 1
    W = 1 << c
    out = []

    def add(name, entries, require, may=(), r=1):
        out.append(_case("%s_c%d" % (name, c), c, entries, require, may, r))

    B, CR, CT, CK, H = "bucket", "chunk_running", "chunk_total", "chunk_k0", "horner"
    # -- buckets --
    for k in (2, 3, 4):
        add("bucket_%d_equal" % k, [G(5, {2: 21})] * k, {(B, "same"), (B, "acc_identity")})
    add("bucket_plus_minus_digit", [G(5, {2: 21}), G(5, {2: -21, 3: 1})], {(B, "opposite")})
    add("bucket_flipped_r", [G(5, {2: 21}), G(5, {2: 21}, flip=True)], {(B, "opposite")})
    add("bucket_p_negp_s", [G(5, {2: 21}), G(5, {2: 21}, flip=True), G(9, {2: 21})], {(B, "acc_identity")},
        may={(B, "opposite")})
    add("bucket_key_p_negp_s", [K(5, {2: 21}), K(5, {2: -21, 3: 1}), K(9, {2: 21})], {(B, "acc_identity")},
        may={(B, "opposite")})
    for tag, S in (("idkey", SP), ("infr", SR)):
        for sg, hi in ((1, {}), (-1, {3: 1})):
            sd = dict(hi)
            sd[2] = 21 * sg
            pd = dict(hi)
            pd[2] = 22 * sg
            nm = "%s_%s" % (tag, "pos" if sg > 0 else "neg")
            add("bucket_sentinel_alone_" + nm, [S(sd)], {(B, "addend_identity")})
            add("bucket_sentinel_p_" + nm, [S(pd), G(5, pd)], {(B, "addend_identity"), (B, "acc_identity")})
            add("bucket_p_sentinel_p_" + nm, [G(5, pd), S(pd), G(5, pd)], {(B, "addend_identity"), (B, "same")})
    add("bucket_t2_t2", [T(2, {2: 21})] * 2, {(B, "same"), (B, "dbl_to_identity")}, r=2)
    add("bucket_t2_t2_t2", [T(2, {2: 21})] * 3, {(B, "same"), (B, "dbl_to_identity"), (B, "acc_identity")}, r=2)
    # -- chunks: chunk ch of a window holds the digits 8 ch + 1 .. 8 ch + 8 --
    add("chunk_top_only", [G(5, {2: 24})], {(CR, "addend_identity"), (CT, "same")})
    add("chunk_bottom_only", [G(5, {2: 17})], {(CR, "acc_identity"), (CT, "acc_identity")})
    add("chunk_cancel_then_s", [G(5, {2: 13}), G(5, {2: 12}, flip=True), G(9, {2: 10})],
        {(CR, "opposite"), (CR, "acc_identity"), (CT, "addend_identity")})
    add("chunk_total_opposite", [G(5, {2: 24}), G(10, {2: 23}, flip=True)], {(CT, "opposite")})
    add("chunk_adjacent_same", [G(5, {2: 21}), G(5, {2: 20})], {(CR, "same"), (CR, "acc_identity")})
    add("chunk_k0_running_zero", [G(5, {2: 46}), G(5, {2: 43}, flip=True)],
        {(CR, "opposite"), (CK, "dbl_of_identity"), (CT, "addend_identity"), (CT, "same")})
    add("chunk_k0_8_order2", [T(2, {2: 9}), G(9, {1: 3})], {(CK, "dbl_to_identity"), (CK, "dbl_of_identity")}, r=2)
    add("chunk_k0_40_order5", [T(5, {2: 41}), G(9, {1: 3})], {(CK, "opposite"), (CK, "dbl_of_identity")}, r=5)
    # -- tree: chunk sum of digit d on [m]G is [d m]G; equal sums from (m, d) and (d', m') with m d = m' d' --
    TR = "tree"
    add("tree_single_first", [G(5, {2: 3})], {(TR, "addend_identity")})
    add("tree_single_middle", [G(5, {2: 8 * 7 + 3})], {(TR, "acc_identity"), (TR, "addend_identity")})
    add("tree_single_last", [G(5, {2: 8 * 15 + 3})], {(TR, "acc_identity")})
    add("tree_copy_then_same", [G(97, {2: 57}), G(57, {2: 97})], {(TR, "acc_identity"), (TR, "same")})
    add("tree_copy_then_generic", [G(5, {2: 57}), G(9, {2: 97})], {(TR, "acc_identity")})
    add("tree_same_same_generic", [G(41, {2: 33}), G(33, {2: 41}), G(9, {2: 49})], {(TR, "same")})
    add("tree_opposite_then_generic", [G(41, {2: 33}), G(33, {2: 41}, flip=True), G(9, {2: 49})],
        {(TR, "opposite"), (TR, "acc_identity")})
    add("tree_first_identity", [G(5, {2: 9}), G(9, {2: 17})], {(TR, "acc_identity")})
    add("tree_t2_plus_t2", [T(2, {2: 33}), T(2, {2: 41}), G(9, {1: 3})], {(TR, "same"), (TR, "dbl_to_identity")}, r=2)
    if c == 16:
        # the same events at tree levels 2 and 3 (groups of 16): chunk indices 16 and 256 apart
        add("tree_level2_same", [G(257, {2: 129}), G(129, {2: 257}), G(9, {2: 8 * 48 + 1})],
            {("tree2", "same")})
        add("tree_level2_opposite", [G(257, {2: 129}), G(129, {2: 257}, flip=True), G(9, {2: 8 * 48 + 1})],
            {("tree2", "opposite"), ("tree2", "acc_identity")})
        add("tree_level3_same", [G(2177, {2: 129}), G(129, {2: 2177}), G(9, {2: 8 * 528 + 1})],
            {("tree3", "same")})
        add("tree_level3_opposite", [G(2177, {2: 129}), G(129, {2: 2177}, flip=True), G(9, {2: 8 * 528 + 1})],
            {("tree3", "opposite"), ("tree3", "acc_identity")})
        add("tree_level3_t2_plus_t2", [T(2, {2: 129}), T(2, {2: 2177}), G(9, {1: 3})],
            {("tree3", "same"), ("tree3", "dbl_to_identity")}, r=2)
        add("tree_level2_copy_then_same", [G(257, {2: 8 * 17 + 1}), G(137, {2: 8 * 32 + 1})],
            {("tree2", "acc_identity"), ("tree2", "same")})
    # -- Horner --
    add("horner_top_windows_empty", [G(5, {0: 3, 1: 4, 2: 5})], {(H, "dbl_of_identity"), (H, "acc_identity")})
    add("horner_same", [G(5, {4: 1}), G(5 * W, {3: 1})], {(H, "same"), (H, "addend_identity")})
    add("horner_opposite_lower_filled", [G(5, {4: 1}), G(5 * W, {3: 1}, flip=True), G(9, {2: 3, 0: 7})],
        {(H, "opposite"), (H, "dbl_of_identity"), (H, "acc_identity")})
    add("horner_opposite_nothing_below", [G(5, {1: 1}), G(5 * W, {0: 1}, flip=True)], {(H, "opposite")})
    add("all_coefficients_zero", [], {(H, "dbl_of_identity")})
    add("horner_only_window0", [G(5, {0: 3}), G(9, {0: 77})], {(H, "acc_identity"), (H, "dbl_of_identity")})
    qd, carry = signed_digits(Q - 1, c, sh.windows)
    assert carry == 0
    add("scalar_q_minus_1", [G(5, dict(enumerate(qd))), K(9, dict(enumerate(qd)))], {(B, "acc_identity")})
    add("horner_order2_window_sum", [T(2, {3: 1}), G(9, {0: 3})],
        {(H, "dbl_to_identity"), (H, "dbl_of_identity"), (H, "acc_identity")}, r=2)
    return out


CASES = _cases_for(8) + _cases_for(16)
TREE_GROUPS = (2, 3, 16, 64)

# lin only: e in {0, 1, q - 1} and raw coefficients {1, q - 1, q, q + 1, 2^256 - 1} on lanes 0, 255, 256 and n - 1 of a
# 600-lane instance (sc_reduce256, sc_mul_mod, the block sum over two blocks and a ragged third, wave_sum_mod_q)
SCALAR_N = 600
SCALAR_LANES = (0, 255, 256, SCALAR_N - 1)
SCALAR_E = (0, 1, Q - 1)
SCALAR_COEFFS = (1, Q - 1, Q, Q + 1, 2 ** 256 - 1)
SCALAR_COMBOS = tuple((co, e) for co in SCALAR_COEFFS for e in SCALAR_E)


def scalar_instances():
    """15 instances: instance i puts the combinations i, i + 1, i + 2, i + 3 (mod 15) on the four lanes"""
    return [[SCALAR_COMBOS[(i + k) % len(SCALAR_COMBOS)] for k in range(len(SCALAR_LANES))]
            for i in range(len(SCALAR_COMBOS))]


def required_events(case, tree_group, events):
    """the required events a walk did NOT produce.  A stage "tree" means any tree level; a named level (tree2, tree3)
    counts with the default groups of 16 only."""
    missing = []
    for stage, kind in case.require:
        if stage == "tree":
            if not any(s.startswith("tree") and k == kind for s, k in events):
                missing.append((stage, kind))
        elif stage.startswith("tree") and tree_group != 16:
            continue
        elif (stage, kind) not in events:
            missing.append((stage, kind))
    return sorted(missing)


def case_digits(case, digs):
    sh = shape_of_c(case.c)
    v = [0] * sh.windows
    for j, d in digs.items():
        v[j] = d
    return v


# ---- the builder ------------------------------------------------------------------------------------------------------
Built = namedtuple("Built", "sigs pks msgs coeffs pk_inf lanes active lin r n")


def _le32(v):
    return int(v).to_bytes(32, "little")


def _aff_bytes(pt):
    return b"".join(int(v).to_bytes(8, "little") for v in pt[0] + pt[1])


class Builder:
    """cases -> the arrays of the public call, through the oracle (keygen, sign, compress, decompress, the challenge
    hash).  Padding: one honest lane repeated with coefficient 0."""

    def __init__(self, orc):
        import pymodel
        self.orc = orc
        self.small = pymodel.SMALL_ORDER_POINTS
        self._r = {}
        sk, nonce = _le32(0x1234567), _le32(0x7654321)
        self.pad_msg = bytes(range(MSG_LEN))
        self.pad_pk, inf = orc.keygen(sk)
        assert not inf
        self.pad_sig = orc.sign(sk, nonce, self.pad_pk, self.pad_msg)

    def mul_g(self, m):
        """[m]G as 96 affine bytes"""
        if m not in self._r:
            pk, inf = self.orc.keygen(_le32(m % Q))
            assert not inf
            self._r[m] = pk
        return self._r[m]

    def r49(self, m, flip):
        """(49 bytes of R, the sign of m they decode to)"""
        c49 = bytearray(self.orc.compress(self.mul_g(m)))
        if flip:
            c49[48] ^= 0x40
        dec = self.orc.decompress(bytes(c49))
        assert dec is not None and not dec[1]
        if dec[0] == self.mul_g(m):
            return bytes(c49), 1
        assert dec[0] == self.mul_g(Q - m)
        return bytes(c49), -1

    def h_of(self, sig, pk, msg):
        return int.from_bytes(self.orc.scalar_from_digest(self.orc.hash_message(sig[:48], pk, msg)), "little")

    def lanes_of(self, entries, c, r):
        """-> per entry (sig81, pk96, pk_inf, msg, coefficient as an int below 2^256, Lane)"""
        sh = shape_of_c(c)
        out = []
        for i, (side, point, spec) in enumerate(entries):
            msg = bytes((i * 7 + k) & 0xFF for k in range(MSG_LEN))
            e = (0x1000003 * (i + 1)) % Q
            raw = None
            if isinstance(spec, tuple):              # ("raw", coefficient, e)
                _, raw, e = spec
                t = raw % Q
            else:
                v = [0] * sh.windows
                for j, d in spec.items():
                    v[j] = d
                t = digits_value(v, c)
                assert 0 < t < Q, "the digits must stand for a scalar in (0, q)"
                assert signed_digits(t, c, sh.windows) == (v, 0), "the digit vector must recode to itself"
            if side == "R":
                if point[0] == "INF":
                    c49, r_elem = bytes(48) + b"\x80", None
                else:
                    c49, sign = self.r49(point[1], len(point) > 2)
                    r_elem = (sign * point[1] % Q, 0)
                sig, pk, inf = c49 + _le32(e), bytes(96), 1
                h = self.h_of(sig, pk, msg)
                out.append((sig, pk, inf, msg, t if raw is None else raw, Lane(r_elem, None, t, h)))
            else:
                sig = bytes(48) + b"\x80" + _le32(e)
                if point[0] == "INF":
                    pk, inf, p_elem = bytes(96), 1, None
                elif point[0] == "T":
                    assert point[1] == r
                    pk, inf, p_elem = _aff_bytes(self.small[point[1]]), 0, (0, (-1) % r)
                else:
                    pk, inf, p_elem = self.mul_g(point[1]), 0, ((-point[1]) % Q, 0)
                h = self.h_of(sig, pk, msg)
                assert h % Q
                s = t * pow(h, -1, Q) % Q
                out.append((sig, pk, inf, msg, s, Lane(None, p_elem, s, h)))
        return out

    def build(self, entries, c, r=1, n=None, at=None):
        """the n-lane call of a case: the entries' lanes at the positions `at` (default: the first ones), padding
        elsewhere"""
        n = n or (PAD_C16 if c == 16 else PAD_C8)
        rows = self.lanes_of(entries, c, r)
        at = list(at) if at is not None else list(range(len(rows)))
        assert len(at) == len(rows) <= n
        sigs = np.tile(np.frombuffer(self.pad_sig, np.uint8), (n, 1))
        pks = np.tile(np.frombuffer(self.pad_pk, np.uint8), (n, 1))
        msgs = np.tile(np.frombuffer(self.pad_msg, np.uint8), (n, 1))
        coeffs = np.zeros((n, 32), np.uint8)
        pk_inf = np.zeros(n, np.uint8)
        lin = 0
        for pos, (sig, pk, inf, msg, co, ln) in zip(at, rows):
            sigs[pos] = np.frombuffer(sig, np.uint8)
            pks[pos] = np.frombuffer(pk, np.uint8)
            msgs[pos] = np.frombuffer(msg, np.uint8)
            coeffs[pos] = np.frombuffer(_le32(co), np.uint8)
            pk_inf[pos] = inf
            lin = (lin + ln.s * int.from_bytes(sig[49:], "little")) % Q
        return Built(sigs, pks, msgs, coeffs, pk_inf, [row[5] for row in rows], at, lin, r, n)

    def build_case(self, case, n=None):
        return self.build(case.entries, case.c, case.r, n)

    def build_scalars(self, combos):
        entries = [("R", ("G", 11 + k), ("raw", co, e)) for k, (co, e) in enumerate(combos)]
        return self.build(entries, 8, 1, SCALAR_N, SCALAR_LANES)

    def element_point(self, elem, r=1):
        """k G + u T as an affine tuple (None for the identity), by the oracle"""
        import msm_records as mr
        pt = self.orc.point_mul(elem[0], mr._aff(self.mul_g(1)))
        if elem[1]:
            pt = self.orc.point_add(pt, self.orc.point_mul(elem[1], self.small[r]))
        return pt


def active(b):
    """the arrays of the active lanes only (a zero coefficient adds nothing to either side): cpu_partial's input"""
    at = b.active
    return b.sigs[at], b.pks[at], b.msgs[at], b.coeffs[at], b.pk_inf[at]
