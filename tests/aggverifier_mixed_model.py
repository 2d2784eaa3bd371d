"""A block against the pool (ssa_aggverifier_push_mixed) as plain Python, beside
tests/aggregate_model.py: what the streaming aggregate verifier holds once it can take lanes from a streaming aggregator,
and what finish does with them.

    [e_agg - S]G  =  sum over the unknown lanes of a_i (R_i - h_i P_i),      S = sum over the known lanes of a_i s_i mod q

A known lane holds the pool's leaf and the pool's scalar and nothing else; an unknown lane holds what the model of
tests/test_aggverifier_host.py holds.  Nothing here knows how the GPU lays anything out."""
import aggregate_model as am
import pymodel as pm

UNKNOWN = 0xFFFFFFFF


class ModelPool:
    """what a mixed push reads of an ssa_aggregator: the leaves and the scalars of the lanes held, by place"""

    def __init__(self, leaves, scalars):
        assert len(leaves) == len(scalars)
        self.leaves, self.es = [list(v) for v in leaves], [int(s) for s in scalars]


class MixedModelVerifier:
    """ssa_aggverifier with section 34's byte per lane.  mul(k, point), decode(r49, pk96) as in ModelVerifier of
    tests/test_aggverifier_host.py: the model's point multiplication and (status and point of R, the key's coordinates,
    key on the curve)."""

    def __init__(self, backend, B, mul, decode):
        self.be, self.B, self.mul, self.decode = backend, B, mul, decode
        self.rpts, self.ppts, self.hs, self.bad, self.known, self.leaves, self.tops = [], [], [], [], [], [], []

    def _reduce(self, held):
        B = self.B
        for b in range(held // B, len(self.leaves) // B):                 # the blocks this push completed
            assert len(self.tops) == b
            self.tops.append(am.tree_top(self.be, self.leaves[B * b: B * (b + 1)]))

    def push_mixed(self, pool, places, rs, pks, msgs):
        """places[i]: UNKNOWN or a place of the pool; rs, pks, msgs: the unknown lanes alone, in block order.
        Refusals are the host form's: ValueError, nothing changed."""
        places = list(places)
        u = sum(p == UNKNOWN for p in places)
        if u != len(rs) or u != len(pks) or u != len(msgs):
            raise ValueError("the call brings as many lanes as the list has sentinels")
        if any(p != UNKNOWN and not 0 <= p < len(pool.leaves) for p in places):
            raise ValueError("a place the pool does not hold")
        held = len(self.leaves)
        rs = [bytes(r) for r in rs]
        fresh = am.leaves(self.be, rs, pks, msgs) if rs else []
        j = 0
        for p in places:
            if p == UNKNOWN:
                r, pk, m = rs[j], pks[j], msgs[j]
                st, pt, px, py, on = self.decode(r, bytes(pk))
                ok = st == "ok" and px is not None and py is not None and on
                self.bad.append(not ok)
                self.rpts.append(pt if ok else None)                      # (None: the sentinel, adds nothing)
                self.ppts.append(pm.pt_neg((px, py)) if ok else None)
                self.hs.append(pm.scalar_from_digest(self.be[1](r[:48], bytes(pk), bytes(m))))
                self.leaves.append(list(fresh[j]))
                self.known.append(False)
                j += 1
            else:                                                         # a copy: the pool may change afterwards
                self.bad.append(False)
                self.rpts.append(None)
                self.ppts.append(None)
                self.hs.append(pool.es[p])                                # the h slot holds the pool's scalar
                self.leaves.append(list(pool.leaves[p]))
                self.known.append(True)
        self._reduce(held)

    def push(self, rs, pks, msgs):
        self.push_mixed(ModelPool([], []), [UNKNOWN] * len(rs), rs, pks, msgs)

    def state(self):
        return (tuple(map(tuple, self.leaves)), tuple(map(tuple, self.tops)), tuple(self.hs), tuple(self.bad),
                tuple(self.known), tuple(map(repr, self.rpts)), tuple(map(repr, self.ppts)))

    def root(self, n):
        B = self.B
        tops = [list(t) for t in self.tops[:n // B]]                      # a copy: the workspace of the call
        if n % B:
            tops.append(am.tree_top(self.be, self.leaves[B * (n // B): n]))
        return am.root_of(self.be, am.tree_top(self.be, tops), n)

    def known_sum(self, n):
        if n == 0 or not any(self.known[:n]):
            return 0
        a = am.coeffs_of_root(self.be, self.root(n), n)
        return sum(a[i] * self.hs[i] for i in range(n) if self.known[i]) % am.Q

    def finish(self, n, e_agg):
        """-> (root, verdict) of the first n lanes under e_agg; reads the state, writes none of it"""
        if e_agg >= am.Q:                                                 # the canonical check is on e_agg itself
            return None, am.MALFORMED
        if n == 0:
            return None, am.OK if e_agg == 0 else am.INVALID_SIGNATURE
        root = self.root(n)
        if any(self.bad[:n]):
            return root, am.MALFORMED
        a = am.coeffs_of_root(self.be, root, n)
        unknown = [i for i in range(n) if not self.known[i]]              # the ascending list of unknown places
        s = sum(a[i] * self.hs[i] for i in range(n) if self.known[i]) % am.Q
        d = (e_agg - s) % am.Q
        if not unknown:                                                   # no MSM: e_agg equals S, or not
            return root, am.OK if d == 0 else am.INVALID_SIGNATURE
        left = None
        for i in unknown:                                                 # row j is place i, with the coefficient of place i
            left = pm.pt_add(left, self.mul(a[i], self.rpts[i]))
            left = pm.pt_add(left, self.mul(a[i] * self.hs[i] % am.Q, self.ppts[i]))
        right = self.mul(d, pm.default_params().generator())
        return root, am.OK if left == right else am.INVALID_SIGNATURE
