"""The admission column of the streaming aggregator and the mixed push that requires a class as
plain Python, beside tests/aggverifier_mixed_model.py.

    ClassPool        what an ssa_aggregator created with SSA_AGGR_HOLD_ADMISSION adds to the pool of section 34: one class
                     per lane, written by the push that admitted it, moved with its lane by the piecewise move of
                     section 30 (gather a piece into a staging array, copy it back, only then the next piece).
    AdmissionVerifier  MixedModelVerifier with a key status per lane and push_mixed_cached: the unknown lanes through a
                     key check, their statuses at their TRUE places, a known lane refused when its class is below
                     `require`; finish lets the key decide, as section 29's does.

Nothing here knows how the GPU lays anything out."""
import aggregate_model as am
from aggverifier_mixed_model import UNKNOWN, MixedModelVerifier, ModelPool

UNSCREENED, SCREENED, KEY_CHECKED = 0, 1, 2
INVALID_PUBLIC_KEY = 1


def move(column, kept, piece):
    """the kept lanes of `column` (a list, or a 2-d numpy array whose SECOND axis is the place: every row is moved alike)
    take the places 0, 1, 2, ... -- as agx_remove_apply walks them: from the first place that changes, in ascending
    pieces of at most `piece` lanes, each gathered into a staging array and copied back before the next is read."""
    kept = list(kept)
    assert all(a < b for a, b in zip(kept, kept[1:])) and all(src >= c for c, src in enumerate(kept))
    m = len(kept)
    f = next((c for c, src in enumerate(kept) if src != c), m)
    two_d = hasattr(column, "shape") and len(column.shape) == 2
    for c0 in range(f, m, piece):
        c1 = min(c0 + piece, m)
        if two_d:
            stage = column[:, kept[c0:c1]].copy()              # the gather: reads the object, writes the staging
            column[:, c0:c1] = stage                           # the copy back: places [c0, c1) alone
        else:
            stage = [column[src] for src in kept[c0:c1]]
            column[c0:c1] = stage
    return m


class ClassPool(ModelPool):
    """ModelPool with the admission column.  `held` lanes are valid; what lies behind is stale, as on the device."""

    def __init__(self, leaves=(), scalars=(), classes=()):
        super().__init__(leaves, scalars)
        assert len(classes) == len(self.es)
        self.adm = [int(c) for c in classes]

    def push(self, leaves, scalars, cls):
        """a push that kept these lanes: the class is the push's, not the lane's"""
        assert cls in (UNSCREENED, SCREENED, KEY_CHECKED)
        self.leaves += [list(v) for v in leaves]
        self.es += [int(s) for s in scalars]
        self.adm += [cls] * len(scalars)

    def remove(self, kept, piece=1 << 30):
        for col in (self.leaves, self.es, self.adm):
            m = move(col, kept, piece)
            del col[m:]

    def drop_front(self, n, piece=1 << 30):
        self.remove(range(n, len(self.es)), piece)

    def reset(self):
        self.leaves, self.es, self.adm = [], [], []


def below(pool, places, require):
    """the known lanes of the list whose class is below `require`: their positions in the list"""
    return [i for i, p in enumerate(places) if p != UNKNOWN and 0 <= p < len(pool.adm) and pool.adm[p] < require]


class AdmissionVerifier(MixedModelVerifier):
    """key_status(pk) -> 0, INVALID_PUBLIC_KEY or MALFORMED: what the key cache says of a key"""

    def __init__(self, backend, B, mul, decode, key_status=lambda pk: 0):
        super().__init__(backend, B, mul, decode)
        self.kst, self.key_status = [], key_status

    def push_mixed(self, pool, places, rs, pks, msgs):
        super().push_mixed(pool, places, rs, pks, msgs)
        self.kst += [0] * len(places)                                     # not checked

    def push_mixed_cached(self, pool, places, rs, pks, msgs, require):
        """the host form: ValueError, nothing changed, for what push_mixed refuses, for a require that is no class, for a
        require > 0 on a pool without the column, and for a named lane below the class"""
        if require not in (0, 1, 2):
            raise ValueError("require is 0, 1 or 2")
        if require and not hasattr(pool, "adm"):
            raise ValueError("the pool records no admission classes")
        if require and below(pool, places, require):
            raise ValueError("a known lane below the required class")
        held = len(self.leaves)
        super().push_mixed(pool, places, rs, pks, msgs)
        self.kst += [0] * len(places)
        j = 0
        for i, p in enumerate(places):
            if p == UNKNOWN:
                self.kst[held + i] = self.key_status(bytes(pks[j]))       # at the lane's place, not at held + j
                j += 1

    def state(self):
        return super().state() + (tuple(self.kst),)

    def finish(self, n, e_agg):
        root, v = super().finish(n, e_agg)
        if n and INVALID_PUBLIC_KEY in self.kst[:n]:                       # the key decides
            return root, INVALID_PUBLIC_KEY
        return root, v
