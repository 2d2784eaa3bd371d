"""The leaf index of the streaming aggregator as plain, SEQUENTIAL Python: the table that
agi_k_insert builds and agi_k_lookup walks, and the lazy state machine the library keeps around it.

    Table        an open-addressing table of 64-bit words, fingerprint's upper half << 32 | place, all ones = empty.
                 The fingerprint is SipHash-2-4 under a 128-bit key over the leaf's 32 bytes and one tag byte (33 bytes:
                 the library's dd_fingerprint<5, 33>); it only picks slots.  Equality is decided on the 32 bytes.
    IndexedPool  leaves in arrival order with `indexed`, `stale` and the counters of ssa_aggregator_index_info: pushes and
                 removals touch no table, sync() and lookup() do all the index work.

The device runs the inserts of one launch in no order; the model runs them in whatever order it is given, one after the
other, which is one of the orders the device may take."""
import struct

EMPTY = (1 << 64) - 1
UNKNOWN = 0xFFFFFFFF
TAG = 0xA4                      # AGI_TAG: the constant fifth word
M64 = (1 << 64) - 1


def _rotl(x, b):
    return ((x << b) | (x >> (64 - b))) & M64


def siphash24(key16, data):
    """SipHash-2-4 (Aumasson, Bernstein 2012) of `data` under the 16-byte key -> a 64-bit integer"""
    k0, k1 = struct.unpack("<QQ", bytes(key16))
    v0, v1, v2, v3 = (k0 ^ 0x736f6d6570736575, k1 ^ 0x646f72616e646f6d, k0 ^ 0x6c7967656e657261, k1 ^ 0x7465646279746573)

    def rounds(n):
        nonlocal v0, v1, v2, v3
        for _ in range(n):
            v0 = (v0 + v1) & M64
            v1 = _rotl(v1, 13) ^ v0
            v0 = _rotl(v0, 32)
            v2 = (v2 + v3) & M64
            v3 = _rotl(v3, 16) ^ v2
            v0 = (v0 + v3) & M64
            v3 = _rotl(v3, 21) ^ v0
            v2 = (v2 + v1) & M64
            v1 = _rotl(v1, 17) ^ v2
            v2 = _rotl(v2, 32)

    data = bytes(data)
    tail = len(data) % 8
    body, last = data[:len(data) - tail], data[len(data) - tail:]
    words = [int.from_bytes(body[i:i + 8], "little") for i in range(0, len(body), 8)]
    words.append(int.from_bytes(last, "little") | ((len(data) & 0xFF) << 56))
    for m in words:
        v3 ^= m
        rounds(2)
        v0 ^= m
    v2 ^= 0xFF
    rounds(4)
    return v0 ^ v1 ^ v2 ^ v3


def fingerprint(key16, leaf32):
    leaf32 = bytes(leaf32)
    assert len(leaf32) == 32
    return siphash24(key16, leaf32 + bytes([TAG]))


class Table:
    """`slots` words (a power of two), walks of at most `bound` slots.  leaves: the pool's leaf column, a list of 32-byte
    strings the table refers to by place."""

    def __init__(self, slots, bound, key16=bytes(range(16))):
        assert slots and slots & (slots - 1) == 0
        self.slots, self.bound, self.key = slots, bound, bytes(key16)
        self.clear()

    def clear(self):
        self.words = [EMPTY] * self.slots
        self.overflowed = 0
        self.lost = set()                 # the places whose insert ran into the bound

    def insert(self, leaves, p, hi):
        """agi_k_insert's thread for place p of a launch over [lo, hi)"""
        fp = fingerprint(self.key, leaves[p])
        tag, s = fp >> 32, fp & 0xFFFFFFFF & (self.slots - 1)
        mine = tag << 32 | p
        for _ in range(self.bound):
            cur = self.words[s]
            if cur == EMPTY:
                self.words[s] = mine
                return True
            o = cur & 0xFFFFFFFF
            if cur >> 32 == tag and o < hi and leaves[o] == leaves[p]:
                self.words[s] = min(cur, mine)            # atomicMin: equal upper halves, the lower place wins
                return True
            s = (s + 1) & (self.slots - 1)
        self.overflowed += 1
        self.lost.add(p)
        return False

    def insert_range(self, leaves, lo, hi, order=None):
        for p in (range(lo, hi) if order is None else order):
            assert lo <= p < hi
            self.insert(leaves, p, hi)

    def lookup(self, leaves, indexed, ident):
        """agi_k_lookup's thread for one id"""
        ident = bytes(ident)
        fp = fingerprint(self.key, ident)
        tag, s = fp >> 32, fp & 0xFFFFFFFF & (self.slots - 1)
        for _ in range(self.bound):
            cur = self.words[s]
            if cur == EMPTY:
                return UNKNOWN
            o = cur & 0xFFFFFFFF
            if cur >> 32 == tag and o < indexed and leaves[o] == ident:
                return o
            s = (s + 1) & (self.slots - 1)
        return UNKNOWN


def lowest_places(leaves):
    """the dictionary a look-up is checked against: leaf -> the lowest place that holds it"""
    d = {}
    for p, leaf in enumerate(leaves):
        d.setdefault(bytes(leaf), p)
    return d


class IndexedPool:
    """the host state of an aggregator made with SSA_AGGR_HOLD_INDEX, and the table behind it"""

    def __init__(self, slots=16, bound=128, key16=bytes(range(16))):
        self.leaves = []
        self.table = Table(slots, bound, key16)
        self.indexed, self.stale = 0, True
        self.rebuilds = self.lookups = self.ids = 0
        self.index_work = 0               # table operations so far: pushes and removals must not move it

    # ---- what leaves the index alone
    def push(self, leaves):
        self.leaves.extend(bytes(x) for x in leaves)

    def remove(self, kept):
        """the lanes at the (ascending) places `kept` stay; a removal that changes nothing leaves the index valid"""
        kept = list(kept)
        if kept == list(range(len(self.leaves))):
            return
        self.leaves = [self.leaves[i] for i in kept]
        self.indexed, self.stale = 0, True

    def reset(self):
        self.leaves = []
        self.indexed, self.stale = 0, True

    # ---- where all index work happens
    def sync(self, order=None):
        if self.stale:
            self.table.clear()
            self.stale, self.indexed = False, 0
            self.rebuilds += 1
            self.index_work += 1
        if self.indexed < len(self.leaves):
            self.table.insert_range(self.leaves, self.indexed, len(self.leaves), order)
            self.indexed = len(self.leaves)
            self.index_work += 1

    def lookup(self, ids):
        ids = [bytes(x) for x in ids]
        if not ids:
            return [], 0
        self.sync()
        self.lookups += 1
        self.ids += len(ids)
        places = [self.table.lookup(self.leaves, self.indexed, x) for x in ids]
        return places, sum(1 for p in places if p == UNKNOWN)
