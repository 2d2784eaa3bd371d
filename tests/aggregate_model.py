"""Half-aggregation of signatures as plain Python: the transcript, the coefficients, the fold and
the point-exact verification, over two callables --

    hash_field_many(rows)            rows of field elements (all of one length) -> one 4-felt digest per row
    hash_message(rx48, pk96, msg)    -> the 32 digest bytes of the challenge hash, before any reduction mod q

Both come from oracle.pymodel (pymodel_backend: the executable specification, slow) or from the C oracle
(oracle_backend: cheap up to 2^17 leaves).  Nothing here knows how the GPU lays the tree out: levels are reduced one
after the other, exactly as the scheme is written down."""
import numpy as np

import pymodel as pm

P, Q = pm.P, pm.Q
TAG_LEAF, TAG_ROOT, TAG_COEFF = 0xA1, 0xA2, 0xA3
COEFF_BITS = 126
OK, INVALID_SIGNATURE, MALFORMED = 0, 2, 3


def pymodel_backend():
    def hash_field_many(rows):
        return [[int(v) for v in pm.rescue_hash_field([int(x) for x in r])] for r in rows]

    def hash_message(rx48, pk96, msg):
        rx = pm.fp6_from_bytes48(bytes(rx48))
        pk = (pm.fp6_from_bytes48(bytes(pk96[:48])), pm.fp6_from_bytes48(bytes(pk96[48:96])))
        return pm.hash_message(rx, pk, bytes(msg))
    return hash_field_many, hash_message


def oracle_backend(orc, threads=16):
    """the C oracle's so_hash_field / so_hash_message, called row by row on the arrays' own memory; large inputs are cut
    into `threads` runs (the calls release the interpreter lock and only read the oracle's parameters)"""
    import ctypes as C
    from concurrent.futures import ThreadPoolExecutor
    lib, vp = orc.lib, C.c_void_p

    def in_runs(m, work):
        if m < 4096 or threads <= 1:
            work(0, m)
            return
        step = (m + threads - 1) // threads
        with ThreadPoolExecutor(threads) as ex:
            list(ex.map(lambda lo: work(lo, min(m, lo + step)), range(0, m, step)))

    def hash_field_many(rows):
        f = np.ascontiguousarray(np.array(rows, dtype=np.uint64))
        m, w = f.shape
        out = np.zeros((m, 4), np.uint64)
        fa, oa, width = f.ctypes.data, out.ctypes.data, C.c_size_t(w)

        def work(lo, hi):
            for i in range(lo, hi):
                lib.so_hash_field(vp(fa + 8 * w * i), width, vp(oa + 32 * i))
        in_runs(m, work)
        return out.tolist()

    def hash_message(rx48, pk96, msg):
        return orc.hash_message(bytes(rx48), bytes(pk96), bytes(msg))

    def hash_message_many(rs49, pks96, msgs):
        m = len(rs49)
        r = np.frombuffer(b"".join(bytes(x)[:49] for x in rs49), np.uint8)
        k = np.frombuffer(b"".join(bytes(x) for x in pks96), np.uint8)
        lens = [len(bytes(x)) for x in msgs]
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        flat = np.frombuffer(b"".join(bytes(x) for x in msgs) + b"\0", np.uint8)
        out = np.zeros((m, 32), np.uint8)
        ra, ka, ma, oa = r.ctypes.data, k.ctypes.data, flat.ctypes.data, out.ctypes.data

        def work(lo, hi):
            for i in range(lo, hi):
                lib.so_hash_message(vp(ra + 49 * i), vp(ka + 96 * i), vp(ma + int(off[i])), C.c_size_t(lens[i]), vp(oa + 32 * i))
        in_runs(m, work)
        return [out[i].tobytes() for i in range(m)]
    return hash_field_many, hash_message, hash_message_many


def digest_felts(h32):
    return [int.from_bytes(h32[8 * k: 8 * k + 8], "little") for k in range(4)]


def leaves(backend, rs49, pks96, msgs):
    """steps 1-2: leaf_i = H(d_i || flag byte || 0xA1)"""
    hfm, hmsg = backend[0], backend[1]
    if len(backend) > 2:                         # a back-end that hashes the messages of all lanes in one go
        digests = backend[2](rs49, pks96, msgs)
    else:
        digests = [hmsg(bytes(r)[:48], bytes(pk), bytes(m)) for r, pk, m in zip(rs49, pks96, msgs)]
    rows = [digest_felts(d) + [bytes(r)[48], TAG_LEAF] for d, r in zip(digests, rs49)]
    return hfm(rows) if rows else []


def tree_top(backend, level):
    """step 3: pairs are hashed, an odd last node of a level moves up unchanged"""
    hfm = backend[0]
    level = [list(v) for v in level]
    while len(level) > 1:
        pairs = [level[2 * k] + level[2 * k + 1] for k in range(len(level) // 2)]
        nxt = hfm(pairs)
        if len(level) % 2:
            nxt = list(nxt) + [level[-1]]
        level = [list(v) for v in nxt]
    return level[0]


def root_of(backend, top, n):
    """step 4"""
    return backend[0]([list(top) + [n, TAG_ROOT]])[0]


def coeffs_of_root(backend, root, n):
    """step 5: 126 bits of the first 16 digest bytes, 0 -> 1"""
    out = []
    for d in backend[0]([list(root) + [i, TAG_COEFF] for i in range(n)]) if n else []:
        a = (int(d[0]) | (int(d[1]) << 64)) & ((1 << COEFF_BITS) - 1)
        out.append(a or 1)
    return out


def coefficients(backend, rs49, pks96, msgs):
    n = len(rs49)
    if n == 0:
        return []
    return coeffs_of_root(backend, root_of(backend, tree_top(backend, leaves(backend, rs49, pks96, msgs)), n), n)


def coeff_bytes(coeffs):
    return np.frombuffer(b"".join(a.to_bytes(16, "little") for a in coeffs), np.uint8).reshape(-1, 16)


def fold(coeffs, sigs81):
    """step 6"""
    return sum(a * int.from_bytes(bytes(s)[49:81], "little") for a, s in zip(coeffs, sigs81)) % Q


def aggregate(backend, sigs81, pks96, msgs):
    """steps 1-7 -> the aggregate's bytes"""
    rs = [bytes(s)[:49] for s in sigs81]
    return b"".join(rs) + fold(coefficients(backend, rs, pks96, msgs), sigs81).to_bytes(32, "little")


def verify(backend, agg, pks96, msgs, pk_inf=None):
    """step 8 with the point arithmetic of pymodel (slow: small n only)"""
    n = len(pks96)
    agg = bytes(agg)
    assert len(agg) == 49 * n + 32
    e_agg = int.from_bytes(agg[49 * n:], "little")
    if e_agg >= Q:
        return MALFORMED
    if n == 0:
        return OK if e_agg == 0 else INVALID_SIGNATURE
    rs = [agg[49 * i: 49 * i + 49] for i in range(n)]
    pts, keys = [], []
    for i in range(n):
        st, r = pm.pt_decompress(rs[i])
        px, py = pm.fp6_from_bytes48(bytes(pks96[i][:48])), pm.fp6_from_bytes48(bytes(pks96[i][48:96]))
        if st != "ok" or px is None or py is None:
            return MALFORMED
        key = None if (pk_inf is not None and pk_inf[i]) else (px, py)
        if not pm.on_curve(key):
            return MALFORMED
        pts.append(r)
        keys.append(key)
    a = coefficients(backend, rs, pks96, msgs)
    left = None
    for i in range(n):
        h = pm.scalar_from_digest(backend[1](rs[i][:48], bytes(pks96[i]), bytes(msgs[i])))
        left = pm.pt_add(left, pm.pt_mul(a[i], pts[i]))
        left = pm.pt_add(left, pm.pt_mul(a[i] * h % Q, pm.pt_neg(keys[i])))
    right = pm.pt_mul(e_agg, pm.default_params().generator())
    return OK if left == right else INVALID_SIGNATURE
