"""Python model of the scalars the device draws (schnorr-sig_amd/csrc/ssa_rng.hpp).

Per call a 44-byte seed S: ChaCha20 key K = S[0:32], nonce N = S[32:44] (RFC 8439, 32-bit block counter).  Lane i of the
call takes B0 = block(K, 2i, N), B1 = block(K, 2i + 1, N) and the scalar from_bytes_wide(B0), or from_bytes_wide(B1)
where the first is 0.  The block function is written from RFC 8439 section 2.3, independent of the kernel."""
import struct

import numpy as np

Q = 0x7AF2599B3B3F22D0563FBF0F990A37B5327AA72330157722D443623EAED4ACCF
SEED_BYTES = 44
RFC8439_KEY = bytes(range(32))
RFC8439_NONCE = bytes.fromhex("000000090000004a00000000")
RFC8439_BLOCK1 = bytes.fromhex(                     # RFC 8439 section 2.3.2, block counter 1
    "10f1e7e4d13b5915500fdd1fa32071c4c7d1f4c733c068030422aa9ac3d46c4e"
    "d2826446079faa0914c2d705d98b02a2b5129cd1de164eb9cbd083e8a2503c4e")
_CONST = (0x61707865, 0x3320646E, 0x79622D32, 0x6B206574)


def chacha20_blocks(key, counters, nonce):
    """RFC 8439 blocks for an array of 32-bit counters -> uint8[len(counters), 64] (vectorised over the counters)"""
    ctr = np.asarray(counters, dtype=np.uint64).astype(np.uint32).reshape(-1)
    k, nn = struct.unpack("<8I", bytes(key)), struct.unpack("<3I", bytes(nonce))
    st = [np.full(ctr.shape, w, np.uint32) for w in _CONST + k] + [ctr] + [np.full(ctr.shape, w, np.uint32) for w in nn]
    x = [a.copy() for a in st]

    def rotl(v, n):
        return (v << np.uint32(n)) | (v >> np.uint32(32 - n))

    def qr(a, b, c, d):
        x[a] += x[b]; x[d] = rotl(x[d] ^ x[a], 16)
        x[c] += x[d]; x[b] = rotl(x[b] ^ x[c], 12)
        x[a] += x[b]; x[d] = rotl(x[d] ^ x[a], 8)
        x[c] += x[d]; x[b] = rotl(x[b] ^ x[c], 7)

    with np.errstate(over="ignore"):
        for _ in range(10):
            qr(0, 4, 8, 12); qr(1, 5, 9, 13); qr(2, 6, 10, 14); qr(3, 7, 11, 15)
            qr(0, 5, 10, 15); qr(1, 6, 11, 12); qr(2, 7, 8, 13); qr(3, 4, 9, 14)
        words = np.stack([a + b for a, b in zip(x, st)], axis=1).astype("<u4")
    return words.view(np.uint8).reshape(-1, 64)


def chacha20_block(key, counter, nonce):
    return chacha20_blocks(key, [counter], nonce)[0].tobytes()


def from_bytes_wide(b64):
    """Scalar::from_bytes_wide: 64 bytes little-endian, mod q"""
    assert len(b64) == 64
    return int.from_bytes(bytes(b64), "little") % Q


def draw_from_blocks(b0, b1):
    """the draw rule on one block pair -> 32 bytes"""
    r = from_bytes_wide(b0)
    if r == 0:
        r = from_bytes_wide(b1)
    return r.to_bytes(32, "little")


def draw(seed, lanes):
    """the scalars of `lanes` (ints, indices in the call) under `seed` -> uint8[len(lanes), 32]"""
    seed = bytes(seed)
    assert len(seed) == SEED_BYTES
    lanes = np.asarray(lanes, dtype=np.uint64).reshape(-1)
    b0 = chacha20_blocks(seed[:32], 2 * lanes, seed[32:])
    b1 = chacha20_blocks(seed[:32], 2 * lanes + 1, seed[32:])
    out = np.zeros((lanes.size, 32), np.uint8)
    for i in range(lanes.size):
        out[i] = np.frombuffer(draw_from_blocks(b0[i].tobytes(), b1[i].tobytes()), np.uint8)
    return out
