"""Independent model of hierarchical key derivation (reference src/derivation.rs), built from the standard library's
hmac / hashlib and the big-int curve model oracle/pymodel.py.  Test infrastructure only.

Scalars are Python ints, points pymodel tuples (None = the identity), chain codes 32-byte strings.  parse(I_L) is
Scalar::from_bytes_non_canonical read as the full reduction mod q of the little-endian 256-bit value."""
import hashlib
import hmac

from pymodel import Q, default_params, pt_add, pt_compress, pt_decompress, pt_mul  # noqa: F401

MASTER_KEY = b"Cheetah - Master extended key seed"
HARDENED = 1 << 31


def hmac512(key, msg):
    return hmac.new(bytes(key), bytes(msg), hashlib.sha512).digest()


def parse(b32):
    return int.from_bytes(b32, "little") % Q


def index_bytes(i):
    return int(i).to_bytes(4, "little")


def is_hardened(i):
    return int(i) >= HARDENED


def generator():
    return default_params().generator()


def pub(sk):
    return pt_mul(sk, generator())


def master(seed):
    """generate_master_key -> (sk, cc) or None"""
    mac = hmac512(MASTER_KEY, seed)
    sk = parse(mac[:32])
    return None if sk == 0 else (sk, mac[32:])


def derive_private(sk, cc, i, pk49=None):
    """ExtendedPrivateKey::derive_private -> (sk', cc') or None.  pk49: compress([sk]G), when the caller has it."""
    if is_hardened(i):
        msg = bytes(17) + sk.to_bytes(32, "little") + index_bytes(i)
    else:
        msg = (pk49 if pk49 is not None else pt_compress(pub(sk))) + index_bytes(i)
    mac = hmac512(cc, msg)
    child = (parse(mac[:32]) + sk) % Q
    return None if child == 0 else (child, mac[32:])


def derive_public(sk, cc, i, pk49=None):
    """ExtendedPrivateKey::derive_public -> (P', cc') or None"""
    r = derive_private(sk, cc, i, pk49)
    return None if r is None else (pub(r[0]), r[1])


def derive_normal_public(pk, cc, i):
    """ExtendedPublicKey::derive_normal_public -> (P', cc') or None (hardened index, T = O); P' may be the identity"""
    if is_hardened(i):
        return None
    mac = hmac512(cc, pt_compress(pk) + index_bytes(i))
    t = pt_mul(parse(mac[:32]), generator())
    if t is None:
        return None
    return pt_add(t, pk), mac[32:]


def xprv_bytes(sk, cc):
    return sk.to_bytes(32, "little") + bytes(cc)


def xpub_bytes(pk, cc):
    return pt_compress(pk) + bytes(cc)
