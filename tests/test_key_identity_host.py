"""What identifies a key on the device, on the CPU (no GPU): the lane and row sources of ssa_dedup.hpp and the one
fingerprint over their words (host-compiled, tests/csrc/key_identity_main.cpp, run as a child process), against a
SipHash-2-4 written here from the paper (Aumasson, Bernstein 2012) and checked on its published vector."""
import os
import shutil
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "csrc", "key_identity_main.cpp")
EXE = os.path.join(HERE, "csrc", "key_identity_main.out")
M = (1 << 64) - 1


def siphash24(key, msg):
    k0, k1 = int.from_bytes(key[:8], "little"), int.from_bytes(key[8:], "little")
    v = [k0 ^ 0x736f6d6570736575, k1 ^ 0x646f72616e646f6d, k0 ^ 0x6c7967656e657261, k1 ^ 0x7465646279746573]
    rotl = lambda x, b: ((x << b) | (x >> (64 - b))) & M      # noqa: E731

    def rounds(k):
        for _ in range(k):
            v[0] = (v[0] + v[1]) & M; v[1] = rotl(v[1], 13) ^ v[0]; v[0] = rotl(v[0], 32)      # noqa: E702
            v[2] = (v[2] + v[3]) & M; v[3] = rotl(v[3], 16) ^ v[2]                              # noqa: E702
            v[0] = (v[0] + v[3]) & M; v[3] = rotl(v[3], 21) ^ v[0]                              # noqa: E702
            v[2] = (v[2] + v[1]) & M; v[1] = rotl(v[1], 17) ^ v[2]; v[2] = rotl(v[2], 32)      # noqa: E702
    padded = msg + bytes(7 - len(msg) % 8) + bytes([len(msg) & 0xFF])
    for i in range(0, len(padded), 8):
        m = int.from_bytes(padded[i:i + 8], "little")
        v[3] ^= m
        rounds(2)
        v[0] ^= m
    v[2] ^= 0xFF
    rounds(4)
    return v[0] ^ v[1] ^ v[2] ^ v[3]


def test_the_python_siphash_gives_the_published_vector():
    assert siphash24(bytes(range(16)), bytes(range(15))) == 0xa129ca6149be45e5


@pytest.fixture(scope="module")
def run():
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not available")
    csrc = os.path.join(os.path.dirname(HERE), "schnorr-sig_amd", "csrc")
    deps = [SRC] + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".hpp")]
    if not os.path.exists(EXE) or any(os.path.getmtime(d) > os.path.getmtime(EXE) for d in deps):
        subprocess.check_call(["hipcc", "--cuda-host-only", "-x", "hip", "-O2", SRC, "-o", EXE])

    def go(cases):
        """cases: (kind, k0, k1, index, misalign, bytes, flags or None) -> per case (words, fingerprint, equals itself)"""
        text = "".join("%s %x %x %x %x %s %s\n" % (kind, k0, k1, index, mis, data.hex(), fl.hex() if fl is not None else "-")
                       for kind, k0, k1, index, mis, data, fl in cases)
        r = subprocess.run([EXE], input=text, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (r.stdout[-500:], r.stderr[-2000:])
        out = [[int(t, 16) for t in ln.split()] for ln in r.stdout.splitlines()]
        assert len(out) == len(cases)
        return [(o[:-2], o[-2], o[-1]) for o in out]
    return go


def _key(rng):
    return int(rng.integers(0, 1 << 63)) * 2 + int(rng.integers(0, 2)), int(rng.integers(0, 1 << 63)) * 2 + 1


def _sip(k0, k1, msg):
    return siphash24(k0.to_bytes(8, "little") + k1.to_bytes(8, "little"), msg)


def test_affine_lanes_and_rows(run):
    """the 12 words of the key and the flag as 0 / 1, from any address, and SipHash-2-4 of the 97 bytes"""
    rng = np.random.default_rng(2201)
    n = 5
    pks = rng.integers(0, 256, size=(n, 96), dtype=np.uint8)
    cases, want = [], []
    for flags in (None, bytes([0, 1, 0x80, 0, 0xFF])):
        for mis in (0, 1, 4, 7):
            for i in range(n):
                k0, k1 = _key(rng)
                cases.append(("AL", k0, k1, i, mis, pks.tobytes(), flags))
                want.append((i, 1 if flags is not None and flags[i] else 0, k0, k1))
                if flags is not None and mis == 0:          # the same key as a row of a cache
                    cases.append(("AR", k0, k1, i, 0, pks.tobytes(), flags))
                    want.append(want[-1])
    assert {w[1] for w in want} == {0, 1}
    for (words, fp, same), (i, flag, k0, k1) in zip(run(cases), want):
        assert len(words) == 13 and same == 1
        assert b"".join(w.to_bytes(8, "little") for w in words[:12]) == pks[i].tobytes()
        assert words[12] == flag                              # null, 0 -> 0; 1, 0x80, 0xff -> 1
        assert fp == _sip(k0, k1, pks[i].tobytes() + bytes([flag]))


def test_wire_lanes_and_rows(run):
    """record i of a 130-byte array gives its 49 bytes: six words and the flag byte; SipHash-2-4 of the 49 bytes"""
    rng = np.random.default_rng(2202)
    n = 6
    rec = rng.integers(0, 256, size=(n, 130), dtype=np.uint8)
    rec[0, 48], rec[1, 48], rec[2, 48] = 0x00, 0x80, 0xFF
    rows = np.zeros((n, 56), dtype=np.uint8)                # what ky_k_decompress stores: the lane's seven words
    rows[:, :49] = rec[:, :49]
    cases, want = [], []
    for mis in (0, 3, 6):
        for i in range(n):
            k0, k1 = _key(rng)
            cases.append(("WL", k0, k1, i, mis, rec.tobytes(), None))
            cases.append(("WR", k0, k1, i, 0, rows.tobytes(), None))
            want += [(i, k0, k1)] * 2
    for (words, fp, same), (i, k0, k1) in zip(run(cases), want):
        assert len(words) == 7 and same == 1
        assert b"".join(w.to_bytes(8, "little") for w in words) == rec[i, :49].tobytes() + bytes(7)
        assert fp == _sip(k0, k1, rec[i, :49].tobytes())


def test_fingerprints_of_edge_words(run):
    """all-zero and all-ones words and keys, both lengths"""
    cases, want = [], []
    for fill in (0x00, 0xFF):
        for k0, k1 in ((0, 0), (M, M), (0x0706050403020100, 0x0f0e0d0c0b0a0908)):
            cases.append(("AL", k0, k1, 0, 0, bytes([fill] * 96), bytes([fill])))
            want.append(_sip(k0, k1, bytes([fill] * 96) + bytes([1 if fill else 0])))
            cases.append(("WL", k0, k1, 0, 0, bytes([fill] * 130), None))
            want.append(_sip(k0, k1, bytes([fill] * 49)))
    assert [fp for _, fp, _ in run(cases)] == want
