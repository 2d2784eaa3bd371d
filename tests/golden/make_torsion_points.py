"""Derives the exact-order torsion points of tests/torsion_points.py with the Python model (oracle/pymodel.py).

    python tests/golden/make_torsion_points.py        # prints the POINTS literal

The group order is N = Q * COFACTOR with COFACTOR = 2 * 5 * 29 * 181 * ...  The parts of prime order 29 and 181 are
[N / p]R for the first decompressed point R of small x (x = (k, 0, 0, 0, 0, 0), k = 0, 1, ...) for which the multiple
is not the identity; the parts of order 2 and 5 are the keys the suite already has (pymodel.SMALL_ORDER_POINTS, derived
the same way).  The composite orders are sums of parts of coprime prime orders -- [N / 58]R alone usually has order 29
or 2, not 58.  tests/test_torsion_points_host.py proves every order and that this script reproduces the literals."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import pymodel as m   # noqa: E402

N = m.Q * m.COFACTOR
COMPOSITES = {58: (2, 29), 145: (5, 29), 290: (2, 5, 29), 362: (2, 181)}


def prime_part(p):
    """([N / p]R, k) for the smallest k >= 0 whose point R of x = k gives a point of order exactly p"""
    assert N % p == 0 and (N // p) % p != 0, "p must divide the group order exactly once"
    k = 0
    while True:
        r = m.pt_decompress_x(m.f6(k, 0, 0, 0, 0, 0))
        if r is not None:
            t = m.pt_mul(N // p, r)
            if t is not None:
                assert m.pt_mul(p, t) is None
                return t, k
        k += 1


def derive():
    parts = {2: m.SMALL_ORDER_POINTS[2], 5: m.SMALL_ORDER_POINTS[5]}
    seeds = {}
    for p in (29, 181):
        parts[p], seeds[p] = prime_part(p)
    points = {29: parts[29], 181: parts[181]}
    for o, primes in COMPOSITES.items():
        t = None
        for p in primes:
            t = m.pt_add(t, parts[p])
        points[o] = t
    return points, seeds


def main():
    points, seeds = derive()
    print("# small x of R: %s" % ", ".join("order %d: x = %d" % kv for kv in sorted(seeds.items())))
    print("POINTS = {")
    for o in sorted(points):
        x, y = points[o]
        print("    %d: ((%s),\n        (%s))," % (o, ", ".join(map(str, x)), ", ".join(map(str, y))))
    print("}")


if __name__ == "__main__":
    main()
