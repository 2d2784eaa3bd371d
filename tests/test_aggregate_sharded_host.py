"""Host-side statements behind the sharded half-aggregation, no GPU: how blocks are dealt to ranks,
and that the tops of blocks of B = 2^t leaves reduce to the top of the whole tree -- the model of tests/aggregate_model.py
over the pure-Python back-end, for every n <= 70."""
import numpy as np
import pytest

import aggregate_model as am
from schnorr_sig_amd.sharding import aggregate_block_range


@pytest.mark.parametrize("B", [1, 2, 4, 512])
@pytest.mark.parametrize("world", [1, 2, 3, 8])
def test_block_ranges_cover_the_lanes_in_whole_blocks(B, world):
    for n in list(range(0, 40)) + [511, 512, 513, 1100, 1537, 1613, 600, 8 * 512, 8 * 512 + 1]:
        blocks = -(-n // B)
        counts, at = [], 0
        for r in range(world):
            lo, hi = aggregate_block_range(n, B, r, world)
            assert lo == at and lo <= hi <= n                            # contiguous, in rank order
            assert lo % B == 0 or lo == n                                # a shard starts on a block boundary
            assert hi % B == 0 or hi == n                                # only the aggregate's last block is ragged
            counts.append(-(-(hi - lo) // B))
            at = hi
            # the restatement: blocks are dealt as evenly as whole numbers allow, earlier ranks first
            base, rem = divmod(blocks, world)
            b_lo = r * base + min(r, rem)
            assert (lo, hi) == (min(b_lo * B, n), min((b_lo + base + (r < rem)) * B, n))
        assert at == n and sum(counts) == blocks and max(counts) - min(counts) <= 1


def test_block_range_refuses_a_block_that_is_no_power_of_two():
    for B in (0, 3, 6, 513):
        with pytest.raises(ValueError):
            aggregate_block_range(100, B, 0, 2)


def block_tops(backend, level, B):
    """what a shard computes: the top of every aligned run of B nodes on its own"""
    return [am.tree_top(backend, level[lo:lo + B]) for lo in range(0, len(level), B)]


def test_block_tops_reduce_to_the_top_of_the_whole_tree():
    hash_rows, seen = am.pymodel_backend()[0], {}

    def cached(rows):            # the same pairs come back for every n and B: each is hashed once
        out = []
        for row in rows:
            key = tuple(int(v) for v in row)
            if key not in seen:
                seen[key] = list(hash_rows([list(key)])[0])
            out.append(seen[key])
        return out
    backend = (cached,)
    rng = np.random.default_rng(0x25B10C)
    level = [[int(v) for v in rng.integers(0, 1 << 62, size=4)] for _ in range(70)]
    whole = {n: am.tree_top(backend, level[:n]) for n in range(1, 71)}
    for B in (1, 2, 4, 8, 64):
        for n in range(1, 71):
            tops = block_tops(backend, level[:n], B)
            assert len(tops) == -(-n // B)
            assert am.tree_top(backend, tops) == whole[n], (B, n)
