"""Random record chains cut into random BGZF blocks and random block ranges, with the range tables the joining rule of block ranges
must accept and refuse: shared by tests/test_distributed.py (distributed.check_range_anchors) and tests/test_range_join.py (the C
rule, csrc/range_join.h)."""
import numpy as np


def random_chains(n=300, seed=123):
    """-> per chain: (total, ranges, shifted, i, overrun).  total: the stream's length; ranges: per rank (first_block, n_blocks,
    first, next), the true anchors; shifted: the same with range i's first record start off by a few bytes (None where no range
    has a start of its own); overrun: the same with the last record running 5 bytes beyond the stream (None where the last anchor
    is not the stream's end)."""
    rng = np.random.default_rng(seed)
    for _ in range(n):
        header = int(rng.integers(20, 3000))
        sizes = rng.integers(40, 900, int(rng.integers(1, 400)))
        starts = header + np.concatenate(([0], np.cumsum(sizes)[:-1]))          # record starts in the stream
        total = int(header + sizes.sum())
        cuts = [0]
        while cuts[-1] < total:
            cuts.append(min(total, cuts[-1] + int(rng.integers(200, 2500))))   # block boundaries (records straddle them)
        nb = len(cuts) - 1
        world = int(rng.integers(1, 9))
        edges = sorted(set([0, nb] + [int(x) for x in rng.integers(0, nb + 1, world - 1)]))
        ranges = []
        for b0, b1 in zip(edges[:-1], edges[1:]):
            lo, hi = cuts[b0], cuts[b1]
            inside = starts[(starts >= lo) & (starts < hi)]
            first = int(inside[0]) if len(inside) and b0 != 0 else -1           # (the range that starts with the file is vouched for by the header)
            if len(inside):
                after = starts[starts >= hi]
                nxt = int(after[0]) if len(after) else total
            else:
                nxt = header if b0 == 0 and hi <= header else -1                # header blocks only: the header says where the records begin
            ranges.append((b0, b1 - b0, first, nxt))
        shifted, i = None, None
        cand = [k for k, r in enumerate(ranges) if r[2] >= 0]
        if cand:
            i = int(rng.choice(cand))
            b0, n_blocks, first, nxt = ranges[i]
            shifted = list(ranges)
            shifted[i] = (b0, n_blocks, first + int(rng.choice([-7, -1, 1, 33])), nxt)
        last = max(k for k, r in enumerate(ranges) if r[3] >= 0)
        overrun = None
        if ranges[last][3] == total:
            overrun = list(ranges)
            overrun[last] = ranges[last][:3] + (ranges[last][3] + 5,)
        yield total, ranges, shifted, i, overrun
