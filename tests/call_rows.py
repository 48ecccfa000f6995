"""Count rows [cov, A, T, C, G, X, I] (indexing.py:134's column order) for the call's sweeps, built deterministically — no random
number anywhere — so that every tie of the ranking and every threshold of the call (|p_i - p_j| <= 10, X >= 15 %, I > 55 %, the
case rule and the three coverage flags at mincov) is met exactly, one below and one above.  Test infrastructure only.

    exhaustive()   every (A, C, G, T, X) with a sum of at most 20 — 53 130 tuples — four times: coverage = the sum, and the sum
                   plus 1, 2 and 3 (tokens that count toward coverage only: N, IUPAC codes, '=', ref-skips).  I is one of {0,
                   floor(11 cov / 20), that plus 1, cov} (55 % of the coverage, from below and from above), capped at the coverage.
                   I takes part in one flag only, TCMI_F_INSCAND, which reads nothing but (cov, I, mincov): the four choices go
                   round by (tuple index + copy) instead of multiplying the rows by four, and every (cov, choice) pair with
                   cov <= 23 still comes up hundreds of times.  212 520 rows.
    lattice()      coverage 1 .. 400.  With f = cov // 10 the gaps between the ranked counts come from
                       top two:  {0, f - 1, f, f + 1}     (f is exactly 10 % where 10 divides cov; else f and f + 1 bracket it)
                       2nd-3rd:  {0, f - 1, f, f + 1, far}
                       3rd-4th:  {0, f, f + 1}
                   (0 / 0 / 0 are the three- and four-way exact ties), X sits on floor(15 cov / 100) and one either side, the top
                   count is the largest that fits the coverage and once a fifth less (the rest of the coverage is class-less), the four
                   counts go to A, C, G, T in all 24 orders in turn (ties are broken by the letter), and I goes round floor(55 cov /
                   100) and one either side.  Then, per coverage, the nine (X, I) pairs around the two thresholds on their own row.
"""
import functools
import itertools

import numpy as np

COV, A, T, C, G, X, I = range(7)
_LETTERS = (A, C, G, T)
_PERMS = tuple(itertools.permutations(_LETTERS))


def _ins_choices(cov):
    h = 11 * cov // 20
    return (0, min(h, cov), min(h + 1, cov), cov)


@functools.lru_cache(maxsize=None)
def exhaustive(max_sum=20):
    """-> int32 [n, 7]"""
    tuples = [(a, c, g, t, x)
              for a in range(max_sum + 1) for c in range(max_sum + 1 - a) for g in range(max_sum + 1 - a - c)
              for t in range(max_sum + 1 - a - c - g) for x in range(max_sum + 1 - a - c - g - t)]
    base = np.array(tuples, np.int32)
    n = len(base)
    out = np.zeros((4 * n, 7), np.int32)
    for extra in range(4):
        blk = out[extra * n:(extra + 1) * n]
        blk[:, A], blk[:, C], blk[:, G], blk[:, T], blk[:, X] = base.T
        blk[:, COV] = base.sum(1) + extra
        table = np.array([_ins_choices(cov) for cov in range(max_sum + 4)], np.int32)
        blk[:, I] = table[blk[:, COV], (np.arange(n) + extra) % 4]
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def lattice(max_cov=400):
    """-> int32 [n, 7]"""
    rows = []
    k = 0
    for cov in range(1, max_cov + 1):
        f = cov // 10
        x15, i55 = 15 * cov // 100, 55 * cov // 100
        for d12 in sorted({0, max(0, f - 1), f, f + 1}):
            for d23 in sorted({0, max(0, f - 1), f, f + 1, 3 * f + 7}):
                for d34 in sorted({0, f, f + 1}):
                    for nx in sorted({max(0, x15 - 1), x15, min(cov, x15 + 1)}):
                        top = (cov - nx + 3 * d12 + 2 * d23 + d34) // 4          # the largest top count that fits
                        for c1 in sorted({top, top - top // 5}):
                            c2, c3, c4 = c1 - d12, c1 - d12 - d23, c1 - d12 - d23 - d34
                            if c4 < 0:
                                c4 = 0                                              # (the fourth count cannot follow: a row all the same)
                            if c3 < 0 or c1 + c2 + c3 + c4 + nx > cov:
                                continue
                            row = [0] * 7
                            row[COV], row[X] = cov, nx
                            for col, cnt in zip(_PERMS[k % 24], (c1, c2, c3, c4)):
                                row[col] = cnt
                            row[I] = min(cov, max(0, i55 - 1 + k % 3))
                            rows.append(row)
                            k += 1
        for nx in sorted({max(0, x15 - 1), x15, min(cov, x15 + 1)}):
            for ni in sorted({max(0, i55 - 1), i55, min(cov, i55 + 1)}):
                row = [0] * 7
                row[COV], row[X], row[I] = cov, nx, ni
                row[_LETTERS[k % 4]] = cov - nx
                rows.append(row)
                k += 1
    out = np.array(rows, np.int32)
    out.setflags(write=False)
    return out


def all_rows():
    return np.concatenate([exhaustive(), lattice()])


def pieces(n, size=99_991):
    """[(a, b)] tiling range(n) into launches none of which is a multiple of 256 positions long"""
    out, a = [], 0
    while a < n:
        b = min(n, a + size)
        if (b - a) % 256 == 0:
            b -= 1
        out.append((a, b))
        a = b
    return out
