"""The call on every tie and threshold (tests/call_rows.py): the C oracle against the Python restatement of the reference on the CPU —
every GPU call test trusts c_oracle.call —, and the call kernel against the C oracle on all rows, through tcmi_call and through
tcmi_call_dev on a matrix with an odd leading dimension.

fp64: a percentage is (c / cov) * 100, two roundings, and the reference compares differences of two of them with 10 (Ambig.py:156-171).
A compiler that contracts p1 - p2 into a fused multiply-add skips one rounding; csrc/Makefile and oracle/Makefile forbid that with
-ffp-contract=off.  test_contracted_differences_would_change_records shows with exact rationals that the exhaustive rows hold
records that such a contraction changes: rows on which a build without the flag can be told from one with it."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

from oracle import c_oracle
from oracle import tc_oracle as orc
from tests import call_rows
from trueconsense_amd import _ffi, engine


def _same(got, want, rows, what):
    for name, g, w in zip(("plain", "alt", "flags"), got, want):
        bad = np.nonzero(np.asarray(g) != np.asarray(w))[0]
        assert len(bad) == 0, (what, name, len(bad), rows[bad[:5]].tolist(), np.asarray(g)[bad[:5]].tolist(), np.asarray(w)[bad[:5]].tolist())


# ------------------------------------------------------------------------------------------------------------------------ CPU
def test_rows_are_what_the_sweep_needs():
    ex, la = call_rows.exhaustive(), call_rows.lattice()
    assert len(ex) == 4 * 53130 and len(np.unique(ex[:, :6], axis=0)) == len(ex)
    assert (ex[:, 1:6].sum(1) <= 20).all() and set((ex[:, 0] - ex[:, 1:6].sum(1)).tolist()) == {0, 1, 2, 3}
    assert (la[:, 1:6].sum(1) <= la[:, 0]).all() and (la[:, 6] <= la[:, 0]).all() and la.min() >= 0
    assert la[:, 0].min() == 1 and la[:, 0].max() == 400
    top = -np.sort(-la[:, 1:5], axis=1)
    ten = la[la[:, 0] % 10 == 0]
    t10 = -np.sort(-ten[:, 1:5], axis=1)
    for d in (-1, 0, 1):                                                         # the top two exactly 10 % apart, one less, one more
        assert ((t10[:, 0] - t10[:, 1]) * 10 == ten[:, 0] + 10 * d).sum() > 100, d
    assert ((top[:, 0] == top[:, 2]) & (top[:, 0] > 0) & (top[:, 2] > top[:, 3])).sum() > 100      # three-way exact ties
    assert ((top[:, 0] == top[:, 3]) & (top[:, 0] > 0)).sum() > 100                                  # four-way exact ties
    assert (la[:, 5] * 100 == 15 * la[:, 0]).sum() > 100 and (la[:, 6] * 100 == 55 * la[:, 0]).sum() > 100
    assert all((b - a) % 256 for a, b in call_rows.pieces(len(ex) + len(la))) and call_rows.pieces(512, 256) == [(0, 255), (255, 510), (510, 512)]


@pytest.mark.parametrize("mincov,amb", ((0, True), (10, False)))
def test_c_oracle_equals_python_oracle_on_exhaustive_rows(mincov, amb):
    rows = call_rows.exhaustive()
    _same(c_oracle.call(rows, mincov, amb), orc.call_records(rows, mincov, amb), rows, (mincov, amb))


@pytest.mark.parametrize("mincov,amb", ((1, True), (21, True)))
def test_c_oracle_equals_python_oracle_on_a_lattice_sample(mincov, amb):
    la = call_rows.lattice()
    rows = la[np.sort(np.random.default_rng(400).choice(len(la), 20_000, replace=False))]
    _same(c_oracle.call(rows, mincov, amb), orc.call_records(rows, mincov, amb), rows, (mincov, amb))
    flags = c_oracle.call(rows, mincov, amb)[2]
    for bit in (1, 2, 4, 8, 16, 64)[mincov <= 1:]:                               # (the sample sees every flag set and clear; no lattice row is below coverage 1)
        assert 0 < int(((flags & bit) != 0).sum()) < len(rows), bit


def _close_table(max_cov, max_cnt):
    """(cov, ci, cj) -> (as the reference evaluates |p_i - p_j| <= 10, with p_i's product fused into the difference, with p_j's)"""
    tab = {}
    for cov in range(1, max_cov + 1):
        q = [c / cov for c in range(max_cnt + 1)]
        p = [v * 100 for v in q]
        for ci in range(max_cnt + 1):
            for cj in range(ci + 1):
                plain = abs(p[ci] - p[cj]) <= 10
                fused_i = abs(float(Fraction(q[ci]) * 100 - Fraction(p[cj]))) <= 10     # fma(q_i, 100, -p_j): one rounding
                fused_j = abs(float(Fraction(p[ci]) - Fraction(q[cj]) * 100)) <= 10     # fma(-q_j, 100, p_i)
                tab[cov, ci, cj] = (plain, fused_i, fused_j)
    return tab


def _ambiguity(rank, cov, close):
    """tc_oracle.ambiguity with the comparison handed in: close(ci, cj) for ci >= cj"""
    if cov == 0:
        return False, None
    (n1, c1), (n2, c2), (n3, c3), (n4, c4) = rank[:4]
    if n1 == "X" or n2 == "X":
        return False, None
    if not close(c1, c2):
        return False, None
    if close(c1, c3) and close(c2, c3):
        if close(c1, c4) and close(c2, c4) and close(c3, c4):
            return True, "N"
        if "X" in (n1, n2, n3):
            return True, "N"
        return True, "".join(sorted((n1, n2, n3)))
    return True, "".join(sorted((n1, n2)))


def test_contracted_differences_would_change_records():
    """Non-vacuity of the fp64 rule: each |p_i - p_j| <= 10 of Ambig.py evaluated a second time as a contracted fma — the product of
    one percentage fused into the subtraction, exact product by fractions.Fraction, one rounding; both operand orders — changes the
    ambiguity verdict (flag TCMI_F_AMBIG, and with it the plain character) of exhaustive rows.  Observed: of the 212 520 rows 1 506 change their record with the
    first percentage's product fused, 1 488 with the second's, 1 506 under at least one of the two.  Among them the rows with coverage
    20 and top counts 8 and 6, or 9 and 7."""
    rows = call_rows.exhaustive()
    tab = _close_table(int(rows[:, 0].max()), int(rows[:, 1:6].max()))
    changed = [0, 0, 0]
    seen_20 = set()
    memo = {}
    for row in rows:
        cov = int(row[0])
        key = (cov,) + tuple(int(v) for v in row[1:6])
        if key not in memo:
            rank = orc.ranked(row)
            want = _ambiguity(rank, cov, lambda a, b: tab[cov, a, b][0])
            assert want[0] == orc.ambiguity(rank, cov)[0]                        # (the restatement above is the oracle's)
            memo[key] = (rank, [_ambiguity(rank, cov, lambda a, b, k=k: tab[cov, a, b][k]) != want for k in (1, 2)])
        rank, diff = memo[key]
        changed[0] += diff[0]
        changed[1] += diff[1]
        changed[2] += diff[0] or diff[1]
        if cov == 20 and (diff[0] or diff[1]):
            seen_20.add((rank[0][1], rank[1][1]))
    print("records changed by a contracted difference: first operand %d, second operand %d, either %d" % tuple(changed))
    assert changed[2] > 0
    assert {(8, 6), (9, 7)} <= seen_20


# ------------------------------------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def ctx():
    with engine.Context(0) as c:
        yield c


@pytest.fixture(scope="module")
def device_rows(ctx):
    """all rows resident once, piece by piece, as planes with an odd leading dimension (tcmi_counts_upload)"""
    import torch
    rows = call_rows.all_rows()
    out = []
    for a, b in call_rows.pieces(len(rows)):
        L = b - a
        ld = L + 1 if L % 2 == 0 else L + 2
        planes = torch.zeros(7 * ld, dtype=torch.int32, device="cuda")
        rec = torch.zeros(3 * ld, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        _ffi.check(_ffi.lib().tcmi_counts_upload(ctx.handle, _ffi.ptr(np.ascontiguousarray(rows[a:b])), L, ld, C.c_void_p(planes.data_ptr())), ctx.handle)
        out.append((a, b, ld, planes, rec))
    return rows, out


@pytest.mark.gpu
@pytest.mark.parametrize("amb", (True, False))
@pytest.mark.parametrize("mincov", (0, 1, 10, 20, 21))
def test_call_kernel_equals_c_oracle_on_all_rows(ctx, device_rows, mincov, amb):
    rows, resident = device_rows
    want = c_oracle.call(rows, mincov, amb)
    for a, b, ld, planes, rec in resident:
        L = b - a
        assert L % 256 and ld % 2 == 1
        piece = np.ascontiguousarray(rows[a:b])
        _same(ctx.call(piece, mincov, amb), [w[a:b] for w in want], piece, ("tcmi_call", mincov, amb, a))
        rec.zero_()
        import torch
        torch.cuda.synchronize()
        base = rec.data_ptr()
        ctx.call_dev(planes.data_ptr(), L, ld, mincov, amb, base, base + ld, base + 2 * ld)
        ctx.sync()
        got = rec.cpu().numpy().reshape(3, ld)
        _same([got[k, :L] for k in range(3)], [w[a:b] for w in want], piece, ("tcmi_call_dev", mincov, amb, a))
        assert not got[:, L:].any()
