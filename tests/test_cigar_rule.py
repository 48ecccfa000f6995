"""CPU: the CIGAR rule (csrc/cigar_rule.h) in a program of its own — tests/cigar_rule_main.cpp, built with AddressSanitizer + UBSan and run
as a child process — against tests/odd_cigars.sums, the rule restated in a few lines of Python: the reference span, the query total Yq
and the verdict "malformed" (span > 0 and Yq >= 2^29) of the generator's records, of the hand-made lists, of the refused records and of
10 000 random word lists of up to 65 535 ops and lengths up to 2^28 - 1.  No record can hold a sum beyond 2^44: 65 535 ops of 2^28 - 1
add up to 2^44 - 2^28 - 65 535, so that largest possible sum is among the lists instead.  The 32-bit form the kernels carry
(tcmi_cigar_step) must give the 64-bit verdict on every list."""
import numpy as np
import pytest

from tests import host_program
from tests import odd_cigars as oc


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    return host_program.build(["tests/cigar_rule_main.cpp"], str(tmp_path_factory.mktemp("cigar_rule") / "cigar_rule_main"))


def judged(prog, tmp_path, lists):
    """-> [(span, Yq, verdict)] by the program; its two verdicts must agree"""
    path = str(tmp_path / "lists.bin")
    with open(path, "wb") as fh:
        for w in lists:
            fh.write(np.uint32(len(w)).tobytes() + np.asarray(w, "<u4").tobytes())
    rows = [tuple(int(x) for x in line.split()) for line in host_program.run(prog, path).stdout.splitlines()]
    assert len(rows) == len(lists)
    assert all(r[2] == r[3] for r in rows), [r for r in rows if r[2] != r[3]][:4]
    return [r[:3] for r in rows]


def test_generator_and_hand_made_records(prog, tmp_path):
    recs = [r for seed in oc.SEEDS for r in oc.seed_case(seed)[0]] + oc.hand_specs() + oc.large_specs()
    lists = [oc.words_of(r) for r in recs]
    got = judged(prog, tmp_path, lists)
    assert got == [oc.sums(w) for w in lists]
    assert not any(v for _, _, v in got) and max(y for _, y, _ in got) == oc.BOUND - 1            # tolerated, up to the last legal total


def test_refused_records_and_the_edges_of_the_bound(prog, tmp_path):
    lists = [[(n << 4) | oc.hb.OPS.index(op) for n, op in cig] for cig in oc.LIARS.values()]
    got = judged(prog, tmp_path, lists)
    assert got == [oc.sums(w) for w in lists] and all(v == 1 for _, _, v in got)
    assert got[0][1] == oc.BOUND and max(y for _, y, _ in got) > 1 << 39
    M, I, D, S, X = 0, 1, 2, 4, 8
    w = lambda n, op: (n << 4) | op
    edges = {
        "one below": ([w(20, M), w(oc.MAXLEN, I), w(oc.BOUND - 21 - oc.MAXLEN, S)], 0),
        "on it": ([w(20, M), w(oc.MAXLEN, I), w(oc.BOUND - 20 - oc.MAXLEN, S)], 1),
        "2^32 + 3: a 32-bit sum would be 3": ([w(oc.MAXLEN, S)] * 16 + [w(16, S), w(3, X)], 1),
        "2^29 and no span: not judged": ([w(oc.MAXLEN, S)] * 3, 0),
        "2^29 in D and N ops: no query": ([w(oc.MAXLEN, D)] * 3 + [w(5, 3)], 0),
        "reserved codes and P count nothing": ([w(oc.MAXLEN, op) for op in (5, 6, 9, 10, 11, 12, 13, 14, 15)] * 4 + [w(5, M)], 0),
        "zero-length ops": ([w(0, op) for op in range(16)] + [w(7, 7)], 0),
        "empty": ([], 0),
    }
    got = judged(prog, tmp_path, [e[0] for e in edges.values()])
    assert [g[2] for g in got] == [e[1] for e in edges.values()], dict(zip(edges, got))
    assert got == [oc.sums(e[0]) for e in edges.values()]
    assert got[2][1] == (1 << 32) + 3


def test_ten_thousand_random_word_lists(prog, tmp_path):
    rng = np.random.default_rng(29)
    lists = []
    for k in range(10000):
        how = k % 10
        n = 65535 if k in (17, 4242) else int(rng.integers(0, 40)) if how < 8 else int(rng.integers(40, 3000))
        ops = rng.integers(0, 16, n, dtype=np.uint32)
        if how in (0, 1, 2):                                                    # short ops: far below the bound
            lens = rng.integers(0, 400, n, dtype=np.uint32)
        elif how in (3, 4, 5):                                                  # sums that land on both sides of 2^29
            lens = rng.integers(0, 1 << int(rng.integers(20, 29)), n, dtype=np.uint32)
        else:                                                                   # every bit of the length field
            lens = rng.integers(0, 1 << 28, n, dtype=np.uint32)
        if how == 9:
            lens[rng.random(n) < 0.5] = oc.MAXLEN
        if k == 17:                                                             # the largest sums a record can hold
            ops[:], lens[:] = 0, oc.MAXLEN
        lists.append((lens << np.uint32(4)) | ops)
    got = judged(prog, tmp_path, lists)
    want = [oc.sums(w.tolist()) for w in lists]
    assert got == want
    verdicts = [v for _, _, v in got]
    near = sum(1 for _, y, _ in got if oc.BOUND // 4 <= y < oc.BOUND)
    assert 1000 < sum(verdicts) < 9000 and near > 100 and max(y for _, y, _ in got) == 65535 * oc.MAXLEN > (1 << 44) - (1 << 29) and max(len(w) for w in lists) == 65535
