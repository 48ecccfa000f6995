"""The joining rule of block ranges in C (csrc/range_join.h: tcmi_split_step's ranks, and a rank's sub-ranges) without a GPU:
tests/range_join_main.cpp and nothing else, built with AddressSanitizer + UBSan and run once over every range table that
tests/test_distributed.py puts to the Python twin, distributed.check_range_anchors — the verdicts must agree — and over three
tables of the sub-range use (inflated = -1: no end of a stream to check), which the twin does not have."""
import re

import pytest

from tests import host_program
from tests.range_chains import random_chains
from trueconsense_amd.distributed import check_range_anchors

TOTAL = 10_000
HAND = [                        # the tables of test_check_range_anchors_joins_the_ranks_ranges_into_one_chain
    [(0, 4, -1, 2500), (4, 4, 2500, 5200), (8, 4, 5200, TOTAL)],
    [(0, 12, -1, -1)],
    [(0, 4, -1, 2500), (4, 0, -1, -1), (4, 8, 2500, TOTAL)],
    [(0, 4, -1, 2500), (4, 4, -1, -1), (8, 4, 2500, TOTAL)],
    [(0, 1, -1, 300), (1, 11, 300, TOTAL)],
    [(0, 4, -1, 2500), (4, 4, 2466, 5200), (8, 4, 5200, TOTAL)],
    [(0, 4, -1, 2500), (4, 4, 2500, 5200), (8, 4, 5200, TOTAL - 7)],
    [(0, 4, -1, -1), (4, 8, 2500, TOTAL)],
]
HAND_KINDS = ["none"] * 5 + ["start", "last", "nobody"]
# a rank's sub-ranges (split_sub_ranges hands the rule inflated = -1): the range starts in the middle of the file, so sub-range 0
# has a start of its own that nobody in front vouches for, and where the last one ends is not the rule's to check
SUB = [
    ([(8, 4, 2000, 2500), (12, 4, 2500, 5200), (16, 4, 5200, 9000)], "ok"),
    ([(8, 4, 2000, 2500), (12, 4, 2466, 5200), (16, 4, 5200, 9000)], "starts a record where the range in front does not end its last one\t1 2466 2500"),
    ([(8, 4, 2000, -1), (12, 4, 2500, 5200), (16, 4, 5200, 9000)], "starts a record, but no range in front says where its last record ends\t1 2500 -1"),
]

C_KIND = {"starts a record where the range in front does not end its last one": "start",
          "starts a record, but no range in front says where its last record ends": "nobody",
          "the last alignment record does not end with the file's stream": "last"}
PY_KIND = [("start", re.compile(r"rank (\d+)'s block range starts a record at stream offset (-?\d+), the range in front ends its last record at (-?\d+)$")),
           ("nobody", re.compile(r"rank (\d+)'s block range starts a record at stream offset (-?\d+), but no range in front says where its last record ends$")),
           ("last", re.compile(r"the last alignment record ends at stream offset (-?\d+), the file's stream at (-?\d+)$"))]


def c_verdict(line):
    """-> (kind, who, at, want) of one output line of the program"""
    if line == "ok":
        return ("none", None, None, None)
    msg, _, nums = line.partition("\t")
    who, at, want = (int(x) for x in nums.split())
    return (C_KIND[msg], who, at, want)


def py_verdict(ranges, inflated):
    """-> (kind, rank, offset, expected) of check_range_anchors; None where its message names none"""
    why = check_range_anchors(ranges, inflated)
    if why is None:
        return ("none", None, None, None)
    for kind, pat in PY_KIND:
        m = pat.match(why)
        if m:
            g = [int(x) for x in m.groups()]
            return (kind, None, g[0], g[1]) if kind == "last" else (kind, g[0], g[1], g[2] if kind == "start" else None)
    raise AssertionError("check_range_anchors says something this test does not know: %r" % why)


@pytest.fixture(scope="module")
def tables():
    """every table as (ranges, inflated, what it is), in the order the program sees them"""
    t = [(r, TOTAL, "hand %d" % k) for k, r in enumerate(HAND)]
    for c, (total, ranges, shifted, _, overrun) in enumerate(random_chains(300, 123)):
        t.append((ranges, total, "chain %d" % c))
        if shifted is not None:
            t.append((shifted, total, "chain %d, a start shifted" % c))
        if overrun is not None:
            t.append((overrun, total, "chain %d, the last record overruns" % c))
    return t + [(r, -1, "sub-ranges %d" % k) for k, (r, _) in enumerate(SUB)]


@pytest.fixture(scope="module")
def verdicts(tables, tmp_path_factory):
    """the program's output lines, one per table: ONE run of the program, which must end clean under both sanitizers"""
    prog = host_program.build(["tests/range_join_main.cpp"], tmp_path_factory.mktemp("range_join") / "range_join_main", skip_without_compiler=True)
    text = "".join("%d %d\n" % (len(r), inflated) + "".join("%d %d %d %d\n" % tuple(x) for x in r) for r, inflated, _ in tables)
    r = host_program.run(prog, input=text)
    lines = r.stdout.split("\n")
    assert lines[-1] == "" and len(lines) - 1 == len(tables), (len(lines), len(tables))
    return lines[:-1]


def test_c_rule_and_python_twin_agree_on_every_table(tables, verdicts):
    """kind of verdict everywhere; the rank where a start is refused; both offsets where a start does not match and where the last
    record does not end the stream.  No table is left out: the kinds are counted."""
    seen = {"none": 0, "start": 0, "nobody": 0, "last": 0}
    compared = 0
    for (ranges, inflated, what), line in zip(tables, verdicts):
        if inflated < 0:
            continue                                            # (the sub-range use: test_sub_range_tables_by_hand)
        c, p = c_verdict(line), py_verdict(ranges, inflated)
        assert c[0] == p[0], (what, ranges, line, p)
        if c[0] in ("start", "nobody"):
            assert c[1] == p[1] and c[2] == p[2], (what, ranges, line, p)
        if c[0] in ("start", "last"):
            assert c[2] == p[2] and c[3] == p[3], (what, ranges, line, p)
        seen[c[0]] += 1
        compared += 1
    assert compared == len(tables) - len(SUB) and compared >= len(HAND) + 300
    assert [c_verdict(v)[0] for v in verdicts[:len(HAND)]] == HAND_KINDS
    assert seen["none"] >= 5 + 300 and min(seen.values()) >= 1, seen          # (every chain's true anchors join)


def test_sub_range_tables_by_hand(tables, verdicts):
    """inflated = -1: a chain that joins, a middle start that is off, a middle range nobody in front vouches for"""
    assert [t[1] for t in tables[-len(SUB):]] == [-1] * len(SUB)
    assert verdicts[-len(SUB):] == [want for _, want in SUB]
