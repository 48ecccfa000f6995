"""The yardsticks of the record-stream tables under --mate-overlap and --dedup (tests/rules_marks.py, the clip of
tests/indel_yardstick.py), without a GPU: on the hand-made cases and the fuzz files of both rules the marks add up to the yardstick's
matrix and the clip-aware insertion totals to its I plane, the fuzz files hold the edges the GPU tests are there for (a D op cut behind
its first column, a D op on the edge, an insertion on either side of it, events of several records), the hand-made pairs give the one
event the rule's words leave, and the joint counts under a rule differ from those without — tests/test_stream_tables_under_rules.py
compares the device with these, and would be vacuous if they did not."""
import functools

import numpy as np
import pytest

from tests import codon_cases as cc
from tests import codon_yardstick as cy
from tests import dedup_cases as dc
from tests import dedup_yardstick as dy
from tests import indel_yardstick as iy
from tests import link_cases as lkc
from tests import links_yardstick as ly
from tests import mate_overlap_cases as mc
from tests import rules_marks as rm

# run -> (a file of rules_marks.FILES, the rule it is read under): each rule's files under that rule, the duplicate rule's also with
# the mate rule on top
RUNS = {"mate_cases": ("mate_cases", "mate"), "dedup_cases+mate": ("dedup_cases", "both")}
RUNS.update({"mate_seed%d" % s: ("mate_seed%d" % s, "mate") for s in mc.FUZZ_SEEDS})
RUNS.update({"dedup_seed%d" % s: ("dedup_seed%d" % s, "dedup") for s in dc.FUZZ_SEEDS})
RUNS.update({"dedup_seed%d+mate" % s: ("dedup_seed%d" % s, "both") for s in dc.FUZZ_SEEDS})
# run -> (specs, reference length, mate rule, duplicate rule)
FILES = {run: (rm.FILES[key][0], rm.FILES[key][2]) + rm.RULES[rule] for run, (key, rule) in RUNS.items()}
FUZZ = sorted(k for k in FILES if "seed" in k)
FUZZ_MATE = [k for k in FUZZ if FILES[k][2]]
FLOORS = (0, mc.FLOOR)
HAND_PAIRS = ("del_first_col", "del_later_col", "ins_inside", "ins_outside")


@functools.lru_cache(maxsize=None)
def arrays(key):
    specs = FILES[key][0]()
    return specs, dc.arrays(specs)


@functools.lru_cache(maxsize=None)
def yard(key, q=0, rules=True):
    _, L, mate, dedup = FILES[key]
    return dy.counts(arrays(key)[1], L, q=q, mate=mate and rules, dedup=dedup and rules)


@functools.lru_cache(maxsize=None)
def marks(key, q=0, rules=True):
    return rm.marks(arrays(key)[1], yard(key, q, rules), q=q)


def test_the_runs_cover_both_rules_files_and_the_gpu_tests_rules():
    assert len(FILES) == 8 and len(FUZZ) == 6 and len(FUZZ_MATE) == 4
    assert {key for key, _ in RUNS.values()} == set(rm.FILES) and all(rule in rm.FILES[key][3] for key, rule in RUNS.values())
    assert dc.FLOOR == mc.FLOOR == 13


@pytest.mark.parametrize("q", FLOORS)
@pytest.mark.parametrize("key", sorted(FILES))
def test_marks_add_up_to_the_matrix_and_insertions_to_the_I_plane(key, q):
    specs, rd = arrays(key)
    y = yard(key, q)
    cls, ins = marks(key, q)                                                    # (asserts that classes and I marks add up to y["counts"])
    assert cls.shape == ins.shape == (len(specs), len(y["counts"])) and cls.any()
    assert y["counters"]["clipped_columns"] > 0 or y["dedup_counters"]["duplicate_records"] > 0
    assert not np.array_equal(y["counts"], yard(key, q, rules=False)["counts"])
    counts, totals = rm.events(specs, rd, y, q=q)
    cols = list(range(len(y["counts"])))
    tot = iy.totals_at(totals, cols)
    assert np.array_equal(tot["ins_total"], y["counts"][:, 6]), np.flatnonzero(tot["ins_total"] != y["counts"][:, 6])[:8].tolist()
    assert (tot["del_total"] <= y["counts"][:, 0]).all()
    if "seed" in key:
        assert ins.any() and counts != rm.events(specs, rd, yard(key, q, rules=False), q=q)[0]


def test_the_default_clip_is_no_clip():
    specs, rd = arrays("mate_seed11")
    assert iy.events(specs) == iy.events(specs, clip=[0] * len(specs)) == rm.events(specs, rd, yard("mate_seed11", rules=False))
    assert all(iy.record_events(r) == iy.record_events(r, clip=0) for r in specs if iy.kept(r))


@pytest.mark.parametrize("key", FUZZ_MATE)
def test_fuzz_holds_the_clip_edges(key):
    specs, _ = arrays(key)
    e = rm.clip_edges(specs, yard(key)["clip"])
    print(key, e)
    assert e["del_cut"] >= 5 and e["del_at_edge"] >= 1 and e["ins_lost"] >= 4 and e["ins_kept"] >= 1, (key, e)


@pytest.mark.parametrize("key", FUZZ)
def test_fuzz_holds_events_of_several_records(key):
    specs, rd = arrays(key)
    counts, _ = rm.events(specs, rd, yard(key))
    several = sum(n >= 2 for n in counts.values())
    print(key, several)
    assert several >= 2, (key, several)


def test_hand_pairs_leave_one_event():
    specs, rd = arrays("mate_cases")
    idx = [i for i, r in enumerate(specs) if r["name"] in HAND_PAIRS]
    sub = [specs[i] for i in idx]
    assert len(sub) == 8
    off, _ = iy.events(sub)
    assert len(off) == 3 and off[(469, iy.DEL, 4, "")] == 2 and sorted(ev[:3] for ev in off) == [(469, iy.DEL, 4), (504, iy.INS, 2), (504, iy.INS, 2)], off
    clip = yard("mate_cases")["clip"]
    on, totals = iy.events(sub, clip=[clip[i] for i in idx])
    outside = [r for r in sub if r["name"] == "ins_outside" and "I" in r["cigar"]][0]
    assert on == {(504, iy.INS, 2, outside["seq"][5:7]): 1} and totals == {504: [1, 0]}, on
    # ... and in the whole file under the rule no other record adds an event on the pairs' columns
    whole, _ = rm.events(specs, rd, yard("mate_cases"))
    assert {ev: n for ev, n in whole.items() if 450 <= ev[0] < 520} == on


@pytest.mark.parametrize("key", FUZZ)
def test_joint_counts_under_the_rule_differ_from_those_without(key):
    mate = FILES[key][2]
    (cls, ins), (cls0, ins0) = marks(key), marks(key, rules=False)
    whole = yard(key)["counts"]
    cols = lkc.window_columns(whole)
    for k in (1, 3):
        j, j0 = ly.joint(cls, cols, k), ly.joint(cls0, cols, k)
        differ = int((j != j0).any((1, 2)).sum())
        print(key, k, differ)
        assert differ >= 0.9 * len(cols) * k, (key, k, differ)                   # (almost all pairs: 299 of 300, 862 to 894 of 900)
        if mate:
            assert (j[:, 0, 1:] > j0[:, 0, 1:]).any()                           # records clipped at a pair's first column and live at its second
    if mate:
        c0s = cc.two_frames(whole)
        a, b = cy.joint(cls, ins, c0s), cy.joint(cls0, ins0, c0s)
        n = int((a["ins_inside"] != b["ins_inside"]).sum())
        print(key, "ins_inside", n)
        assert n >= 1 and not np.array_equal(a["j"], b["j"]), key
