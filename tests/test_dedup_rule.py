"""--dedup without a GPU: the rule's text (csrc/dedup_rule.h) as a program of its own (tests/dedup_rule_main.cpp), built plain and under
AddressSanitizer + UBSan, against the yardstick (tests/dedup_yardstick.py) on the hand-made cases and the fuzz seeds; the yardstick
against what the cases were made to show; the conditions the GPU fuzz relies on; and the command line's argument handling.  The
kernels' tests are tests/test_dedup.py."""
import dataclasses

import numpy as np
import pytest

from oracle import tc_oracle as orc
from tests import dedup_cases as dc
from tests import dedup_yardstick as dy
from tests import host_program
from tests import mate_overlap_cases as mc
from tests import mate_overlap_yardstick as my
from tests.cli_run import base_args as _base
from tests.cli_run import stub_files
from trueconsense_amd import TrueConsense as cli
from trueconsense_amd import _ffi, engine

DATA = ("cases",) + tuple("seed%d" % s for s in dc.FUZZ_SEEDS)
# the rule's text: what every test in here is about (the yardstick restates it, the program compiles it)
RULE_TEXT = open(_ffi.__file__.replace("_ffi.py", "csrc/dedup_rule.h")).read()


def reads_of(key):
    return dc.arrays(dc.cases() if key == "cases" else dc.fuzz_specs(int(key[4:])))


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("dedup_rule_main")
    src = ["tests/dedup_rule_main.cpp"]
    return {"plain": host_program.build(src, d / "dedup_rule_main", sanitize=False), "sanitized": host_program.build(src, d / "dedup_rule_main_san")}


def fnv1a(data):
    h = 0xCBF29CE484222325
    for b in data:
        h = ((h ^ b) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    return h


# ---- the yardstick on the hand-made cases ------------------------------------------------------------------------------------------------
def test_the_cases_show_what_they_were_made_for():
    specs = dc.cases()
    rd = dc.arrays(specs)
    for f, want in ((dy.NONE, "dup"), (dc.FILTER, "dup_f")):
        v = dy.verdicts(rd, f)
        bad = [(r["name"], bool(v["dup"][i]), r[want]) for i, r in enumerate(specs) if bool(v["dup"][i]) != r[want]]
        assert not bad, (f, bad)
        have = dy.classes(rd, f)
        assert have >= set(dc.CLASSES), sorted(set(dc.CLASSES) - have)
        assert ("filtered_best" in have) == (f != dy.NONE)
        c = v["counters"]
        assert c["duplicate_templates"] == sum(len(ts) - 1 for ts in v["templates"].values()) and c["duplicate_records"] == int(v["dup"].sum())
    by_name = {}
    for i, r in enumerate(specs):
        by_name.setdefault(r["name"], []).append(i)
    # the ends the cases were placed on: clips of both sorts in front of a forward read, behind a reverse one; a negative one
    assert {dy.end(rd, by_name[k][0]) for k in ("clip_none", "clip_soft", "clip_hard")} == {(0, 140, 0)}
    assert dy.end(rd, by_name["rev_a"][0]) == dy.end(rd, by_name["rev_b"][0]) == (0, 229, 1) and dy.end(rd, by_name["rev_c"][0]) == (0, 231, 1)
    assert dy.end(rd, by_name["neg_a"][0]) == dy.end(rd, by_name["neg_b"][0]) == (0, -3, 0)
    assert dy.score(rd, by_name["ff_none"][0]) == 0 and dy.score(rd, by_name["q14"][0]) == 0 and dy.score(rd, by_name["q15"][0]) == 15
    # a duplicate is piled up and adds nothing; with the mate rule also on the surviving pair still gets its overlap clip
    on, off = dy.counts(rd, dc.L), dy.counts(rd, dc.L, dedup=False)
    assert on["n_piled"] == off["n_piled"] and on["max_end"] == off["max_end"]
    lost = sum(my.span(rd, i)[1] - my.span(rd, i)[0] + 1 for i in np.flatnonzero(on["dup"]))
    assert off["counts"][:, 0].sum() - on["counts"][:, 0].sum() == lost > 0
    both = dy.counts(rd, dc.L, mate=True)
    lo = [i for i in by_name["ovl_a"] if both["clip"][i] > 0]
    assert len(lo) == 1 and both["clip"][lo[0]] == 20 and not both["dup"][lo[0]] and both["counters"]["pairs"] > 0
    assert all(both["clip"][i] == 40 for i in by_name["ovl_b"])
    assert both["dedup_counters"] == on["dedup_counters"] and on["counters"]["pairs"] == 0


def test_the_same_key_on_two_references():
    """a file of two references is judged reference by reference: a set of two on each, neither sees the other"""
    specs = dc.two_refs()
    for tid in (0, 1):
        mine = mc.on_reference_0(specs, tid)
        v = dy.verdicts(dc.arrays(mine))
        assert [bool(x) for x in v["dup"]] == [r["dup"] for r in mine] == [True, False] and v["counters"]["duplicate_sets"] == 1
    both = dy.verdicts(dc.arrays([dict(r, tid=0) for r in specs]))      # (on one reference they would be one set of four)
    assert both["counters"]["duplicate_sets"] == 1 and both["counters"]["duplicate_templates"] == 3


def test_the_tie_break_follows_the_file():
    specs = dc.fuzz_specs(dc.FUZZ_SEEDS[0])
    a, b = dy.verdicts(dc.arrays(specs)), None
    perm = dc.permuted(specs, 5)
    b = dy.verdicts(dc.arrays(perm))
    assert a["counters"] == b["counters"]                                   # which templates exist does not depend on the order
    name_a = {(r["name"], r["flag"], r["pos"]) for i, r in enumerate(specs) if a["dup"][i]}
    name_b = {(r["name"], r["flag"], r["pos"]) for i, r in enumerate(perm) if b["dup"][i]}
    assert name_a != name_b                                                 # ... the winner of a tie does


# ---- the rule's text as a program ------------------------------------------------------------------------------------------------------------
def program_input(rd, f, v, extra=()):
    n = int(rd["n_reads"])
    lines = []
    for i in range(n):
        cig = ["%d" % ((ln << 4) | op) for op, ln in orc.read_cigar(rd, i)]
        q = bytes(dy.quals(rd, i)).hex() or "-"
        lines.append("%d %d %d %d %d %d %s %s" % (int(my.kept(rd, i, f)), int(rd["flag"][i]), int(rd["tid"][i]), int(rd["pos"][i]),
                                                   v["mate"].get(i, -1) + 1, len(cig), " ".join(cig), q))
    return lines + list(extra)


@pytest.mark.parametrize("key", DATA)
@pytest.mark.parametrize("build", ("plain", "sanitized"))
def test_rule_program_against_the_yardstick(programs, tmp_path, build, key):
    rd = reads_of(key)
    f = dc.FILTER if key != "cases" else dy.NONE
    v = dy.verdicts(rd, f)
    n = int(rd["n_reads"])
    leaders = {t[1]: (k, t[0]) for k, ts in v["templates"].items() for t in ts}
    # every template against its key's winner, and the winners among themselves
    duels = [(t[1], v["winner"][k]) for k, ts in v["templates"].items() for t in ts]
    wl = sorted(v["winner"].values())
    duels += list(zip(wl, wl[1:]))
    # one more record without SEQ and QUAL (l_seq == 0 scores 0), kept, forward, a fragment
    lines = program_input(rd, f, v) + ["1 0 0 7 0 1 %d -" % ((30 << 4) | 0)]
    inp, out = str(tmp_path / "r.in"), str(tmp_path / "r.out")
    with open(inp, "w") as fh:
        fh.write("%d %d\n" % (n + 1, len(duels)) + "\n".join(lines) + "\n" + "".join("%d %d\n" % d for d in duels))
    r = host_program.run(programs[build], inp, out)
    assert r.stdout.strip() == "ok %d" % (n + 1), (r.stdout[-500:], r.stderr[-2000:])
    got = [ln.split() for ln in open(out).read().split("\n") if ln]
    assert len(got) == n + 1 + len(duels)
    for i in range(n):
        ex, u5, rev, score, kb, h = got[i]
        assert int(ex) == int(dy.examined(rd, i, f)), i
        if int(ex):
            assert (int(u5), int(rev)) == dy.end(rd, i)[1:] and int(score) == dy.score(rd, i), (i, got[i], dy.end(rd, i), dy.score(rd, i))
        if i in leaders:
            want = dy.key_bytes(leaders[i][0])
            assert kb == want.hex() and int(h, 16) == fnv1a(want), (i, kb, want.hex())
        else:
            assert kb == "-" and h == "-", i
    assert got[n][:4] == ["1", "7", "0", "0"]
    for (a, b), line in zip(duels, got[n + 1:]):
        (_, sa), (_, sb) = leaders[a], leaders[b]
        assert int(line[0]) == int((sa, -a) > (sb, -b)), (a, b, sa, sb, line)
    # keys: equal bytes exactly for equal keys
    assert len({dy.key_bytes(k) for k in v["templates"]}) == len(v["templates"])


# ---- what the GPU fuzz relies on -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", dc.FUZZ_SEEDS)
def test_fuzz_seeds_hold_every_class(seed):
    rd = dc.arrays(dc.fuzz_specs(seed))
    for f in (dy.NONE, dc.FILTER):
        v = dy.verdicts(rd, f)
        have = dy.classes(rd, f)
        assert have >= set(dc.CLASSES), (seed, f, sorted(set(dc.CLASSES) - have))          # no class may be empty
        sets = [(k[0], len(ts)) for k, ts in v["templates"].items() if len(ts) >= 2]
        assert sum(1 for kind, _ in sets if kind == "F") >= 20 and sum(1 for kind, _ in sets if kind == "P") >= 10, (seed, f, len(sets))
        ties = sum(1 for ts in v["templates"].values() if len(ts) >= 2 and sorted(t[0] for t in ts)[-1] == sorted(t[0] for t in ts)[-2])
        assert ties >= 3 and v["counters"]["duplicate_records"] > v["counters"]["duplicate_templates"] > 100
    assert "filtered_best" in dy.classes(rd, dc.FILTER)
    # the matrix differs from the one without the rule, under the mate rule too
    for mate in (False, True):
        assert not np.array_equal(dy.counts(rd, dc.FUZZ_L, mate=mate)["counts"], dy.counts(rd, dc.FUZZ_L, mate=mate, dedup=False)["counts"])
    assert np.array_equal(dy.counts(rd, dc.FUZZ_L, mate=True, dedup=False)["counts"], my.counts(rd, dc.FUZZ_L)["counts"])


# ---- the command line ---------------------------------------------------------------------------------------------------------------------------
def test_cli_accepts_the_flag_and_refuses_by_name(tmp_path, capsys):
    f = stub_files(tmp_path)
    a = cli.GetArgs(_base(f) + ["--dedup"])
    assert a.dedup is True and cli.GetArgs(_base(f)).dedup is False
    assert cli.rules_of(a).dedup is True and cli.rules_of(cli.GetArgs(_base(f) + ["--dedup", "--mate-overlap", "--min-baseq", "13"])) == \
        engine.ReadRules(None, 13, None, True, True)
    with pytest.raises(SystemExit) as e:
        cli.GetArgs(_base(f) + ["--dedup", "--gpus", "2"])
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert "--dedup does not go with -i --gpus N" in err and "a template's other records may lie in another rank's block range" in err
    bed = tmp_path / "s.bed"
    bed.write_text("ref\t10\t30\tA_1_LEFT\t1\t+\nref\t200\t220\tA_1_RIGHT\t1\t-\n")
    with pytest.raises(SystemExit) as e:
        cli.GetArgs(_base(f) + ["--dedup", "--amplicon-reads", str(tmp_path / "ar.tsv"), "--amplicon-scheme", str(bed)])
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert "--dedup does not go with --amplicon-reads" in err and "would count the duplicates" in err


def test_cli_forwards_the_flag_to_batch_children(tmp_path):
    f = stub_files(tmp_path, names=("x.bam", "r.fa", "f.gff", "m.tsv"))
    args = ["--batch", f["m.tsv"], "-ref", f["r.fa"], "-gff", f["f.gff"], "-cov", "30", "--gpus", "2"]
    on = cli._child_argv(cli.GetArgs(args + ["--dedup", "--mate-overlap"]), False)
    assert "--dedup" in on and "--mate-overlap" in on
    assert "--dedup" not in cli._child_argv(cli.GetArgs(args + ["--mate-overlap"]), False)


def test_stats_keys():
    s = cli.dedup_stats(True, {"templates": 9, "duplicate_templates": 3, "duplicate_records": 5, "duplicate_sets": 2})
    assert s == {"dedup": True, "dedup_templates": 9, "duplicate_templates": 3, "duplicate_records": 5, "duplicate_sets": 2}
    assert cli.dedup_stats(False, None) == {"dedup": False, "dedup_templates": 0, "duplicate_templates": 0, "duplicate_records": 0, "duplicate_sets": 0}


def test_bindings_and_defaults():
    text = open(_ffi.__file__.replace("_ffi.py", "../include/tcmi.h")).read()
    for name in ("tcmi_ctx_set_dedup", "tcmi_readset_dedup", "tcmi_readset_duplicates"):
        assert name + "(" in text and getattr(_ffi.lib(), name)
    assert "TCMI_K_NKERNELS = %d " % (_ffi.K_MATE_JOIN + 1) in text                  # (no profile slot of its own: the join's bracket)
    assert hasattr(engine.Context, "set_dedup") and engine.Context.dedup is False and hasattr(engine.ReadSet, "duplicates")
    assert hasattr(engine.FileRunner, "dedup_totals")
    assert engine.ReadRules() == engine.ReadRules(None, 0, None, False) and engine.ReadRules().dedup is False
    assert [f.name for f in dataclasses.fields(engine.ReadRules)][-1] == "dedup"
    assert "#include <hip" not in RULE_TEXT and "hip_runtime" not in RULE_TEXT


# ---- the numpy restatements of the scale tests -----------------------------------------------------------------------------------------------------
def test_numpy_restatement_against_the_yardstick():
    from tests import dedup_big as db
    from tests import mate_big as mb
    rd = mb.head(mb.generate(100001), 2000)                                     # (a prefix: pairs whose mate lies behind it are fragments)
    dup, cnt = db.verdicts(rd)
    v = dy.verdicts(mb.as_reads(rd))
    assert cnt == v["counters"] and np.array_equal(dup, v["dup"]), (cnt, v["counters"])
    assert cnt["duplicate_sets"] > 50 and cnt["duplicate_records"] > cnt["duplicate_templates"] > 200
    kinds = {k[0] for k, ts in v["templates"].items() if len(ts) >= 2}
    assert kinds == {"F", "P"}


def test_one_key_file_against_the_yardstick(tmp_path):
    from tests import dedup_big as db
    dup, cov, L = db.one_key_and_distinct(tmp_path / "one.bam", 300)
    rd = db.one_key_reads(300)
    y = dy.counts(rd, L)
    assert np.array_equal(dup, y["dup"]) and np.array_equal(cov, y["counts"][:L, 0])
    assert y["dedup_counters"] == {"templates": 600, "duplicate_templates": 299, "duplicate_records": 299, "duplicate_sets": 1}
    from oracle import c_oracle
    got = c_oracle.read_bam(str(tmp_path / "one.bam"))                          # (the file holds the records the arrays say)
    assert np.array_equal(got["pos"], rd["pos"]) and np.array_equal(got["cigar"], rd["cigar"]) and int(got["n_reads"]) == 600
