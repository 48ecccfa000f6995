"""--mate-overlap without a GPU: the rule's text (csrc/mate_rule.h) as a program of its own (tests/mate_rule_main.cpp), built plain and
under AddressSanitizer + UBSan, against the yardstick (tests/mate_overlap_yardstick.py) on the hand-made cases and the fuzz seeds; the
yardstick against what the cases were made to show; the conditions the GPU fuzz relies on; the numpy restatement of the scale test against
the yardstick; and the command line's argument handling.  The kernels' tests are tests/test_mate_overlap.py."""
import numpy as np
import pytest

from tests import host_program
from tests import mate_big as mb
from tests import mate_overlap_cases as mc
from tests import mate_overlap_yardstick as my
from tests.cli_run import base_args as _base
from tests.cli_run import stub_files
from trueconsense_amd import TrueConsense as cli
from trueconsense_amd import _ffi, engine

DATA = ("cases",) + tuple("seed%d" % s for s in mc.FUZZ_SEEDS)


def reads_of(key):
    return mc.arrays(mc.cases()[0] if key == "cases" else mc.fuzz_specs(int(key[4:])))


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("mate_rule_main")
    src = ["tests/mate_rule_main.cpp"]
    return {"plain": host_program.build(src, d / "mate_rule_main", sanitize=False), "sanitized": host_program.build(src, d / "mate_rule_main_san")}


def fnv1a(name, tid, lo, hi):
    h = 0xCBF29CE484222325
    for b in name + b"".join(int(v & 0xFFFFFFFF).to_bytes(4, "little") for v in (tid, lo, hi)):
        h = ((h ^ b) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    return h


# ---- the yardstick on the hand-made cases ------------------------------------------------------------------------------------------------
def test_the_cases_show_what_they_were_made_for():
    specs, expect = mc.cases()
    rd = mc.arrays(specs)
    y = my.counts(rd, mc.L)
    by_name = {}
    for i, r in enumerate(specs):
        by_name.setdefault(r["name"], []).append(i)
    losers = {lo: wi for lo, wi in y["pairs"]}
    for name, clip in expect.items():
        mine = [i for i in by_name[name] if i in losers]
        if clip is None:
            assert not mine and all(y["clip"][i] == 0 for i in by_name[name]), name
        else:
            assert len(mine) == 1 and y["clip"][mine[0]] == clip, (name, mine, [y["clip"][i] for i in by_name[name]])
    assert y["counters"]["ambiguous"] == 4 and all(y["classes"][i] == "ambiguous" for i in by_name["twice"])
    # equal pos: the 0x80 record loses, in both file orders
    for name, at in (("eq_first_then_last", 1), ("eq_last_then_first", 0)):
        lo = [i for i in by_name[name] if i in losers][0]
        assert specs[lo]["flag"] & 0x80 and by_name[name].index(lo) == at, name
    assert {y["classes"][i] for i in by_name["mismatch"]} == {"next_pos_mismatch"} and {y["classes"][i] for i in by_name["two_firsts"]} == {"same_end"}
    assert {y["classes"][i] for i in by_name["off_by_one"]} == {"single"} and {y["classes"][i] for i in by_name["other_ref"]} == {"other_reference"}
    assert sorted(y["classes"][i] for i in by_name["with_extras"] if i in y["classes"]) == ["secondary", "supplementary"]
    # a loser clipped from end to end is piled up and adds nothing; the long reads' clips lie on both sides of 1 023 columns
    lo = [i for i in by_name["contained"] if i in losers][0]
    assert y["clip"][lo] == my.span(rd, lo)[1] - my.span(rd, lo)[0] + 1 and not my.tokens(rd, lo, y["clip"][lo])[0]
    assert expect["long_below"] < 1023 < expect["long_above"]
    # under the filter the winner of low_mapq_winner is gone and its mate keeps everything
    yf = my.counts(rd, mc.L, f=mc.FILTER)
    assert all(yf["clip"][i] == 0 for i in by_name["low_mapq_winner"]) and yf["counters"]["pairs"] == y["counters"]["pairs"] - 1
    # under the table: the loser's head primer is longer / shorter than its clip; the winner's tail is masked and so the columns are empty
    yp = my.counts(rd, mc.L, primers=mc.PRIMERS)
    assert yp["n_masked"] > 0 and np.array_equal(yp["clip"], y["clip"])
    # the setting off: the doubled evidence
    off = my.counts(rd, mc.L, mate=False)
    assert off["counts"][:, 0].sum() - y["counts"][:, 0].sum() == y["counters"]["clipped_columns"] > 0


# ---- the rule's text as a program ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", DATA)
@pytest.mark.parametrize("build", ("plain", "sanitized"))
def test_rule_program_against_the_yardstick(programs, tmp_path, build, key):
    rd = reads_of(key)
    f = mc.FILTER if key != "cases" else my.NONE
    y = my.counts(rd, mc.L, f=f)
    idx = [i for i in range(int(rd["n_reads"])) if my.kept(rd, i, f)]
    inp, out = str(tmp_path / "r.in"), str(tmp_path / "r.out")
    with open(inp, "w") as fh:
        for i in idx:
            flag, tid, pos, ntid, npos = my.fields(rd, i)
            p, q = my.span(rd, i)
            fh.write("%d %d %d %d %d %d %d %s\n" % (flag, tid, pos, ntid, npos, p, q, my.name(rd, i).hex() or "-"))
    r = host_program.run(programs[build], inp, out)
    assert r.stdout.strip() == "ok %d" % len(idx), (r.stdout[-500:], r.stderr[-2000:])
    got = [ln.split() for ln in open(out).read().split("\n") if ln]
    assert len(got) == len(idx)
    losers = {lo for lo, _ in y["pairs"]}
    in_pair = losers | {wi for _, wi in y["pairs"]}
    for i, (elig, h, members, pair, loses, clip) in zip(idx, got):
        flag, tid, pos, ntid, npos = my.fields(rd, i)
        assert int(elig) == (my.why_not_eligible(flag, tid, pos, ntid, npos) is None), i
        assert int(h, 16) == fnv1a(my.name(rd, i), tid, min(pos, npos), max(pos, npos)), i
        assert (int(pair), int(loses), int(clip)) == (int(i in in_pair), int(i in losers), y["clip"][i]), (i, pair, loses, clip)
        assert (int(members) >= 3) == (y["classes"].get(i) == "ambiguous"), i


# ---- what the GPU fuzz relies on -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", mc.FUZZ_SEEDS)
def test_fuzz_seeds_hold_every_class(seed):
    rd = mc.arrays(mc.fuzz_specs(seed))
    for f in (my.NONE, mc.FILTER):
        y = my.counts(rd, mc.L, f=f)
        assert sum(1 for lo, _ in y["pairs"] if y["clip"][lo] > 0) >= 100, (seed, f, y["counters"])
        seen = set(y["classes"].values())
        assert seen >= set(my.CLASSES), (seed, f, sorted(set(my.CLASSES) - seen))
        assert y["counters"]["ambiguous"] >= 3
    # pairs whose winner fails the filter: their losers keep everything
    a, b = my.counts(rd, mc.L), my.counts(rd, mc.L, f=mc.FILTER)
    assert any(a["clip"][i] > 0 and b["clip"][i] == 0 and my.kept(rd, i, mc.FILTER) for i in range(int(rd["n_reads"])))


# ---- the numpy restatement of the scale test -------------------------------------------------------------------------------------------------------
def test_numpy_restatement_against_the_yardstick():
    rd = mb.head(mb.generate(100001), 2000)                                     # (a prefix: pairs whose mate lies behind it are single records)
    clip, cnt = mb.join(rd)
    y = my.counts(mb.as_reads(rd), mb.L)
    assert cnt == y["counters"] and cnt["pairs"] > 500 and cnt["clipped_reads"] > 400, cnt
    assert np.array_equal(clip, np.array(y["clip"]))
    classes = set(y["classes"].values())
    assert {"single", "not_proper", "same_end"} <= classes, classes
    n_pos = len(y["counts"])
    assert np.array_equal(mb.matrix(rd, n_pos, clip), y["counts"])
    assert not np.array_equal(mb.matrix(rd, n_pos, np.zeros_like(clip)), y["counts"])


# ---- the command line ---------------------------------------------------------------------------------------------------------------------------
def test_cli_refuses_split_ranks_by_name(tmp_path, capsys):
    f = stub_files(tmp_path)
    with pytest.raises(SystemExit) as e:
        cli.GetArgs(_base(f) + ["--mate-overlap", "--gpus", "2"])
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert "--mate-overlap does not go with -i --gpus N" in err and "another rank's block range" in err
    a = cli.GetArgs(_base(f) + ["--mate-overlap"])
    assert a.mate_overlap is True and cli.GetArgs(_base(f)).mate_overlap is False


def test_cli_forwards_the_flag_to_batch_children(tmp_path):
    f = stub_files(tmp_path, names=("x.bam", "r.fa", "f.gff", "m.tsv"))
    args = ["--batch", f["m.tsv"], "-ref", f["r.fa"], "-gff", f["f.gff"], "-cov", "30", "--gpus", "2"]
    on = cli._child_argv(cli.GetArgs(args + ["--mate-overlap", "--min-baseq", "13"]), False)
    assert "--mate-overlap" in on and on[on.index("--min-baseq") + 1] == "13"
    assert "--mate-overlap" not in cli._child_argv(cli.GetArgs(args), False)


def test_stats_keys():
    s = cli.mate_stats(True, {"pairs": 3, "clipped_reads": 2, "clipped_columns": 17, "ambiguous": 4})
    assert s == {"mate_overlap": True, "mate_pairs": 3, "reads_mate_clipped": 2, "columns_mate_clipped": 17, "mate_ambiguous": 4}
    assert cli.mate_stats(False, None) == {"mate_overlap": False, "mate_pairs": 0, "reads_mate_clipped": 0, "columns_mate_clipped": 0, "mate_ambiguous": 0}


def test_bindings_name_the_slot_and_the_entry_points():
    text = open(_ffi.__file__.replace("_ffi.py", "../include/tcmi.h")).read()
    assert "TCMI_K_MATE_JOIN = %d " % _ffi.K_MATE_JOIN in text and "TCMI_K_NKERNELS = %d " % (_ffi.K_MATE_JOIN + 1) in text
    assert hasattr(engine.Context, "set_mate_overlap") and engine.Context.mate_overlap is False
    lib = _ffi.lib()
    assert lib.tcmi_ctx_set_mate_overlap and lib.tcmi_readset_mate_overlap
