"""The variant table without a GPU: the yardstick (tests/variant_yardstick.py) pinned against a hand-written table, the product's rule
(csrc/variants_rule.h) and row writer (csrc/variants_text.cpp) as a program of their own under AddressSanitizer + UBSan against the
yardstick, and the command line's argument handling.  The kernels' tests are tests/test_variant_table.py."""
import struct
from fractions import Fraction

import numpy as np
import pytest

from tests import host_program
from tests import variant_yardstick as vy
from tests.cli_run import base_args as _base
from tests.cli_run import stub_files
from trueconsense_amd import TrueConsense as cli
from trueconsense_amd import _ffi, engine


# min_af = 1/4, min_alt_depth = 2, min_depth = 10, n_ref = 12 over 13 positions        (coverage, A, T, C, G, X, I)
HAND_REF = b"AAcNGTTGARtA"
HAND_COUNTS = np.array([
    (20, 15, 5, 0, 0, 0, 0),        # 0  A: T at exactly 1/4 — the tie is in
    (20, 16, 4, 0, 0, 0, 0),        # 1  A: T one read below the tie
    (40, 0, 0, 30, 10, 0, 0),       # 2  c (lower case): C is the reference allele, G at the tie
    (40, 10, 10, 10, 10, 0, 0),     # 3  N: no record
    (0, 0, 0, 0, 0, 0, 0),          # 4  cov = 0
    (9, 0, 0, 9, 0, 0, 0),          # 5  cov = min_depth - 1
    (10, 0, 0, 9, 0, 0, 1),         # 6  cov = min_depth: C passes, I is below min_alt_depth
    (100, 30, 30, 30, 5, 30, 30),   # 7  G: all five alternates pass, the reference allele is present and left out
    (100, 100, 0, 0, 0, 0, 0),      # 8  A: only the reference allele
    (50, 25, 0, 0, 25, 0, 0),       # 9  R (IUPAC): no record
    (12, 0, 12, 0, 0, 3, 3),        # 10 t: X and I at the tie; T is the reference allele
    (30, 0, 0, 0, 0, 30, 0),        # 11 A: every read deletes the column
    (30, 0, 30, 0, 0, 0, 0),        # 12 p >= n_ref
], np.int32)
HAND_RULE = (1, 4, 2, 10)
HAND_WANT = [(0, 2, 5, 20), (2, 4, 10, 40), (6, 3, 9, 10), (7, 1, 30, 100), (7, 2, 30, 100), (7, 3, 30, 100), (7, 5, 30, 100),
             (7, 6, 30, 100), (10, 5, 3, 12), (10, 6, 3, 12), (11, 5, 30, 30)]
HAND_TEXT = ("ctg\t1\tA\tT\t5\t20\t0.250000\n" "ctg\t3\tC\tG\t10\t40\t0.250000\n" "ctg\t7\tT\tC\t9\t10\t0.900000\n"
             "ctg\t8\tG\tA\t30\t100\t0.300000\n" "ctg\t8\tG\tT\t30\t100\t0.300000\n" "ctg\t8\tG\tC\t30\t100\t0.300000\n"
             "ctg\t8\tG\t*\t30\t100\t0.300000\n" "ctg\t8\tG\t+\t30\t100\t0.300000\n" "ctg\t11\tT\t*\t3\t12\t0.250000\n"
             "ctg\t11\tT\t+\t3\t12\t0.250000\n" "ctg\t12\tA\t*\t30\t30\t1.000000\n")


def test_yardstick_on_the_hand_written_table():
    assert vy.records(HAND_COUNTS, HAND_REF, *HAND_RULE) == HAND_WANT
    assert vy.text(HAND_WANT, "ctg", HAND_REF) == HAND_TEXT
    # min_depth = 0 still needs one read; min_alt_depth = 1 lets position 6's single insertion mark in; the whole reference: position 12
    got = vy.records(HAND_COUNTS, HAND_REF + b"A", 1, 4, 1, 0)
    assert (4, 1, 0, 0) not in got and not any(p == 4 for p, *_ in got)
    assert (5, 3, 9, 9) in got and (6, 6, 1, 10) not in got and (12, 2, 30, 30) in got      # (1 of 10 is below 1/4)
    assert (6, 6, 1, 10) in vy.records(HAND_COUNTS, HAND_REF, 1, 10, 1, 0)
    assert vy.records(HAND_COUNTS, HAND_REF, 0, 1, 1, 0)[:3] == [(0, 2, 5, 20), (1, 2, 4, 20), (2, 4, 10, 40)]   # min_af 0: the depth decides
    assert vy.text([(5, 3, 9, 9)], "x", HAND_REF, pos_offset=4) == "x\t2\tT\tC\t9\t9\t1.000000\n"


def random_matrix(n=2000, seed=11):
    """counts up to 2^31 - 1 (the products with den = 10^6 need 64 bits), ties and near-ties planted at the top of the range"""
    rng = np.random.default_rng(seed)
    c = rng.integers(0, 1 << 31, (n, 7), dtype=np.int64)
    c[rng.random((n, 7)) < 0.3] //= 1 << 20                         # small counters next to large ones
    c[:, 0] = np.where(rng.random(n) < 0.7, c[:, 1:5].sum(1) % (1 << 31), c[:, 0])
    for k, p in enumerate(range(0, n, 50)):                         # cov * 333 333 / 10^6 exactly, one read more, one read less
        cov = 1000000 * int(rng.integers(1, 2147))
        c[p, 0] = cov
        c[p, 1 + k % 6] = cov // 1000000 * 333333 + (k % 3 - 1)
    c[7] = (1 << 31) - 1
    ref = rng.choice(np.frombuffer(b"ACGTacgtACGTNnRY\0", np.uint8), n)
    return c.astype(np.int32), ref.tobytes()


def run_program(prog, tmp_path, tag, counts, ref, rule, region, pos_offset=0):
    inp, rec, txt = (str(tmp_path / (tag + ext)) for ext in (".in", ".rec", ".txt"))
    with open(inp, "wb") as fh:
        fh.write(struct.pack("<8q", len(counts), len(ref), *rule, pos_offset, len(region.encode())))
        fh.write(region.encode() + ref + np.ascontiguousarray(counts, np.int32).tobytes())
    r = host_program.run(prog, inp, rec, txt)
    assert r.stdout.startswith("ok "), (r.stdout[-2000:], r.stderr[-4000:])
    return np.fromfile(rec, vy.DTYPE), open(txt).read()


def test_rule_and_text_program_under_sanitizers(tmp_path):
    """tests/variants_main.cpp + csrc/variants_rule.h + csrc/variants_text.cpp and nothing else, with AddressSanitizer + UBSan, run as
    a program: its records equal the yardstick's, its text a Python formatting of the same records"""
    prog = host_program.build(["tests/variants_main.cpp", "trueconsense_amd/csrc/variants_text.cpp"], tmp_path / "variants_main")
    got, text = run_program(prog, tmp_path, "hand", HAND_COUNTS, HAND_REF, HAND_RULE, "ctg")
    assert got.tolist() == HAND_WANT and text == HAND_TEXT
    counts, ref = random_matrix()
    for tag, rule in (("big", (333333, 1000000, 1, 10)), ("all", (0, 1, 1, 0)), ("one", (1, 1, 1, 0)), ("deep", (1, 1000000, 1 << 30, (1 << 31) - 1))):
        want = vy.records(counts, ref, *rule)
        got, text = run_program(prog, tmp_path, tag, counts, ref, rule, "MN908947.3")
        assert np.array_equal(got, vy.as_array(want)), tag
        assert text == vy.text(want, "MN908947.3", ref), tag
        assert (len(want) > 1500) if tag == "all" else (len(want) > 0 or tag == "deep"), (tag, len(want))
    ties = vy.records(counts, ref, 333333, 1000000, 1, 10)
    assert sum(1 for p, a, c, t in ties if c * 1000000 == 333333 * t) >= 5                 # the planted ties are in (and need 64 bits)
    # a reference shorter than the matrix: nothing from the columns behind it
    want = vy.records(counts[:300], ref[:250], 1, 50, 3, 5)
    got, text = run_program(prog, tmp_path, "part", counts[:300], ref[:250], (1, 50, 3, 5), "seg 2")
    assert got.tolist() == want and text == vy.text(want, "seg 2", ref) and 200 < max(r[0] for r in want) < 250


def test_text_writer_through_the_abi():
    """tcmi_variants_text as Python calls it (no GPU): rows, an offset, and its refusals"""
    recs = vy.as_array(HAND_WANT)
    assert engine.variants_text(recs, "ctg", HAND_REF) == HAND_TEXT
    assert engine.variants_text(recs[2:], "s", HAND_REF, pos_offset=6) == vy.text(HAND_WANT[2:], "s", HAND_REF, 6)
    assert engine.variants_text(recs[:0], "ctg", HAND_REF) == ""
    assert engine.VARIANTS_HEADER == "REGION\tPOS\tREF\tALT\tALT_DP\tTOTAL_DP\tALT_FREQ\n"
    for bad in ([(12, 1, 1, 1)], [(0, 0, 1, 1)], [(0, 7, 1, 1)], [(0, 1, 1, 0)], [(-1, 1, 1, 1)]):
        with pytest.raises(_ffi.TcmiError) as e:
            engine.variants_text(vy.as_array(bad), "ctg", HAND_REF)
        assert e.value.code == _ffi.E_ARG
    with pytest.raises(_ffi.TcmiError):
        engine.variants_text(recs, "ctg", HAND_REF, pos_offset=1)                           # a record in front of the offset


# ------------------------------------------------------------------------------------------------------------- command line


def test_min_af_spellings_and_defaults(tmp_path):
    f = stub_files(tmp_path, ("x.bam", "r.fa", "f.gff", "o.csv.gz"))
    got = [cli.GetArgs(_base(f) + ["--variant-table", "t.tsv", "--min-af", s]).min_af for s in ("0.03", "3e-2", "3/100")]
    assert got == [Fraction(3, 100)] * 3 and all(isinstance(x, Fraction) for x in got)
    assert engine.min_af_fraction("0.03") == engine.min_af_fraction("3e-2") == engine.min_af_fraction("3/100") == (3, 100)
    assert engine.min_af_fraction(0.03) == (3, 100) and engine.min_af_fraction("1") == (1, 1) and engine.min_af_fraction("0") == (0, 1)
    assert engine.min_af_fraction("1/1000000") == (1, 1000000)
    a = cli.GetArgs(_base(f) + ["--variant-table", "t.tsv"])
    assert (a.variant_table, a.min_af, a.min_alt_depth, a.variant_min_depth, a.variant_thresholds_given) == ("t.tsv", Fraction(3, 100), 1, 10, False)
    b = cli.GetArgs(_base(f))
    assert (b.variant_table, b.min_af, b.min_alt_depth, b.variant_min_depth, b.variant_thresholds_given) == (None, Fraction(3, 100), 1, 10, False)
    assert cli.variants_of(a) == dict(min_af=Fraction(3, 100), min_alt_depth=1, min_depth=10)
    c = cli.GetArgs(_base(f) + ["--variant-table", "t.tsv", "--min-alt-depth", "4", "--variant-min-depth", "0", "--min-af", "1/8"])
    assert cli.variants_of(c) == dict(min_af=Fraction(1, 8), min_alt_depth=4, min_depth=0) and c.variant_thresholds_given


@pytest.mark.parametrize("extra", (["--min-af", "1.5"], ["--min-af=-0.1"], ["--min-af", "1/3000001"], ["--min-af", "abc"], ["--min-af", "1/0"],
                                   ["--min-alt-depth", "0"], ["--variant-min-depth", "-1"], ["--min-alt-depth", "2147483648"]))
def test_bad_thresholds_are_refused(tmp_path, capsys, extra):
    f = stub_files(tmp_path, ("x.bam", "r.fa", "f.gff", "o.csv.gz"))
    with pytest.raises(SystemExit) as e:
        cli.GetArgs(_base(f) + ["--variant-table", "t.tsv"] + extra)
    assert e.value.code == 2 and extra[0].split("=")[0] in capsys.readouterr().err


def test_thresholds_need_a_table_and_batch_takes_the_manifest(tmp_path, capsys):
    f = stub_files(tmp_path, ("x.bam", "r.fa", "f.gff", "o.csv.gz"))
    for extra in (["--min-af", "0.1"], ["--min-alt-depth", "3"], ["--variant-min-depth", "20"]):
        with pytest.raises(SystemExit) as e:
            cli.GetArgs(_base(f) + extra)
        assert e.value.code == 2 and "--variant-table" in capsys.readouterr().err
    man = tmp_path / "m.tsv"
    man.write_text("%s\tS0\to0.fa\n%s\tS1\to1.fa\t-\t-\t-\t%s\n%s\tS2\to2.fa\tv.vcf\t\t\t-\n" % (f["x.bam"], f["x.bam"], tmp_path / "t1.tsv", f["x.bam"]))
    batch = ["--batch", str(man), "-ref", f["r.fa"], "-gff", f["f.gff"], "-cov", "30"]
    with pytest.raises(SystemExit) as e:                                # --variant-table itself: refused with --batch, as --index-override is
        cli.GetArgs(batch + ["--variant-table", "t.tsv"])
    assert e.value.code == 2 and "7th column" in capsys.readouterr().err
    a = cli.GetArgs(batch + ["--min-af", "0.2"])
    rows = cli.read_manifest(a)
    assert [r[6] for r in rows] == [None, str(tmp_path / "t1.tsv"), None] and rows[2][3:6] == ["v.vcf", None, None] and rows[0][3:] == [None] * 4
    six = tmp_path / "six.tsv"
    six.write_text("%s\tS0\to0.fa\tv.vcf\tg.gff\td.tsv\n" % f["x.bam"])
    b = cli.GetArgs(["--batch", str(six), "-ref", f["r.fa"], "-gff", f["f.gff"], "-cov", "30"])
    assert cli.read_manifest(b) == [[f["x.bam"], "S0", "o0.fa", "v.vcf", "g.gff", "d.tsv", None]]      # a manifest of before: as before
    with pytest.raises(SystemExit) as e:                                # thresholds, and no line names a table
        cli.read_manifest(cli.GetArgs(["--batch", str(six), "-ref", f["r.fa"], "-gff", f["f.gff"], "-cov", "30", "--min-alt-depth", "2"]))
    assert e.value.code == 1 and "7th column" in capsys.readouterr().out


def test_children_get_the_thresholds_only_when_set(tmp_path):
    f = stub_files(tmp_path, ("x.bam", "r.fa", "f.gff", "o.csv.gz"))
    plain = cli._child_argv(cli.GetArgs(_base(f)), True)
    assert not any(x.startswith(("--min-af", "--variant", "--min-alt")) for x in plain)
    a = cli.GetArgs(_base(f) + ["--variant-table", "t.tsv", "--min-af", "3e-2", "--min-alt-depth", "2"])
    argv = cli._child_argv(a, True)
    assert argv[argv.index("--variant-table") + 1] == "t.tsv" and argv[argv.index("--min-af") + 1] == "3/100"
    back = cli.GetArgs(argv)                                            # a child parses what the parent understood
    assert cli.variants_of(back) == cli.variants_of(a) and back.variant_table == "t.tsv"
    man = tmp_path / "m.tsv"
    man.write_text("%s\tS0\to0.fa\t-\t-\t-\tt0.tsv\n" % f["x.bam"])
    b = cli.GetArgs(["--batch", str(man), "-ref", f["r.fa"], "-gff", f["f.gff"], "-cov", "30", "--variant-min-depth", "7"])
    argv = cli._child_argv(b, False)
    assert "--variant-table" not in argv and argv[argv.index("--variant-min-depth") + 1] == "7"


def test_batch_over_gpus_with_a_mixed_manifest(tmp_path, monkeypatch, capsys):
    """`--batch m.tsv --gpus 2 --min-af 0.05` where one sample of three names a table: the thresholds-without-a-table check is the
    parent's, over the whole manifest; a shard without a table gets no thresholds and its child's own checks pass; the shard with
    the table gets them"""
    f = stub_files(tmp_path, ("x.bam", "r.fa", "f.gff", "o.csv.gz"))
    man = tmp_path / "m.tsv"
    man.write_text("%s\tS0\to0.fa\n%s\tS1\to1.fa\t-\t-\t-\t%s\n%s\tS2\to2.fa\tv.vcf\t\t\t-\n" % (f["x.bam"], f["x.bam"], tmp_path / "t1.tsv", f["x.bam"]))
    seen = []

    def fake_spawn(cmds, envs):                                         # (the shards live as long as the children)
        for cmd in cmds:
            child = cli.GetArgs(cmd[3:])                                # what the child parses ...
            seen.append((cmd[3:], child, cli.read_manifest(child)))     # ... and its manifest check, which must not exit
        return 0
    monkeypatch.setattr("trueconsense_amd.launch._spawn", fake_spawn)
    common = ["-ref", f["r.fa"], "-gff", f["f.gff"], "-cov", "30"]
    cli.main(["--batch", str(man), "--gpus", "2"] + common + ["--min-af", "0.05"])
    assert len(seen) == 2
    (argv0, a0, rows0), (argv1, a1, rows1) = seen
    assert [r[1] for r in rows0] == ["S0", "S2"] and [r[6] for r in rows0] == [None, None]       # shard 0 names no table: no thresholds
    assert "--min-af" not in argv0 and not a0.variant_thresholds_given
    assert [r[1] for r in rows1] == ["S1"] and rows1[0][6] == str(tmp_path / "t1.tsv")
    assert argv1[argv1.index("--min-af") + 1] == "1/20" and a1.min_af == Fraction(1, 20) and a1.variant_thresholds_given
    # no line of the whole manifest names a table: refused once, by the parent, before anything is dealt out
    six = tmp_path / "six.tsv"
    six.write_text("%s\tS0\to0.fa\n%s\tS1\to1.fa\tv.vcf\tg.gff\td.tsv\t-\n" % (f["x.bam"], f["x.bam"]))
    del seen[:]
    with pytest.raises(SystemExit) as e:
        cli.main(["--batch", str(six), "--gpus", "2"] + common + ["--min-alt-depth", "2"])
    assert e.value.code == 1 and not seen and "7th column" in capsys.readouterr().out
    cli.main(["--batch", str(six), "--gpus", "2"] + common)            # without thresholds: dealt out as before
    assert len(seen) == 2 and all("--min-af" not in argv for argv, _, _ in seen)

