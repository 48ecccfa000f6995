"""--codon-table on the command line.  Without a GPU: the argument handling, every refusal by its message, what StreamCounts asks of
the step, and the file's writer (cli_tables.write_codon_table) on hand-written counts.  On the GPU: two changes inside one codon on
the same reads and on different reads, a - strand CDS, --per-contig and the --stats keys, against tests/codon_yardstick.py.  The
kernel's tests are tests/test_codon_counts.py, the rule's tests/test_codon_rule.py."""
import json
import os

import numpy as np
import pytest

from tests import cli_run as cr
from tests import codon_cases as cc
from tests import codon_yardstick as cy
from tests import links_yardstick as ly
from tests import primer_yardstick as py
from tests import read_specs as rsp
from tests import variant_yardstick as vy
from tests.cli_run import base_args as _base
from tests.cli_run import stub_files
from trueconsense_amd import TrueConsense as cli
from trueconsense_amd import _ffi, cli_tables, engine
from trueconsense_amd.io import bamwriter

STAT_KEYS = ("codon_frames", "codon_codons", "codon_rows", "codon_rows_multi")


# ---- without a GPU -----------------------------------------------------------------------------------------------------------------------
def test_parsing_and_the_child_arguments(tmp_path):
    f = stub_files(tmp_path, ("x.bam", "r.fa", "f.gff", "o.csv.gz"))
    a = cli.GetArgs(_base(f) + ["--variant-table", "t.tsv", "--codon-table", "c.tsv"])
    assert a.codon_table == "c.tsv" and cli.codons_of(a) == "c.tsv"
    b = cli.GetArgs(_base(f) + ["--variant-table", "t.tsv"])
    assert b.codon_table is None and cli.codons_of(b) is None and "--codon-table" not in cli._child_argv(b, True)
    argv = cli._child_argv(a, True)                                             # a child parses what the parent understood
    back = cli.GetArgs(argv)
    assert argv[argv.index("--codon-table") + 1] == "c.tsv" and cli.codons_of(back) == "c.tsv" and back.variant_table == "t.tsv"
    assert "--codon-table" not in cli._child_argv(a, False)
    every = cli.GetArgs(_base(f) + ["--variant-table", "t.tsv", "--codon-table", "c.tsv", "--variant-strand", "--variant-links", "l.tsv", "--indel-table", "i.tsv",
                                    "--variant-evidence", "e.tsv", "--min-baseq", "13", "--min-mapq", "20", "--mate-overlap", "--dedup", "--per-contig"])
    assert cli.codons_of(every) == "c.tsv" and every.per_contig


def test_what_the_step_is_asked_for(tmp_path):
    f = stub_files(tmp_path, ("x.bam", "r.fa", "f.gff"))
    a = cli.GetArgs(_base(f) + ["--variant-table", "t.tsv", "--codon-table", "c.tsv", "--min-af", "1/20", "--min-alt-depth", "2", "--variant-min-depth", "7"])
    want = cli_tables.StreamCounts(a)
    assert want and want.need == "--codon-table" and want.codons == "c.tsv" and want.lists_records
    assert want.variants == cli.variants_of(a) and want.variants["min_alt_depth"] == 2 and want.variants["min_depth"] == 7
    assert "codon_counts" not in cli_tables.StreamCounts.KEYS and cli_tables.StreamCounts.KEYS == ("amplicon_reads", "variant_strand", "variant_links")
    assert want.split_kwargs("ACGT") == dict(amplicon_reads=None, variant_strand=None, variant_links=None)
    both = cli_tables.StreamCounts(cli.GetArgs(_base(f) + ["--variant-table", "t.tsv", "--codon-table", "c.tsv", "--variant-links", "l.tsv"]))
    assert both.need == "--variant-links" and both.codons == "c.tsv"
    none = cli_tables.StreamCounts(cli.GetArgs(_base(f) + ["--variant-table", "t.tsv"]))
    assert not none and none.codons is None and none.need is None and not none.lists_records


def test_refusals_exit_1_with_one_line_and_write_nothing(tmp_path, capsys, monkeypatch):
    monkeypatch.chdir(tmp_path)
    f = stub_files(tmp_path, ("x.bam", "r.fa", "f.gff", "o.csv.gz"))
    man = tmp_path / "m.tsv"
    man.write_text("%s\tS0\to0.fa\t-\t-\t-\tt0.tsv\n" % f["x.bam"])
    batch = ["--batch", str(man), "-ref", f["r.fa"], "-gff", f["f.gff"], "-cov", "30"]
    before = sorted(os.listdir(tmp_path))
    for argv, word in ((_base(f) + ["--codon-table", "c.tsv"], "--codon-table needs --variant-table."),
                       (batch + ["--codon-table", "c.tsv"], "--codon-table goes with a single sample (-i): --batch is refused, its file runner has no hook behind its steps."),
                       (batch + ["--codon-table", "c.tsv", "--gpus", "2"], "--batch is refused"),
                       (_base(f) + ["--variant-table", "t.tsv", "--codon-table", "c.tsv", "--index-override", f["o.csv.gz"]],
                        "--codon-table does not go with --index-override: the overridden matrix no longer equals the reads."),
                       (_base(f) + ["--variant-table", "t.tsv", "--codon-table", "c.tsv", "--gpus", "2"],
                        "--codon-table does not go with -i --gpus N: the ranks' counters would have to be added up on rank 0, which is not built.")):
        for call in (cli.GetArgs, cli.main):
            with pytest.raises(SystemExit) as e:
                call(argv)
            out = capsys.readouterr().out
            assert e.value.code == 1 and word in out and out.count("\n") == 1 and out.endswith("Exiting...\n"), (argv, out)
    assert sorted(os.listdir(tmp_path)) == before
    ok = cli.GetArgs(_base(f) + ["--variant-table", "t.tsv", "--codon-table", "c.tsv", "--gpus", "1"])       # one GPU is no split
    assert ok.codon_table == "c.tsv"


def _namespace(tmp_path, flag=True):
    f = stub_files(tmp_path, ("x.bam", "r.fa", "f.gff"))
    return cli.GetArgs(_base(f) + ["--variant-table", str(tmp_path / "t.tsv")] + (["--codon-table", str(tmp_path / "c.tsv")] if flag else []))


def test_write_codon_table_on_hand_written_counts(tmp_path):
    a = _namespace(tmp_path)
    want = cli_tables.StreamCounts(a)
    counts, frames, names, matrix, ref = cc.hand_part()
    part = cli_tables.CodonPart(counts, frames, names, "chr", ref, 0, matrix)
    assert cli_tables.CodonPart._fields == ("counts", "frames", "names", "region", "ref", "pos_offset", "matrix")
    stats = cli_tables.write_codon_table(a, [part], want)
    text = cy.text(counts, frames.tolist(), names, "chr", ref, 3, 100, 1, 10)
    assert open(a.codon_table).read() == engine.CODONS_HEADER + text and engine.CODONS_HEADER == cy.HEADER
    assert [ln.split("\t")[7:11] for ln in text.splitlines()] == [["ATA", "I", "MIS", "1"], ["TTA", "L", "MIS", "2"], ["GCT", "A", "SYN", "1"]]
    assert stats == dict(codon_frames=1, codon_codons=2, codon_rows=3, codon_rows_multi=1) and tuple(stats) == STAT_KEYS
    # two parts: a second contig 512 columns up the axis, its rows with its own positions behind the first one's
    c2, f2, n2, m2, r2 = cc.hand_part(512)
    m2[:12] = matrix
    axis = ref + r2[12:]
    got = {"codon_counts": np.concatenate([counts, c2])}
    parts = [cli_tables.codon_part_of_columns(got, np.concatenate([frames, f2]), names + ["orfB"], m2, lo, lo + 12, rid, axis[:lo + 12], lo)
             for lo, rid in ((0, "c0"), (512, "c1"))]
    assert [len(p.counts) for p in parts] == [2, 2] and [p.names for p in parts] == [["orfA"], ["orfB"]] and parts[1].frames.tolist() == f2.tolist()
    stats = cli_tables.write_codon_table(a, parts, want)
    assert open(a.codon_table).read() == engine.CODONS_HEADER + text.replace("chr\t", "c0\t") + text.replace("chr\t", "c1\t").replace("orfA", "orfB")
    assert stats == dict(codon_frames=2, codon_codons=4, codon_rows=6, codon_rows_multi=2)
    # no codons, no frames: the header alone; without the flag: nothing written, zeros
    empty = cli_tables.CodonPart(counts[:0], frames[:0], [], "chr", ref, 0, matrix)
    assert cli_tables.write_codon_table(a, [empty], want) == dict.fromkeys(STAT_KEYS, 0) and open(a.codon_table).read() == engine.CODONS_HEADER
    os.remove(a.codon_table)
    off = _namespace(tmp_path, False)
    assert cli_tables.write_codon_table(off, [part], cli_tables.StreamCounts(off)) == dict.fromkeys(STAT_KEYS, 0) and not os.path.exists(a.codon_table)


def test_a_broken_invariant_leaves_the_file_unwritten(tmp_path):
    a = _namespace(tmp_path)
    want = cli_tables.StreamCounts(a)
    counts, frames, names, matrix, ref = cc.hand_part()
    good = cli_tables.CodonPart(counts, frames, names, "chr", ref, 0, matrix)
    bad = counts.copy()
    bad[1]["j"][4, 3, 1] += 1
    with pytest.raises(_ffi.TcmiError) as e:
        cli_tables.write_codon_table(a, [good, cli_tables.CodonPart(bad, frames, names, "chr", ref, 0, matrix)], want)
    assert e.value.code == _ffi.E_ARG and not os.path.exists(a.codon_table)
    with open(a.codon_table, "w") as fh:                                        # ... and a file of before as it was
        fh.write("kept")
    with pytest.raises(_ffi.TcmiError):
        cli_tables.write_codon_table(a, [cli_tables.CodonPart(bad, frames, names, "chr", ref, 0, matrix)], want)
    assert open(a.codon_table).read() == "kept"


# ---- on the GPU --------------------------------------------------------------------------------------------------------------------------
def yardstick(specs, ref, frames, names, region="ref"):
    """-> (the codon table's rows, the variant records, the codons' records) of the yardsticks at the command line's default thresholds"""
    rd = rsp.arrays(specs)
    whole = py.counts(rd, cc.CL)[0]
    recs = vy.records(whole, ref.encode(), 3, 100, 1, 10)
    c0s = cy.select(recs, frames)
    counts = cy.joint(ly.classes(rd, cc.CL, n_pos=len(whole)), cy.ins_marks(rd, cc.CL, n_pos=len(whole)), c0s)
    assert not cy.invariant(counts, whole)
    return cy.text(counts, frames, names, region, ref.encode(), 3, 100, 1, 10), recs, counts


def phases_of(path):
    return [ln.split("\t")[-1] for ln in open(path).read().splitlines()[1:]]


@pytest.mark.gpu
def test_two_changes_in_one_codon_on_the_same_reads_and_on_different_reads(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    plus, minus = [{"start": cc.CDS_START + 1, "end": 270, "strand": "+"}], [{"start": cc.CDS_START + 1, "end": 270, "strand": "-"}]
    f_plus, f_minus = [(cc.CDS_START, 270, 1, 0)], [(cc.CDS_START, 270, -1, 0)]
    tables = {}
    for cis in (True, False):
        tag = "cis" if cis else "trans"
        ref, specs = cc.cli_case(cis)
        want, recs, counts = yardstick(specs, ref, f_plus, ["orf0"])
        assert [(p, a) for p, a, *_ in recs] == [(cc.CODON, 1), (cc.CODON + 1, 1)] and counts["pos"].tolist() == [cc.CODON]      # the same two rows of the variant table
        bamwriter.write_bam(tag + ".bam", rsp.arrays(specs), ref_len=cc.CL, block=4096)
        common = cr.setup_cli(ref, plus)
        cr.run_cli(monkeypatch, ["-i", tag + ".bam", "-name", "S"] + common + cr.out_args(tag) + ["--variant-table", tag + ".var", "--variant-links", tag + ".lnk",
                                                                                                  "--codon-table", tag + ".cod", "--stats", tag + ".json"])
        assert open(tag + ".cod").read() == engine.CODONS_HEADER + want
        rows = [ln.split("\t") for ln in want.splitlines()]
        number = str((cc.CODON - cc.CDS_START) // 3 + 1)
        if cis:                                                                 # GGG -> AAG on a third of the reads: one row, K, neither R nor E
            assert [r[:11] for r in rows] == [["ref", "orf0", "+", number, str(cc.CODON + 1), "GGG", "G", "AAG", "K", "MIS", "2"]]
            assert rows[0][11:] == ["20", "60", "%.6f" % (20 / 60), "0", "0", "0"] and phases_of(tag + ".lnk") == ["CIS"]
        else:                                                                   # AGG on a third, GAG on another: two rows, R and E
            assert [r[7:11] for r in rows] == [["AGG", "R", "MIS", "1"], ["GAG", "E", "MIS", "1"]] and phases_of(tag + ".lnk") == ["TRANS"]
        stats = json.load(open(tag + ".json"))
        assert {k: stats[k] for k in STAT_KEYS} == dict(codon_frames=1, codon_codons=1, codon_rows=len(rows), codon_rows_multi=int(cis))
        tables[tag] = open(tag + ".var").read()
        # without the flag: every other output byte for byte, no file, no keys
        cr.run_cli(monkeypatch, ["-i", tag + ".bam", "-name", "S"] + common + cr.out_args(tag + "0") + ["--variant-table", tag + "0.var", "--variant-links", tag + "0.lnk",
                                                                                                        "--stats", tag + "0.json"])
        assert cr.outputs(tag) == cr.outputs(tag + "0") and open(tag + "0.var").read() == tables[tag] and open(tag + "0.lnk").read() == open(tag + ".lnk").read()
        assert not any(k in json.load(open(tag + "0.json")) for k in STAT_KEYS) and not os.path.exists(tag + "0.cod")
        # the same columns under a - strand CDS: the reverse-complement codons
        want_m, _, _ = yardstick(specs, ref, f_minus, ["orf0"])
        common = cr.setup_cli(ref, minus)
        cr.run_cli(monkeypatch, ["-i", tag + ".bam", "-name", "S"] + common + ["-o", tag + "m.fa", "--variant-table", tag + "m.var", "--codon-table", tag + "m.cod"])
        assert open(tag + "m.cod").read() == engine.CODONS_HEADER + want_m and open(tag + "m.var").read() == tables[tag]
        rows_m = [ln.split("\t") for ln in want_m.splitlines()]
        assert [r[2:9] for r in rows_m] == ([["-", "58", str(cc.CODON + 1), "CCC", "P", "CTT", "L"]] if cis else
                                            [["-", "58", str(cc.CODON + 1), "CCC", "P", "CCT", "P"], ["-", "58", str(cc.CODON + 1), "CCC", "P", "CTC", "L"]])
        # a GFF without a usable CDS row: the header and no rows
        with open("g.gff", "w") as fh:
            fh.write("##gff-version 3\nref\tsynthetic\tgene\t31\t270\t.\t+\t.\tID=g0\nref\tsynthetic\tCDS\t31\t270\t.\t.\t0\tID=c0\n")
        cr.run_cli(monkeypatch, ["-i", tag + ".bam", "-name", "S", "-ref", "r.fa", "-gff", "g.gff", "-cov", "10", "-o", tag + "n.fa", "--variant-table", tag + "n.var",
                                 "--codon-table", tag + "n.cod"])
        assert open(tag + "n.cod").read() == engine.CODONS_HEADER and open(tag + "n.var").read() == tables[tag]
    assert tables["cis"] == tables["trans"]                                     # the variant table cannot tell the two files apart


@pytest.mark.gpu
def test_per_contig_gives_the_same_rows_under_two_regions(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    from trueconsense_amd import synthetic as syn
    ref, specs = cc.cli_case(True)
    orfs = [{"start": cc.CDS_START + 1, "end": 270, "strand": "+"}]
    want, recs, _ = yardstick(specs, ref, [(cc.CDS_START, 270, 1, 0)], ["orf0"])
    two = sorted([dict(r, tid=t, name="%s_%d" % (r["name"], t)) for t in (0, 1) for r in specs], key=lambda r: (r["tid"], r["pos"]))
    bamwriter.write_bam("P.bam", rsp.arrays(two), refs=[("c0", cc.CL), ("c1", cc.CL)], block=4096)
    with open("p.fa", "w") as fh:
        fh.write(">c0\n%s\n>c1\n%s\n" % (ref, ref))
    with open("p.gff", "w") as fh:
        fh.write("##gff-version 3\n" + syn.gff_text(orfs, seqid="c0")[1] + syn.gff_text(orfs, seqid="c1")[1])
    cr.run_cli(monkeypatch, ["-i", "P.bam", "-ref", "p.fa", "-gff", "p.gff", "-cov", "10", "-name", "S", "--per-contig", "-o", "p.fa.out", "--variant-table", "p.var",
                             "--codon-table", "p.cod", "--stats", "p.json"])
    assert want and open("p.cod").read() == engine.CODONS_HEADER + want.replace("ref\t", "c0\t") + want.replace("ref\t", "c1\t")
    sp = json.load(open("p.json"))
    assert {k: sp[k] for k in STAT_KEYS} == dict(codon_frames=2, codon_codons=2, codon_rows=2, codon_rows_multi=2) and sp["variant_records"] == 2 * len(recs)
    cr.run_cli(monkeypatch, ["-i", "P.bam", "-ref", "p.fa", "-gff", "p.gff", "-cov", "10", "-name", "S", "--per-contig", "-o", "q.fa.out", "--variant-table", "q.var",
                             "--stats", "q.json"])
    assert open("q.var").read() == open("p.var").read() and open("q.fa.out").read() == open("p.fa.out").read()
    assert not any(k in json.load(open("q.json")) for k in STAT_KEYS)
