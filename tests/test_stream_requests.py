"""The counts taken behind the step — --amplicon-reads, --variant-strand, --variant-links — as the command line asks for them:
cli_tables.StreamCounts (one request for every runner), cli_tables.write_tables (one writer), cli_args.GetArgs' refusals, and
distributed._agree / _sum_to_root (the ranks' agreement and the one sum to rank 0) over a real two-process gloo group.  The gpu-marked
tests run the three flags at once through every runner: each file must be the one the same runner writes under that flag alone."""
import itertools
import json
import os
import signal
import socket
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

from tests import amplicon_reads_cases as arc
from tests import cli_run as cr
from tests import link_cases as lkc
from tests import read_specs as rsp
from tests import schemes as sch
from tests import sum_ranks
from trueconsense_amd import TrueConsense as cli
from trueconsense_amd import _ffi, engine
from trueconsense_amd import distributed as td
from trueconsense_amd import synthetic as syn
from trueconsense_amd.io import bamwriter


# ---- the agreement and the sum ------------------------------------------------------------------------------------------------------
def test_sum_to_root_without_a_group():
    mine = np.arange(28, dtype=np.int32).reshape(2, 14)
    assert td._sum_to_root("strand counts", lambda: mine, None, False) is mine
    assert td._agree(None, None, False) is None and td._agree((-3, "x"), None, False) == (-3, "x")

    def refused():
        raise _ffi.TcmiError(_ffi.E_UNSUPPORTED, "gone")
    with pytest.raises(_ffi.TcmiError) as e:
        td._sum_to_root("link counts", refused, None, False)
    assert e.value.code == _ffi.E_UNSUPPORTED and str(e.value) == "libtcmi error -9: consensus_split_bamfile: link counts: libtcmi error -9: gone"


def test_agree_and_sum_to_root_over_gloo():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ, PYTHONPATH=cr.ROOT)
    procs = [subprocess.Popen([sys.executable, "-m", "tests.sum_ranks", str(r), str(port)], env=env, cwd=cr.ROOT, stdout=subprocess.PIPE,
                              stderr=subprocess.PIPE, text=True) for r in (0, 1)]
    try:
        outs = [p.communicate(timeout=60) for p in procs]
    finally:
        for p in procs:                                     # (a rank that waits for the other past the limit: neither is left behind)
            if p.poll() is None:
                p.kill()
                p.communicate()
    assert [p.returncode for p in procs] == [0, 0], [o[1][-1500:] for o in outs]
    got = [json.loads(o[0].strip().splitlines()[-1]) for o in outs]
    for rank, g in enumerate(got):
        assert g["agree_root"] == [-3, "rank 0"] and g["agree_other"] == [-4, "rank 1"] and g["agree_both"] == [-3, "rank 0"] and g["agree_none"] is None
        code = _ffi.E_NOMEM
        assert g["refused"] == [code, "libtcmi error %d: consensus_split_bamfile: %s: libtcmi error %d: %s" % (code, sum_ranks.WHAT, code, sum_ranks.MSG)]
        assert g["empty_untouched"] is True and g["barrier"] is True
    assert got[0]["sum"] == (sum_ranks.own_array(0) + sum_ranks.own_array(1)).tolist() == [[11, 22], [33, 44], [55, 66]]


# ---- the request ----------------------------------------------------------------------------------------------------------------------
FLAGS = {"reads": ["--amplicon-reads", "r.tsv", "--amplicon-reads-slack", "7"], "strand": ["--variant-strand", "--strand-ratio", "1/5"],
         "links": ["--variant-links", "l.tsv", "--link-neighbours", "3"]}
ZERO = dict(variant_records=0, variant_strand_bias=0, variant_strand_low=0, variant_link_rows=0, variant_links_cis=0, variant_links_trans=0,
            variant_links_mixed=0, variant_links_none=0, variant_links_low=0, variant_evidence_lowq=0, variant_evidence_lowmq=0, variant_evidence_end=0)


def _parsed(f, which):
    """-> (the namespace of `which` flags, the namespace a --gpus child parses from it); x.bam is no BAM: the reference's name comes from -ref"""
    table = ["--variant-table", "t.tsv", "--min-af", "1/20"] if which != ("reads",) else []
    a = cli.GetArgs(cr.base_args(f) + table + (["--amplicon-scheme", f["s.bed"]] if "reads" in which else []) + [x for w in which for x in FLAGS[w]])
    back = cli.GetArgs(cli._child_argv(a, True))
    a.input = back.input = None
    return a, back


@pytest.mark.parametrize("which", [c for n in (1, 2, 3) for c in itertools.combinations(("reads", "strand", "links"), n)])
def test_need_names_one_flag(tmp_path, which):
    a, back = _parsed(sch.scheme_files(tmp_path), which)
    for ns in (a, back):
        want = cli.StreamCounts(ns)
        assert want and want.need == ("--variant-strand" if "strand" in which else "--variant-links" if "links" in which else "--amplicon-reads")
        assert want.lists_records == ("strand" in which or "links" in which)
        assert (bool(want.areads), bool(want.srule), bool(want.links)) == tuple(w in which for w in ("reads", "strand", "links"))


def test_the_empty_request(tmp_path):
    a = cli.GetArgs(cr.base_args(sch.scheme_files(tmp_path)))
    want = cli.StreamCounts(a)
    assert not want and want.need is None and not want.lists_records
    assert want.stats() == want.stats({}) == dict(amplicon_reads_ambiguous=0, amplicon_reads_unassigned=0)
    assert want.split_kwargs("ACGT") == dict(amplicon_reads=None, variant_strand=None, variant_links=None)
    assert want.from_parts(("text", "counts", {})) == ({}, None)
    assert cli.write_tables(a, [], want) == ZERO and list(cli.write_tables(a, [], want)) == list(ZERO)

    class NoCalls:                                          # (nothing is asked of the context)
        pass
    assert want.count(NoCalls(), None) == {}


def test_split_keywords_and_parts(tmp_path):
    a, back = _parsed(sch.scheme_files(tmp_path), ("reads", "strand", "links"))
    for ns in (a, back):
        want, areads = cli.StreamCounts(ns), cli.amplicon_reads_of(ns)
        var = dict(cli.variants_of(ns), ref="ACGT")
        assert var == dict(min_af=Fraction(1, 20), min_alt_depth=1, min_depth=10, ref="ACGT") and areads[2] == 7
        assert want.split_kwargs("ACGT") == dict(amplicon_reads=areads[1:], variant_strand=var, variant_links=(var, 3))
        assert want.stats({"amplicon_reads": {"reads": np.array([5, 4, 3, 2])}}) == dict(amplicon_reads_ambiguous=3, amplicon_reads_unassigned=2)
    # rank 0's tuple: one item per count asked for, in the order amplicon reads, strand, links
    parts = ("text", "counts", {}, "R", ("recs", "S"), ("recs", "K"))
    assert cli.StreamCounts(a).from_parts(parts) == (dict(amplicon_reads="R", variant_strand="S", variant_links="K"), "recs")
    for which, tail, got in ((("strand",), (("recs", "S"),), dict(variant_strand="S")), (("links",), (("recs", "K"),), dict(variant_links="K")),
                             (("reads", "links"), ("R", ("recs", "K")), dict(amplicon_reads="R", variant_links="K")),
                             (("strand", "links"), (("recs", "S"), ("recs", "K")), dict(variant_strand="S", variant_links="K"))):
        one = _parsed(sch.scheme_files(tmp_path), which)[0]
        assert cli.StreamCounts(one).from_parts(parts[:3] + tail) == (got, "recs")
    only = _parsed(sch.scheme_files(tmp_path), ("reads",))[0]
    assert cli.StreamCounts(only).from_parts(parts[:4]) == (dict(amplicon_reads="R"), None)
    assert cli.StreamCounts(only).split_kwargs("ACGT") == dict(amplicon_reads=cli.amplicon_reads_of(only)[1:], variant_strand=None, variant_links=None)


def test_count_fetches_the_records_once():
    class Want(cli.StreamCounts):
        def __init__(self, areads, srule, links):           # (the settings as the parsed namespace gives them)
            self.areads, self.srule, self.links, self.lists_records = areads, srule, links, bool(srule or links)

    class Ctx:
        def __init__(self):
            self.calls = []

        def __getattr__(self, name):
            return lambda *args, **kw: self.calls.append((name,) + args) or name
    ctx = Ctx()
    got = Want(("amps", [(1, 2, 3, 4)], 5), dict(strand_ratio=1), ("l.tsv", 2, {})).count(ctx, "rs")
    assert got == dict(amplicon_reads="amplicon_reads", variant_strand="strand_counts_of", variant_links="link_counts_of") and list(got) == list(cli.StreamCounts.KEYS)
    assert ctx.calls == [("amplicon_reads", "rs", [(1, 2, 3, 4)], 5), ("step_variants",), ("strand_counts_of", "rs", "step_variants"),
                         ("link_counts_of", "rs", "step_variants", 2)]
    ctx = Ctx()
    Want(None, None, ("l.tsv", 7, {})).count(ctx, "rs", records="given")
    assert ctx.calls == [("link_counts_of", "rs", "given", 7)]
    ctx = Ctx()
    Want(("amps", [], 0), None, None).count(ctx, "rs")
    assert ctx.calls == [("amplicon_reads", "rs", [], 0)]


# ---- GetArgs' refusals: the lines of before, word for word --------------------------------------------------------------------------
STRAND_LINES = ("--strand-min-depth / --strand-ratio need --variant-strand. Exiting...",
                "--variant-strand goes with a single sample (-i): --batch is refused, its file runner has no hook behind its steps. Exiting...",
                "--variant-strand needs --variant-table. Exiting...",
                "--variant-strand does not go with --index-override: the overridden matrix no longer equals the reads. Exiting...")
LINKS_LINES = ("--link-neighbours / --link-min-depth / --link-ratio need --variant-links. Exiting...",
               "--variant-links goes with a single sample (-i): --batch is refused, its file runner has no hook behind its steps. Exiting...",
               "--variant-links needs --variant-table. Exiting...",
               "--variant-links does not go with --index-override: the overridden matrix no longer equals the reads. Exiting...")


@pytest.mark.parametrize("flag, dependant, lines", ((["--variant-strand"], ["--strand-ratio", "1/5"], STRAND_LINES),
                                                    (["--variant-links", "l.tsv"], ["--link-min-depth", "5"], LINKS_LINES)))
def test_refusals_word_for_word(tmp_path, capsys, flag, dependant, lines):
    f = sch.scheme_files(tmp_path)
    (tmp_path / "o.csv.gz").write_text("x")
    man = tmp_path / "m.tsv"
    man.write_text("%s\tS0\to0.fa\t-\t-\t-\tt0.tsv\n" % f["x.bam"])
    batch = ["--batch", str(man), "-ref", f["r.fa"], "-gff", f["f.gff"], "-cov", "30"]
    table = ["--variant-table", "t.tsv"]
    for argv, line in zip((cr.base_args(f) + table + dependant, batch + flag, cr.base_args(f) + flag,
                           cr.base_args(f) + table + flag + ["--index-override", str(tmp_path / "o.csv.gz")]), lines):
        with pytest.raises(SystemExit) as e:
            cli.GetArgs(argv)
        said = capsys.readouterr()
        assert e.value.code == 1 and said.out == line + "\n" and said.err == "", argv


def test_strand_is_refused_before_links(tmp_path, capsys):
    f = sch.scheme_files(tmp_path)
    for order in ((["--link-min-depth", "5"], ["--strand-min-depth", "5"]), (["--strand-min-depth", "5"], ["--link-min-depth", "5"])):
        with pytest.raises(SystemExit) as e:
            cli.GetArgs(cr.base_args(f) + ["--variant-table", "t.tsv"] + order[0] + order[1])
        assert e.value.code == 1 and capsys.readouterr().out == STRAND_LINES[0] + "\n"
    # ... and both before the parser's own errors (exit 2): thresholds of a table that is not asked for
    with pytest.raises(SystemExit) as e:
        cli.GetArgs(cr.base_args(f) + ["--min-af", "0.1", "--variant-links", "l.tsv"])
    assert e.value.code == 1 and capsys.readouterr().out == LINKS_LINES[2] + "\n"


# ---- the three flags at once, through every runner ------------------------------------------------------------------------------------
OWNED = {"strand": ("variant_strand_bias", "variant_strand_low"), "links": tuple(k for k in ZERO if k.startswith("variant_link")),
         "reads": ("amplicon_reads_ambiguous", "amplicon_reads_unassigned")}


def _cli_case(tmp_path, two_contigs=False, split_records=False):
    """tests/link_cases.cli_case (720 reads of 100 bases over 1 200 columns; its two-contig copy) in the working directory, and a
    scheme of two overlapping amplicons on every reference -> the command line's common arguments"""
    ref, orfs, specs = lkc.cli_case()
    amps = arc.tiled(2, 30, 500, 650)
    sch.write_scheme("s.bed", [r for chrom in ("ref", "c0", "c1") for r in arc.scheme_rows_for(chrom, amps)])
    if not two_contigs:
        bamwriter.write_bam("A.bam", rsp.arrays(specs), ref_len=lkc.CL, block=4096, split_records=split_records)
        return ["-i", "A.bam", "-name", "S"] + cr.setup_cli(ref, orfs)
    two = sorted([dict(r, tid=t, name="%s_%d" % (r["name"], t)) for t in (0, 1) for r in specs], key=lambda r: (r["tid"], r["pos"]))
    bamwriter.write_bam("P.bam", rsp.arrays(two), refs=[("c0", lkc.CL), ("c1", lkc.CL)], block=4096)
    with open("p.fa", "w") as fh:
        fh.write(">c0\n%s\n>c1\n%s\n" % (ref, ref))
    with open("p.gff", "w") as fh:
        fh.write("##gff-version 3\n" + syn.gff_text(orfs, seqid="c0")[1] + syn.gff_text(orfs, seqid="c1")[1])
    return ["-i", "P.bam", "-ref", "p.fa", "-gff", "p.gff", "-cov", "10", "-name", "S", "--per-contig"]


def _asked(tag, which):
    """the flags of `which` for the run `tag`: its files are tag.var, tag.lnk, tag.reads"""
    out = ["-o", tag + ".fa"]
    if "strand" in which or "links" in which:
        out += ["--variant-table", tag + ".var"]
    if "strand" in which:
        out += ["--variant-strand"]
    if "links" in which:
        out += ["--variant-links", tag + ".lnk"]
    if "reads" in which:
        out += ["--amplicon-reads", tag + ".reads", "--amplicon-scheme", "s.bed"]
    return out


def _same_files_as_alone():
    """all.* against strand.var, links.lnk, reads.reads (and the plain table links.var against the strand table's first columns)"""
    read = lambda p: open(p).read()
    assert read("all.var") == read("strand.var") and read("all.var").startswith(engine.VARIANTS_STRAND_HEADER) and read("all.var").count("\n") > 8
    assert read("all.lnk") == read("links.lnk") and read("all.lnk").startswith(engine.VARIANTS_LINKS_HEADER) and read("all.lnk").count("\n") > 8
    assert read("all.reads") == read("reads.reads") and read("all.reads").startswith(engine.AMPLICON_READS_HEADER)
    assert [ln.split("\t")[:7] for ln in read("all.var").splitlines()[1:]] == [ln.split("\t") for ln in read("links.var").splitlines()[1:]]
    assert read("all.fa") == read("strand.fa") == read("links.fa") == read("reads.fa")
    assert not any(os.path.exists(p) for p in ("strand.lnk", "strand.reads", "links.reads", "reads.var", "reads.lnk"))


@pytest.mark.gpu
@pytest.mark.parametrize("two_contigs", (False, True))
def test_three_flags_at_once_in_process(tmp_path, monkeypatch, two_contigs):
    """the single-sample runner, and --per-contig on the two-contig copy"""
    monkeypatch.chdir(tmp_path)
    common = _cli_case(tmp_path, two_contigs)
    for tag, which in (("all", ("strand", "links", "reads")), ("strand", ("strand",)), ("links", ("links",)), ("reads", ("reads",))):
        cr.run_cli(monkeypatch, common + _asked(tag, which) + ["--stats", tag + ".json"])
    _same_files_as_alone()
    stats = {tag: json.load(open(tag + ".json")) for tag in ("all", "strand", "links", "reads")}
    assert open("all.reads").read().count("\n") == 1 + (4 if two_contigs else 2) + 2       # the header, every contig's two amplicons, *ambiguous and *unassigned
    for tag, keys in OWNED.items():
        assert set(stats[tag]) == set(stats["all"])
        assert {k: stats["all"][k] for k in keys} == {k: stats[tag][k] for k in keys}
        assert all(stats[other][k] == 0 for other in OWNED if other != tag for k in keys)
    assert stats["all"]["variant_records"] == stats["strand"]["variant_records"] == stats["links"]["variant_records"] > 0 == stats["reads"]["variant_records"]
    assert stats["all"]["variant_link_rows"] > 0 and stats["all"]["variant_links_cis"] > 0
    assert stats["all"]["amplicon_reads_ambiguous"] > 0 and stats["all"]["amplicon_reads_unassigned"] > 0


@pytest.mark.gpu
def test_three_flags_at_once_over_two_gpus(tmp_path, monkeypatch):
    """--gpus 2 (two ranks rehearsed on this one GPU, gloo for the exchange); the four runs side by side: eight ranks on the card"""
    monkeypatch.chdir(tmp_path)
    common = _cli_case(tmp_path, split_records=True)
    env = dict(os.environ, TCMI_SPLIT_ONE_GPU="1", TCMI_SPLIT_BACKEND="gloo", PYTHONPATH=cr.ROOT)
    runs = (("all", ("strand", "links", "reads")), ("strand", ("strand",)), ("links", ("links",)), ("reads", ("reads",)))
    procs = [subprocess.Popen([sys.executable, "-m", "trueconsense_amd.TrueConsense"] + common + _asked(tag, which) + ["--gpus", "2", "-t", "2"], env=env,
                              stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, start_new_session=True) for tag, which in runs]
    try:
        outs = [p.communicate(timeout=300) for p in procs]
    finally:
        for p in procs:                                     # (a run past the limit: its ranks go with it)
            if p.poll() is None:
                os.killpg(p.pid, signal.SIGKILL)
                p.communicate()
    assert [p.returncode for p in procs] == [0] * 4, [o[1][-1500:] for o in outs]
    _same_files_as_alone()
