"""Driving the command line from the tests: the repository's root, stand-in input files for the argument parser, the process's own
cli.main, the four output files of a run, and a fresh child process under the two-ranks-on-one-GPU environment.  No tests in here;
nothing here touches a GPU when it is imported."""
import gzip
import os
import subprocess
import sys

from trueconsense_amd import TrueConsense as cli
from trueconsense_amd import _ffi
from trueconsense_amd import synthetic as sy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def stub_files(tmp_path, names=("x.bam", "r.fa", "f.gff")):
    """files the argument parser only has to find -> {name: path}"""
    p = {}
    for name in names:
        (tmp_path / name).write_text("x")
        p[name] = str(tmp_path / name)
    return p


def base_args(f, out="out.fa"):
    return ["-i", f["x.bam"], "-ref", f["r.fa"], "-gff", f["f.gff"], "-cov", "30", "-name", "S", "-o", out]


def run_cli(monkeypatch, args):
    monkeypatch.setattr(sys, "argv", ["TrueConsense", "ARGS"])
    cli.main(args)


def out_args(t):
    return ["-o", t + ".fa", "-vcf", t + ".vcf", "-ogff", t + ".gff", "-doc", t + ".tsv"]


def outputs(tag):
    """FASTA, GFF, TSV and the VCF outside its ## header lines"""
    vcf = [ln for ln in open(tag + ".vcf") if not ln.startswith("##")]
    return open(tag + ".fa").read(), open(tag + ".gff").read(), open(tag + ".tsv").read(), vcf


def doc_column(path):
    return [int(ln.split("\t")[1]) for ln in open(path).read().split("\n") if ln.strip()]


def gff_rows(orfs):
    return [{"start": o["start"], "end": o["end"], "strand": o["strand"]} for o in orfs]


def setup_cli(ref, orfs, seqid="ref"):
    """r.fa and g.gff in the working directory -> the arguments that name them"""
    open("r.fa", "w").write(">%s x\n%s\n" % (seqid, ref))
    head, body = sy.gff_text(orfs, seqid=seqid)
    open("g.gff", "w").write(head + body)
    return ["-ref", "r.fa", "-gff", "g.gff", "-cov", "10"]


def setup_contigs(recs, rows):
    """r.fa and g.gff of several contigs: recs = [(name, sequence)], rows = [(name, orfs)]"""
    with open("r.fa", "w") as fh:
        for name, ref in recs:
            fh.write(">%s\n%s\n" % (name, ref))
    with open("g.gff", "w") as fh:
        fh.write("##gff-version 3\n")
        for name, orfs in rows:
            fh.write(sy.gff_text(orfs, seqid=name)[1])


def write_override(path, counts):
    """gzipped CSV (position, coverage, A, T, C, G, X, I) over every position"""
    with gzip.open(path, "wt") as fh:
        fh.write("," + ",".join(_ffi.COLS) + "\n")
        for i, row in enumerate(counts, 1):
            fh.write("%d,%s\n" % (i, ",".join(str(int(v)) for v in row)))


def run_two_ranks(args, env_extra=None):
    """`TrueConsense args` as a fresh child process in the environment that rehearses two ranks on this one GPU (gloo for the
    exchange); with --gpus 2 among args the child starts the two ranks.  -> the completed process"""
    env = dict(os.environ, TCMI_SPLIT_ONE_GPU="1", TCMI_SPLIT_BACKEND="gloo", PYTHONPATH=ROOT, **(env_extra or {}))
    r = subprocess.run([sys.executable, "-m", "trueconsense_amd.TrueConsense"] + list(args), env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-1500:]
    return r


def run_split_worker(args, env_extra=None):
    """the worker of `-i --gpus N` (trueconsense_amd.split_main) as the one rank of a world of one, in a fresh child process"""
    env = {k: v for k, v in os.environ.items() if k not in ("TCMI_SPLIT_ONE_GPU", "TCMI_SPLIT_BACKEND")}
    env.update(PYTHONPATH=ROOT, RANK="0", WORLD_SIZE="1", LOCAL_RANK="0", **(env_extra or {}))
    r = subprocess.run([sys.executable, "-m", "trueconsense_amd.split_main"] + list(args), env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-1500:]
    return r
