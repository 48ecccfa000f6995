"""The native writers of --batch without a GPU: csrc/outputs_text.cpp (coverage TSV, corrected GFF, VCF, the file they go to) as a
program of its own under AddressSanitizer + UBSan (tests/outputs_main.cpp, run as a child process; nothing is loaded into Python)
against the golden outputs of the real reference and, where those do not reach, against the Python twin Outputs.vcf_text.  The same
writers behind a GPU run of the file runner: the --batch tests of tests/test_gpu_parity.py."""
import json
import os

import numpy as np
import pytest

from oracle import tc_oracle as orc
from tests import host_program
from tests import synth_small as ss
from trueconsense_amd import Events, Outputs, Sequences, _ffi

OK = 0


def load(name):
    with open(os.path.join(os.path.dirname(__file__), "golden", name + ".json")) as fh:
        return json.load(fh)


def gffdict(orfs):
    """the rows tests/test_host_walk.py::test_writers_match_reference walks"""
    return {k: {"seqid": "S", "source": "x", "type": "CDS", "start": o["start"], "end": o["end"], "score": ".",
                "strand": o["strand"], "phase": "0", "attributes": "ID=o%d;Name=orf%d" % (k, k),
                "Name": "orf%d" % k, "ID": "o%d" % k} for k, o in enumerate(orfs)}


def _esc(s):
    return s.replace("\\", "\\\\").replace("\n", "\\n").replace("\t", "\\t")


def _ints(values):
    return " ".join(str(int(v)) for v in values)


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    return host_program.build(["tests/outputs_main.cpp", "trueconsense_amd/csrc/outputs_text.cpp"], tmp_path_factory.mktemp("outputs") / "outputs_main")


def run_case(prog, mode, cols=(), **fields):
    """-> (code, the refusal's words, text)"""
    lines = ["mode " + mode] + ["%s %s" % (k, _esc(v)) for k, v in fields.items()] + ["col " + _esc(c) for c in cols]
    out = host_program.run(prog, input="\n".join(lines) + "\n").stdout
    code, why, text = out.split("\n", 2)
    assert code.startswith("code ") and why.startswith("why "), out[:200]
    return int(code[5:]), why[4:], text


def vcf_fields(ref, cons, cov, mincov, ins, head):
    """the program's input for Outputs.vcf_text(.., list(ref), cons, {pos: coverage}, mincov, ins is not None, ins)"""
    pos = sorted(ins or {})
    bases = [str(b) for p in pos for b in (ins[p].values())]
    assert len(bases) == len(pos)                                   # one accepted token per position (Events.inserts_from_flags)
    off = np.concatenate([[0], np.cumsum([len(b) for b in bases])]).astype(np.int64)
    return dict(head=head, refid="refid", ref=ref, cons=cons, ints=_ints(cov), mincov=str(mincov), inspos=_ints(pos), insoff=_ints(off),
                insseq="".join(bases))


HEAD = Outputs.vcf_header("DATE", ["ARGS"], "ref.fa", "refid")


def test_writers_match_the_golden_outputs(prog):
    """every run of tests/golden/outputs.json, from the inputs tests/test_host_walk.py::test_writers_match_reference builds: the three
    native writers give the reference's VCF, GFF and coverage TSV byte for byte"""
    n_runs = n_indel = 0
    for case in load("outputs"):
        spec = case["spec"]
        reads = ss.reads_from_spec(spec)
        counts = np.array(case["counts"], np.int64)
        for key, run in case["runs"].items():
            assert "raises" not in run, (case["name"], key)
            plain, alt, flags = orc.call_records(counts, spec["mincov"], key == "amb1")
            has, ins = Events.inserts_from_flags(flags, reads)
            _, gff = Sequences.consensus_from_records(plain, alt, flags, gffdict(spec["orfs"]), ins, True)
            c0, _ = Sequences.consensus_from_records(plain, alt, flags, gffdict(spec["orfs"]), ins, False)
            got = run_case(prog, "vcf", **vcf_fields(spec["ref"], c0, counts[:, 0], spec["mincov"], ins if has else None, HEAD))
            assert got == (OK, "", run["vcf"]), (case["name"], key)
            rows = [gff[k] for k in gff]                            # (the native writer's seqid is the sample's name: these rows' "S")
            got = run_case(prog, "gff", cols=[c for row in rows for c in Outputs.gff_row_columns(row)], head="##gff-version 3\n", name="S",
                           ns=_ints(r["start"] for r in rows), ne=_ints(r["end"] for r in rows))
            assert got == (OK, "", run["gff"]), (case["name"], key)
            assert run_case(prog, "tsv", ints=_ints(counts[:, 0])) == (OK, "", run["tsv"]), (case["name"], key)
            n_runs += 1
            n_indel += "INDEL\n" in run["vcf"]
    assert n_runs == 28 and n_indel == 12                           # 14 cases x 2 runs: none left out; 12 of the VCFs hold indel rows


# What the goldens do not reach: (name, ref, insert-free consensus, coverage column, mincov, inserts, Python raises)
HAND = [
    ("deletion to the end of the consensus", "ACGTAC", "ACGT--", [10] * 6, 3, None, True),
    ("consensus shorter than the reference", "ACGTAC", "ACGT", [10] * 6, 3, None, True),
    ("coverage past L: indel row", "ACGTAC", "ACG-AC", [10] * 3, 3, None, True),
    ("coverage past L: substitution at index 0", "ACGT", "TCGT", [5], 3, None, True),
    ("substitution at index 0 reads position 2", "ACGT", "TCGT", [5, 7], 3, None, False),
    ("coverage past L: substitution at the last index", "ACGT", "ACGA", [5] * 3, 3, None, True),
    ("coverage past L: insert", "ACGT", "ACGT", [5, 5], 3, {2: {"1": "G"}}, True),
    ("deletion at index 0", "ACGTAC", "--GTAT", [11, 12, 13, 14, 15, 16, 17], 3, None, False),
    ("deletion run cut at the reference's end", "ACGT", "AC---G", [9] * 6, 3, None, False),
    ("insert with dp == mincov", "ACGTAC", "ACGTAC", [10, 10, 10, 30, 10, 10], 30, {3: {"2": "GG"}}, False),
    ("insert with dp == mincov + 1", "ACGTAC", "ACGTAC", [10, 10, 10, 30, 10, 10], 29, {3: {"2": "GG"}}, False),
    ("lower-case consensus", "ACGTac", "acgtAC", [20] * 6, 3, None, False),
    ("inserts at adjacent positions", "ACGTAC", "ACGTAC", [50] * 6, 10, {2: {"1": "G"}, 3: {"2": "TT"}}, False),
    ("insert under a deletion run", "ACGTAC", "AC---C", [50] * 6, 10, {3: {"1": "A"}, 5: {"3": "CCC"}}, False),
    ("insert at a deletion's first index", "ACGTACGTACGT", "AC--ACGTACGT", [50] * 12, 10, {2: {"1": "G"}}, False),
]


@pytest.mark.parametrize("name,ref,cons,cov,mincov,ins,raises", HAND, ids=[h[0] for h in HAND])
def test_vcf_agrees_with_the_python_twin(prog, name, ref, cons, cov, mincov, ins, raises):
    """TCMI_OK with Outputs.vcf_text's text where Python returns, TCMI_E_KEYERROR where it raises KeyError or IndexError"""
    idict = {i + 1: {"coverage": c} for i, c in enumerate(cov)}
    code, why, text = run_case(prog, "vcf", **vcf_fields(ref, cons, cov, mincov, ins, HEAD))
    if raises:
        with pytest.raises((KeyError, IndexError)):
            Outputs.vcf_text("DATE", ["ARGS"], "ref.fa", "refid", list(ref), cons, idict, mincov, ins is not None, ins)
        assert code == _ffi.E_KEYERROR and why.startswith("VCF: ") and "upstream" in why and text == ""
        return
    want = Outputs.vcf_text("DATE", ["ARGS"], "ref.fa", "refid", list(ref), cons, idict, mincov, ins is not None, ins)
    assert (code, why, text) == (OK, "", want)
    assert len(want) > len(HEAD) or name == "insert with dp == mincov"         # a row was written, but for the insert at the bound


def test_hand_cases_hit_what_they_name(prog):
    """the rows of a few hand-made cases spelled out, so that a twin that drifted along with the writer is seen"""
    rows = {h[0]: run_case(prog, "vcf", **vcf_fields(*h[1:6], ""))[2] for h in HAND if not h[6]}
    assert rows["deletion at index 0"] == "refid\t0\t.\tCAC\tT\t.\tPASS\tDP=11;INDEL\nrefid\t6\t.\tC\tT\t.\tPASS\tDP=16\n"
    assert rows["substitution at index 0 reads position 2"] == "refid\t1\t.\tA\tT\t.\tPASS\tDP=7\n"
    assert rows["deletion run cut at the reference's end"] == "refid\t2\t.\tCGT\tC\t.\tPASS\tDP=9;INDEL\n"
    assert rows["insert with dp == mincov"] == ""
    assert rows["insert with dp == mincov + 1"] == "refid\t3\t.\tT\tTGG\t.\tPASS\tDP=30;INDEL\n"
    assert rows["lower-case consensus"] == "refid\t5\t.\ta\tA\t.\tPASS\tDP=20\nrefid\t6\t.\tc\tC\t.\tPASS\tDP=20\n"
    assert rows["inserts at adjacent positions"] == "refid\t2\t.\tG\tGG\t.\tPASS\tDP=50;INDEL\nrefid\t3\t.\tT\tTTT\t.\tPASS\tDP=50;INDEL\n"
    assert rows["insert under a deletion run"] == "refid\t2\t.\tCGTA\tC\t.\tPASS\tDP=50;INDEL\nrefid\t5\t.\tC\tCCCC\t.\tPASS\tDP=50;INDEL\n"
    assert rows["insert at a deletion's first index"] == "refid\t2\t.\tCGT\tC\t.\tPASS\tDP=50;INDEL\nrefid\t2\t.\tG\t-G\t.\tPASS\tDP=50;INDEL\n"


def test_put_int_and_the_coverage_column(prog):
    big = [0, -1, -(1 << 63), (1 << 63) - 1]
    assert run_case(prog, "int", ints=_ints(big)) == (OK, "", "".join("%d\n" % v for v in big))
    assert run_case(prog, "tsv", ints="") == (OK, "", "")                              # L = 0
    for c in (0, -1, 7, (1 << 31) - 1, -(1 << 31)):                                         # L = 1
        assert run_case(prog, "tsv", ints=str(c)) == (OK, "", "1\t%d\n" % c)


def test_write_file(prog, tmp_path):
    good = tmp_path / "o.txt"
    assert run_case(prog, "write", path=str(good), text="a\tb\n\\c\n") == (OK, "", "")
    assert good.read_bytes() == b"a\tb\n\\c\n"
    bad = tmp_path / "no_such_directory" / "o.txt"
    assert run_case(prog, "write", path=str(bad), text="x") == (_ffi.E_IO, "cannot write %s" % bad, "")
    assert not os.path.exists(bad) and not os.path.exists(bad.parent)
