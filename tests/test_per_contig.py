"""--per-contig: BAMs aligned to a multi-record reference (a segmented virus, several targets).

Every contig's results must be what the single-contig path gives on that contig's share of the inputs: its reads with tid 0
and one @SQ, its FASTA record, its GFF rows.  The CPU tests cover the readers, the FASTA helper and the command line's refusals;
the GPU tests compare the contig layout's count matrix, extents, insert tokens and the four output files with those split runs."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.cli_run import ROOT, run_cli
from trueconsense_amd import _ffi, contigs, engine
from trueconsense_amd import synthetic as sy
from trueconsense_amd.io import bamwriter, fasta


def concat(parts):
    """[(tid, reads dict), ...] -> one reads dict in that order, with a tid array (and the mate / name fields where given)."""
    out = {"pos": [], "flag": [], "l_qseq": [], "tid": [], "cigar": [], "seq": [], "qual": [], "next_tid": [], "next_pos": [], "tlen": []}
    co, so = [0], [0]
    for tid, r in parts:
        n = int(r["n_reads"])
        if n == 0:
            continue
        out["pos"].append(np.asarray(r["pos"], np.int32))
        out["flag"].append(np.asarray(r["flag"], np.uint16))
        out["l_qseq"].append(np.asarray(r["l_qseq"], np.int32))
        out["tid"].append(np.full(n, tid, np.int32) if np.isscalar(tid) else np.asarray(tid, np.int32))
        c0, s0 = co[-1], so[-1]
        rc, rs = np.asarray(r["cigar_off"], np.uint64), np.asarray(r["seq_off"], np.uint64)
        out["cigar"].append(np.asarray(r["cigar"], np.uint32)[int(rc[0]):int(rc[n])])
        out["seq"].append(np.asarray(r["seq"], np.uint8)[int(rs[0]):int(rs[n])])
        co.extend((rc[1:n + 1] - rc[0] + c0).tolist())
        so.extend((rs[1:n + 1] - rs[0] + s0).tolist())
        lq = np.asarray(r["l_qseq"], np.int64)
        out["qual"].append(np.asarray(r["qual"], np.uint8)[:int(lq.sum())] if r.get("qual") is not None else np.full(int(lq.sum()), 30, np.uint8))
        for k, dflt in (("next_tid", -1), ("next_pos", -1), ("tlen", 0)):
            out[k].append(np.asarray(r[k], np.int32) if r.get(k) is not None else np.full(n, dflt, np.int32))
    res = {k: (np.concatenate(v) if v else np.zeros(0, np.uint8 if k in ("seq", "qual") else np.int32)) for k, v in out.items()}
    res["flag"] = res["flag"].astype(np.uint16)
    res["cigar"] = res["cigar"].astype(np.uint32)
    res["n_reads"] = len(res["pos"])
    res["cigar_off"] = np.asarray(co, np.uint64)
    res["seq_off"] = np.asarray(so, np.uint64)
    return res


def subset(reads, keep):
    """The reads of a boolean mask, offsets rebuilt."""
    return concat([(int(reads["tid"][i]), subset_one(reads, int(i))) for i in np.nonzero(keep)[0]])


# the fixture: header refs A, X (not in the FASTA), B (no reads), C (reads longer than 512 positions + an insert candidate)
def fixture(tmp_path, long_reads=True):
    ra, oa = sy.make_reference(seed=11, L=2341, cds=[(101, 1300)])
    rc, oc = sy.make_reference(seed=13, L=1778, cds=[(201, 1500)])
    rx, _ = sy.make_reference(seed=17, L=900, cds=[])
    rb, _ = sy.make_reference(seed=19, L=1027, cds=[])
    a = sy.make_reads(ra, 900, seed=3, indel_sites=sy.default_indel_sites(oa, seed=5))
    a["pos"][-1] = len(ra) - 60                                 # overhangs A's end by 90 positions (within the guard)
    x = sy.make_reads(rx, 200, seed=4)
    c = sy.make_reads(rc, 700, seed=6, indel_sites=[(900, "I", "GAT", 0.9), (400, "D", 3, 0.5)])
    parts = [(0, a), (1, x), (3, c)]
    if long_reads:
        parts.append((3, sy.make_reads(rc, 40, read_len=700, seed=8)))
    reads = sort_reads(concat(parts))
    refs = [("A", len(ra)), ("X", len(rx)), ("B", len(rb)), ("C", len(rc))]
    records = [("A", ra), ("B", rb), ("C", rc)]                # the FASTA: X is not in it
    gff_rows = {"A": oa, "B": [], "C": oc}
    bam = str(tmp_path / "multi.bam")
    bamwriter.write_bam(bam, reads, refs=refs)
    return reads, refs, records, gff_rows, bam


def sort_reads(reads):
    """Reads in (tid, pos) order (a coordinate-sorted BAM)."""
    order = np.lexsort((reads["pos"], reads["tid"]))
    parts = []
    for i in order.tolist():
        parts.append((int(reads["tid"][i]), subset_one(reads, i)))
    return concat(parts)


def subset_one(reads, i):
    one = {"n_reads": 1, "pos": reads["pos"][i:i + 1], "flag": reads["flag"][i:i + 1], "l_qseq": reads["l_qseq"][i:i + 1],
           "cigar_off": np.array([0, reads["cigar_off"][i + 1] - reads["cigar_off"][i]], np.uint64),
           "cigar": reads["cigar"][int(reads["cigar_off"][i]):int(reads["cigar_off"][i + 1])],
           "seq_off": np.array([0, reads["seq_off"][i + 1] - reads["seq_off"][i]], np.uint64),
           "seq": reads["seq"][int(reads["seq_off"][i]):int(reads["seq_off"][i + 1])]}
    q0 = int(np.sum(reads["l_qseq"][:i]))
    one["qual"] = reads["qual"][q0:q0 + int(reads["l_qseq"][i])]
    for k in ("next_tid", "next_pos", "tlen"):
        one[k] = reads[k][i:i + 1]
    return one


def split_reads(reads, tid):
    """Contig `tid`'s reads with tid 0 (the split BAM's records)."""
    r = subset(reads, reads["tid"] == tid)
    r["tid"] = np.zeros(r["n_reads"], np.int32)
    return r


def write_fasta(path, records):
    with open(path, "w") as fh:
        for rid, seq in records:
            fh.write(">%s segment\n" % rid)
            for o in range(0, len(seq), 60):
                fh.write(seq[o:o + 60] + "\n")


def write_gff(path, rows_by_contig, contigs_):
    with open(path, "w") as fh:
        fh.write("##gff-version 3\n")
        for c in contigs_:
            for k, o in enumerate(rows_by_contig[c]):
                fh.write("%s\tsynthetic\tCDS\t%d\t%d\t.\t%s\t0\tID=%s_cds%d;Name=orf%d\n" % (c, o["start"], o["end"], o["strand"], c, k, k))


# ------------------------------------------------------------------ CPU
def test_read_records(tmp_path):
    p = str(tmp_path / "r.fa")
    with open(p, "w") as fh:
        fh.write(">one first segment\nACGT\nAC\n>two\n\nGG\n>three x\n")
    assert fasta.read_records(p) == [("one", "ACGTAC"), ("two", "GG"), ("three", "")]
    assert fasta.read_first_record(p) == ("one", "ACGTAC")


def test_host_reader_header_of_three_contigs(tmp_path):
    r = sy.make_reads(sy.make_reference(seed=1, L=800, cds=[])[0], 30, seed=2)
    p = str(tmp_path / "three.bam")
    bamwriter.write_bam(p, concat([(0, r)]), refs=[("chrA", 800), ("chrB", 1200), ("segment_3", 55)])
    b = engine.BamFile(p)
    assert b.references == ("chrA",) and b.lengths == (800,)
    assert b.all_references == ("chrA", "chrB", "segment_3") and b.all_lengths == (800, 1200, 55)
    assert contigs.bam_header_refs(p) == (["chrA", "chrB", "segment_3"], [800, 1200, 55])
    b.close()


def test_layout_slots():
    shift, slot, n = contigs.layout_for([("C", "A" * 10), ("A", "A" * 5000)], ["A", "X", "C"], [4000, 7, 12])
    assert shift.tolist() == [0, -1, 9216] and slot.tolist() == [9216, 0, 4352] and n == 9216 + 4352
    assert all(s % 256 == 0 for s in slot)
    with pytest.raises(contigs.ContigError, match='"Q"'):
        contigs.layout_for([("Q", "ACGT")], ["A"], [4])


def _cli(args, cwd):
    env = dict(os.environ, PYTHONPATH=ROOT, HIP_VISIBLE_DEVICES="-1")      # (no GPU may be touched by a refusal)
    return subprocess.run([sys.executable, "-m", "trueconsense_amd.TrueConsense"] + args, cwd=cwd, env=env,
                          capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize("extra", [["--batch", "m.tsv"], ["--gpus", "2"], ["--index-override", "o.csv.gz"]])
def test_cli_refusals(tmp_path, extra):
    r = sy.make_reads(sy.make_reference(seed=1, L=800, cds=[])[0], 30, seed=2)
    bamwriter.write_bam(str(tmp_path / "in.bam"), concat([(0, r)]), refs=[("A", 800), ("B", 300)])
    write_fasta(str(tmp_path / "r.fa"), [("A", "A" * 800), ("B", "C" * 300)])
    (tmp_path / "f.gff").write_text("##gff-version 3\n")
    (tmp_path / "m.tsv").write_text("in.bam\tS\tS.fa\n")
    (tmp_path / "o.csv.gz").write_bytes(b"")
    p = _cli(["-i", "in.bam", "-ref", "r.fa", "-gff", "f.gff", "-cov", "5", "-name", "S", "-o", "S.fa", "--per-contig"] + extra, tmp_path)
    assert p.returncode == 1, p.stdout + p.stderr
    assert "--per-contig does not go with" in p.stdout
    assert not (tmp_path / "S.fa").exists()


def test_cli_refuses_a_fasta_record_missing_from_the_header(tmp_path):
    r = sy.make_reads(sy.make_reference(seed=1, L=800, cds=[])[0], 30, seed=2)
    bamwriter.write_bam(str(tmp_path / "in.bam"), concat([(0, r)]), refs=[("A", 800), ("B", 300)])
    write_fasta(str(tmp_path / "r.fa"), [("A", "A" * 800), ("segment_7", "C" * 300)])
    (tmp_path / "f.gff").write_text("##gff-version 3\n")
    p = _cli(["-i", "in.bam", "-ref", "r.fa", "-gff", "f.gff", "-cov", "5", "-name", "S", "-o", "S.fa", "--per-contig"], tmp_path)
    assert p.returncode == 1 and '"segment_7"' in p.stdout, p.stdout + p.stderr
    assert not (tmp_path / "S.fa").exists()


# ------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def ctx():
    with engine.Context(0) as c:
        yield c


def _layout(refs, records):
    return contigs.layout_for(records, [n for n, _ in refs], [ln for _, ln in refs])


@pytest.mark.gpu
@pytest.mark.parametrize("how", ["device", "host", "cigar_walk"])
def test_counts_per_contig(ctx, tmp_path, how):
    from oracle import c_oracle
    reads, refs, records, _, bam = fixture(tmp_path)
    shift, slot, n = _layout(refs, records)
    if how == "device":
        d = engine.DeviceBam(bam)
        assert d.all_references == ("A", "X", "B", "C") and d.references == ("A",)
        ctx.set_layout(shift, slot)
        try:
            rs = ctx.upload_bamfile(d)
        finally:
            ctx.set_layout()
        d.close()
        assert rs.packed_on_device
    else:
        ctx.set_option("tally_variant", 1 if how == "cigar_walk" else 0)
        host = engine.BamFile(bam)
        ctx.set_layout(shift, slot)
        try:
            rs = ctx.upload(host)
        finally:
            ctx.set_layout()
            ctx.set_option("tally_variant", 0)
    ext = rs.ref_extents(len(refs))
    counts = ctx.step(rs, n, 0, True)[3]
    assert rs.dropped() == int(np.sum((reads["tid"] == 1) & ((reads["flag"] & 4) == 0) & (reads["pos"] >= 0))) == 200
    rs.free()
    assert ext[1] == 0 and ext[2] == 0                          # X is dropped, B has no reads
    assert counts[int(shift[2]):int(shift[2]) + int(slot[2])].sum() == 0
    for t, (name, _) in enumerate(refs):
        if shift[t] < 0:
            continue
        mine = split_reads(reads, t)
        want_L = engine.reads_extent(mine, 0) if mine["n_reads"] else 0
        assert ext[t] == want_L, name
        L = max(want_L, len(dict(records)[name]), 1)
        want = c_oracle.tally(mine, L) if mine["n_reads"] else np.zeros((L, 7), np.int32)
        got = counts[int(shift[t]):int(shift[t]) + int(slot[t])]
        assert np.array_equal(got[:L], want), name
        assert not got[L:].any(), name


@pytest.mark.gpu
def test_unsorted_file_counts(ctx, tmp_path):
    from oracle import c_oracle
    reads, refs, records, _, _ = fixture(tmp_path, long_reads=False)
    rev = subset(reads, np.ones(reads["n_reads"], bool))
    order = np.argsort(-rev["pos"], kind="stable")                  # positions descend: not sorted
    rev = concat([(int(rev["tid"][i]), subset_one(rev, i)) for i in order.tolist()])
    shift, slot, n = _layout(refs, records)
    ctx.set_layout(shift, slot)
    try:
        rs = ctx.upload(rev)
    finally:
        ctx.set_layout()
    counts = ctx.step(rs, n, 0, True)[3]
    rs.free()
    for t in (0, 3):
        mine = split_reads(reads, t)
        L = max(engine.reads_extent(mine, 0), len(dict(records)[refs[t][0]]))
        assert np.array_equal(counts[int(shift[t]):int(shift[t]) + L], c_oracle.tally(mine, L))


@pytest.mark.gpu
def test_insert_tokens_with_a_layout(ctx, tmp_path):
    reads, refs, records, _, bam = fixture(tmp_path, long_reads=False)
    # a mate pair split over A and C: not an overlapping pair
    ia, ic = int(np.nonzero(reads["tid"] == 0)[0][0]), int(np.nonzero(reads["tid"] == 3)[0][0])
    for i, j in ((ia, ic), (ic, ia)):
        reads["flag"][i] = 1 | 2 | (64 if i == ia else 128)
        reads["next_tid"][i], reads["next_pos"][i] = reads["tid"][j], reads["pos"][j]
    bamwriter.write_bam(bam, reads, refs=refs)
    shift, slot, n = _layout(refs, records)
    host = engine.BamFile(bam)
    ctx.set_layout(shift, slot)
    try:
        d = engine.DeviceBam(bam)
        rs = ctx.upload_bamfile(d)
        counts = ctx.step(rs, n, 0, True)[3]
        with pytest.raises(_ffi.TcmiError):                         # (the device sweep declines a layout: the host sweep takes it)
            ctx.readset_modal_tokens(rs, [int(shift[3]) + 900])
        rs.free()
        d.close()
    finally:
        ctx.set_layout()
    for t in (0, 3):
        cand = [p + 1 for p in range(int(slot[t])) if counts[int(shift[t]) + p, 6] * 100 > 55 * max(counts[int(shift[t]) + p, 0], 1)]
        cand = sorted(set(cand) | {901, 401, 1})
        got = engine.modal_tokens(host, [int(shift[t]) + p for p in cand], layout=(shift, slot))
        mine = split_reads(reads, t)
        mine["next_tid"] = np.where(reads["next_tid"][reads["tid"] == t] == t, 0, np.where(reads["next_tid"][reads["tid"] == t] < 0, -1, 1)).astype(np.int32)
        mine["name_off"] = None
        want = engine.modal_tokens({k: v for k, v in mine.items() if v is not None}, cand)
        assert {p - int(shift[t]): v for p, v in got.items()} == want
    host.close()


@pytest.mark.gpu
def test_cli_per_contig_equals_split_runs(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    reads, refs, records, gff_rows, bam = fixture(tmp_path)
    write_fasta("flu.fa", records)
    write_gff("flu.gff", gff_rows, ["A", "B", "C"])
    run_cli(monkeypatch, ["-i", bam, "-ref", "flu.fa", "-gff", "flu.gff", "-cov", "10", "-name", "S", "-o", "S.fa", "-vcf", "S.vcf",
                          "-ogff", "S.gff", "-doc", "S.tsv", "--per-contig", "--stats", "S.json"])
    import json
    stats = json.load(open("S.json"))
    assert stats["contigs"] == 3 and stats["dropped_reads"] == 200      # (the reads on X, which the FASTA does not name)
    want_fa, want_vcf, want_gff, want_tsv, contig_lines = "", "", "##gff-version 3\n", "", ""
    for t, (name, _) in enumerate(refs):
        if name == "X":
            continue
        seq = dict(records)[name]
        sub = split_reads(reads, t)
        bamwriter.write_bam("%s.bam" % name, sub, refs=[(name, dict(refs)[name])])
        write_fasta("%s.fa" % name, [(name, seq)])
        write_gff("%s.gff" % name, gff_rows, [name])
        run_cli(monkeypatch, ["-i", "%s.bam" % name, "-ref", "%s.fa" % name, "-gff", "%s.gff" % name, "-cov", "10", "-name", "S_%s" % name,
                              "-o", "o_%s.fa" % name, "-vcf", "o_%s.vcf" % name, "-ogff", "o_%s.gff" % name, "-doc", "o_%s.tsv" % name])
        want_fa += open("o_%s.fa" % name).read()
        want_vcf += "".join(ln for ln in open("o_%s.vcf" % name) if not ln.startswith("#"))
        want_gff += open("o_%s.gff" % name).read()[len("##gff-version 3\n"):]
        want_tsv += "".join("%s\t%s" % (name, ln) for ln in open("o_%s.tsv" % name))
        contig_lines += "##contig=<ID=%s>\n" % name
    got_vcf = open("S.vcf").read()
    assert open("S.fa").read() == want_fa and want_fa.count(">") == 3
    assert "".join(ln for ln in got_vcf.splitlines(True) if not ln.startswith("#")) == want_vcf
    assert contig_lines in got_vcf and got_vcf.count("##contig=") == 3
    assert open("S.gff").read() == want_gff
    assert open("S.tsv").read() == want_tsv
    assert "GAT" in open("o_C.vcf").read() or "GAT" in open("o_C.fa").read()     # (the insert candidate on the last contig was taken)


@pytest.mark.gpu
def test_read_past_its_slot_is_refused(ctx, tmp_path, monkeypatch, capsys):
    monkeypatch.chdir(tmp_path)
    ra, _ = sy.make_reference(seed=11, L=600, cds=[])
    r = sy.make_reads(ra, 50, seed=3)
    r["pos"][-1] = 600 + contigs.GUARD + 200                    # ends past A's slot (4 864 positions)
    reads = concat([(0, r), (1, sy.make_reads(ra, 20, seed=4))])
    refs = [("A", 600), ("B", 600)]
    bamwriter.write_bam("in.bam", reads, refs=refs)
    write_fasta("r.fa", [("A", ra), ("B", ra)])
    shift, slot, n = _layout(refs, [("A", ra), ("B", ra)])
    ctx.set_layout(shift, slot)
    try:
        for up in (lambda: ctx.upload_bamfile(engine.DeviceBam("in.bam")), lambda: ctx.upload(engine.BamFile("in.bam"))):
            with pytest.raises(_ffi.TcmiError) as e:
                up()
            assert e.value.code == _ffi.E_UNSUPPORTED
            assert "read 49 on reference 0 ends past the end of its contig's slot" in str(e.value)
    finally:
        ctx.set_layout()
    (tmp_path / "f.gff").write_text("##gff-version 3\n")
    with pytest.raises(SystemExit) as e:
        run_cli(monkeypatch, ["-i", "in.bam", "-ref", "r.fa", "-gff", "f.gff", "-cov", "5", "-name", "S", "-o", "S.fa", "-vcf", "S.vcf",
                              "--per-contig"])
    assert e.value.code == 1
    assert 'read "r49" on contig "A" ends past the end' in capsys.readouterr().err
    assert not (tmp_path / "S.fa").exists() and not (tmp_path / "S.vcf").exists()


@pytest.mark.gpu
def test_layout_table_is_reused_and_guarded(ctx, tmp_path):
    reads, refs, records, _, bam = fixture(tmp_path)               # (reads longer than 512 positions on C: tallied with the table)
    shift, slot, n = _layout(refs, records)
    d = engine.DeviceBam(bam)
    ctx.set_layout(shift, slot)
    rs = ctx.upload_bamfile(d)
    ctx.set_layout()                                                # clearing keeps the table: the step still finds it
    want = ctx.step(rs, n, 0, True)[3]
    ctx.set_layout(shift[::-1].copy() * 0 - 1, slot)                # another layout rewrites the one table ...
    with pytest.raises(_ffi.TcmiError) as e:                        # ... so the read set uploaded under the first one is refused
        ctx.step(rs, n, 0, True)
    assert e.value.code == _ffi.E_UNSUPPORTED
    rs.free()
    for _ in range(3):                                              # the same layout again and again: one table, same counts
        ctx.set_layout(shift, slot)
        rs = ctx.upload_bamfile(d)
        assert np.array_equal(ctx.step(rs, n, 0, True)[3], want)
        rs.free()
    ctx.set_layout()
    d.close()


@pytest.mark.gpu
def test_default_path_unchanged(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    reads, refs, records, gff_rows, bam = fixture(tmp_path, long_reads=False)
    write_fasta("flu.fa", records)
    write_gff("flu.gff", gff_rows, ["A", "B", "C"])
    with pytest.raises(_ffi.TcmiError) as e:                        # without the flag a multi-contig file is refused, as before
        run_cli(monkeypatch, ["-i", bam, "-ref", "flu.fa", "-gff", "flu.gff", "-cov", "10", "-name", "S", "-o", "S.fa"])
    assert e.value.code == _ffi.E_UNSUPPORTED
    # a single-contig file: --per-contig gives today's outputs under -name S_A, plus the contig column of the TSV
    sub = split_reads(reads, 0)
    bamwriter.write_bam("A.bam", sub, refs=[("A", refs[0][1])])
    write_fasta("A.fa", [records[0]])
    write_gff("A.gff", gff_rows, ["A"])
    common = ["-i", "A.bam", "-ref", "A.fa", "-gff", "A.gff", "-cov", "10"]
    run_cli(monkeypatch, common + ["-name", "S_A", "-o", "d.fa", "-vcf", "d.vcf", "-ogff", "d.gff", "-doc", "d.tsv"])
    run_cli(monkeypatch, common + ["-name", "S", "-o", "p.fa", "-vcf", "p.vcf", "-ogff", "p.gff", "-doc", "p.tsv", "--per-contig"])
    assert open("p.fa").read() == open("d.fa").read()
    assert open("p.gff").read() == open("d.gff").read()
    assert open("p.vcf").read() == open("d.vcf").read()          # (sys.argv is the same placeholder in both runs)
    assert open("p.tsv").read() == "".join("A\t" + ln for ln in open("d.tsv"))
