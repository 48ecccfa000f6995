"""cli_tables.TablePart / write_tables / part_of_columns without a GPU: the one way from the counts behind the step to the files of
--variant-table, --variant-links, --indel-table and --variant-evidence.  Everything expected is engine.*_text and the *_HEADER
constants called directly on tests/table_rows.py's hand-written rows, never through write_tables."""
import os

import numpy as np
import pytest

from tests import cli_run as cr
from tests import table_rows as tr
from trueconsense_amd import _ffi, cli_args, engine
from trueconsense_amd import cli_tables as ct

FILES = ("t.tsv", "l.tsv", "i.tsv", "e.tsv")
KEYS = ("variant_records", "variant_strand_bias", "variant_strand_low", "variant_link_rows", "variant_links_cis", "variant_links_trans",
        "variant_links_mixed", "variant_links_none", "variant_links_low", "variant_evidence_lowq", "variant_evidence_lowmq", "variant_evidence_end")


def asked(tmp_path, flags=("strand", "links", "indels", "evidence")):
    """-> (the namespace with the tables' files in tmp_path, its StreamCounts, {file name: path})"""
    f = {n: str(tmp_path / n) for n in FILES}
    more = {"strand": ["--variant-strand"], "links": ["--variant-links", f["l.tsv"], "--link-neighbours", "2"], "indels": ["--indel-table", f["i.tsv"]],
            "evidence": ["--variant-evidence", f["e.tsv"]]}
    a = cli_args.GetArgs(cr.base_args(cr.stub_files(tmp_path)) + ["--variant-table", f["t.tsv"]] + [x for w in flags for x in more[w]])
    return a, ct.StreamCounts(a), f


def part(cols=tr.COLS, region="ctg", pos_offset=0):
    return ct.TablePart(tr.records(cols), region, tr.REF, pos_offset, tr.strand(cols), tr.links(2, cols), tr.indels(tr.indel_rows(cols)), tr.evidence(cols))


def texts(want, parts):
    """the four files' rows from the text functions themselves, part after part"""
    _, k, lrule = want.links
    return {"t.tsv": "".join(engine.variants_strand_text(p.records, p.strand, p.region, p.ref, p.pos_offset, **want.srule) for p in parts),
            "l.tsv": "".join(engine.variants_links_text(p.records, p.links, k, p.region, p.ref, p.pos_offset, **lrule) for p in parts),
            "i.tsv": "".join(engine.indels_text(*p.indels, p.records, p.region, p.ref, p.pos_offset) for p in parts),
            "e.tsv": "".join(engine.variants_evidence_text(p.records, p.evidence, p.region, p.ref, p.pos_offset, **want.evidence[1]) for p in parts)}


HEADERS = {"t.tsv": engine.VARIANTS_STRAND_HEADER, "l.tsv": engine.VARIANTS_LINKS_HEADER, "i.tsv": engine.INDELS_HEADER, "e.tsv": engine.VARIANTS_EVIDENCE_HEADER}


def stats_of(rows, n_records):
    return dict(variant_records=n_records, variant_strand_bias=rows["t.tsv"].count("\tBIAS\n"), variant_strand_low=rows["t.tsv"].count("\tLOW\n"),
                **ct.link_stats(rows["l.tsv"]), **ct.evidence_stats(rows["e.tsv"]))


def test_one_part(tmp_path):
    a, want, f = asked(tmp_path)
    p = part()
    assert {"*", "+"} <= {ln.split("\t")[3] for ln in engine.variants_text(p.records, "ctg", tr.REF).splitlines()}
    rows = texts(want, [p])
    assert all(rows.values()) and rows["i.tsv"].endswith("ctg\t11\tDEL\t4\tTANN\t3\t12\t0.250000\n")        # (N beyond the reference)
    got = ct.write_tables(a, [p], want)
    for name in FILES:
        assert open(f[name]).read() == HEADERS[name] + rows[name], name
    assert got == stats_of(rows, 6) and list(got) == list(KEYS)
    assert got["variant_strand_bias"] == 2 and got["variant_strand_low"] == 1 and got["variant_link_rows"] == 8 and got["variant_evidence_end"] >= 2
    # without --variant-strand: the plain table, the strand keys 0; the files not asked for are not written
    (tmp_path / "plain").mkdir()
    a, want, f = asked(tmp_path / "plain", ("links",))
    got = ct.write_tables(a, [p], want)
    assert open(f["t.tsv"]).read() == engine.VARIANTS_HEADER + engine.variants_text(p.records, "ctg", tr.REF)
    assert open(f["l.tsv"]).read() == HEADERS["l.tsv"] + rows["l.tsv"] and not os.path.exists(f["i.tsv"]) and not os.path.exists(f["e.tsv"])
    assert got == dict(stats_of(rows, 6), variant_strand_bias=0, variant_strand_low=0, **ct.evidence_stats()) and list(got) == list(KEYS)


def test_two_parts(tmp_path):
    a, want, f = asked(tmp_path)
    parts = [part((0, 2)), part((7, 10), "seg 2", 6)]
    rows = texts(want, parts)
    got = ct.write_tables(a, parts, want)
    for name in FILES:
        assert open(f[name]).read() == HEADERS[name] + rows[name], name
    assert got == stats_of(rows, 6)
    assert rows["t.tsv"].startswith("ctg\t1\tA\tT\t") and "seg 2\t2\tG\tA\t" in rows["t.tsv"] and rows["i.tsv"].endswith("seg 2\t5\tDEL\t4\tTANN\t3\t12\t0.250000\n")
    # a link row stays inside its part: the one part's table pairs columns 2 and 7, the two parts' never
    pairs = [(ln.split("\t")[0], int(ln.split("\t")[1]), int(ln.split("\t")[4])) for ln in rows["l.tsv"].splitlines()]
    assert sorted(set(pairs)) == [("ctg", 1, 3), ("seg 2", 2, 5)]
    assert "ctg\t3\tC\tG\t8\tG\tA\t" in texts(want, [part()])["l.tsv"]


def only(dtype, key, at):
    out = np.zeros(len(at), dtype)
    out[key] = at
    return out


def test_part_of_columns_cuts_every_array_by_its_own_key():
    """two slots of 256 columns, sequences of 100 and 120: rows in the first slot's guard columns and in the second slot"""
    table = only(engine.VARIANT_DTYPE, "pos", [5, 99, 100, 255, 256, 375, 376])
    got = {"variant_strand": only(engine.STRAND_DTYPE, "pos", [0, 100, 300]), "variant_links": only(engine.LINK_DTYPE, "a", [7, 7, 99, 99, 180, 180, 256, 256]),
           "variant_evidence": only(engine.EVIDENCE_DTYPE, "pos", [99, 101, 255, 370, 400]),
           "indel_events": (only(engine.INDEL_EVENT_DTYPE, "pos", [50, 50, 150, 256]), b"ACGT", only(engine.INDEL_TOTALS_DTYPE, "pos", [50, 150, 256, 511]))}
    got["variant_links"]["b"] = [99, 180, 180, 256, 256, 300, 300, -1]              # (the second column plays no part)
    ref = np.zeros(512, np.uint8)
    one = ct.part_of_columns(table, got, 0, 100, "c1", ref[:100], 0)
    two = ct.part_of_columns(table, got, 256, 376, "c2", ref[:376], 256)
    assert (one.region, len(one.ref), one.pos_offset, two.region, len(two.ref), two.pos_offset) == ("c1", 100, 0, "c2", 376, 256)
    assert [p.records["pos"].tolist() for p in (one, two)] == [[5, 99], [256, 375]]
    assert [p.strand["pos"].tolist() for p in (one, two)] == [[0], [300]]
    assert [p.links["a"].tolist() for p in (one, two)] == [[7, 7, 99, 99], [256, 256]] and one.links["b"].tolist() == [99, 180, 180, 256]
    assert [p.evidence["pos"].tolist() for p in (one, two)] == [[99], [370]]
    assert [(p.indels[0]["pos"].tolist(), p.indels[1], p.indels[2]["pos"].tolist()) for p in (one, two)] == [([50, 50], b"ACGT", [50]), ([256], b"ACGT", [256])]
    for p, x in ((one, one.records), (two, two.records)):
        assert x.dtype == engine.VARIANT_DTYPE and p.links.dtype == engine.LINK_DTYPE
    # what was not counted stays None
    bare = ct.part_of_columns(table, {"amplicon_reads": object()}, 0, 100, "c1", ref[:100], 0)
    assert bare[4:] == (None, None, None, None) and bare.records["pos"].tolist() == [5, 99]
    assert ct.part_of_columns(None, {}, 0, 100, "c1", ref, 0).records is None


def test_the_parts_of_an_axis_write_the_rows_below_each_contigs_length(tmp_path):
    """the hand-written rows in both slots of that axis, and rows in the guard columns of both, which no file may show"""
    a, want, f = asked(tmp_path)
    lens, shifts = (100, 120), (0, 256)
    ref = np.zeros(512, np.uint8)
    for n, s in zip(lens, shifts):
        ref[s:s + n] = np.frombuffer(tr.REF + b"A" * (n - len(tr.REF)), np.uint8)
    guard = [(100, 2, 5, 20), (255, 5, 7, 9), (376, 3, 4, 8), (400, 6, 2, 6)]
    gcols = [g[0] for g in guard]
    cols = sorted([c + s for s in shifts for c in tr.COLS] + gcols)
    table = np.sort(np.concatenate([tr.records(shift=s) for s in shifts] + [np.array(guard, engine.VARIANT_DTYPE)]), order="pos", kind="stable")
    counted = {"variant_strand": np.sort(np.concatenate([tr.strand(shift=s) for s in shifts] + [only(engine.STRAND_DTYPE, "pos", gcols)]), order="pos"),
               "variant_evidence": np.sort(np.concatenate([tr.evidence(shift=s) for s in shifts] + [only(engine.EVIDENCE_DTYPE, "pos", gcols)]), order="pos"),
               "variant_links": tr.axis_links(2, cols, {c + s: (s, c) for s in shifts for c in tr.COLS}),
               "indel_events": tr.indels(sorted(tr.indel_rows(shift=0) + tr.indel_rows(shift=256) + [(255, 2, 2, "", 7, 9), (400, 1, 1, "G", 2, 6)], key=lambda t: t[:4]))}
    assert counted["variant_links"]["a"].tolist() == [c for c in cols for _ in range(2)] and (table["pos"] == np.sort(table["pos"])).all()
    parts = [ct.part_of_columns(table, counted, s, s + n, name, ref[:s + n], s) for name, n, s in zip(("c1", "c2"), lens, shifts)]
    assert np.concatenate([p.records["pos"] for p in parts]).tolist() == [p + s for s in shifts for p, *_ in tr.RECS]
    assert 266 in parts[1].links["a"] and 376 in parts[1].links["b"] and 100 in parts[0].links["b"]          # (pairs that leave the contig: cut by "a", written by nobody)
    # expected: each contig alone, from arrays that never held a guard row
    alone = [ct.TablePart(tr.records(shift=s), name, ref[:s + n], s, tr.strand(shift=s), tr.links(2, shift=s), tr.indels(tr.indel_rows(shift=s)), tr.evidence(shift=s))
             for name, n, s in zip(("c1", "c2"), lens, shifts)]
    rows = texts(want, alone)
    assert rows["t.tsv"].count("\n") == 12 and rows["i.tsv"].count("TAAA") == 2 and "c2\t11\tDEL\t4\tTAAA\t3\t12\t0.250000\n" in rows["i.tsv"]
    got = ct.write_tables(a, parts, want)
    for name in FILES:
        assert open(f[name]).read() == HEADERS[name] + rows[name], name
    assert got == stats_of(rows, 12)
    # a contig without rows: a part that writes no row
    empty = ct.part_of_columns(table, counted, 270, 376, "c3", ref[:376], 270)
    assert len(empty.records) == len(empty.strand) == len(empty.links) == len(empty.evidence) == len(empty.indels[0]) == len(empty.indels[2]) == 0
    got = ct.write_tables(a, [empty], want)
    assert [open(f[name]).read() for name in FILES] == [HEADERS[name] for name in FILES] and got == dict.fromkeys(KEYS, 0)


@pytest.mark.parametrize("broken, unwritten, written", (("strand", "t.tsv", ()), ("evidence", "e.tsv", ("t.tsv", "l.tsv", "i.tsv"))))
def test_counts_that_do_not_add_up_leave_their_file_unwritten(tmp_path, broken, unwritten, written):
    a, want, f = asked(tmp_path)
    p = part()
    bad = getattr(p, broken).copy()
    bad["fwd" if broken == "strand" else "n"][1][4] += 1                        # one G more at column 2 than the record has
    with pytest.raises(_ffi.TcmiError) as e:
        ct.write_tables(a, [part((0,)), p._replace(**{broken: bad})], want)     # (the first part is sound: nothing of it is written either)
    assert e.value.code == _ffi.E_ARG
    assert not os.path.exists(f[unwritten]) and [os.path.exists(f[n]) for n in FILES if n != unwritten] == [n in written for n in FILES if n != unwritten]


def test_no_variant_table_writes_nothing(tmp_path):
    a, want, f = asked(tmp_path)
    a.variant_table = None
    got = ct.write_tables(a, [part()], want)
    assert got == dict.fromkeys(KEYS, 0) and list(got) == list(KEYS) and len(got) == 12
    assert not any(os.path.exists(p) for p in f.values())
