"""--indel-table without a GPU: the yardstick (tests/indel_yardstick) on hand-written records with known answers and its invariant on
every fuzz seed and mode; the rule's host twin (tcmi_indel_passes) against Python's fractions; the hash (tcmi_indel_hash) against a
restatement; the host twin of the kernels' walk over the inserted bases; the merge of event lists; the writer (tcmi_indels_text); the
command line's refusals.  csrc/indel_rule.h, csrc/cigar_host.h and csrc/indels_text.cpp also run in a program of their own
(tests/indel_main.cpp), plain and under AddressSanitizer + UBSan."""
import ctypes as C
import os
import struct
from fractions import Fraction

import numpy as np
import pytest

from tests import fuzz_masked as fm
from tests import host_program
from tests import indel_yardstick as iy
from tests import synth_small as ss
from tests.cli_run import base_args as _base
from tests.cli_run import stub_files
from trueconsense_amd import TrueConsense as cli
from trueconsense_amd import _ffi, engine

TOP = (1 << 31) - 1
INS, DEL = iy.INS, iy.DEL
VARIANT = np.dtype([("pos", np.int32), ("allele", np.int32), ("count", np.int32), ("cov", np.int32)])


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("indel_main")
    src = ["tests/indel_main.cpp", "trueconsense_amd/csrc/indels_text.cpp"]
    return {"plain": host_program.build(src, d / "indel_main", sanitize=False), "sanitized": host_program.build(src, d / "indel_main_san")}


def _run(prog, mode, tmp_path, payload):
    inp, out = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    open(inp, "wb").write(payload)
    r = host_program.run(prog, mode, inp, out)
    assert r.stdout.startswith("ok "), (r.stdout[-2000:], r.stderr[-4000:])
    return open(out, "rb").read()


def rec(pos, cigar, seq=None, qual=None, flag=0, name="r"):
    n = sum(k for op, k in ss.parse_cigar(cigar) if op in iy.QUERY_OPS)
    seq = "".join("ACGT"[i % 4] for i in range(n)) if seq is None else seq
    return {"pos": pos, "flag": flag, "cigar": cigar, "seq": seq, "qual": [30] * len(seq) if qual is None and seq != "*" else (qual or []), "name": name, "tid": 0,
            "mapq": 60}


# ---- the yardstick on records with known answers -----------------------------------------------------------------------------------------
def test_i_runs_with_p_between_them():
    #             0123 4 56 78  9 (query)
    r = rec(100, "4M1I2P2I1S3M", "ACGTTGCAAAA")
    assert iy.record_events(r) == [(103, INS, 3, "TGC")]                        # the S stops an insertion that began with an I
    r = rec(100, "4M1P1I2S2I1H3M", "ACGTTAAGCAAA")
    assert iy.record_events(r) == [(103, INS, 3, "TGC")]                        # behind a P everything up to the next reference op: S consumes query
    assert iy.record_events(rec(100, "4M1P")) == [] and iy.record_events(rec(100, "4M1P3M")) == [] and iy.record_events(rec(100, "4M1I")) == [(103, INS, 1, "A")]
    assert iy.record_events(rec(100, "4M2S1I3M")) == []                         # an S first: no insertion is reported


def test_1d_plus_i_gives_both_kinds_on_one_column():
    r = rec(100, "4M1D2I3M", "ACGTGGAAA")
    assert iy.record_events(r) == [(104, DEL, 1, ""), (104, INS, 2, "GG")]
    r = rec(100, "4M3D2I3M", "ACGTGGAAA")                                       # a longer deletion: the kinds part
    assert iy.record_events(r) == [(104, DEL, 3, ""), (106, INS, 2, "GG")]
    assert iy.record_events(rec(100, "4M2D3D3M")) == [(104, DEL, 2, ""), (106, DEL, 3, "")]     # adjacent D ops are not merged
    assert iy.record_events(rec(100, "4M2N1I3M", "ACGTCAAA")) == [(105, INS, 1, "C")]           # a reference skip is no deletion


def test_a_d_op_cut_by_a_primers_edge():
    r = rec(100, "10M4D10M")                                                    # columns 100..123, the deletion on 110..113
    assert iy.record_events(r) == [(110, DEL, 4, "")]
    assert iy.record_events(r, [(95, 111, False)]) == []                        # head mask up to 110: the first column is masked, no event
    assert iy.record_events(r, [(95, 110, False)]) == [(110, DEL, 4, "")]       # ... up to 109: it is counted
    assert iy.record_events(r, [(112, 130, True)]) == [(110, DEL, 4, "")]       # cut on a later column: the event stays (its later '*' columns go)
    assert iy.record_events(r, [(110, 130, True)]) == []
    assert iy.record_events(r, [(100, 104, False)], shift=0) == [(110, DEL, 4, "")]


def test_the_floor_at_the_ops_query_index():
    q = [30] * 20
    q[10] = 5                                                                   # the base behind the deletion: the D token's query index
    assert iy.record_events(rec(100, "10M4D10M", qual=q), q=13) == []
    assert iy.record_events(rec(100, "10M4D10M", qual=q), q=5) == [(110, DEL, 4, "")]
    q = [30] * 12
    q[3] = 5                                                                    # the matched base in front of the insertion
    r = rec(100, "4M2I6M", "ACGTGGAAAAAA", q)
    assert iy.record_events(r, q=13) == [] and iy.record_events(r, q=0) == [(103, INS, 2, "GG")]
    q = [30] * 12
    q[4] = q[5] = 2                                                             # the inserted bases' own qualities are not asked
    assert iy.record_events(rec(100, "4M2I6M", "ACGTGGAAAAAA", q), q=13) == [(103, INS, 2, "GG")]


def test_seq_star_short_seq_and_the_last_match():
    assert iy.record_events(rec(100, "4M2I6M", "*")) == [(103, INS, 2, "NN")]
    assert iy.record_events(rec(100, "4M2I6M", "*"), q=1) == []                 # no SEQ, no QUAL: quality 0 is below any floor
    assert iy.record_events(rec(100, "4M3I6M", "ACGTG")) == [(103, INS, 3, "GNN")]
    assert iy.record_events(rec(100, "4M2I", "ACGTCC")) == [(103, INS, 2, "CC")]                # an insertion at the read's last match
    assert iy.record_events(rec(100, "4M2I3S", "ACGTCCAAA")) == [(103, INS, 2, "CC")]
    assert not iy.kept(rec(100, "4M", flag=4)) and not iy.kept(rec(100, "4S")) and iy.kept(rec(100, "4M"))


@pytest.mark.parametrize("mode", sorted(fm.MODES))
@pytest.mark.parametrize("seed", fm.SEEDS)
def test_the_invariant_on_the_yardstick_alone(seed, mode):
    """the insertions anchored on a column are the yardstick matrix's I plane there; the deletions are at most its coverage"""
    tabled, slack, q, f = fm.MODES[mode]
    counts, totals = iy.events(fm.fuzz(seed), fm.table_of(seed) if tabled else (), q, slack, f)
    matrix = fm.yardstick(seed, None, None, f, tabled, q, slack)[0]
    ins = np.zeros(len(matrix), np.int64)
    for c, (n_ins, n_del) in totals.items():
        ins[c] = n_ins
        assert n_del <= matrix[c, 0], (seed, mode, c)
    assert np.array_equal(ins, matrix[:, 6]) and ins.sum() > 50, (seed, mode, np.argwhere(ins != matrix[:, 6])[:5].tolist())
    assert sum(n_del for _, n_del in totals.values()) < matrix[:, 5].sum()      # (no identity for deletions: a deletion's later '*' columns anchor nothing)


# ---- the rule's host twin ------------------------------------------------------------------------------------------------------------------
def test_passes_against_fractions(programs, tmp_path):
    rng = np.random.default_rng(3)
    cases = []
    for _ in range(3000):
        den = int(rng.choice([1, 2, 3, 10, 100, 997, 1000000]))
        num = int(rng.integers(0, den + 1))
        cov = int(rng.choice([0, 1, 9, 10, 11, 100, 1000, TOP, int(rng.integers(1, TOP))]))
        count = int(rng.integers(0, cov + 1))
        if rng.random() < 0.3 and cov:                                          # an exact tie, and its neighbours
            count = min(cov, max(0, -(-num * cov // den) + int(rng.integers(-1, 2))))
        cases.append((count, cov, num, den, int(rng.choice([1, 2, 5])), int(rng.choice([0, 1, 10, 11]))))
    cases += [(TOP, TOP, 1000000, 1000000, 1, 0), (TOP - 1, TOP, 1000000, 1000000, 1, 0), (TOP, TOP, 999999, 1000000, TOP, TOP), (3, 100, 3, 100, 1, 10),
              (2, 100, 3, 100, 1, 10), (0, 0, 0, 1, 1, 0), (1, 9, 0, 1, 1, 10), (0, 10, 0, 1, 1, 10)]
    want = [int(iy.passes(*c)) for c in cases]
    assert 0.2 < sum(want) / len(want) < 0.8
    lib = _ffi.lib()
    assert [lib.tcmi_indel_passes(*c) for c in cases] == want
    for prog in programs.values():
        got = _run(prog, "passes", tmp_path, struct.pack("<q", len(cases)) + np.array(cases, np.int64).tobytes())
        assert np.frombuffer(got, np.int32).tolist() == want
    for bad in ((-1, 5, 1, 10, 1, 0), (1, -5, 1, 10, 1, 0), (1, 5, 11, 10, 1, 0), (1, 5, -1, 10, 1, 0), (1, 5, 1, 0, 1, 0), (1, 5, 1, 1000001, 1, 0),
                (1, 5, 1, 10, 0, 0), (1, 5, 1, 10, 1, -1)):
        assert lib.tcmi_indel_passes(*bad) == _ffi.E_ARG, bad
    assert engine.indel_passes(3, 100) and not engine.indel_passes(2, 100) and not engine.indel_passes(9, 9)


# ---- the hash ------------------------------------------------------------------------------------------------------------------------------
def test_hash_against_the_restatement(programs, tmp_path):
    rng = np.random.default_rng(4)
    cases = [(int(seed), int(bits), [int(x) for x in rng.integers(0, 16, int(rng.choice([0, 1, 2, 3, 7, 50])))]) for seed in range(4) for bits in (0, 8, 34)
             for _ in range(40)]
    want = [iy.hash_(seed, nib, bits) for seed, bits, nib in cases]
    assert [engine.indel_hash(seed, nib, bits) for seed, bits, nib in cases] == want
    assert all(w == 0 for w, c in zip(want, cases) if c[1] == 0) and max(want) >> 33 == 1 and all(w < 256 for w, c in zip(want, cases) if c[1] == 8)
    assert len({iy.hash_(s, [1, 2, 4], 34) for s in range(4)}) == 4 and iy.hash_(0, [1, 2], 34) != iy.hash_(0, [1, 2, 0], 34)
    payload = struct.pack("<q", len(cases)) + b"".join(struct.pack("<qqq", seed, bits, len(nib)) + bytes(nib) for seed, bits, nib in cases)
    for prog in programs.values():
        assert np.frombuffer(_run(prog, "hash", tmp_path, payload), np.uint64).tolist() == want


# ---- the host twin of the walk over the inserted bases -----------------------------------------------------------------------------------
def test_the_walk_against_the_yardstick(programs, tmp_path):
    rng = np.random.default_rng(5)
    cases = []
    for _ in range(600):
        n = int(rng.integers(1, 9))
        ops = [(int(rng.choice([0, 1, 1, 2, 3, 4, 5, 6, 6, 7, 8])), int(rng.integers(0, 5))) for _ in range(n)]
        cases.append((ops, int(rng.integers(0, n)), int(rng.integers(0, 50))))
    cases.append(([(0, 4), (1, 1), (6, 2), (1, 2), (4, 1), (0, 3)], 0, 4))
    cases.append(([(0, 4), (6, 1), (1, 1), (4, 2), (1, 2), (5, 1), (0, 3)], 0, 4))
    want = [iy.inserted(ops, k, y) for ops, k, y in cases]
    assert want[-2:] == [[4, 5, 6], [4, 7, 8]] and sum(bool(w) for w in want) > 50
    payload = struct.pack("<q", len(cases)) + b"".join(struct.pack("<qqq", len(ops), k, y) + np.array([n << 4 | op for op, n in ops], np.uint32).tobytes()
                                                       for ops, k, y in cases)
    for prog in programs.values():
        got = np.frombuffer(_run(prog, "walk", tmp_path, payload), np.int64).tolist()
        at = 0
        for w in want:
            assert got[at] == len(w) and got[at + 1:at + 1 + len(w)] == w
            at += 1 + len(w)
        assert at == len(got)


# ---- the merge of the parts' lists -------------------------------------------------------------------------------------------------------
def _merge(prog, tmp_path, parts, rule=None):
    payload = struct.pack("<qqqqqq", len(parts), rule is not None, *(rule or (0, 1, 1, 0)))
    for rep in parts:
        ev, text = iy.arrays(rep)
        payload += struct.pack("<qq", len(ev), len(text)) + ev.tobytes() + text
    got = _run(prog, "merge", tmp_path, payload)
    ok, n, tl = struct.unpack_from("<qqq", got)
    if not ok:
        return None
    ev = np.frombuffer(got, iy.EVENT_DTYPE, n, 24)
    return iy.unpack(ev, got[24 + 32 * n:24 + 32 * n + tl])


def test_merge_of_parts(programs, tmp_path):
    a = [(7, INS, 2, "AC", 3, 40), (7, DEL, 3, "", 1, 40), (9, INS, 1, "T", 2, 10)]
    b = [(9, INS, 1, "T", 1, 10), (7, INS, 2, "AG", 5, 40), (7, INS, 2, "AC", 1, 40), (3, DEL, 9, "", 4, 8), (7, INS, 1, "T", 1, 40)]
    merged = [(3, DEL, 9, "", 4, 8), (7, INS, 1, "T", 1, 40), (7, INS, 2, "AC", 4, 40), (7, INS, 2, "AG", 5, 40), (7, DEL, 3, "", 1, 40), (9, INS, 1, "T", 3, 10)]
    for prog in programs.values():
        assert _merge(prog, tmp_path, [a, b]) == merged == sorted(merged, key=lambda t: t[:4])
        assert _merge(prog, tmp_path, [b[::-1], [], a[::-1]]) == merged         # any order in, THE order out
        # the rule on the summed count: (7, INS, AC) passes 1/10 of 40 only with both parts' records
        assert _merge(prog, tmp_path, [a, b], (1, 10, 1, 0)) == [t for t in merged if iy.passes(t[4], t[5], 1, 10, 1, 0)] == [merged[0], merged[2], merged[3], merged[5]]
        assert _merge(prog, tmp_path, [a], (1, 10, 1, 0)) == [(9, INS, 1, "T", 2, 10)]
        assert _merge(prog, tmp_path, [a, [(7, INS, 2, "AC", 1, 41)]]) is None  # equal events that disagree on the coverage
        assert _merge(prog, tmp_path, []) == []


# ---- the writer ----------------------------------------------------------------------------------------------------------------------------
REF = b"acgtACGTNNacgtacgtac"
RECS = [(2, 6, 5, 50), (4, 5, 9, 60), (5, 5, 4, 60), (5, 6, 7, 60), (8, 1, 3, 70), (18, 5, 2, 20)]       # (pos, allele, count, cov); allele 5 '*', 6 '+'
REP = [(2, INS, 1, "T", 2, 50), (2, INS, 2, "AC", 3, 50), (4, DEL, 2, "", 9, 60), (5, INS, 3, "NRY", 7, 60), (5, DEL, 1, "", 1, 60), (18, DEL, 4, "", 2, 20)]
TOTALS = {2: [5, 0], 4: [0, 9], 5: [7, 1], 18: [0, 2]}
ROWS = ("ctg\t3\tINS\t1\tT\t2\t50\t0.040000\n" "ctg\t3\tINS\t2\tAC\t3\t50\t0.060000\n" "ctg\t5\tDEL\t2\tAC\t9\t60\t0.150000\n"
        "ctg\t6\tINS\t3\tNRY\t7\t60\t0.116667\n" "ctg\t6\tDEL\t1\tC\t1\t60\t0.016667\n" "ctg\t19\tDEL\t4\tACNN\t2\t20\t0.100000\n")


def _text_payload(rep, totals, recs, region=b"ctg", ref=REF, pos_offset=0, text=None, events=None):
    ev, tx = iy.arrays(rep)
    ev = ev if events is None else events
    tx = tx if text is None else text
    cols = sorted(totals)
    tot = iy.totals_at(totals, cols)
    recs = np.array(recs, VARIANT)
    return struct.pack("<7q", len(ev), len(tx), len(tot), len(recs), pos_offset, len(region), len(ref)) + region + ref + tx + ev.tobytes() + tot.tobytes() + recs.tobytes()


def _text(prog, tmp_path, *args, **kw):
    got = _run(prog, "text", tmp_path, _text_payload(*args, **kw))
    head, _, rows = got.partition(b"\n")
    rc, ln = (int(x) for x in head.split())
    assert ln == len(rows)
    return rc, rows.decode()


def test_rows_against_hand_formatted_text(programs, tmp_path):
    assert iy.text(REP, "ctg", REF) == ROWS and REP == sorted(REP, key=lambda t: t[:4])
    ev, tx = iy.arrays(REP)
    assert engine.indels_text(ev, tx, iy.totals_at(TOTALS, sorted(TOTALS)), np.array(RECS, VARIANT), "ctg", REF) == ROWS
    for prog in programs.values():
        assert _text(prog, tmp_path, REP, TOTALS, RECS) == (0, ROWS)
        assert _text(prog, tmp_path, [], {}, []) == (0, "")
        assert _text(prog, tmp_path, [], TOTALS, RECS) == (0, "")               # totals and no reported event
        rc, rows = _text(prog, tmp_path, REP[:3], {2: [5, 0], 4: [0, 9]}, RECS[:2], pos_offset=2)
        assert rc == 0 and rows == "ctg\t1\tINS\t1\tT\t2\t50\t0.040000\nctg\t1\tINS\t2\tAC\t3\t50\t0.060000\nctg\t3\tDEL\t2\tAC\t9\t60\t0.150000\n"


def test_every_refusal_of_the_writer(programs, tmp_path):
    def broken(**kw):
        totals = {c: list(v) for c, v in TOTALS.items()}
        totals.update(kw.pop("totals", {}))
        for c in kw.pop("drop", ()):
            del totals[c]
        rep = kw.pop("rep", REP)
        recs = kw.pop("recs", RECS)
        return (rep, totals, recs), kw

    ev, _ = iy.arrays(REP)
    off_text = ev.copy()
    off_text["text_off"][3] = 4                                                 # three letters from offset 4 of six
    no_kind = ev.copy()
    no_kind["kind"][0] = 3
    cases = {
        "the invariant: a '+' row's depth is not the insertions' total": broken(totals={5: [6, 1]}),
        "more deletions than coverage": broken(totals={18: [0, 21]}),
        "a total's position is not a '*' or '+' record's": broken(totals={3: [0, 0]}),
        "a position without totals": broken(drop=[4]),
        "totals at a base record's position": broken(totals={8: [0, 0]}),
        "the sort order: kind": broken(rep=[REP[0], REP[1], REP[2], REP[4], REP[3], REP[5]]),
        "the sort order: bases": broken(rep=[(2, INS, 2, "AG", 1, 50), (2, INS, 2, "AC", 3, 50)]),
        "the same event twice": broken(rep=[REP[0], REP[0]]),
        "an event on no queried position": broken(rep=[(3, DEL, 1, "", 1, 50)]),
        "an event's coverage is not the records'": broken(rep=[(2, INS, 1, "T", 2, 51)]),
        "more records than the kind's total": broken(rep=[(2, INS, 1, "T", 6, 50)]),
        "a length of zero": broken(rep=[(4, DEL, 0, "", 1, 60)]),
        "letters outside the text": broken(events=off_text),
        "no such kind": broken(events=no_kind),
        "no such letter": broken(text=b"TACnRY"),
        "a record in front of the offset": broken(pos_offset=3),
        "a record beyond the reference": broken(ref=REF[:18]),
        "records out of order": broken(recs=RECS[::-1]),
    }
    for prog in programs.values():
        for label, (args, kw) in cases.items():
            assert _text(prog, tmp_path, *args, **kw) == (_ffi.E_ARG, ""), label
    lib, ln = _ffi.lib(), C.c_int64(5)
    assert lib.tcmi_indels_text(None, 0, None, 0, None, 0, None, 0, None, 0, None, 0, None, 0, C.byref(ln)) == _ffi.E_ARG and ln.value == 0
    assert lib.tcmi_indels_text(None, -1, None, 0, None, 0, None, 0, b"c", 0, None, 0, None, 0, C.byref(ln)) == _ffi.E_ARG
    with pytest.raises(_ffi.TcmiError):
        engine.indels_text(*iy.arrays(REP), iy.totals_at({**TOTALS, 5: [6, 1]}, sorted(TOTALS)), np.array(RECS, VARIANT), "ctg", REF)


def test_the_columns_the_command_line_asks_about():
    cols, cov = engine.indel_columns(np.array(RECS, VARIANT))
    assert cols.tolist() == [2, 4, 5, 18] and cov.tolist() == [50, 60, 60, 20]
    cols, cov = engine.indel_columns(np.zeros(0, VARIANT))
    assert len(cols) == 0 and len(cov) == 0
    assert engine.INDELS_HEADER == iy.HEADER and engine.INDEL_EVENT_DTYPE == iy.EVENT_DTYPE and engine.INDEL_TOTALS_DTYPE == iy.TOTALS_DTYPE
    assert _ffi.K_INDEL_EVENTS == 15 and _ffi.lib().tcmi_abi_version() == 5


# ---- the command line ----------------------------------------------------------------------------------------------------------------------
def test_the_flag_and_what_it_counts_under(tmp_path):
    f = stub_files(tmp_path, ("x.bam", "r.fa", "f.gff", "o.csv.gz"))
    a = cli.GetArgs(_base(f) + ["--variant-table", "t.tsv", "--indel-table", "i.tsv", "--min-af", "1/10", "--min-alt-depth", "2", "--variant-min-depth", "5"])
    want = cli.StreamCounts(a)
    assert a.indel_table == "i.tsv" and want and want.indels == "i.tsv" and want.lists_records and want.need == "--indel-table"
    assert want.variants == dict(min_af=Fraction(1, 10), min_alt_depth=2, min_depth=5)
    b = cli.GetArgs(_base(f) + ["--variant-table", "t.tsv"])
    assert b.indel_table is None and not cli.StreamCounts(b)


def test_refusals_exit_1_with_one_line_and_write_nothing(tmp_path, capsys, monkeypatch):
    monkeypatch.chdir(tmp_path)
    f = stub_files(tmp_path, ("x.bam", "r.fa", "f.gff", "o.csv.gz"))
    man = tmp_path / "m.tsv"
    man.write_text("%s\tS0\to0.fa\t-\t-\t-\tt0.tsv\n" % f["x.bam"])
    batch = ["--batch", str(man), "-ref", f["r.fa"], "-gff", f["f.gff"], "-cov", "30"]
    both = ["--variant-table", "t.tsv", "--indel-table", "i.tsv"]
    before = sorted(os.listdir(tmp_path))
    for argv, word in ((_base(f) + ["--indel-table", "i.tsv"], "--indel-table needs --variant-table"),
                       (batch + ["--indel-table", "i.tsv"], "--batch is refused"),
                       (batch + ["--indel-table", "i.tsv", "--gpus", "2"], "--batch is refused"),
                       (_base(f) + both + ["--index-override", f["o.csv.gz"]], "--index-override"),
                       (_base(f) + both + ["--gpus", "2"], "-i --gpus N"),
                       (_base(f) + both + ["--gpus", "8", "--variant-strand"], "-i --gpus N")):
        for call in (cli.GetArgs, cli.main):
            with pytest.raises(SystemExit) as e:
                call(argv)
            out = capsys.readouterr().out
            assert e.value.code == 1 and word in out and "--indel-table" in out and out.count("\n") == 1 and out.endswith("Exiting...\n"), (argv, out)
    assert sorted(os.listdir(tmp_path)) == before
