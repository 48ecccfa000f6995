"""CPU: the records of tests/odd_cigars.py before any of them goes to a GPU.  The generator keeps its promises (every class among the
kept records of every seed, in every setting); the three references — the column-major emulator (tc_oracle.pileup_columns), the
read-major C oracle and tc_oracle.read_tokens through the primer yardstick — agree on every tolerated file; the host reader
(engine.BamFile) and the host packer (tests/host_pack_main.cpp under AddressSanitizer + UBSan) give the oracle's matrix on them, refuse
every file with a liar in it with TCMI_E_FORMAT and the record's index, and take the files whose liar is ignored anyway."""
import collections

import numpy as np
import pytest

from oracle import c_oracle
from oracle import tc_oracle as orc
from tests import host_pack_program as hpp
from tests import odd_cigars as oc
from tests import primer_yardstick as py
from tests import read_specs as rs
from trueconsense_amd import engine
from trueconsense_amd.io import bamwriter


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    return hpp.build_program(str(tmp_path_factory.mktemp("odd_host") / "host_pack_main"))


def tolerated():
    """-> [(label, records, arrays)]: the seeds and the hand-made list"""
    out = [("seed%d" % s,) + oc.seed_case(s) for s in oc.SEEDS]
    hand = oc.hand_specs()
    return out + [("hand", hand, rs.arrays(hand))]


# ---- 1. the generator's promises -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", oc.SEEDS)
def test_generator_keeps_its_promises(seed):
    specs, rd = oc.seed_case(seed)
    assert 1800 <= len(specs) <= 2200 and [r["pos"] for r in specs] == sorted(r["pos"] for r in specs)
    kept = [r for r in specs if oc.kept(r)]
    assert len(kept) * 3 >= len(specs)
    assert [oc.kept(r) for r in specs] == [orc.read_piles_up(rd, i) for i in range(len(specs))]
    per_class = collections.Counter(oc.class_of(r) for r in kept)
    for cls in oc.CLASSES:
        if cls in oc.NOT_KEPT:
            assert per_class[cls] == 0 and any(oc.class_of(r) == cls for r in specs), cls
            continue
        assert per_class[cls] >= 20, (cls, per_class[cls])
        mine = [r for r in kept if oc.class_of(r) == cls]
        assert {oc.setting_of(r) for r in mine} == set(oc.SETTINGS), cls
        assert {bool(r["flag"] & 16) for r in mine} == {False, True}, cls                      # both strands
        assert any(oc.sums(oc.words_of(r))[0] > oc.LONG for r in mine), cls                     # tally_stream_kernel's
        quals = [q for r in mine for q in r["qual"]]
        assert cls in ("DN_only", "seq_star") or (12 in quals and 13 in quals) or cls == "qual_ff", cls      # around the floor 13
    assert max(oc.sums(oc.words_of(r))[1] for r in specs) < oc.BOUND
    # what the classes say of SEQ against the CIGAR's query total
    for r in kept:
        cls, yq, n = oc.class_of(r), oc.sums(oc.words_of(r))[1], 0 if r["seq"] == "*" else len(r["seq"])
        if cls.startswith("seq_short"):
            assert 0 < n < yq and (cls != "seq_short_1" or n == yq - 1)
        elif cls.startswith("seq_long"):
            assert n > yq and (cls != "seq_long_1" or n == yq + 1)
        elif cls == "seq_star":
            assert n == 0 < yq
        elif cls == "seq_odd":
            assert n == yq and n % 2 == 1
        elif cls == "qual_ff":
            assert set(r["qual"]) == {255}
    # at a mask edge: the record's first column in a '+' primer or its last in a '-' primer of the seed's table
    table = oc.fm.table_of(seed)
    edge = [r for r in kept if oc.setting_of(r) == "edge"]
    masked = sum(py.read_mask(r["pos"], r["pos"] + oc.sums(oc.words_of(r))[0] - 1, table) != (r["pos"], r["pos"] + oc.sums(oc.words_of(r))[0]) for r in edge)
    assert masked * 10 >= len(edge) * 9, (masked, len(edge))


def test_hand_made_lists_hold_what_they_name():
    hand = oc.hand_specs()
    ops = collections.Counter(op for r in hand for op, _ in oc.ss.parse_cigar(r["cigar"]))
    assert set(ops) == set(range(16)) and any(n == 0 for r in hand for _, n in oc.ss.parse_cigar(r["cigar"]))
    assert {r["flag"] & 16 for r in hand} == {0, 16}
    large = oc.large_specs()
    totals = sorted(oc.sums(oc.words_of(r))[1] for r in large)
    assert totals[-1] == oc.BOUND - 1 and (1 << 20) + 19 in totals and (1 << 20) + 20 in totals and 536870012 in totals
    for kind, cig in oc.LIARS.items():
        span, yq, bad = oc.sums([(n << 4) | oc.hb.OPS.index(op) for n, op in cig])
        assert span == 20 and bad == 1 and yq >= oc.BOUND, kind
    assert oc.sums([(n << 4) | oc.hb.OPS.index(op) for n, op in oc.LIARS["yq_2p29"]])[1] == oc.BOUND
    assert oc.sums([(n << 4) | oc.hb.OPS.index(op) for n, op in oc.LIARS["S_x9"]])[1] % (1 << 32) >= 1 << 31          # negative as int32
    assert oc.sums([(n << 4) | oc.hb.OPS.index(op) for n, op in oc.LIARS["S_x17"]])[1] % (1 << 32) < oc.BOUND         # positive again, and below the bound


# ---- 2. the three references agree -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("label", ["seed%d" % s for s in oc.SEEDS] + ["hand"])
def test_three_references_agree(label):
    _, specs, rd = next(t for t in tolerated() if t[0] == label)
    n_pos = c_oracle.extent(rd, oc.L)
    by_c = c_oracle.tally(rd, n_pos)
    by_columns = orc.tally_matrix(rd, oc.L)
    by_tokens = py.counts(rd, oc.L)[0]
    assert np.array_equal(by_c, by_columns), np.argwhere(by_c != by_columns)[:6].tolist()
    assert np.array_equal(by_c, by_tokens), np.argwhere(by_c != by_tokens)[:6].tolist()
    assert by_c[:, 5].sum() > 0 and by_c[:, 6].sum() > 0


def test_large_but_legal_totals_by_hand_and_by_the_c_oracle():
    large = oc.large_specs()
    rd = rs.arrays(large)
    want = oc.large_matrix(large, 400)
    assert np.array_equal(c_oracle.tally(rd, 400), want)
    assert want[129, 6] == 1 and want[134, 6] == 1 and want[100:112, 1:5].sum() == 0 and want[150:170, 1:5].sum() == 0


# ---- 3. the host reader and the host packer ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("label", ["seed%d" % s for s in oc.SEEDS] + ["hand", "large"])
def test_host_reader_and_packer_give_the_oracle_matrix(prog, tmp_path, label):
    rd = rs.arrays(oc.large_specs()) if label == "large" else next(t for t in tolerated() if t[0] == label)[2]
    path = str(tmp_path / "A.bam")
    bamwriter.write_bam(path, rd, ref_len=oc.L, block=4096)
    b = engine.BamFile(path)
    assert b.n_reads == rd["n_reads"]
    a = b.arrays()
    assert np.array_equal(a["cigar"][:len(rd["cigar"])], rd["cigar"])
    reads = {k: np.array(a[k]) for k in ("pos", "flag", "l_qseq", "tid", "cigar_off", "cigar", "seq_off", "seq")}
    reads["n_reads"] = b.n_reads
    hpp.check(prog, tmp_path, reads, L=c_oracle.extent(rd, 0))


def host_verdict(prog, tmp_path, path, read_filter=None):
    b = engine.BamFile(path, read_filter=read_filter)
    a = b.arrays()
    reads = {k: np.array(a[k]) for k in ("pos", "flag", "l_qseq", "tid", "cigar_off", "cigar", "seq_off", "seq")}
    reads["n_reads"] = b.n_reads
    return reads, hpp.run(prog, tmp_path, reads)


@pytest.mark.parametrize("kind", list(oc.LIARS))
def test_host_route_refuses_a_liar_wherever_it_lies(prog, tmp_path, kind):
    for place in oc.PLACES:
        path = str(tmp_path / "liar.bam")
        at = oc.refused_file(path, kind, place)
        reads, got = host_verdict(prog, tmp_path, path)
        assert reads["n_reads"] == 41
        yq = oc.sums(reads["cigar"][int(reads["cigar_off"][at]):int(reads["cigar_off"][at + 1])])[1]
        assert got[:2] == ("refused", hpp.E_FORMAT) and "read %d " % at in got[2] and " %d query bases" % yq in got[2], (place, at, got)


@pytest.mark.parametrize("kind", list(oc.LIARS))
def test_host_route_takes_a_liar_that_is_ignored_anyway(prog, tmp_path, kind):
    good = str(tmp_path / "good.bam")
    oc.good_file(good)
    want = c_oracle.tally(c_oracle.read_bam(good), oc.GOOD_L)
    assert want[:, 0].max() >= 2 and want[:, 5].sum() > 0 and want[:, 6].sum() > 0
    for form in oc.IGNORED:
        path = str(tmp_path / "ignored.bam")
        oc.refused_file(path, kind, "middle", form)
        reads, got = host_verdict(prog, tmp_path, path, read_filter=oc.F if form == "filtered" else None)
        assert isinstance(got, dict), (form, got)
        assert reads["n_reads"] == (40 if form == "filtered" else 41)
        assert np.array_equal(hpp.decode(got, oc.GOOD_L)[0], want), form
