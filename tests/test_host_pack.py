"""CPU: the host packer (csrc/host_pack.h, host_pack.cpp: select, plan_chunks, pack_aligned, pack_general) in a program of its own —
tests/host_pack_main.cpp, built here with AddressSanitizer + UBSan and run as a child process — against a restatement of the packed
layout (csrc/readset_layout.h) in this file: the packed arrays are decoded with numpy back into a count matrix that must equal the
oracle's bit for bit, every chunk must keep what tally_planes_kernel takes on trust, every refusal must come with its code and text,
and no sanitizer may report (a report ends the program with a non-zero status)."""
import re

import numpy as np
import pytest

from oracle import c_oracle
from tests import fuzz_reads as fz
from tests import synth_small as ss
from tests.host_pack_program import (DEFAULTS, E_ARG, E_UNSUPPORTED, EV_I, EV_OTHER, EV_X, EVPOS, F_BLOCK, F_MAXSPAN, F_MAXSTAGE, F_MAXW, F_SEG, F_SEQCAP,
                                     OUT_TYPES, P_NPL, P_SUB, ROUND, TOTALS, algorithmic_bytes, balanced_chunk, build_program, check, chunk_reads, decode,
                                     fuzz_cases, plain_reads, read_words, run, short_reads, slices_of, stage_reads)


# ---- the program: tests/host_pack_program.py ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    return build_program(str(tmp_path_factory.mktemp("host_pack") / "host_pack_main"))


# ---- the inputs --------------------------------------------------------------------------------------------------------------------------


def concat(parts, tids):
    """several read dicts as one, part k on reference tids[k]"""
    out = {"n_reads": sum(p["n_reads"] for p in parts)}
    for k in ("pos", "flag", "l_qseq", "cigar", "seq"):
        out[k] = np.concatenate([p[k] for p in parts])
    out["tid"] = np.concatenate([np.full(p["n_reads"], t, np.int32) for p, t in zip(parts, tids)])
    for k, v in (("cigar_off", "cigar"), ("seq_off", "seq")):
        shift = np.cumsum([0] + [len(p[v]) for p in parts[:-1]])
        out[k] = np.concatenate([parts[0][k][:1]] + [p[k][1:] + np.uint64(s) for p, s in zip(parts, shift)]).astype(np.uint64)
    return out


@pytest.fixture(scope="module")
def fuzz():
    return fuzz_cases()


@pytest.fixture(scope="module")
def short():
    return short_reads()


# ---- the tests ---------------------------------------------------------------------------------------------------------------------------
def test_every_cigar_op_sorted_unsorted_and_long_reads(prog, tmp_path, fuzz):
    for name, reads in fuzz:
        d, _ = check(prog, tmp_path, reads)
        T = d["totals"]
        assert T["g_reads"] == 0 and T["f_events"] > 0, name
        spans = np.array([sum(l for op, l in zip(reads["cigar"][a:b] & 15, reads["cigar"][a:b] >> 4) if op in (0, 2, 3, 7, 8))
                          for a, b in zip(reads["cigar_off"][:-1].astype(int), reads["cigar_off"][1:].astype(int))])
        keep = (reads["flag"] & 4 == 0) & (reads["tid"] == 0) & (spans > 0)
        assert T["alg"] == algorithmic_bytes(reads, keep), name
        if name == "long":                                            # pieces of F_SEG positions, re-sorted: more entries than reads
            as_it_is = np.array([re.fullmatch("5*4*[078]+4*5*", "".join(str(op) for op in reads["cigar"][a:b] & 15)) is not None
                                 for a, b in zip(reads["cigar_off"][:-1].astype(int), reads["cigar_off"][1:].astype(int))]) & (spans <= F_MAXSPAN)
            pieces = np.where(as_it_is, 1, -(-spans // F_SEG))
            assert spans[keep].max() > 2 * F_SEG and T["n_piled"] == T["f_reads"] == pieces[keep].sum() > keep.sum()
            starts = np.concatenate([c["P0"] + (d["f_lenoff"][c["read0"]:c["read0"] + c["n_reads"]] & 1023) for c in d["f_chunk"]])
            assert np.all(np.diff(starts.astype(np.int64)) >= 0)
        else:
            assert T["n_piled"] == T["f_reads"] == keep.sum(), name


def test_reads_per_lane_rule_caps_a_chunk_before_its_stages_do(prog, tmp_path, short):
    # chunk_stages = 8 is the default's eight stages without the balanced cap.  Sorted starts: a chunk's window is as wide as its own reads
    # reach, the first one's below 512 positions (S = 17), and its eight stages fill up before a lane has seen 255 reads (the chunk closes
    # on the size the window WITH the next read would allow, so it may end a little short of eight full stages)
    d, largest = check(prog, tmp_path, short, chunk_stages=8)
    c = d["f_chunk"][0]
    S, sub = slices_of(int(c["Wn"])), int(c["sub_reads"])
    assert 8 * sub < 255 * S and 7 * sub < largest == c["n_reads"] <= 8 * sub
    # the same reads in any order: every chunk's window spans all of them, S = 10, and 255 reads per lane x 10 slices < 8 stages of 480 reads
    order = np.random.default_rng(70).permutation(6000)
    mixed = dict(short, pos=short["pos"][order], l_qseq=short["l_qseq"][order], cigar=short["cigar"][order])
    mixed["seq_off"] = np.concatenate([[0], np.cumsum((mixed["l_qseq"] + 1) // 2)]).astype(np.uint64)
    mixed["seq"] = np.concatenate([short["seq"][int(a):int(b)] for a, b in zip(short["seq_off"][order], short["seq_off"][order + 1])])
    d, largest = check(prog, tmp_path, mixed, chunk_stages=8)
    c = d["f_chunk"][0]
    S, sub = slices_of(int(c["Wn"])), int(c["sub_reads"])
    assert S == 10 and sub == 480 and 255 * S < 8 * sub and largest == c["n_reads"] == 255 * S // sub * sub == 2400


def test_run_count_field_rolls_over_at_4095(prog, tmp_path):
    rng = np.random.default_rng(5)
    one = plain_reads(rng, [33], [150])
    reads = plain_reads(rng, np.full(5000, 33), np.full(5000, 150))
    reads["seq"] = np.tile(one["seq"], 5000)
    d, _ = check(prog, tmp_path, reads, chunk_stages=8)
    # a window of 150 positions leaves S = 51 slices and stages of 408 reads: a chunk ends at 8 x 408 reads, below the field's limit
    assert list(d["f_covrun"] >> 20) == [3264, 1736] == [int(c["n_reads"]) for c in d["f_chunk"]]
    # 100 bases: S = 64, stages of 512, a chunk of 4 096 equal reads — one more than the field counts
    one = plain_reads(rng, [32], [100])
    reads = plain_reads(rng, np.full(5000, 32), np.full(5000, 100))
    reads["seq"] = np.tile(one["seq"], 5000)
    d, largest = check(prog, tmp_path, reads, chunk_stages=8)
    assert largest == 4096 and list(d["f_covrun"] >> 20) == [4095, 1, 904]              # a run was split although its reads are equal


def test_header_limits_512_513_600_601(prog, tmp_path):
    rng = np.random.default_rng(6)
    lens, cigars = [], []
    for n in (512, 513, 600, 601):
        lens += [n, n - 1]
        cigars += ["%dM" % n, "%dM1D%dM" % (n // 2, n - 1 - n // 2)]                # as it is (<= 600), and projected: one piece or two
    reads = plain_reads(rng, np.sort(rng.integers(0, 3000, 8 * 20)), lens * 20, cigars * 20)
    d, _ = check(prog, tmp_path, reads)
    got = set(int(v) for v in (d["f_lenoff"] >> 10) & 1023)
    assert got == {512, 513, 600, 1, 88, 89}                                          # 601 = 512 + 89, projected 513 = 512 + 1, 600 = 512 + 88


def test_balanced_cap_stage_count_and_stage_cap(prog, tmp_path, short):
    d, largest = check(prog, tmp_path, short, slots=8)
    assert largest == 750 == balanced_chunk(6000, 8) and [int(c["n_reads"]) for c in d["f_chunk"]] == [750] * 8
    # 1 024 slots: 6 reads per slot would do, the cap's floor of 64 holds
    d, largest = check(prog, tmp_path, short, slots=1024)
    assert largest == 64 == balanced_chunk(6000, 1024) and len(d["f_chunk"]) == -(-6000 // 64)
    d, largest = check(prog, tmp_path, short, chunk_stages=1)
    assert all(c["n_reads"] <= c["sub_reads"] and not c["stage_end"][1:].any() for c in d["f_chunk"]) and largest == d["f_chunk"][0]["sub_reads"]
    d, largest = check(prog, tmp_path, short, stage_cap=64, chunk_stages=8)
    assert all(c["sub_reads"] <= max(64, 4 * slices_of(int(c["Wn"]))) < stage_reads(int(c["Wn"]), 5, 0) for c in d["f_chunk"])
    assert len(d["f_chunk"]) > 2 and max(int(c["n_reads"]) // int(c["sub_reads"]) for c in d["f_chunk"]) >= 7


def test_batch_of_three_with_stride(prog, tmp_path):
    rng = np.random.default_rng(8)
    batch = [fz.random_reads(rng, 300, 1900) for _ in range(3)]
    assert max(c_oracle.extent(r, 0) for r in batch) <= 2048
    d = run(prog, tmp_path, batch, stride=2048)
    got, _ = decode(d, 3 * 2048)
    assert np.array_equal(got, np.concatenate([c_oracle.tally(r, 2048) for r in batch]))
    assert d["totals"]["n_reads"] == 900 and d["totals"]["max_end"] == 2 * 2048 + c_oracle.extent(batch[2], 0)


def test_contig_layout_drops_counts_and_refuses(prog, tmp_path):
    rng = np.random.default_rng(9)
    parts = [fz.random_reads(rng, 300, 900), fz.random_reads(rng, 200, 500), fz.random_reads(rng, 50, 400)]
    for p in parts:
        p["pos"][p["tid"] < 0] = -1                                                   # (tid -1 goes: part k lies on reference k)
    ext = [c_oracle.extent(p, 0) for p in parts]
    reads = concat(parts, [0, 1, 2])
    layout = [(0, 1024), (1024 + 256, ext[1]), (-1, 0)]                               # reference 2 has no slot
    d = run(prog, tmp_path, reads, layout=layout)
    L = layout[1][0] + ext[1]
    got, _ = decode(d, L)
    want = np.zeros((L, 7), np.int64)
    want[:ext[0]] = c_oracle.tally(parts[0], ext[0])
    want[layout[1][0]:] = c_oracle.tally(parts[1], ext[1])
    assert np.array_equal(got, want)
    mapped2 = int(((parts[2]["flag"] & 4 == 0) & (parts[2]["pos"] >= 0)).sum())
    assert d["totals"]["n_dropped"] == mapped2 > 0 and list(d["ref_ext"]) == [ext[0], ext[1], 0] and d["totals"]["max_end"] == L
    # a read past its slot
    layout[1] = (layout[1][0], ext[1] - 1)
    ends = parts[1]["pos"].astype(np.int64) + [sum(l for op, l in ss.parse_cigar("".join("%d%s" % (w >> 4, "MIDNSHP=X"[w & 15]) for w in parts[1]["cigar"][a:b]))
                                                   if op in (0, 2, 3, 7, 8)) for a, b in zip(parts[1]["cigar_off"][:-1].astype(int), parts[1]["cigar_off"][1:].astype(int))]
    i = int(np.flatnonzero((ends == ext[1]) & (parts[1]["flag"] & 4 == 0))[0])
    assert run(prog, tmp_path, reads, layout=layout) == ("refused", E_UNSUPPORTED, "read %d on reference 1 ends past the end of its contig's slot (at %d)"
                                                         % (300 + i, ext[1]))


def test_general_set_far_positions_no_projection_no_fast_path(prog, tmp_path, fuzz):
    # positions around 2^29: the reads that end below it stay in the aligned set, the others go to the general set
    rng = np.random.default_rng(10)
    base = EVPOS - 2048
    near = fz.random_reads(rng, 600, 4000)
    want = c_oracle.tally(near, 4200)
    near["pos"] = (near["pos"].astype(np.int64) + base).astype(np.int32)
    d = run(prog, tmp_path, near)
    got, _ = decode(d, 4200, base=base)
    assert np.array_equal(got, want) and d["totals"]["g_reads"] > 50 and d["totals"]["f_reads"] > 50
    assert d["g_pos"].min() + 1 > EVPOS - 600 and d["totals"]["max_end"] > EVPOS
    reads = fuzz[0][1]
    d, _ = check(prog, tmp_path, reads, project_reads=0)                             # only [H][S] M.. [S][H] stays aligned
    assert d["totals"]["g_reads"] > 500 and d["totals"]["f_reads"] > 100 and d["totals"]["f_events"] > 0
    assert not (d["f_event"] & (EV_X | EV_I)).any()
    d, _ = check(prog, tmp_path, reads, use_fast=0)
    assert d["totals"]["f_reads"] == 0 and d["totals"]["g_reads"] == d["totals"]["n_piled"] and d["totals"]["f_words"] == 0


def test_every_refusal_of_select_code_and_text(prog, tmp_path):
    rng = np.random.default_rng(11)
    reads = plain_reads(rng, [10, 20, 30], [50, 50, 50])
    reads["tid"][1] = 1
    text = ("read 1 is mapped to reference 1: only single-reference alignments are supported (the reference implementation keys columns by "
            "position only and fails on these)")
    assert run(prog, tmp_path, reads) == ("refused", E_UNSUPPORTED, text[:159])      # (the text as far as the library's 160-byte buffer holds it)
    reads = plain_reads(rng, [10, 20, 30], [50, 50, 50])
    reads["l_qseq"][2] = -1
    assert run(prog, tmp_path, reads) == ("refused", E_ARG, "read 2 has negative l_qseq")
    reads = plain_reads(rng, [10, 20, 30], [50, 50, 50])
    reads["seq_off"][3] -= 1
    reads["seq"] = reads["seq"][:-1]
    assert run(prog, tmp_path, reads) == ("refused", E_ARG, "read 2: seq bytes 24 < ceil(l_qseq/2)")
    batch = [plain_reads(rng, [10], [50]), plain_reads(rng, [10, 2000], [50, 50])]
    assert run(prog, tmp_path, batch, stride=2048) == ("refused", E_ARG, "read 1 of a batched BAM ends at 2050, beyond the batch stride 2048")
    reads = plain_reads(rng, [10, (1 << 31) - 4096 - 50], [50, 50])
    assert run(prog, tmp_path, reads) == ("refused", E_UNSUPPORTED, "read 1 ends beyond 2^31")
    reads["pos"][1] -= 1                                                              # ... and the last position that is taken
    assert run(prog, tmp_path, reads)["totals"]["g_reads"] == 1


def test_empty_input_and_no_read_that_piles_up(prog, tmp_path):
    rng = np.random.default_rng(12)
    empty = ss.reads_from_spec({"reads": []})
    nothing = plain_reads(rng, [10, 20, -1], [50, 50, 50], ["50M", "50S", "50M"])
    nothing["flag"][0] = 4
    for reads, n in ((empty, 0), (nothing, 3)):
        d = run(prog, tmp_path, reads)
        assert d["totals"] == dict(dict.fromkeys(TOTALS, 0), n_reads=n)
        assert all(len(d[k]) == 0 for k in OUT_TYPES if k not in ("totals", "g_round_cig", "g_round_seq")) and list(d["g_round_cig"]) == [0]


def test_dump_is_byte_identical_for_1_3_and_8_threads(prog, tmp_path, fuzz):
    # 22 copies of the sorted case side by side: above 65 536 reads the classification itself runs in slices that are joined in order
    reads = fuzz[0][1]
    tiled = concat([reads] * 22, [0] * 22)
    tiled["tid"] = np.tile(reads["tid"], 22)
    tiled["pos"] = (np.tile(reads["pos"], 22) + np.repeat(np.arange(22) * 2048, reads["n_reads"])).astype(np.int32)
    for name, r in fuzz + [("tiled", tiled)]:
        dumps = [run(prog, tmp_path, r, raw=True, threads=t) for t in (1, 3, 8)]
        assert dumps[0] == dumps[1] == dumps[2] and len(dumps[0]) > 1000, name
