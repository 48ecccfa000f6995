"""The insert tokens (Events.ExtractInserts, Events.py:47-82) on fuzzed read sets (tests/fuzz_reads.py token_specs), against the
oracle's region pile-up (oracle/tc_oracle.py region_tokens) at every column: the host sweep (from arrays, from a BAM file: the
windowed path, under a contig layout), the vote over entries (tests/entries_py.py -> tcmi_modal_from_entries) and, on the GPU, the
device entries field by field, the device vote under both packers, block ranges, refusals and a whole file to its FASTA."""
import functools
from collections import Counter

import ctypes as C
import numpy as np
import pytest

from oracle import tc_oracle as orc
from tests import entries_py
from tests import fuzz_reads as fz
from tests import synth_small as ss
from trueconsense_amd import _ffi, contigs, distributed, engine
from trueconsense_amd import synthetic as sy
from trueconsense_amd.io import bamwriter

SEEDS = (0, 1, 2, 3)
L = 400
PAST = 12                                     # columns asked for past the reference's end
MATE_REF = ("mate_ref", 500)                  # a second @SQ: the reference of mates "on another reference"


@functools.lru_cache(maxsize=None)
def case(seed):
    """-> (reference, reads dict, specs); seed 0 carries the 8 600-read start position"""
    rng = np.random.default_rng(1000 + seed)
    ref, _ = sy.make_reference(seed=seed + 1, L=L, cds=[])
    specs = fz.token_specs(rng, ref, deep=seed == 0)
    return ref, ss.reads_from_spec({"reads": specs}), specs


def n_placed(reads):
    """the placed reads: a prefix (unplaced ones sit at the end of a sorted file)"""
    return int(np.count_nonzero((np.asarray(reads["tid"]) >= 0) & (np.asarray(reads["pos"]) >= 0)))


def max_span(reads):
    co = np.asarray(reads["cigar_off"], np.int64)
    return max(sum(int(w) >> 4 for w in reads["cigar"][co[i]:co[i + 1]] if int(w) & 15 in (0, 2, 3, 7, 8)) for i in range(int(reads["n_reads"])))


def part(reads, a, b):
    """reads [a, b) as a dict of their own, names and mate fields kept"""
    co, so, qo, no = (np.asarray(reads[k], np.int64) for k in ("cigar_off", "seq_off", "qual_off", "name_off"))
    out = {"n_reads": b - a}
    for k in ("pos", "flag", "l_qseq", "tid", "next_tid", "next_pos", "tlen"):
        out[k] = np.ascontiguousarray(reads[k][a:b])
    for k, o in (("cigar", co), ("seq", so), ("qual", qo), ("names", no)):
        out[k + "_off"] = (o[a:b + 1] - o[a]).astype(np.uint64)
        out[k] = np.ascontiguousarray(reads[k][int(o[a]):int(o[b])])
    if not len(out["names"]):
        out["names"] = np.zeros(1, np.uint8)
    out["name_off"] = out.pop("names_off")
    return out


def window(reads, pos1, span):
    """[a, b): the placed reads that can reach column pos1 - 1 (sorted by position, spans of at most `span`)"""
    pos = np.asarray(reads["pos"])[:n_placed(reads)]
    c = pos1 - 1
    return int(np.searchsorted(pos, c - span + 1, "left")), int(np.searchsorted(pos, c, "right"))


def modal(tokens):
    return (Counter(t.upper() for t in tokens).most_common(1)[0][0] if tokens else None, len(tokens))


@functools.lru_cache(maxsize=None)
def oracle(seed):
    """{1-based column: (modal upper-cased token or None, token count)} at every column of the case, and past its end"""
    _, reads, _ = case(seed)
    span = max_span(reads)
    out = {}
    for p in range(1, L + PAST + 1):
        a, b = window(reads, p, span)
        out[p] = modal(orc.region_tokens(part(reads, a, b), p)) if b > a else (None, 0)
    return out


def write(tmp_path, name, reads, refs=None):
    path = str(tmp_path / name)
    bamwriter.write_bam(path, reads, refs=refs or [("ref", L), MATE_REF], level=4)
    return path


# ---------------------------------------------------------------------------------------------------------------------- CPU
@pytest.mark.parametrize("seed", SEEDS)
def test_host_sweep_equals_the_oracle_at_every_column(seed):
    """tcmi_modal_tokens from the arrays (every read visited) at every column, and past the end."""
    _, reads, _ = case(seed)
    want = oracle(seed)
    assert engine.modal_tokens(reads, list(want)) == want


@pytest.mark.parametrize("seed", SEEDS)
def test_host_sweep_of_the_written_file_equals_the_oracle(seed, tmp_path):
    """The same reads as a sorted BAM through the host reader: the windowed sweep (only the reads that can reach a column)."""
    _, reads, _ = case(seed)
    bam = engine.BamFile(write(tmp_path, "f.bam", reads))
    assert bam.sorted == 1
    want = oracle(seed)
    assert engine.modal_tokens(bam, list(want)) == want
    bam.close()


def test_the_fuzz_reaches_the_cases_it_is_for():
    """Planted insertions become modal (short, 12 / 13 bases, 40+, on '*' / '>' / '<' tokens), exact ties between two
    insertions occur, the deep column is capped at max_depth, and SEQ-less / short-SEQ mates overlap their mates."""
    toks = [t for s in SEEDS for t, _ in oracle(s).values() if t]
    ins = [t for t in toks if "+" in t]
    lens = {int(t.split("+")[1].rstrip("ACGTNRYKMSWBDHV.,=")) for t in ins}
    assert len(ins) >= 12 and {12, 13} <= lens and max(lens) >= 40 and min(lens) <= 11
    assert any(t[0] in "*><" for t in ins) and any("," in t or "." in t for t in ins)
    _, deep, _ = case(0)
    a, b = window(deep, L // 2 + 1, max_span(deep))
    dp = part(deep, a, b)
    assert len(orc.region_tokens(dp, L // 2 + 1, min_base_quality=0)) == 8000 < len(orc.region_tokens(dp, L // 2 + 1, min_base_quality=0, max_depth=0))
    ties = 0
    for s in SEEDS:
        _, reads, _ = case(s)
        span = max_span(reads)
        for p, (t, n) in oracle(s).items():
            if t and "+" in t and n:
                a, b = window(reads, p, span)
                top = Counter(x.upper() for x in orc.region_tokens(part(reads, a, b), p)).most_common(2)
                ties += len(top) == 2 and top[0][1] == top[1][1] and "+" in top[1][0]
    assert ties >= 2
    seqless = 0
    for s in SEEDS:
        by_name = {}
        for r in case(s)[2]:
            by_name.setdefault(r["name"], []).append(r)
        seqless += sum(1 for rs in by_name.values() if len(rs) == 2 and rs[0]["flag"] & 2 and any(len(r["qual"]) < fz._qlen(ss_cig(r)) for r in rs))
    assert seqless >= 10


def ss_cig(r):
    return [(l, "MIDNSHP=X"[op]) for op, l in ss.parse_cigar(r["cigar"])]


def vote(ents, off, text):
    """tcmi_modal_from_entries (the configs[4] root's vote, no prober) -> ([(token or None, count)], status flags)"""
    n = len(off) - 1
    a = np.frombuffer(ents, np.uint8).copy() if ents else np.zeros(48, np.uint8)
    o = np.ascontiguousarray(off, np.int64)
    tb = np.frombuffer(text, np.uint8).copy() if text else np.zeros(1, np.uint8)
    cap = 1 << 20
    buf = C.create_string_buffer(cap)
    toff, cnt, st = np.zeros(n + 1, np.int64), np.zeros(n, np.int64), C.c_int32(0)
    _ffi.check(_ffi.lib().tcmi_modal_from_entries(n, a.ctypes.data_as(C.c_void_p), o.ctypes.data_as(C.c_void_p), 13, 8000, 1,
                                                  tb.ctypes.data_as(C.c_void_p), len(text), C.cast(buf, C.c_void_p), cap,
                                                  toff.ctypes.data_as(C.c_void_p), cnt.ctypes.data_as(C.c_void_p), C.byref(st)))
    return [(buf.raw[toff[k]:toff[k + 1]].decode("ascii") if cnt[k] else None, int(cnt[k])) for k in range(n)], st.value


def needs_probe(ents):
    """does the column hold two entries of one properly paired name, one of them a deletion / ref-skip whose next query base is a
    matched one (what only a probe of the other mate can settle)?"""
    e = np.frombuffer(ents, entries_py.ENT)
    names = Counter(int(h) for h, f in zip(e["name_hash"], e["flag"]) if f & 2)
    return any(names[int(x["name_hash"])] >= 2 and x["flag"] & 2 and not x["bits"] & 0x10 and x["qref"] >= 0 for x in e)


@pytest.mark.parametrize("seed", SEEDS)
def test_entry_vote_equals_the_oracle_where_no_probe_is_needed(seed):
    """entries_py.entries_for (the Python statement of the device's 48-byte entries) -> tcmi_modal_from_entries, column by column:
    the oracle's answer wherever status bit 1 (TCMI_TOKENS_OVERLAP_UNKNOWN) is clear; where it is set, the column really holds a
    pair of mates that needs a probe."""
    _, reads, _ = case(seed)
    span = max_span(reads)
    want = oracle(seed)
    probed = 0
    for p in want:
        a, b = window(reads, p, span)
        ents, off, text = entries_py.entries_for(part(reads, a, b), [p], j0=a) if b > a else (b"", [0, 0], b"")
        got, st = vote(ents, off, text)
        if st & 2:
            assert needs_probe(ents), p
            probed += 1
        else:
            assert got[0] == want[p], p
        assert not st & 1 or seed == 0                  # (max_depth drops reads on the deep column only)
    assert len(want) - probed >= len(want) // 2
    if seed == 1:
        assert probed >= 1


def test_contig_layout_equals_the_sweep_of_each_split_contig(tmp_path):
    """tcmi_modal_tokens_layout (the only token source of --per-contig) over 5 contigs plus a header reference the FASTA does not
    name and unplaced reads, names kept: on every column of every slot it equals the single-contig sweep of that contig's reads."""
    rng = np.random.default_rng(77)
    hdr = [("c0", 310), ("X", 200), ("c1", 257), ("c2", 400), ("c3", 123), ("c4", 345)]
    refs = {n: sy.make_reference(seed=20 + t, L=ln, cds=[])[0] for t, (n, ln) in enumerate(hdr)}
    specs = []
    for t, (n, _) in enumerate(hdr):
        specs += fz.token_specs(rng, refs[n], tid=t, tag=n + "_", n_ref=len(hdr))
    specs.sort(key=lambda r: (r["tid"] < 0, r["tid"], r["pos"]))
    reads = ss.reads_from_spec({"reads": specs})
    records = [(n, refs[n]) for n, _ in hdr if n != "X"]
    shift, slot, _ = contigs.layout_for(records, [n for n, _ in hdr], [ln for _, ln in hdr])
    bam = engine.BamFile(write(tmp_path, "multi.bam", reads, refs=hdr))
    n_ins = 0
    for t, (name, _) in enumerate(hdr):
        if shift[t] < 0:
            continue
        mine = []
        for r in specs:
            if r["tid"] == t:
                r = dict(r, tid=0, mtid=0 if r.get("mtid", -1) == t else -1 if r.get("mtid", -1) < 0 else 1)
                mine.append(r)
        want = engine.modal_tokens(ss.reads_from_spec({"reads": mine}), range(1, int(slot[t]) + 1))
        axis = [int(shift[t]) + p for p in range(1, int(slot[t]) + 1)]
        for src in (reads, bam):
            got = engine.modal_tokens(src, axis, layout=(shift, slot))
            assert {p - int(shift[t]): v for p, v in got.items()} == want, name
        n_ins += sum(1 for v, _ in want.values() if v and "+" in v)
    assert n_ins >= 20
    bam.close()


def test_crosscheck_cases_have_seqless_mates():
    """tools/pysam_crosscheck.py carries mates without SEQ / with a short SEQ, so that pysam can pin the rule where it is."""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import pysam_crosscheck
    names = [c[0] for c in pysam_crosscheck.cases()]
    assert any("SEQ" in n and "mates" in n for n in names)


# ---------------------------------------------------------------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def ctx():
    with engine.Context(0) as c:
        yield c


def _long_text(key, text):
    at, n = (key >> 8) & 0xFFFFFFFF, (key >> 40) & 0x7FFFFF
    return bytes(text[at:at + n])


@pytest.mark.gpu
@pytest.mark.parametrize("seed", (0, 1))
def test_device_entries_field_by_field(ctx, tmp_path, seed):
    """tcmi_readset_ins_entries (ins_entries_kernel over the device-decoded file) against entries_py.entries_for on the same reads:
    every field of every entry that has a token, long insertions by their text, file order within a column."""
    _, reads, _ = case(seed)
    d = engine.DeviceBam(write(tmp_path, "f.bam", reads))
    rs = ctx.upload_bamfile(d)
    assert rs.packed_on_device
    cols = list(range(1, L + PAST + 1))
    ents, off, text = distributed._entries_of_readset(ctx, rs, cols)
    rs.free()
    d.close()
    dev = np.frombuffer(ents, entries_py.ENT)
    span = max_span(reads)
    n_long = n_cmp = 0
    for k, p in enumerate(cols):
        got = dev[off[k]:off[k + 1]]
        got = got[got["key"] != 0]
        assert np.all(np.diff(got["j"].astype(np.int64)) > 0), p
        a, b = window(reads, p, span)
        pe, _, ptext = entries_py.entries_for(part(reads, a, b), [p], j0=a) if b > a else (b"", None, b"")
        want = np.frombuffer(pe, entries_py.ENT)
        assert len(got) == len(want), p
        for f in ("name_hash", "pos", "end", "mpos", "isize", "l_qseq", "flag", "qual", "bits", "qref"):
            assert np.array_equal(got[f], want[f]), (p, f, np.nonzero(got[f] != want[f])[0][:5])
        long_ = (want["bits"] & 0x40) != 0
        mask = np.uint64(~(0xFFFFFFFF << 8) & 0xFFFFFFFFFFFFFFFF)
        assert np.array_equal(got["key"] & np.where(long_, mask, np.uint64(0xFFFFFFFFFFFFFFFF)),
                              want["key"] & np.where(long_, mask, np.uint64(0xFFFFFFFFFFFFFFFF))), p
        for g, w in zip(got[long_], want[long_]):
            assert _long_text(int(g["key"]), text) == _long_text(int(w["key"]), ptext), p
            n_long += 1
        n_cmp += len(got)
    assert n_long >= 10 and n_cmp > 10000


@pytest.mark.gpu
@pytest.mark.parametrize("seed", SEEDS)
def test_device_tokens_equal_the_host_sweep_and_the_oracle(ctx, tmp_path, seed):
    """ctx.readset_modal_tokens == modal_tokens(BamFile) == oracle at every column (thousands of entries: a multi-block
    ins_entries_kernel grid), under the one-sync packer and the several-kernel one."""
    _, reads, _ = case(seed)
    path = write(tmp_path, "f.bam", reads)
    want = oracle(seed)
    cols = list(want)
    bam = engine.BamFile(path)
    assert engine.modal_tokens(bam, cols) == want
    bam.close()
    d = engine.DeviceBam(path)
    try:
        for one_sync in (1, 0):
            ctx.set_option("one_sync", one_sync)
            t0 = ctx.stat("one_sync_taken")
            rs = ctx.upload_bamfile(d)
            assert ctx.stat("one_sync_taken") - t0 == one_sync, ctx.stat("one_sync_last_decline_flags")
            assert ctx.readset_modal_tokens(rs, cols) == want, one_sync
            assert ctx.readset_modal_tokens(rs, [1, L, L + 1, L + PAST]) == {p: want[p] for p in (1, L, L + 1, L + PAST)}
            rs.free()
    finally:
        ctx.set_option("one_sync", 1)
        d.close()


@pytest.mark.gpu
def test_block_ranges_vote_to_the_whole_file(ctx, tmp_path):
    """The file cut into 3 ranges of BGZF blocks (the ranks of configs[4]): entries per range, rebased and voted on in range order,
    give the whole-file device answer wherever status bit 1 is clear."""
    _, reads, _ = case(1)
    path = str(tmp_path / "f.bam")
    bamwriter.write_bam(path, reads, refs=[("ref", L), MATE_REF], level=4, block=4096)
    d = engine.DeviceBam(path)
    assert d.n_blocks >= 6
    cols = list(range(1, L + PAST + 1))
    rs = ctx.upload_bamfile(d)
    whole = ctx.readset_modal_tokens(rs, cols)
    rs.free()
    cuts = [0, d.n_blocks // 3, 2 * d.n_blocks // 3 + 1, d.n_blocks]
    pieces = []
    for a, b in zip(cuts, cuts[1:]):
        rs = ctx.upload_bamfile(d, blocks=(a, b - a))
        pieces.append(distributed._entries_of_readset(ctx, rs, cols))
        rs.free()
    d.close()
    assert all(len(e) for e, _, _ in pieces)
    probed = 0
    for k, p in enumerate(cols):
        got, st = distributed._vote([p], [(e[o[k] * 48:o[k + 1] * 48], [0, o[k + 1] - o[k]], t) for e, o, t in pieces])
        if st & 2:
            probed += 1
            continue
        assert got[p] == whole[p][0], p
    assert len(cols) - probed >= len(cols) // 2
    assert sum(1 for t, _ in whole.values() if t and "+" in t) >= 5


@pytest.mark.gpu
def test_refusals_then_the_host_sweep(ctx, tmp_path):
    """Kept reads out of order (ins_sorted_kernel) and a read longer than 512 positions: E_UNSUPPORTED from the device, never a wrong
    vote; the host sweep of the same file gives the oracle's answer."""
    _, reads, specs = case(2)
    placed = [r for r in specs if r["tid"] >= 0]
    unplaced = [r for r in specs if r["tid"] < 0]
    a, b = next(i for i, r in enumerate(placed) if r["flag"] == 0 and r["pos"] > 50), None
    b = next(i for i in range(a + 1, len(placed)) if placed[i]["flag"] == 0 and placed[i]["pos"] > placed[a]["pos"] + 30)
    swapped = list(placed)
    swapped[a], swapped[b] = swapped[b], swapped[a]
    longer = placed + [{"pos": 10, "flag": 0, "cigar": "30M600N30M", "seq": "A" * 60, "qual": 30, "name": "long", "tid": 0}]
    longer.sort(key=lambda r: r["pos"])
    for name, sp in (("unsorted", swapped), ("long", longer)):
        rd = ss.reads_from_spec({"reads": sp + unplaced})
        path = write(tmp_path, name + ".bam", rd)
        d = engine.DeviceBam(path)
        rs = ctx.upload_bamfile(d)
        cols = list(range(1, L + 1, 7))
        with pytest.raises(_ffi.TcmiError) as e:
            ctx.readset_modal_tokens(rs, cols)
        assert e.value.code == _ffi.E_UNSUPPORTED, name
        if rs.packed_on_device:
            assert ("not sorted" if name == "unsorted" else "long reads") in str(e.value), str(e.value)
        rs.free()
        d.close()
        host = engine.modal_tokens(engine.BamFile(path), cols)
        for p in cols:
            assert host[p] == modal(orc.region_tokens(rd, p)), (name, p)


@pytest.mark.gpu
def test_planted_insertions_end_to_end_against_the_oracle_chain(ctx, tmp_path):
    """A fuzz BAM with planted insertions through FileRunner (device decode, device tokens, walk) -> the FASTA of the oracle chain
    (c_oracle.tally -> list_inserts over the region pile-up -> build_consensus)."""
    from oracle import c_oracle
    Lr = 3000
    rng = np.random.default_rng(5)
    ref, orfs = sy.make_reference(seed=9, L=Lr, cds=[(100, 1300), (1500, 2800)])
    specs = [r for r in fz.token_specs(rng, ref, background=Lr // 6, n_pairs=Lr // 30, n_sites=40, overhang=False)
             if r["pos"] + fz._span(ss_cig(r)) <= Lr]                   # (every read within the reference)
    reads = ss.reads_from_spec({"reads": specs})
    path = write(tmp_path, "e2e.bam", reads, refs=[("ref", Lr), MATE_REF])
    mincov = 8
    runner = engine.FileRunner(ctx, [{"start": o["start"], "end": o["end"], "strand": "+"} for o in orfs], mincov, gpu_streams=1)
    text = runner.run([path], names=["S"], ref_len=Lr)[0]
    assert runner.decoded_on["device"] == 1
    runner.close()
    counts = c_oracle.tally(reads, Lr)
    span = max_span(reads)

    def toks(p):
        a, b = window(reads, p, span)
        return orc.region_tokens(part(reads, a, b), p) if b > a else []
    has, ins = orc.list_inserts(counts, mincov, toks)
    assert has and len(ins) >= 3
    cons, _ = orc.build_consensus(mincov, counts.astype(np.int64), [dict(o) for o in orfs], True, ins, True)
    assert text == orc.fasta_text("S", mincov, cons)


def test_rebase_leaves_slots_without_a_token_alone():
    """tcmi_ins_entries_rebase moves the text offsets of long insertions only: a slot with key 0 (a read without a token on the
    column, whose other fields the kernel does not write) stays key 0 whatever its bits say; else the vote sees a phantom token."""
    e = np.zeros(3, entries_py.ENT)
    e["bits"] = 0x40
    e["key"][1] = (1 << 63) | ord("A") | (7 << 8) | (20 << 40)
    e["bits"][2] = 0x40 | 0x80
    e["key"][2] = (1 << 63) | ord("C")
    raw = e.copy()
    _ffi.check(_ffi.lib().tcmi_ins_entries_rebase(raw.ctypes.data_as(C.c_void_p), len(raw), 100))
    assert raw["key"][0] == 0 and raw["key"][2] == e["key"][2]
    assert raw["key"][1] == (1 << 63) | ord("A") | (107 << 8) | (20 << 40)
