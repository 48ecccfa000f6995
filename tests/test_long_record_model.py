"""CPU: the record chain where records cover dozens of BGZF blocks — the host rule (csrc/bgzf_host.cpp: tcmi_bam_chain_check, run by
tests/bgzf_host_main.cpp's `chainfile` mode under AddressSanitizer + UBSan) and the joining rule of block ranges
(distributed.check_range_anchors) against the plain model of tests/long_records.py, on the three files the device tests decode
(tests/test_long_record_chain.py): 512-byte blocks filled to the brim, 512-byte blocks cut as htslib cuts them, 1024-byte blocks
filled to the brim — four records of 9 000 .. 49 999 bases among 6 500 short ones."""
import numpy as np
import pytest

from tests import host_program
from tests import long_records as lr
from trueconsense_amd.distributed import check_range_anchors

E_UNSUPPORTED = -9
KINDS = ((512, True), (512, False), (1024, True))


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("long_records")
    return [lr.Model(lr.build(tmp, block, split)[0]) for block, split in KINDS]


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    return host_program.build(["tests/bgzf_host_main.cpp", "trueconsense_amd/csrc/bgzf_host.cpp"], tmp_path_factory.mktemp("bgzf_host") / "bgzf_host_main", libs=["-lz"])


def test_the_files_reach_the_paths_the_device_tests_are_about(models, tmp_path):
    lr.check_conditions(*models)
    # the variant whose long records start in a block's last three bytes: the size field straddles the block's end, and a record in
    # front starts in the same block (the block's search cannot see a start with fewer than four bytes: the chain arrives there)
    path, _, _, _, which = lr.build(tmp_path, 512, True, tail=True)
    m = lr.Model(path)
    for i in which:
        s, _ = m.touched(i)
        assert m.rec[i] - m.start[s] == 509 and m.first[s] < 509 and m.lo[s + 1] - 1 == i
    assert m.n_blocks > 2048 and not lr.false_finds(m)


def test_the_models_ranges_partition_the_file_and_their_anchors_meet(models):
    """every record starts in exactly one range of a cut list; a range's first record starts where the nearest range in front that
    holds a record ends its last one; the first range's records start where the header ends and the last range's end with the stream"""
    for m in models:
        se = [m.touched(i) for i in m.long_records()]
        lists = lr.cut_lists(m, n_random=200)
        inside = refused = 0
        for cuts in lists:
            ranges = m.cut(cuts)
            at, expect = 0, None
            for r in ranges:
                i0, i1 = r["records"]
                assert i0 == at and i1 >= i0
                at = i1
                if i1 == i0:
                    assert (r["range_first"], r["range_next"], r["refused"]) == (-1, -1, False)
                    inside += any(s < r["first_block"] and r["first_block"] + r["n_own"] - 1 < e for s, e in se)
                    continue
                assert r["range_first"] == (-1 if i0 == 0 else expect if expect is not None else r["range_first"])
                assert (r["range_first"] >= 0) == (i0 > 0) and m.rec[i0] == (r["range_first"] if i0 else m.rec[0])
                expect = r["range_next"]
                refused += r["refused"]
            assert at == len(m.rec) and expect == m.inflated
        assert inside >= 5 and refused >= 5, (inside, refused)


def test_host_rule_gives_the_models_verdict_and_anchors_for_every_window(models, prog, tmp_path):
    """tcmi_bam_chain_check over the model's block table, from EVERY first block with a set of lengths each: the refusal "a record
    longer than a BGZF block at the end of a block range" (at the block taken along) exactly where the model says the last record
    overruns that block, else no refusal and the model's anchors."""
    for k, m in enumerate(models):
        windows = lr.sweep_windows(m)
        table = tmp_path / ("table%d.txt" % k)
        table.write_text(m.table_text(windows))
        lines = host_program.run(prog, "chainfile", table).stdout.split("\n")
        assert lines[-1] == "" and len(lines) - 1 == len(windows) >= 5 * m.n_blocks
        n_refused = n_inside = n_mid = 0
        for (fb, own, nb, ranged), line in zip(windows, lines):
            code, block, first, nxt, what = line.split(" ", 4)
            r = m.range(fb, own)
            assert r["n"] == nb
            if r["refused"]:
                assert (int(code), int(block)) == (E_UNSUPPORTED, own) and lr.E_UNSUPPORTED_WORDS in what, (fb, own, line)
                n_refused += 1
                continue
            base = int(m.start[fb])
            want = tuple(x - base if x >= 0 else -1 for x in (r["range_first"], r["range_next"]))
            assert (int(code), int(first), int(nxt)) == (0,) + want and what == "", (fb, own, line, want)
            n_inside += r["records"][0] == r["records"][1] and m.entry[fb] == -2
            n_mid += r["range_first"] >= 0 and m.first[fb] == lr.NONE
        assert n_refused > 100 and n_inside > 100 and n_mid > 100, (n_refused, n_inside, n_mid)


def test_range_anchors_of_the_model_join_and_one_moved_byte_does_not(models):
    """check_range_anchors over the model's anchors: None for every cut list — cuts inside long records and ranges wholly inside one
    included —, and the same table with one anchor moved by one byte is refused."""
    rng = np.random.default_rng(11)
    for m in models:
        clean = 0
        for cuts in lr.cut_lists(m, n_random=100):
            ranges = m.cut(cuts)
            table = m.anchors(ranges)
            assert check_range_anchors(table, m.inflated) is None, (cuts, table)
            clean += not any(r["refused"] for r in ranges)
            movable = [(k, j) for k, t in enumerate(table) for j in (2, 3) if t[j] >= 0]
            k, j = movable[int(rng.integers(0, len(movable)))]
            moved = list(table)
            moved[k] = tuple(x + (1 if i == j else 0) for i, x in enumerate(table[k]))
            assert check_range_anchors(moved, m.inflated) is not None, (cuts, table, k, j)
        assert clean >= 4


def test_the_restated_decode_takes_the_files_and_refuses_a_planted_head(models, tmp_path):
    """long_records.predict — every block's own search (bgzf_copy's plausibility test), its chain of size fields, rec_vouch's
    withdrawal and the host rule, in Python — on the files the device tests decode: the three recipes decode; of eight files with
    arbitrary bytes in their long records at least half do (the device test holds the device to this verdict, seed by seed); a whole
    plausible head planted in the body of a block inside a record is refused at that block, the four-byte one in a block's tail is
    withdrawn."""
    for m in models:
        assert lr.predict(m) is None
    verdicts = [lr.predict(lr.Model(lr.build_arbitrary(tmp_path, seed)[0])) for seed in range(8)]
    assert sum(v is None for v in verdicts) >= 4, verdicts
    specs, which = lr.make_specs()
    path = str(tmp_path / "planted.bam")
    pick = lambda inside: next(b for b in inside if b > 1024)
    _, b = lr.plant(path, specs, which[2], lr.record_head(2000), 100, pick, "r", lr.REF_LEN)
    m = lr.Model(path)
    assert lr.predict(m) == "the chain does not close at block %d (found 100, expected %d)" % (b, _expected(m, b))
    specs, which = lr.make_specs()
    _, b = lr.plant(path, specs, which[2], b"\x40\0\0\0", -4, pick, "r", lr.REF_LEN)
    m = lr.Model(path)
    assert m.first[b] == lr.NONE and lr.block_search(m, b) != lr.NONE and lr.predict(m) is None


def _expected(m, b):
    """bytes of the record that covers block b that lie behind the block's start"""
    i = int(np.searchsorted(m.rec, m.start[b], "right")) - 1
    return int(m.end[i] - m.start[b])
