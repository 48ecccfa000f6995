"""The device packer's record of itself without a GPU: csrc/pack_caps.h as a program of its own (tests/pack_caps_main.cpp), built plain and
under AddressSanitizer + UBSan.  Its flag values against the numbers the tests admit declines by; its capacities against what
tests/capacity_files.py restates, file by file, and against the literals tests/test_capacity_files.py pins; and each packer's arena
scratch summed against the same list taken from a counting stand-in for the arena.  Nothing is loaded into Python."""
import pytest

from tests import capacity_files as cf
from tests import device_file as dvf
from tests import host_program

BUILDS = ("plain", "sanitized")
SLOTS = (512, 2048)                             # resident workgroups of the tally kernel (an MI355X: 256 CUs, 4 a CU)
LONGEST = 8 * 400                               # readset_layout.h TCMI_F_LONGEST


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("pack_caps_main")
    src = ["tests/pack_caps_main.cpp"]
    return {"plain": host_program.build(src, d / "pack_caps_main", sanitize=False), "sanitized": host_program.build(src, d / "pack_caps_main_san")}


@pytest.fixture(scope="module")
def facts(tmp_path_factory):
    d = tmp_path_factory.mktemp("pack_caps_files")
    return {case: cf.facts(cf.write(d / (case + ".bam"), case)) for case in cf.CASES + ("long_only",)}


def ints(programs, build, *args):
    return [int(v) for v in host_program.run(programs[build], *args).stdout.split()]


def grid_of(rec_cap, slots, balance):
    """pk_pack's grid from a capacity, restated: at least the workgroups the reads-per-workgroup rule leaves for any count up to it"""
    full = -(-rec_cap // 1024)
    if not balance:
        return full + -(-rec_cap // 2048)
    return max(max(1, -(-rec_cap // (slots * LONGEST))) * slots, full)


# ---- the flags ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("build", BUILDS)
def test_flag_values_are_the_numbers_the_tests_hold(programs, build):
    out = host_program.run(programs[build], "flags").stdout.split()
    flags = dict(zip(out[0::2], map(int, out[1::2])))
    assert len(flags) == 12 and len(set(flags.values())) == 12 and all(v & (v - 1) == 0 for v in flags.values()), flags
    for name in ("PKF_EVENT_OVF", "PKF_CHUNK_OVF", "PKF_WORD_OVF", "PKF_REC_OVF"):
        assert flags[name] == getattr(cf, name), name
    assert flags["PKF_EVENT_OVF"] == dvf.PKF_EVENT_OVF
    assert (flags["PKF_REC_OVF"], flags["PKF_SLOT_OVF"]) == (0x800, 1 << 13)


# ---- the capacities ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("build", BUILDS)
def test_capacities_are_what_capacity_files_restates(programs, facts, build):
    for case, f in facts.items():
        len_bound = f["ref_len"] + 65536
        for hint in sorted({f["hint"], 0, 1703}):
            for safe in (0, 1):
                want = f["caps"](0 if safe else hint)
                for slots in SLOTS:
                    for balance in (0, 1):
                        rec, word, chunk, event, n_wg = ints(programs, build, "caps", f["inflated"], hint, safe, len_bound, slots, balance)
                        what = (case, hint, safe, slots, balance)
                        assert {"rec_cap": rec, "word_cap": word, "event_cap": event} == want, what
                        assert n_wg == grid_of(rec, slots, balance), what
                        assert chunk == min(rec, 4 * n_wg + len_bound // 128 + 64), what
        assert f["caps"](0)["rec_cap"] == f["safe_rec_cap"]


@pytest.mark.parametrize("build", BUILDS)
def test_capacities_are_the_literals_the_capacity_tests_pin(programs, facts, build):
    f = facts["wide_skips"]
    rec, word, _chunk, event, _n_wg = ints(programs, build, "caps", f["inflated"], f["hint"], 0, f["ref_len"] + 65536, 1024, 1)
    assert (rec, word, event) == (23212, 244929, 1 << 20)
    f = facts["hint_too_large"]
    assert ints(programs, build, "caps", f["inflated"], f["hint"], 0, f["ref_len"] + 65536, 1024, 1)[0] == 9804
    assert ints(programs, build, "caps", f["inflated"], f["hint"], 1, f["ref_len"] + 65536, 1024, 1)[0] == 35353
    assert ints(programs, build, "caps", f["inflated"], 35, 0, f["ref_len"] + 65536, 1024, 1)[0] == 35353         # (a record takes 36 bytes at least: no hint)
    assert ints(programs, build, "caps", f["inflated"], 36, 0, f["ref_len"] + 65536, 1024, 1)[0] == 35353 < f["inflated"] // 36 * 5 // 4 + 8192
    # d: every read of sparse_beyond_ref_len opens a chunk, and that is beyond the chunk capacity of every grid the file is written for
    f = facts["sparse_beyond_ref_len"]
    for slots in (256, 512, cf.SPARSE_MAX_SLOTS):
        chunk, n_wg = ints(programs, build, "caps", f["inflated"], f["hint"], 0, f["ref_len"] + 65536, slots, 1)[2::2]
        assert n_wg == slots and chunk == 4 * slots + 615 < cf.N_SPARSE, (slots, chunk, n_wg)


@pytest.mark.parametrize("build", BUILDS)
def test_totals_fit_up_to_the_capacity_and_not_one_beyond(programs, build):
    rec, word, chunk, event = 23212, 244929, 4711, 1 << 20
    fits = lambda *tot: ints(programs, build, "fits", rec, word, chunk, event, *tot)[0]
    assert fits(rec, word - 18, chunk, event) == 0 == fits(0, 0, 0, 0)
    assert fits(rec + 1, word - 18, chunk, event) == cf.PKF_REC_OVF
    assert fits(rec, word - 17, chunk, event) == cf.PKF_WORD_OVF        # (the zero pair in front and the last load's 16 words: 18)
    assert fits(rec, word - 18, chunk + 1, event) == cf.PKF_CHUNK_OVF
    assert fits(rec, word - 18, chunk, event + 1) == cf.PKF_EVENT_OVF
    assert fits(rec + 1, word, chunk + 1, event + 1) == cf.PKF_REC_OVF | cf.PKF_WORD_OVF | cf.PKF_CHUNK_OVF | cf.PKF_EVENT_OVF


@pytest.mark.parametrize("build", BUILDS)
def test_report_pin_offsets(programs, build):
    assert ints(programs, build, "pin", 0) == [256, 256, 256, 256, 512]             # (the several-kernel packer: totals, then the mate counters)
    assert ints(programs, build, "pin", 100) == [256, 256 + 1024, 256 + 1024 + 512, 256 + 1024 + 512 + 512, 256 + 1024 + 512 + 512 + 256]
    alg, end, stat, mate, size = ints(programs, build, "pin", 16384)
    assert (end - alg, stat - end, mate - stat, size - mate) == (16384 * 8, 16384 * 4, 16384 * 4, 256)


# ---- the arena scratch -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("start", (0, 256, 1000))
@pytest.mark.parametrize("build", BUILDS)
def test_scratch_summed_is_scratch_taken(programs, build, start):
    """records in {0, 1, 255, 256, 257, 65 537}, blocks in {1, 16 383, 16 384}, the mate rule on and off, the prefix kernels on and off,
    flat arrays and a stream; the several-kernel packer also with half and none of its records kept"""
    lines = host_program.run(programs[build], "scratch", start).stdout.strip().split("\n")
    assert lines[-1] == "ok %d" % (6 * 2 * 2 * 3 + 6 * 3 * 2 * 2) and len(lines) == 145, lines[-3:]
    seen = set()
    for ln in lines[:-1]:
        key, _, totals = ln.partition(" : ")
        summed, taken = map(int, totals.split())
        assert summed == taken >= start, ln
        seen.add(key)
    assert len(seen) == 144 - 12                # (half of no record and of one record is none of them)
    assert {"several 65537 1 1 65537", "several 0 0 0 0", "one_sync 65537 16384 1 1", "one_sync 0 1 0 0"} <= seen


def old_rest_bytes(n_rec, nb, mate):
    """what bam_device.hip reserved per record and per block before the lists: one formula for whichever packer came"""
    al = lambda b: (b + 255) & ~255
    slots = 1024
    while slots < 2 * (n_rec + 1):
        slots <<= 1
    mate_bytes = slots * 8 + 256 + al((n_rec + 1) * 4 + 4) + 3 * 256 if mate else 0
    return (mate_bytes + al(n_rec * 8 + 8) + al(n_rec * 4 + 4) * 12 + al((n_rec // 256 + 2) * 8) * 3 + al(nb * 33 + 64) + al(nb * 8) * 4 + al(nb * 4)
            + 8192 + 32 * 256)


@pytest.mark.parametrize("build", BUILDS)
def test_the_lists_reserve_no_more_than_the_old_bound(programs, build):
    """the hand-counted bound they replace held for every branch: the larger list stays below it, and each says what it takes a record"""
    for n_rec in (1040, 14775, 35353, 1_000_000, 6_250_000):
        for nb in (1, 40, 16383, 16384, 67000):
            for mate in (0, 1):
                for option in (-1, 0, 1):
                    several, one = ints(programs, build, "rest", n_rec, nb, mate, option)
                    assert max(several, one) <= old_rest_bytes(n_rec, nb, mate), (n_rec, nb, mate, option, several, one)
    # bytes a record and a block: the slope of the sums (far from the mate table's doubling; blocks by 32: no alignment step in between)
    per = lambda k, n, nb, option: ints(programs, build, "rest", n, nb, 0, option)[k]
    assert per(1, 2 << 20, 64, -1) - per(1, 1 << 20, 64, -1) == 52 << 20
    assert per(0, 2 << 20, 64, -1) - per(0, 1 << 20, 64, -1) == (52 << 20) + 20 * ((1 << 20) // 256)
    assert per(1, 1000, 16384 + 3200, -1) - per(1, 1000, 16384, -1) == 32 * 3200
    assert per(1, 1000, 16384 + 3200, 0) - per(1, 1000, 16384, 0) == 56 * 3200
