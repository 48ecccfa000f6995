"""The mate join's table (csrc/mate_join.hip) and the duplicate rule's (csrc/dedup.hip) on keys that collide: the files of
tests/join_keys.py — two keys of one tag and one home slot that only the compare of the full key tells apart (names of two lengths, names
that differ in their first dword, one name at two places, names of 253 and 254 bytes; two pair keys, a fragment key and a pair key), a
chain of more than 80 strangers from the table's last slot round to slot 0, groups split by strangers, a group of five of which the build
enters three — through both packers, every count exact against the yardsticks (tests/mate_overlap_yardstick.py,
tests/dedup_yardstick.py).  What is claimed for the keys is proved without a device in tests/test_join_keys.py."""
import contextlib

import numpy as np
import pytest

from tests import dedup_yardstick as dy
from tests import device_file as dvf
from tests import join_keys as jk
from tests import mate_overlap_yardstick as my
from trueconsense_amd import engine

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    with engine.Context(0) as c:
        yield c


@pytest.fixture(scope="module")
def store(tmp_path_factory):
    """the module's directory; the files written once, the yardsticks computed once"""
    return {"dir": tmp_path_factory.mktemp("join_collisions")}


def once(store, key, make):
    if key not in store:
        store[key] = make()
    return store[key]


def data(store, key):
    """-> (path, arrays, reference length) of a case of join_keys"""
    def make():
        c = jk.case(key)
        return jk.write(store["dir"] / (key + ".bam"), c["specs"], c["L"]), jk.arrays(c["specs"]), c["L"]
    return once(store, ("data", key), make)


def yard(store, key, mate, dedup):
    """the mate rule alone: mate_overlap_yardstick.counts; with the duplicate rule: dedup_yardstick.counts (the join's counters are its
    "counters", zeros with the mate rule off)"""
    _, rd, L = data(store, key)
    return once(store, ("yard", key, mate, dedup), lambda: dy.counts(rd, L, mate=mate) if dedup else my.counts(rd, L))


@contextlib.contextmanager
def uploaded(ctx, path, how, mate, dedup):
    """the file under the rules, which are on for the upload alone"""
    ctx.set_mate_overlap(mate)
    ctx.set_dedup(dedup)
    try:
        with dvf.uploaded(ctx, path, how=how) as rs:
            ctx.set_mate_overlap(False)
            ctx.set_dedup(False)
            yield rs
    finally:
        ctx.set_mate_overlap(False)
        ctx.set_dedup(False)


def check(ctx, rs, y, mate, dedup):
    """the matrix, the rules' counters, n_piled and max_end, and — under the duplicate rule — the verdict of every record: all exact"""
    got = ctx.step(rs, len(y["counts"]), 0, True)[3]
    bad = np.argwhere(got != y["counts"])
    assert len(bad) == 0, (len(bad), bad[:6].tolist(), got[tuple(bad[:6].T)].tolist(), y["counts"][tuple(bad[:6].T)].tolist())
    assert rs.mate_overlap == dict(y["counters"], on=int(mate)), (rs.mate_overlap, y["counters"])
    assert (rs.n_piled, rs.max_end, rs.primer_masked_reads) == (y["n_piled"], y["max_end"], y["n_masked"])
    if dedup:
        assert rs.dedup == dict(y["dedup_counters"], on=1), (rs.dedup, y["dedup_counters"])
        dup = rs.duplicates()
        assert dup.dtype == bool and np.array_equal(dup, y["dup"]), np.flatnonzero(dup != y["dup"])[:10].tolist()


def run(ctx, store, key, how, mate, dedup, times=1):
    path, _, _ = data(store, key)
    y = yard(store, key, mate, dedup)
    for _ in range(times):
        with uploaded(ctx, path, how, mate, dedup) as rs:
            assert rs.route == how
            check(ctx, rs, y, mate, dedup)
    return y


# ---- the mate join ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", dvf.PACKERS)
@pytest.mark.parametrize("key", [k for k in jk.MATE_CASES if k.startswith("m1_")])
def test_m1_colliding_names_are_two_pairs(ctx, store, key, how):
    """the same integers, one tag, one home slot: same_name alone decides (tests/test_join_keys.py: forced equal, four ambiguous records)"""
    y = run(ctx, store, key, how, True, False)
    assert y["counters"] == {"pairs": 2, "clipped_reads": 2, "clipped_columns": 60, "ambiguous": 0}


@pytest.mark.parametrize("how", dvf.PACKERS)
def test_m2_one_name_at_colliding_places_is_two_pairs(ctx, store, how):
    """one name, one tag, one home slot: tcmi_mate_same_ints alone decides.  The places lie below 2^19: a matrix of 15 MB"""
    y = run(ctx, store, "m2", how, True, False)
    assert y["counters"] == {"pairs": 2, "clipped_reads": 2, "clipped_columns": 40, "ambiguous": 0}


@pytest.mark.parametrize("how", dvf.PACKERS)
def test_m3_a_chain_of_strangers_round_the_tables_end(ctx, store, how):
    y = run(ctx, store, "m3", how, True, False)
    assert y["counters"]["pairs"] == jk.M3_PAIRS and y["counters"]["ambiguous"] == 0


@pytest.mark.parametrize("how", dvf.PACKERS)
def test_m4_groups_split_by_strangers_every_time(ctx, store, how):
    """the build's order is not fixed: three uploads, each equal to the yardstick — so equal to each other"""
    y = run(ctx, store, "m4", how, True, False, times=3)
    assert y["counters"]["pairs"] == jk.M3_PAIRS + 2 and y["counters"]["ambiguous"] == 3 + 5


@pytest.mark.parametrize("how", dvf.PACKERS)
def test_m5_name_lengths_at_the_edges(ctx, store, how):
    y = run(ctx, store, "m5", how, True, False)
    assert y["counters"]["pairs"] == len(jk.M5_NAMES) + 4 and y["counters"]["ambiguous"] == 0


@pytest.mark.parametrize("how", dvf.PACKERS)
def test_m6_the_cluster_under_both_rules(ctx, store, how):
    """mate_idx feeds the duplicate rule: M4's file under --dedup --mate-overlap, and under --dedup alone (the join runs for mate_idx only)"""
    y = run(ctx, store, "m4", how, True, True)
    assert y["counters"]["ambiguous"] == 8 and y["dedup_counters"]["duplicate_templates"] >= jk.M3_PAIRS
    run(ctx, store, "m4", how, False, True)


# ---- the duplicate rule --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", dvf.PACKERS)
@pytest.mark.parametrize("key", jk.DUP_CASES)
def test_colliding_template_keys_are_two_sets(ctx, store, key, how):
    """D1: two pair keys of one tag and one home slot, the better template of each survives; D2: inside a cluster of 44 stranger keys
    round the table's end, a wavefront's lanes on dozens of slots; D3: a fragment key and a pair key; D4: equal scores, each key's own
    lowest leader survives.  tcmi_dup_key_same alone decides (tests/test_join_keys.py: forced equal, one set and three duplicates)"""
    y = run(ctx, store, key, how, False, True)
    c = y["dedup_counters"]
    if key in ("d1", "d3", "d4"):
        assert (c["duplicate_sets"], c["duplicate_templates"]) == (2, 2)
    else:
        assert (c["duplicate_sets"], c["duplicate_templates"]) == (13, 13)


@pytest.mark.parametrize("how", dvf.PACKERS)
def test_d2_under_both_rules(ctx, store, how):
    run(ctx, store, "d2", how, True, True)
