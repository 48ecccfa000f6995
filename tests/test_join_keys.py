"""The colliding keys of tests/join_keys.py without a GPU: what is claimed for every committed key set — keys different, tags equal,
home slots under both packers' tables, who lands before whom in a chain — from the hashes that the rule programs print
(tests/mate_rule_main.cpp, tests/dedup_rule_main.cpp: the shared headers' text, built under AddressSanitizer + UBSan), the numpy
restatements held against those, and the yardsticks on every file with the condition that makes the file worth running: the yardstick
with the colliding keys forced equal gives other counters and another matrix, or the chain is as long as claimed and wraps under both
table sizes.  The kernels on the same files: tests/test_join_collisions.py."""
import numpy as np
import pytest

from tests import dedup_yardstick as dy
from tests import host_program
from tests import join_keys as jk
from tests import mate_overlap_yardstick as my

SIZES = (1024, 1 << jk.BITS)                                        # the several-kernel packer's table, and the largest the one-sync packer's gets


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("join_keys")
    return {"dir": d, "mate": host_program.build(["tests/mate_rule_main.cpp"], d / "mate_rule_main"),
            "dup": host_program.build(["tests/dedup_rule_main.cpp"], d / "dedup_rule_main")}


def run_program(programs, which, lines, n):
    inp, out = str(programs["dir"] / "r.in"), str(programs["dir"] / "r.out")
    with open(inp, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    r = host_program.run(programs[which], inp, out)
    assert r.stdout.strip() == "ok %d" % n, (r.stdout[-500:], r.stderr[-2000:])
    got = [ln.split() for ln in open(out).read().split("\n") if ln]
    assert len(got) == n
    return got


def mate_hashes(programs, rd):
    """-> per record: the join's hash as csrc/mate_rule.h computes it (every record of these files is eligible)"""
    got = run_program(programs, "mate", jk.mate_program_lines(rd), int(rd["n_reads"]))
    assert all(g[0] == "1" for g in got)
    return [int(g[1], 16) for g in got]


def dup_keys(programs, rd):
    """-> {leader: (the twelve key bytes, the hash)} as csrc/dedup_rule.h computes them, the join's pairs the yardstick's"""
    v = dy.verdicts(rd)
    got = run_program(programs, "dup", jk.dup_program_lines(rd, v["mate"]), int(rd["n_reads"]))
    out = {i: (bytes.fromhex(g[4]), int(g[5], 16)) for i, g in enumerate(got) if g[4] != "-"}
    assert sorted(out) == sorted(t[1] for ts in v["templates"].values() for t in ts)
    return out, v


def key_of(rd, i):
    flag, tid, pos, ntid, npos = my.fields(rd, i)
    return my.name(rd, i), tid, min(pos, npos), max(pos, npos)


def records_named(rd, name):
    return [i for i in range(int(rd["n_reads"])) if my.name(rd, i) == name]


def collides(ha, hb):
    """equal tags, and one home slot under both table sizes"""
    return ha >> 32 == hb >> 32 and all(ha & (s - 1) == hb & (s - 1) for s in SIZES)


# ---- the files and their tables -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", jk.MATE_CASES + jk.DUP_CASES)
def test_tables_of_every_file(tmp_path, key):
    """at most 512 records and 64 KiB: 1024 slots from the several-kernel packer, at most 1 << BITS from the one-sync packer"""
    c = jk.case(key)
    path = jk.write(tmp_path / "a.bam", c["specs"], c["L"])
    slots = jk.table_slots(path)
    assert len(c["specs"]) <= jk.MOST_RECORDS and jk.cf.facts(path)["inflated"] <= jk.MOST_INFLATED
    assert slots["several_kernels"] == SIZES[0] and SIZES[0] <= slots["one_sync"] <= SIZES[1], slots
    assert jk.mate_slots(512) == 1024 and jk.mate_slots(513) == 2048 and jk.mate_slots(0) == 1024 and jk.mate_slots(2048) == 4096


@pytest.mark.parametrize("key", jk.MATE_CASES)
def test_numpy_join_hash_equals_the_program(programs, key):
    rd = jk.arrays(jk.mate_case(key)["specs"])
    for i, h in enumerate(mate_hashes(programs, rd)):
        name, tid, lo, hi = key_of(rd, i)
        assert int(jk.mate_hash(name, tid, lo, hi)) == h, i
        assert int(jk.tag(h)) == h >> 32 and all(int(jk.home(h, s)) == h & (s - 1) for s in SIZES)


@pytest.mark.parametrize("key", jk.DUP_CASES + ("m4",))
def test_numpy_duplicate_hash_equals_the_program(programs, key):
    rd = jk.arrays(jk.case(key)["specs"])
    keys, v = dup_keys(programs, rd)
    for k, ts in v["templates"].items():
        words = jk.pair_key(k[1], k[2], k[3]) if k[0] == "P" else jk.fragment_key(k[1], k[2])
        for _, leader, _ in ts:
            kb, h = keys[leader]
            assert kb == dy.key_bytes(k) == b"".join(int(w).to_bytes(4, "little") for w in words), (leader, k)
            assert int(jk.dup_hash(*words)) == h, (leader, k)


def test_the_searches_find_what_is_committed_on_a_small_budget():
    """the search functions on budgets of a second: the cheap ones give the constants back, the dear ones run and find colliding keys
    of a weaker kind (fewer bits) — the functions are alive; `python -m tests.join_keys` spends the real budgets"""
    assert tuple(jk.search_homes(4, 1 << 18, 10, jk.M3_INTS, 48)) == jk.M3_NAMES
    assert tuple(jk.search_fragment_homes(9, 1 << 18, jk.FRAG_POS, 1 << 20, 48)) == jk.D_STRANGERS
    for a, b in jk.search_names(1, 1 << 16, (9, 10), jk.M1_INTS) + jk.search_tail3(10, 94 ** 3, jk.M1_INTS)[1]:
        assert a != b and int(jk.collide(jk.mate_hash(a, *jk.M1_INTS))) == int(jk.collide(jk.mate_hash(b, *jk.M1_INTS)))
    for a, b in jk.search_places(3, 1 << 16, jk.M2_NAME, 1 << 19, 1 << 11) + jk.search_pair_keys(7, 1 << 16, jk.A_FROM, jk.B_FROM, jk.D_WIDTH):
        assert a != b
    assert jk.search_fragment_keys(8, 1 << 16, 1 << 28, (jk.A_FROM, jk.B_FROM, 65535)) == []


# ---- M1, M2, M5: one compare of the full key tells two pairs apart -----------------------------------------------------------------------------
def two_pairs_not_one_group(c, n_pairs=2, clipped=2):
    """the yardstick on the file: `n_pairs` pairs, nothing ambiguous; on the control — the colliding keys forced equal — their four
    records are one ambiguous group, and the matrix is another"""
    rd, ctl = jk.arrays(c["specs"]), jk.arrays(c["control"])
    y, yc = my.counts(rd, c["L"]), my.counts(ctl, c["L"])
    assert y["counters"]["pairs"] == n_pairs and y["counters"]["ambiguous"] == 0 and y["counters"]["clipped_reads"] >= clipped, y["counters"]
    assert yc["counters"]["ambiguous"] == 4 and yc["counters"]["pairs"] == n_pairs - 2, yc["counters"]
    assert y["counts"].shape != yc["counts"].shape or not np.array_equal(y["counts"], yc["counts"])
    return rd, y


@pytest.mark.parametrize("variant", [k for k, v in jk.M1.items() if v])
def test_m1_names_collide_under_the_same_integers(programs, variant):
    c = jk.mate_case("m1_" + variant)
    rd, y = two_pairs_not_one_group(c)
    h = mate_hashes(programs, rd)
    a, b = c["names"]
    ia, ib = records_named(rd, a), records_named(rd, b)
    assert a != b and len(ia) == len(ib) == 2
    assert len({key_of(rd, i)[1:] for i in ia + ib}) == 1 and key_of(rd, ia[0])[1:] == c["ints"]      # the same integers: the name alone decides
    assert h[ia[0]] == h[ia[1]] != h[ib[0]] == h[ib[1]] and collides(h[ia[0]], h[ib[0]])
    if variant == "lengths":
        assert len(a) != len(b)
    if variant == "dword":
        assert len(a) == len(b) and a[:4] != b[:4]
    if variant == "tail3":
        assert len(a) == len(b) and len(a) % 4 == 3 and a[:-3] == b[:-3]
    # each pair's loser is clipped by the overlap
    assert sorted(y["clip"]) == [0, 0, 30, 30]


def test_m1_tail3_was_not_found():
    """the one required variant that the search's budget did not give (tests/join_keys.py says why a larger one would not either)"""
    assert jk.M1["tail3"] is None and "m1_tail3" not in jk.MATE_CASES


def test_same_name_on_every_length_and_differing_byte(programs):
    """... so the compare the kernels compile (csrc/mate_rule.h tcmi_mate_same_name) runs here, under both sanitizers: every name length
    1 .. 12 x every byte position x three ways to differ, equal names over different bytes behind them, names of n and n + 1 bytes —
    the whole dwords and the masked tails of one, two and three bytes"""
    r = host_program.run(programs["mate"], "--names")
    assert r.stdout.strip() == "names ok 1512", (r.stdout[-500:], r.stderr[-2000:])
    text = open(jk.__file__.replace("tests/join_keys.py", "trueconsense_amd/csrc/mate_join.hip")).read()
    assert "tcmi_mate_same_name(a.n_name, b.n_name" in text                     # (the kernels call that text, they hold no compare of their own)


def test_m2_places_collide_under_one_name(programs):
    c = jk.mate_case("m2")
    rd, y = two_pairs_not_one_group(c)
    h = mate_hashes(programs, rd)
    keys = [key_of(rd, i) for i in range(4)]
    assert {k[0] for k in keys} == {jk.M2_NAME} and len(set(keys)) == 2 and {k[2:] for k in keys} == set(jk.M2_PLACES)
    (ha, hb) = sorted(set(h))
    assert collides(ha, hb)
    assert sorted(y["clip"]) == [0, 0, 20, 20] and max(k[3] for k in keys) + 2048 < c["L"] == jk.M2_L


def test_m5_name_lengths_at_the_edges(programs):
    c = jk.mate_case("m5")
    n_pairs = len(jk.M5_NAMES) + 4
    rd, y = two_pairs_not_one_group(c, n_pairs, n_pairs)
    assert [len(n) for n in jk.M5_NAMES] == [1, 2, 3, 4, 5, 7, 8, 253, 254]
    a, b = jk.M5_LAST_BYTE
    assert len(a) == len(b) == 254 and a[:-1] == b[:-1] and a[-1] != b[-1]
    assert key_of(rd, records_named(rd, a)[0])[1:] == key_of(rd, records_named(rd, b)[0])[1:]
    for name in jk.M5_NAMES + jk.M5_LAST_BYTE + jk.M5_EDGE:         # every name's two records are a pair
        lo = [i for i in records_named(rd, name) if y["clip"][i] > 0]
        assert len(records_named(rd, name)) == 2 and len(lo) == 1, name
    # the two names of 253 and 254 bytes collide under one set of integers: the length check alone tells them apart
    h = mate_hashes(programs, rd)
    a, b = c["names"]
    ia, ib = records_named(rd, a), records_named(rd, b)
    assert (len(a), len(b)) == (253, 254) and key_of(rd, ia[0])[1:] == key_of(rd, ib[0])[1:] == c["ints"]
    assert h[ia[0]] != h[ib[0]] and collides(h[ia[0]], h[ib[0]])


# ---- M3, M4, M6: a chain of strangers on the table's last slots --------------------------------------------------------------------------------
def cluster_layouts(h, keys, n_chain):
    """the build's table for every order and both sizes -> [(what, table)]; the chain from the last slot holds n_chain entries at
    least and runs round to slot 0"""
    out = []
    for slots in SIZES:
        for what, (order, lockstep) in jk.orders(len(h)).items():
            table = jk.mate_table(h, keys, slots, order, lockstep)
            chain = jk.chain_from(table, slots - 1)
            assert len(chain) >= n_chain and table[0] >= 0 and table[slots - 2] < 0, (slots, what, len(chain))
            assert sum(1 for t in table if t >= 0) == len(chain)    # (the file's entries are this one chain)
            out.append(((slots, what), table, chain))
    return out


def test_m3_strangers_share_the_last_slot(programs):
    c = jk.mate_case("m3")
    rd = jk.arrays(c["specs"])
    h = mate_hashes(programs, rd)
    keys = [key_of(rd, i) for i in range(len(h))]
    assert len(set(keys)) == jk.M3_PAIRS >= 40 and len({x >> 32 for x in h}) == jk.M3_PAIRS            # strangers: every key a tag of its own
    assert all(x & (s - 1) == s - 1 for x in h for s in SIZES)                                         # ... and the last slot for its home
    for what, table, chain in cluster_layouts(h, keys, 2 * jk.M3_PAIRS):
        assert sorted(chain) == list(range(len(h))), what
    y = my.counts(rd, c["L"])
    assert y["counters"] == {"pairs": jk.M3_PAIRS, "clipped_reads": jk.M3_PAIRS, "clipped_columns": 10 * jk.M3_PAIRS, "ambiguous": 0}


def test_m4_groups_split_by_strangers(programs):
    c = jk.mate_case("m4")
    rd = jk.arrays(c["specs"])
    h = mate_hashes(programs, rd)
    keys = [key_of(rd, i) for i in range(len(h))]
    a, b = c["pair"]
    ia, ib, i3, i5 = (records_named(rd, n) for n in (a, b, c["three"], c["five"]))
    assert (len(ia), len(ib), len(i3), len(i5)) == (2, 2, 3, 5) and all(len({keys[i] for i in g}) == 1 for g in (ia, ib, i3, i5))
    # the colliding pair: one set of integers, the cluster's; a home inside the cluster under both sizes
    assert a != b and keys[ia[0]][1:] == keys[ib[0]][1:] == jk.M3_INTS and h[ia[0]] != h[ib[0]] and collides(h[ia[0]], h[ib[0]])
    assert bool(jk.near(h[ia[0]])) and all(h[ia[0]] & (s - 1) in [s - 1] + list(range(jk.NEAR_FIRST)) for s in SIZES)
    assert all(h[i] & (s - 1) == s - 1 for i in i3 + i5 for s in SIZES)
    for what, table, chain in cluster_layouts(h, keys, 2 * jk.M3_PAIRS + 4 + 3 + 3):
        at = {r: k for k, r in enumerate(chain)}
        assert len([i for i in i5 if i in at]) == 3 and len(chain) == len(h) - 2, what              # the build enters three of the five
        assert all(i in at for i in ia + ib + i3), what
        # members of one group with foreign entries between them: most groups, and — in the file's own order — the group of three, the
        # five and both colliding pairs
        groups = {}
        for r in chain:
            groups.setdefault(keys[r], []).append(at[r])
        split = {k for k, where in groups.items() if max(where) - min(where) >= len(where)}
        assert len(split) >= 30, (what, len(split))
        if what[1] in ("file", "lockstep"):
            assert {keys[ia[0]], keys[ib[0]], keys[i3[0]], keys[i5[0]]} <= split, what
    y = my.counts(rd, c["L"])
    assert y["counters"]["pairs"] == jk.M3_PAIRS + 2 and y["counters"]["ambiguous"] == 8 and set(i3 + i5) == {i for i, k in y["classes"].items() if k == "ambiguous"}
    yc = my.counts(jk.arrays(c["control"]), c["L"])
    assert yc["counters"]["pairs"] == jk.M3_PAIRS and yc["counters"]["ambiguous"] == 12 and not np.array_equal(y["counts"], yc["counts"])


def test_m6_the_same_file_under_both_rules(programs):
    """M4's records are, to the duplicate rule, pairs of one key and the fragments that the ambiguous groups fall into: the rule marks
    most of the file, and the matrix is neither the mate rule's nor the plain one"""
    c = jk.mate_case("m4")
    rd = jk.arrays(c["specs"])
    y = dy.counts(rd, c["L"], mate=True)
    assert y["counters"]["ambiguous"] == 8 and y["dedup_counters"]["templates"] == jk.M3_PAIRS + 2 + 8
    assert y["dedup_counters"]["duplicate_templates"] >= jk.M3_PAIRS and y["dedup_counters"]["duplicate_sets"] >= 2
    assert not np.array_equal(y["counts"], my.counts(rd, c["L"])["counts"])
    assert not np.array_equal(y["counts"], dy.counts(rd, c["L"], mate=False)["counts"])


# ---- D1, D2, D3, D4: one compare of the full key tells two templates' keys apart ------------------------------------------------------------------
def merged(v, keys):
    """the verdicts a table that trusted the tag would give: the templates of `keys` as one set -> (dup, duplicate sets, duplicate templates)"""
    dup = v["dup"].copy()
    ts = [t for k in keys for t in v["templates"][k]]
    best = max(ts, key=lambda t: (t[0], -t[1]))
    for t in ts:
        for i in t[2]:
            dup[i] = t is not best
    return dup


def colliding_templates(programs, c):
    """-> (arrays, verdicts, the two colliding keys as the yardstick names them, A first): their bytes differ, their hashes collide"""
    rd = jk.arrays(c["specs"])
    keys, v = dup_keys(programs, rd)
    by_bytes = {}
    for leader, (kb, h) in keys.items():
        by_bytes.setdefault(kb, set()).add(h)
    # (a case names its keys by the ends of an FR pair, or by the key words themselves)
    words = [jk.pair_key(0, (k[0], 0), (k[1], 1)) if len(k) == 2 else k for k in c["keys"]]
    want = [b"".join(int(w & 0xFFFFFFFF).to_bytes(4, "little") for w in ws) for ws in words]
    assert want[0] != want[1] and all(len(by_bytes[w]) == 1 for w in want)
    ha, hb = (next(iter(by_bytes[w])) for w in want)
    assert ha != hb and collides(ha, hb)
    names = [next(k for k in v["templates"] if dy.key_bytes(k) == w) for w in want]
    return rd, v, names, (ha, hb)


@pytest.mark.parametrize("key", ("d1", "d4"))
def test_d1_d4_pair_keys_collide(programs, key):
    c = jk.dup_case(key)
    rd, v, (ka, kb), (ha, _) = colliding_templates(programs, c)
    assert ka[0] == kb[0] == "P" and bool(jk.near(ha))
    assert v["counters"] == {"templates": 4, "duplicate_templates": 2, "duplicate_records": 4, "duplicate_sets": 2}
    leaders = {k: sorted(t[1] for t in v["templates"][k]) for k in (ka, kb)}
    scores = {t[1]: t[0] for k in (ka, kb) for t in v["templates"][k]}
    assert sorted(leaders[ka] + leaders[kb]) == [0, 1, 2, 3] and [("A" if i in leaders[ka] else "B") for i in range(4)] == list(c["order"])
    if key == "d1":                                                 # different scores: the better template of EACH key survives
        assert {v["winner"][ka], v["winner"][kb]} == {1, 2} and scores[1] > scores[0] and scores[2] > scores[3] and scores[2] > scores[1]
    else:                                                           # equal scores: each key's own lowest leader, not the other key's lower one
        assert len(set(scores.values())) == 1 and (v["winner"][kb], v["winner"][ka]) == (0, 1) and leaders[ka] == [1, 2]
    # a table that trusted the tag: one set, three duplicates — as the yardstick on the control, whose keys ARE equal
    assert int(merged(v, (ka, kb)).sum()) == 6 and not np.array_equal(merged(v, (ka, kb)), v["dup"])
    y, yc = dy.counts(rd, c["L"]), dy.counts(jk.arrays(c["control"]), c["L"])
    assert yc["dedup_counters"] == {"templates": 4, "duplicate_templates": 3, "duplicate_records": 6, "duplicate_sets": 1}
    assert np.array_equal(yc["dup"], merged(v, (ka, kb))) and not np.array_equal(y["counts"], yc["counts"])


def test_d2_colliding_keys_inside_a_cluster(programs):
    c = jk.dup_case("d2")
    rd, v, (ka, kb), _ = colliding_templates(programs, c)
    keys, _ = dup_keys(programs, rd)
    strangers = [k for k in v["templates"] if k[0] == "F"]
    hs = {k: keys[v["templates"][k][0][1]][1] for k in v["templates"]}
    assert len(strangers) == jk.D_N_STRANGERS >= 40 and len({hs[k] >> 32 for k in strangers}) == len(strangers)
    assert all(hs[k] & (s - 1) == s - 1 for k in strangers for s in SIZES)
    assert sum(len(v["templates"][k]) == 2 for k in strangers) == 11
    leaders = sorted(keys)
    ident = {i: kb_ for i, (kb_, _) in keys.items()}
    for slots in SIZES:
        for what, (order, lockstep) in jk.orders(len(leaders)).items():
            table, slot_of = jk.dup_table({i: keys[i][1] for i in leaders}, ident, slots, [leaders[k] for k in order], lockstep)
            chain = jk.chain_from(table, slots - 1)
            assert len(chain) == len(strangers) + 2 and table[0] >= 0, (slots, what)                # one slot per key, round the table's end
            sa, sb = (slot_of[v["templates"][k][0][1]] for k in (ka, kb))
            assert sa != sb and {sa, sb} <= {(slots - 1 + k) & (slots - 1) for k in range(len(chain))}, (slots, what)
            # a wavefront's lanes hold several distinct slots, and some of them twice
            first_wave = [slot_of[i] for i in leaders[:64]]
            assert len(set(first_wave)) >= 40 and len(first_wave) - len(set(first_wave)) >= 8
    assert v["counters"]["duplicate_sets"] == 13 and v["counters"]["duplicate_templates"] == 13
    y, yc = dy.counts(rd, c["L"]), dy.counts(jk.arrays(c["control"]), c["L"])
    assert yc["dedup_counters"]["duplicate_sets"] == 12 and yc["dedup_counters"]["duplicate_templates"] == 14
    assert not np.array_equal(y["counts"], yc["counts"])


def test_d3_what_the_search_found(programs):
    """a fragment key and a pair key that collide; no two fragment keys were found (tests/join_keys.py)"""
    assert jk.D3_FRAGMENT_FRAGMENT is None and "d3" in jk.DUP_CASES
    c = jk.dup_case("d3")
    rd, v, (kf, kp), _ = colliding_templates(programs, c)
    assert (kf[0], kp[0]) == ("F", "P") and kf[2][1] == 1
    assert v["counters"] == {"templates": 4, "duplicate_templates": 2, "duplicate_records": 3, "duplicate_sets": 2}
    assert v["winner"] == {kf: 1, kp: 2}
    m = merged(v, (kf, kp))                                         # bit 2 of the key keeps the two apart: no records have them equal
    assert int(m.sum()) == 4 and not np.array_equal(m, v["dup"])
