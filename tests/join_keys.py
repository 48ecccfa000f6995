"""Keys that collide in the mate join's table (csrc/mate_join.hip) and in the duplicate rule's (csrc/dedup.hip), and the files made of them.
Both tables are open addressing over a 64-bit FNV-1a: the slot is the hash's low bits, the entry's 32-bit tag its high word, and a lane that
meets its own tag compares the full key.  Random keys share a tag once in 2^32, so that comparison's false branch, a chain that wraps from
the last slot to slot 0 and a group split by strangers need keys that were searched for.  In here:

  * both hashes restated in numpy (mate_hash, dup_hash), the tables' size for a file under either packer (table_slots), a key's home
    slot, and the build kernels' probing restated on key identities (mate_table, dup_table: no hashes compared, only who is who);
  * the seeded searches (search_*), each with a budget in candidate keys, and what they found as constants: names as bytes, positions,
    hard clips.  Tests read the constants; nothing searches when the suite runs.  `python -m tests.join_keys` runs every search again;
  * the files of tests/test_join_keys.py (which proves, without a device, what is claimed for the constants from the rule programs'
    output) and tests/test_join_collisions.py (which runs them through the kernels).

"Colliding" means: equal tag, and equal in the low BITS bits of the hash — BITS = 12, the log2 of the larger of the two tables a file of
at most 512 records and 64 KiB gets (the several-kernel packer's 1024 slots, the one-sync packer's 4096 at the most), so two colliding
keys share their home slot under both.  CLUSTER is the home slot of the cluster files: the low BITS bits all ones, the last slot of both
tables.  NEAR are the homes a key may have to lie INSIDE such a cluster of 80 entries or more: the last slot and the first 64.

Not searched for: two names that differ only in a tail of one or two bytes behind the last whole dword (94 resp. 94^2 tails per prefix
against 2^44: an estimated 10^11 resp. 10^9 hashes for one pair).  The three-byte tail was, and none was found (see the constants);
all three tails are compared without a device by tests/mate_rule_main.cpp --names.  No tests in here; opens no device."""
import functools

import numpy as np

from oracle import tc_oracle as orc
from tests import capacity_files as cf
from tests import dedup_yardstick as dy
from tests import mate_overlap_yardstick as my
from tests import read_specs as rs
from tests import synth_small as ss
from trueconsense_amd.io import bamwriter

BASIS, PRIME = np.uint64(0xCBF29CE484222325), np.uint64(0x100000001B3)
BITS = 12
CLUSTER = (1 << BITS) - 1
NEAR_FIRST = 64                                         # a home below it, or CLUSTER itself, lies inside a cluster of >= 80 entries
MOST_RECORDS, MOST_INFLATED = 512, 1 << 16              # a file within both gets tables of at most 1 << BITS slots
FIRST, LAST = 99, 147                                   # 0x1 | 0x2 | 0x20 | 0x40 and 0x1 | 0x2 | 0x10 | 0x80
PRINTABLE = np.arange(33, 127, dtype=np.uint8)          # the 94 bytes a SAM read name may hold ('!' .. '~'); '@' is among them


# ---- the hashes, restated ---------------------------------------------------------------------------------------------------------------
def fnv_bytes(h, cols):
    """h: uint64 array [n] (or one value), cols: uint8 [n, k] (or [k]: the same bytes for all) -> FNV-1a over the k bytes, in order"""
    h = np.asarray(h, np.uint64)
    cols = np.asarray(cols, np.uint8)
    with np.errstate(over="ignore"):
        for k in range(cols.shape[-1]):
            h = (h ^ cols[..., k].astype(np.uint64)) * PRIME
    return h


def fnv_words(h, *words):
    """... over 32-bit words, each little-endian (values are taken modulo 2^32: a negative u5 as the kernels store it)"""
    h = np.asarray(h, np.uint64)
    with np.errstate(over="ignore"):
        for w in words:
            w = (np.asarray(w, np.int64) & 0xFFFFFFFF).astype(np.uint64)
            for k in range(4):
                h = (h ^ ((w >> np.uint64(8 * k)) & np.uint64(0xFF))) * PRIME
    return h


def mate_hash(names, tid, lo, hi):
    """the join's hash (mate_rule.h tcmi_mate_hash): names uint8 [n, k] — or one name as bytes —, then refID, min and max of pos and next_pos"""
    if isinstance(names, (bytes, bytearray)):
        names = np.frombuffer(bytes(names), np.uint8)
    return fnv_words(fnv_bytes(BASIS, names), tid, lo, hi)


def dup_hash(w0, w1, w2):
    """the duplicate rule's (dedup_rule.h tcmi_dup_hash) over the three key words"""
    return fnv_words(BASIS, w0, w1, w2)


def pair_key(tid, end_a, end_b):
    """(u5, rev) of both ends -> the key words of a pair (dedup_rule.h tcmi_dup_key_pair)"""
    a, b = sorted([tuple(end_a), tuple(end_b)])
    return (tid << 3) | 4 | (a[1] << 1) | b[1], a[0] & 0xFFFFFFFF, b[0] & 0xFFFFFFFF


def fragment_key(tid, end):
    return (tid << 3) | (end[1] << 1), end[0] & 0xFFFFFFFF, 0


def tag(h):
    return np.asarray(h, np.uint64) >> np.uint64(32)


def home(h, slots):
    return np.asarray(h, np.uint64) & np.uint64(slots - 1)


def collide(h):
    """what two colliding keys share: tag << BITS | the low BITS bits"""
    h = np.asarray(h, np.uint64)
    return (tag(h) << np.uint64(BITS)) | (h & np.uint64(CLUSTER))


def near(h):
    """the key's home lies inside a cluster at CLUSTER of 80 entries or more, under every table of 1024 .. 1 << BITS slots"""
    low = np.asarray(h, np.uint64) & np.uint64(CLUSTER)
    return (low == np.uint64(CLUSTER)) | (low < np.uint64(NEAR_FIRST))


# ---- the tables, restated -----------------------------------------------------------------------------------------------------------------
def mate_slots(rec_cap):
    """pack_caps.h tcmi_mate_slots"""
    s = 1024
    while s < 2 * rec_cap:
        s <<= 1
    return s


def table_slots(path):
    """-> {packer: slots of both rules' tables for the file}: the several-kernel packer sizes them by the exact record count, the
    one-sync packer by pk_one_sync_caps' rec_cap (capacity_files.facts restates it).  The hint plays no part in a file this small —
    inflated / hint * 5 / 4 + 8192 lies above the other two bounds —, so neither does the file the context saw before."""
    f = cf.facts(path)
    assert f["safe_rec_cap"] < 8192
    return {"several_kernels": mate_slots(f["n_rec"]), "one_sync": mate_slots(f["caps"](f["hint"])["rec_cap"])}


def _probe(n, order, lockstep, step):
    """`step(i)` makes one try of record i's and says whether it is done.  In `order`, one record after the other — or, lockstep, as
    the lanes of a wavefront go: every record that is not done makes one try per round, in `order` within the round."""
    if not lockstep:
        for i in order:
            for _ in range(n):
                if step(i):
                    break
            else:
                raise AssertionError("the table filled")
        return
    todo = list(order)
    for _ in range(n):
        todo = [i for i in todo if not step(i)]
        if not todo:
            return
    raise AssertionError("the table filled")


def mate_table(hashes, key_of, slots, order, lockstep=False):
    """mate_build_kernel on records given by their hash and their key's identity (key_of[i]: anything that compares equal exactly for
    equal keys) -> the table: the record per slot, -1: empty.  A record that has met three of its key is not entered."""
    mask = slots - 1
    table = [-1] * slots
    at = {i: int(hashes[i]) & mask for i in order}
    seen = dict.fromkeys(order, 0)

    def step(i):
        s = at[i]
        if table[s] < 0:
            table[s] = i
            return True
        if key_of[table[s]] == key_of[i]:
            seen[i] += 1
            if seen[i] >= 3:
                return True
        at[i] = (s + 1) & mask
        return False
    _probe(slots + 1, order, lockstep, step)
    return table


def dup_table(hashes, key_of, slots, order, lockstep=False):
    """dup_build_kernel on leaders -> (table: the claiming leader per slot, -1: empty; slot_of: {leader: its key's slot})"""
    mask = slots - 1
    table = [-1] * slots
    at = {i: int(hashes[i]) & mask for i in order}

    def step(i):
        s = at[i]
        if table[s] < 0:
            table[s] = i
            return True
        if key_of[table[s]] == key_of[i]:
            return True
        at[i] = (s + 1) & mask
        return False
    _probe(slots + 1, order, lockstep, step)
    return table, at


def orders(n, seeds=(1, 2, 3, 4)):
    """the insertion orders the layouts are asserted for: {name: (order, lockstep)} — the file's order, its reverse, wavefronts of 64 in
    lockstep forwards and backwards, and seeded shuffles one by one and in lockstep"""
    fwd = list(range(n))
    out = {"file": (fwd, False), "reverse": (fwd[::-1], False), "lockstep": (fwd, True), "lockstep_reverse": (fwd[::-1], True)}
    for s in seeds:
        p = [int(k) for k in np.random.default_rng(s).permutation(n)]
        out["shuffle%d" % s] = (p, False)
        out["lockstep_shuffle%d" % s] = (p, True)
    return out


def chain_from(table, start):
    """-> the records of the run of full slots from `start` on, in probing order (round the table's end)"""
    out, s = [], start
    while table[s] >= 0 and len(out) < len(table):
        out.append(table[s])
        s = (s + 1) & (len(table) - 1)
    return out


# ---- the searches ---------------------------------------------------------------------------------------------------------------------------
def _names(rng, n, k, prefix=b""):
    """n names: `prefix`, then k random printable bytes -> uint8 [n, len(prefix) + k]"""
    tail = PRINTABLE[rng.integers(0, len(PRINTABLE), (n, k))]
    if not prefix:
        return tail
    return np.concatenate([np.broadcast_to(np.frombuffer(prefix, np.uint8), (n, len(prefix))), tail], axis=1)


def _chunks(budget, size=1 << 22):
    """the budget in pieces that fit memory"""
    return [min(size, budget - at) for at in range(0, budget, size)]


def _equal_pairs(c):
    """c: uint64 [n] -> [(i, j)], i < j, of neighbours in sorted order that are equal (a run of three gives two pairs)"""
    o = np.argsort(c, kind="stable")
    s = c[o]
    at = np.flatnonzero(s[1:] == s[:-1])
    return [(int(min(o[k], o[k + 1])), int(max(o[k], o[k + 1]))) for k in at]


def search_names(seed, budget, lengths, ints, prefixes=None, inside=False):
    """Read names of `lengths` (as many candidates of each; prefixes[k]: what the names of lengths[k] begin with) under one set of
    integers ints = (tid, lo, hi) -> [(name a, name b)] that collide, a before b in candidate order.  inside: only names whose home is
    near().  budget: candidate names in all."""
    rng = np.random.default_rng(seed)
    per = budget // len(lengths)
    names, hs = [], []
    for k, ln in enumerate(lengths):
        pre = prefixes[k] if prefixes else b""
        front = fnv_bytes(BASIS, np.frombuffer(pre, np.uint8))
        ms, hk = [], []
        for n in _chunks(per):
            m = _names(rng, n, ln - len(pre))
            h = fnv_words(fnv_bytes(front, m), *ints)
            keep = near(h) if inside else np.ones(n, bool)
            ms.append(m[keep])
            hk.append(h[keep])
        names.append(np.concatenate(ms))
        hs.append(np.concatenate(hk))
    h = np.concatenate(hs)
    which = np.concatenate([np.full(len(x), k) for k, x in enumerate(hs)])
    base = np.cumsum([0] + [len(x) for x in hs])
    out = []
    for i, j in _equal_pairs(collide(h)):
        a, b = ((prefixes[which[x]] if prefixes else b"") + bytes(names[which[x]][x - base[which[x]]]) for x in (i, j))
        if a != b:
            out.append((a, b))
    return out


def search_tail3(seed, budget, ints, n_prefix_bytes=8):
    """Names of n_prefix_bytes + 3 bytes that share their prefix — whole dwords — and differ in the three bytes behind it only: every
    94^3 tails under one random prefix after the other, until one holds a colliding pair or `budget` candidates are spent
    -> (prefixes tried, [(name a, name b)] of the first prefix that has one)"""
    assert n_prefix_bytes % 4 == 0
    rng = np.random.default_rng(seed)
    g = np.arange(len(PRINTABLE))
    tails = PRINTABLE[np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)]
    tried = 0
    while (tried + 1) * len(tails) <= budget:
        prefix = bytes(_names(rng, 1, n_prefix_bytes)[0])
        tried += 1
        h = fnv_words(fnv_bytes(fnv_bytes(BASIS, np.frombuffer(prefix, np.uint8)), tails), *ints)
        found = [(prefix + bytes(tails[i]), prefix + bytes(tails[j])) for i, j in _equal_pairs(collide(h))]
        if found:
            return tried, found
    return tried, []


def search_places(seed, budget, name, pos_below, dist_below):
    """ONE name at different places: (lo, hi) with lo < pos_below, hi - lo < dist_below, on reference 0 -> [((lo, hi), (lo, hi))] that collide"""
    rng = np.random.default_rng(seed)
    lo = rng.integers(0, pos_below, budget)
    hi = lo + rng.integers(0, dist_below, budget)
    h = fnv_words(fnv_bytes(BASIS, np.frombuffer(name, np.uint8)), 0, lo, hi)
    out = [((int(lo[i]), int(hi[i])), (int(lo[j]), int(hi[j]))) for i, j in _equal_pairs(collide(h))]
    return [p for p in out if p[0] != p[1]]


def search_homes(seed, budget, n_bytes, ints, want):
    """names of n_bytes under ints whose home is CLUSTER -> the first `want` of them (different tags), in candidate order"""
    rng = np.random.default_rng(seed)
    m = _names(rng, budget, n_bytes)
    h = mate_hash(m, *ints)
    at = np.flatnonzero((h & np.uint64(CLUSTER)) == np.uint64(CLUSTER))
    out, tags = [], set()
    for i in at:
        if int(tag(h[i])) not in tags and len(out) < want:
            tags.add(int(tag(h[i])))
            out.append(bytes(m[i]))
    return out


def _pair_words(u5a, u5b):
    """FR pairs on reference 0, the forward end at u5a < u5b, the reverse end's: the key words"""
    return np.full(len(u5a), 4 | 1), u5a, u5b


def search_pair_keys(seed, budget, a_from, b_from, width, inside=True):
    """Pair keys (forward end u5_a in [a_from - width, a_from], reverse end u5_b in [b_from, b_from + width]: what hard clips of up to
    `width` bases in front of the one and behind the other reach without moving a base) -> [((u5_a, u5_b), (u5_a, u5_b))] that collide;
    inside: whose home is near()"""
    rng = np.random.default_rng(seed)
    As, Bs, Hs = [], [], []
    for n in _chunks(budget):
        a = a_from - rng.integers(0, width + 1, n)
        b = b_from + rng.integers(0, width + 1, n)
        h = dup_hash(*_pair_words(a, b))
        keep = near(h) if inside else np.ones(n, bool)
        As.append(a[keep])
        Bs.append(b[keep])
        Hs.append(h[keep])
    a, b, h = np.concatenate(As), np.concatenate(Bs), np.concatenate(Hs)
    out = [((int(a[i]), int(b[i])), (int(a[j]), int(b[j]))) for i, j in _equal_pairs(collide(h))]
    return [p for p in out if p[0] != p[1]]


def search_fragment_keys(seed, budget, u5_below, pairs_too=None):
    """Fragment keys on reference 0 (u5 < u5_below, both strands), half the budget — and, pairs_too = (a_from, b_from, width), pair
    keys as search_pair_keys draws them for the other half -> [(key words, key words)] that collide, fragment–fragment and
    fragment–pair alike (pair–pair ones are dropped: search_pair_keys' business)"""
    rng = np.random.default_rng(seed)
    n = budget // 2 if pairs_too else budget
    w0 = 2 * rng.integers(0, 2, n)
    w1 = rng.integers(0, u5_below, n)
    w2 = np.zeros(n, np.int64)
    if pairs_too:
        a_from, b_from, width = pairs_too
        w0 = np.concatenate([w0, np.full(n, 5)])
        w1 = np.concatenate([w1, a_from - rng.integers(0, width + 1, n)])
        w2 = np.concatenate([w2, b_from + rng.integers(0, width + 1, n)])
    h = dup_hash(w0, w1, w2)
    key = lambda i: (int(w0[i]), int(w1[i]), int(w2[i]))
    out = [(key(i), key(j)) for i, j in _equal_pairs(collide(h))]
    return [p for p in out if p[0] != p[1] and not (p[0][0] & 4 and p[1][0] & 4)]


def search_fragment_homes(seed, budget, u5_from, width, want):
    """forward fragment keys with u5 in [u5_from - width, u5_from] whose home is CLUSTER -> the first `want` u5 (different tags)"""
    rng = np.random.default_rng(seed)
    u5 = np.unique(u5_from - rng.integers(0, width + 1, budget))
    h = dup_hash(np.zeros(len(u5), np.int64), u5, np.zeros(len(u5), np.int64))
    at = np.flatnonzero((h & np.uint64(CLUSTER)) == np.uint64(CLUSTER))
    out, tags = [], set()
    for i in at:
        if int(tag(h[i])) not in tags and len(out) < want:
            tags.add(int(tag(h[i])))
            out.append(int(u5[i]))
    return out


# ---- what the searches found ------------------------------------------------------------------------------------------------------------------
# Each constant with the call that found it (SEARCHES below runs them all again) and its budget in candidate keys.  Two searches found
# nothing, and a larger budget would not help them: the hash is FNV-1a, one multiplication per byte, so the difference of two hashes
# depends — up to the carries of the XOR — only on the DIFFERENCES of the bytes that differ, not on what stands around them.  Keys that
# differ in few bytes have few differences to offer against the 2^44 a collision needs, whatever the prefix:
#   * search_tail3: 400 prefixes x 94^3 tails = 3.3e8 names of 11 bytes that differ in their last three only: no pair (three byte
#     differences: at most 2^27 of them).  M1["tail3"] is None: no file of the suite sends two names with equal whole dwords and
#     different tails through the kernels.  That branch of the compare (mate_rule.h tcmi_mate_same_name, the text the kernels compile)
#     is checked without a device instead: tests/mate_rule_main.cpp --names, every length 1 .. 12 x every differing byte, the
#     one- and two-byte tails among them;
#   * search_fragment_keys: 2^24 fragment keys (u5 < 2^28, both strands): no fragment–fragment pair.  Fragment–pair ones it finds.
# The same shows in smaller ranges of the searches that did find: one name at places below 2^16 (distance < 256), 2^17 and 2^18: nothing
# among 2^24 each, below 2^19 (distance < 2048): 14; pair keys with both ends within 2^16: nothing inside a cluster among 2^27, within
# 2^20: 9.
M1_INTS = (0, 100, 130)
M1 = {
    "lengths": (b"{0Eu^ae^[", b"]RNAvIJY3a"),                       # search_names(1, 1 << 24, (9, 10), M1_INTS): 4 pairs, the first of two lengths
    "dword": (b"qL_~]0g[lg", b"3!0@NY5B_5"),                        # search_names(2, 1 << 24, (10,), M1_INTS): 1 pair
    "tail3": None,                                                  # search_tail3(10, 400 * 94 ** 3, M1_INTS): none
}
M2_NAME = b"one_name"
M2_PLACES = ((135002, 135422), (396528, 396634))                    # search_places(3, 1 << 24, M2_NAME, 1 << 19, 1 << 11): the first of 14
M2_L = 1 << 19
M3_INTS = (0, 200, 230)
M3_PAIRS = 40
M3_NAMES = (                                                        # search_homes(4, 1 << 18, 10, M3_INTS, 48): home CLUSTER, 48 tags
    b"@M}E0$ur*,", b"9ZGn^z,f+9", b"GS:ruE;@Yz", b"%kDWz~|h+^", b"~b!pG2?Kj<", b"~#Kqq@[gG=", b";{Lp-%dEu:", b"=_#eEG9^s,", b"4*#<9e&~#H",
    b"Itnm}4<hf)", b"+Hbem{.1_4", b"Y/JFLHl*Jd", b"-|_/^#\"d1}", b"koM]t-E_tY", b";7;]gZZtcf", b"+;JZAaeu(^", b"N5SK9OMk'\\", b"Ain;FHKy[X",
    b"PB?qjrq'zP", b"|E\\b)hjQGv", b"jPyq,-p~tS", b"Qo2v%K]<(+", b"t5BHe]^/,(", b"\"wI!rI0^p~", b"6/XY'BtGVJ", b"pp;qvi#4<N", b"e\"LwP0t;BC",
    b"VxVNJOk`pv", b"RdT+'[ZT5F", b"o*.Rr'Oi$^", b"\\VH(NU3W$S", b"kR45B;!Vg[", b"`()uva2)7g", b"=uHJAcls!h", b"J8TJ+Ph!n*", b"<3\\R+0SV;r",
    b"\"TO;<XQsWq", b"Q.!,@r`M$9", b"NEI?Vns/wP", b"rPK1,|EEcU", b"]l$S}j<&l[", b"u1IIe%HEx#", b"JhN*O4VpQ6", b"yc2MMi52cY", b"cb)w%xT7%|",
    b"|(#X7`4r`*", b"7Pi5|+Z+FC", b"FF\\su/zD;4")
M4_PAIR = (b"iu1a=H98MS", b"#g{HPV=Z{!")                             # search_names(6, 1 << 27, (10,), M3_INTS, inside=True): the first of 5
M5_INTS = (0, 300, 330)
M5_PREFIX = b"n" * 240
M5_EDGE = (M5_PREFIX + b"l^T!]hDHfo\\.y", M5_PREFIX + b"X2LL/y_h-zK'ei")     # search_names(5, 1 << 24, (253, 254), M5_INTS, prefixes=(M5_PREFIX,) * 2):
#                                                                     9 pairs, the first of 253 and 254 bytes
M5_NAMES = (b"a", b"bb", b"ccc", b"dddd", b"eeeee", b"fffffff", b"gggggggg", b"h" * 253, b"i" * 254)      # (not searched: every length of the edges)
M5_LAST_BYTE = (b"j" * 253 + b"A", b"j" * 253 + b"B")
D_WIDTH = (1 << 20) - 1
D_KEYS = ((-356491, 362494), (-340547, 884142))                     # search_pair_keys(7, 1 << 27, A_FROM, B_FROM, D_WIDTH): the first of 9, inside
D_N_STRANGERS = 44
D_STRANGERS = (                                                     # search_fragment_homes(9, 1 << 18, FRAG_POS, 1 << 20, 48): home CLUSTER, 48 tags
    -1046397, -1044718, -1008537, -1002602, -985616, -953529, -945177, -935376, -906561, -887314, -870191, -869536, -868062, -832316, -825722,
    -810784, -795998, -789396, -782129, -718124, -667155, -665841, -657489, -643943, -617556, -542580, -519659, -484113, -454749, -446717,
    -432787, -419304, -403477, -390521, -389132, -381755, -344690, -325313, -316404, -315523, -305554, -300577, -268539, -263542, -259343,
    -234927, -219804, -182568)
# search_fragment_keys(8, 1 << 25, 1 << 28, (A_FROM, B_FROM, 65535)): 2^24 fragment keys and 2^24 pair keys: no fragment–fragment pair, 13
# fragment–pair ones; the first whose fragment a record can have (a reverse one: a forward fragment's u5 lies below its pos).  Key words.
D3_FRAGMENT_FRAGMENT = None
D3_FRAGMENT_PAIR = ((2, 86690048, 0), (5, -33316, 60480))


# ---- the files ------------------------------------------------------------------------------------------------------------------------------
# A case: {"specs": records in file order, "L": the reference's length, "control": the same records with the colliding keys forced equal
# (absent where the case's condition is a chain's layout), further entries: what the case's tests look up}
L = 600


def _rec(rng, name, flag, pos, cigar, mpos, q=30):
    cig = [(n, "MIDNSHP=X"[op]) for op, n in ss.parse_cigar(cigar)]
    r = rs.mk(rng, pos, cig, [q] * sum(k for k, op in cig if op in "MIS=X"), name.decode("ascii"), flag=flag)
    r.update(mtid=0 if mpos >= 0 else -1, mpos=mpos, mapq=60, tlen=0)
    return r


def _pair(rng, name, p1, c1, p2, c2, q=30, flags=(FIRST, LAST)):
    return [_rec(rng, name, flags[0], p1, c1, p2, q), _rec(rng, name, flags[1], p2, c2, p1, q)]


def _by_pos(specs):
    """sorted by pos, records of equal pos in the order they were made: a pair's records lie apart, a group's among the others'"""
    return sorted(specs, key=lambda r: r["pos"])


def _renamed(specs, old, new):
    return [dict(r, name=new.decode("ascii")) if r["name"] == old.decode("ascii") else r for r in specs]


def _two_pairs(seed, names, ints, length=60):
    rng = np.random.default_rng(seed)
    _, lo, hi = ints
    cig = "%dM" % length
    specs = _by_pos(_pair(rng, names[0], lo, cig, hi, cig) + _pair(rng, names[1], lo, cig, hi, cig))
    return {"specs": specs, "L": L, "control": _renamed(specs, names[1], names[0]), "names": names, "ints": ints}


@functools.lru_cache(maxsize=None)
def mate_case(key):
    """the mate join's files, MATE_CASES"""
    if key.startswith("m1_"):
        return _two_pairs(11, M1[key[3:]], M1_INTS)
    if key == "m2":
        rng = np.random.default_rng(12)
        specs = []
        for lo, hi in M2_PLACES:
            cig = "%dM" % (hi - lo + 20)
            specs += _pair(rng, M2_NAME, lo, cig, hi, cig)
        (lo, hi), _ = M2_PLACES
        control = specs[:2] + [dict(specs[2], pos=lo, mpos=hi), dict(specs[3], pos=hi, mpos=lo)]
        return {"specs": _by_pos(specs), "L": M2_L, "control": _by_pos(control)}
    if key in ("m3", "m4"):
        rng = np.random.default_rng(13)
        _, lo, hi = M3_INTS
        specs = []
        for name in M3_NAMES[:M3_PAIRS]:
            specs += _pair(rng, name, lo, "40M", hi, "40M")
        if key == "m3":
            return {"specs": _by_pos(specs), "L": L, "strangers": M3_NAMES[:M3_PAIRS]}
        for name in M4_PAIR:
            specs += _pair(rng, name, lo, "40M", hi, "40M")
        three, five = M3_NAMES[M3_PAIRS], M3_NAMES[M3_PAIRS + 1]
        specs += _pair(rng, three, lo, "40M", hi, "40M") + [_rec(rng, three, LAST, hi, "38M", lo)]
        specs += _pair(rng, five, lo, "40M", hi, "40M") + [_rec(rng, five, FIRST, lo, "37M", hi)] + \
            [_rec(rng, five, LAST, hi, "%dM" % n, lo, q=20 + n) for n in (36, 35)]
        specs = _by_pos(specs)
        return {"specs": specs, "L": L, "control": _renamed(specs, M4_PAIR[1], M4_PAIR[0]), "strangers": M3_NAMES[:M3_PAIRS], "pair": M4_PAIR,
                "three": three, "five": five}
    if key == "m5":
        rng = np.random.default_rng(15)
        specs, at = [], 10
        for name in M5_NAMES:
            specs += _pair(rng, name, at, "30M", at + 10, "30M")
            at += 12
        for name in M5_LAST_BYTE:                                   # (one place: the last byte alone keeps the two pairs apart)
            specs += _pair(rng, name, at, "30M", at + 10, "30M")
        _, lo, hi = M5_INTS
        for name in M5_EDGE:
            specs += _pair(rng, name, lo, "60M", hi, "60M")
        specs = _by_pos(specs)
        return {"specs": specs, "L": L, "control": _renamed(specs, M5_EDGE[1], M5_EDGE[0]), "names": M5_EDGE, "ints": M5_INTS}
    raise KeyError(key)


MATE_CASES = tuple("m1_" + k for k, v in M1.items() if v) + ("m2", "m3", "m4", "m5")
FWD_POS, REV_POS, READ = 300, 340, 40                   # the duplicate cases' pairs: 40M forwards at 300, 40M reverse at 340
A_FROM, B_FROM = FWD_POS, REV_POS + READ - 1            # ... whose ends hard clips move down from 300 and up from 379
FRAG_POS, FRAG_READ = 100, 30                           # the stranger fragments: 30M forwards at 100, u5 moved down by hard clips


def _dup_pair(rng, name, ends, q):
    """a proper FR pair at FWD_POS / REV_POS whose ends are ends = (u5 of the forward record, u5 of the reverse one), by hard clips"""
    c1 = ("%dH" % (A_FROM - ends[0]) if ends[0] < A_FROM else "") + "%dM" % READ
    c2 = "%dM" % READ + ("%dH" % (ends[1] - B_FROM) if ends[1] > B_FROM else "")
    return _pair(rng, name, FWD_POS, c1, REV_POS, c2, q)


def _dup_frag(rng, name, u5, q):
    return _rec(rng, name, 0, FRAG_POS, ("%dH" % (FRAG_POS - u5) if u5 < FRAG_POS else "") + "%dM" % FRAG_READ, -1, q)


def _four_templates(seed, keys, order, quals):
    """four pairs: order[k] in "AB" says whose key template k has (the file's order: leaders 0 .. 3), quals[k] its base quality
    -> the case; its control gives every template key A"""
    rng = np.random.default_rng(seed)
    ends = {"A": keys[0], "B": keys[1]}
    specs, control = [], []
    for k, (who, q) in enumerate(zip(order, quals)):
        name = b"%s%d" % (who.encode(), k)
        specs += _dup_pair(rng, name, ends[who], q)
        control += _dup_pair(np.random.default_rng(seed + 100 + k), name, ends["A"], q)
    for r, c in zip(specs, control):                                # (the control's records differ in their clips alone)
        c.update(seq=r["seq"])
    return {"specs": _by_pos(specs), "L": L, "control": _by_pos(control), "order": order, "keys": keys}


@functools.lru_cache(maxsize=None)
def dup_case(key):
    """the duplicate rule's files, DUP_CASES"""
    if key == "d1":
        return _four_templates(21, D_KEYS, "AABB", (30, 35, 36, 25))
    if key == "d4":
        return _four_templates(24, D_KEYS, "BAAB", (30, 30, 30, 30))
    if key == "d2":
        c = dict(_four_templates(21, D_KEYS, "AABB", (30, 35, 36, 25)))
        rng = np.random.default_rng(22)
        frags = []
        for k, u5 in enumerate(D_STRANGERS[:D_N_STRANGERS]):
            frags.append(_dup_frag(rng, b"s%d" % k, u5, 30))
            if k % 4 == 0:                                          # (every fourth stranger key has two templates; the later one is the better)
                frags.append(_dup_frag(rng, b"s%d_again" % k, u5, 31))
        c["specs"] = _by_pos(frags + c["specs"])
        c["control"] = _by_pos(frags + c["control"])
        c["strangers"] = D_STRANGERS[:D_N_STRANGERS]
        return c
    if key == "d3":
        # two reverse fragments of the fragment key in front of two pairs of the pair key; the better pair is the best of all four
        rng = np.random.default_rng(23)
        (_, u5, _), (_, a, b) = D3_FRAGMENT_PAIR
        cig = "%dM%dH" % (FRAG_READ, u5 - (FRAG_POS + FRAG_READ - 1))
        specs = [_rec(rng, b"f%d" % k, 16, FRAG_POS, cig, -1, q) for k, q in enumerate((30, 35))]
        for k, q in enumerate((36, 25)):
            specs += _dup_pair(rng, b"p%d" % k, (a, b), q)
        return {"specs": _by_pos(specs), "L": L, "keys": D3_FRAGMENT_PAIR}
    raise KeyError(key)


DUP_CASES = ("d1", "d2", "d4") + (("d3",) if D3_FRAGMENT_PAIR else ())


def case(key):
    return mate_case(key) if key.startswith("m") else dup_case(key)


def write(path, specs, ref_len):
    """the records as a BAM file of one reference"""
    bamwriter.write_bam(str(path), arrays(specs), "ref", ref_len, block=4096)
    return str(path)


# ---- the records as the rule programs read them (tests/mate_rule_main.cpp, tests/dedup_rule_main.cpp) ---------------------------------------
def mate_program_lines(rd):
    """one line per record (every record of these files is kept)"""
    out = []
    for i in range(int(rd["n_reads"])):
        p, q = my.span(rd, i)
        out.append("%d %d %d %d %d %d %d %s" % (my.fields(rd, i) + (p, q, my.name(rd, i).hex() or "-")))
    return out


def dup_program_lines(rd, mate):
    """mate: {record: its mate} of the join's pairs (dedup_yardstick.verdicts' "mate")"""
    out = ["%d 0" % int(rd["n_reads"])]
    for i in range(int(rd["n_reads"])):
        cig = ["%d" % ((ln << 4) | op) for op, ln in orc.read_cigar(rd, i)]
        out.append("1 %d %d %d %d %d %s %s" % (int(rd["flag"][i]), int(rd["tid"][i]), int(rd["pos"][i]), mate.get(i, -1) + 1, len(cig),
                                              " ".join(cig), bytes(dy.quals(rd, i)).hex() or "-"))
    return out


def arrays(specs):
    return rs.arrays(specs)


# ---- every search again -------------------------------------------------------------------------------------------------------------------------
SEARCHES = (
    ("M1 lengths", lambda: search_names(1, 1 << 24, (9, 10), M1_INTS)),
    ("M1 dword", lambda: search_names(2, 1 << 24, (10,), M1_INTS)),
    ("M1 tail3", lambda: search_tail3(10, 400 * 94 ** 3, M1_INTS)),
    ("M2", lambda: search_places(3, 1 << 24, M2_NAME, 1 << 19, 1 << 11)),
    ("M3", lambda: search_homes(4, 1 << 18, 10, M3_INTS, 48)),
    ("M4", lambda: search_names(6, 1 << 27, (10,), M3_INTS, inside=True)),
    ("M5", lambda: search_names(5, 1 << 24, (253, 254), M5_INTS, prefixes=(M5_PREFIX,) * 2)),
    ("D keys", lambda: search_pair_keys(7, 1 << 27, A_FROM, B_FROM, D_WIDTH)),
    ("D strangers", lambda: search_fragment_homes(9, 1 << 18, FRAG_POS, 1 << 20, 48)),
    ("D3", lambda: search_fragment_keys(8, 1 << 25, 1 << 28, (A_FROM, B_FROM, 65535))),
)

if __name__ == "__main__":
    for what, search in SEARCHES:
        print(what, search())
