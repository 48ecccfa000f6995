"""What the duplicate rule must make of tests/mate_big.py's files (reads of 50M, every quality 30: every set is a tie, the lowest leader
wins), restated in numpy — the keys are found with np.unique, not taken from how the file was made — and a file of one key with many
templates next to as many keys of one template each.  The restatement is pinned to tests/dedup_yardstick.py on a 2 000-record prefix in
tests/test_dedup_rule.py; tests/test_dedup.py then uses it at a record count that yardstick cannot afford.  No GPU, no tests in here."""
import numpy as np

from tests import mate_big as mb
from trueconsense_amd.io import bamwriter

COUNTERS = ("templates", "duplicate_templates", "duplicate_records", "duplicate_sets")


def pairs(rd):
    """-> mate int64 [n]: the record a record is paired with by the mate join's rule, -1: none (mate_big.join's groups)"""
    n = len(rd["pos"])
    flag, pos, npos = rd["flag"].astype(np.int64), rd["pos"].astype(np.int64), rd["next_pos"].astype(np.int64)
    eligible = ((flag & 3) == 3) & ((flag & (8 | 0x100 | 0x800)) == 0) & (((flag >> 6) ^ (flag >> 7)) & 1 == 1) & (npos >= 0)
    idx = np.flatnonzero(eligible)
    key = np.stack([rd["name"][idx], np.minimum(pos[idx], npos[idx]), np.maximum(pos[idx], npos[idx])], 1)
    _, inv, cnt = np.unique(key, axis=0, return_inverse=True, return_counts=True)
    inv = inv.reshape(-1)
    order = np.argsort(inv, kind="stable")
    members = idx[order]
    two = np.flatnonzero(cnt[inv[order]] == 2)[0::2]
    a, b = members[two], members[two + 1]
    ok = (npos[a] == pos[b]) & (npos[b] == pos[a]) & (((flag[a] & 0x40) != 0) != ((flag[b] & 0x40) != 0))
    mate = np.full(n, -1, np.int64)
    mate[a[ok]], mate[b[ok]] = b[ok], a[ok]
    return mate


def verdicts(rd):
    """-> (dup bool [n], {counter: n}): every record is examined (mapped, primary) and scores the same"""
    n = len(rd["pos"])
    mate = pairs(rd)
    rev = (rd["flag"].astype(np.int64) >> 4) & 1
    u5 = rd["pos"].astype(np.int64) + rev * (mb.LEN - 1)
    i = np.arange(n)
    lead = np.flatnonzero((mate < 0) | (mate > i))
    m = mate[lead]
    paired = m >= 0
    mu5, mrev = np.where(paired, u5[np.maximum(m, 0)], 0), np.where(paired, rev[np.maximum(m, 0)], 0)
    first = ~paired | (u5[lead] < mu5) | ((u5[lead] == mu5) & (rev[lead] <= mrev))
    key = np.stack([paired.astype(np.int64), np.where(first, u5[lead], mu5), np.where(first, rev[lead], mrev),
                    np.where(paired, np.where(first, mu5, u5[lead]), 0), np.where(paired, np.where(first, mrev, rev[lead]), 0)], 1)
    _, inv, cnt = np.unique(key, axis=0, return_inverse=True, return_counts=True)
    inv = inv.reshape(-1)
    best = np.full(len(cnt), n, np.int64)
    np.minimum.at(best, inv, lead)                              # (equal scores within a key: the lowest leader)
    loses = best[inv] != lead
    dup = np.zeros(n, bool)
    dup[lead[loses]] = True
    dup[m[loses & paired]] = True
    return dup, {"templates": int(len(lead)), "duplicate_templates": int(loses.sum()), "duplicate_records": int(dup.sum()),
                 "duplicate_sets": int((cnt >= 2).sum())}


# ---- one key, many templates ------------------------------------------------------------------------------------------------------------------
ONE_LEN = 30
ONE_AT = 50


def one_key_and_distinct(path, n_each, seed=9):
    """n_each forward fragments of 30M at column 50 — their scores as distinct as 30 qualities allow (30 x 93 < n_each), one of them the
    only best, in the middle of the file's set —, then n_each more at n_each distinct columns.  -> (dup bool [2 n_each], coverage int64
    [L] of the records that are no duplicates, L)"""
    rng = np.random.default_rng(seed)
    n = 2 * n_each
    L = 200 + n_each + ONE_LEN + 100
    pos = np.concatenate([np.full(n_each, ONE_AT), 200 + np.arange(n_each)]).astype(np.int32)
    qual = rng.integers(2, 41, (n, ONE_LEN)).astype(np.uint8)
    best = n_each // 2 + 1
    qual[best] = 41                                             # (30 x 41: above every other record's sum)
    score = np.where(qual >= 15, qual, 0).sum(1)
    assert (score[:n_each] == score[best]).sum() == 1 and score[:n_each].max() == score[best]
    rec_len = 32 + 8 + 4 + ONE_LEN // 2 + ONE_LEN
    rec = np.zeros((n, 4 + rec_len), np.uint8)

    def put(col, arr, dt):
        a = np.ascontiguousarray(arr, dt).view(np.uint8).reshape(n, -1)
        rec[:, col:col + a.shape[1]] = a
    put(0, np.full(n, rec_len), "<i4")
    put(8, pos, "<i4")
    rec[:, 12] = 8
    rec[:, 13] = 60
    put(14, np.full(n, 4681), "<u2")
    put(16, np.full(n, 1), "<u2")
    put(20, np.full(n, ONE_LEN), "<u4")
    put(24, np.full(n, -1), "<i4")
    put(28, np.full(n, -1), "<i4")
    for k in range(7):
        rec[:, 36 + 6 - k] = 48 + (np.arange(n) // 10 ** k) % 10
    put(44, np.full(n, ONE_LEN << 4), "<u4")
    rec[:, 48:48 + ONE_LEN // 2] = 0x11                         # (every base A)
    rec[:, 48 + ONE_LEN // 2:] = qual
    text = ("@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:ref\tLN:%d\n" % L).encode()
    headb = b"BAM\1" + np.int32(len(text)).tobytes() + text + np.int32(1).tobytes() + np.int32(4).tobytes() + b"ref\0" + np.int32(L).tobytes()
    per = max(1, 0xFF00 // (4 + rec_len))
    with open(path, "wb") as fh:
        fh.write(bamwriter._bgzf_block(headb, 1))
        flat = rec.reshape(-1)
        step = per * (4 + rec_len)
        for o in range(0, flat.size, step):
            fh.write(bamwriter._bgzf_block(flat[o:o + step].tobytes(), 1))
        fh.write(bamwriter._EOF)
    dup = np.zeros(n, bool)
    dup[:n_each] = True
    dup[best] = False
    cov = np.zeros(L + 1, np.int64)
    np.add.at(cov, pos[~dup], 1)
    np.add.at(cov, pos[~dup] + ONE_LEN, -1)
    return dup, np.cumsum(cov)[:L], L


def one_key_reads(n_each, seed=9):
    """the flat arrays of a SMALL one_key_and_distinct file, for the yardstick (the same generator state: the same qualities)"""
    rng = np.random.default_rng(seed)
    n = 2 * n_each
    pos = np.concatenate([np.full(n_each, ONE_AT), 200 + np.arange(n_each)]).astype(np.int32)
    qual = rng.integers(2, 41, (n, ONE_LEN)).astype(np.uint8)
    qual[n_each // 2 + 1] = 41
    names = np.zeros((n, 7), np.uint8)
    for k in range(7):
        names[:, 6 - k] = 48 + (np.arange(n) // 10 ** k) % 10
    return {"n_reads": n, "pos": pos, "flag": np.zeros(n, np.uint16), "l_qseq": np.full(n, ONE_LEN, np.int32), "tid": np.zeros(n, np.int32),
            "cigar_off": np.arange(n + 1, dtype=np.uint64), "cigar": np.full(n, ONE_LEN << 4, np.uint32),
            "seq_off": np.arange(n + 1, dtype=np.uint64) * (ONE_LEN // 2), "seq": np.full(n * (ONE_LEN // 2), 0x11, np.uint8),
            "qual_off": np.arange(n + 1, dtype=np.uint64) * ONE_LEN, "qual": qual.reshape(-1).copy(),
            "name_off": np.arange(n + 1, dtype=np.uint64) * 7, "names": names.reshape(-1).copy(),
            "next_tid": np.full(n, -1, np.int32), "next_pos": np.full(n, -1, np.int32), "tlen": np.zeros(n, np.int32), "mapq": np.full(n, 60, np.uint8)}
