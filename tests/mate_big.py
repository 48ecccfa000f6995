"""Read pairs of one fixed length with one M op each, by the hundred thousand, written with numpy, and what the mate join and the step
must give for them, restated in numpy: the groups are found with np.unique over (name, min, max), not taken from how the file was made.
The restatement is pinned to tests/mate_overlap_yardstick.py on a 2 000-record prefix in tests/test_mate_rule.py;
tests/test_mate_overlap.py then uses it at a record count that yardstick cannot afford.  No GPU, no tests in here."""
import numpy as np

from trueconsense_amd.io import bamwriter

LEN = 50                                                                        # every read is 50M
L = 1600
NAME = 9                                                                        # digits of a name
NIBBLES = np.array([1, 8, 2, 4], np.uint8)                                      # A T C G as BAM writes them
PLANE = np.zeros(16, np.int64)
PLANE[[1, 8, 2, 4]] = (1, 2, 3, 4)
FIRST, LAST = 99, 147


def generate(n, seed=3):
    """-> dict(pos, flag, base [n, LEN], name int64 [n], next_pos), sorted by pos: n // 2 pairs with unique names whose second mate starts
    0 .. 59 columns behind the first (50 and more: no shared column), a single record when n is odd; a few pairs not proper, a few of
    two firsts"""
    rng = np.random.default_rng(seed)
    n_pairs = n // 2
    j = np.arange(n_pairs, dtype=np.int64)
    base = j * (L - 120) // max(n_pairs, 1)
    d = rng.integers(0, 60, n_pairs)
    pos = np.concatenate([base, base + d, np.full(n - 2 * n_pairs, L - 60)])
    npos = np.concatenate([base + d, base, np.full(n - 2 * n_pairs, -1)])
    f2 = np.where(j % 97 == 5, LAST & ~2, np.where(j % 89 == 7, FIRST | 16, LAST))
    flag = np.concatenate([np.full(n_pairs, FIRST), f2, np.zeros(n - 2 * n_pairs, np.int64)])
    name = np.concatenate([j, j, np.full(n - 2 * n_pairs, n_pairs)])
    order = np.argsort(pos, kind="stable")
    return dict(pos=pos[order].astype(np.int32), flag=flag[order].astype(np.uint16), name=name[order], next_pos=npos[order].astype(np.int32),
                base=NIBBLES[rng.integers(0, 4, (n, LEN))])


def head(rd, n):
    return {k: v[:n] for k, v in rd.items()}


def name_bytes(rd):
    n = len(rd["pos"])
    out = np.zeros((n, NAME), np.uint8)
    for k in range(NAME):
        out[:, NAME - 1 - k] = 48 + (rd["name"] // 10 ** k) % 10
    return out


def write(path, rd):
    """the records as a BAM file, whole records per BGZF block as htslib cuts them"""
    n = len(rd["pos"])
    nb = LEN // 2
    rec_len = 32 + NAME + 1 + 4 + nb + LEN
    rec = np.zeros((n, 4 + rec_len), np.uint8)

    def put(col, arr, dt):
        a = np.ascontiguousarray(arr, dt).view(np.uint8).reshape(n, -1)
        rec[:, col:col + a.shape[1]] = a
    put(0, np.full(n, rec_len), "<i4")
    put(8, rd["pos"], "<i4")
    rec[:, 12] = NAME + 1
    rec[:, 13] = 60
    put(14, np.full(n, 4681), "<u2")
    put(16, np.full(n, 1), "<u2")
    put(18, rd["flag"], "<u2")
    put(20, np.full(n, LEN), "<u4")
    put(24, np.where(rd["next_pos"] >= 0, 0, -1), "<i4")
    put(28, rd["next_pos"], "<i4")
    rec[:, 36:36 + NAME] = name_bytes(rd)
    put(36 + NAME + 1, np.full(n, LEN << 4), "<u4")
    s0 = 36 + NAME + 1 + 4
    rec[:, s0:s0 + nb] = (rd["base"][:, 0::2] << 4) | rd["base"][:, 1::2]
    rec[:, s0 + nb:s0 + nb + LEN] = 30
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
    return str(path)


def as_reads(rd):
    """the records as the flat arrays the oracle and the yardsticks read"""
    n = len(rd["pos"])
    packed = (rd["base"][:, 0::2] << 4) | rd["base"][:, 1::2]
    return {"n_reads": n, "pos": rd["pos"], "flag": rd["flag"], "l_qseq": np.full(n, LEN, np.int32), "tid": np.zeros(n, np.int32),
            "cigar_off": np.arange(n + 1, dtype=np.uint64), "cigar": np.full(n, LEN << 4, np.uint32),
            "seq_off": np.arange(n + 1, dtype=np.uint64) * (LEN // 2), "seq": packed.reshape(-1).copy(),
            "qual_off": np.arange(n + 1, dtype=np.uint64) * LEN, "qual": np.full(n * LEN, 30, np.uint8),
            "name_off": np.arange(n + 1, dtype=np.uint64) * NAME, "names": name_bytes(rd).reshape(-1).copy(),
            "next_tid": np.where(rd["next_pos"] >= 0, 0, -1).astype(np.int32), "next_pos": rd["next_pos"], "tlen": np.zeros(n, np.int32),
            "mapq": np.full(n, 60, np.uint8)}


def join(rd):
    """-> (clip int64 [n], {counter: n})"""
    n = len(rd["pos"])
    flag, pos, npos = rd["flag"].astype(np.int64), rd["pos"].astype(np.int64), rd["next_pos"].astype(np.int64)
    eligible = ((flag & 3) == 3) & ((flag & (8 | 0x100 | 0x800)) == 0) & (((flag >> 6) ^ (flag >> 7)) & 1 == 1) & (npos >= 0)
    idx = np.flatnonzero(eligible)
    key = np.stack([rd["name"][idx], np.minimum(pos[idx], npos[idx]), np.maximum(pos[idx], npos[idx])], 1)
    _, inv, cnt = np.unique(key, axis=0, return_inverse=True, return_counts=True)
    inv = inv.reshape(-1)
    clip = np.zeros(n, np.int64)
    order = np.argsort(inv, kind="stable")
    members = idx[order]                                                        # grouped, in file order within a group
    size = cnt[inv[order]]
    two = np.flatnonzero(size == 2)[0::2]
    a, b = members[two], members[two + 1]
    pair = (npos[a] == pos[b]) & (npos[b] == pos[a]) & (((flag[a] & 0x40) != 0) != ((flag[b] & 0x40) != 0))
    a, b = a[pair], b[pair]
    a_loses = (pos[a] > pos[b]) | ((pos[a] == pos[b]) & ((flag[a] & 0x80) != 0))
    lo, wi = np.where(a_loses, a, b), np.where(a_loses, b, a)
    clip[lo] = np.maximum(0, np.minimum(pos[wi], pos[lo]) + LEN - 1 - pos[lo] + 1)
    return clip, {"pairs": int(len(lo)), "clipped_reads": int((clip > 0).sum()), "clipped_columns": int(clip.sum()), "ambiguous": int(size[size >= 3].sum())}


def matrix(rd, n_pos, clip):
    """-> int32 [n_pos, 7]: every record's tokens from its column pos + clip on"""
    p = rd["pos"].astype(np.int64)
    out = np.zeros(n_pos * 8, np.int64)
    for o in range(LEN):
        ok = clip <= o
        out += np.bincount(((p + o) * 8 + PLANE[rd["base"][:, o]])[ok], minlength=len(out))
    out = out.reshape(n_pos, 8)
    m = np.zeros((n_pos, 7), np.int32)
    m[:, 0] = out[:, 1:5].sum(1)
    m[:, 1:5] = out[:, 1:5]
    return m
