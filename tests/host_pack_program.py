"""The host packer's stand-alone program (tests/host_pack_main.cpp + csrc/host_pack.cpp) for tests/test_host_pack.py,
tests/test_odd_cigars_host.py and the parity test on the GPU: csrc/readset_layout.h restated, the dump formats the program reads and
writes, one run of it, its packed arrays decoded back into a count matrix against the oracle's, and the inputs the files put to it.  No tests in here."""
import os

import numpy as np

from oracle import c_oracle
from tests import fuzz_reads as fz
from tests import host_program
from tests import synth_small as ss

E_ARG, E_FORMAT, E_UNSUPPORTED = -3, -5, -9
# csrc/readset_layout.h, restated
ROUND, F_BLOCK, F_MAXW, F_MAXSPAN, F_SEG, F_SEQCAP, F_MAXSTAGE, P_NPL, P_SUB = 256, 256, 96, 600, 512, 6144, 8, 8, 512
EVPOS, EV_OTHER, EV_X, EV_I = 1 << 29, 1 << 29, 1 << 30, 1 << 31
CHUNK = np.dtype([("read0", "<i8"), ("word0", "<i8"), ("n_reads", "<i4"), ("P0", "<i4"), ("Wn", "<i4"), ("sub_reads", "<i4"),
                  ("stage_end", "<i4", (F_MAXSTAGE,)), ("run0", "<i8"), ("n_runs", "<i4"), ("reserved", "<i4")])
assert CHUNK.itemsize == 80, CHUNK.itemsize
TOTALS = ("n_reads", "n_piled", "alg", "max_end", "n_dropped", "f_reads", "f_chunks", "f_words", "f_events", "g_reads", "n_rounds", "n_cigar", "n_seqw")
OUT_TYPES = {"totals": "<i8", "ref_ext": "<i8", "f_lenoff": "<u4", "f_event": "<u4", "f_seq": "<u4", "f_chunk": CHUNK, "f_covrun": "<u4",
             "g_pos": "<i4", "g_meta": "<u4", "g_lseq": "<i4", "g_cigar": "<u4", "g_seq": "<u4", "g_round_cig": "<i8", "g_round_seq": "<i8"}
DEFAULTS = dict(threads=8, slots=1024, stride=0, layout=None, project_reads=1, use_fast=1, chunk_stages=0, stage_cap=0)


# ---- the program -----------------------------------------------------------------------------------------------------------------------
def build_program(out, sanitize=True):
    """tests/host_pack_main.cpp + csrc/host_pack.cpp and nothing else -> the program `out`"""
    return host_program.build(["tests/host_pack_main.cpp", "trueconsense_amd/csrc/host_pack.cpp"], out, sanitize, libs=["-lpthread"])


def _record(name, a):
    raw = np.ascontiguousarray(a).tobytes()
    return name.encode().ljust(16, b"\0") + np.uint64(len(raw)).tobytes() + raw


def write_dump(path, batch):
    """the read dicts of the tests -> the flat dump the program reads"""
    with open(path, "wb") as f:
        f.write(_record("n_batch", np.int64(len(batch))))
        for r in batch:
            n = int(r["n_reads"])
            f.write(_record("n_reads", np.int64(n)))
            tid = r.get("tid")
            for name, a, t in (("pos", r["pos"], "<i4"), ("flag", r["flag"], "<u2"), ("l_qseq", r["l_qseq"], "<i4"),
                               ("tid", np.zeros(n, np.int32) if tid is None else tid, "<i4"), ("cigar_off", r["cigar_off"], "<u8"),
                               ("cigar", r["cigar"], "<u4"), ("seq_off", r["seq_off"], "<u8"), ("seq", r["seq"], "u1")):
                f.write(_record(name, np.asarray(a).astype(t)))


def read_dump(path):
    raw, out, at = open(path, "rb").read(), {}, 0
    while at < len(raw):
        name = raw[at:at + 16].rstrip(b"\0").decode()
        n = int(np.frombuffer(raw, "<u8", 1, at + 16)[0])
        out[name] = np.frombuffer(raw, OUT_TYPES[name], n // np.dtype(OUT_TYPES[name]).itemsize, at + 24)
        at += 24 + n
    assert list(out) == list(OUT_TYPES), list(out)
    out["totals"] = dict(zip(TOTALS, (int(v) for v in out["totals"])))
    return out


def run(prog, tmp, batch, raw=False, **opt):
    """-> the decoded output dump (raw: its bytes), or ("refused", code, text)"""
    o = dict(DEFAULTS, **opt)
    src, dst = os.path.join(str(tmp), "in.dump"), os.path.join(str(tmp), "out.dump")
    write_dump(src, batch if isinstance(batch, (list, tuple)) else [batch])
    if os.path.exists(dst):
        os.remove(dst)
    args = [src, dst]
    for k in ("threads", "slots", "stride", "project_reads", "use_fast", "chunk_stages", "stage_cap"):
        args += ["--" + k.replace("_", "-"), str(o[k])]
    if o["layout"]:
        args += ["--layout", ",".join("%d:%d" % sl for sl in o["layout"])]
    r = host_program.run(prog, *args)
    if r.stdout.startswith("refused "):
        _, code, text = r.stdout.rstrip("\n").split(" ", 2)
        assert not os.path.exists(dst), dst
        return "refused", int(code), text
    assert r.stdout == "packed\n", r.stdout
    return open(dst, "rb").read() if raw else read_dump(dst)


# ---- the packed layout restated (csrc/readset_layout.h) and decoded back into a count matrix ----------------------------------------------------------------------------------------------
def slices_of(Wn):
    return F_BLOCK // max(2, (Wn * 8 + 31) // 32)


def read_words(length):
    return 2 * ((length + 31) // 32) + 2


def stage_reads(Wn, maxnw, stage_cap):
    S = slices_of(Wn)
    cap = min(P_SUB, (F_SEQCAP - 16 - 2) // read_words(maxnw * 8))
    if stage_cap > 0:
        cap = min(cap, max(stage_cap, S * 4))
    sub = S * 4 * max(1, cap // (S * 4))
    return sub if sub <= cap else max(S, cap // S * S)


def chunk_reads(sub, Wn, n_stages, balanced_cap):
    return min(max(sub, min(((1 << P_NPL) - 1) * slices_of(Wn), n_stages * sub) // sub * sub), balanced_cap)


def balanced_chunk(nf, slots):
    longest = F_MAXSTAGE * 400
    k = max(1, -(-nf // (slots * longest)))
    return max(64, -(-nf // (k * slots)))


def _bits(words, n):
    return np.unpackbits(np.ascontiguousarray(words).view(np.uint8), bitorder="little")[:n].astype(np.int32)


def decode(d, L, base=0, **opt):
    """The packed read set -> its count matrix [L, 7] over positions [base, base + L), by the layout comment alone; asserts on the way
    what tally_planes_kernel takes on trust of every chunk."""
    o = dict(DEFAULTS, **opt)
    T, ch, lenoff, seq, runs, ev = d["totals"], d["f_chunk"], d["f_lenoff"], d["f_seq"], d["f_covrun"], d["f_event"]
    assert (T["f_reads"], T["f_chunks"], T["f_words"], T["f_events"]) == (len(lenoff), len(ch), len(seq), len(ev))
    assert T["n_piled"] == T["f_reads"] + T["g_reads"] and T["f_words"] % 4 == 0
    n_stages = min(o["chunk_stages"], F_MAXSTAGE) if o["chunk_stages"] > 0 else F_MAXSTAGE
    cap = balanced_chunk(len(lenoff), o["slots"]) if o["chunk_stages"] == 0 else 1 << 62
    m = np.zeros((L + 1, 7), np.int64)
    cov = np.zeros(L + 2, np.int64)
    read_at, run_at, word_at, largest = 0, 0, 0, 0
    for c in ch:
        n, P0, Wn, sub, word0 = int(c["n_reads"]), int(c["P0"]), int(c["Wn"]), int(c["sub_reads"]), int(c["word0"])
        S = slices_of(Wn)
        assert c["read0"] == read_at and c["run0"] == run_at and n >= 1 and c["reserved"] == 0          # reads and runs tile their arrays
        assert word0 % 4 == 0 and word0 >= word_at and P0 % 8 == 0 and 1 <= Wn <= F_MAXW and 1 <= sub <= P_SUB
        assert n <= ((1 << P_NPL) - 1) * S and n <= F_MAXSTAGE * sub and n <= n_stages * sub and n <= cap
        n_st = -(-n // sub)
        ends = [int(e) for e in c["stage_end"]]
        assert all(a < b for a, b in zip(ends[:n_st - 1], ends[1:n_st])) and not any(ends[n_st:])
        assert all((ends[i] - (ends[i - 1] - 2 if i else 0)) <= F_SEQCAP - 16 for i in range(n_st))
        # coverage: the run words, a difference array
        rw = runs[run_at:run_at + int(c["n_runs"])].astype(np.int64)
        r_rel, r_len, r_cnt = rw & 1023, (rw >> 10) & 1023, rw >> 20
        assert len(rw) >= 1 and r_cnt.min() >= 1 and r_cnt.max() <= 4095 and r_cnt.sum() == n
        np.add.at(cov, P0 + r_rel - base, r_cnt)
        np.add.at(cov, P0 + r_rel + r_len - base, -r_cnt)
        hd = lenoff[read_at:read_at + n].astype(np.int64)
        rel, ln, pair = hd & 1023, (hd >> 10) & 1023, hd >> 20
        assert np.array_equal(np.repeat(rw & 0xFFFFF, r_cnt), hd & 0xFFFFF)                            # the runs are the reads, in order
        assert ln.min() >= 1 and (rel + ln).max() <= Wn * 8
        assert sub == stage_reads(Wn, int((ln.max() + 7) // 8), o["stage_cap"])
        largest = max(largest, n)
        cursor = word0 + 2
        for j in range(n):
            st = j // sub
            start = word0 + (ends[st - 1] - 2 if st else 0)
            a, nwords = start + 2 * int(pair[j]), 2 * ((int(ln[j]) + 31) // 32)
            assert a == cursor and not seq[a - 2] and not seq[a - 1]                                   # packed back to back, a zero pair in front
            assert a + nwords + 2 <= word0 + ends[st]
            planes = seq[a:a + nwords].reshape(-1, 2)
            code = _bits(planes[:, 0], int(ln[j])) + 2 * _bits(planes[:, 1], int(ln[j]))
            p = P0 + int(rel[j]) - base
            for k, col in ((1, 3), (2, 4), (3, 2)):                                                    # C, G, T in the oracle's columns
                m[p:p + int(ln[j]), col] += code == k
            cursor = a + nwords + 2
            if (j + 1) % sub == 0 or j + 1 == n:
                assert ends[st] == cursor - word0 and not seq[cursor - 2] and not seq[cursor - 1]      # ... and one behind the stage's last
        read_at, run_at, word_at = read_at + n, run_at + int(c["n_runs"]), cursor
    assert read_at == len(lenoff) and run_at == len(runs) and word_at <= len(seq)
    m[:, 0] = np.cumsum(cov)[:L + 1]
    e = ev.astype(np.int64)
    assert len(e) == 0 or ((e >> 29).min() >= 1 and (e & (EVPOS - 1)).max() < T["max_end"])           # a kind, and a position below 2^29
    other = np.zeros(L + 1, np.int64)
    for bit, into in ((EV_OTHER, other), (EV_X, m[:, 5]), (EV_I, m[:, 6])):
        np.add.at(into, (e[(e & bit) != 0] & (EVPOS - 1)) - base, 1)
    m[:, 1] = m[:, 0] - m[:, 2] - m[:, 3] - m[:, 4] - other                                            # A by subtraction
    assert not m[L].any()
    # the general set: back into a read dict, tallied by the oracle
    ng = T["g_reads"]
    if ng:
        nc, lq = (d["g_meta"] & 0xFFFF).astype(np.uint64), d["g_lseq"].astype(np.int64)
        coff, soff = np.concatenate([[0], np.cumsum(nc)]).astype(np.uint64), np.concatenate([[0], np.cumsum((lq + 7) // 8)]).astype(np.uint64)
        assert T["n_rounds"] == -(-ng // ROUND) and (T["n_cigar"], T["n_seqw"]) == (int(coff[-1]), int(soff[-1]))
        at = list(range(0, ng, ROUND)) + [ng]
        assert np.array_equal(d["g_round_cig"], coff[at].astype(np.int64)) and np.array_equal(d["g_round_seq"], soff[at].astype(np.int64))
        b = d["g_seq"].view(np.uint8)
        g = {"n_reads": ng, "pos": (d["g_pos"].astype(np.int64) - base).astype(np.int32), "flag": (d["g_meta"] >> 16).astype(np.uint16),
             "l_qseq": d["g_lseq"].astype(np.int32), "cigar_off": coff, "cigar": np.ascontiguousarray(d["g_cigar"]), "seq_off": soff * np.uint64(4),
             "seq": np.ascontiguousarray((b << 4) | (b >> 4)), "tid": None}
        m[:L] += c_oracle.tally(g, L)
    else:
        assert (T["n_rounds"], T["n_cigar"], T["n_seqw"]) == (0, 0, 0)
    return m[:L], largest


def algorithmic_bytes(reads, keep):
    nc = np.diff(reads["cigar_off"].astype(np.int64))
    return int((12 + 4 * nc + (reads["l_qseq"].astype(np.int64) + 1) // 2)[keep].sum())


def check(prog, tmp, reads, L=None, **opt):
    """pack, decode, compare with the oracle -> (the dump, the largest chunk's reads)"""
    L = L or c_oracle.extent(reads, 0)
    d = run(prog, tmp, reads, **opt)
    assert isinstance(d, dict), d
    got, largest = decode(d, L, **opt)
    want = c_oracle.tally(reads, L)
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    assert d["totals"]["n_reads"] == reads["n_reads"] and d["totals"]["max_end"] == L
    return d, largest


# ---- the inputs --------------------------------------------------------------------------------------------------------------------------
def plain_reads(rng, starts, lens, cigars=None):
    """reads of the given starts and lengths ("<len>M" unless cigars says otherwise), random bases"""
    cigars = cigars or ["%dM" % n for n in lens]
    return ss.reads_from_spec({"reads": [{"pos": int(p), "flag": 0, "cigar": c, "seq": "".join("ACGT"[k] for k in rng.integers(0, 4, int(n)))}
                                         for p, n, c in zip(starts, lens, cigars)]})


def fuzz_cases():
    rng = np.random.default_rng(2024)
    return [("sorted", fz.random_reads(rng, 3000, 1500)), ("unsorted", fz.random_reads(rng, 3000, 1500, sort=False)),
            ("long", fz.random_reads(rng, 400, 20000, long_reads=True))]


def short_reads():
    """6 000 reads of 20-40 bases on sorted starts in [0, 700): one window, S = 10 depth slices"""
    rng = np.random.default_rng(7)
    starts, lens = np.sort(rng.integers(0, 700, 6000)), rng.integers(20, 41, 6000)
    starts[0], starts[-1], lens[-1] = 0, 699, 40                    # (all of [0, 739): 93 grid words, 24 lane groups)
    return plain_reads(rng, starts, lens)
