"""The host packer's stand-alone program (tests/host_pack_main.cpp + csrc/host_pack.cpp) for tests/test_host_pack.py and the parity
test on the GPU: csrc/readset_layout.h restated, the dump formats the program reads and writes, one run of it, and the inputs both
files put to it.  No tests in here."""
import os

import numpy as np

from tests import fuzz_reads as fz
from tests import host_program
from tests import synth_small as ss

E_ARG, E_UNSUPPORTED = -3, -9
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
