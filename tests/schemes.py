"""Primer and amplicon schemes of the tests and the files they are read from: the primer yardstick's scheme with its BED writer and the
product's compiled table, the hand-written amplicon scheme of the scheme rule with what it must turn into, and the two writers of
scheme rows.  No tests in here."""
import ctypes as C

import numpy as np

from tests import cli_run
from tests import primer_yardstick as py
from trueconsense_amd import _ffi

PRIMER_SCHEME = py.scheme()         # '+' [s, s + 24), '-' [s + 376, s + 400), s = 30, 330, ...: 12 primers


def write_primer_bed(path, primers, chrom="ref", extra=()):
    with open(path, "w") as fh:
        fh.write("# scheme\ntrack name=primers\n\n")
        for k, (s, e, rev) in enumerate(primers):
            fh.write("%s\t%d\t%d\tp%d_%s\t%d\t%s\n" % (chrom, s, e, k, "RIGHT" if rev else "LEFT", 1 + k % 2, "-" if rev else "+"))
        for line in extra:
            fh.write(line + "\n")
    return path


def compile_primers(primers, slack, cap=None):
    """tcmi_primers_compile -> (rc, head segments, tail segments, message)"""
    n = len(primers)
    s = np.ascontiguousarray([p[0] for p in primers], np.int64)
    e = np.ascontiguousarray([p[1] for p in primers], np.int64)
    r = np.ascontiguousarray([int(p[2]) for p in primers], np.int32)
    cap = 2 * n + 1 if cap is None else cap
    head, tail = np.zeros((cap, 3), np.int32), np.zeros((cap, 3), np.int32)
    nh, nt = C.c_int32(0), C.c_int32(0)
    msg = C.create_string_buffer(200)
    rc = _ffi.lib().tcmi_primers_compile(n, _ffi.ptr(s), _ffi.ptr(e), _ffi.ptr(r), slack, cap, _ffi.ptr(head), C.byref(nh), _ffi.ptr(tail), C.byref(nt), msg, 200)
    return rc, head[:nh.value], tail[:nt.value], msg.value.decode()


def write_scheme(path, rows):
    """scheme rows (chrom, start, end, name, pool, strand) as a bare BED file"""
    with open(path, "w") as fh:
        for r in rows:
            fh.write("\t".join(str(x) for x in r) + "\n")
    return path


def write_scheme_bed(path, rows, sep="\t"):
    """... behind a comment, a track line and an empty line"""
    with open(path, "w") as fh:
        fh.write("# a scheme\ntrack name=x\n\n")
        for r in rows:
            fh.write(sep.join(str(x) for x in r) + "\n")
    return str(path)


# ------------------------------------------------------------------------------------------------------------- the scheme rule
AMPLICON_SCHEME = [
    ("chrA", 10, 30, "nCoV-2019_1_LEFT", "1", "+"),
    ("chrA", 400, 420, "nCoV-2019_1_RIGHT", "1", "-"),
    ("chrA", 320, 342, "nCoV-2019_2_LEFT", "2", "+"),
    ("chrA", 700, 720, "nCoV-2019_2_RIGHT", "2", "-"),
    ("chrA", 14, 34, "nCoV-2019_1_LEFT_alt1", "9", "+"),        # an alternate: merges into amplicon 1, whose pool stays "1"
    ("chrA", 690, 712, "nCoV-2019_2_right_ALT", "2", "-"),      # any case; the field behind the side is ignored
    ("chrA", 640, 660, "nCoV-2019_3_LEFT", "1", "+"),
    ("chrA", 1000, 1020, "nCoV-2019_3_RIGHT_1", "1", "-"),
    ("chrB", 5, 25, "seg_LEFT_b_LEFT", "1", "+"),                 # the LAST side field counts: key "seg_LEFT_b"
    ("chrB", 300, 320, "seg_LEFT_b_RIGHT", "1", "-"),
    ("chrB", 100, 110, "in_LEFT", "2", "+"),                      # nested in seg_LEFT_b: cuts its unique region in two
    ("chrB", 150, 160, "in_RIGHT", "2", "-"),
    ("chrB", 50, 80, "ov_LEFT", "1", "+"),                        # primers that overlap: the insert is empty at its start
    ("chrB", 70, 90, "ov_RIGHT", "1", "-"),
]
AMPLICON_WANT = {
    "full": [("chrA", "nCoV-2019_1", "1", 10, 420), ("chrA", "nCoV-2019_2", "2", 320, 720), ("chrA", "nCoV-2019_3", "1", 640, 1020),
             ("chrB", "seg_LEFT_b", "1", 5, 320), ("chrB", "ov", "1", 50, 90), ("chrB", "in", "2", 100, 160)],
    "insert": [("chrA", "nCoV-2019_1", "1", 34, 400), ("chrA", "nCoV-2019_2", "2", 342, 690), ("chrA", "nCoV-2019_3", "1", 660, 1000),
               ("chrB", "seg_LEFT_b", "1", 25, 300), ("chrB", "ov", "1", 80, 80), ("chrB", "in", "2", 110, 150)],
    # seg_LEFT_b's insert [25, 300) minus ov [50, 90) and in [100, 160): [25, 50), [90, 100), [160, 300) -> the longest; `in` lies
    # wholly inside seg_LEFT_b's full: it vanishes
    "unique": [("chrA", "nCoV-2019_1", "1", 34, 320), ("chrA", "nCoV-2019_2", "2", 420, 640), ("chrA", "nCoV-2019_3", "1", 720, 1000),
               ("chrB", "seg_LEFT_b", "1", 160, 300), ("chrB", "ov", "1", 80, 80), ("chrB", "in", "2", 110, 110)],
}


def scheme_files(tmp_path):
    """stand-in input files for the argument parser, a reference named chrA and the amplicon scheme as s.bed -> {name: path}"""
    p = cli_run.stub_files(tmp_path, ("x.bam", "f.gff", "p.bed"))
    (tmp_path / "r.fa").write_text(">chrA\nACGT\n")
    p["r.fa"] = str(tmp_path / "r.fa")
    p["s.bed"] = write_scheme_bed(tmp_path / "s.bed", AMPLICON_SCHEME)
    return p
