"""Primer schemes as BED files (the format of ARTIC's *.primer.bed, `ivar trim -b`, `samtools ampliconclip -b`).

Columns: chrom, start, end, name, score / pool, strand — tab or blank separated, 0-based and end-exclusive.  Lines that start with
`#`, `track` or `browser` and blank lines are ignored; anything else that does not parse is an error that names its line."""
from collections import namedtuple


class PrimerBedError(ValueError):
    pass


def read_bed(path):
    """-> [(chrom, start, end, reverse)], reverse True for a '-' (right) primer; PrimerBedError names the file and the line."""
    rows = []
    with open(path) as fh:
        for ln, line in enumerate(fh, 1):
            text = line.strip()
            if not text or text.startswith(("#", "track", "browser")):
                continue
            f = text.split("\t") if "\t" in text else text.split()
            where = "%s:%d" % (path, ln)
            if len(f) < 6:
                raise PrimerBedError("%s: a primer row has six columns (chrom, start, end, name, score, strand), this one has %d" % (where, len(f)))
            try:
                start, end = int(f[1]), int(f[2])
            except ValueError:
                raise PrimerBedError("%s: start and end are integers, not %r and %r" % (where, f[1], f[2])) from None
            if start < 0 or end <= start:
                raise PrimerBedError("%s: [%d, %d) is not an interval" % (where, start, end))
            if f[5] not in ("+", "-"):
                raise PrimerBedError("%s: the strand in column 6 is '+' or '-', not %r" % (where, f[5]))
            rows.append((f[0], start, end, f[5] == "-"))
    return rows


def rows_for_reference(rows, name):
    """The rows on reference `name`, as Context.set_primers takes them: [(start, end, reverse)]."""
    return [(s, e, r) for c, s, e, r in rows if c == name]


def rows_for_layout(rows, names, shift):
    """A contig layout (names[t] starts at shift[t] on the axis; < 0: no slot): every row shifted by its contig's slot — the slots
    are disjoint, so one table serves the axis; rows that name no contig of the layout are ignored."""
    at = {n: int(shift[t]) for t, n in enumerate(names) if int(shift[t]) >= 0}
    return [(s + at[c], e + at[c], r) for c, s, e, r in rows if c in at]


# ---- the scheme's amplicons (--amplicon-table) ------------------------------------------------------------------------------
SchemeRow = namedtuple("SchemeRow", "chrom start end name pool reverse where")      # where: "file:line", for the errors
Amplicon = namedtuple("Amplicon", "chrom name pool start end")                      # [start, end): the interval the table reports
REGIONS = ("insert", "unique", "full")


def read_scheme(path):
    """-> [SchemeRow]: read_bed's rows (same lines, same errors) with the name (column 4) and the pool (column 5) kept."""
    rows = []
    with open(path) as fh:
        for ln, line in enumerate(fh, 1):
            text = line.strip()
            if not text or text.startswith(("#", "track", "browser")):
                continue
            f = text.split("\t") if "\t" in text else text.split()
            where = "%s:%d" % (path, ln)
            if len(f) < 6:
                raise PrimerBedError("%s: a primer row has six columns (chrom, start, end, name, score, strand), this one has %d" % (where, len(f)))
            try:
                start, end = int(f[1]), int(f[2])
            except ValueError:
                raise PrimerBedError("%s: start and end are integers, not %r and %r" % (where, f[1], f[2])) from None
            if start < 0 or end <= start:
                raise PrimerBedError("%s: [%d, %d) is not an interval" % (where, start, end))
            if f[5] not in ("+", "-"):
                raise PrimerBedError("%s: the strand in column 6 is '+' or '-', not %r" % (where, f[5]))
            rows.append(SchemeRow(f[0], start, end, f[3], f[4], f[5] == "-", where))
    return rows


def _side_of(row):
    """a primer's name -> (the amplicon's key, "LEFT" / "RIGHT"): the name is split at "_"; the LAST field equal to LEFT or RIGHT
    (any case) is the side, the fields in front of it, joined, the key; those behind it (alt, alt1, 1) are ignored."""
    f = row.name.split("_")
    for k in range(len(f) - 1, -1, -1):
        if f[k].upper() in ("LEFT", "RIGHT"):
            return "_".join(f[:k]), f[k].upper()
    raise PrimerBedError("%s: the primer name %r has no _LEFT or _RIGHT field: which side of which amplicon is it?" % (row.where, row.name))


def amplicons(rows, region="insert"):
    """read_scheme's rows -> [Amplicon], ordered by (the chrom's first line in the file, full start, key).  Alternates merge:
    full = [min LEFT start, max RIGHT end), insert = [max LEFT end, min RIGHT start) — empty at its start when the primers overlap.
    The pool is column 5 of the amplicon's first row.  region: "insert", "full", or "unique" — the insert minus every other
    amplicon's full on the same chrom; of several pieces the longest (the first of equal longest); nothing left: empty at the
    insert's start.  PrimerBedError (file and line) for a name without a side, LEFT on '-' or RIGHT on '+', an amplicon without one
    of its sides, sides on different chroms."""
    if region not in REGIONS:
        raise ValueError("region is one of %s, not %r" % (", ".join(REGIONS), region))
    seen, chrom_order = {}, {}
    for r in rows:
        key, side = _side_of(r)
        if r.reverse != (side == "RIGHT"):
            raise PrimerBedError("%s: %r is a %s primer on the '%s' strand" % (r.where, r.name, side, "-" if r.reverse else "+"))
        chrom_order.setdefault(r.chrom, len(chrom_order))
        a = seen.setdefault(key, {"chrom": r.chrom, "pool": r.pool, "where": r.where, "LEFT": [], "RIGHT": []})
        if a["chrom"] != r.chrom:
            raise PrimerBedError("%s: %r lies on %r, the amplicon's other primers (%s) on %r" % (r.where, r.name, r.chrom, a["where"], a["chrom"]))
        a[side].append((r.start, r.end))
    built = []
    for key, a in seen.items():
        for side in ("LEFT", "RIGHT"):
            if not a[side]:
                raise PrimerBedError("%s: amplicon %r has no %s primer" % (a["where"], key, side))
        full = (min(s for s, _ in a["LEFT"]), max(e for _, e in a["RIGHT"]))
        ins = max(e for _, e in a["LEFT"])
        insert = (ins, max(ins, min(s for s, _ in a["RIGHT"])))
        built.append((chrom_order[a["chrom"]], full[0], key, a["chrom"], a["pool"], full, insert))
    built.sort(key=lambda b: b[:3])
    out = []
    for b in built:
        _, _, key, chrom, pool, full, insert = b
        if region == "full":
            iv = full
        elif region == "insert":
            iv = insert
        else:
            pieces = [insert]
            for o in built:
                if o is b or o[3] != chrom:
                    continue
                lo, hi = o[5]
                cut = []
                for s, e in pieces:
                    if hi <= s or lo >= e:
                        cut.append((s, e))
                        continue
                    if s < lo:
                        cut.append((s, lo))
                    if hi < e:
                        cut.append((hi, e))
                pieces = cut
            iv = (insert[0], insert[0])
            for s, e in pieces:                     # (in ascending order: the first of equal longest stays)
                if e - s > iv[1] - iv[0]:
                    iv = (s, e)
        out.append(Amplicon(chrom, key, pool, iv[0], iv[1]))
    return out


def amplicon_zones(rows):
    """read_scheme's rows -> [(fs, le, rs, fe)], one per amplicon in amplicons()' order (which does not depend on the region): fs the
    smallest LEFT start, le the largest LEFT end, rs the smallest RIGHT start, fe the largest RIGHT end — alternates merge as
    amplicons() merges them, and its errors are this function's.  le > rs (overlapping primers) is legal: what --amplicon-reads
    matches a read's two ends against."""
    sides = {}
    for r in rows:
        key, side = _side_of(r)
        z = sides.setdefault((r.chrom, key), {"LEFT": [], "RIGHT": []})
        z[side].append((r.start, r.end))
    out = []
    for m in amplicons(rows, "full"):
        z = sides[(m.chrom, m.name)]
        out.append((min(s for s, _ in z["LEFT"]), max(e for _, e in z["LEFT"]), min(s for s, _ in z["RIGHT"]), max(e for _, e in z["RIGHT"])))
    return out


def amplicons_for_layout(amps, names, shift):
    """A contig layout (names[t] starts at shift[t] on the axis; < 0: no slot) -> [(Amplicon, its slot's shift)] for the amplicons on
    contigs the layout holds, in the amplicons' order; the others are ignored (as rows_for_layout ignores their primers)."""
    at = {n: int(shift[t]) for t, n in enumerate(names) if int(shift[t]) >= 0}
    return [(a, at[a.chrom]) for a in amps if a.chrom in at]
