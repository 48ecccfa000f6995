"""Primer schemes as BED files (the format of ARTIC's *.primer.bed, `ivar trim -b`, `samtools ampliconclip -b`).

Columns: chrom, start, end, name, score / pool, strand — tab or blank separated, 0-based and end-exclusive.  Lines that start with
`#`, `track` or `browser` and blank lines are ignored; anything else that does not parse is an error that names its line."""


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
