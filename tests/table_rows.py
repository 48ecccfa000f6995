"""The hand-written rows of tests/test_cli_tables.py: ONE set of variant records, a '*' and a '+' row among them, with strand, link,
evidence and indel counts that each add up to them — the rows of tests/test_strand_rule.py, test_links_rule.py and
test_evidence_rule.py at the four columns the link rows cover, and indel events made for them here — on their own reference, or
shifted into a slot of a longer axis.  No tests in here."""
import numpy as np

from tests import evidence_yardstick as ey
from tests import indel_yardstick as iy
from tests import links_yardstick as ly
from tests import strand_yardstick as sy
from tests import variant_yardstick as vy

REF = b"AAcNGTTGARtA"
COLS = (0, 2, 7, 10)
RECS = [(0, 2, 5, 20), (2, 4, 10, 40), (2, 5, 4, 40), (7, 1, 30, 100), (7, 6, 30, 100), (10, 5, 3, 12)]     # (pos, allele, count, cov); 5 '*', 6 '+'
#        column -> (fwd, rev) in plane order (coverage, A, T, C, G, X, I)
STRAND = {0: ((10, 8, 2, 0, 0, 0, 0), (10, 7, 3, 0, 0, 0, 0)),
          2: ((30, 0, 0, 20, 10, 0, 0), (10, 0, 0, 6, 0, 4, 0)),            # G on the forward strand only, X on the reverse only: BIAS twice
          7: ((50, 15, 15, 15, 5, 15, 15), (50, 15, 15, 15, 0, 15, 15)),
          10: ((6, 0, 6, 0, 0, 3, 3), (6, 0, 6, 0, 0, 0, 0))}               # 6 reads a strand: LOW under the default depth of 10
#        column -> (n, qual, mapq, dist) in plane order
EV = {0: ((20, 15, 5, 0, 0, 0, 0), (700, 600, 99, 0, 0, 0, 0), (1200, 900, 300, 0, 0, 0, 0), (200, 150, 25, 0, 0, 0, 0)),          # T: LOWQ
      2: ((40, 0, 0, 26, 10, 4, 0), (1400, 0, 0, 1000, 200, 160, 0), (2400, 0, 0, 1560, 199, 240, 0), (400, 0, 0, 300, 49, 8, 0)),  # G: LOWMQ, END; X: END
      7: ((100, 30, 15, 15, 5, 15, 30), (3000, 599, 15, 15, 101, 15, 600), (6000, 600, 15, 15, 301, 15, 599), (1000, 150, 15, 15, 26, 15, 149)),
      10: ((12, 0, 9, 0, 0, 3, 0), (400, 0, 300, 0, 0, 0, 0), (700, 0, 500, 0, 0, 0, 0), (100, 0, 80, 0, 0, 0, 0))}                # X, all sums 0: every name
# the classes of the records' tokens at a column (1..4 A, T, C, G; 5 X; 6 coverage alone), and per pair of columns
# {(class at the first, class at the second): records} — class 0: no token there; every pair's marginals are the columns' classes
CLASSES = {0: {1: 15, 2: 5}, 2: {3: 26, 4: 10, 5: 4}, 7: {1: 30, 4: 65, 6: 5}, 10: {2: 9, 5: 3}}
PAIRS = {(0, 2): {(2, 4): 5, (1, 3): 10, (1, 5): 2, (1, 0): 3, (0, 4): 5, (0, 5): 2, (0, 3): 16},
         (0, 7): {(1, 0): 15, (2, 0): 5, (0, 1): 30, (0, 4): 65, (0, 6): 5},
         (0, 10): {(1, 0): 15, (2, 0): 5, (0, 2): 9, (0, 5): 3},
         (2, 7): {(4, 1): 6, (4, 4): 4, (5, 1): 1, (5, 4): 1, (5, 0): 2, (3, 1): 3, (3, 4): 20, (3, 6): 1, (3, 0): 2, (0, 1): 20, (0, 4): 40, (0, 6): 4},
         (2, 10): {(3, 2): 6, (3, 0): 20, (4, 0): 10, (5, 0): 4, (0, 2): 3, (0, 5): 3},
         (7, 10): {(1, 5): 3, (1, 2): 1, (1, 0): 26, (4, 2): 8, (4, 0): 57, (6, 0): 5}}
# (pos, kind, len, bases, count, cov) in THE order: the insertions at 7 add up to the '+' row; the deletion at 10 runs past the reference
INDELS = [(2, iy.DEL, 3, "", 4, 40), (7, iy.INS, 1, "T", 12, 100), (7, iy.INS, 2, "AC", 18, 100), (10, iy.DEL, 4, "", 3, 12)]


def records(cols=COLS, shift=0):
    return vy.as_array([(p + shift, a, c, t) for p, a, c, t in RECS if p in cols])


def strand(cols=COLS, shift=0):
    return sy.records([c + shift for c in cols], [STRAND[c][0] for c in cols], [STRAND[c][1] for c in cols])


def evidence(cols=COLS, shift=0):
    return ey.records([c + shift for c in cols], [np.array([EV[c][k] for c in cols], np.int64).reshape(len(cols), 7) for k in range(4)])


def indel_rows(cols=COLS, shift=0):
    return [(p + shift,) + tuple(rest) for p, *rest in INDELS if p in cols]


def indels(rows):
    """indel_rows' rows (of several shifts, and others), sorted -> (events, text, totals) as Context.indel_events returns them: a total
    is the sum of the events of its kind on the column"""
    events, text = iy.arrays(rows)
    totals = {}
    for p, kind, _, _, n, _ in rows:
        totals.setdefault(p, [0, 0])[kind - 1] += n
    return events, text, iy.totals_at(totals, sorted(totals))


def axis_links(k, cols, hand):
    """the link records of the axis' columns `cols` (ascending) with k neighbours; hand = {column: (shift, column of COLS)} says which
    hold the hand-written rows.  Two of them under one shift: PAIRS.  A hand-written column and any other behind it: no record spans
    both — the first column's classes with no token at the second.  Anything else (and b = -1): zeros."""
    cols = list(cols)
    j = np.zeros((len(cols) * k, 7, 7), np.int32)
    for i, a in enumerate(cols):
        for d in range(1, k + 1):
            if i + d >= len(cols) or a not in hand:
                continue
            b = cols[i + d]
            if b in hand and hand[b][0] == hand[a][0]:
                for (x, y), v in PAIRS[(hand[a][1], hand[b][1])].items():
                    j[i * k + d - 1][x][y] = v
            else:
                for x, v in CLASSES[hand[a][1]].items():
                    j[i * k + d - 1][x][0] = v
    return ly.records(cols, k, j)


def links(k, cols=COLS, shift=0):
    return axis_links(k, [c + shift for c in cols], {c + shift: (shift, c) for c in cols})
