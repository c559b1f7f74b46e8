"""The balanced breaker's restatement (tests/balance_ref.py) checked without a GPU: against an enumeration of every break
vector, against `fit_ref.fit_row` (only `start` and `length` may differ, the cost never rises), on the four elliptic balloons
of DESIGN.md section 4.32's table, and through `glyphs.place_lines`."""
import itertools

import numpy as np
import pytest

import balance_ref as BAL
import fit_ref as FR
import layout_ref as LR
from conftest import pkg
from test_fit_ref import rows_table


def _enumerate(cum, widths, breaks):
    """Every vector 0 = s_0 < s_1 < .. < s_n = G: the admissible one of least cost, among equals the lexicographically largest
    (s_1, .., s_(n-1)); None where none is admissible.  Also the number of admissible vectors that attain the least cost."""
    G, n = len(cum) - 1, len(widths)
    best, ties = None, 0
    for inner in itertools.combinations(range(1, G), n - 1):
        s = (0,) + inner + (G,)
        if any(breaks is not None and not breaks[e - 1] for e in inner):
            continue
        if any(cum[s[k + 1]] - cum[s[k]] > widths[k] for k in range(n)):
            continue
        key = (-sum((widths[k] - (cum[s[k + 1]] - cum[s[k]])) ** 2 for k in range(n)), inner)
        ties = 1 if best is None or key[0] > best[0] else ties + (key[0] == best[0])
        best = key if best is None or key > best else best
    if best is None:
        return None, 0
    s = (0,) + best[1] + (G,)
    return ([(s[k], s[k + 1]) for k in range(n)], -best[0]), ties


def test_the_restatement_equals_an_enumeration_of_every_break_vector():
    """G <= 10, n <= 4, random widths, advances with zeros and optional break tables, 3000 draws and hand-made ties: the
    lines and the cost are the enumeration's.  Ties that only the lexicographic rule decides and draws without an admissible
    vector both occur."""
    rng = np.random.default_rng(5)
    tied = none = some = 0
    draws = []
    for _ in range(3000):
        G, n = int(rng.integers(1, 11)), int(rng.integers(1, 5))
        adv = rng.integers(0, 5, G) * rng.integers(0, 2, G)              # about half of the advances are 0
        widths = [int(v) for v in rng.integers(1, 14, n)]
        breaks = None if rng.random() < 0.4 else rng.random(G) < 0.5
        draws.append((adv, widths, breaks))
    # monospace runs in equal slots: every way to hand out the spare room costs the same
    draws += [(np.full((G,), 2), [w] * n, None) for G, n, w in ((7, 3, 6), (9, 4, 6), (10, 4, 8), (6, 2, 10), (4, 4, 2))]
    draws += [(np.zeros((G,), np.int64), [3] * n, None) for G, n in ((5, 3), (10, 4), (4, 4), (3, 4))]
    for adv, widths, breaks in draws:
        cum = [0] + [int(v) for v in np.cumsum(adv)]
        want, ties = _enumerate(cum, widths, breaks)
        got = BAL.balanced(cum, widths, breaks)
        assert got == want, (cum, widths, breaks)
        none += want is None
        some += want is not None
        tied += ties > 1
        if want is not None:
            assert BAL.cost_of(cum, widths, want[0]) == want[1] < 2 ** 35
    assert tied >= 50 and none >= 200 and some >= 500, (tied, none, some)
    print(f"\n{len(draws)} draws: {some} with an answer, {tied} of them decided by the lexicographic rule, {none} without one")


def _blocks():
    """(plane, window, anchor, cums, lines, gaps, breaks, inset, balloon status): the layout material and ellipses with runs."""
    rng = np.random.default_rng(9)
    out = []
    for i, (name, plane, anchor, status) in enumerate(LR.material()):
        if plane.size > 70 * 70 * 4:
            continue
        h, w = plane.shape
        G = 30 if i % 3 else 8
        base = rng.integers(0, 7, G)
        cums = [np.concatenate([[0], np.cumsum(base * s // 6)]) for s in (3, 5, 8, 12)]
        brk = (None, BAL.word_breaks(G, rng), np.zeros((G,), bool))[i % 3]
        out.append((plane, (4, 6, 4 + w, 6 + h), (anchor[0] + 4, anchor[1] + 6), cums, [4, 6, 9, 13], [i % 2] * 4, brk, (0, 2)[i % 2],
                    status))
    for h, w, G in ((70, 110, 40), (60, 60, 25), (90, 50, 33)):
        base = rng.integers(1, 7, G)
        cums = [np.concatenate([[0], np.cumsum(base * s // 6)]) for s in (3, 5, 8, 12)]
        for brk in (None, BAL.word_breaks(G, rng)):
            out.append((FR.ellipse(h, w), (0, 0, w, h), (w // 2, h // 2), cums, [4, 6, 9, 13], [1] * 4, brk, 2, 0))
    return out


def test_only_start_and_length_differ_and_the_cost_never_rises():
    """On every block status, cand, n_lines, n_inner and every record's x1, y and width are `fit_ref.fit_row`'s; the lines
    are admissible, hold the run and cost at most what the greedy lines cost; a block that is not OK is all 0; where the
    greedy lines stand no vector is admissible, so the greedy stack took a hard break."""
    improved = stood = 0
    for plane, win, anchor, cums, lines, gaps, brk, inset, status in _blocks():
        greedy = FR.fit_row(plane, win, anchor, cums, lines, gaps, breaks=brk, inset=inset, balloon_status=status)
        row, bal = BAL.balance_row(plane, win, anchor, cums, lines, gaps, breaks=brk, inset=inset, balloon_status=status)
        assert [row[k] for k in FR.FIELDS[:4]] == [greedy[k] for k in FR.FIELDS[:4]]
        assert [r[1:4] for r in row["lines"]] == [r[1:4] for r in greedy["lines"]]
        if row["status"] != FR.OK:
            assert row == greedy and bal == dict(balanced=0, cost=0)
            continue
        n, cum = row["n_lines"], [int(v) for v in cums[row["cand"]]]
        G = len(cum) - 1
        recs, grecs = row["lines"][:n], greedy["lines"][:n]
        greedy_cost = sum((r[3] - r[4]) ** 2 for r in grecs)
        starts = [r[0] for r in recs] + [G]
        assert starts[0] == 0 and all(a < b for a, b in zip(starts, starts[1:]))
        assert all(r[4] == cum[e] - cum[r[0]] <= r[3] for r, e in zip(recs, starts[1:]))
        assert bal["cost"] == sum((r[3] - r[4]) ** 2 for r in recs) <= greedy_cost
        assert sum(r[3] - r[4] for r in recs) == sum(r[3] - r[4] for r in grecs)      # the slack only moves
        if bal["balanced"]:
            assert all(brk is None or brk[e - 1] for e in starts[1:-1])
            improved += bal["cost"] < greedy_cost
        else:
            assert recs == grecs and brk is not None and any(not brk[e - 1] for e in starts[1:-1])
            stood += 1
    assert improved >= 3 and stood >= 1, (improved, stood)


# window (h, w), glyphs -> size, greedy slack per line, balanced slack per line
ELLIPSES = [((120, 160, 40), 20, [32, 26, 6, 52], [32, 26, 36, 22]),
            ((100, 100, 30), 15, [25, 48, 34, 11], [25, 48, 34, 11]),
            ((160, 120, 60), 16, [26, 0, 18, 18, 48, 26], [26, 48, 18, 2, 16, 26]),
            ((90, 200, 50), 16, [8, 56, 48], [8, 56, 48])]
SIZES = [6, 8, 10, 11, 12, 13, 14, 15, 16, 18, 20, 24]


def ellipse_cases():
    """The four elliptic balloons with word break tables drawn in order from one generator: advance = size // 2, line
    height = size, gap 0, inset 2, the anchor at the window's centre."""
    rng = np.random.default_rng(0)
    out = []
    for (h, w, G), _, _, _ in ELLIPSES:
        br = BAL.word_breaks(G, rng)
        cums = [np.arange(G + 1) * (s // 2) for s in SIZES]
        out.append((FR.ellipse(h, w), (0, 0, w, h), (w // 2, h // 2), cums, list(SIZES), [0] * len(SIZES), br))
    return out


def test_the_four_ellipses_of_the_table():
    """Strictly better on the 120 x 160 and 160 x 120 balloons, the greedy lines on the other two, at the same size and line
    count; the slacks are the table's."""
    for (plane, win, anchor, cums, lines, gaps, br), (_, size, g_slack, b_slack) in zip(ellipse_cases(), ELLIPSES):
        greedy = FR.fit_row(plane, win, anchor, cums, lines, gaps, breaks=br, inset=2)
        row, bal = BAL.balance_row(plane, win, anchor, cums, lines, gaps, breaks=br, inset=2)
        n = row["n_lines"]
        assert row["status"] == FR.OK and SIZES[row["cand"]] == size and n == len(g_slack) == greedy["n_lines"]
        assert [r[3] - r[4] for r in greedy["lines"][:n]] == g_slack
        assert [r[3] - r[4] for r in row["lines"][:n]] == b_slack
        assert bal == dict(balanced=1, cost=sum(x * x for x in b_slack))
        assert (bal["cost"] < sum(x * x for x in g_slack)) == (g_slack != b_slack)
        assert (row == greedy) == (g_slack == b_slack)


def test_place_lines_accepts_balanced_records():
    """`glyphs.place_lines` on balanced rows: its length check holds, and the positions are `fit_ref.place`'s."""
    p = pkg()
    rows, advs = [], []
    for plane, win, anchor, cums, lines, gaps, br in ellipse_cases():
        row, _ = BAL.balance_row(plane, win, anchor, cums, lines, gaps, breaks=br, inset=2)
        rows.append(row)
        advs.append(np.diff(cums[row["cand"]]))
    fit = p.layout.ShapedFit(np.zeros((4, 2), np.int32), rows_table(p, rows), np.zeros((4, 2), np.int64), 2)
    assert not fit.balanced.any() and not fit.cost.any() and fit.bal_rows is None      # no balance table was given
    bears = [np.zeros((len(a), 2), np.int64) for a in advs]
    for align in ("left", "center", "right"):
        want = np.concatenate([FR.place(r, a, b, align) for r, a, b in zip(rows, advs, bears)])
        got = p.glyphs.place_lines(fit, [len(a) for a in advs], np.concatenate(advs), np.concatenate(bears), align=align)
        assert np.array_equal(got, want), align
    bal = np.zeros((4,), p.layout.FIT_BALANCE_DTYPE)
    bal["balanced"], bal["cost"] = [1, 0, 1, 0], [5, 0, 2 ** 34, 0]
    fit = p.layout.ShapedFit(np.zeros((4, 2), np.int32), rows_table(p, rows), np.zeros((4, 2), np.int64), 2, bal)
    assert fit.balanced.tolist() == [True, False, True, False] and fit.cost.tolist() == [5, 0, 2 ** 34, 0]
    with pytest.raises(ValueError):
        p.layout.ShapedFit(np.zeros((4, 2), np.int32), rows_table(p, rows), np.zeros((4, 2), np.int64), 2, bal[:3])
