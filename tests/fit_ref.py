"""numpy restatement of the shaped-fit rule (include/ctd_hip.h, "shaped fit"): per block with a balloon region, the region
eroded by `inset`, the axis run of every row, the slot of every line of a stack, `glyphs.flow`'s greedy breaker with the
slot's width for the box's, and the largest candidate that has a stack that fits.  Written from the rule's statement,
straightforward and slow: the axis runs come from the positions of a row's zeros, a slot from the max / min of its rows'
runs, and the breaker adds advances glyph by glyph -- nothing like the kernel's bit scans, its int16 table and its binary
search in the cumulative advances (csrc/kernels_fit.hip).  The kernel is compared with `fit_row` field by field
(tests/test_gpu_fit.py); tests/test_fit_ref.py holds the parts against a pixel scan, ANDed rows, `glyphs.flow` and a brute
force over every (candidate, n)."""
import numpy as np

import balloon_ref as BR
from layout_ref import MAX_INSET, erode, material  # noqa: F401  (the planes and the erosion are the layout rule's)

OK, NO_REGION, NO_TEXT, NO_ANCHOR, NO_FIT = range(5)
MAX_CANDS, MAX_LINES, MAX_GLYPHS = 16, 32, 4096
FIELDS = ("status", "cand", "n_lines", "n_inner", "lines")


def axis_runs(inner, ax):
    """Per row of the plane (l, r), the maximal run [l, r) of ones that contains column ax, or None."""
    inner = np.asarray(inner, bool)
    h, w = inner.shape
    out = []
    for y in range(h):
        if not (0 <= ax < w) or not inner[y, ax]:
            out.append(None)
            continue
        zeros = np.flatnonzero(~inner[y])
        left, right = zeros[zeros < ax], zeros[zeros > ax]
        out.append((int(left[-1]) + 1 if len(left) else 0, int(right[0]) if len(right) else w))
    return out


def slot(runs, t, h, ax):
    """(x1, width) of the slot of top row t at height h, or None: rows t .. t + h - 1 inside the plane, each with a run."""
    if t < 0 or t + h > len(runs) or any(runs[y] is None for y in range(t, t + h)):
        return None
    L = max(runs[y][0] for y in range(t, t + h))
    R = min(runs[y][1] for y in range(t, t + h))
    half = min(ax - L, R - ax)
    return ax - half, 2 * half


def stack_tops(ay, n, h, g):
    total = n * h + (n - 1) * g
    top = ay - (total >> 1)
    return [top + k * (h + g) for k in range(n)]


def greedy(cum, widths, breaks=None):
    """The breaker over the lines' widths, glyph by glyph: [(start, end)] of len(widths) lines that hold all the glyphs, none of
    them empty, or None (a first glyph that does not fit, glyphs left over, a line left empty)."""
    G = len(cum) - 1
    lines, s = [], 0
    for width in widths:
        if s >= G:
            return None
        end, used = s, 0
        while end < G and used + (cum[end + 1] - cum[end]) <= width:
            used += cum[end + 1] - cum[end]
            end += 1
        if end == s:
            return None
        if end < G and breaks is not None:
            allowed = [j for j in range(s, end) if breaks[j]]
            if allowed:
                end = allowed[-1] + 1
        lines.append((s, end))
        s = end
    return lines if s == G else None


def try_stack(runs, ax, ay, cum, h, g, n, breaks=None):
    """The lines [(start, x1, top, width, length)] of the stack of n lines in window coordinates, or None where it does not fit."""
    tops = stack_tops(ay, n, h, g)
    slots = [slot(runs, t, h, ax) for t in tops]
    if any(s is None for s in slots):
        return None
    placed = greedy(cum, [s[1] for s in slots], breaks)
    if placed is None:
        return None
    return [(s, sl[0], t, sl[1], int(cum[e] - cum[s])) for (s, e), sl, t in zip(placed, slots, tops)]


def _zero_row(status):
    return dict(status=status, cand=0, n_lines=0, n_inner=0, lines=[[0] * 5 for _ in range(MAX_LINES)])


def fit_row(region, win, anchor, cums, lines, gaps, breaks=None, inset=2, balloon_status=BR.OK, max_words=BR.MAX_WORDS):
    """The row of one block.  region: B_b as a boolean (wh, ww) plane over the window `win` = (wx1, wy1, wx2, wy2) (ignored
    where `balloon_status` is not OK); anchor: (x, y) in page coordinates; cums[c]: the run's G + 1 cumulative advances at
    candidate c, lines[c] and gaps[c] its line height and gap; breaks: one truth value per glyph, or None."""
    if not 0 <= inset <= MAX_INSET:
        raise ValueError("inset 0..16")
    cums = [[int(v) for v in c] for c in cums]
    if len(cums) > MAX_CANDS or len(lines) != len(cums) or len(gaps) != len(cums):
        raise ValueError("at most 16 candidates, a line height and a gap each")
    if any(h < 1 for h in lines) or any(g < 0 for g in gaps):
        raise ValueError("line >= 1, gap >= 0")
    G = len(cums[0]) - 1 if cums else 0
    if G > MAX_GLYPHS or any(len(c) != G + 1 or c[0] != 0 or any(b < a for a, b in zip(c, c[1:])) for c in cums):
        raise ValueError("cumulative advances: G + 1 of them, from 0, not decreasing")
    if balloon_status != BR.OK or BR.n_words(win)[1] > max_words:
        return _zero_row(NO_REGION)
    if G == 0 or not cums:
        return _zero_row(NO_TEXT)
    wx1, wy1, wx2, wy2 = win
    ww, wh = max(wx2 - wx1, 0), max(wy2 - wy1, 0)
    inner = erode(np.asarray(region, bool).reshape(wh, ww), inset)
    ax, ay = int(anchor[0]) - wx1, int(anchor[1]) - wy1
    if not (0 <= ax < ww and 0 <= ay < wh and inner[ay, ax]):
        return _zero_row(NO_ANCHOR)
    runs = axis_runs(inner, ax)
    for c in range(len(cums) - 1, -1, -1):
        for n in range(1, MAX_LINES + 1):
            got = try_stack(runs, ax, ay, cums[c], lines[c], gaps[c], n, breaks)
            if got is not None:
                recs = [[s, x1 + wx1, t + wy1, w, ln] for s, x1, t, w, ln in got] + [[0] * 5 for _ in range(MAX_LINES - n)]
                return dict(status=OK, cand=c, n_lines=n, n_inner=int(inner.sum()), lines=recs)
    return _zero_row(NO_FIT)


def row_dict(row):
    """A record of the kernel's result table as the dict `fit_row` returns."""
    out = {k: int(row[k]) for k in FIELDS[:4]}
    out["lines"] = [[int(r[f]) for f in ("start", "x1", "y", "width", "length")] for r in row["lines"]]
    return out


def place(row, adv, bearing, align="center"):
    """Glyph positions (G, 2) of an OK row: a glyph goes to (slot x1 + shift + pen + bearing_x, line top + bearing_y), the
    shift "left" 0, "center" slack >> 1, "right" the slack, as `glyphs.flow` shifts a line in its box."""
    adv, bearing = [int(a) for a in adv], np.asarray(bearing, np.int64).reshape(-1, 2)
    xy = np.zeros((len(adv), 2), np.int64)
    recs = row["lines"][:row["n_lines"]]
    ends = [r[0] for r in recs[1:]] + [len(adv)]
    for (s, x1, top, width, length), e in zip(recs, ends):
        slack = width - length
        pen = x1 + {"left": 0, "center": slack >> 1, "right": slack}[align]
        for i in range(s, e):
            xy[i] = (pen + bearing[i, 0], top + bearing[i, 1])
            pen += adv[i]
    return xy


def ellipse(h, w):
    """The pixels whose centres lie inside the ellipse inscribed in an (h, w) window."""
    ys, xs = np.mgrid[:h, :w].astype(np.int64)
    return (2 * xs + 1 - w) ** 2 * h * h + (2 * ys + 1 - h) ** 2 * w * w <= w * w * h * h


def mono_cums(G, sizes):
    """Monospace runs: advance = size.  ([cum per size], line heights, gaps of 0)"""
    return [np.arange(G + 1) * s for s in sizes], list(sizes), [0] * len(sizes)
