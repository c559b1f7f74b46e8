"""The shaped fit without a GPU: the parts of the numpy restatement (tests/fit_ref.py) against second methods -- axis runs
against a pixel scan, slots against ANDed rows, the breaker against `glyphs.flow`, the chosen candidate against a brute force
over every (candidate, n) -- what an OK row promises, the four ellipses of the issue's measurement, `glyphs.place_lines`
against the restatement's glyph-by-glyph placement, and the argument checks of `layout.fit_tables`.  The kernel itself is
compared with the restatement in tests/test_gpu_fit.py."""
import types

import numpy as np
import pytest

import fit_ref as FR
import layout_ref as LR
from conftest import pkg


def _planes():
    """(name, eroded plane, anchor (x, y)): the layout material at insets 0 and 2, ellipses and noise."""
    rng = np.random.default_rng(31)
    out = []
    for name, plane, anchor, _ in LR.material():
        if plane.size <= 70 * 70 * 4:
            for m in (0, 2):
                out.append((f"{name}@{m}", LR.erode(plane, m), anchor))
    for h, w in ((40, 60), (31, 97), (64, 64)):
        e = FR.ellipse(h, w)
        out.append((f"ellipse_{h}x{w}", e, (w // 2, h // 2)))
        out.append((f"ellipse_{h}x{w}_off", e & (rng.random((h, w)) < 0.995), (w // 3, h // 2)))
    return out


def _scan(plane, ax, y):
    """The run that contains (ax, y), pixel by pixel."""
    h, w = plane.shape
    if not (0 <= ax < w) or not plane[y, ax]:
        return None
    l, r = ax, ax + 1
    while l > 0 and plane[y, l - 1]:
        l -= 1
    while r < w and plane[y, r]:
        r += 1
    return l, r


def test_axis_runs_equal_a_pixel_scan():
    n = 0
    for name, plane, (ax, ay) in _planes():
        runs = FR.axis_runs(plane, ax)
        assert runs == [_scan(plane, ax, y) for y in range(plane.shape[0])], name
        n += sum(r is not None for r in runs)
    assert n > 1000


def test_a_slot_is_the_axis_run_of_the_anded_rows_made_symmetric():
    """The identity the kernel's table rests on: the run that contains ax of an AND of rows is the intersection of the rows'
    own axis runs, so max l / min r over the rows is that run."""
    seen = none = 0
    for name, plane, (ax, ay) in _planes():
        h, w = plane.shape
        if not 0 <= ax < w:
            continue
        runs = FR.axis_runs(plane, ax)
        for hh in (1, 2, 5, 13):
            for t in range(-1, h - hh + 2):
                got = FR.slot(runs, t, hh, ax)
                if t < 0 or t + hh > h:
                    assert got is None
                    continue
                run = _scan(plane[t:t + hh].all(axis=0)[None], ax, 0)
                if run is None:
                    assert got is None, (name, t, hh)
                    none += 1
                else:
                    half = min(ax - run[0], run[1] - ax)
                    assert got == (ax - half, 2 * half), (name, t, hh)
                    assert plane[t:t + hh, got[0]:got[0] + got[1]].all()
                    seen += 1
    assert seen > 2000 and none > 500


def _flow_starts(p, adv, width, h, g, breaks):
    """The line starts `glyphs.flow` gives the run in a box of `width`."""
    G = len(adv)
    atlas = types.SimpleNamespace(sizes=np.full((G, 2), h), advance=np.stack([adv, np.full((G,), h)], 1), bearing=np.zeros((G, 2), np.int64))
    xy, _ = p.glyphs.flow(np.arange(G), atlas, (0, 0, width, 10 ** 6), line=h, gap=g, breaks=breaks, align="left")
    ys = xy[:, 1]
    return [0] + [i for i in range(1, G) if ys[i] != ys[i - 1]]


def test_on_a_full_rectangle_the_lines_are_flows():
    """An all-ones plane with the anchor at its centre has the same slot on every line, so the stack's line starts are those
    of `glyphs.flow` in a box of the slot's width -- with and without a break table, with advances of 0."""
    p = pkg()
    rng = np.random.default_rng(5)
    done = 0
    for i in range(60):
        h, g = int(rng.integers(3, 9)), int(rng.integers(0, 4))
        G = int(rng.integers(1, 40))
        adv = rng.integers(0 if i % 3 == 0 else 1, 12, G)
        breaks = None if i % 2 else rng.random(G) < 0.4
        W, H = int(rng.integers(24, 90)), 400
        ax, ay = W // 2, H // 2
        row = FR.fit_row(np.ones((H, W), bool), (0, 0, W, H), (ax, ay), [np.concatenate([[0], np.cumsum(adv)])], [h], [g],
                         breaks=breaks, inset=0)
        width = 2 * min(ax, W - ax)
        if row["status"] != FR.OK:
            assert row["status"] == FR.NO_FIT
            continue
        recs = row["lines"][:row["n_lines"]]
        assert all(r[3] == width and r[1] == ax - width // 2 for r in recs)
        assert [r[0] for r in recs] == _flow_starts(p, adv, width, h, g, breaks)
        assert [r[2] for r in recs] == FR.stack_tops(ay, len(recs), h, g)
        done += 1
    assert done > 40


def _brute(inner, ax, ay, cums, lines, gaps, breaks):
    """{(c, n)} of the stacks that fit, by ANDed rows and a searchsorted breaker -- a second method."""
    H, W = inner.shape
    allowed = None if breaks is None else np.flatnonzero(breaks)
    out = set()
    for c, (cum, h, g) in enumerate(zip(cums, lines, gaps)):
        cum = np.asarray(cum, np.int64)
        G = len(cum) - 1
        for n in range(1, FR.MAX_LINES + 1):
            total = n * h + (n - 1) * g
            top = ay - (total >> 1)
            s, good = 0, True
            for k in range(n):
                t = top + k * (h + g)
                if s >= G or t < 0 or t + h > H:
                    good = False
                    break
                run = _scan(inner[t:t + h].all(axis=0)[None], ax, 0)
                if run is None:
                    good = False
                    break
                width = 2 * min(ax - run[0], run[1] - ax)
                end = min(int(np.searchsorted(cum, cum[s] + width, side="right")) - 1, G)
                if end <= s:
                    good = False
                    break
                if end < G and allowed is not None:
                    j = int(np.searchsorted(allowed, end - 1, side="right")) - 1
                    if j >= 0 and allowed[j] >= s:
                        end = int(allowed[j]) + 1
                s = end
            if good and s == G:
                out.add((c, n))
    return out


def test_ok_rows_keep_their_promises_and_the_candidate_is_the_brute_force_one():
    """Over ellipses, noise and the layout material, with several candidates: every slot of an OK row lies inside E_b and is
    symmetric about the anchor's column, every line's length is at most its width, the lines partition the run, and (cand,
    n_lines) is the largest candidate, and its smallest n, that a brute force over all (c, n) accepts; NO_FIT where it accepts
    none.  Candidates need not be monotone: a case where a middle candidate fails and a larger one fits is among them."""
    rng = np.random.default_rng(8)
    status = [0] * 5
    gaps_seen = 0
    for i, (name, inner, (ax, ay)) in enumerate(_planes()):
        H, W = inner.shape
        G = int(rng.integers(1, 30))
        sizes = [3, 4, 6, 8, 11]
        advs = [rng.integers(0, s + 1, G) for s in sizes]
        cums = [np.concatenate([[0], np.cumsum(a)]) for a in advs]
        lines, gaps = sizes, [i % 3] * len(sizes)
        breaks = None if i % 2 else rng.random(G) < 0.5
        row = FR.fit_row(inner, (10, 20, 10 + W, 20 + H), (ax + 10, ay + 20), cums, lines, gaps, breaks=breaks, inset=0)
        status[row["status"]] += 1
        if row["status"] == FR.NO_ANCHOR:
            assert not (0 <= ax < W and 0 <= ay < H and inner[ay, ax])
            continue
        accepted = _brute(inner, ax, ay, cums, lines, gaps, breaks)
        if row["status"] == FR.NO_FIT:
            assert not accepted, name
            continue
        c = max(a[0] for a in accepted)
        assert (row["cand"], row["n_lines"]) == (c, min(a[1] for a in accepted if a[0] == c)), name
        gaps_seen += len({a[0] for a in accepted}) < c + 1       # a smaller candidate that does not fit
        recs = row["lines"][:row["n_lines"]]
        assert row["lines"][row["n_lines"]:] == [[0] * 5] * (FR.MAX_LINES - row["n_lines"])
        starts = [r[0] for r in recs] + [G]
        assert starts[0] == 0 and all(b > a for a, b in zip(starts, starts[1:]))
        for (s, x1, y, width, length), e in zip(recs, starts[1:]):
            assert inner[y - 20: y - 20 + lines[c], x1 - 10: x1 - 10 + width].all() and y >= 20 and y + lines[c] <= 20 + H
            assert x1 - 10 + width // 2 == ax and width % 2 == 0
            assert length == cums[c][e] - cums[c][s] <= width
        assert row["n_inner"] == int(inner.sum())
    assert status[FR.OK] > 20 and status[FR.NO_ANCHOR] > 3 and status[FR.NO_FIT] > 3, status
    # not monotone: the middle candidate's tall lines pass the window, the larger one's advances are small
    inner = np.ones((12, 40), bool)
    row = FR.fit_row(inner, (0, 0, 40, 12), (20, 6), [np.arange(7) * 5, np.arange(7) * 6, np.arange(7) * 6], [4, 13, 5], [0, 0, 0], inset=0)
    assert (row["status"], row["cand"], row["n_lines"]) == (FR.OK, 2, 1)
    assert _brute(inner, 20, 6, [np.arange(7) * 5, np.arange(7) * 6, np.arange(7) * 6], [4, 13, 5], [0, 0, 0], None) == {(0, 1), (2, 1)}


class _Mono:
    """A monospace font for `glyphs.fit`: every advance and the line height are the size."""

    def metrics(self, gids, size, vertical=False):
        n = len(gids)
        return types.SimpleNamespace(sizes=np.full((n, 2), size), advance=np.full((n, 2), size), bearing=np.zeros((n, 2), np.int64),
                                     line=int(size))


ELLIPSES = (((120, 160), 40), ((100, 100), 30), ((160, 120), 60), ((90, 200), 50))


def ellipse_sizes(p):
    """Per ellipse (the size `glyphs.fit` picks in the largest rectangle, the shaped size), sizes 6 .. 40, monospace, gap 0,
    the region eroded by 2."""
    sizes = list(range(6, 41))
    out = []
    for (h, w), G in ELLIPSES:
        plane = FR.ellipse(h, w)
        _, rect = LR.best_rect(LR.erode(plane, 2))
        size, fits = p.glyphs.fit(np.zeros((G,), np.int64), _Mono(), rect, sizes)
        assert fits
        cums, lines, gaps = FR.mono_cums(G, sizes)
        row = FR.fit_row(plane, (0, 0, w, h), (w // 2, h // 2), cums[:16], lines[:16], gaps[:16], inset=2)
        best = sizes[row["cand"]] if row["status"] == FR.OK else 0
        for lo in range(16, len(sizes), 16):                 # 35 sizes, 16 candidates a call: the largest over the calls
            row = FR.fit_row(plane, (0, 0, w, h), (w // 2, h // 2), cums[lo:lo + 16], lines[lo:lo + 16], gaps[lo:lo + 16], inset=2)
            if row["status"] == FR.OK:
                best = max(best, sizes[lo + row["cand"]])
        out.append((size, best))
    return out


def test_the_shaped_size_beats_the_rectangle_on_the_four_ellipses():
    """Four elliptic balloons (window h x w, glyphs): 120 x 160 with 40, 100 x 100 with 30, 160 x 120 with 60, 90 x 200 with
    50; monospace advances (advance = size), gap 0, sizes 6 .. 40, the region eroded by 2.  `glyphs.fit` in the largest
    rectangle (`layout_ref.best_rect`) against the shaped fit about the centre.  Observed (rectangle, shaped): (14, 16),
    (11, 12), (11, 14), (11, 14): the shaped size is strictly larger on every one."""
    got = ellipse_sizes(pkg())
    print(f"\n(rectangle, shaped) sizes: {got}")
    assert all(shaped > rect for rect, shaped in got), got
    assert got == [(14, 16), (11, 12), (11, 14), (11, 14)]


def rows_table(p, dicts):
    """`fit_ref` rows as the kernel's table (`layout.FIT_ROW_DTYPE`)."""
    rows = np.zeros((len(dicts),), p.layout.FIT_ROW_DTYPE)
    for r, d in zip(rows, dicts):
        r["status"], r["cand"], r["n_lines"], r["n_inner"] = d["status"], d["cand"], d["n_lines"], d["n_inner"]
        r["lines"] = [tuple(x) for x in d["lines"]]
    return rows


def test_place_lines_equals_the_glyph_by_glyph_placement():
    """`glyphs.place_lines` over several blocks at once against `fit_ref.place` block by block, for the three alignments, with
    bearings; blocks that are not OK are left out; a run the fit was not made with is refused."""
    p = pkg()
    rng = np.random.default_rng(3)
    dicts, advs, bears = [], [], []
    for h, w, G in ((60, 90, 25), (40, 40, 9), (30, 30, 0), (80, 50, 31), (20, 200, 12)):
        adv = rng.integers(0, 9, G)
        cum = np.concatenate([[0], np.cumsum(adv)])
        dicts.append(FR.fit_row(FR.ellipse(h, w), (5, 7, 5 + w, 7 + h), (5 + w // 2, 7 + h // 2), [cum], [6], [1], inset=1))
        advs.append(adv), bears.append(rng.integers(-3, 4, (G, 2)))
    assert [d["status"] for d in dicts].count(FR.OK) >= 3 and dicts[2]["status"] == FR.NO_TEXT
    fit = p.layout.ShapedFit(np.zeros((5, 2), np.int32), rows_table(p, dicts), np.zeros((5, 2), np.int64), 1)
    ok = [j for j, d in enumerate(dicts) if d["status"] == FR.OK]
    assert fit.ok.tolist() == [d["status"] == FR.OK for d in dicts] and repr(fit).startswith("ShapedFit(5 blocks")
    count = [len(advs[j]) for j in ok]
    adv, bear = np.concatenate([advs[j] for j in ok]), np.concatenate([bears[j] for j in ok])
    for align in ("left", "center", "right"):
        want = np.concatenate([FR.place(dicts[j], advs[j], bears[j], align) for j in ok])
        assert np.array_equal(p.glyphs.place_lines(fit, count, adv, bear, align=align), want), align
    one = p.glyphs.place_lines(fit, [count[-1]], advs[ok[-1]], bears[ok[-1]], blocks=[ok[-1]])
    assert np.array_equal(one, FR.place(dicts[ok[-1]], advs[ok[-1]], bears[ok[-1]]))
    with pytest.raises(ValueError):
        p.glyphs.place_lines(fit, count, adv + 1, bear)
    with pytest.raises(ValueError):
        p.glyphs.place_lines(fit, [0], [], np.zeros((0, 2), np.int64), blocks=[2])
    with pytest.raises(ValueError):
        p.glyphs.place_lines(fit, count, adv, bear, align="justify")


def test_fit_tables_and_their_argument_checks():
    p = pkg()
    Y, L = p.layout, p._lib
    cum = [np.array([[0, 2, 4], [0, 3, 6]]), None, np.array([[0, 1], [0, 2]]), np.zeros((2, 1), np.int64)]
    jobs, cands, flat, brk = Y.fit_tables(cum, np.array([5, 7]), 1, breaks=[[True, False], None, [1], []])
    assert jobs["n_glyphs"].tolist() == [2, 0, 1, 0] and jobs["n_cands"].tolist() == [2, 0, 2, 2] and jobs["cand0"].tolist() == [0, 2, 2, 4]
    assert jobs["break0"].tolist() == [0, -1, 2, 3] and brk.tolist() == [1, 0, 1] and flat.tolist() == [0, 2, 4, 0, 3, 6, 0, 1, 0, 2, 0, 0]
    assert cands["cum0"].tolist() == [0, 3, 6, 8, 10, 11] and cands["gap"].tolist() == [1] * 6
    with pytest.raises(ValueError):                          # a shared array wants the same count everywhere
        Y.fit_tables(cum + [np.zeros((3, 1), np.int64)], np.array([5, 7]), 1)
    jobs, cands, _, _ = Y.fit_tables(cum[:3], np.array([5, 7]), [[0, 1], [], [2, 3]])
    assert cands["line"].tolist() == [5, 7, 5, 7] and cands["gap"].tolist() == [0, 1, 2, 3]
    for bad in ([np.array([[1, 2]])], [np.array([[0, 3, 2]])], [np.array([0, 1])], [np.array([[0.0, 1.0]])],
                [np.zeros((17, 2), np.int64)], [np.zeros((1, L.FIT_MAX_GLYPHS + 2), np.int64)], [np.array([[0, 2 ** 31]])]):
        with pytest.raises(ValueError):
            Y.fit_tables(bad, 5, 0)
    good = [np.array([[0, 1, 2]])]
    for line, gap in ((0, 0), (5, -1), (2.5, 0), (True, 0), ([[5, 6]], 0), (np.array([5, 6]), 0)):
        with pytest.raises(ValueError):
            Y.fit_tables(good, line, gap)
    for breaks in ([[True]], [[True, False]] * 2):
        with pytest.raises(ValueError):
            Y.fit_tables(good, 5, 0, breaks=breaks)
    assert (L.FIT_MAX_CANDS, L.FIT_MAX_LINES, FR.MAX_GLYPHS) == (FR.MAX_CANDS, FR.MAX_LINES, L.FIT_MAX_GLYPHS)
    assert [L.FIT_OK, L.FIT_NO_REGION, L.FIT_NO_TEXT, L.FIT_NO_ANCHOR, L.FIT_NO_FIT] == [FR.OK, FR.NO_REGION, FR.NO_TEXT, FR.NO_ANCHOR, FR.NO_FIT]
    assert Y.FIT_ROW_DTYPE.itemsize == 656 and Y.FIT_JOB_DTYPE.itemsize == 24 and Y.FIT_CAND_DTYPE.itemsize == 16
