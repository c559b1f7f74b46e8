"""Font colours without a GPU: the rule's own promises on its numpy restatement (tests/color_ref.py), the pooling / apply
arithmetic of `colors.LineColors` on hand-made columns, argument checks, and the layout of the two ABI structs against the
header.  The kernel itself is compared with the restatement in tests/test_gpu_colors.py."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import color_ref as R
from conftest import ROOT, pkg


# ---- the rule ----------------------------------------------------------------------------------------------------------

def test_flat_pages_give_back_their_two_colours_exactly():
    """Two-colour pages with bar glyphs (a red / green pair among them), tight mask and mask dilated by 2, axis-aligned quad,
    reversed winding, tilted quad, quads that leave the page: fill and surround are exactly the two colours, status OK."""
    n = 0
    for page, mask, quad, text, back in R.flat_cases():
        r = R.line_color(page, mask, quad)
        assert r["status"] == R.OK, (quad, text, back, r)
        assert r["fg"] == text and r["bg"] == back, (quad, text, back, r)
        assert r["n_fg"] >= 1 and r["n_bg"] >= 1 and r["n_on"] >= r["n_fg"]
        n += 1
    assert n == len(R.FLAT_COLOURS) * 2 * len(R.FLAT_QUADS)
    # the two windings select the same pixels
    page, mask = R.flat_page(*R.FLAT_COLOURS[0])
    assert R.line_color(page, mask, R.FLAT_QUADS[0]) == R.line_color(page, mask, R.FLAT_QUADS[1])
    # the dilated mask holds background under it and the fill still comes from the glyphs alone
    r = R.line_color(page, R.dilate(mask, 2), R.FLAT_QUADS[0])
    assert r["n_on"] > r["n_fg"] == R.line_color(page, mask, R.FLAT_QUADS[0])["n_fg"]


def test_status_cases():
    page, mask = R.flat_page((20, 30, 40), (200, 210, 220))
    q = R.FLAT_QUADS[0]
    r = R.line_color(page, np.zeros_like(mask), q)
    assert r["status"] == R.NO_MASK and r["n_on"] == 0 and r["n_off"] == 27 * 141 and r["g_off"] > 0
    assert r["fg"] == r["bg"] == r["s_fg"] == r["s_bg"] == [0, 0, 0] and r["n_fg"] == r["n_bg"] == 0
    r = R.line_color(page, np.full_like(mask, 255), q)
    assert r["status"] == R.NO_CONTRAST and r["n_off"] == 0 and r["n_fg"] == r["n_on"] == 27 * 141 and r["n_bg"] == 0
    assert r["bg"] == r["fg"] and r["fg"] == R._mean(page[12:39, 10:151].reshape(-1, 3).astype(np.int64).sum(0), 27 * 141)
    for out in ([-50, -40, -10, -40, -10, -5, -50, -5], [200, 10, 260, 10, 260, 40, 200, 40], [10, 96, 60, 96, 60, 140, 10, 140]):
        r = R.line_color(page, mask, out)
        assert r["status"] == R.EMPTY and all(r[k] in (0, [0, 0, 0]) for k in R.FIELDS if k != "status")
    # one point: that pixel's colour, fill = surround
    r = R.line_color(page, mask, [13, 20] * 4)
    assert mask[20, 13] and r["status"] == R.NO_CONTRAST and r["n_on"] == 1 and r["fg"] == r["bg"] == [20, 30, 40]
    assert R.line_color(page, mask, [11, 20] * 4)["status"] == R.NO_MASK          # the same on a background pixel
    # means tie with both classes present: fill = mean under the mask, surround = mean off it
    grey_page = np.full((40, 60, 3), 90, np.uint8)
    m = np.zeros((40, 60), np.uint8)
    m[10:20, 10:30] = 255
    r = R.line_color(grey_page, m, [5, 5, 50, 5, 50, 30, 5, 30])
    assert r["status"] == R.NO_CONTRAST and r["n_fg"] == 200 and r["n_bg"] == 46 * 26 - 200 and r["fg"] == r["bg"] == [90, 90, 90]
    # the cap: decided from the quad and the declared page size, before a pixel is looked at
    big = np.lib.stride_tricks.as_strided(np.zeros((1, 1, 3), np.uint8), (4097, 4096, 3), (0, 0, 1))
    bigm = np.lib.stride_tricks.as_strided(np.zeros((1, 1), np.uint8), (4097, 4096), (0, 0))
    r = R.line_color(big, bigm, [0, 0, 4095, 0, 4095, 4096, 0, 4096])
    assert r["status"] == R.TOO_LARGE and all(r[k] in (0, [0, 0, 0]) for k in R.FIELDS if k != "status")
    assert R.line_color(big, bigm, [-5, -5, 5000, -5, 5000, 5000, -5, 5000])["status"] == R.TOO_LARGE
    assert R.line_color(page, mask, [0, 0, R.MAX_COORD + 1, 0, 50, 50, 0, 50])["status"] == R.TOO_LARGE
    assert R.line_color(page, mask, [0, 0, R.MAX_COORD, 0, 50, 50, 0, 50])["status"] == R.OK


def test_random_pages_ok_means_both_classes_and_the_two_text_like_forms_agree():
    """300 seeded random 20 x 30 pages, random masks, jittered quads: status OK implies n_fg >= 1 and n_bg >= 1, and the
    distance form and the single-threshold form of 'text-like' select the same greys."""
    rng = np.random.default_rng(5)
    seen = set()
    for case in range(300):
        page = rng.integers(0, 256, (20, 30, 3), dtype=np.uint8)
        if case % 3 == 0:                                    # few grey levels: ties and near-ties between the means
            page = (page // 128 * 100 + 20).astype(np.uint8)
        mask = (rng.random((20, 30)) < rng.choice([0.05, 0.3, 0.5, 0.9])).astype(np.uint8) * rng.integers(1, 256, dtype=np.uint8)
        x0, y0, w, h = int(rng.integers(-3, 20)), int(rng.integers(-3, 12)), int(rng.integers(1, 16)), int(rng.integers(1, 12))
        quad = (np.array([[x0, y0], [x0 + w, y0], [x0 + w, y0 + h], [x0, y0 + h]]) + rng.integers(-2, 3, (4, 2))).reshape(8)
        r = R.line_color(page, mask, quad)
        seen.add(r["status"])
        assert r["n_on"] + r["n_off"] >= r["n_bg"] + r["n_fg"]
        if r["status"] == R.OK:
            assert r["n_fg"] >= 1 and r["n_bg"] >= 1, (case, r)
        if r["n_on"] and r["n_off"]:
            args = (r["n_on"], r["n_off"], r["g_on"], r["g_off"])
            g = np.arange(256)
            assert np.array_equal(R.text_like_distance(g, *args), R.text_like_threshold(g, *args)), (case, args)
    assert R.OK in seen and len(seen) >= 2
    # the two forms at the bounds of the arithmetic: 2^24 pixels of the extreme greys
    for args in ((1 << 23, 1 << 23, 255 << 23, 0), (1, (1 << 24) - 1, 0, 255 * ((1 << 24) - 1)), (3, 5, 3 * 77, 5 * 77 + 1),
                 ((1 << 24) - 1, 1, 100 * ((1 << 24) - 1) + 1, 100)):
        g = np.arange(256)
        assert np.array_equal(R.text_like_distance(g, *args), R.text_like_threshold(g, *args)), args


# ---- the Python layer ------------------------------------------------------------------------------------------------------

def _rows(p, recs):
    rows = np.zeros((len(recs),), p.colors.OUT_DTYPE)
    for i, r in enumerate(recs):
        for k, v in r.items():
            rows[k][i] = v
    return rows


def _blk(p, n_lines, **kw):
    return p.textblock.TextBlock([0, 0, 50, 50], lines=[[[0, 10 * i], [50, 10 * i], [50, 10 * i + 8], [0, 10 * i + 8]]
                                                         for i in range(n_lines)], **kw)


def test_line_colors_pooling_and_apply_on_hand_made_columns():
    p = pkg()
    L = p._lib
    recs = [  # page 0 block 0: a long and a short line (sums in BGR); block 1: only invalid lines; page 1 block 0: no contrast
        dict(status=L.COLOR_OK, n_fg=100, s_fg=[1000, 2000, 3000], n_bg=300, s_bg=[60000, 60300, 60600], fg=[10, 20, 30], bg=[200, 201, 202]),
        dict(status=L.COLOR_OK, n_fg=7, s_fg=[700, 700, 701], n_bg=10, s_bg=[1000, 1004, 1005], fg=[100, 100, 100], bg=[100, 100, 101]),
        dict(status=L.COLOR_NO_MASK, n_off=50, g_off=999),
        dict(status=L.COLOR_EMPTY),
        dict(status=L.COLOR_TOO_LARGE),
        dict(status=L.COLOR_NO_MASK, n_fg=9, s_fg=[9, 9, 9]),        # sums of a line that is not pooled must not count
        dict(status=L.COLOR_NO_CONTRAST, n_fg=4, s_fg=[40, 80, 122], n_bg=0, fg=[10, 20, 31], bg=[10, 20, 31], n_on=4),
    ]
    index = [(0, 0, 0), (0, 0, 1), (0, 1, 0), (0, 1, 1), (0, 1, 2), (0, 1, 3), (1, 0, 0)]
    lc = p.colors.LineColors(index, _rows(p, recs))
    assert len(lc) == 7 and lc.fg.dtype == np.uint8 and lc.fg[0].tolist() == [30, 20, 10] and lc.bg[1].tolist() == [101, 100, 100]
    bc = lc.blocks()
    assert bc.index.tolist() == [[0, 0], [0, 1], [1, 0]] and bc.valid.tolist() == [True, False, True]
    mean = lambda s, n: (2 * s + n) // (2 * n)                   # noqa: E731
    want_fg = [mean(3000 + 701, 107), mean(2000 + 700, 107), mean(1000 + 700, 107)]          # RGB
    want_bg = [mean(60600 + 1005, 310), mean(60300 + 1004, 310), mean(60000 + 1000, 310)]
    assert bc.fg[0].tolist() == want_fg and bc.bg[0].tolist() == want_bg
    assert bc.fg[1].tolist() == bc.bg[1].tolist() == [0, 0, 0]
    assert bc.fg[2].tolist() == [31, 20, 10] and bc.bg[2].tolist() == [31, 20, 10]            # 122 / 4 = 30.5 rounds up
    for rows, j in ((recs[:2], 0), (recs[2:6], 1), (recs[6:], 2)):                             # the restatement's pooling
        full = [{**dict(status=0, n_fg=0, s_fg=[0, 0, 0], n_bg=0, s_bg=[0, 0, 0]), **r} for r in rows]
        ok, fg, bg = R.pooled(full)
        assert (ok, fg, bg) == (bool(bc.valid[j]), bc.fg[j].tolist(), bc.bg[j].tolist())

    pages = [[_blk(p, 2), _blk(p, 4, fg_r=1)], (None, None, [_blk(p, 1)])]                     # a list and a result triple
    assert pages[0][0].stroke_width == 0
    got = lc.apply(pages)
    assert got.index.tolist() == bc.index.tolist()
    a, b, c = pages[0][0], pages[0][1], pages[1][2][0]
    fg, bg = a.get_font_colors()
    assert fg.tolist() == want_fg and bg.tolist() == want_bg and a.accumulate_color is True
    assert [a.fg_r, a.fg_g, a.fg_b] == [2 * v for v in want_fg]                                # sums over the lines, as the reference stores them
    fg_bgr, _ = a.get_font_colors(bgr=True)
    assert fg_bgr.tolist() == want_fg[::-1]
    assert a.stroke_width == a.default_stroke_width == 0.2                                     # the colours differ by more than 40
    # a block without a valid line stays as it was
    assert [b.fg_r, b.fg_g, b.fg_b, b.bg_r, b.bg_g, b.bg_b] == [1, 0, 0, 0, 0, 0]
    fresh = _blk(p, 3)
    assert [fresh.fg_r, fresh.fg_g, fresh.fg_b, fresh.bg_r, fresh.bg_g, fresh.bg_b] == [0] * 6 and fresh.stroke_width == 0
    fg, bg = c.get_font_colors()
    assert fg.tolist() == bg.tolist() == [31, 20, 10] and c.stroke_width == 0                  # equal colours: no stroke
    # 40 is the last difference without a stroke
    d = _blk(p, 1)
    d.set_font_colors([100, 100, 100], [120, 110, 90], accumulate=True)
    assert d.stroke_width == 0
    d.set_font_colors([100, 100, 100], [121, 110, 90], accumulate=True)
    assert d.stroke_width == d.default_stroke_width
    # the JSON record carries them
    rec = __import__("json").loads(p.annotations.blocks_json([a]))[0]
    assert [rec["fg_r"], rec["fg_g"], rec["fg_b"]] == [2 * v for v in want_fg]

    empty = p.colors.LineColors(np.zeros((0, 3), np.int32), np.zeros((0,), p.colors.OUT_DTYPE))
    assert len(empty) == 0 and len(empty.blocks().valid) == 0 and empty.apply([]).index.shape == (0, 2)


def test_line_colors_argument_checks_need_no_gpu():
    p = pkg()
    page, mask = np.zeros((20, 30, 3), np.uint8), np.zeros((20, 30), np.uint8)
    blk = _blk(p, 1)
    for pg, mk in ((page[:, :, 0], mask), (page.astype(np.int32), mask), (page, mask[:, :29]), (page, mask.astype(bool)),
                   (np.zeros((20, 30, 1), np.uint8), mask), (page, np.zeros((20, 30, 1), np.uint8))):
        with pytest.raises(ValueError):
            p.colors.line_colors([pg], [mk], [[blk]])
    with pytest.raises(ValueError):
        p.colors.line_colors([page], [mask, mask], [[blk]])
    with pytest.raises(ValueError):
        p.colors.line_colors([page], [mask], [])
    none = p.colors.line_colors([page], [mask], [[]])                        # no line: nothing to launch
    assert len(none) == 0 and none.fg.shape == (0, 3)
    import torch
    if not torch.cuda.is_available():
        with pytest.raises(p._lib.CtdError):
            p.colors.line_colors([page], [mask], [[blk]])


def test_detect_stream_rejects_lazy_with_font_colors_before_any_work():
    """The check is the first statement of the generator: no pool, no GPU needed to see it."""
    p = pkg()
    det = object.__new__(p.detector.TextDetector)
    with pytest.raises(ValueError):
        next(p.detector.TextDetector.detect_stream(det, [], lazy=True, font_colors=True))


# ---- ABI -------------------------------------------------------------------------------------------------------------------

def test_color_structs_have_the_c_layout():
    """`colors.JOB_DTYPE` / `OUT_DTYPE` and `_lib.CtdColorJob` / `CtdLineColor` against the header, compiled: sizes and every
    field's offset; the constants."""
    p = pkg()
    L, CO = p._lib, p.colors
    jf = ("page_dev", "mask_dev", "H", "W", "pitch", "mask_pitch", "quad")
    of = ("n_fg", "s_fg", "n_bg", "s_bg", "g_on", "g_off", "n_on", "n_off", "status", "fg", "bg", "pad_")
    prog = ('#include <stdio.h>\n#include <stddef.h>\n#include "ctd_hip.h"\nint main(void){ printf("%zu %zu", '
            'sizeof(ctd_color_job), sizeof(ctd_line_color));\n' +
            "".join(f'printf(" %zu", offsetof(ctd_color_job, {f}));\n' for f in jf) +
            "".join(f'printf(" %zu", offsetof(ctd_line_color, {f}));\n' for f in of) +
            'printf(" %d %d %d %d %d %d %d %d\\n", CTD_COLOR_OK, CTD_COLOR_EMPTY, CTD_COLOR_NO_MASK, CTD_COLOR_NO_CONTRAST, '
            'CTD_COLOR_TOO_LARGE, CTD_COLOR_MAX_PIXELS, CTD_COLOR_MAX_COORD, CTD_ABI_VERSION); return 0; }\n')
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c")
        open(c, "w").write(prog)
        exe = os.path.join(d, "t")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        vals = [int(v) for v in subprocess.check_output([exe]).split()]
    J, O = L.CtdColorJob, L.CtdLineColor
    assert vals[:2] == [C.sizeof(J), C.sizeof(O)] == [CO.JOB_DTYPE.itemsize, CO.OUT_DTYPE.itemsize] == [64, 104]
    assert vals[2:2 + len(jf)] == [getattr(J, f).offset for f in jf] == [CO.JOB_DTYPE.fields[f][1] for f in jf]
    assert vals[9:9 + len(of)] == [getattr(O, f).offset for f in of] == [CO.OUT_DTYPE.fields[f][1] for f in of]
    assert vals[21:] == [L.COLOR_OK, L.COLOR_EMPTY, L.COLOR_NO_MASK, L.COLOR_NO_CONTRAST, L.COLOR_TOO_LARGE, L.COLOR_MAX_PIXELS,
                         L.COLOR_MAX_COORD, L.ABI_VERSION]
    assert vals[21:26] == [R.OK, R.EMPTY, R.NO_MASK, R.NO_CONTRAST, R.TOO_LARGE] and vals[26:28] == [R.MAX_PIXELS, R.MAX_COORD]
