"""The raster rule without a GPU: the restatement (tests/raster_ref.py) on shapes whose bytes are known, its distance from the
exact area, `glyphs.segments_from_ops`, `OutlineFont.metrics` against the restatement's box, `glyphs.fit` against a linear
scan, the ABI struct and constants against the header, the entry point's refusals.  The kernel is compared with the
restatement, byte for byte, in tests/test_gpu_raster.py."""
import ctypes as C
import glob
import os
import re

import numpy as np
import pytest

import raster_ref as RR
from c_layout import compiled_flat
from conftest import pkg

ONE = 65536                                                # a pixel a font unit


# ---- the rule on shapes whose bytes are known ----------------------------------------------------------------------------------

def test_pixel_aligned_rectangles_are_full():
    for x1, y1, x2, y2 in ((2, 3, 12, 8), (-7, -4, -1, 9), (0, 0, 1, 1), (0, 0, 130, 3)):
        cov, bx, by = RR.rasterise(RR.rect(x1, y1, x2, y2), ONE)
        assert cov.shape == (y2 - y1, x2 - x1) and (bx, by) == (x1, -y2) and (cov == 255).all()
    cov, bx, by = RR.rasterise(RR.rect(0, 0, 10, 10), 3 * ONE)      # a scale of three pixels a unit
    assert cov.shape == (30, 30) and (cov == 255).all()
    assert RR.box(np.zeros((0, 6), np.int32), ONE) == (0, 0, 0, 0) and RR.rasterise(np.zeros((0, 6), np.int32), ONE)[0].shape == (0, 0)


def test_a_rectangle_at_quarter_pixel_offsets_gives_the_analytic_bytes():
    """A quarter of a pixel a font unit: the rectangle 1 .. 11 x 1 .. 7 covers x 0.25 .. 2.75, y 0.25 .. 1.75.  Sixteen sample
    rows see quarters exactly, so the byte is (255 round(4096 cx cy) + 2048) >> 12 of the covered fractions."""
    cov, bx, by = RR.rasterise(RR.rect(1, 1, 11, 7), ONE // 4)
    fx, fy = np.array([0.75, 1.0, 0.75]), np.array([0.75, 0.75])
    want = (255 * np.rint(4096 * fy[:, None] * fx[None, :]).astype(np.int64) + 2048) >> 12
    assert (bx, by) == (0, -2) and np.array_equal(cov, want) and want.tolist() == [[143, 191, 143], [143, 191, 143]]
    cov, bx, by = RR.rasterise(RR.rect(2, 0, 5, 4), ONE // 4)        # x 0.5 .. 1.25: two columns, a half and a quarter
    assert np.array_equal(cov, [[(255 * 2048 + 2048) >> 12, (255 * 1024 + 2048) >> 12]]) and cov.tolist() == [[128, 64]]


def test_clockwise_equals_counter_clockwise():
    for S in (RR.scale_of(17, 1000), RR.scale_of(48, 1000)):
        a, b = RR.rasterise(RR.blob(), S), RR.rasterise(RR.blob(cw=True), S)
        assert a[1:] == b[1:] and a[0].max() == 255
        # the same edges walked the other way round: every byte
        sg = RR.random_outline(np.random.default_rng(5), contours=1)
        back = sg[::-1, [4, 5, 2, 3, 0, 1]]
        assert np.array_equal(RR.rasterise(sg, S)[0], RR.rasterise(back, S)[0])
    assert np.array_equal(RR.rasterise(RR.rect(1, 1, 11, 7), ONE // 4)[0], RR.rasterise(RR.rect(1, 1, 11, 7, cw=True), ONE // 4)[0])


def test_a_counter_oriented_inner_contour_cuts_a_hole_and_overlap_saturates():
    outer = RR.rect(0, 0, 20, 20)
    ring = RR.rasterise(np.concatenate([outer, RR.rect(5, 5, 15, 15, cw=True)]), ONE)[0]
    assert (ring[5:15, 5:15] == 0).all() and ring.sum() == 255 * 300
    same = RR.rasterise(np.concatenate([outer, RR.rect(5, 5, 15, 15)]), ONE)[0]      # winding 2 inside: saturates
    assert (same == 255).all()
    two = RR.rasterise(np.concatenate([RR.rect(0, 0, 12, 8), RR.rect(6, 4, 20, 14)]), ONE)[0]
    want = np.zeros((14, 20), np.uint8)
    want[6:14, 0:12] = 255                                 # y up: the first rectangle is the lower one
    want[0:10, 6:20] = 255
    assert np.array_equal(two, want)


def test_flatten_levels_and_horizontal_edges():
    for lv, S in enumerate(RR.ARCH_SCALE_OF_LEVEL):
        sg = RR.arch()
        assert RR.level(RR.transform(sg, S)[0]) == lv and len(RR.flatten(sg, S)) == (1 << lv) + 1
        e = RR.flatten(sg, S)
        assert np.array_equal(e[:-1, 2:], e[1:, :2])       # the edges of a contour join end to start
    bx, by, w, h = RR.box(RR.arch(), ONE)
    cov = RR.rasterise(RR.arch(), ONE)[0]
    assert (w, h) == (200, 200) and (cov[:99] == 0).all() and cov[150, 100] == 255    # the curve stays in the box's lower half
    flat = np.array([RR.line((0, 0), (10, 0)), RR.line((10, 0), (0, 0))], np.int32)     # horizontal edges only
    assert RR.box(flat, ONE) == (0, 0, 10, 0) and RR.rasterise(flat, ONE)[0].shape == (0, 10)


# ---- the rule against the exact area ------------------------------------------------------------------------------------------

def _clip_area(poly, px, py):
    """The area of a convex polygon (float64 (n, 2)) inside the pixel px .. px + 1, py .. py + 1: Sutherland-Hodgman."""
    for axis, bound, keep_above in ((0, px, True), (0, px + 1, False), (1, py, True), (1, py + 1, False)):
        if len(poly) == 0:
            return 0.0
        out = []
        for a, b in zip(poly, np.roll(poly, -1, axis=0)):
            ia = (a[axis] >= bound) if keep_above else (a[axis] <= bound)
            ib = (b[axis] >= bound) if keep_above else (b[axis] <= bound)
            if ia:
                out.append(a)
            if ia != ib:
                t = (bound - a[axis]) / (b[axis] - a[axis])
                out.append(a + t * (b - a))
        poly = np.array(out).reshape(-1, 2)
    if len(poly) < 3:
        return 0.0
    x, y = poly[:, 0], poly[:, 1]
    return 0.5 * abs(float(np.dot(x, np.roll(y, -1)) - np.dot(y, np.roll(x, -1))))


EXACT_AREA_BAR = 6.24                                      # levels; see the docstring below


def test_the_rule_is_within_a_bar_of_the_exact_area_on_convex_polygons():
    """A sanity bound on the RULE, not on the kernel: 32 seeded convex polygons (5 .. 12 corners on an ellipse, 1000 units an
    em, 6 .. 40 px an em, straight edges) against the exact float64 area of the ideal polygon in every pixel, by clipping.
    Measured here on the CPU: over the 2 796 pixels the largest difference is 5.24 levels of 255, the mean 0.26 (the large
    ones lie on near-horizontal edges, which 16 sample rows place to 1/16 pixel: up to 1/32 of a pixel's area, 8 levels).
    The bar is that largest difference plus one level, 6.24."""
    rng = np.random.default_rng(2024)
    worst, total, n = 0, 0.0, 0
    for case in range(32):
        k = int(rng.integers(5, 13))
        ang = np.sort(rng.random(k) * 2 * np.pi)
        c, ax = rng.integers(300, 700, 2), rng.integers(80, 300, 2)
        pts = np.stack([c[0] + ax[0] * np.cos(ang), c[1] + ax[1] * np.sin(ang)], 1).round().astype(np.int64)
        S = RR.scale_of(float(rng.integers(6, 41)), 1000)
        cov, bx, by = RR.rasterise(RR.polygon(pts), S)
        ideal = np.stack([pts[:, 0] * S / 65536.0, -pts[:, 1] * S / 65536.0], 1)
        for py in range(cov.shape[0]):
            for px in range(cov.shape[1]):
                want = 255.0 * _clip_area(ideal, bx + px, by + py)
                diff = abs(float(cov[py, px]) - want)
                worst, total, n = max(worst, diff), total + diff, n + 1
    print(f"\nexact area: {n} pixels, largest difference {worst:.2f} levels, mean {total / n:.3f}")
    assert n > 2000 and worst <= EXACT_AREA_BAR


# ---- segments_from_ops -------------------------------------------------------------------------------------------------------

def test_segments_from_ops_on_hand_written_cases():
    G = pkg().glyphs
    sq = [("moveTo", ((0, 0),)), ("lineTo", ((10, 0),)), ("lineTo", ((10, 10),)), ("lineTo", ((0, 10),)), ("closePath", ())]
    got = G.segments_from_ops(sq)
    assert got.dtype == np.int32 and np.array_equal(got, RR.rect(0, 0, 10, 10))
    assert np.array_equal(G.segments_from_ops(sq[:-1] + [("lineTo", ((0, 0),)), ("closePath", ())]), got)   # closed already
    assert np.array_equal(G.segments_from_ops(sq[:-1] + [("endPath", ())]), got)                          # a fill closes it
    # one off-curve point; two with the implied on-curve point between them, rounded up; a qCurveTo of one point is a line
    q = [("moveTo", ((0, 0),)), ("qCurveTo", ((5, 10), (10, 0))), ("qCurveTo", ((10, -4), (3, -5), (0, 0))), ("closePath", ())]
    assert G.segments_from_ops(q).tolist() == [[0, 0, 5, 10, 10, 0], [10, 0, 10, -4, 7, -4], [7, -4, 3, -5, 0, 0]]
    assert G.segments_from_ops([("moveTo", ((1, 2),)), ("qCurveTo", ((5, 6),)), ("closePath", ())]).tolist() == \
        [[1, 2, 1, 2, 5, 6], [5, 6, 5, 6, 1, 2]]
    # off-curve points only: the contour starts at the implied point between the last and the first
    ring = G.segments_from_ops([("qCurveTo", ((0, 0), (10, 0), (10, 10), (0, 10), None)), ("closePath", ())])
    assert ring.tolist() == [[0, 5, 0, 0, 5, 0], [5, 0, 10, 0, 10, 5], [10, 5, 10, 10, 5, 10], [5, 10, 0, 10, 0, 5]]
    # two contours; nothing at all
    two = G.segments_from_ops(sq + [("moveTo", ((20, 0),)), ("lineTo", ((30, 0),)), ("lineTo", ((30, 5),)), ("closePath", ())])
    assert len(two) == 7 and two[-1].tolist() == [30, 5, 30, 5, 20, 0]
    assert G.segments_from_ops([]).shape == (0, 6)
    with pytest.raises(ValueError, match="cu2qu"):
        G.segments_from_ops([("moveTo", ((0, 0),)), ("curveTo", ((1, 1), (2, 2), (3, 0)))])
    for bad in ([("lineTo", ((1, 1),))], [("moveTo", ((0.5, 0),))], [("moveTo", ((1 << 16, 0),))], [("arcTo", ())]):
        with pytest.raises(ValueError):
            G.segments_from_ops(bad)
    # what it returns rasterises: the square is full
    assert (RR.rasterise(got, ONE)[0] == 255).all()


def test_segments_from_ops_against_a_recording_pen():
    """DejaVu Sans through fontTools where both are on the box: the segments' end points are the pen's own on-curve points,
    the implied ones within half a font unit of fontTools' decomposition, and every contour is closed."""
    pytest.importorskip("fontTools")
    mpl = pytest.importorskip("matplotlib")
    from fontTools.pens.basePen import decomposeQuadraticSegment
    from fontTools.pens.recordingPen import RecordingPen
    from fontTools.ttLib import TTFont
    found = glob.glob(os.path.join(os.path.dirname(mpl.__file__), "mpl-data", "fonts", "ttf", "DejaVuSans.ttf"))
    if not found:
        pytest.skip("matplotlib ships no DejaVuSans.ttf here")
    G = pkg().glyphs
    font = TTFont(found[0])
    gs, cmap = font.getGlyphSet(), font.getBestCmap()
    n_curves = 0
    for ch in "Wgo8&%i":
        pen = RecordingPen()
        gs[cmap[ord(ch)]].draw(pen)
        got = G.segments_from_ops(pen.value)
        want, cur, start = [], None, None
        for name, args in pen.value:
            if name == "moveTo":
                cur = start = args[0]
            elif name == "lineTo":
                want.append((cur, cur, args[0]))
                cur = args[0]
            elif name == "qCurveTo":
                for c, e in decomposeQuadraticSegment(args):
                    want.append((cur, c, e))
                    cur = e
            elif name in ("closePath", "endPath") and cur != start:
                want.append((cur, cur, start))
        assert len(got) == len(want) and len(got) > 3
        assert np.abs(got.reshape(-1, 3, 2) - np.array(want, np.float64)).max() <= 0.5
        n_curves += int(((got[:, 2:4] != got[:, 0:2]).any(1) & (got[:, 2:4] != got[:, 4:6]).any(1)).sum())
        cov = RR.rasterise(got, RR.scale_of(24, font["head"].unitsPerEm))[0]
        assert cov.max() == 255 and 4 < cov.shape[0] <= 32
    assert n_curves > 50


# ---- OutlineFont.metrics, fit ----------------------------------------------------------------------------------------------------

def _font(G, n=24, seed=9):
    rng = np.random.default_rng(seed)
    outlines = [RR.random_outline(rng) for _ in range(n - 1)] + [np.zeros((0, 6), np.int32)]
    font = G.OutlineFont(1000, 800, 200)
    gids = font.add(outlines, [int(a) for a in rng.integers(300, 900, n - 1)] + [350])
    assert gids.tolist() == list(range(n)) and gids.dtype == np.int32 and len(font) == n
    return font, outlines


def test_metrics_equal_the_restatements_box():
    G = pkg().glyphs
    font, outlines = _font(G)
    assert font.n_segs == sum(len(o) for o in outlines) and font.seg_first.tolist() == np.cumsum([0] + [len(o) for o in outlines])[:-1].tolist()
    for size in (7, 12.5, 24, 48, 300):
        S = font.scale(size)
        assert S == RR.scale_of(size, 1000)
        gids = [3, 0, 23, 3, 11]
        m = font.metrics(gids, size)
        base, down = (800 * S + 32768) >> 16, (200 * S + 32768) >> 16
        for i, g in enumerate(gids):
            bx, by, w, h = RR.box(outlines[g], S)
            assert m.sizes[i].tolist() == [h, w] and m.box[i].tolist() == [bx, by, w, h]
            assert m.bearing[i].tolist() == [bx, base + by]
            assert m.advance[i].tolist() == [(int(font.advance[g]) * S + 32768) >> 16, base + down]
        assert (m.baseline, m.line, m.scale) == (base, base + down, S) and m.sizes[2].tolist() == [0, 0]
        assert np.array_equal(G.outline_boxes([outlines[g] for g in gids], S), m.box)     # the loose-outline form of the same box
        v = font.metrics(gids, size, vertical=True)
        assert np.array_equal(v.sizes, m.sizes) and np.array_equal(v.advance, m.advance)
        assert np.array_equal(v.bearing[:, 1], m.bearing[:, 1]) and not v.bearing[:, 0].any() and v.line == (1000 * S + 32768) >> 16
    for bad in (dict(gids=[24], size=12), dict(gids=[-1], size=12), dict(gids=[0], size=0), dict(gids=[0], size=70000)):
        with pytest.raises(ValueError):
            font.metrics(**bad)
    with pytest.raises(ValueError):
        font.add([np.zeros((2, 5), np.int32)], [10])
    with pytest.raises(ValueError):
        font.add([np.full((1, 6), 40000, np.int32)], [10])


def test_fit_against_a_linear_scan():
    """`fit` bisects; a linear scan over all sizes is the oracle, and `fits` is monotone in the size on every seeded case (what
    the bisection stands on)."""
    G = pkg().glyphs
    font, _ = _font(G)
    rng = np.random.default_rng(21)
    sizes = [8, 10, 12, 14, 16, 18, 20, 24, 28, 32, 40, 48, 64]
    n_none = n_all = n_mid = 0
    for case in range(120):
        run = rng.integers(0, len(font), int(rng.integers(1, 30)))
        rect = (10, 20, 10 + int(rng.integers(6, 300)), 20 + int(rng.integers(6, 300)))
        kw = dict(vertical=bool(case & 1), gap=int(rng.integers(0, 4)), align=("left", "center", "right")[case % 3])
        if case % 4 == 3:
            kw["breaks"] = rng.random(len(run)) < 0.4
        fits = [G.flow_outlines(run, font, rect, s, **kw)[1] for s in sizes]
        assert fits == sorted(fits, reverse=True), (case, fits)           # monotone: once it stops fitting it never fits again
        want = (max(s for s, f in zip(sizes, fits) if f), True) if any(fits) else (sizes[0], False)
        assert G.fit(run, font, rect, sizes, **kw) == want, case
        n_none += not any(fits)
        n_all += all(fits)
        n_mid += any(fits) and not all(fits)
    print(f"\nfit: none {n_none}, some {n_mid}, all {n_all}")
    assert n_none >= 3 and n_mid > 40 and n_all > 5
    # flow_outlines is flow on the font's metrics, the line the scaled ascent + descent
    run = np.array([3, 5, 3, 23, 7])
    m = font.metrics(np.unique(run), 24)
    xy, f = G.flow(np.searchsorted(np.unique(run), run), m, (0, 0, 200, 100), line=m.line, gap=2)
    xy2, f2 = G.flow_outlines(run, font, (0, 0, 200, 100), 24, gap=2)
    assert np.array_equal(xy, xy2) and f == f2
    for bad in ([], [12, 12], [14, 12]):
        with pytest.raises(ValueError):
            G.fit(run, font, (0, 0, 50, 50), bad)


# ---- ABI ---------------------------------------------------------------------------------------------------------------------

def test_the_raster_job_has_the_c_layout_and_the_entry_point_refuses():
    """`glyphs.RASTER_JOB_DTYPE` and `_lib.CtdRasterJob` against the header, compiled; the constants; the launch-shape
    constants against csrc/kernels.h; the entry point is exported and bound, refuses bad arguments before it launches
    anything, and takes the empty call (no GPU is needed for any of it)."""
    p = pkg()
    L, G = p._lib, p.glyphs
    fs = ("off", "w", "h", "bx", "by", "seg_first", "seg_count", "scale", "pad_")
    consts = ("CTD_RASTER_MAX_SIDE", "CTD_RASTER_MAX_SCALE", "CTD_RASTER_OK", "CTD_RASTER_EMPTY", "CTD_RASTER_REFUSED", "CTD_ABI_VERSION")
    vals = compiled_flat({"ctd_raster_job": fs}, consts)
    assert vals[0] == C.sizeof(L.CtdRasterJob) == G.RASTER_JOB_DTYPE.itemsize == 40
    assert vals[1:10] == [getattr(L.CtdRasterJob, f).offset for f in fs] == [G.RASTER_JOB_DTYPE.fields[f][1] for f in fs]
    assert [f for f, _ in L.CtdRasterJob._fields_] == list(fs) and G.RASTER_JOB_DTYPE.names == fs
    assert vals[10:] == [L.RASTER_MAX_SIDE, L.RASTER_MAX_SCALE, L.RASTER_OK, L.RASTER_EMPTY, L.RASTER_REFUSED, L.ABI_VERSION]
    assert vals[-1] == 10 and (RR.MAX_SIDE, RR.MAX_SCALE, RR.OK, RR.EMPTY, RR.REFUSED) == tuple(vals[10:15])
    src = open(os.path.join(os.path.dirname(L.__file__), "csrc", "kernels.h")).read()
    shape = re.search(r"RS_BAND_H = (\d+), RS_CHUNK_W = (\d+), RS_SEG_CHUNK = (\d+), RS_BANDS_Y = (\d+);", src)
    assert [int(v) for v in shape.groups()] == [L.RASTER_BAND_H, L.RASTER_CHUNK_W, L.RASTER_SEG_CHUNK, L.RASTER_BANDS_Y]
    assert "ctd_rasterise_glyphs" in L.SYMBOLS and hasattr(L.lib(), "ctd_rasterise_glyphs")
    lib = L.lib()
    good = [8, 4, 8, 2, 8, 64, 8, None]                    # segs, n_segs, jobs, n_jobs, atlas, atlas_bytes, status, stream
    for i in (1, 3, 5):                                    # a negative count, a negative atlas_bytes
        a = list(good)
        a[i] = -1
        assert lib.ctd_rasterise_glyphs(*a) != L.OK, i
        assert b"bad sizes" in lib.ctd_last_error()
    for i in (0, 2, 4, 6):                                 # a missing table where its count is positive
        a = list(good)
        a[i] = None
        assert lib.ctd_rasterise_glyphs(*a) != L.OK, i
        assert b"null" in lib.ctd_last_error()
    assert lib.ctd_rasterise_glyphs(8, 4, 8, (1 << 24) + 1, 8, 64, 8, None) != L.OK
    # no jobs: nothing at all, whatever else is there
    assert lib.ctd_rasterise_glyphs(None, 0, None, 0, None, 0, None, None) == L.OK
    assert lib.ctd_rasterise_glyphs(8, 4, None, 0, 8, 64, None, None) == L.OK


def test_rasterise_needs_a_gpu_and_the_font_does_not():
    import torch
    p = pkg()
    G = p.glyphs
    font, _ = _font(G, n=4)
    assert "OutlineFont" in G.__all__ and "fit" in G.__all__ and "segments_from_ops" in G.__all__
    assert font.metrics([0, 1], 20).sizes.shape == (2, 2)
    if not torch.cuda.is_available():
        with pytest.raises(p._lib.CtdError):
            font._sync()
