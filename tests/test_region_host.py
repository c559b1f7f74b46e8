"""CPU: `ctd_region_transforms` (csrc/host_region.cpp: margin, ratio, crop size, four-point homography and its inverse of
`TextBlock.get_transformed_region`, reference utils/textblock.py:162-194) against the numpy restatement tests/region_ref.py,
and that restatement's warp against what a warp must do on cases with a known answer.  No GPU."""
import numpy as np
import pytest

import region_ref as R
from conftest import pkg

LANGS = ["eng", "ja", "unknown"]
N_QUADS = 720                       # >= 600: 240 of each kind


def seeded_quads(n=N_QUADS, seed=20240):
    """(quad (4,2) int, kind, font_size, (im_w, im_h)) -- three kinds, the detector's point order (clockwise from the top
    left): axis-aligned boxes; boxes turned by up to +-45 degrees and truncated to integers; boxes with every corner
    jittered by +-4 px (true perspective).  Page coordinates up to 4500.  Every third case of a kind sits at the page's
    border with a font size whose margin (font_size / 3) runs into the clip to [0, im_w] x [0, im_h]; every fifth box is
    tall instead of wide (the lines of vertical blocks)."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        kind = k % 3
        im_w, im_h = int(rng.integers(600, 4500)), int(rng.integers(600, 4500))
        w, h = int(rng.integers(30, min(1500, im_w - 60))), int(rng.integers(12, 120))
        if (k // 3) % 5 == 4:
            w, h = h, min(w, im_h - 60)
        at_border = (k // 3) % 3 == 2
        if at_border:
            x0 = int(rng.choice([0, 1, im_w - w - 1, im_w - w]))
            y0 = int(rng.choice([0, 2, im_h - h - 2, im_h - h]))
            fs = float(rng.integers(12, 90))
        else:
            x0, y0 = int(rng.integers(20, im_w - w - 20)), int(rng.integers(20, im_h - h - 20))
            fs = float(rng.integers(9, 60)) if k % 2 else float(rng.integers(9, 60)) + float(rng.random())
        q = np.array([[x0, y0], [x0 + w, y0], [x0 + w, y0 + h], [x0, y0 + h]], np.float64)
        if kind == 1:
            a = np.deg2rad(rng.uniform(-45, 45))
            c = q.mean(0)
            q = np.trunc((q - c) @ np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]).T + c)
        elif kind == 2:
            q = q + rng.integers(-4, 5, (4, 2))
        out.append((q.astype(np.int32), ("axis", "turned", "jittered")[kind], fs, (im_w, im_h)))
    return out


def probe(Minv, w, h):
    """Source coordinates (1/32-px units) of the four output corners and the centre under `Minv`, by the warp's own
    expression."""
    fX, fY = R.source_coords(Minv, w, h)
    pts = [(0, 0), (0, w - 1), (h - 1, w - 1), (h - 1, 0), ((h - 1) // 2, (w - 1) // 2)]
    return np.array([[fX[p], fY[p]] for p in pts])


def test_region_transforms_equal_the_restatement():
    """Every seeded quad x {eng, ja, unknown} x {horizontal, vertical}: status, w and h EQUAL (both sides evaluate the ratio
    in one float64 order, so not even a rounding tie of textheight / ratio may differ), and the source coordinates the
    product's Minv (8x8 LU + adjugate) maps the crop's corners and centre to within the tie band of the restatement's
    (LAPACK solve + inverse).  The measured maximum is printed and recorded in DESIGN section 5."""
    RG = pkg().regions
    L = pkg()._lib
    quads = seeded_quads()
    assert len(quads) >= 600 and {k for _, k, _, _ in quads} == {"axis", "turned", "jittered"}
    cases = [(q, kind, fs, sz, lang, vert) for q, kind, fs, sz in quads for lang in LANGS for vert in (False, True)]
    wh, M, Minv, status = RG.transforms(np.array([c[0] for c in cases]), [LANGS.index(c[4]) for c in cases],
                                        [c[5] for c in cases], [c[2] for c in cases], [c[3][0] for c in cases],
                                        [c[3][1] for c in cases], 48)
    worst, worst_fwd, n_ok, n_bad, clipped = 0.0, 0.0, 0, 0, 0
    for i, (q, kind, fs, (im_w, im_h), lang, vert) in enumerate(cases):
        src = R.line_quad(q, lang, vert, fs, im_w, im_h)
        if lang != "ja" and not (lang == "unknown" and vert):
            e = fs / 3
            clipped += bool((q[:, 0].min() - e < 0) or (q[:, 0].max() + e > im_w) or (q[:, 1].min() - e < 0) or
                            (q[:, 1].max() + e > im_h))
        try:
            w, h, Mr, Mir = R.transform(q, lang, vert, fs, im_w, im_h, 48)
        except ValueError:
            assert status[i] == L.REGION_DEGENERATE and tuple(wh[i]) == (0, 0), (i, kind, lang, vert, q.tolist(), wh[i])
            n_bad += 1
            continue
        assert status[i] == L.REGION_OK and tuple(wh[i]) == (w, h), (i, kind, lang, vert, q.tolist(), wh[i], (w, h))
        n_ok += 1
        d = float(np.abs(probe(Minv[i], w, h) - probe(Mir, w, h)).max())
        worst = max(worst, d)
        assert d <= R.BAND, (i, kind, lang, vert, q.tolist(), d)
        # M itself: the quad (with its margin) lands on the crop's corners
        p = np.c_[src, np.ones(4)] @ M[i].T
        fwd = float(np.abs(p[:, :2] / p[:, 2:] - [[0, 0], [w - 1, 0], [w - 1, h - 1], [0, h - 1]]).max())
        worst_fwd = max(worst_fwd, fwd)
        assert fwd < 1e-6, (i, fwd)
    print(f"\n{len(cases)} cases: {n_ok} valid, {n_bad} degenerate on both sides, {clipped} with a clipped margin; max |product - "
          f"restatement| of the mapped corners / centre = {worst:.3g} of a 1/32-px unit (band {R.BAND:g}); max corner residual "
          f"of M = {worst_fwd:.3g} px")
    assert n_ok >= 2400 and clipped >= 300


def test_degenerate_quads_are_invalid_not_fatal():
    """Collinear points, zero width, zero height, a single point: status DEGENERATE with size (0, 0), in the middle of a batch
    whose other lines stay valid; the restatement raises on each."""
    RG = pkg().regions
    L = pkg()._lib
    good = [[100, 100], [400, 100], [400, 140], [100, 140]]
    bad = {
        "collinear horizontal": [[10, 50], [100, 50], [200, 50], [300, 50]],
        "collinear diagonal": [[10, 10], [110, 60], [210, 110], [310, 160]],
        "collinear, wide and flat": [[100, 100], [400, 100], [400, 100], [100, 100]],
        "zero width": [[100, 100], [100, 100], [100, 140], [100, 140]],
        "a single point": [[7, 7]] * 4,
        "three corners on a line": [[0, 0], [100, 0], [200, 0], [0, 50]],
    }
    names = list(bad)
    for vert in (False, True):
        for lang in (1, 2, 0):
            quads = [good] + [bad[k] for k in names] + [good]
            wh, M, Minv, status = RG.transforms(np.array(quads), lang, vert, 0.0, 2000, 2000, 48)
            assert status[0] == status[-1] == L.REGION_OK and (wh[0] == wh[-1]).all() and wh[0].min() >= 1
            for k, name in enumerate(names, start=1):
                assert status[k] == L.REGION_DEGENERATE and tuple(wh[k]) == (0, 0), (name, vert, lang, wh[k])
                assert not M[k].any() and not Minv[k].any()
                with pytest.raises(ValueError):
                    R.transform(bad[name], LANGS[lang], vert, 0.0, 2000, 2000, 48)
    # nothing to do is fine
    wh, M, Minv, status = RG.transforms(np.zeros((0, 8), np.int32), [], [], [], [], [], 48)
    assert wh.shape == (0, 2) and status.shape == (0,)


def test_sizes_follow_round_half_even_and_truncation():
    """int(textheight) truncates; the other side is Python's round (half to even) of textheight / ratio."""
    RG = pkg().regions
    # ratio 40 / 100: 48 / 0.4 = 120 exactly; ratio 32 / 100 -> 150 exactly; 3 / 32 -> 48 / (3/32) = 512
    for (w0, h0), want in (((100, 40), 120), ((100, 32), 150), ((32, 3), 512)):
        q = [[10, 10], [10 + w0, 10], [10 + w0, 10 + h0], [10, 10 + h0]]
        wh, _, _, st = RG.transforms([q], 1, False, 0.0, 1000, 1000, 48)
        assert st[0] == 0 and tuple(wh[0]) == (want, 48) and R.transform(q, "ja", False, 0.0, 1000, 1000, 48)[:2] == (want, 48)
    # a tie: textheight 3, ratio 2 / 1 -> 1.5 -> 2 (even); textheight 5 -> 2.5 -> 2 (even), not 3
    q = [[10, 10], [20, 10], [20, 30], [10, 30]]
    for th, want in ((3, 2), (5, 2), (7, 4)):
        wh, _, _, st = RG.transforms([q], 1, False, 0.0, 1000, 1000, th)
        assert st[0] == 0 and tuple(wh[0]) == (want, th) == R.transform(q, "ja", False, 0.0, 1000, 1000, th)[:2]
    wh, _, _, st = RG.transforms([q], 1, False, 0.0, 1000, 1000, 48.9)
    assert st[0] == 0 and wh[0][1] == 48 and R.transform(q, "ja", False, 0.0, 1000, 1000, 48.9)[:2] == tuple(wh[0])


def test_restatement_translation_returns_the_source_window_and_zero_border():
    """`region_ref` itself: with a pure integer translation as Minv the warp IS the source window, byte for byte, in 1 and 3
    channels; taps beyond the border read 0; a half-pixel shift averages two neighbours with OpenCV's rounding; the rotation
    is cv2.rotate(.., ROTATE_90_COUNTERCLOCKWISE)."""
    rng = np.random.default_rng(5)
    for shape in ((37, 53), (37, 53, 3)):
        img = rng.integers(0, 256, shape, dtype=np.uint8)
        Minv = np.array([[1, 0, 11], [0, 1, 5], [0, 0, 1]], np.float64)
        got = R.warp(img, Minv, 20, 13)
        assert got.dtype == np.uint8 and np.array_equal(got, img[5:18, 11:31])
        region, band, cands, _ = R.warp_candidates(img, Minv, 20, 13)
        assert np.array_equal(region, got) and not band.any() and all(np.array_equal(c, got) for c in cands)
        # a window hanging over every border: inside equals the image, outside is 0
        Minv = np.array([[1, 0, -4], [0, 1, -3], [0, 0, 1]], np.float64)
        got = R.warp(img, Minv, 64, 45)
        want = np.zeros((45, 64) + shape[2:], np.uint8)
        want[3:40, 4:57] = img
        assert np.array_equal(got, want)
        # wholly outside
        assert not R.warp(img, np.array([[1, 0, 500], [0, 1, 0], [0, 0, 1]], np.float64), 9, 7).any()
        # the rotation
        Minv = np.array([[1, 0, 11], [0, 1, 5], [0, 0, 1]], np.float64)
        rot = R.warp(img, Minv, 20, 13, rotate=True)
        assert rot.shape[:2] == (20, 13)
        src = img[5:18, 11:31]
        for i in (0, 7, 19):
            for j in (0, 4, 12):
                assert np.array_equal(rot[i, j], src[j, 20 - 1 - i])
    # half a pixel to the right: (a + b + 1) >> 1 of neighbours in OpenCV's fixed point = (16384 (a + b) + 16384) >> 15
    img = rng.integers(0, 256, (8, 9), dtype=np.uint8)
    got = R.warp(img, np.array([[1, 0, 0.5], [0, 1, 0], [0, 0, 1]], np.float64), 8, 8)
    want = ((img[:, :-1].astype(np.int64) + img[:, 1:] + 1) >> 1).astype(np.uint8)
    assert np.array_equal(got, want)
    # the tie band: x + 1/64 px is a rounding boundary of the 1/32-px grid
    region, band, cands, (fX, fY) = R.warp_candidates(img, np.array([[1, 0, 1 / 64], [0, 1, 0], [0, 0, 1]], np.float64), 8, 8)
    assert band.all() and np.array_equal(cands[0], img[:, :8]) and np.array_equal(cands[0], cands[2])
    assert not np.array_equal(cands[1], cands[0]) and any(np.array_equal(region, c) for c in cands)
