"""No GPU: the tilted-text rule's restatement tests/tilt_ref.py against itself and against the package's host side -- the
pinned (c, s) table, the two maps, the sign against `textblock._turn`, the conservative tile binning, the argument checks that
run before any upload, and the containment property at the inputs tests/test_gpu_tilt.py uses."""
import numpy as np
import pytest
import torch

import balloon_ref as BR
import glyph_ref as GR
import tilt_ref as T
from conftest import pkg

ANGLES = range(-180, 181)


# ---- 1. the table and the maps -------------------------------------------------------------------------------------------------

def test_the_cs_table_is_pinned():
    """What numpy's cos and sin give, rounded, is the table built from 91 pinned cosines by symmetry alone; the typeset calls
    make the same pairs; no product lies near a rounding tie."""
    p = pkg()
    tab = p.balloons.cs_of(np.arange(-180, 181))
    assert tab.shape == (361, 2) and tab.dtype == np.int64
    assert [tuple(r) for r in tab.tolist()] == [T.cs(a) for a in ANGLES]
    a, _, cs = p.typeset._tilt_args(np.arange(-180, 181), None, 361)
    assert np.array_equal(cs, tab) and np.array_equal(a, np.arange(-180, 181))
    assert T.cs(0) == (65536, 0) and T.cs(90) == (0, 65536) and T.cs(-90) == (0, -65536) and T.cs(180) == (-65536, 0) == T.cs(-180)
    assert T.cs(30) == (56756, 32768) and T.cs(-45) == (46341, -46341)
    t = np.deg2rad(np.arange(-180, 181, dtype=np.float64))
    for v in (np.cos(t) * 65536, np.sin(t) * 65536):
        assert np.abs(np.abs(v - np.floor(v)) - 0.5).min() > 0.004
    c, s = tab[:, 0], tab[:, 1]
    assert (c * c + s * s <= 65537 ** 2).all() and (c * c + s * s >= 65535 ** 2).all()      # what the compositor's frame box needs


def test_angle_zero_is_the_identity_of_both_maps():
    rng = np.random.default_rng(0)
    x, y = rng.integers(-5000, 5000, 200), rng.integers(-5000, 5000, 200)
    for pivot in ((0, 0), (37, -12), (4000, 9)):
        PX, PY = T.to_page(x, y, pivot, 65536, 0)
        u, v = T.to_frame(x, y, pivot, 65536, 0)
        assert np.array_equal(PX, x << 16) and np.array_equal(PY, y << 16) and np.array_equal(u, x << 16) and np.array_equal(v, y << 16)
    plane = rng.random((33, 70)) < 0.5
    assert np.array_equal(T.tilt_plane(plane, (5, 9, 75, 42), (-3, 100), 65536, 0), plane)


@pytest.mark.parametrize("side", [1, 9, 65])
def test_quarter_turns_permute_an_odd_square_window_about_its_centre(side):
    rng = np.random.default_rng(side)
    plane = rng.random((side, side)) < 0.4
    win = (10, 20, 10 + side, 20 + side)
    pivot = (10 + side // 2, 20 + side // 2)
    # frame -> page with (c, s) = (0, 1): PX = ax - dy, PY = ay + dx: frame (row y, column x) reads page (row x, column m - y)
    got = {a: T.tilt_plane(plane, win, pivot, *T.cs(a)) for a in (90, -90, 180, -180)}
    yy, xx = np.mgrid[0:side, 0:side]
    m = side - 1
    assert np.array_equal(got[90], plane[xx, m - yy]) and np.array_equal(got[-90], plane[m - xx, yy])
    assert np.array_equal(got[180], plane[::-1, ::-1]) and np.array_equal(got[-180], got[180])
    for g in got.values():
        assert g.sum() == plane.sum()
    assert np.array_equal(T.tilt_plane(got[90], win, pivot, *T.cs(-90)), plane)


def test_frame_to_page_to_frame_lands_within_a_pixel():
    rng = np.random.default_rng(3)
    x, y = rng.integers(-600, 600, 400), rng.integers(-600, 600, 400)
    worst = 0
    for a in ANGLES:
        c, s = T.cs(a)
        pivot = (int(rng.integers(-300, 300)), int(rng.integers(-300, 300)))
        PX, PY = T.to_page(x, y, pivot, c, s)
        u, v = T.to_frame(T.nearest(PX), T.nearest(PY), pivot, c, s)
        worst = max(worst, int(np.abs(u - (x << 16)).max()), int(np.abs(v - (y << 16)).max()))
    assert worst < 65536, worst / 65536


def test_page_to_frame_is_textblock_turn_and_makes_an_angled_blocks_lines_axis_parallel():
    """A synthetic block of angle t: three text lines, rectangles along the direction (cos t, sin t) in image coordinates (x
    right, y down).  page -> frame with the block's angle gives what `textblock._turn(pts, pivot, angle)` gives, up to
    rounding, and every line quad becomes axis-parallel."""
    p = pkg()
    for angle in (20, -25, 45, 3, -90, 135):
        t = np.deg2rad(angle)
        d, nrm = np.array([np.cos(t), np.sin(t)]), np.array([-np.sin(t), np.cos(t)])
        centre = np.array([300.0, 200.0])
        quads = []
        for k in (-1, 0, 1):
            o = centre + nrm * 30 * k
            quads.append([o - d * 80 - nrm * 10, o + d * 80 - nrm * 10, o + d * 80 + nrm * 10, o - d * 80 + nrm * 10])
        quads = np.rint(np.array(quads)).astype(np.int64)
        pivot = (300, 200)
        turned = p.textblock._turn(quads, pivot, angle)
        u, v = T.to_frame(quads[..., 0], quads[..., 1], pivot, *T.cs(angle))
        assert np.abs(turned[..., 0] - u / 65536).max() <= 1.01 and np.abs(turned[..., 1] - v / 65536).max() <= 1.01, angle
        fx, fy = u / 65536, v / 65536
        assert np.abs(fy[:, 0] - fy[:, 1]).max() <= 1.5 and np.abs(fy[:, 2] - fy[:, 3]).max() <= 1.5, angle      # top and bottom edges
        assert np.abs(fx[:, 0] - fx[:, 3]).max() <= 1.5 and np.abs(fx[:, 1] - fx[:, 2]).max() <= 1.5, angle      # left and right
        assert (fx[:, 1] - fx[:, 0] > 150).all() and (fy[:, 3] - fy[:, 0] > 15).all()                            # not mirrored
        # the other sign does not
        u2, v2 = T.to_frame(quads[..., 0], quads[..., 1], pivot, *T.cs(-angle))
        if angle not in (-90,):
            assert np.abs(v2[:, 0] - v2[:, 1]).max() / 65536 > 5, angle


# ---- 2. the host side of the package -----------------------------------------------------------------------------------------------

def test_every_pixel_the_restatement_writes_lies_in_a_binned_tile():
    p = pkg()
    ts = p.typeset
    rng = np.random.default_rng(1)
    atlas = GR.small_atlas()
    H, W = 130, 200
    pages = [rng.integers(0, 256, (H, W, 3), dtype=np.uint8)]
    tested = 0
    for trial in range(60):
        ang = int(rng.integers(-180, 181)) or 7
        piv = (int(rng.integers(-20, 220)), int(rng.integers(-20, 150)))
        r = int(rng.integers(0, 13))
        clip = None if trial % 3 else (20, 10, 150, 100)
        layers = [T.tlayer(0, ang, piv, r, clip=clip)]
        places = [(0, int(rng.integers(0, 10)), int(rng.integers(-10, 200)), int(rng.integers(-10, 130))) for _ in range(4)]
        _, rows, written = T.typeset(pages, layers, places, atlas)
        sizes = np.array([atlas[g].shape for _, g, _, _ in places])
        xy = np.array([(x, y) for _, _, x, y in places])
        _, pv, cs = ts._tilt_args([ang], [piv], 1)
        tiles, entries, status = ts.tilt_tables([(H, W)], [0], [0] * 4, sizes, xy, r, clip, pv, cs)
        cover = np.zeros((H, W), bool)
        for t in tiles[:-1]:
            cover[t["ty"] * 32:(t["ty"] + 1) * 32, t["tx"] * 64:(t["tx"] + 1) * 64] = True
        assert not (written[0] & ~cover).any(), (ang, piv, r)
        # ... and per placement: what a placement alone writes lies in the tiles that list it
        for i in range(4):
            _, _, w1 = T.typeset(pages, layers, [places[i]], atlas)
            mine = np.zeros((H, W), bool)
            for k, t in enumerate(tiles[:-1]):
                if i in entries[t["first"]:tiles[k + 1]["first"]]:
                    mine[t["ty"] * 32:(t["ty"] + 1) * 32, t["tx"] * 64:(t["tx"] + 1) * 64] = True
            assert not (w1[0] & ~mine).any()
        tested += int(rows[0, 0] > 0)
        assert (status[0] == p._lib.TYPESET_OK) or rows[0].sum() == 0
    assert tested >= 20
    # the entries of a tile ascend, every tile once
    assert (np.diff(tiles["first"]) > 0).all()


def _regions(n=3):
    p = pkg()
    B = p.balloons
    rows = np.zeros((n,), B.ROW_DTYPE)
    win = np.array([[0, 0, 64, 10]] * n, np.int64).reshape(n, 4)
    return B.BalloonRegions(np.stack([np.zeros(n), np.arange(n)], axis=1), rows, win, np.ones(n, np.int64), np.arange(n) * 10,
                            np.zeros(n, bool), torch.zeros((n * 10,), dtype=torch.int64).view(torch.uint64), np.zeros((n,), p.erase.ROW_DTYPE))


def test_argument_errors_come_before_any_upload():
    p = pkg()
    br = _regions()
    for bad in ([0, 1], [0, 1, 181], [0, -181, 0], [0.0, 1.0, 2.0], [True, False, True], 5, None):
        with pytest.raises(ValueError):
            p.balloons.tilt_regions(br, bad)
    for bad in ([[0, 0]] * 2, [[0.5, 0]] * 3, [[0, 0, 0]] * 3, [[1 << 30, 0]] * 3):
        with pytest.raises(ValueError):
            p.balloons.tilt_regions(br, [0, 10, 20], pivots=bad)
    page = np.zeros((40, 60, 3), np.uint8)
    bm = [np.full((5, 9), 255, np.uint8)]
    for bad in (dict(angle=181), dict(angle=-181), dict(angle=1.5), dict(angle=[1, 2]), dict(pivot=(3, 4)), dict(angle=10, pivot=(1, 2, 3)),
                dict(angle=10, pivot=(0.5, 1)), dict(angle=10, pivot=(1 << 28, 0)), dict(angle=True)):
        with pytest.raises(ValueError):
            p.typeset.typeset_pages([page], [0], bm, [(5, 5)], **bad)
    with pytest.raises(ValueError):                                       # a tilted call's xy stays within 2^27
        p.typeset.typeset_pages([page], [0], bm, [(1 << 28, 5)], angle=10)
    assert p.typeset._tilt_args(None, None, 4) is None and p.typeset._tilt_args(0, (5, 5), 4) is None
    assert p.typeset._tilt_args([0, 0, 0, 0], None, 4) is None
    # an empty set of regions needs no GPU
    empty = p.balloons.tilt_regions(_regions(0), np.zeros((0,), np.int64))
    assert len(empty) == 0 and empty.angle is not None and empty.cs.shape == (0, 2)


# ---- 3. containment --------------------------------------------------------------------------------------------------------------

def written_outside(region, win, pivot, angle, inset, r):
    """The pixels the compositor writes (F > 0 or S > 0) outside `region`, where U is the whole eroded frame region."""
    c, s = T.cs(angle)
    E = T.erode(T.tilt_plane(region, win, pivot, c, s), inset)
    h, w = region.shape
    Fg = T.coverage(E.astype(np.uint8) * 255, win[0], win[1], pivot, c, s, win[0] - 2 * r - 2, win[1] - 2 * r - 2, win[2] + 2 * r + 2,
                    win[3] + 2 * r + 2)
    import typeset_ref as TR
    S = TR.dilate(Fg, r)
    ink = (Fg[r:Fg.shape[0] - r, r:Fg.shape[1] - r] > 0) | (S > 0)
    inside = np.zeros(ink.shape, bool)
    inside[r + 2:r + 2 + h, r + 2:r + 2 + w] = region
    return int((ink & ~inside).sum()), int(E.sum())


CHAIN_SHAPE, CHAIN = (230, 480), (((120, 115), (100, 55), 20), ((360, 115), (100, 30), -25))


@pytest.mark.parametrize("inset,r", [(1, 0), (2, 0), (4, 3), (5, 3), (14, 12)])
def test_no_written_pixel_leaves_the_region(inset, r):
    """At the chain test's two balloons and blocks, and on a sweep of ellipses, orientations and angles: with the region eroded
    by `inset` in the frame, nothing the compositor writes with outline radius r lies outside the upright region."""
    win = (0, 0, 230, 230)
    cases = [(T.ellipse((230, 230), (115, 115), semi, turn), turn) for _, semi, turn in CHAIN]
    cases += [(T.ellipse((230, 230), (115, 115), (100, 55), 20), a) for a in range(-180, 181, 45)]
    cases += [(T.ellipse((230, 230), (115, 115), (60, 60), 0), a) for a in (-37, 3, 15, 90)]
    cases += [(T.ellipse((230, 230), (115, 115), (100, 30), 70), a) for a in (70, -20, 0, 179)]
    for region, angle in cases:
        out, kept = written_outside(region, win, (115, 115), angle, inset, r)
        assert out == 0 and (kept > 0 or inset > 10), (angle, inset, r, out)
