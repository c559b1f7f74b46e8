"""The pull-push fill rule (include/ctd_hip.h, `ctd_fill_rest`) without a GPU: the three numpy restatements of
tests/fill_ref.py agree byte for byte, the rule has the properties the header states, `fill.fill_tables` plans what the header's
scratch layout says, and `fill.fill_rest` refuses bad arguments -- and a machine without a GPU -- loudly."""
import numpy as np
import pytest
import torch

import fill_ref as R
from conftest import pkg


def test_the_three_restatements_agree_byte_for_byte():
    """Plain loops, whole levels and the tile-wise emulation of the three launches on every page of the material (the nine
    sizes, every hole pattern): the same `out`, the same row."""
    n_status = [0, 0, 0]
    for (name, page, hole), (out, row) in zip(R.material(), R.reference()):
        o2, r2 = R.fill_emul(page, hole)
        assert r2 == row and np.array_equal(o2, out), name
        o3, r3 = R.fill_loops(page, hole)
        assert r3 == row and np.array_equal(o3, out), name
        assert out.dtype == np.uint8 and out.shape == page.shape
        assert np.array_equal(out[hole == 0], page[hole == 0]), name          # known pixels pass through
        assert row["n_hole"] == int((hole != 0).sum()) and row["levels"] == len(R.level_shapes(*hole.shape)) - 1
        n_status[row["status"]] += 1
    assert all(n_status), n_status
    names = [m[0] for m in R.material()]
    assert len(set(names)) == len(names)
    i = names.index("200x330-none-flat")
    assert R.reference()[i - 1][1]["status"] == R.OK and R.reference()[i + 1][1]["status"] == R.OK   # between pages with holes


def test_the_big_holes_leave_level_six_pixels_to_the_coarse_push():
    """The 130 x 200 holes of the 200 x 330 page cover whole aligned tiles: a level-6 pixel is unknown after the pull."""
    for name, page, hole in R.material():
        if "-big_" not in name:
            continue
        k = hole == 0
        c = page.astype(np.int64)
        for _ in range(6):
            c, k = R.pull_level(c, k)
        assert k.shape == (4, 6) and not k.all() and k.any(), name


def test_filled_values_stay_within_the_known_range():
    for (name, page, hole), (out, row) in zip(R.material(), R.reference()):
        if row["status"] != R.OK:
            continue
        known = page[hole == 0]
        lo, hi = known.min(axis=0), known.max(axis=0)
        filled = out[hole != 0]
        assert (filled >= lo).all() and (filled <= hi).all(), name
        assert (np.array(row["top"]) >= lo).all() and (np.array(row["top"]) <= hi).all()


def test_a_page_of_one_known_colour_is_filled_with_exactly_it():
    n = 0
    for (name, page, hole), (out, row) in zip(R.material(), R.reference()):
        if name.endswith("-flat") and row["status"] == R.OK:
            assert (out == page).all() and row["top"] == [17, 250, 133], name
            n += 1
    assert n >= 15
    # and where only the KNOWN pixels have one colour
    rng = np.random.default_rng(5)
    page = rng.integers(0, 256, (70, 90, 3), dtype=np.uint8)
    hole = (rng.random((70, 90)) < 0.6).astype(np.uint8)
    page[hole == 0] = (3, 200, 255)
    out, row = R.fill_vec(page, hole)
    assert (out == np.array((3, 200, 255))).all() and row["top"] == [3, 200, 255]


@pytest.mark.parametrize("H,W", [(1, 7), (9, 1), (64, 64), (97, 83), (65, 129)])
def test_one_known_pixel_at_a_corner_colours_the_whole_page(H, W):
    rng = np.random.default_rng(H * W)
    for cy, cx in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)):
        page = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        hole = np.full((H, W), 255, np.uint8)
        hole[cy, cx] = 0
        for f in (R.fill_vec, R.fill_emul):
            out, row = f(page, hole)
            assert (out == page[cy, cx]).all() and row["top"] == page[cy, cx].tolist() and row["n_hole"] == H * W - 1


def test_no_hole_and_no_known_are_copies():
    rng = np.random.default_rng(8)
    page = rng.integers(0, 256, (66, 70, 3), dtype=np.uint8)
    for f in (R.fill_loops, R.fill_vec, R.fill_emul):
        out, row = f(page, np.zeros((66, 70), np.uint8))
        assert np.array_equal(out, page) and row["status"] == R.NO_HOLE and row["n_hole"] == 0 and row["levels"] == 7
        assert row["top"] == R.fill_vec(page, np.zeros((66, 70), np.uint8))[1]["top"] != [0, 0, 0]
        out, row = f(page, np.full((66, 70), 9, np.uint8))
        assert np.array_equal(out, page) and row == {"status": R.NO_KNOWN, "n_hole": 66 * 70, "levels": 7, "top": [0, 0, 0]}
    out, row = R.fill_vec(page[:1, :1], np.zeros((1, 1), np.uint8))
    assert row == {"status": R.NO_HOLE, "n_hole": 0, "levels": 0, "top": page[0, 0].tolist()}


def test_fill_tables_plans_the_levels_and_the_scratch():
    F, L = pkg().fill, pkg()._lib
    assert (L.FILL_OK, L.FILL_NO_HOLE, L.FILL_NO_KNOWN) == (R.OK, R.NO_HOLE, R.NO_KNOWN)
    assert (L.FILL_MAX_SIDE, L.FILL_TILE) == (R.MAX_SIDE, R.TILE)
    shapes = list(R.SIZES) + [(8192, 8192), (8192, 1), (1, 4097), (4096, 4097), (2, 2), (128, 129)]
    tile0, n_tiles, lvl0, dwords, levels = F.fill_tables(shapes)
    tiles = [((h + 63) // 64) * ((w + 63) // 64) for h, w in shapes]
    assert tile0.tolist() == [sum(tiles[:i]) for i in range(len(shapes))] and n_tiles == sum(tiles)
    planes = []
    for (h, w), T in zip(shapes, levels.tolist()):
        ls = R.level_shapes(h, w)
        assert F.level_shapes(h, w) == ls and T == len(ls) - 1
        ls = ls + [(1, 1)] * 6                                      # beyond T a level is a 1 x 1 copy of the top
        planes.append(sum(a * b for a, b in ls[1:7]))
        assert ls[6] == ((h + 63) // 64, (w + 63) // 64)            # a tile is one level-6 pixel
    assert lvl0.tolist() == [n_tiles + sum(planes[:i]) for i in range(len(shapes))] and dwords == n_tiles + sum(planes)
    assert levels[len(R.SIZES)] == 13 and levels[0] == 0 and levels[8] == 9
    empty = F.fill_tables([])
    assert empty[1] == 0 and empty[3] == 0 and len(empty[0]) == 0
    for bad in ((0, 5), (5, 0), (8193, 5), (5, 8193)):
        with pytest.raises(ValueError):
            F.fill_tables([(4, 4), bad])
    assert F.PAGE_DTYPE.itemsize == 56 and F.ROW_DTYPE.itemsize == 32 and F.PAGE_DTYPE.fields["lvl0"][1] == 48


def test_fill_rest_refuses_bad_arguments():
    F = pkg().fill
    page, hole = np.zeros((20, 30, 3), np.uint8), np.zeros((20, 30), np.uint8)
    for pg, hl in ((page[:, :, 0], hole), (page[:, :, :2], hole), (page, hole[:, :29]), (page, hole[:19]), (page.astype(np.int32), hole),
                   (page, hole.astype(bool)), (page[:0], hole[:0]), (page[:, :0], hole[:, :0]), (torch.zeros((20, 30, 3)), hole),
                   (page, torch.zeros((20, 30), dtype=torch.int16))):
        with pytest.raises(ValueError):
            F.fill_rest([pg], [hl])
    with pytest.raises(ValueError):
        F.fill_rest([page, page], [hole])
    wide = np.lib.stride_tricks.as_strided(np.zeros((3,), np.uint8), (2, 8193, 3), (0, 0, 1))    # declared, never allocated
    with pytest.raises(ValueError):
        F.fill_rest([wide], [np.lib.stride_tricks.as_strided(np.zeros((1,), np.uint8), (2, 8193), (0, 0))])


def test_fill_rest_raises_without_a_gpu():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    p = pkg()
    page, hole = np.zeros((20, 30, 3), np.uint8), np.ones((20, 30), np.uint8)
    with pytest.raises(p._lib.CtdError):
        p.fill.fill_rest([page], [hole])
    assert len(p.fill.fill_rest([], [])) == 0                       # nothing to do needs no GPU
