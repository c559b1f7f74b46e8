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


def test_large_material_is_what_the_page_launch_needs():
    """The six sizes plan T = 13, 13, 13, 10, 11, 11 and 128, 128, 256, 256, 289, 378 tiles; every pattern of every size is
    there once; all three statuses occur; every size above 256 tiles has an OK page whose level-6 plane has unknown pixels,
    and so has one at 256; the pages and masks are read-only."""
    F = pkg().fill
    tile0, n_tiles, lvl0, dwords, levels = F.fill_tables(R.LARGE_SIZES)
    tiles = [128, 128, 2 * 128, 16 * 16, 17 * 17, 18 * 21]
    assert levels.tolist() == [13, 13, 13, 10, 11, 11] and n_tiles == sum(tiles)
    assert tile0.tolist() == [sum(tiles[:i]) for i in range(6)]
    assert [len(R.level_shapes(h, w)) - 1 for h, w in R.LARGE_SIZES] == levels.tolist()
    assert [R.level_shapes(h, w)[6] for h, w in R.LARGE_SIZES] == [(1, 128), (128, 1), (2, 128), (16, 16), (17, 17), (18, 21)]
    assert all(a % 2 for lv in R.level_shapes(65, 8129)[1:6] for a in lv[1:]) and R.level_shapes(65, 8129)[6][1] == 128
    assert [lv[0] for lv in R.level_shapes(1025, 1025)[6:]] == [17, 9, 5, 3, 2, 1]
    material, want = R.large_material(), R.large_reference()
    names = [m[0] for m in material]
    assert len(names) == len(set(names)) <= 42 and len(want) == len(names)
    assert R.large_material() is material and R.large_reference() is want
    deep = {}
    for (name, page, hole), (out, row) in zip(material, want):
        assert not page.flags.writeable and not hole.flags.writeable and not out.flags.writeable
        assert (hole.shape in R.LARGE_SIZES) and page.shape == hole.shape + (3,) and name.startswith("%dx%d-" % hole.shape)
        assert row["n_hole"] == int((hole != 0).sum()) and row["levels"] == len(R.level_shapes(*hole.shape)) - 1
        assert np.array_equal(out[hole == 0], page[hole == 0]), name
        k6 = R.known_plane(hole, 6)
        assert k6.shape == R.level_shapes(*hole.shape)[6]
        if row["status"] == R.OK and not k6.all():
            deep.setdefault(hole.shape, []).append(name)
        if "-one_known_" in name:
            cy, cx = np.argwhere(hole == 0)[0]
            assert (out == page[cy, cx]).all() and row["top"] == page[cy, cx].tolist() and int(k6.sum()) == 1, name
        if name.endswith("-flat") and row["status"] == R.OK:
            assert (out == page).all(), name
    assert sorted({w[1]["status"] for w in want}) == [R.OK, R.NO_HOLE, R.NO_KNOWN]
    assert set(deep) == set(R.LARGE_SIZES), deep
    for size in R.LARGE_SIZES[3:]:
        assert any("-big-" in n for n in deep[size]) and any("-islands-" in n for n in deep[size]), deep[size]
    # the big holes leave unknown pixels next to known ones on every level below the top (the corner one: the last row and
    # column of the odd planes), the islands mix n = 1, 2, 3 above level 6
    i = names.index("1025x1025-big-ramp")
    for l in (6, 7, 8, 9, 10):
        k = R.known_plane(material[i][2], l)
        assert k.any() and not k.all(), l
    i = names.index("1025x1025-islands-" + ("noise", "ramp", "flat")[7 % 3])
    k = R.known_plane(material[i][2], 6)
    kp = np.zeros((18, 18), int)
    kp[:17, :17] = k
    assert {1, 2, 3} <= set(kp.reshape(9, 2, 9, 2).sum(axis=(1, 3)).ravel().tolist())


def test_the_emulated_launches_equal_the_rule_on_the_large_pages():
    """`fill_emul` -- strided tile loops, the halo's index ranges, the level layout -- against `fill_vec` on every large case
    of at most 70 000 pixels, and on the two `one_known` cases of 1025 x 1025 at opposite corners (the emulation is slow)."""
    material, want = R.large_material(), R.large_reference()
    n = 0
    for (name, page, hole), (out, row) in zip(material, want):
        if hole.size <= 70000 or name in ("1025x1025-one_known_0_0-noise", "1025x1025-one_known_1024_1024-noise"):
            o2, r2 = R.fill_emul(page, hole)
            assert r2 == row and np.array_equal(o2, out), name
            n += 1
    assert n == 12


def _block_cases():
    """[(name, Q, M)]: Q from 1 x 1 to 130 x 170 under the hole patterns of `holes_of` (the random ones, the checker, one known
    pixel at a corner, single holes at every edge and corner), and the capacity page's parts at 128 x 128."""
    rng = np.random.default_rng(77)
    out = []
    for H, W in ((1, 1), (1, 7), (9, 1), (5, 6), (17, 23), (63, 65), (130, 170)):
        for i, (name, M) in enumerate(R.holes_of(H, W, rng)):
            if (H, W) == (130, 170) and name in ("all", "none", "random0.02", "random0.98", "singles01", "singles10"):
                continue
            Q = (rng.integers(0, 256, (H, W, 3), dtype=np.uint8), R.ramp_page(H, W))[i % 2]
            out.append((f"{H}x{W}-{name}", Q, M))
    M = np.zeros((40, 50), np.uint8)                                # holes flush with every edge and corner, and one inside
    M[:3, :4] = M[:5, -2:] = M[-1:, :9] = M[-6:, -7:] = M[17:22, :1] = M[:2, 20:31] = M[-3:, 25:27] = M[11:19, -1:] = M[9:25, 13:30] = 3
    out.append(("40x50-edges", rng.integers(0, 256, (40, 50, 3), dtype=np.uint8), M))
    out.append(("128x128-capacity-parts", rng.integers(0, 256, (128, 128, 3), dtype=np.uint8), R.block_mask(128, rng)))
    M = np.zeros((128, 128), np.uint8)                              # and its companion's: aligned squares, a quarter of the page
    M[64:, :64], M[:32, 64:96], M[48:64, 16:32] = 255, 2, 1
    M[rng.integers(0, 128, 5), rng.integers(0, 128, 5)] = 77
    out.insert(-1, ("128x128-deep-parts", R.ramp_page(128, 128), M))
    return out


@pytest.mark.parametrize("s", [1, 2, 3])
def test_fill_blocks_equals_the_rule_on_the_repeated_page(s):
    """`fill_blocks(Q, M, s)` == `fill_vec(repeat(Q), repeat(M))`, every byte and the row: the reference of the capacity page
    is the rule itself."""
    n_ok = 0
    for name, Q, M in _block_cases():
        out, row = R.fill_blocks(Q, M, s)
        o2, r2 = R.fill_vec(R.repeat_blocks(Q, s), R.repeat_blocks(M, s))
        assert row == r2, (name, row, r2)
        assert out.dtype == np.uint8 and np.array_equal(out, o2), (name, int((out != o2).any(axis=2).sum()))
        n_ok += row["status"] == R.OK
    assert n_ok >= 40
    Q, M = _block_cases()[-1][1:]
    for win in (1, 3, 200):                                          # whatever the windows
        assert np.array_equal(R.fill_blocks(Q, M, s, win=win)[0], R.fill_blocks(Q, M, s)[0])
    assert np.array_equal(R.fill_blocks(Q, M, 0)[0], R.fill_vec(Q, M)[0])


def test_capacity_blocks_reach_every_level_of_the_page_launch():
    """The capacity page's blocks: 1024 x 1024 at s = 3 is 8192 x 8192 with T = 13 and 16 384 tiles; the large hole starts at no
    multiple of 8 blocks, covers whole tiles and cuts others, and leaves unknown pixels on levels 6 .. 9 but not 10; every
    corner and the whole right and bottom edge are hole; a tile holds 64 block colours."""
    Q, M, s = R.capacity_blocks()
    assert Q.shape == (1024, 1024, 3) and M.shape == (1024, 1024) and s == 3 and R.capacity_blocks()[0] is Q
    plan = pkg().fill.fill_tables([(8192, 8192)])
    assert plan[1] == 16384 and plan[4].tolist() == [13]
    ys, xs = np.flatnonzero((M == 255).any(axis=1)), np.flatnonzero((M == 255).any(axis=0))
    assert (ys[0] % 8, xs[0] % 8, len(ys), len(xs)) == (5, 3, 160, 200)
    assert [bool(R.known_plane(M, l - 3).all()) for l in (6, 7, 8, 9, 10)] == [False, False, False, False, True]
    holes_per_tile = (M != 0).reshape(128, 8, 128, 8).sum(axis=(1, 3))
    assert (holes_per_tile == 64).sum() >= 19 * 24 and ((holes_per_tile > 0) & (holes_per_tile < 64)).sum() > 300
    assert M[0, 0] and M[0, -1] and M[-1, 0] and M[-1, -1] and M[:, -1].all() and M[-1, :].all()
    assert 250 <= int((M == 77).sum()) <= 300
    assert len(np.unique(Q[:8, :8].reshape(64, 3), axis=0)) == 64
    out, row = R.fill_vec(Q, M)
    assert row["status"] == R.OK and row["levels"] == 10
    # noise averages out: the top levels of that page are all alike, and its companion's are not
    c, k = Q.astype(np.int64), M == 0
    for _ in range(7):
        c, k = R.pull_level(c, k)
    assert k.all() and int(np.ptp(c)) <= 8                          # means of >= 5000 bytes of noise each: sigma about 1
    Q2, M2, s2 = R.capacity_blocks(deep=True)
    assert s2 == 3 and [bool(R.known_plane(M2, l - 3).all()) for l in range(6, 14)] == [False] * 7 + [True]
    c, k = Q2.astype(np.int64), M2 == 0
    for _ in range(7):
        c, k = R.pull_level(c, k)
    assert not k.all() and int(np.ptp(c[k][:, 0])) > 100 and R.fill_vec(Q2, M2)[1]["status"] == R.OK


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
