"""-m gpu: `ctd_fill_rest` (csrc/kernels_fill.hip) at the page sizes and buffer layouts its header promises and
tests/test_gpu_fill.py never reaches: pages of more than 256 tiles and up to T = 13 (the strided loops, the level layout and
the edge guards and clamps of `fill_page_kernel`), the 8192 x 8192 page (its dynamic LDS at capacity), and the raw entry point
with outputs and pages at every byte alignment, pitched rows, and guard bytes around everything the launches may write.  The
rule is integers only: every comparison is EXACT.  The references are `fill_ref.large_reference()` (`fill_vec`, made once)
and `fill_ref.fill_blocks` (the rule's scaling property, for the page `fill_vec` cannot reach)."""
import ctypes as C
import time

import numpy as np
import pytest
import torch

import fill_ref as R
from conftest import pkg
from test_gpu_fill import _compare

pytestmark = pytest.mark.gpu

OUT_SENTINEL = 0xA5
GUARD = 4096                                                         # dwords around the scratch, bytes x 4 around the rows
SCRATCH_SENTINEL = 0x5EA7C0DE                                        # k = 0x5e: no level pixel looks like it
ROWS_SENTINEL = 0xC3


def _align(n, a=256):
    return (n + a - 1) // a * a


def _arena(items, fill, rng=None):
    """Place 2-D byte arrays in one host arena: item = (rows (H, n) u8, pitch, misalignment 0 .. 3).  Every array
    starts `misalignment` bytes behind a 256-byte boundary with at least 256 arena bytes before it and after its last row; the
    arena is `fill` (or noise, for an input) wherever no row lies.  -> (arena, offsets, mask of the bytes that rows own)."""
    offs, cur = [], 256
    for rows, pitch, mis in items:
        offs.append(_align(cur) + mis)
        cur = offs[-1] + (rows.shape[0] - 1) * pitch + rows.shape[1] + 256
    size = _align(cur) + 256
    arena = np.full((size,), fill, np.uint8) if rng is None else rng.integers(0, 256, (size,), dtype=np.uint8)
    owned = np.zeros((size,), bool)
    for (rows, pitch, mis), off in zip(items, offs):
        h, n = rows.shape
        assert pitch >= n
        view = np.lib.stride_tricks.as_strided(arena[off:], (h, n), (pitch, 1))
        view[...] = rows
        np.lib.stride_tricks.as_strided(owned[off:], (h, n), (pitch, 1))[...] = True
    return arena, offs, owned


def _raw_fill(cases, want, layout=None, names=None):
    """ONE `ctd_fill_rest` call through ctypes on a hand-made table.  cases = [(page, hole)], want = [(out, row)], layout[i] =
    (out_dev & 3, page_dev & 3, out_pitch - 3 W, hole_pitch - W, pitch - 3 W), default all 0.  All outputs lie in one arena
    pre-filled with a sentinel, all pages in one and all masks in one (noise between their rows); the scratch buffer is
    `scratch_dwords` between two guards of GUARD dwords of a sentinel, the rows `n_pages` rows between two guards.  Asserts:
    every row field and `pad_`; every arena byte -- a row's 3 W bytes the reference's, every other one the sentinel: the gaps
    between rows, the bytes before each `out_dev` and after each page's last row --; all four guards; the input arenas
    unchanged.  -> the rows."""
    F, L = pkg().fill, pkg()._lib
    dev = torch.device("cuda:0")
    n = len(cases)
    layout = layout or [(0, 0, 0, 0, 0)] * n
    names = names or [str(i) for i in range(n)]
    rng = np.random.default_rng(n)
    shapes = [c[1].shape for c in cases]
    out_items = [(w[0].reshape(h, 3 * wd), 3 * wd + lay[2], lay[0]) for w, (h, wd), lay in zip(want, shapes, layout)]
    page_items = [(c[0].reshape(h, 3 * wd), 3 * wd + lay[4], lay[1]) for c, (h, wd), lay in zip(cases, shapes, layout)]
    hole_items = [(c[1], wd + lay[3], 0) for c, (h, wd), lay in zip(cases, shapes, layout)]
    exp_arena, out_offs, owned = _arena(out_items, OUT_SENTINEL)
    page_arena, page_offs, _ = _arena(page_items, 0, rng)
    hole_arena, hole_offs, _ = _arena(hole_items, 0, rng)
    page_d, hole_d = torch.from_numpy(page_arena).to(dev), torch.from_numpy(hole_arena).to(dev)
    page_keep, hole_keep = page_d.clone(), hole_d.clone()
    out_d = torch.full((len(exp_arena),), OUT_SENTINEL, dtype=torch.uint8, device=dev)
    assert page_d.data_ptr() % 256 == 0 and hole_d.data_ptr() % 256 == 0 and out_d.data_ptr() % 256 == 0

    tile0, n_tiles, lvl0, scratch_dwords, levels = F.fill_tables(shapes)
    pt = np.zeros((n,), F.PAGE_DTYPE)
    pt["page_dev"] = page_d.data_ptr() + np.array(page_offs, np.uint64)
    pt["hole_dev"] = hole_d.data_ptr() + np.array(hole_offs, np.uint64)
    pt["out_dev"] = out_d.data_ptr() + np.array(out_offs, np.uint64)
    pt["H"], pt["W"] = [s[0] for s in shapes], [s[1] for s in shapes]
    pt["out_pitch"], pt["pitch"], pt["hole_pitch"] = [i[1] for i in out_items], [i[1] for i in page_items], [i[1] for i in hole_items]
    pt["tile0"], pt["lvl0"] = tile0, lvl0
    for i, lay in enumerate(layout):
        assert (int(pt["out_dev"][i]) & 3, int(pt["page_dev"][i]) & 3) == lay[:2]
        assert pt["out_pitch"][i] - 3 * pt["W"][i] == lay[2] and pt["hole_pitch"][i] - pt["W"][i] == lay[3]
    tab = torch.from_numpy(pt.view(np.uint8)).to(dev)
    scratch = torch.full((GUARD + scratch_dwords + GUARD,), SCRATCH_SENTINEL, dtype=torch.int32, device=dev)
    rb = F.ROW_DTYPE.itemsize
    rows_d = torch.full((4 * GUARD + n * rb + 4 * GUARD,), ROWS_SENTINEL, dtype=torch.uint8, device=dev)
    prm = L.CtdFillParams(n_tiles)
    rc = L.lib().ctd_fill_rest(tab.data_ptr(), n, C.byref(prm), scratch.data_ptr() + 4 * GUARD, rows_d.data_ptr() + 4 * GUARD, None)
    assert rc == L.OK, L.lib().ctd_last_error()
    torch.cuda.synchronize()

    rows_h = rows_d.cpu().numpy()
    assert (rows_h[:4 * GUARD] == ROWS_SENTINEL).all() and (rows_h[4 * GUARD + n * rb:] == ROWS_SENTINEL).all(), "rows guards"
    assert bool((scratch[:GUARD] == SCRATCH_SENTINEL).all()) and bool((scratch[GUARD + scratch_dwords:] == SCRATCH_SENTINEL).all()), \
        "scratch guards"
    assert torch.equal(page_d, page_keep) and torch.equal(hole_d, hole_keep), "an input arena changed"
    rows = rows_h[4 * GUARD:4 * GUARD + n * rb].view(F.ROW_DTYPE)
    bad = []
    for i, (_, row) in enumerate(want):
        got = R.row_dict(rows[i])
        if got != row or rows[i]["pad_"].any():
            bad.append((names[i], {f: (got[f], row[f]) for f in R.FIELDS if got[f] != row[f]}, rows[i]["pad_"].tolist()))
    assert not bad, f"{len(bad)} rows differ, first: {bad[:4]}"
    assert rows["levels"].tolist() == levels.tolist()
    exp_d = torch.from_numpy(exp_arena).to(dev)
    if not torch.equal(out_d, exp_d):
        got = out_d.cpu().numpy()
        diff = got != exp_arena
        report = [("outside every row", int((diff & ~owned).sum()), np.flatnonzero(diff & ~owned)[:6].tolist())] if (diff & ~owned).any() else []
        for i, ((h, wd), off, item) in enumerate(zip(shapes, out_offs, out_items)):
            d = np.lib.stride_tricks.as_strided(diff[off:], (h, wd, 3), (item[1], 3, 1)).any(axis=2)
            if d.any():                                              # the count and the first tiles, not the arrays
                tiles = sorted({(int(y) // 64, int(x) // 64) for y, x in np.argwhere(d)[:4096]})[:6]
                report.append((names[i], layout[i], int(d.sum()), "tiles (ty, tx)", tiles, "first (y, x)", np.argwhere(d)[:3].tolist()))
        raise AssertionError(f"{int(diff.sum())} arena bytes differ: {report[:6]}")
    return rows


def _names(material):
    return [m[0] for m in material]


def _deep(hole, row):
    """The page launch pushes into level 6 of this page: the row is OK and the reference's level-6 plane has unknown pixels."""
    return row["status"] == R.OK and not R.known_plane(hole, 6).all()


def test_large_pages_in_one_call_between_pages_of_one_tile():
    """Every case of `large_material()` in ONE `fill.fill_rest` call, five 1 x 1 and 64 x 64 pages of `material()` spread between
    them, so that pages of hundreds of tiles stand between pages of one tile in the tile prefix: every row field, every byte,
    against `fill_vec`.  All three statuses occur; every size above 256 tiles has an OK case with unknown level-6 pixels."""
    F = pkg().fill
    large, want_l = R.large_material(), R.large_reference()
    small = [i for i, m in enumerate(R.material()) if m[1].shape[:2] in ((1, 1), (64, 64))]
    small = [small[0], small[2], small[len(small) // 2], small[-4], small[-1]]
    assert {R.material()[i][1].shape[:2] for i in small} == {(1, 1), (64, 64)}
    order = [("l", i) for i in range(len(large))]
    for j, i in enumerate(small):                                    # first, last and spread between
        order.insert((j * (len(order) + 1)) // (len(small) - 1) if j else 0, ("s", i))
    assert order[0][0] == "s" and order[-1][0] == "s" and sum(k == "s" for k, _ in order) == 5
    cases = [(large if k == "l" else R.material())[i] for k, i in order]
    want = [(want_l if k == "l" else R.reference())[i] for k, i in order]
    tiles = [((c[2].shape[0] + 63) // 64) * ((c[2].shape[1] + 63) // 64) for c in cases]
    assert any(a == 1 and b > 256 for a, b in zip(tiles, tiles[1:])) and tiles[0] == tiles[-1] == 1 and max(tiles) == 378
    # what the case list must hold, read from the reference alone
    assert {w[1]["status"] for w in want_l} == {R.OK, R.NO_HOLE, R.NO_KNOWN}
    assert 13 in {w[1]["levels"] for w in want_l}
    for size in R.LARGE_SIZES:
        if ((size[0] + 63) // 64) * ((size[1] + 63) // 64) > 256:
            assert any(m[2].shape == size and _deep(m[2], w[1]) for m, w in zip(large, want_l)), size
    dev = torch.device("cuda:0")
    fp = F.fill_rest([torch.from_numpy(c[1].copy()).to(dev) for c in cases], [torch.from_numpy(c[2].copy()).to(dev) for c in cases])
    _compare(fp, None, None, want, _names(cases))


@pytest.mark.parametrize("size", R.LARGE_SIZES, ids=lambda s: "%dx%d" % s)
def test_a_large_page_alone_between_guards(size):
    """Each size in a call of one page -- `one_known` (the page launch pushes everywhere), `random0.5` for the thin pages --
    through the raw entry point, with guards around the scratch and the rows and a sentinel behind the output."""
    large, want = R.large_material(), R.large_reference()
    name = {(1, 8192): "1x8192-random0.5-ramp", (8192, 1): "8192x1-random0.5-ramp", (65, 8129): "65x8129-one_known_64_0-noise",
            (1024, 1024): "1024x1024-one_known_0_0-ramp", (1025, 1025): "1025x1025-one_known_0_1024-ramp",
            (1100, 1300): "1100x1300-one_known_1099_0-noise"}[size]
    i = _names(large).index(name)
    assert large[i][2].shape == size and want[i][1]["status"] == R.OK
    assert min(size) == 1 or _deep(large[i][2], want[i][1])
    rows = _raw_fill([large[i][1:]], [want[i]], names=[name])
    assert rows["levels"][0] == (13, 13, 13, 10, 11, 11)[R.LARGE_SIZES.index(size)]


@pytest.mark.parametrize("deep", [False, True], ids=["blocks", "deep"])
def test_the_capacity_page_against_the_scaled_rule(deep):
    """8192 x 8192, T = 13, 16 384 tiles, the page launch's LDS at its capacity: noise and holes on 8 x 8 blocks
    (`fill_ref.capacity_blocks`) against `fill_ref.fill_blocks`, every row field and every byte, the scratch and the rows
    between guards.  `blocks` has unknown pixels on levels 6 .. 9; `deep`, a ramp with aligned holes of up to a quarter of the
    page, on 6 .. 12, so that every pixel of the top levels and where it lies in LDS shows in the output.  Most of the time
    is the host's: the reference, 450 MB up and the compare."""
    Q, M, s = R.capacity_blocks(deep)
    t0 = time.perf_counter()
    want = R.fill_blocks(Q, M, s)
    t1 = time.perf_counter()
    page, hole = R.repeat_blocks(Q, s), R.repeat_blocks(M, s)
    assert hole.shape == (R.MAX_SIDE, R.MAX_SIDE) and page.shape == (R.MAX_SIDE, R.MAX_SIDE, 3) == want[0].shape
    assert want[1]["status"] == R.OK and want[1]["levels"] == 13 and want[1]["n_hole"] == int((M != 0).sum()) * 64
    for l in range(6, 13 if deep else 10):                           # these levels have unknown pixels
        assert not R.known_plane(M, l - s).all(), l
    t2 = time.perf_counter()
    rows = _raw_fill([(page, hole)], [want], names=["8192x8192-" + ("deep" if deep else "blocks")])
    print(f"\nfill_blocks {t1 - t0:.2f} s, repeat {t2 - t1:.2f} s, call and compare {time.perf_counter() - t2:.2f} s")
    assert rows["levels"][0] == 13 and rows["status"][0] == R.OK
    del want, page, hole
    torch.cuda.empty_cache()


def test_a_flat_capacity_page_with_holes_in_every_tile():
    """8192 x 8192 of ONE colour, half of its pixels holes, all on the device: a page whose known pixels have one colour is
    filled with exactly it, so `out == page`; n_hole is the mask's count and top the colour.  Every tile has holes: the whole
    pyramid is read and all 16 384 tiles push."""
    F = pkg().fill
    dev = torch.device("cuda:0")
    colour = (201, 3, 118)
    page = torch.tensor(colour, dtype=torch.uint8, device=dev).expand(R.MAX_SIDE, R.MAX_SIDE, 3).contiguous()
    g = torch.Generator(device=dev).manual_seed(8192)
    mask = (torch.rand((R.MAX_SIDE, R.MAX_SIDE), generator=g, device=dev) < 0.5).to(torch.uint8) * 201
    n_hole = int(mask.count_nonzero())
    per_tile = mask.view(128, 64, 128, 64).ne(0).sum(dim=(1, 3))
    assert int(per_tile.min()) > 0 and int(per_tile.max()) < 4096 and abs(n_hole - 2 ** 25) < 2 ** 16
    fp = F.fill_rest([page], [mask])
    assert R.row_dict(fp.rows[0]) == {"status": R.OK, "n_hole": n_hole, "levels": 13, "top": list(colour)}
    assert not fp.rows[0]["pad_"].any()
    assert fp.pages[0].shape == page.shape and torch.equal(fp.pages[0], page)
    assert int(mask.count_nonzero()) == n_hole
    del fp, page, mask, per_tile
    torch.cuda.empty_cache()


def test_every_alignment_and_pitch_of_the_output_mover():
    """The raw entry point, 144 pages in one call: the 97 x 83, 65 x 129 and 130 x 67 pages of `material()` under `random0.5`,
    `checker` and `random0.98`, 16 copies each, one for every (out_dev & 3, page_dev & 3); out_pitch - 3 W cycles through 0, 1, 2, 3, 7,
    hole_pitch - W through 0, 1, 5 and pitch - 3 W through 0, 2, 5 across the copies.  So `lead` = 0 .. 3 meets x0 = 64, the
    last unit of a row is short, rows have gaps, and the funnel shift runs at every `sh`.  `_raw_fill` checks every byte of
    the output arena, the guards and the inputs."""
    material, ref = R.material(), R.reference()
    names = _names(material)
    picked = [names.index(f"{size}-{pat}") for size in ("97x83", "65x129", "130x67")
              for pat in ("random0.5-noise", "checker-flat", "random0.98-ramp")]   # the checker lies on a flat page: one more
    cases, want, layout, tags = [], [], [], []
    for i in picked:
        assert ref[i][1]["status"] == R.OK
        for copy in range(16):
            k = len(cases)
            cases.append(material[i][1:])
            want.append(ref[i])
            layout.append((copy & 3, copy >> 2, (0, 1, 2, 3, 7)[k % 5], (0, 1, 5)[k % 3], (0, 2, 5)[k % 3]))
            tags.append(f"{names[i]}#{copy}")
    assert len(cases) == 144
    for i in range(0, 144, 16):
        assert {lay[:2] for lay in layout[i:i + 16]} == {(a, b) for a in range(4) for b in range(4)}
    assert {lay[2] for lay in layout} == {0, 1, 2, 3, 7} and {lay[3] for lay in layout} == {0, 1, 5}
    for a in range(4):                                               # every out_dev & 3 meets every out pitch gap
        assert {lay[2] for lay in layout if lay[0] == a} == {0, 1, 2, 3, 7}
    _raw_fill(cases, want, layout, tags)
