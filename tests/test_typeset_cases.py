"""The material of tests/test_gpu_typeset_walk.py (tests/typeset_cases.py) holds what its docstrings promise, without a GPU: a
case that has silently become vacuous fails HERE and does not pass on the GPU.  Run lengths are read from
`glyphs.glyph_tables` -- and, for the same cases sent through `tilted_kernel`, from `typeset.tilt_tables` -- the pixel claims
from the restatement tests/glyph_ref.py; and on every case and every seed the host tables of both calls equal the brute-force
loops of the restatements."""
import numpy as np
import pytest

import glyph_ref as GR
import typeset_cases as TC
import typeset_ref as TR
from conftest import pkg

SEEDS = [name for name, _, _ in TC.SEED_CASES]


def _columns(pages, bitmaps, layers, places):
    shapes = [pg.shape[:2] for pg in pages]
    clip = [ly.get("clip") or (0, 0, shapes[ly["page"]][1], shapes[ly["page"]][0]) for ly in layers]
    return shapes, dict(page_of=[ly["page"] for ly in layers], layer_of=[q[0] for q in places],
                        sizes=np.array(TC.sizes_of(bitmaps, places), np.int64).reshape(-1, 2),
                        xy=np.array([(q[2], q[3]) for q in places], np.int64).reshape(-1, 2),
                        radius=[ly["r"] for ly in layers], clip=clip)


def _tile_runs(name):
    """{(page, tx, ty): [the layer of every entry of that tile, in order]} from `glyphs.glyph_tables`."""
    pages, bitmaps, layers, places = TC.case(name)
    shapes, col = _columns(pages, bitmaps, layers, places)
    tiles, entries, _ = pkg().glyphs.glyph_tables(shapes, **col)
    first = tiles["first"]
    return {(int(t["page"]), int(t["tx"]), int(t["ty"])): [places[i][0] for i in entries[first[k]:first[k + 1]]]
            for k, t in enumerate(tiles[:-1])}


def _tilt_runs(name):
    """`_tile_runs` of the call that sends the case through `tilted_kernel` (`TC.tilted`), from `typeset.tilt_tables`, which
    bins by a box grown by one pixel and by r + 1: a tile may list more placements than on the upright path."""
    pages, bitmaps, _, places = TC.case(name)
    layers, angle, pivot = TC.tilted(name)
    shapes, col = _columns(pages, bitmaps, layers, places)
    T = pkg().typeset
    _, pv, cs = T._tilt_args(angle, pivot, len(layers))
    assert cs[:-1].tolist() == [[65536, 0]] * (len(layers) - 1) and cs[-1, 1] != 0
    tiles, entries, status = T.tilt_tables(shapes, col["page_of"], col["layer_of"], col["sizes"], col["xy"], col["radius"], col["clip"], pv, cs)
    assert status.tolist() == TC.statuses(name) + [pkg()._lib.TYPESET_EMPTY]
    first = tiles["first"]
    return {(int(t["page"]), int(t["tx"]), int(t["ty"])): [places[i][0] for i in entries[first[k]:first[k + 1]]]
            for k, t in enumerate(tiles[:-1])}


def _grown_meets(layer, place, bitmaps, shape, tile):
    """Whether the placement's glyph, grown by r and cut to page and clip, meets tile (tx, ty)."""
    h, w = bitmaps[place[1]].shape
    x1, y1, x2, y2 = GR._grown(layer, place[2], place[3], w, h, *shape)
    tx, ty = tile
    return h > 0 and w > 0 and max(x1, tx * TC.TW) < min(x2, tx * TC.TW + TC.TW) and max(y1, ty * TC.TH) < min(y2, ty * TC.TH + TC.TH)


def _paste(bitmaps, places, idx, H, W, m=100):
    """The max-paste and the sum of the placements `idx` on a canvas of the page grown by m: (max, sum) int64."""
    mx, sm = np.zeros((H + 2 * m, W + 2 * m), np.int64), np.zeros((H + 2 * m, W + 2 * m), np.int64)
    for i in idx:
        _, g, x, y = places[i]
        b = bitmaps[g].astype(np.int64)
        if b.size:
            v = (slice(y + m, y + m + b.shape[0]), slice(x + m, x + m + b.shape[1]))
            mx[v] = np.maximum(mx[v], b)
            sm[v] += b
    return mx, sm


# ---- the hand-made cases -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", TC.RUN_N)
@pytest.mark.parametrize("r", TC.RUN_R)
def test_run_then_other_has_a_run_of_n_and_a_layer_that_overwrites_it(n, r):
    name = f"run_then_other-n{n}-r{r}"
    pages, bitmaps, layers, places = TC.case(name)
    assert pages[0].shape == (TC.TH, TC.TW, 3) and all(3 <= s <= 6 for b in bitmaps for s in b.shape) and all(b.all() for b in bitmaps)
    assert _tile_runs(name) == {(0, 0, 0): [0] * n + [1] * 3}
    assert layers[0]["r"] == r != layers[1]["r"] and layers[0]["fill"] != layers[1]["fill"] and layers[0]["stroke"] != layers[1]["stroke"]
    want, rows, _ = TC.reference(name)
    alone = GR.typeset(pages, layers[:1], places[:n], bitmaps)[0][0]
    wrote0 = (alone != pages[0]).any(axis=2)
    changed = (want[0] != alone).any(axis=2)
    assert (wrote0 & changed).sum() > 50 and rows[1, 1] > rows[1, 0] > 20 and rows[0, 0] > 500


@pytest.mark.parametrize("n", TC.LAST_N)
@pytest.mark.parametrize("r", TC.RUN_R)
def test_run_is_last_ends_the_entries_at_a_chunk_end(n, r):
    name = f"run_is_last-n{n}-r{r}"
    assert n % TC.NC == 0 and _tile_runs(name) == {(0, 0, 0): [0] * n}
    assert TC.reference(name)[1][0, 0] > 500


def test_cross_chunk_max_has_both_directions_and_first_chunk_only_bytes():
    pages, bitmaps, layers, places = TC.case("cross_chunk_max")
    assert _tile_runs("cross_chunk_max") == {(0, 0, 0): [0] * 300} and layers[0]["r"] == 3
    a, b = bitmaps[places[0][1]].astype(int), bitmaps[places[280][1]].astype(int)
    assert places[0][2:] == places[280][2:] == (50, 20) and a.shape == b.shape == (6, 6)
    assert (a > b).sum() >= 5 and (b > a).sum() >= 5 and a.all() and b.all()
    assert all(q[2] + bitmaps[q[1]].shape[1] <= 48 for i, q in enumerate(places) if i not in (0, 280))   # nobody else reaches them
    m = 100
    f1, _ = _paste(bitmaps, places, range(0, TC.NC), TC.TH, TC.TW, m)
    f2, _ = _paste(bitmaps, places, range(TC.NC, 300), TC.TH, TC.TW, m)
    second = [places[i] for i in range(TC.NC, 300)]
    bx1, by1 = min(q[2] for q in second), min(q[3] for q in second)
    bx2, by2 = max(q[2] + bitmaps[q[1]].shape[1] for q in second), max(q[3] + bitmaps[q[1]].shape[0] for q in second)
    inside = np.zeros_like(f1, bool)
    inside[max(by1, 0) + m:min(by2, TC.TH) + m, max(bx1, 0) + m:min(bx2, TC.TW) + m] = True
    assert ((f1 > 0) & (f2 == 0) & inside).sum() > 100       # the second chunk must keep these
    assert ((f1 > f2) & (f2 > 0)).sum() > 50 and ((f2 > f1) & (f1 > 0)).sum() > 50


@pytest.mark.parametrize("first", (True, False))
def test_idle_chunk_has_no_placement_within_r_of_its_tile(first):
    pages, bitmaps, layers, places = TC.case("idle_chunk-first" if first else "idle_chunk-last")
    assert pages[0].shape == (TC.TH, 2 * TC.TW, 3) and len(places) == 300 and len(layers) == 1 and layers[0]["r"] == 12
    shape = pages[0].shape[:2]
    meets = np.array([[_grown_meets(layers[0], q, bitmaps, shape, (tx, 0)) for q in places] for tx in (0, 1)])
    idle0, busy0 = (slice(0, TC.NC), slice(TC.NC, 300)) if first else (slice(TC.NC, 300), slice(0, TC.NC))
    assert not meets[0, idle0].any() and meets[0, busy0].all()           # tile 0: one chunk idle, the other all there
    assert not meets[1, busy0].any() and meets[1, idle0].all()           # tile 1: the other way round
    assert TC.reference("idle_chunk-first" if first else "idle_chunk-last")[1][0, 0] > 1000


def test_long_run_over_seams_is_multi_chunk_in_every_tile_and_cut_by_its_clip():
    pages, bitmaps, layers, places = TC.case("long_run_over_seams-r12")
    assert pages[0].shape == (2 * TC.TH, 2 * TC.TW, 3) and len(places) == 300 and layers[0]["r"] == 12
    runs = _tile_runs("long_run_over_seams-r12")
    assert sorted(runs) == [(0, 0, 0), (0, 0, 1), (0, 1, 0), (0, 1, 1)] and all(len(v) > TC.NC for v in runs.values())
    cx1, cy1, cx2, cy2 = layers[0]["clip"]
    cut = [q for q in places if (q[2] < cx1 < q[2] + bitmaps[q[1]].shape[1] or q[2] < cx2 < q[2] + bitmaps[q[1]].shape[1] or
                                 q[3] < cy1 < q[3] + bitmaps[q[1]].shape[0] or q[3] < cy2 < q[3] + bitmaps[q[1]].shape[0])]
    assert len(cut) >= 8
    over_x = [q for q in places if q[2] <= 63 and q[2] + bitmaps[q[1]].shape[1] >= 65]
    over_y = [q for q in places if q[3] <= 31 and q[3] + bitmaps[q[1]].shape[0] >= 33]
    assert len(over_x) > 50 and len(over_y) > 50
    want, rows, _ = TC.reference("long_run_over_seams-r12")
    wrote = (want[0] != pages[0]).any(axis=2)
    assert all(wrote[y:y + TC.TH, x:x + TC.TW].sum() > 100 for y in (0, TC.TH) for x in (0, TC.TW))
    assert not wrote[:cy1].any() and not wrote[cy2:].any() and not wrote[:, :cx1].any() and not wrote[:, cx2:].any()


@pytest.mark.parametrize("r,rows", TC.BATCH_ROWS)
def test_batch_rows_gather_the_stated_bytes(r, rows):
    name = f"batch_rows-r{r}-rows{rows}"
    pages, bitmaps, layers, places = TC.case(name)
    x1, y1, x2, y2 = layers[0]["clip"]
    assert (x1, x2) == (0, TC.TW) and 0 <= y1 < y2 <= TC.TH and y2 - y1 == rows and layers[0]["r"] == r
    assert rows + 2 * r == {(0, 32): 32, (1, 30): 32, (1, 31): 33, (12, 8): 32, (12, 9): 33, (12, 32): 56}[(r, rows)]
    n_bytes = (rows + 2 * r) * TC.CW
    assert n_bytes == {32: TC.BATCH, 33: TC.BATCH + TC.CW, 56: 4928}[rows + 2 * r]
    want, rw, _ = TC.reference(name)
    wrote = (want[0] != pages[0]).any(axis=2)
    assert wrote[y1].sum() > 20 and wrote[y2 - 1].sum() > 20 and not wrote[:y1].any() and not wrote[y2:].any()
    assert len(_tile_runs(name)[(0, 0, 0)]) > 40


def test_batch_rows_cover_one_batch_one_batch_and_a_row_and_the_whole_patch():
    assert sorted(rows + 2 * r for r, rows in TC.BATCH_ROWS) == [32, 32, 32, 33, 33, 56]


def test_radius_ladder_has_all_13_radii_on_the_same_pixels():
    pages, bitmaps, layers, places = TC.case("radius_ladder")
    assert [ly["r"] for ly in layers] == list(TC.LADDER) and sorted(TC.LADDER) == list(range(13))
    assert len({ly["fill"] for ly in layers}) == len({ly["stroke"] for ly in layers}) == 13
    assert _tile_runs("radius_ladder")[(0, 0, 0)] == sorted(q[0] for q in places)
    common = np.ones((TC.TH, TC.TW), bool)
    for li in range(13):
        mine = [q for q in places if q[0] == li]
        assert 2 <= len(mine) <= 4
        for _, g, x, y in mine:
            box = np.zeros_like(common)
            box[y:y + bitmaps[g].shape[0], x:x + bitmaps[g].shape[1]] = True
            common &= box
    assert common.sum() >= 4                                 # every glyph of every layer covers these pixels
    _, rows, _ = TC.reference("radius_ladder")
    assert (rows[:, 0] > 0).all() and all((rows[li, 1] > rows[li, 0]) == (r > 0) for li, r in enumerate(TC.LADDER))


@pytest.mark.parametrize("name", [name for name, _, _ in TC.API_CASES])
def test_the_tilted_binning_keeps_what_the_case_is_there_for(name):
    """Through `tilted_kernel` the entries of a tile come from `tilt_tables`: the entry counts the case exists for still occur."""
    pages, bitmaps, layers, places = TC.case(name)
    up, tl = _tile_runs(name), _tilt_runs(name)
    assert sorted(tl) == sorted(up) and all(len(tl[k]) >= len(up[k]) and tl[k] == sorted(tl[k]) for k in up)
    fn, args = TC.CASES[name]
    if fn is TC.run_then_other:
        assert tl == {(0, 0, 0): [0] * args[0] + [1] * 3}
    elif fn is TC.run_is_last:
        assert args[0] % TC.NC == 0 and tl == {(0, 0, 0): [0] * args[0]}
    elif fn is TC.cross_chunk_max:
        assert tl == {(0, 0, 0): [0] * 300}                   # placement 280 is entry 280: in the second chunk
    elif fn is TC.long_run_over_seams:
        assert len(tl) == 4 and all(len(v) > TC.NC for v in tl.values())
    elif fn is TC.batch_rows:
        assert len(tl[(0, 0, 0)]) > 40                        # the bytes gathered come from the clip, which is the layer's
    else:
        assert fn is TC.radius_ladder and tl[(0, 0, 0)] == sorted(q[0] for q in places)


# ---- the sweep -----------------------------------------------------------------------------------------------------------------

def test_the_sweep_covers_what_it_is_there_for():
    assert len(SEEDS) == TC.N_SEEDS >= 16
    radii, status, sides = set(), set(), set()
    corner = maxsum = cut = negative = 0
    for name in SEEDS:
        pages, bitmaps, layers, places = TC.case(name)
        shapes = [pg.shape[:2] for pg in pages]
        assert 1 <= len(pages) <= 3 and 1 <= len(layers) <= 12 and all(1 <= s <= 200 for sh in shapes for s in sh)
        sides |= {s for sh in shapes for s in sh}
        st = TC.statuses(name)
        status |= set(st)
        radii |= {ly["r"] for ly, s in zip(layers, st) if s == TR.OK}
        _, rows, _ = TC.reference(name)
        assert rows[:, 0].sum() > 0, f"{name} writes nothing"
        for li, ly in enumerate(layers):
            H, W = shapes[ly["page"]]
            cx1, cy1, cx2, cy2 = ly.get("clip") or (0, 0, W, H)
            mine = [i for i, q in enumerate(places) if q[0] == li]
            assert len(mine) <= 41
            for i in mine:
                _, g, x, y = places[i]
                h, w = bitmaps[g].shape
                if h == 0 or w == 0:
                    continue
                vx1, vy1, vx2, vy2 = max(x, 0), max(y, 0), min(x + w, W), min(y + h, H)          # the glyph on the page
                if vx1 >= vx2 or vy1 >= vy2:
                    continue
                ix1, iy1, ix2, iy2 = max(vx1, cx1), max(vy1, cy1), min(vx2, cx2), min(vy2, cy2)  # ... and in the clip
                seen = ix1 < ix2 and iy1 < iy2
                cut += seen and (ix2 - ix1) * (iy2 - iy1) < (vx2 - vx1) * (vy2 - vy1)
                negative += seen and (x < 0 or y < 0)
                kx, ky = (ix1 // TC.TW + 1) * TC.TW, (iy1 // TC.TH + 1) * TC.TH                   # the next seams
                corner += seen and ix1 < kx < ix2 and iy1 < ky < iy2
            mx, sm = _paste(bitmaps, places, mine, H, W)
            on_page = (slice(100 + max(cy1, 0), 100 + min(cy2, H)), slice(100 + max(cx1, 0), 100 + min(cx2, W)))
            maxsum += bool((np.minimum(sm, 255) != mx)[on_page].any())
    assert radii == set(range(13)) and status == {TR.OK, TR.EMPTY, TR.OUTSIDE}
    assert set(TC.FORCED) <= sides
    assert corner and maxsum and cut and negative, (corner, maxsum, cut, negative)
    L = pkg()._lib
    assert (L.TYPESET_OK, L.TYPESET_EMPTY, L.TYPESET_OUTSIDE) == (TR.OK, TR.EMPTY, TR.OUTSIDE)


def test_the_sweep_draws_its_values_and_sizes_as_stated():
    sizes, values, colours, kinds = set(), set(), set(), set()
    for name in SEEDS:
        pages, bitmaps, layers, places = TC.case(name)
        sizes |= {bitmaps[q[1]].shape for q in places}
        values |= {int(v) for q in places[:20] for v in np.unique(bitmaps[q[1]])}
        colours |= {c for ly in layers for c in ly["fill"] + ly["stroke"]}
        for ly in layers:
            H, W = pages[ly["page"]].shape[:2]
            c = ly.get("clip")
            kinds.add("none" if c is None else "empty" if c[0] >= c[2] or c[1] >= c[3] else
                      "beyond" if c[0] < 0 and c[1] < 0 and c[2] > W and c[3] > H else "inside" if 0 <= c[0] and c[2] <= W and 0 <= c[1] and c[3] <= H else "cutting")
    assert {(0, 0), (1, 1), (40, 40)} <= sizes and {0, 1, 127, 254, 255} <= values and {0, 255} <= colours
    assert kinds == {"none", "empty", "beyond", "inside", "cutting"}


# ---- the host tables against the brute-force loops, on every case and seed -----------------------------------------------------------

@pytest.mark.parametrize("name", sorted(TC.CASES))
def test_host_tables_equal_the_brute_force_loops(name):
    p = pkg()
    G, T, L = p.glyphs, p.typeset, p._lib
    pages, bitmaps, layers, places = TC.case(name)
    shapes, col = _columns(pages, bitmaps, layers, places)
    tiles, entries, status = G.glyph_tables(shapes, **col)
    wt, we = GR.tables_brute(shapes, layers, places, col["sizes"].tolist(), L.TYPESET_TILE_W, L.TYPESET_TILE_H)
    assert [tuple(int(v) for v in t) for t in tiles[:-1]] == wt[:-1] and int(tiles["first"][-1]) == len(we) == wt[-1][3]
    assert entries.dtype == np.int32 and entries.tolist() == we and status.tolist() == TC.statuses(name)
    bl = GR.composed(layers, places, bitmaps, shapes)
    clip = [ly.get("clip") or (0, 0, shapes[ly["page"]][1], shapes[ly["page"]][0]) for ly in bl]
    tiles, entries, status = T.typeset_tables(shapes, [ly["page"] for ly in bl], [ly["cov"].shape for ly in bl],
                                              [(ly["x0"], ly["y0"]) for ly in bl], [ly["r"] for ly in bl], clip)
    wt, we = TR.tables_brute(shapes, bl, L.TYPESET_TILE_W, L.TYPESET_TILE_H)
    assert [tuple(int(v) for v in t) for t in tiles[:-1]] == wt[:-1] and int(tiles["first"][-1]) == len(we) == wt[-1][3]
    assert entries.tolist() == we and status.tolist() == [TR.status_of(ly, *shapes[ly["page"]]) for ly in bl]
