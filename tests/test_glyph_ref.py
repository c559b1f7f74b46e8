"""Typeset from a glyph atlas without a GPU: `glyphs.glyph_tables` against a brute-force loop over pages, tiles and placements
(tests/glyph_ref.py); its status column; `glyphs.flow` against a scalar loop, and its properties; the composed bitmaps of the
restatement; the ABI structs and constants against the header; the entry point's refusals.  The kernel itself is compared
with the restatement, and with `typeset_pages` on the same bitmaps, in tests/test_gpu_glyphs.py."""
import ctypes as C
import types

import numpy as np
import pytest

import glyph_ref as GR
import typeset_ref as TR
from c_layout import compiled_flat
from conftest import pkg


def _columns(layers, places, atlas):
    return dict(page_of=[ly["page"] for ly in layers], layer_of=[p[0] for p in places],
                sizes=np.array([atlas[p[1]].shape for p in places], np.int64).reshape(-1, 2),
                xy=np.array([(p[2], p[3]) for p in places], np.int64).reshape(-1, 2), radius=[ly["r"] for ly in layers])


def _clips(layers, shapes):
    return [ly.get("clip") or (0, 0, shapes[ly["page"]][1], shapes[ly["page"]][0]) for ly in layers]


def _check_tables(G, L, shapes, layers, places, atlas):
    col = _columns(layers, places, atlas)
    tiles, entries, status = G.glyph_tables(shapes, clip=_clips(layers, shapes), **col)
    want_tiles, want_entries = GR.tables_brute(shapes, layers, places, col["sizes"].tolist(), L.TYPESET_TILE_W, L.TYPESET_TILE_H)
    assert tiles.dtype == G.TILE_DTYPE and entries.dtype == np.int32
    assert [tuple(int(v) for v in t) for t in tiles[:-1]] == want_tiles[:-1] and int(tiles["first"][-1]) == len(want_entries)
    assert entries.tolist() == want_entries
    assert status.tolist() == [GR.status_of(li, layers, places, col["sizes"].tolist(), shapes) for li in range(len(layers))]
    keys = [tuple(int(v) for v in t)[:3] for t in tiles[:-1]]
    assert len(set(keys)) == len(keys) and keys == sorted(keys, key=lambda k: (k[0], k[2], k[1]))    # once, page- then row-major
    first = tiles["first"].astype(np.int64)
    assert (np.diff(first) > 0).all()
    lay = np.array(col["layer_of"], np.int64)
    for a, b in zip(first[:-1], first[1:]):
        assert (np.diff(entries[a:b]) > 0).all() and (np.diff(lay[entries[a:b]]) >= 0).all()   # ascending: layers consecutive
    return tiles, entries, status


def test_glyph_tables_against_a_brute_force_loop():
    p = pkg()
    G, L = p.glyphs, p._lib
    assert G.TILE_DTYPE is p.typeset.TILE_DTYPE
    atlas = GR.small_atlas()
    layers, places = GR.small_case()
    tiles, entries, status = _check_tables(G, L, TR.SHAPES, layers, places, atlas)
    assert {TR.OK, TR.EMPTY, TR.OUTSIDE} == set(status.tolist()) and status.tolist().count(TR.EMPTY) == 2
    assert (L.TYPESET_OK, L.TYPESET_EMPTY, L.TYPESET_OUTSIDE) == (TR.OK, TR.EMPTY, TR.OUTSIDE)
    assert len(entries) > len(places)                        # glyphs lie in more than one tile
    # random runs on random layers, a third of them with a clip of their own
    rng = np.random.default_rng(11)
    shapes = TR.SHAPES + [(200, 300)]
    layers, places = [], []
    for li in range(40):
        pg = int(rng.integers(0, len(shapes)))
        H, W = shapes[pg]
        clip = None
        if li % 3 == 0:
            cx, cy = sorted(rng.integers(-20, W + 20, 2)), sorted(rng.integers(-20, H + 20, 2))
            clip = (int(cx[0]), int(cy[0]), int(cx[1]), int(cy[1]))
        layers.append(GR.glayer(pg, int(rng.integers(0, 13)), clip=clip))
        for _ in range(int(rng.integers(0, 9))):
            places.append((li, int(rng.integers(0, len(atlas))), int(rng.integers(-60, W + 30)), int(rng.integers(-60, H + 30))))
    _check_tables(G, L, shapes, layers, places, atlas)
    # the default clip is the page; one radius and one clip for all layers; nothing at all
    layers, places = GR.small_case()
    sub = [dict(ly) for ly in layers]
    for ly in sub:
        ly.pop("clip", None)
    col = _columns(sub, places, atlas)
    t1, e1, s1 = G.glyph_tables(TR.SHAPES, **col)
    t2, e2, s2 = G.glyph_tables(TR.SHAPES, clip=_clips(sub, TR.SHAPES), **col)
    assert t1.tobytes() == t2.tobytes() and e1.tobytes() == e2.tobytes() and s1.tolist() == s2.tolist()
    col["radius"] = 4
    t3, e3, _ = G.glyph_tables(TR.SHAPES, clip=(10, 10, 60, 60), **col)
    for ly in sub:
        ly["r"], ly["clip"] = 4, (10, 10, 60, 60)
    wt, we = GR.tables_brute(TR.SHAPES, sub, places, col["sizes"].tolist(), 64, 32)
    assert [tuple(int(v) for v in t) for t in t3[:-1]] == wt[:-1] and e3.tolist() == we
    t0, e0, s0 = G.glyph_tables(TR.SHAPES, [], [], np.zeros((0, 2), np.int64), np.zeros((0, 2), np.int64))
    assert len(t0) == 1 and t0["first"][0] == 0 and len(e0) == 0 and len(s0) == 0
    t0, e0, s0 = G.glyph_tables(TR.SHAPES, [0, 3], [], np.zeros((0, 2), np.int64), np.zeros((0, 2), np.int64))
    assert len(t0) == 1 and len(e0) == 0 and s0.tolist() == [TR.EMPTY, TR.EMPTY]


def test_one_placement_per_layer_gives_the_tables_of_typeset_tables():
    """Both calls bin through one `_bin_tiles`: a layer that is one glyph is a bitmap layer, so on the same rectangles
    `glyph_tables` returns the bytes of `typeset_tables`: the tiles, the entries (a placement's index is its layer's) and
    the status.  The hand-made layers of tests/typeset_ref.py (every radius, clips, empty and outside ones) and seeded
    random ones, a third with a clip of their own, on `TR.SHAPES` and a page of several tiles both ways."""
    p = pkg()
    G, T = p.glyphs, p.typeset
    assert G._bin_tiles is T._bin_tiles
    rng = np.random.default_rng(7)
    shapes = TR.SHAPES + [(200, 300)]
    layers = TR.small_layers()
    for i in range(120):
        pg = int(rng.integers(0, len(shapes)))
        H, W = shapes[pg]
        clip = None
        if i % 3 == 0:
            cx, cy = sorted(rng.integers(-20, W + 20, 2)), sorted(rng.integers(-20, H + 20, 2))
            clip = (int(cx[0]), int(cy[0]), int(cx[1]), int(cy[1]))
        layers.append(TR.layer(pg, np.zeros((int(rng.integers(0, 90)), int(rng.integers(0, 90))), np.uint8),
                               int(rng.integers(-100, W + 20)), int(rng.integers(-100, H + 20)), int(rng.integers(0, 13)), clip=clip))
    page_of, radius = [ly["page"] for ly in layers], [ly["r"] for ly in layers]
    sizes, xy = [ly["cov"].shape for ly in layers], [(ly["x0"], ly["y0"]) for ly in layers]
    seen, most = set(), 0
    for clip in (_clips(layers, shapes), None, (10, 10, 60, 60)):
        for r in (radius, 0, 12):
            t1, e1, s1 = T.typeset_tables(shapes, page_of, sizes, xy, r, clip)
            t2, e2, s2 = G.glyph_tables(shapes, page_of, np.arange(len(layers)), sizes, xy, r, clip)
            assert t1.dtype == t2.dtype and t1.tobytes() == t2.tobytes() and len(t1) > 1
            assert e1.dtype == e2.dtype == np.int32 and e1.tobytes() == e2.tobytes() and len(e1) > len(t1)
            assert s1.dtype == s2.dtype and s1.tolist() == s2.tolist()
            seen |= set(s1.tolist())
            most = max(most, len(t1))
    assert seen == {TR.OK, TR.EMPTY, TR.OUTSIDE} and most > 40           # the page clips: tiles of every page


def test_glyph_tables_refusals():
    G = pkg().glyphs
    ok = dict(shapes=TR.SHAPES, page_of=[0, 0], layer_of=[0, 1], sizes=[(3, 3), (3, 3)], xy=[(0, 0), (5, 5)], radius=0, clip=None)
    G.glyph_tables(**ok)
    for bad in (dict(layer_of=[1, 0]), dict(layer_of=[0, 2]), dict(layer_of=[-1, 0]), dict(layer_of=[0]), dict(page_of=[0, 4]),
                dict(page_of=[-1, 0]), dict(sizes=[(8193, 1), (1, 1)]), dict(sizes=[(-1, 1), (1, 1)]), dict(radius=13),
                dict(radius=-1), dict(radius=[1, 2, 3]), dict(radius=1.5), dict(xy=[(2 ** 29 + 1, 0), (0, 0)]),
                dict(xy=[(0.5, 0), (0, 0)]), dict(xy=[(0, 0)]), dict(clip=(0, 0, 1)), dict(clip=(0, 0, 2 ** 31, 1)),
                dict(shapes=[(0, 5)]), dict(shapes=[(8193, 5)])):
        kw = dict(ok)
        kw.update(bad)
        with pytest.raises(ValueError):
            G.glyph_tables(**kw)


def test_composed_bitmaps_are_a_max_paste():
    """What both GPU comparisons stand on: overlap is max and not sum, a glyph placed twice counts once, invalid placements
    and glyphs without pixels leave nothing, and what lies beyond the page grown by r is cut off."""
    atlas = GR.small_atlas()
    ly = GR.glayer(0, 2)
    a = GR.compose(0, ly, [(0, 5, 10, 90), (0, 6, 20, 95)], atlas, (130, 70))
    assert (a["x0"], a["y0"]) == (10, 90) and a["cov"].shape == (24, 34)
    want = np.zeros((24, 34), np.int64)
    want[:24, :24] = atlas[5]
    both = want.copy()
    both[5:21, 10:34] = np.maximum(both[5:21, 10:34], atlas[6])
    assert np.array_equal(a["cov"], both)
    summed = want.copy()
    summed[5:21, 10:34] += atlas[6]
    assert (np.minimum(summed, 255) != both).any()          # a saturating sum would be another bitmap
    twice = GR.compose(0, ly, [(0, 5, 10, 90), (0, 6, 20, 95), (0, 5, 10, 90)], atlas, (130, 70))
    assert np.array_equal(twice["cov"], a["cov"])            # idempotent
    bad = [(0, 5, 10, 90), (1, 6, 0, 0), (0, 10, 0, 0), (0, -1, 0, 0), (0, 3, 0, 0), (0, 7, 0, 0), (0, 6, 2 ** 29 + 1, 0)]
    only = GR.compose(0, ly, bad, atlas, (130, 70))
    assert np.array_equal(only["cov"], atlas[5]) and (only["x0"], only["y0"]) == (10, 90)
    assert GR.compose(0, ly, bad, atlas, (130, 70), beyond={5})["cov"].size == 0
    far = GR.compose(0, ly, [(0, 5, -500, 10), (0, 5, 60, 10)], atlas, (130, 70))
    assert (far["x0"], far["cov"].shape) == (-3, (24, 76))   # cut to the page grown by r + 1
    pages = TR.small_pages()
    layers, places = GR.small_case()
    out, rows, bl = GR.typeset(pages, layers, places, atlas)
    assert len(bl) == len(layers) and rows[:9, 0].min() > 0 and not rows[9:12].any()
    assert [i for i, (x, y) in enumerate(zip(out, pages)) if not np.array_equal(x, y)] == [0, 1, 2, 3]
    ov_l, ov_p = GR.overlapping()
    a = GR.typeset(pages, ov_l, ov_p, atlas)[0]
    b = GR.typeset(pages, ov_l[::-1], [(1 - p[0],) + p[1:] for p in ov_p[2:] + ov_p[:2]], atlas)[0]
    assert (a[0] != b[0]).sum() > 100                        # the order of overlapping layers matters


# ---- flow ---------------------------------------------------------------------------------------------------------------------

def _metrics(seed=3, n=12):
    rng = np.random.default_rng(seed)
    sizes = rng.integers(0, 20, (n, 2))
    sizes[0] = (0, 0)
    advance = np.stack([sizes[:, 1] + rng.integers(0, 4, n), sizes[:, 0] + rng.integers(0, 4, n)], axis=1)
    advance[0] = (6, 6)                                      # a space: no pixels, an advance
    advance[1] = (0, 0)                                      # a combining mark: no advance
    bearing = rng.integers(-2, 3, (n, 2))
    return types.SimpleNamespace(sizes=sizes.astype(np.int64), advance=advance.astype(np.int64), bearing=bearing.astype(np.int64))


def test_flow_against_a_scalar_loop():
    G = pkg().glyphs
    m = _metrics()
    rng = np.random.default_rng(4)
    n_fit = n_not = n_hard = 0
    for case in range(300):
        n = int(rng.integers(0, 40))
        ids = rng.integers(0, len(m.sizes), n)
        w, h = int(rng.integers(1, 200)), int(rng.integers(1, 200))
        x1, y1 = int(rng.integers(-50, 50)), int(rng.integers(-50, 50))
        rect = (x1, y1, x1 + w, y1 + h)
        kw = dict(vertical=bool(case & 1), align=("left", "center", "right")[case % 3], gap=int(rng.integers(0, 5)))
        if case % 4 >= 2:
            kw["breaks"] = rng.random(n) < (0.0 if case % 8 == 2 else 0.3)
        if case % 5 == 0:
            kw["line"] = int(rng.integers(0, 30))
        xy, fits = G.flow(ids, m, rect, **kw)
        want, want_fits = GR.flow_brute(ids.tolist(), m.sizes.tolist(), m.advance.tolist(), m.bearing.tolist(), rect, **kw)
        assert xy.shape == (n, 2) and xy.dtype == np.int64
        assert [tuple(v) for v in xy.tolist()] == want and fits is want_fits, (case, kw)
        n_fit += fits
        n_not += not fits
        n_hard += "breaks" in kw and not kw["breaks"].any() and n > 3
    assert n_fit > 40 and n_not > 40 and n_hard > 5


def test_flow_properties():
    """Order is kept; where `fits`, no glyph's advance cell leaves the box; the documented positions on a hand-made run."""
    G = pkg().glyphs
    sizes = np.array([(10, 8)] * 6 + [(4, 4)], np.int64)     # (h, w)
    m = types.SimpleNamespace(sizes=sizes, advance=sizes[:, ::-1].copy(), bearing=np.zeros((7, 2), np.int64))
    xy, fits = G.flow([0, 1, 2, 3, 4], m, (100, 50, 120, 80))                # 20 wide: two glyphs a line, three lines of 10
    assert fits and xy.tolist() == [[102, 50], [110, 50], [102, 60], [110, 60], [106, 70]]
    xy, fits = G.flow([0, 1, 2, 3, 4], m, (100, 50, 120, 80), align="left", gap=1)
    assert not fits and xy.tolist() == [[100, 49], [108, 49], [100, 60], [108, 60], [100, 71]]   # 32 high in 30: overhangs evenly
    xy, fits = G.flow([0, 1, 2, 3, 4], m, (100, 50, 120, 80), align="right", breaks=np.array([0, 0, 1, 0, 0], bool))
    assert xy.tolist() == [[104, 50], [112, 50], [112, 60], [104, 70], [112, 70]]     # hard break after 1, allowed one after 2
    xy, fits = G.flow([0, 6, 2], m, (0, 0, 30, 15), vertical=True)           # columns of 8 from the right, two glyphs in the first
    assert fits and xy.tolist() == [[15, 0], [17, 10], [7, 2]]               # the 4-wide glyph centred in its column
    assert G.flow([0], m, (0, 0, 5, 40))[1] is False and G.flow([], m, (0, 0, 5, 5))[0].shape == (0, 2)
    rng = np.random.default_rng(8)
    for case in range(200):
        n = int(rng.integers(1, 30))
        ids = rng.integers(0, 7, n)
        rect = (5, 7, 5 + int(rng.integers(4, 120)), 7 + int(rng.integers(4, 120)))
        vertical = bool(case & 1)
        xy, fits = G.flow(ids, m, rect, vertical=vertical, align=("left", "center", "right")[case % 3])
        a, c = (1, 0) if vertical else (0, 1)                # the axis along a line, and across
        for i in range(1, n):                                # reading order: along the line, else on to the next line
            assert xy[i, a] >= xy[i - 1, a] + m.advance[ids[i - 1], a] or (xy[i, c] < xy[i - 1, c] if vertical else xy[i, c] > xy[i - 1, c])
        if fits:
            assert xy[:, 0].min() >= rect[0] and xy[:, 1].min() >= rect[1]
            assert (xy[:, 0] + sizes[ids, 1]).max() <= rect[2] and (xy[:, 1] + sizes[ids, 0]).max() <= rect[3]
    for bad in (dict(align="middle"), dict(breaks=[True]), dict(line=-1)):
        with pytest.raises(ValueError):
            G.flow([0, 1], m, (0, 0, 50, 50), **bad)
    with pytest.raises(ValueError):
        G.flow([7], m, (0, 0, 50, 50))
    with pytest.raises(ValueError):
        G.flow([0], m, (0, 0, 50))


# ---- ABI ---------------------------------------------------------------------------------------------------------------------

def test_glyph_structs_have_the_c_layout():
    """`glyphs.*_DTYPE` and the `_lib` mirrors against the header, compiled: sizes, every field's offset, the constants; the
    entry point is exported and bound, refuses bad arguments before it launches anything, and takes the empty call."""
    p = pkg()
    L, G = p._lib, p.glyphs
    fields = {"ctd_glyph_layer": ("page", "clip", "fill", "stroke", "radius", "pad_", "pad2_"),
              "ctd_glyph_place": ("layer", "glyph", "x", "y"),
              "ctd_glyph_record": ("off", "w", "h"),
              "ctd_glyph_params": ("n_layers", "n_pages", "n_tiles", "n_entries", "n_places", "n_glyphs", "atlas_bytes")}
    consts = ("CTD_TYPESET_MAX_SIDE", "CTD_TYPESET_MAX_RADIUS", "CTD_TYPESET_TILE_W", "CTD_TYPESET_TILE_H", "CTD_ABI_VERSION")
    vals = compiled_flat(fields, consts)
    mirrors = {"ctd_glyph_layer": (L.CtdGlyphLayer, G.LAYER_DTYPE, 32), "ctd_glyph_place": (L.CtdGlyphPlace, G.PLACE_DTYPE, 16),
               "ctd_glyph_record": (L.CtdGlyphRecord, G.RECORD_DTYPE, 16), "ctd_glyph_params": (L.CtdGlyphParams, None, 32)}
    k = 0
    for s, fs in fields.items():
        ct, dt, size = mirrors[s]
        assert vals[k] == C.sizeof(ct) == size and (dt is None or dt.itemsize == size), s
        assert vals[k + 1:k + 1 + len(fs)] == [getattr(ct, f).offset for f in fs], s
        assert [f for f, _ in ct._fields_] == list(fs)
        if dt is not None:
            assert vals[k + 1:k + 1 + len(fs)] == [dt.fields[f][1] for f in fs] and dt.names == fs, s
        k += 1 + len(fs)
    assert vals[k:] == [L.TYPESET_MAX_SIDE, L.TYPESET_MAX_RADIUS, L.TYPESET_TILE_W, L.TYPESET_TILE_H, L.ABI_VERSION]
    assert vals[-1] == 10                                    # added within ABI v10
    assert "ctd_typeset_glyphs" in L.SYMBOLS and hasattr(L.lib(), "ctd_typeset_glyphs")
    # the entry point refuses before anything else (nothing is launched: no GPU is needed)
    lib = L.lib()
    good = (1, 1, 1, 1, 1, 1, 16)
    for i in range(7):                                       # a negative count, a negative atlas_bytes
        v = list(good)
        v[i] = -1
        assert lib.ctd_typeset_glyphs(8, 8, 8, 8, 8, 8, 8, C.byref(L.CtdGlyphParams(*v)), 8, None) != L.OK, v
    assert b"bad sizes" in lib.ctd_last_error()
    prm = L.CtdGlyphParams(*good)
    assert lib.ctd_typeset_glyphs(8, 8, 8, 8, 8, 8, 8, None, 8, None) != L.OK
    for i in (0, 1, 2, 3, 4, 5, 6, 8):                       # a missing table where its count is positive; atlas NULL with bytes
        args = [8, 8, 8, 8, 8, 8, 8, C.byref(prm), 8, None]
        args[i] = None
        assert lib.ctd_typeset_glyphs(*args) != L.OK, i
    assert b"null" in lib.ctd_last_error()
    # no tiles or no layers: nothing at all, whatever else is there
    assert lib.ctd_typeset_glyphs(None, None, None, None, None, None, None, C.byref(L.CtdGlyphParams(0, 0, 0, 0, 0, 0, 0)), None, None) == L.OK
    assert lib.ctd_typeset_glyphs(8, 8, 8, 8, None, None, 8, C.byref(L.CtdGlyphParams(3, 3, 0, 0, 5, 5, 64)), 8, None) == L.OK
    assert lib.ctd_typeset_glyphs(8, None, 8, 8, 8, 8, 8, C.byref(L.CtdGlyphParams(0, 3, 2, 4, 5, 5, 64)), None, None) == L.OK


def test_the_atlas_needs_a_gpu():
    import torch
    p = pkg()
    assert p.glyphs.__name__.endswith(".glyphs")             # in the package's lazy module list
    if not torch.cuda.is_available():
        with pytest.raises(p._lib.CtdError):
            p.glyphs.GlyphAtlas()
    page = np.zeros((20, 30, 3), np.uint8)
    with pytest.raises(ValueError):
        p.glyphs.typeset_glyphs([page], None, [0], [0], [0], [(1, 1)])      # no atlas: refused before anything else
    with pytest.raises(ValueError):
        p.glyphs.typeset_glyphs([page[..., 0]], None, [0], [0], [0], [(1, 1)])
