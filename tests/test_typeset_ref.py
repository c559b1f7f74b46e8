"""Typeset without a GPU: what the rule of include/ctd_hip.h promises, checked on its numpy restatement (tests/typeset_ref.py);
`typeset.typeset_tables` against a brute-force loop over pages, tiles and layers; `typeset.place`; argument checks of
`typeset.typeset_pages`; the ABI structs and constants against the header; the entry point's refusals.  The kernel itself is
compared with the restatement in tests/test_gpu_typeset.py."""
import ctypes as C

import numpy as np
import pytest

import typeset_ref as TR
from c_layout import compiled_flat
from conftest import pkg


# ---- the rule ----------------------------------------------------------------------------------------------------------

def test_blend_identities_over_all_alpha():
    c, k = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    assert np.array_equal(TR.blend(c, k, 0), c) and np.array_equal(TR.blend(c, k, 255), k)      # the endpoints
    for a in range(256):
        b = TR.blend(c, k, a)
        assert (b >= np.minimum(c, k)).all() and (b <= np.maximum(c, k)).all(), a               # always between c and k
        assert np.array_equal(np.diag(b), np.arange(256)), a                                    # a colour onto itself stays
    assert TR.blend(0, 255, 128) == 128 and TR.blend(255, 0, 128) == 127 and TR.blend(10, 20, 127) == 15


def test_disk_sizes_and_half_widths():
    assert {r: len(TR.disk(r)) for r in range(1, 13)} == TR.DISK_SIZES and TR.disk(0) == [(0, 0)]
    for r in range(1, 13):
        d = set(TR.disk(r))
        assert all((-dx, dy) in d and (dx, -dy) in d and (dy, dx) in d for dx, dy in d)
        # a row of the disk is a run -k .. k with k = floor(sqrt(r^2 - dy^2)): what a running horizontal max may rely on
        for dy in range(-r, r + 1):
            xs = sorted(dx for dx, y in d if y == dy)
            k = int(np.floor(np.sqrt(r * r - dy * dy)))
            assert xs == list(range(-k, k + 1))
        assert len({int(np.floor(np.sqrt(r * r - dy * dy))) for dy in range(r + 1)}) <= 9
    # the outline of one pixel is the disk
    for r in (1, 5, 12):
        Fg = np.zeros((4 * r + 1, 4 * r + 1), np.uint8)
        Fg[2 * r, 2 * r] = 200
        S = TR.dilate(Fg, r)
        assert (S > 0).sum() == TR.DISK_SIZES[r] and set(np.unique(S)) == {0, 200}


def test_radius_zero_is_a_plain_alpha_paste_and_full_coverage_gives_the_fill():
    rng = np.random.default_rng(1)
    page = rng.integers(0, 256, (40, 50, 3), dtype=np.uint8)
    cov = TR.noise(12, 17, 3)
    fill = (10, 200, 90)
    out, rows = TR.typeset([page], [TR.layer(0, cov, 7, 9, 0, fill, (255, 0, 255))])
    want = page.copy().astype(np.int64)
    a = cov.astype(np.int64)[..., None]
    want[9:21, 7:24] = (want[9:21, 7:24] * (255 - a) + np.array(fill) * a + 127) // 255
    assert np.array_equal(out[0], want.astype(np.uint8)) and rows.tolist() == [[int((cov > 0).sum()), 0]]
    # coverage 255 gives exactly the fill colour; around it, S = 255 gives exactly the stroke colour; beyond r nothing changes
    out, rows = TR.typeset([page], [TR.layer(0, TR.solid(6, 8), 20, 15, 3, fill, (1, 2, 3))])
    assert (out[0][15:21, 20:28] == np.array(fill, np.uint8)).all()
    ring = np.ones((40, 50), bool)
    ring[15:21, 20:28] = False
    changed = (out[0] != page).any(axis=2)
    assert (out[0][changed & ring] == np.array((1, 2, 3), np.uint8)).all()
    assert not changed[:12].any() and not changed[24:].any() and not changed[:, :17].any() and not changed[:, 31:].any()
    assert rows.tolist() == [[48, (6 + 6) * (8 + 6) - (49 - 29)]]       # the corners lack what a 7 x 7 square has over the disk
    # the order of overlapping layers matters
    pages = TR.small_pages()
    ov = TR.overlapping()
    a, _ = TR.typeset(pages, ov)
    b, _ = TR.typeset(pages, [ov[1], ov[0], ov[2]])
    assert (a[0] != b[0]).sum() > 100
    # invalid layers draw nothing
    bad = [TR.layer(4, cov, 0, 0, 1), TR.layer(-1, cov, 0, 0, 1), TR.layer(0, cov, 0, 0, 13), TR.layer(0, cov, 0, 0, 1, w=8193),
           TR.layer(0, cov, 0, 0, 1, beyond=True), TR.layer(0, np.zeros((0, 4), np.uint8), 0, 0, 1)]
    out, rows = TR.typeset(pages, bad)
    assert all(np.array_equal(x, y) for x, y in zip(out, pages)) and not rows.any()


# ---- the tables -----------------------------------------------------------------------------------------------------------

def _columns(layers):
    page_of = [ly["page"] for ly in layers]
    sizes = [ly["cov"].shape for ly in layers]
    xy = [(ly["x0"], ly["y0"]) for ly in layers]
    radius = [ly["r"] for ly in layers]
    return page_of, sizes, xy, radius


def _clips(layers, shapes):
    return [ly.get("clip") or (0, 0, shapes[ly["page"]][1], shapes[ly["page"]][0]) for ly in layers]


def test_typeset_tables_against_a_brute_force_loop():
    p = pkg()
    T, L = p.typeset, p._lib
    rng = np.random.default_rng(7)
    shapes = TR.SHAPES + [(200, 300)]
    layers = TR.small_layers()
    for i in range(120):                                     # random layers, a third of them with a clip of their own
        pg = int(rng.integers(0, len(shapes)))
        H, W = shapes[pg]
        h, w = int(rng.integers(0, 90)), int(rng.integers(0, 90))
        clip = None
        if i % 3 == 0:
            cx, cy = sorted(rng.integers(-20, W + 20, 2)), sorted(rng.integers(-20, H + 20, 2))
            clip = (int(cx[0]), int(cy[0]), int(cx[1]), int(cy[1]))
        layers.append(TR.layer(pg, np.zeros((h, w), np.uint8), int(rng.integers(-100, W + 20)), int(rng.integers(-100, H + 20)),
                               int(rng.integers(0, 13)), clip=clip))
    tiles, entries, status = T.typeset_tables(shapes, *_columns(layers), _clips(layers, shapes))
    want_tiles, want_entries = TR.tables_brute(shapes, layers, L.TYPESET_TILE_W, L.TYPESET_TILE_H)
    assert tiles.dtype == T.TILE_DTYPE and entries.dtype == np.int32
    assert [tuple(int(v) for v in t) for t in tiles[:-1]] == want_tiles[:-1] and int(tiles["first"][-1]) == len(want_entries)
    assert entries.tolist() == want_entries
    assert status.tolist() == [TR.status_of(ly, *shapes[ly["page"]]) for ly in layers]
    assert {TR.OK, TR.EMPTY, TR.OUTSIDE} == set(status.tolist()) and (L.TYPESET_OK, L.TYPESET_EMPTY, L.TYPESET_OUTSIDE) == (0, 1, 2)
    keys = [tuple(int(v) for v in t)[:3] for t in tiles[:-1]]
    assert len(set(keys)) == len(keys) and keys == sorted(keys, key=lambda k: (k[0], k[2], k[1]))    # once, page- then row-major
    first = tiles["first"].astype(np.int64)
    assert (np.diff(first) > 0).all()
    for a, b in zip(first[:-1], first[1:]):
        assert (np.diff(entries[a:b]) > 0).all()             # ascending within a tile
    assert len(tiles) > 40 and len(entries) > len(layers)    # many layers lie in more than one tile
    # the default clip is the page; one radius / one clip for all layers; no layer at all
    sub = [ly for ly in TR.small_layers() if "clip" not in ly]
    t1, e1, s1 = T.typeset_tables(TR.SHAPES, *_columns(sub))
    t2, e2, s2 = T.typeset_tables(TR.SHAPES, *_columns(sub), _clips(sub, TR.SHAPES))
    assert t1.tobytes() == t2.tobytes() and e1.tobytes() == e2.tobytes() and s1.tolist() == s2.tolist()
    po, sz, xy, _ = _columns(sub)
    t3, e3, _ = T.typeset_tables(TR.SHAPES, po, sz, xy, 4, (10, 10, 60, 60))
    for ly in sub:
        ly["r"], ly["clip"] = 4, (10, 10, 60, 60)
    wt, we = TR.tables_brute(TR.SHAPES, sub, 64, 32)
    assert [tuple(int(v) for v in t) for t in t3[:-1]] == wt[:-1] and e3.tolist() == we
    t0, e0, s0 = T.typeset_tables(TR.SHAPES, [], [], [])
    assert len(t0) == 1 and t0["first"][0] == 0 and len(e0) == 0 and len(s0) == 0
    for bad in (dict(page_of=[4]), dict(page_of=[-1]), dict(sizes=[(8193, 1)]), dict(sizes=[(-1, 1)]), dict(radius=13), dict(radius=-1),
                dict(xy=[(2 ** 29 + 1, 0)]), dict(xy=[(0.5, 0)]), dict(sizes=[(1, 1), (2, 2)]), dict(clip=(0, 0, 1)),
                dict(clip=(0, 0, 2 ** 31, 1)), dict(shapes=[(0, 5)]), dict(shapes=[(8193, 5)]), dict(radius=1.5)):
        kw = dict(shapes=TR.SHAPES, page_of=[0], sizes=[(3, 3)], xy=[(0, 0)], radius=0, clip=None)
        kw.update(bad)
        with pytest.raises(ValueError):
            T.typeset_tables(**kw)


def test_place_on_even_and_odd_slack_and_on_a_bitmap_larger_than_its_box():
    T = pkg().typeset
    rects = [(10, 20, 30, 40), (10, 20, 31, 41), (10, 20, 30, 40), (10, 20, 30, 40), (0, 0, 5, 5)]
    sizes = [(10, 10), (10, 10), (26, 30), (20, 20), (5, 5)]                   # (h, w)
    xy, fits = T.place(rects, sizes)
    assert xy.tolist() == [[15, 25], [15, 25], [5, 17], [10, 20], [0, 0]]       # odd slack: the odd pixel goes right and down
    assert fits.tolist() == [True, True, False, True, True]
    xy2, fits2 = T.place(rects, sizes, radius=[5, 6, 0, 1, 0])
    assert np.array_equal(xy, xy2) and fits2.tolist() == [True, False, False, False, True]
    assert T.place([(0, 0, 4, 4)], [(7, 5)])[0].tolist() == [[-1, -2]]          # -1 >> 1 = -1, -3 >> 1 = -2: the floor, not toward 0
    e = T.place(np.zeros((0, 4), np.int64), np.zeros((0, 2), np.int64))
    assert e[0].shape == (0, 2) and e[1].shape == (0,)
    with pytest.raises(ValueError):
        T.place([(0, 0, 4, 4)], [(1, 1), (2, 2)])


def test_typeset_pages_argument_checks_need_no_gpu():
    p = pkg()
    T = p.typeset
    page = np.zeros((20, 30, 3), np.uint8)
    bm = np.full((3, 4), 255, np.uint8)
    ok = dict(pages=[page], page_of=[0], bitmaps=[bm], xy=[(1, 1)])
    for bad in (dict(pages=[page[..., 0]]), dict(pages=[page.astype(np.float32)]), dict(page_of=[1]), dict(page_of=[0, 0]),
                dict(bitmaps=[bm.astype(np.int32)]), dict(bitmaps=[bm[None]]), dict(bitmaps=[bm.tolist()]), dict(xy=[(1, 1, 1)]),
                dict(xy=[(0.5, 1)]), dict(fill=(0, 0)), dict(fill=(0, 0, 256)), dict(stroke=(-1, 0, 0)), dict(stroke=(0.5, 0, 0)),
                dict(radius=13), dict(radius=-1), dict(radius=[1, 2]), dict(clip=(0, 0, 5)), dict(inplace=True)):
        kw = dict(ok)
        kw.update(bad)
        with pytest.raises(ValueError):
            T.typeset_pages(**kw)
    import torch
    if not torch.cuda.is_available():
        with pytest.raises(p._lib.CtdError):
            T.typeset_pages(**ok)
        with pytest.raises(p._lib.CtdError):
            T.typeset_pages([page], [], [], np.zeros((0, 2), np.int64))


# ---- ABI -------------------------------------------------------------------------------------------------------------------

def test_typeset_structs_have_the_c_layout():
    """`typeset.*_DTYPE` and the `_lib` mirrors against the header, compiled: sizes, every field's offset, the constants; the
    entry point is exported and bound, refuses bad arguments before it launches anything, and takes the n = 0 call."""
    p = pkg()
    L, T = p._lib, p.typeset
    fields = {"ctd_typeset_page": ("page_dev", "H", "W", "pitch"),
              "ctd_typeset_layer": ("cov0", "page", "x0", "y0", "w", "h", "cov_pitch", "clip", "fill", "stroke", "radius", "pad_"),
              "ctd_typeset_tile": ("page", "tx", "ty", "first"),
              "ctd_typeset_params": ("n_layers", "n_pages", "n_tiles", "n_entries", "cov_bytes", "pad_"),
              "ctd_typeset_row": ("n_fill", "n_stroke")}
    consts = ("CTD_TYPESET_MAX_SIDE", "CTD_TYPESET_MAX_RADIUS", "CTD_TYPESET_TILE_W", "CTD_TYPESET_TILE_H", "CTD_ABI_VERSION")
    vals = compiled_flat(fields, consts)
    mirrors = {"ctd_typeset_page": (L.CtdTypesetPage, T.PAGE_DTYPE, 24), "ctd_typeset_layer": (L.CtdTypesetLayer, T.LAYER_DTYPE, 56),
               "ctd_typeset_tile": (L.CtdTypesetTile, T.TILE_DTYPE, 16), "ctd_typeset_params": (L.CtdTypesetParams, None, 32),
               "ctd_typeset_row": (L.CtdTypesetRow, T.ROW_DTYPE, 8)}
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
    assert vals[k:k + 2] == [TR.MAX_SIDE, TR.MAX_RADIUS] == [8192, 12] and vals[-1] == 10
    assert "ctd_typeset" in L.SYMBOLS and hasattr(L.lib(), "ctd_typeset")
    # the entry point refuses before anything else (nothing is launched: no GPU is needed)
    lib = L.lib()
    good = (1, 1, 1, 1, 16)
    for i in range(5):                                       # a negative count, a negative cov_bytes
        v = list(good)
        v[i] = -1
        assert lib.ctd_typeset(8, 8, 8, 8, 8, C.byref(L.CtdTypesetParams(*v)), 8, None) != L.OK, v
    assert b"bad sizes" in lib.ctd_last_error()
    prm = L.CtdTypesetParams(*good)
    assert lib.ctd_typeset(8, 8, 8, 8, 8, None, 8, None) != L.OK
    for i in (0, 1, 2, 3, 4, 6):                             # a missing table where its count is positive; cov NULL with bytes
        args = [8, 8, 8, 8, 8, C.byref(prm), 8, None]
        args[i] = None
        assert lib.ctd_typeset(*args) != L.OK, i
    assert b"null" in lib.ctd_last_error()
    # n_layers = 0: nothing to clear, nothing to launch, with or without tiles
    assert lib.ctd_typeset(None, None, None, None, None, C.byref(L.CtdTypesetParams(0, 0, 0, 0, 0)), None, None) == L.OK
    assert lib.ctd_typeset(8, None, 8, None, None, C.byref(L.CtdTypesetParams(0, 3, 2, 0, 0)), None, None) == L.OK
