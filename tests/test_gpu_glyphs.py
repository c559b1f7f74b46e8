"""-m gpu: typeset from a glyph atlas -- `ctd_typeset_glyphs` (csrc/kernels_glyphs.hip), `glyphs.GlyphAtlas`,
`glyphs.typeset_glyphs` and `TextDetector.typeset_glyphs` -- against TWO oracles that share the composed block bitmaps of
tests/glyph_ref.py (a layer's valid placements max-pasted, one glyph after the other) and nothing else: the sequential numpy
restatement `typeset_ref.typeset` for every page byte and every row field, and `typeset.typeset_pages`, the bitmap kernel,
for the pages byte for byte.  Integers only, so every comparison is EXACT.  The placements the kernel must refuse are driven
through ctypes with tables that list every placement in every tile."""
import ctypes as C

import numpy as np
import pytest
import torch

import glyph_ref as GR
import test_gpu_regions as TG
import typeset_ref as TR
from conftest import pkg

pytestmark = pytest.mark.gpu

GUARD = 0xA5


def _rgb(c):
    return tuple(c)[::-1]                                   # the restatement's colours are in page (BGR) order


def _same(got_pages, want_pages):
    return [i for i, (g, w) in enumerate(zip(got_pages, want_pages)) if g.shape != w.shape or not np.array_equal(g, w)]


def _atlas(p, bitmaps):
    a = p.glyphs.GlyphAtlas()
    ids = a.add(bitmaps)
    assert ids.tolist() == list(range(len(bitmaps))) and ids.dtype == np.int32
    return a


def _args(pages, layers, places):
    shapes = [tuple(pg.shape[:2]) for pg in pages]
    clip = [ly.get("clip") or (0, 0, shapes[ly["page"]][1], shapes[ly["page"]][0]) for ly in layers]
    return dict(page_of=[ly["page"] for ly in layers], layer_of=[q[0] for q in places], glyph=[q[1] for q in places],
                xy=np.array([(q[2], q[3]) for q in places], np.int64).reshape(-1, 2),
                fill=np.array([_rgb(ly["fill"]) for ly in layers], np.int64).reshape(-1, 3),
                stroke=np.array([_rgb(ly["stroke"]) for ly in layers], np.int64).reshape(-1, 3),
                radius=np.array([ly["r"] for ly in layers], np.int64), clip=np.array(clip, np.int64).reshape(-1, 4))


def _bitmap_api(p, pages, bl, **kw):
    """`typeset.typeset_pages`, the bitmap kernel, on the composed bitmap layers."""
    shapes = [tuple(pg.shape[:2]) for pg in pages]
    clip = [ly.get("clip") or (0, 0, shapes[ly["page"]][1], shapes[ly["page"]][0]) for ly in bl]
    return p.typeset.typeset_pages(pages, [ly["page"] for ly in bl], [ly["cov"] for ly in bl],
                                   np.array([(ly["x0"], ly["y0"]) for ly in bl], np.int64).reshape(-1, 2),
                                   fill=np.array([_rgb(ly["fill"]) for ly in bl], np.int64).reshape(-1, 3),
                                   stroke=np.array([_rgb(ly["stroke"]) for ly in bl], np.int64).reshape(-1, 3),
                                   radius=np.array([ly["r"] for ly in bl], np.int64),
                                   clip=np.array(clip, np.int64).reshape(-1, 4), **kw)


def _both(p, pages, layers, places, bitmaps, atlas=None, **kw):
    """One `typeset_glyphs` call against both oracles: the restatement (pages and rows) and the bitmap kernel (pages)."""
    atlas = _atlas(p, bitmaps) if atlas is None else atlas
    want, want_rows, bl = GR.typeset(pages, layers, places, bitmaps)
    tp = p.glyphs.typeset_glyphs(pages, atlas, **_args(pages, layers, places), **kw)
    got = tp.to_host()
    assert not _same(got, want), f"pages {_same(got, want)} differ from the restatement"
    assert np.array_equal(np.stack([tp.n_fill, tp.n_stroke], axis=1), want_rows)
    other = _bitmap_api(p, pages, bl).to_host()
    assert not _same(got, other), f"pages {_same(got, other)} differ from typeset_pages on the composed bitmaps"
    return tp, want, want_rows, bl


_REF = {}


def _small():
    """The small pages, their glyph layers and the restatement's answer, computed once."""
    if "small" not in _REF:
        pages, bitmaps = TR.small_pages(), GR.small_atlas()
        layers, places = GR.small_case()
        _REF["small"] = (pages, bitmaps, layers, places) + GR.typeset(pages, layers, places, bitmaps)
    return _REF["small"]


# ---- 1. the small pages ------------------------------------------------------------------------------------------------------

def test_small_pages_equal_both_oracles_in_every_byte():
    """One call over the four small pages with 13 hand-made glyph layers; the material holds what its comments promise."""
    p = pkg()
    pages, bitmaps, layers, places, want, want_rows, bl = _small()
    assert [pg.shape[:2] for pg in pages] == [(130, 70), (32, 64), (1, 1), (67, 129)]
    sizes = [bitmaps[q[1]].shape for q in places]
    # a glyph across the tile corner x = 63/64, y = 31/32
    g, x, y = places[0][1:]
    assert x <= 63 < 64 < x + bitmaps[g].shape[1] and y <= 31 < 32 < y + bitmaps[g].shape[0]
    # r = 12 with a glyph 11 / 12 pixels inside the neighbouring tile: only the halo of the first reaches tile 0
    assert layers[1]["r"] == 12 and [q[2] for q in places if q[0] == 1] == [64 + 11, 64 + 12]
    assert want_rows[1, 1] > want_rows[1, 0] == 128
    halo = (want[3][:, :64] != pages[3][:, :64]).any(axis=2)
    assert halo[10:18, 52:].any() and not halo[40:48, 52:].any()
    # two glyphs of one layer overlap, and the max is not the sum
    a, b = bitmaps[5].astype(np.int64), bitmaps[6].astype(np.int64)
    assert ((a[5:21, 10:24] > 0) & (b[:, :14] > 0)).any() and (np.minimum(a[5:21, 10:24] + b[:, :14], 255) != np.maximum(a[5:21, 10:24], b[:, :14])).any()
    assert sum(1 for q in places if q[0] == 3 and q[1] == 4) == 50          # one glyph id 50 times
    run = [q[1] for q in places if q[0] == 4]
    assert bitmaps[run[1]].size == 0 and bitmaps[run[3]].size == 0 and bitmaps[run[0]].size and bitmaps[run[4]].size
    assert "clip" in layers[5] and want_rows[5, 0] < (bitmaps[6] > 0).sum()  # the clip cuts the glyph
    status = [GR.status_of(li, layers, places, sizes, TR.SHAPES) for li in range(len(layers))]
    assert status.count(TR.EMPTY) == 2 and status.count(TR.OUTSIDE) == 1
    tp, _, _, _ = _both(p, pages, layers, places, bitmaps)
    assert tp.status.tolist() == status and len(tp) == len(layers) and tp.xy.shape == (len(places), 2)
    assert want_rows[:, 0].sum() > 1000 and want_rows[:, 1].sum() > want_rows[:, 0].sum()
    assert all(t.is_cuda and t.is_contiguous() for t in tp.pages)
    assert len({t.untyped_storage().data_ptr() for t in tp.pages}) == 1                 # views of one allocation
    atlas = _atlas(p, bitmaps)
    again = p.glyphs.typeset_glyphs([torch.from_numpy(pg).cuda() for pg in pages], atlas, stream=torch.cuda.Stream(),
                                    **_args(pages, layers, places))
    assert not _same(again.to_host(), want) and again.rows.tobytes() == tp.rows.tobytes()
    # one colour, one radius, the default clip
    one = p.glyphs.typeset_glyphs(pages[:1], atlas, [0, 0], [0, 0, 1], [5, 6, 1], [(5, 5), (20, 12), (30, 90)], fill=(1, 2, 3),
                                  stroke=(250, 128, 0), radius=3)
    ref = GR.typeset(pages[:1], [GR.glayer(0, 3, (3, 2, 1), (0, 128, 250))] * 2, [(0, 5, 5, 5), (0, 6, 20, 12), (1, 1, 30, 90)], bitmaps)
    assert not _same(one.to_host(), ref[0]) and np.array_equal(one.rows.view(np.int32).reshape(-1, 2), ref[1])
    atlas.close()


def test_two_layers_overlapping_on_one_tile_in_both_orders():
    p = pkg()
    pages, bitmaps = TR.small_pages(), GR.small_atlas()
    layers, places = GR.overlapping()
    a = _both(p, pages, layers, places, bitmaps)[1]
    swapped = [(1 - q[0],) + q[1:] for q in places[2:] + places[:2]]
    b = _both(p, pages, layers[::-1], swapped, bitmaps)[1]
    assert (a[0] != b[0]).sum() > 100                        # the bytes differ, as for bitmap layers


# ---- 2. the caller's buffers ----------------------------------------------------------------------------------------------------

def _odd_views(pages, want):
    """The pages as views at an odd byte offset with an odd pitch inside ONE buffer of GUARD bytes: (host, expect, buf,
    views) with host the buffer holding `pages`, expect the same buffer holding `want`, buf a device copy of host and views
    the pages inside buf."""
    pitch = [(3 * pg.shape[1] + 7) | 1 for pg in pages]
    offs, at = [], 33
    for pg, pt in zip(pages, pitch):
        offs.append(at)
        at = (at + pg.shape[0] * pt + 10) | 1                             # keeps every offset odd
    assert all(o % 2 == 1 for o in offs) and all(q % 2 == 1 for q in pitch)
    host = np.full((at + 64,), GUARD, np.uint8)
    expect = host.copy()
    for pg, w, o, pt in zip(pages, want, offs, pitch):
        H, W = pg.shape[:2]
        np.lib.stride_tricks.as_strided(host[o:], (H, W, 3), (pt, 3, 1))[...] = pg
        np.lib.stride_tricks.as_strided(expect[o:], (H, W, 3), (pt, 3, 1))[...] = w
    buf = torch.from_numpy(host).cuda()
    views = [torch.as_strided(buf, (pg.shape[0], pg.shape[1], 3), (pt, 3, 1), o) for pg, o, pt in zip(pages, offs, pitch)]
    return host, expect, buf, views


def test_views_at_an_odd_offset_and_pitch_and_untouched_guards():
    """The small pages as views at an odd byte offset with an odd pitch inside one larger buffer: `inplace=False` leaves every
    byte of it as it was; `inplace=True` writes the views and nothing around or between their rows."""
    p = pkg()
    pages, bitmaps, layers, places, want, want_rows, bl = _small()
    host, expect, buf, views = _odd_views(pages, want)
    atlas = _atlas(p, bitmaps)
    kw = _args(pages, layers, places)
    tp = p.glyphs.typeset_glyphs(views, atlas, **kw)
    assert np.array_equal(buf.cpu().numpy(), host), "inplace=False wrote its inputs"
    assert not _same(tp.to_host(), want) and all(t.data_ptr() != v.data_ptr() for t, v in zip(tp.pages, views))
    tp = p.glyphs.typeset_glyphs(views, atlas, inplace=True, **kw)
    assert all(t.data_ptr() == v.data_ptr() for t, v in zip(tp.pages, views))
    got = buf.cpu().numpy()
    bad = np.flatnonzero(got != expect)
    assert not len(bad), f"{len(bad)} bytes differ, first at {bad[:5]}"
    assert np.array_equal(np.stack([tp.n_fill, tp.n_stroke], axis=1), want_rows)
    with pytest.raises(ValueError):
        p.glyphs.typeset_glyphs(pages, atlas, inplace=True, **kw)          # host pages cannot be written in place
    with pytest.raises(ValueError):
        p.glyphs.typeset_glyphs([v.permute(1, 0, 2) for v in views], atlas, inplace=True, **kw)


# ---- 3. capacity ------------------------------------------------------------------------------------------------------------

def test_a_large_glyph_over_many_tiles():
    """A 200 x 300 glyph (w x h) over a 230 x 330 page and across its edges, r = 3, with a small glyph on top in the same layer."""
    p = pkg()
    rng = np.random.default_rng(12)
    pages = [rng.integers(0, 256, (330, 230, 3), dtype=np.uint8)]
    big = np.where(rng.random((300, 200)) < 0.3, TR.noise(300, 200, 1), 0).astype(np.uint8)
    bitmaps = [big, TR.glyph(24, 24, 2)]
    layers = [GR.glayer(0, 3, (0, 0, 0), (255, 255, 255)), GR.glayer(0, 0, (255, 0, 128), (0, 255, 64))]
    places = [(0, 0, 20, 15), (0, 1, 100, 100), (1, 0, -150, 200)]
    tp, want, want_rows, bl = _both(p, pages, layers, places, bitmaps)
    assert want_rows[0, 0] > 15000 and want_rows[0, 1] > want_rows[0, 0] and want_rows[1, 1] == 0 < want_rows[1, 0]


def test_600_glyphs_on_one_tile_in_one_layer_and_in_600_layers():
    """600 placements of 2 x 2 glyphs on one 64 x 32 page: as ONE layer (more than a chunk of the kernel's staging: no cap on
    the glyphs of a layer) and as 600 layers (no cap on the groups of a tile, and their order is kept)."""
    p = pkg()
    rng = np.random.default_rng(13)
    pages = [rng.integers(0, 256, (32, 64, 3), dtype=np.uint8)]
    bitmaps = [TR.noise(2, 2, 200 + i) | 1 for i in range(8)]
    pos = [(int(rng.integers(0, 8)), int(rng.integers(-1, 64)), int(rng.integers(-1, 32))) for _ in range(600)]
    one = [GR.glayer(0, 2, (10, 20, 30), (250, 240, 230))]
    tp, want, rows, _ = _both(p, pages, one, [(0,) + q for q in pos], bitmaps)
    assert 1000 < rows[0, 0] < rows[0, 1] <= 2048
    many = [GR.glayer(0, int(rng.integers(0, 3)), tuple(int(v) for v in rng.integers(0, 256, 3)), tuple(int(v) for v in rng.integers(0, 256, 3)))
            for _ in range(600)]
    places = [(i,) + q for i, q in enumerate(pos)]
    tp, want, rows, _ = _both(p, pages, many, places, bitmaps)
    assert (rows[:, 0] > 0).all()
    back = GR.typeset(pages, many[::-1], [(599 - q[0],) + q[1:] for q in places[::-1]], bitmaps)[0]
    assert (back[0] != want[0]).sum() > 1000                 # the same layers the other way round are another page


def test_an_atlas_grown_across_two_adds_keeps_bytes_and_ids():
    p = pkg()
    first = [TR.glyph(24, 24, i) for i in range(5)]          # 2880 bytes: inside the first capacity
    second = [TR.noise(40, 50, 10 + i) for i in range(4)] + [np.zeros((0, 0), np.uint8)]     # 8000 more: past it
    atlas = p.glyphs.GlyphAtlas()
    cap = atlas._cov.numel()
    a = atlas.add(first, advance=[(25, 26)] * 5, bearing=[(1, -1)] * 5)
    before = atlas._cov.data_ptr()
    assert a.tolist() == [0, 1, 2, 3, 4] and atlas.nbytes == 2880 <= cap and len(atlas) == 5
    b = atlas.add(second)
    assert b.tolist() == [5, 6, 7, 8, 9] and atlas.nbytes == 10880 > cap and atlas._cov.numel() >= 10880 and atlas._cov.data_ptr() != before
    assert atlas._cov.numel() % cap == 0 and (atlas._cov.numel() // cap) & (atlas._cov.numel() // cap - 1) == 0    # doubled
    every = first + second
    assert np.array_equal(atlas._cov[:atlas.nbytes].cpu().numpy(), np.concatenate([g.ravel() for g in every]))
    rec = atlas._rec[:10 * 16].cpu().numpy().view(p.glyphs.RECORD_DTYPE)
    assert rec["off"].tolist() == atlas.offsets.tolist() == np.cumsum([0] + [g.size for g in every[:-1]]).tolist()
    assert np.array_equal(np.stack([rec["h"], rec["w"]], axis=1), atlas.sizes) and atlas.sizes.tolist() == [list(g.shape) for g in every]
    assert atlas.advance[:5].tolist() == [[25, 26]] * 5 and atlas.advance[5:].tolist() == [[50, 40]] * 4 + [[0, 0]]
    assert atlas.bearing[0].tolist() == [1, -1] and not atlas.bearing[5:].any()
    pages = TR.small_pages()
    layers = [GR.glayer(0, 2, (1, 2, 3), (200, 210, 220)), GR.glayer(3, 1, (255, 0, 0), (0, 0, 255))]
    places = [(0, 1, 5, 5), (0, 7, 10, 40), (0, 9, 3, 3), (1, 4, 60, 20), (1, 5, 70, 10)]
    _both(p, pages, layers, places, every, atlas=atlas)
    atlas.close()
    with pytest.raises(p._lib.CtdError):
        atlas.add(first)
    with pytest.raises(ValueError):
        p.glyphs.typeset_glyphs(pages, atlas, **_args(pages, layers, places))


# ---- 4. refusals ------------------------------------------------------------------------------------------------------------

def _raw(p, pages, layers, places, bitmaps, atlas_bytes=None, tilted=False):
    """One `ctd_typeset_glyphs` call through ctypes on dense device pages (in place).  The tile table lists EVERY tile of
    every page and, in each, EVERY placement in ascending order: the kernel has to refuse whatever does not belong there.
    The atlas allocation is the packed glyphs plus 64 spare bytes; `atlas_bytes` is what the call is told.  The rows.
    tilted: the same tables to `ctd_typeset_tilted`, every layer a `ctd_tilt_layer` with (c, s) = (65536, 0) about (9, 9)."""
    L, T, G = p._lib, p.typeset, p.glyphs
    dev = pages[0].device
    shapes = [tuple(pg.shape[:2]) for pg in pages]
    nl, n = len(layers), len(places)
    pt, lt, qt = np.zeros((len(pages),), T.PAGE_DTYPE), np.zeros((nl,), T.TILT_LAYER_DTYPE if tilted else G.LAYER_DTYPE), np.zeros((n,), G.PLACE_DTYPE)
    pt["page_dev"], pt["H"], pt["W"] = [pg.data_ptr() for pg in pages], [s[0] for s in shapes], [s[1] for s in shapes]
    pt["pitch"] = [pg.stride(0) for pg in pages]
    for i, ly in enumerate(layers):
        H, W = shapes[ly["page"]]
        lt[i]["page"], lt[i]["clip"], lt[i]["radius"] = ly["page"], ly.get("clip") or (0, 0, W, H), ly["r"]
        lt[i]["fill"], lt[i]["stroke"] = ly["fill"], ly["stroke"]
    if tilted:
        lt["ax"], lt["ay"], lt["c"], lt["s"] = 9, 9, 65536, 0
    qt["layer"], qt["glyph"], qt["x"], qt["y"] = [q[0] for q in places], [q[1] for q in places], [q[2] for q in places], [q[3] for q in places]
    rec = np.zeros((len(bitmaps),), G.RECORD_DTYPE)
    area = np.array([b.size for b in bitmaps], np.int64)
    rec["off"], rec["h"], rec["w"] = np.cumsum(area) - area, [b.shape[0] for b in bitmaps], [b.shape[1] for b in bitmaps]
    tiles = [(pg, tx, ty) for pg, (H, W) in enumerate(shapes) for ty in range((H + 31) // 32) for tx in range((W + 63) // 64)]
    tt = np.zeros((len(tiles) + 1,), T.TILE_DTYPE)
    tt["page"][:-1], tt["tx"][:-1], tt["ty"][:-1] = [t[0] for t in tiles], [t[1] for t in tiles], [t[2] for t in tiles]
    tt["first"] = np.arange(len(tiles) + 1) * n
    entries = np.tile(np.arange(n, dtype=np.int32), len(tiles))
    cov = np.concatenate([b.ravel() for b in bitmaps] + [np.full((64,), 255, np.uint8)])
    up = [torch.from_numpy(x.view(np.uint8).copy()).to(dev) for x in (pt, lt, qt, rec, tt, entries, cov)]
    rows = torch.full((nl * 8 + 64,), GUARD, dtype=torch.uint8, device=dev)
    total = int(area.sum())
    prm = L.CtdGlyphParams(nl, len(pages), len(tiles), len(entries), n, len(bitmaps), total if atlas_bytes is None else atlas_bytes)
    st = torch.cuda.current_stream(dev)
    what = "ctd_typeset_tilted" if tilted else "ctd_typeset_glyphs"
    L.check(getattr(L.lib(), what)(*[u.data_ptr() for u in up], C.byref(prm), rows.data_ptr(), st.cuda_stream), what)
    st.synchronize()
    host = rows.cpu().numpy()
    assert (host[nl * 8:] == GUARD).all(), "a byte behind the row table was written"
    return host[:nl * 8].view(np.int32).reshape(nl, 2)


def test_placements_the_kernel_must_refuse_draw_and_count_nothing():
    """A bad glyph id, a bad layer, a coordinate beyond 2^29, the layers of other pages in every tile's entries, and a record
    that ends one byte beyond atlas_bytes (the allocation is larger, so nothing can fault), inside an otherwise valid call:
    they draw nothing and count nothing, and the rest of the call is exact."""
    p = pkg()
    host = TR.small_pages(6)
    bitmaps = GR.small_atlas()[:9] + [TR.solid(9, 9)]        # the last glyph is the one that will lie beyond
    last = len(bitmaps) - 1
    layers = [GR.glayer(0, 3, (200, 10, 10), (0, 0, 0)), GR.glayer(3, 12, (5, 6, 7), (200, 201, 202)),
              GR.glayer(1, 3, (9, 8, 7), (100, 110, 120)), GR.glayer(0, 2, (10, 200, 10), (255, 255, 0))]
    good = [(0, 5, 10, 70), (0, 6, 22, 72), (1, 8, 50, 20), (1, 0, 60, 30), (2, 1, 20, 10), (3, 6, 14, 76), (3, 5, 30, 70)]
    places = (good[:2] + [(0, len(bitmaps), 12, 72), (0, -1, 12, 72), (0, 2, 2 ** 29 + 1, 70), (0, 2, 12, -2 ** 29 - 1)] + good[2:5] +
              [(2, last, 30, 12)] + good[5:] + [(4, 2, 10, 70), (-1, 2, 10, 70), (2 ** 30, 2, 10, 70)])
    want, want_rows, _ = GR.typeset(host, layers, places, bitmaps, beyond={last})
    clean = GR.typeset(host, layers, good, bitmaps)
    assert not _same(want, clean[0]) and np.array_equal(want_rows, clean[1]) and (want_rows[:, 0] > 0).all()
    pages = [torch.from_numpy(pg).cuda() for pg in host]
    total = sum(b.size for b in bitmaps)
    rows = _raw(p, pages, layers, places, bitmaps, atlas_bytes=total - 1)
    assert not _same([pg.cpu().numpy() for pg in pages], want) and np.array_equal(rows, want_rows)
    # with the last byte inside atlas_bytes that glyph is drawn
    want2, rows2, _ = GR.typeset(host, layers, places, bitmaps)
    pages = [torch.from_numpy(pg).cuda() for pg in host]
    assert np.array_equal(_raw(p, pages, layers, places, bitmaps), rows2) and not _same([pg.cpu().numpy() for pg in pages], want2)
    assert rows2[2, 0] > want_rows[2, 0] and not np.array_equal(want2[1], want[1])


def test_bad_arguments_are_refused_and_nothing_launches_for_nothing():
    p = pkg()
    L, G = p._lib, p.glyphs
    lib = L.lib()
    prm = L.CtdGlyphParams(1, 1, 1, 1, 1, 1, 16)
    for i in (0, 1, 2, 3, 4, 5, 6, 8):
        args = [8, 8, 8, 8, 8, 8, 8, C.byref(prm), 8, None]
        args[i] = None
        assert lib.ctd_typeset_glyphs(*args) != L.OK, i
    for i in range(7):
        v = [1, 1, 1, 1, 1, 1, 16]
        v[i] = -1
        assert lib.ctd_typeset_glyphs(8, 8, 8, 8, 8, 8, 8, C.byref(L.CtdGlyphParams(*v)), 8, None) != L.OK
    # zero tiles: nothing at all, the rows are not touched
    page = torch.full((8, 8, 3), 77, dtype=torch.uint8, device="cuda")
    rows = torch.full((32,), GUARD, dtype=torch.uint8, device="cuda")
    lay = torch.zeros((3 * 32,), dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream()
    assert lib.ctd_typeset_glyphs(None, lay.data_ptr(), None, None, None, None, None, C.byref(L.CtdGlyphParams(3, 0, 0, 0, 0, 0, 0)),
                                  rows.data_ptr(), st.cuda_stream) == L.OK
    st.synchronize()
    assert rows.cpu().tolist() == [GUARD] * 32
    atlas = _atlas(p, GR.small_atlas())
    none = G.typeset_glyphs([page], atlas, [], [], [], np.zeros((0, 2), np.int64))                 # zero layers
    assert len(none) == 0 and torch.equal(none.pages[0], page) and none.pages[0].data_ptr() != page.data_ptr()
    empty = G.typeset_glyphs([page], atlas, [0, 0], [], [], np.zeros((0, 2), np.int64), radius=2)  # zero placements
    assert empty.status.tolist() == [L.TYPESET_EMPTY] * 2 and not empty.n_fill.any() and torch.equal(empty.pages[0], page)
    nopage = G.typeset_glyphs([], atlas, [], [], [], np.zeros((0, 2), np.int64))                   # zero pages
    assert nopage.pages == [] and len(nopage) == 0
    off = G.typeset_glyphs([page], atlas, [0], [0, 0], [2, 3], [(50, 50), (1, 1)], radius=2, inplace=True)   # placements and no tile
    assert off.status.tolist() == [L.TYPESET_OUTSIDE] and off.rows.tolist() == [(0, 0)] and (page == 77).all()
    ok = dict(pages=[page], atlas=atlas, page_of=[0], layer_of=[0, 0], glyph=[0, 1], xy=[(1, 1), (2, 2)])
    for bad in (dict(radius=13), dict(fill=(0, 0, 300)), dict(page_of=[1]), dict(glyph=[0, 10]), dict(glyph=[-1, 0]),
                dict(layer_of=[0, 1]), dict(page_of=[0, 0], layer_of=[1, 0]), dict(xy=[(1, 1)]), dict(xy=[(0.5, 1), (2, 2)]),
                dict(clip=(0, 0, 5)), dict(atlas=None), dict(pages=[page[..., 0]]), dict(stroke=(-1, 0, 0))):
        kw = dict(ok)
        kw.update(bad)
        with pytest.raises(ValueError):
            G.typeset_glyphs(**kw)
    assert (page == 77).all()
    torch.cuda.synchronize()


# ---- 5. the chain ------------------------------------------------------------------------------------------------------------

def test_the_chain_through_the_detector():
    """detect, fill_rest, layout_boxes, `TextDetector.typeset_glyphs` on synth pages with a hand-made 16-glyph atlas: equal,
    byte for byte, to `TextDetector.typeset` given the bitmaps the restatement composes from the same `flow` positions."""
    p, det = pkg(), TG.detector()
    pages = [p.synth.text_like_page((256, 256), 3, n_blocks=4), p.synth.text_like_page((200, 300), 4, n_blocks=2)]
    results = det.detect_batch(pages)
    fp = det.fill_rest(pages, results)
    lb = det.layout_boxes(pages, results)
    assert len(lb) >= 3 and lb.ok.sum() >= 1
    bitmaps = [TR.glyph(6 + k % 3, 5 + k % 4, 30 + k) for k in range(15)] + [np.zeros((0, 0), np.uint8)]
    atlas = p.glyphs.GlyphAtlas(device=det.net.device)
    atlas.add(bitmaps, advance=[(b.shape[1] + 1, b.shape[0] + 1) for b in bitmaps[:15]] + [(4, 4)])
    rng = np.random.default_rng(14)
    runs = [rng.integers(0, 16, 6 + 3 * j) for j in range(len(lb))]
    if len(lb) > 3:
        runs[3] = None
    tp = det.typeset_glyphs(fp.pages, lb, atlas, runs, fill=(10, 20, 30), stroke=(255, 250, 245), radius=2, gap=1)
    idx = [j for j in range(len(lb)) if lb.ok[j] and runs[j] is not None]
    assert tp.layer_of.tolist() == [idx.index(j) if j in idx else -1 for j in range(len(lb))] and len(tp.fits) == len(idx) == len(tp)
    # the same flow positions, composed on the host into one bitmap a block, through the bitmap path
    host = [f.cpu().numpy() for f in fp.pages]
    block_maps, at, layers, places = [None] * len(lb), 0, [], []
    for i, j in enumerate(idx):
        rect = lb.a_rect[j] if lb.a_area[j] > 0 else lb.rect[j]
        xy, fits = p.glyphs.flow(runs[j], atlas, rect, gap=1)
        assert np.array_equal(xy, tp.xy[at:at + len(xy)]) and bool(fits) == bool(tp.fits[i])
        at += len(xy)
        layers.append(GR.glayer(int(lb.index[j, 0]), 2, (30, 20, 10), (245, 250, 255)))
        places += [(i, int(g), int(x), int(y)) for g, (x, y) in zip(runs[j], xy)]
    want, want_rows, bl = GR.typeset(host, layers, places, bitmaps)
    got = tp.to_host()
    assert not _same(got, want) and np.array_equal(tp.rows.view(np.int32).reshape(-1, 2), want_rows)
    assert (want_rows[:, 0] > 0).all() and (want_rows[:, 1] > want_rows[:, 0]).all()
    # `TextDetector.typeset` centres a bitmap in the block's rectangle: give it the composed bitmap on the rectangle grown
    # evenly by m, far enough to hold every glyph, which `place` puts at (x1 - m, y1 - m)
    for i, j in enumerate(idx):
        x1, y1, x2, y2 = (int(v) for v in (lb.a_rect[j] if lb.a_area[j] > 0 else lb.rect[j]))
        cov, x0, y0 = bl[i]["cov"], bl[i]["x0"], bl[i]["y0"]
        m = max(0, x1 - x0, y1 - y0, x0 + cov.shape[1] - x2, y0 + cov.shape[0] - y2)
        block_maps[j] = np.zeros((y2 - y1 + 2 * m, x2 - x1 + 2 * m), np.uint8)
        block_maps[j][y0 - y1 + m:y0 - y1 + m + cov.shape[0], x0 - x1 + m:x0 - x1 + m + cov.shape[1]] = cov
    direct = det.typeset(fp.pages, lb, block_maps, fill=(10, 20, 30), stroke=(255, 250, 245), radius=2)
    assert not _same(got, direct.to_host()) and direct.layer_of.tolist() == tp.layer_of.tolist()
    assert np.array_equal(direct.rows.view(np.int32).reshape(-1, 2), want_rows)
    print(f"\n{len(lb)} blocks, {len(layers)} layers, {len(places)} glyphs, n_fill {tp.n_fill.tolist()}, fits {tp.fits.tolist()}")
    assert all(torch.equal(f, torch.from_numpy(h).to(f.device)) for f, h in zip(fp.pages, host))     # inplace=False
    same = det.typeset_glyphs(fp.pages, lb, atlas, runs, fill=(10, 20, 30), stroke=(255, 250, 245), radius=2, gap=1, inplace=True)
    assert all(a.data_ptr() == b.data_ptr() for a, b in zip(same.pages, fp.pages)) and not _same(same.to_host(), got)
    with pytest.raises(ValueError):
        det.typeset_glyphs(fp.pages, lb, atlas, runs[:-1])
    with pytest.raises(ValueError):
        det.typeset_glyphs(fp.pages, lb, atlas, runs, prefer="best")
    atlas.close()
