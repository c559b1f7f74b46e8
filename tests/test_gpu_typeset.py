"""-m gpu: typeset -- `ctd_typeset` (csrc/kernels_typeset.hip), `typeset.typeset_pages` and `TextDetector.typeset` -- against
the numpy restatement tests/typeset_ref.py, which works layer by layer over whole pages with one shifted copy of the coverage
per offset of the disk.  The rule is integers only, so every comparison is EXACT: every byte of every page, every field of
every row.  The layers the kernel must refuse are driven through ctypes with tables from the restatement's brute-force loop."""
import ctypes as C

import numpy as np
import pytest
import torch

import test_gpu_layout as TGL
import test_gpu_regions as TG
import typeset_ref as TR
from conftest import pkg

pytestmark = pytest.mark.gpu

GUARD = 0xA5


def _rgb(c):
    return tuple(c)[::-1]                                   # the restatement's colours are in page (BGR) order


def _api(p, pages, layers, **kw):
    """`typeset_pages` on the restatement's layers (valid ones only): per-layer colours, radius and clip."""
    shapes = [tuple(pg.shape[:2]) for pg in pages]
    clip = [ly.get("clip") or (0, 0, shapes[ly["page"]][1], shapes[ly["page"]][0]) for ly in layers]
    return p.typeset.typeset_pages(pages, [ly["page"] for ly in layers], [ly["cov"] for ly in layers],
                                   np.array([(ly["x0"], ly["y0"]) for ly in layers], np.int64).reshape(-1, 2),
                                   fill=np.array([_rgb(ly["fill"]) for ly in layers], np.int64).reshape(-1, 3),
                                   stroke=np.array([_rgb(ly["stroke"]) for ly in layers], np.int64).reshape(-1, 3),
                                   radius=np.array([ly["r"] for ly in layers], np.int64),
                                   clip=np.array(clip, np.int64).reshape(-1, 4), **kw)


def _same(got_pages, want_pages):
    return [i for i, (g, w) in enumerate(zip(got_pages, want_pages)) if g.shape != w.shape or not np.array_equal(g, w)]


def _raw(p, pages, layers, cov_bytes=None):
    """One `ctd_typeset` call through ctypes on dense device pages (in place), tables from `typeset_ref.tables_brute`, the
    layer table as the layers state it (w / h override the bitmap's shape).  Returns the rows."""
    L, T = p._lib, p.typeset
    dev = pages[0].device
    shapes = [tuple(pg.shape[:2]) for pg in pages]
    tiles, entries = TR.tables_brute(shapes, layers, L.TYPESET_TILE_W, L.TYPESET_TILE_H)
    n = len(layers)
    pt, lt = np.zeros((len(pages),), T.PAGE_DTYPE), np.zeros((n,), T.LAYER_DTYPE)
    pt["page_dev"], pt["H"], pt["W"] = [pg.data_ptr() for pg in pages], [s[0] for s in shapes], [s[1] for s in shapes]
    pt["pitch"] = [pg.stride(0) for pg in pages]
    at = 0
    for i, ly in enumerate(layers):
        h, w = ly["cov"].shape
        H, W = shapes[ly["page"]] if 0 <= ly["page"] < len(shapes) else (0, 0)
        lt[i]["cov0"], lt[i]["page"], lt[i]["x0"], lt[i]["y0"], lt[i]["cov_pitch"] = at, ly["page"], ly["x0"], ly["y0"], w
        lt[i]["w"], lt[i]["h"], lt[i]["radius"] = ly.get("w", w), ly.get("h", h), ly["r"]
        lt[i]["clip"], lt[i]["fill"], lt[i]["stroke"] = ly.get("clip") or (0, 0, W, H), ly["fill"], ly["stroke"]
        at += h * w
    cov = np.concatenate([ly["cov"].ravel() for ly in layers] + [np.full((64,), 255, np.uint8)])
    tt = np.array(tiles, np.int32).reshape(-1, 4).view(T.TILE_DTYPE).reshape(-1)
    up = [torch.from_numpy(x.view(np.uint8).copy()).to(dev) for x in (pt, lt, tt, np.array(entries, np.int32), cov)]
    rows = torch.full((n * 8 + 64,), GUARD, dtype=torch.uint8, device=dev)
    prm = L.CtdTypesetParams(n, len(pages), len(tiles) - 1, len(entries), at if cov_bytes is None else cov_bytes, 0)
    st = torch.cuda.current_stream(dev)
    L.check(L.lib().ctd_typeset(*[u.data_ptr() for u in up], C.byref(prm), rows.data_ptr(), st.cuda_stream), "ctd_typeset")
    st.synchronize()
    host = rows.cpu().numpy()
    assert (host[n * 8:] == GUARD).all(), "a byte behind the row table was written"
    return host[:n * 8].view(np.int32).reshape(n, 2)


_REF = {}


def _small():
    """The small pages, their layers and the restatement's answer, computed once."""
    if "small" not in _REF:
        pages, layers = TR.small_pages(), TR.small_layers()
        _REF["small"] = (pages, layers) + TR.typeset(pages, layers)
    return _REF["small"]


# ---- 1. the small pages ------------------------------------------------------------------------------------------------------

def test_small_pages_equal_the_restatement_in_every_byte():
    """One call over four small pages with about 40 hand-made layers; the material holds what its comments promise."""
    p = pkg()
    pages, layers, want, want_rows = _small()
    assert [pg.shape[:2] for pg in pages] == [(130, 70), (32, 64), (1, 1), (67, 129)] and 40 <= len(layers) <= 60
    assert {ly["r"] for ly in layers} == set(range(13))
    assert any(ly["cov"].shape == (1, 1) and ly["cov"][0, 0] == v for v in (255, 1) for ly in layers)
    assert {0, 255} <= {c for ly in layers for c in ly["fill"] + ly["stroke"]}
    status = [TR.status_of(ly, *TR.SHAPES[ly["page"]]) for ly in layers]
    assert status.count(TR.EMPTY) == 2 and status.count(TR.OUTSIDE) >= 4
    # the three overlapping layers: their order matters in the restatement
    ov = TR.overlapping()
    a, b = TR.typeset(pages, ov)[0], TR.typeset(pages, [ov[1], ov[0], ov[2]])[0]
    assert (a[0] != b[0]).sum() > 100
    # the seam layers' outlines reach tiles their bitmaps do not
    seam = [ly for ly in layers if ly["r"] == 12 and ly["page"] == 3 and ly["x0"] + ly["cov"].shape[1] in (63, 64)]
    assert len(seam) == 2 and all(TR.written_rect(ly, 67, 129)[2] > 64 + 10 for ly in seam)
    tp = _api(p, pages, layers)
    got = tp.to_host()
    assert not _same(got, want), f"pages {_same(got, want)} differ"
    assert np.array_equal(np.stack([tp.n_fill, tp.n_stroke], axis=1), want_rows) and tp.status.tolist() == status
    assert want_rows[:, 0].sum() > 1000 and want_rows[:, 1].sum() > want_rows[:, 0].sum()
    assert all(t.is_cuda and t.is_contiguous() for t in tp.pages) and len(tp) == len(layers)
    assert len({t.untyped_storage().data_ptr() for t in tp.pages}) == 1                 # views of one allocation
    again = _api(p, [torch.from_numpy(pg).cuda() for pg in pages], layers, stream=torch.cuda.Stream())
    assert not _same(again.to_host(), want) and again.rows.tobytes() == tp.rows.tobytes()
    # the swapped order gives the restatement's other answer
    assert not _same(_api(p, pages, [ov[1], ov[0], ov[2]]).to_host(), b)
    # one colour, one radius, the default clip
    one = p.typeset.typeset_pages(pages[:1], [0, 0], [TR.glyph(20, 30, 1), TR.noise(9, 9, 2)], [(5, 5), (30, 90)], fill=(1, 2, 3),
                                  stroke=(250, 128, 0), radius=3)
    ref = TR.typeset(pages[:1], [TR.layer(0, TR.glyph(20, 30, 1), 5, 5, 3, (3, 2, 1), (0, 128, 250)),
                                 TR.layer(0, TR.noise(9, 9, 2), 30, 90, 3, (3, 2, 1), (0, 128, 250))])
    assert not _same(one.to_host(), ref[0]) and np.array_equal(one.rows.view(np.int32).reshape(-1, 2), ref[1])


# ---- 2. the caller's buffers ----------------------------------------------------------------------------------------------------

def test_views_at_an_odd_offset_and_pitch_and_untouched_guards():
    """The same pages as views at an odd byte offset with an odd pitch inside one larger buffer: `inplace=False` leaves every
    byte of it as it was; `inplace=True` writes the views and nothing around or between their rows."""
    p = pkg()
    pages, layers, want, want_rows = _small()
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
    tp = _api(p, views, layers)
    assert np.array_equal(buf.cpu().numpy(), host), "inplace=False wrote its inputs"
    assert not _same(tp.to_host(), want) and all(t.data_ptr() != v.data_ptr() for t, v in zip(tp.pages, views))
    tp = _api(p, views, layers, inplace=True)
    assert all(t.data_ptr() == v.data_ptr() for t, v in zip(tp.pages, views))
    got = buf.cpu().numpy()
    bad = np.flatnonzero(got != expect)
    assert not len(bad), f"{len(bad)} bytes differ, first at {bad[:5]}"
    assert np.array_equal(np.stack([tp.n_fill, tp.n_stroke], axis=1), want_rows)
    with pytest.raises(ValueError):
        _api(p, pages, layers, inplace=True)                 # host pages cannot be written in place
    with pytest.raises(ValueError):
        _api(p, [v.permute(1, 0, 2) for v in views], layers, inplace=True)


# ---- 3. capacity ------------------------------------------------------------------------------------------------------------

def test_the_longest_bitmaps_at_radius_12():
    """A 16 x 8192 and an 8192 x 16 bitmap at r = 12 on pages with a side of 8192, in one call."""
    p = pkg()
    rng = np.random.default_rng(9)
    pages = [rng.integers(0, 256, (48, 8192, 3), dtype=np.uint8), rng.integers(0, 256, (8192, 48, 3), dtype=np.uint8)]
    wide = np.where(rng.random((16, 8192)) < 0.02, TR.noise(16, 8192, 1), 0).astype(np.uint8)
    layers = [TR.layer(0, wide, 0, 16, 12, (0, 0, 0), (255, 255, 255)),
              TR.layer(1, np.ascontiguousarray(wide.T), 16, 0, 12, (255, 0, 128), (0, 255, 64))]
    want, want_rows = TR.typeset(pages, layers)
    tp = _api(p, pages, layers)
    assert not _same(tp.to_host(), want) and np.array_equal(tp.rows.view(np.int32).reshape(-1, 2), want_rows)
    assert want_rows[0, 0] == want_rows[1, 0] > 1000 and want_rows[0, 1] == want_rows[1, 1] > 20 * want_rows[0, 0]


def test_a_thousand_layers_on_one_tile():
    """1000 layers of 3 x 3 on one 64 x 32 page: the layer loop has no cap, and the order is kept."""
    p = pkg()
    rng = np.random.default_rng(10)
    pages = [rng.integers(0, 256, (32, 64, 3), dtype=np.uint8)]
    layers = [TR.layer(0, TR.noise(3, 3, 100 + i), int(rng.integers(-2, 64)), int(rng.integers(-2, 32)), int(rng.integers(0, 3)),
                       tuple(int(v) for v in rng.integers(0, 256, 3)), tuple(int(v) for v in rng.integers(0, 256, 3)))
              for i in range(1000)]
    want, want_rows = TR.typeset(pages, layers)
    tp = _api(p, pages, layers)
    assert not _same(tp.to_host(), want) and np.array_equal(tp.rows.view(np.int32).reshape(-1, 2), want_rows)
    assert (want_rows[:, 0] > 0).sum() > 990
    back = TR.typeset(pages, layers[::-1])[0]
    assert (back[0] != want[0]).sum() > 1000                 # the same layers the other way round are another page


def test_layers_the_kernel_must_refuse_draw_and_count_nothing():
    """w = 8193, h = 0, r = 13, a page that is none, and a bitmap that ends one byte beyond cov_bytes, inside an otherwise valid
    call: they draw nothing and count nothing, and the rest of the call is exact."""
    p = pkg()
    host = TR.small_pages(6)
    good = TR.overlapping() + [TR.layer(3, TR.glyph(12, 40, 3), 50, 20, 12, (5, 6, 7), (200, 201, 202))]
    cov = TR.solid(9, 9)
    layers = good[:2] + [TR.layer(0, cov, 30, 70, 2, w=8193), TR.layer(0, cov, 34, 74, 13), TR.layer(0, cov, 30, 66, 2, h=0),
                         TR.layer(7, cov, 30, 66, 2), TR.layer(-1, cov, 30, 66, 2)] + good[2:] + [TR.layer(1, cov, 20, 10, 3, beyond=True)]
    want, want_rows = TR.typeset(host, layers)
    clean = TR.typeset(host, good)
    assert not _same(want, clean[0]) and np.array_equal(want[1], host[1])
    assert np.array_equal(want_rows[[0, 1, 7, 8]], clean[1]) and not want_rows[[2, 3, 4, 5, 6, 9]].any()
    pages = [torch.from_numpy(pg).cuda() for pg in host]
    total = sum(ly["cov"].size for ly in layers)
    rows = _raw(p, pages, layers, cov_bytes=total - 1)
    assert not _same([pg.cpu().numpy() for pg in pages], want) and np.array_equal(rows, want_rows)
    # with the last byte inside cov_bytes that layer is drawn
    layers[-1].pop("beyond")
    want2, rows2 = TR.typeset(host, layers)
    pages = [torch.from_numpy(pg).cuda() for pg in host]
    assert np.array_equal(_raw(p, pages, layers, cov_bytes=total), rows2) and not _same([pg.cpu().numpy() for pg in pages], want2)
    assert rows2[-1, 0] == 81 and not np.array_equal(want2[1], host[1])


# ---- 4. refusals ------------------------------------------------------------------------------------------------------------

def test_bad_arguments_are_refused_and_nothing_launches_for_nothing():
    p = pkg()
    L, T = p._lib, p.typeset
    lib = L.lib()
    prm = L.CtdTypesetParams(1, 1, 1, 1, 16, 0)
    for i in (0, 1, 2, 3, 4, 6):
        args = [8, 8, 8, 8, 8, C.byref(prm), 8, None]
        args[i] = None
        assert lib.ctd_typeset(*args) != L.OK, i
    for i in range(5):
        v = [1, 1, 1, 1, 16]
        v[i] = -1
        assert lib.ctd_typeset(8, 8, 8, 8, 8, C.byref(L.CtdTypesetParams(*v)), 8, None) != L.OK
    assert lib.ctd_typeset(8, 8, 8, 8, 8, None, 8, None) != L.OK
    # n_tiles = 0: nothing launches, the rows are still cleared; n_layers = 0: nothing at all
    page = torch.full((8, 8, 3), 77, dtype=torch.uint8, device="cuda")
    rows = torch.full((3 * 8 + 8,), GUARD, dtype=torch.uint8, device="cuda")
    lay = torch.zeros((3 * 56,), dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream()
    assert lib.ctd_typeset(None, lay.data_ptr(), None, None, None, C.byref(L.CtdTypesetParams(3, 0, 0, 0, 0, 0)), rows.data_ptr(),
                           st.cuda_stream) == L.OK
    assert lib.ctd_typeset(None, None, None, None, None, C.byref(L.CtdTypesetParams(0, 0, 0, 0, 0, 0)), None, st.cuda_stream) == L.OK
    st.synchronize()
    assert rows.cpu().tolist() == [0] * 24 + [GUARD] * 8
    none = T.typeset_pages([page], [], [], np.zeros((0, 2), np.int64))
    assert len(none) == 0 and torch.equal(none.pages[0], page) and none.pages[0].data_ptr() != page.data_ptr()
    off = T.typeset_pages([page], [0], [TR.solid(2, 2)], [(50, 50)], radius=2, inplace=True)       # a layer and no tile
    assert off.status.tolist() == [L.TYPESET_OUTSIDE] and off.rows.tolist() == [(0, 0)] and (page == 77).all()
    for bad in (dict(radius=13), dict(fill=(0, 0, 300)), dict(page_of=[1]), dict(bitmaps=[TR.solid(2, 2).astype(np.int16)])):
        kw = dict(pages=[page], page_of=[0], bitmaps=[TR.solid(2, 2)], xy=[(1, 1)])
        kw.update(bad)
        with pytest.raises(ValueError):
            T.typeset_pages(**kw)
    torch.cuda.synchronize()


# ---- 5. the chain ------------------------------------------------------------------------------------------------------------

def _check_chain(det, filled, lb, bitmaps, radius, fill, stroke):
    """`det.typeset` against the restatement applied to the same filled pages; what is skipped; where it wrote."""
    host = [f.cpu().numpy() for f in filled]
    tp = det.typeset(filled, lb, bitmaps, fill=fill, stroke=stroke, radius=radius)
    layers, layer_of = [], []
    for j in range(len(lb)):
        if not lb.ok[j] or bitmaps[j] is None:
            layer_of.append(-1)
            continue
        x1, y1, x2, y2 = (int(v) for v in (lb.a_rect[j] if lb.a_area[j] > 0 else lb.rect[j]))
        h, w = bitmaps[j].shape
        layer_of.append(len(layers))
        layers.append(TR.layer(int(lb.index[j, 0]), bitmaps[j], x1 + ((x2 - x1 - w) >> 1), y1 + ((y2 - y1 - h) >> 1), radius,
                               fill[::-1], stroke[::-1]))
    want, want_rows = TR.typeset(host, layers)
    got = tp.to_host()
    assert not _same(got, want) and np.array_equal(tp.rows.view(np.int32).reshape(-1, 2), want_rows)
    assert tp.layer_of.tolist() == layer_of and len(tp.fits) == len(layers)
    allowed = [np.zeros(h.shape[:2], bool) for h in host]
    for ly in layers:
        x1, y1, x2, y2 = TR.written_rect(ly, *host[ly["page"]].shape[:2])
        allowed[ly["page"]][y1:y2, x1:x2] = True
    for g, h, a in zip(got, host, allowed):
        assert not (g != h).any(axis=2)[~a].any()            # nothing outside the placed rectangles grown by r
    assert all(torch.equal(f, torch.from_numpy(h).to(f.device)) for f, h in zip(filled, host))     # inplace=False
    return tp, layers


def test_the_chain_on_the_chamber_pages():
    """erase, fill, balloons, layout boxes, typeset on the chamber pages of tests/balloon_ref.py."""
    p, det = pkg(), TG.detector()
    material = TGL._chambers()
    pages, masks = [m[0] for m in material], [m[1] for m in material]
    lists = [[TGL._Blk(b) for b in m[2]] for m in material]
    er = p.erase.erase_text(pages, masks, lists)
    fp = p.fill.fill_rest(er.pages, er.rest)
    lb = p.layout.layout_boxes(p.balloons.balloon_regions(pages, masks, lists, erased=er))
    assert lb.ok.all() and len(lb) == 4
    bitmaps = [TR.glyph(20, 40, 1), None, TR.glyph(60, 30, 2), TR.noise(12, 50, 3)]      # one skipped, one taller than its box
    tp, layers = _check_chain(det, fp.pages, lb, bitmaps, 3, (10, 20, 30), (255, 250, 245))
    assert tp.layer_of.tolist() == [0, -1, 1, 2] and tp.fits.tolist() == [True, False, True]
    assert (tp.n_fill > 0).all() and (tp.n_stroke > tp.n_fill).all()
    rect = det.typeset(fp.pages, lb, bitmaps, prefer="rect")
    assert rect.layer_of.tolist() == [0, -1, 1, 2] and (rect.n_stroke == 0).all()
    with pytest.raises(ValueError):
        det.typeset(fp.pages, lb, bitmaps[:3])
    with pytest.raises(ValueError):
        det.typeset(fp.pages, lb, bitmaps, prefer="best")


def test_the_chain_through_the_detector():
    """detect, fill_rest, layout_boxes, typeset on synth pages, as tests/test_gpu_layout.py does for the boxes."""
    p, det = pkg(), TG.detector()
    pages = [p.synth.text_like_page((256, 256), 3, n_blocks=4), p.synth.text_like_page((200, 300), 4, n_blocks=2)]
    results = det.detect_batch(pages)
    fp = det.fill_rest(pages, results)
    lb = det.layout_boxes(pages, results)
    assert len(lb) >= 3 and lb.ok.sum() >= 1
    bitmaps = [TR.glyph(14 + j, 30 + 3 * j, j) for j in range(len(lb))]
    tp, layers = _check_chain(det, fp.pages, lb, bitmaps, 2, (0, 0, 0), (255, 255, 255))
    print(f"\n{len(lb)} blocks, {len(layers)} layers, n_fill {tp.n_fill.tolist()}, n_stroke {tp.n_stroke.tolist()}")
    assert (tp.layer_of >= 0).sum() == lb.ok.sum() == len(layers)
    same = det.typeset(fp.pages, lb, bitmaps, radius=2, inplace=True)
    assert all(a.data_ptr() == b.data_ptr() for a, b in zip(same.pages, fp.pages)) and not _same(same.to_host(), tp.to_host())
