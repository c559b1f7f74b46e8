"""-m gpu: tilted text -- `ctd_balloon_tilt` (csrc/kernels_tilt.hip), `ctd_typeset_tilted` (csrc/kernels_tilted.hip),
`balloons.tilt_regions`, the `angle` / `pivot` keywords of `glyphs.typeset_glyphs` and `typeset.typeset_pages`, and
`TextDetector.layout_boxes(tilt=True)` with the typeset calls behind it -- against the numpy restatement tests/tilt_ref.py.
The rule is integers only, so every comparison is EXACT: every field of every row, every word of every plane, every byte of
every page.  One call carries all blocks or layers of a material."""
import ctypes as C

import numpy as np
import pytest
import torch

import balloon_ref as BR
import glyph_ref as GR
import tilt_ref as T
import typeset_ref as TR
import test_gpu_raster as TRS
import test_gpu_regions as TG
from conftest import pkg

pytestmark = pytest.mark.gpu

ANGLES = (0, 3, -3, 15, 37, 45, 90, -90, 180)


# ---- 1. tilted planes ----------------------------------------------------------------------------------------------------------

def _source_row(plane, win, H, W, n_seed, footprint):
    """An OK balloon row over `plane` (what the balloon or the footprint call leaves)."""
    row = T.tilt_row(dict(flags=T.FOOTPRINT if footprint else 0, n_seed=n_seed), plane, win, H, W)
    row["flags"] &= ~T.TILTED
    return row


def _zero(status):
    return dict(status=status, area=0, bbox=[0] * 4, flags=0, n_seed=0, sum_x=0, sum_y=0)


def geometry_blocks():
    """Windows 63, 64, 65 and 129 wide at x origins 0, 1, 62 and 63 mod 64 on a 40 x 400 page, a seeded plane in each, every
    angle of ANGLES on each; pivots at the window's centre, at its top-left corner, and outside it.  (plane, window, pivot,
    angle, footprint)"""
    rng = np.random.default_rng(40)
    out = []
    for k, (origin, width) in enumerate(((0, 63), (1, 64), (62, 65), (63, 129), (128, 129), (271, 129))):
        win = (origin, 3, origin + width, 3 + 30 + k)
        plane = rng.random((win[3] - win[1], width)) < 0.55
        plane[:, 0] |= rng.random(plane.shape[0]) < 0.3
        for a in ANGLES:
            for pivot in (((win[0] + win[2]) >> 1, (win[1] + win[3]) >> 1), (win[0], win[1]), (win[2] + 40, -25)):
                out.append((plane, win, pivot, a, bool((k + a) & 1)))
    return out


def mixed_blocks():
    """OK, NOT_PLAIN, a 2731 x 130 window of 8193 words (TOO_LARGE: it owns no words) and a 512 x 1024 one of exactly 8192."""
    rng = np.random.default_rng(41)
    small = rng.random((20, 70)) < 0.5
    big = np.zeros((1024, 512), bool)
    big[100:900, 50:460] = rng.random((800, 410)) < 0.9
    return [(small, (5, 5, 75, 25), (40, 15), 37, False), (None, (100, 5, 170, 25), (135, 15), 15, False),
            ("too large", (0, 0, 130, 2731), (65, 1000), 20, False), (big, (0, 0, 512, 1024), (256, 512), -25, True),
            (small, (5, 5, 75, 25), (40, 15), 0, True)]


def _regions(blocks, H, W):
    """A `BalloonRegions` laid out as `balloon_regions` lays one out, its planes uploaded; and per block (row, words)."""
    p = pkg()
    B = p.balloons
    n = len(blocks)
    rows = np.zeros((n,), B.ROW_DTYPE)
    win = np.array([b[1] for b in blocks], np.int64).reshape(n, 4)
    nw = (win[:, 2] - win[:, 0] + 63) >> 6
    words = nw * (win[:, 3] - win[:, 1])
    too_large = words > BR.MAX_WORDS
    owned = np.where(too_large, 0, words)
    word0 = np.cumsum(owned) - owned
    bits = np.zeros((int(owned.sum()),), np.uint64)
    src = []
    for k, (plane, w, pivot, angle, fp) in enumerate(blocks):
        if plane is None:
            row, wd = _zero(BR.NOT_PLAIN), np.zeros((int(words[k]),), np.uint64)
        elif isinstance(plane, str):
            row, wd = _zero(BR.TOO_LARGE), None
        else:
            row, wd = _source_row(plane, w, H, W, 7 + k, fp), BR.pack(plane)
        for f in BR.FIELDS:
            rows[k][f] = row[f]
        if wd is not None:
            bits[word0[k]: word0[k] + len(wd)] = wd
        src.append((row, wd))
    dev = torch.device("cuda:0")
    br = B.BalloonRegions(np.stack([np.zeros(n, np.int64), np.arange(n)], axis=1), rows, win, nw, word0, too_large,
                          torch.from_numpy(bits.view(np.int64)).to(dev).view(torch.uint64), np.zeros((n,), p.erase.ROW_DTYPE))
    br.shapes = [(H, W)]
    return br, src


def _check(tr, br, blocks, src, H, W, max_words=BR.MAX_WORDS):
    rows, bits = tr.to_host()
    bad = []
    for k, ((plane, win, pivot, angle, fp), (row, wd)) in enumerate(zip(blocks, src)):
        want_row, want_words = T.tilt_block(row, wd, win, pivot, angle, H, W, max_words)
        got = BR.row_dict(rows[k])
        if got != want_row:
            bad.append((k, win, pivot, angle, {f: (got[f], want_row[f]) for f in BR.FIELDS if got[f] != want_row[f]}))
        if want_words is not None:
            w0 = int(br.word0[k])
            if not np.array_equal(bits[w0:w0 + len(want_words)], want_words):
                bad.append((k, win, pivot, angle, "words"))
    assert not bad, bad[:5]
    assert np.array_equal(tr.index, br.index) and np.array_equal(tr.windows, br.windows) and np.array_equal(tr.word0, br.word0)
    assert tr.bits.data_ptr() != br.bits.data_ptr() and tr.bits.numel() == br.bits.numel()


def test_tilted_planes_equal_the_restatement_in_every_field_and_word():
    p = pkg()
    blocks = geometry_blocks()
    br, src = _regions(blocks, 40, 400)
    before = br.bits.view(torch.int64).clone()
    tr = p.balloons.tilt_regions(br, [b[3] for b in blocks], pivots=[b[2] for b in blocks])
    _check(tr, br, blocks, src, 40, 400)
    assert torch.equal(br.bits.view(torch.int64), before)                # the source is read only
    assert set((br.windows[:, 0] % 64).tolist()) >= {0, 1, 62, 63} and set((br.windows[:, 2] - br.windows[:, 0]).tolist()) == {63, 64, 65, 129}
    assert tr.ok.all() and (tr.flags & T.TILTED != 0).all() and np.array_equal(tr.flags & T.FOOTPRINT, br.flags & T.FOOTPRINT)
    assert tr.angle.tolist() == [b[3] for b in blocks] and tr.pivot.tolist() == [list(b[2]) for b in blocks]
    assert [tuple(v) for v in tr.cs.tolist()] == [T.cs(b[3]) for b in blocks]
    # angle 0: the source plane and the source row, plus bit 9, wherever the pivot lies
    a, b = tr.to_host(), br.to_host()
    zero = [k for k, blk in enumerate(blocks) if blk[3] == 0]
    assert len(zero) == 18
    for k in zero:
        w0, n = int(br.word0[k]), int(br.nw[k]) * int(br.windows[k, 3] - br.windows[k, 1])
        assert np.array_equal(a[1][w0:w0 + n], b[1][w0:w0 + n])
        want = b[0][k].copy()
        want["flags"] |= T.TILTED
        assert a[0][k].tobytes() == want.tobytes()
    # quarter turns keep the area where the pivot is the centre of an odd square; a turn about a far pivot may empty the plane
    assert any(r["area"] == 0 for r in a[0]) and any(r["area"] > 0 and blk[3] == 45 for r, blk in zip(a[0], blocks))
    # the default pivot is the window's centre; the same call twice gives the same bytes
    d = p.balloons.tilt_regions(br, [b[3] for b in blocks])
    assert d.pivot.tolist() == [[(b[1][0] + b[1][2]) >> 1, (b[1][1] + b[1][3]) >> 1] for b in blocks]
    again = p.balloons.tilt_regions(br, [b[3] for b in blocks], pivots=[b[2] for b in blocks], stream=torch.cuda.Stream())
    assert again.rows.tobytes() == tr.rows.tobytes() and torch.equal(again.bits.view(torch.int64), tr.bits.view(torch.int64))


def test_every_status_and_the_largest_window_in_one_call():
    p = pkg()
    blocks = mixed_blocks()
    br, src = _regions(blocks, 2731, 512)
    assert br.too_large.tolist() == [False, False, True, False, False] and int(br.nw[3]) * 1024 == 8192 and int(br.nw[2]) * 2731 == 8193
    tr = p.balloons.tilt_regions(br, [b[3] for b in blocks], pivots=[b[2] for b in blocks])
    _check(tr, br, blocks, src, 2731, 512)
    assert tr.status.tolist() == [BR.OK, BR.NOT_PLAIN, BR.TOO_LARGE, BR.OK, BR.OK]
    assert tr.rows[1].tobytes() == br.rows[1].tobytes() and tr.rows[2].tobytes() == br.rows[2].tobytes()
    assert tr.flags.tolist()[3] & (T.TILTED | T.FOOTPRINT) == T.TILTED | T.FOOTPRINT and tr.area[3] > 100000
    w0 = int(br.word0[1])
    assert not tr.to_host()[1][w0:w0 + 40].any()
    lb = p.layout.layout_boxes(tr, inset=0)                              # downstream takes it as it stands
    assert lb.status.tolist() == [p._lib.LAYOUT_OK, p._lib.LAYOUT_NO_REGION, p._lib.LAYOUT_NO_REGION, p._lib.LAYOUT_OK, p._lib.LAYOUT_OK]


SENT = np.uint64(0xA5A5A5A5A5A5A5A5)


class _Tables:
    """The tables of a `ctd_balloon_tilt` call laid out by the test: output rows and a guarded output bit buffer pre-filled with
    0xA5, 1 .. 3 guard words behind every block."""

    def __init__(self, blocks, H, W):
        p = pkg()
        B = p.balloons
        self.blocks, self.H, self.W = blocks, H, W
        n = self.n = len(blocks)
        jobs, rows = np.zeros((n,), B.TILT_JOB_DTYPE), np.zeros((n,), B.ROW_DTYPE)
        at, self.layout, self.max_words = 3, [], 0
        src_bits = []
        for k, (plane, win, pivot, angle, fp) in enumerate(blocks):
            nw, words = BR.n_words(win)
            if plane is None:
                row, wd = _zero(BR.NOT_PLAIN), np.zeros((words,), np.uint64)
            elif isinstance(plane, str):
                row, wd = _zero(BR.TOO_LARGE), None
            else:
                row, wd = _source_row(plane, win, H, W, 7 + k, fp), BR.pack(plane)
            for f in BR.FIELDS:
                rows[k][f] = row[f]
            c, s = T.cs(angle)
            jobs[k]["win"], jobs[k]["ax"], jobs[k]["ay"], jobs[k]["c"], jobs[k]["s"] = win, pivot[0], pivot[1], c, s
            jobs[k]["W"], jobs[k]["H"], jobs[k]["word0"] = W, H, at
            self.layout.append((at, row, wd))
            if wd is not None:
                src_bits.append((at, wd))
                at += len(wd) + 1 + k % 3
                self.max_words = max(self.max_words, len(wd))
        self.total = at + 2
        src = np.full((self.total,), 0x5A5A5A5A5A5A5A5A, np.uint64)
        for a, wd in src_bits:
            src[a:a + len(wd)] = wd
        dev = torch.device("cuda:0")
        self.tab = torch.from_numpy(np.concatenate([jobs.view(np.uint8), rows.view(np.uint8)])).to(dev)
        self.src = torch.from_numpy(src.view(np.int64)).to(dev)
        self.fill()

    def fill(self):
        dev = self.tab.device
        self.bits = torch.full((self.total * 8,), 0xA5, dtype=torch.uint8, device=dev)
        self.rows_dev = torch.full((64 + self.n * 48 + 64,), 0xA5, dtype=torch.uint8, device=dev)

    def call(self, max_words=None, n=None, prm=True, **null):
        L = pkg()._lib
        t = self.tab.data_ptr()
        a = dict(jobs=t, brows=t + self.n * 48, src=self.src.data_ptr(), rows=self.rows_dev.data_ptr() + 64, bits=self.bits.data_ptr())
        a.update(null)
        prm = L.CtdTiltParams(self.max_words if max_words is None else max_words) if prm else None
        rc = L.lib().ctd_balloon_tilt(a["jobs"], self.n if n is None else n, a["brows"], a["src"], C.byref(prm) if prm is not None else None,
                                      a["rows"], a["bits"], None)
        torch.cuda.synchronize()
        return rc

    def untouched(self):
        return bool((self.bits == 0xA5).all()) and bool((self.rows_dev == 0xA5).all())


def _tables():
    blocks = [b for b in geometry_blocks()[::7]] + mixed_blocks()[:2] + [("too large", (0, 0, 130, 2731), (65, 1000), 20, False)]
    return _Tables(blocks, 2731, 400)


def test_the_entry_point_touches_nothing_but_its_rows_and_words():
    """`ctd_balloon_tilt` ALONE through ctypes on rows and a guarded bit buffer that hold 0xA5: every row and every owned word
    is the restatement's, every guard and the bytes around the rows still hold 0xA5.  With a smaller max_words the blocks
    beyond it come back TOO_LARGE and their words stay untouched."""
    p = pkg()
    t = _tables()
    for max_words in (None, 40):
        t.fill()
        p._lib.check(t.call(max_words), "ctd_balloon_tilt")
        raw = t.rows_dev.cpu().numpy()
        assert (raw[:64] == 0xA5).all() and (raw[-64:] == 0xA5).all()
        rows = raw[64:-64].view(p.balloons.ROW_DTYPE)
        bits = t.bits.cpu().numpy().view(np.uint64)
        guard = np.ones((t.total,), bool)
        kinds = set()
        for k, ((plane, win, pivot, angle, fp), (at, row, wd)) in enumerate(zip(t.blocks, t.layout)):
            want_row, want_words = T.tilt_block(row, wd, win, pivot, angle, t.H, t.W, t.max_words if max_words is None else max_words)
            assert BR.row_dict(rows[k]) == want_row, (k, win, angle)
            kinds.add(want_row["status"])
            if want_words is not None:
                assert np.array_equal(bits[at:at + len(want_words)], want_words), k
                guard[at:at + len(want_words)] = False
        assert kinds == {BR.OK, BR.NOT_PLAIN, BR.TOO_LARGE} and guard.sum() >= t.n and (bits[guard] == SENT).all()


def test_the_entry_point_refuses_bad_arguments_without_a_launch():
    L = pkg()._lib
    t = _tables()
    assert t.call(8193) != L.OK and t.call(-1) != L.OK and t.call(n=-1) != L.OK and t.call(prm=False) != L.OK
    for null in ("jobs", "brows", "src", "rows", "bits"):
        assert t.call(**{null: None}) != L.OK, null
    assert t.untouched()
    assert t.call(n=0) == L.OK and t.untouched()                          # n = 0: nothing launched


# ---- 2. the compositor ---------------------------------------------------------------------------------------------------------

def _run(pages, layers, places, atlas_maps, into=None):
    """`glyphs.typeset_glyphs` with the layers' angles and pivots, and the restatement's pages and rows.  into: device tensors
    that hold the pages, written in place."""
    p = pkg()
    G = p.glyphs
    atlas = G.GlyphAtlas()
    atlas.add(atlas_maps)
    col = lambda key: [ly[key] for ly in layers]
    clip = [ly.get("clip") or (0, 0, pages[ly["page"]].shape[1], pages[ly["page"]].shape[0]) for ly in layers]
    tp = G.typeset_glyphs(pages if into is None else into, atlas, col("page"), [q[0] for q in places], [q[1] for q in places], [(q[2], q[3]) for q in places],
                          fill=[f[::-1] for f in col("fill")], stroke=[s[::-1] for s in col("stroke")], radius=col("r"), clip=clip,
                          angle=col("angle"), pivot=col("pivot"), inplace=into is not None)
    want_pages, want_rows, written = T.typeset(pages, layers, places, atlas_maps)
    return tp, want_pages, want_rows, written


def _same(tp, want_pages, want_rows, what=""):
    for i, (a, b) in enumerate(zip(tp.to_host(), want_pages)):
        diff = np.argwhere((a != b).any(axis=2))
        assert len(diff) == 0, (what, i, len(diff), diff[:4].tolist())
    assert np.array_equal(np.stack([tp.n_fill, tp.n_stroke], axis=1), want_rows), what


def test_angle_zero_is_typeset_glyphs_to_the_byte():
    """`glyph_ref.small_case` through tilted_kernel with (65536, 0) on every drawn layer -- one more layer, tilted and empty,
    sends the call there -- against `typeset_glyphs` without the keywords and against the glyph restatement."""
    p = pkg()
    G = p.glyphs
    pages, atlas_maps = TR.small_pages(), GR.small_atlas()
    layers, places = GR.small_case()
    atlas = G.GlyphAtlas()
    atlas.add(atlas_maps)
    nl = len(layers)
    col = lambda key: [ly[key] for ly in layers]
    clip = [ly.get("clip") or (0, 0, pages[ly["page"]].shape[1], pages[ly["page"]].shape[0]) for ly in layers]
    args = ([q[0] for q in places], [q[1] for q in places], [(q[2], q[3]) for q in places])
    kw = dict(fill=[f[::-1] for f in col("fill")] + [(0, 0, 0)], stroke=[s[::-1] for s in col("stroke")] + [(0, 0, 0)],
              radius=col("r") + [3], clip=clip + [(0, 0, 70, 130)])
    up = G.typeset_glyphs(pages, atlas, col("page") + [0], *args, **kw)
    tilted = G.typeset_glyphs(pages, atlas, col("page") + [0], *args, angle=[0] * nl + [5], pivot=[(9, 9)] * (nl + 1), **kw)
    assert all(np.array_equal(a, b) for a, b in zip(up.to_host(), tilted.to_host())) and up.rows.tobytes() == tilted.rows.tobytes()
    want_pages, want_rows, _ = GR.typeset(pages, layers, places, atlas_maps)
    assert all(np.array_equal(a, b) for a, b in zip(tilted.to_host(), want_pages))
    assert np.array_equal(np.stack([tilted.n_fill, tilted.n_stroke], axis=1)[:nl], want_rows) and tilted.n_fill.sum() > 0
    assert tilted.status[nl] == p._lib.TYPESET_EMPTY
    # the restatement of this file says the same at angle 0
    tl = [dict(ly, angle=0, pivot=(3, 4)) for ly in layers]
    mine = T.typeset(pages, tl, places, atlas_maps)
    assert all(np.array_equal(a, b) for a, b in zip(mine[0], want_pages)) and np.array_equal(mine[1], want_rows)
    # all angles 0 or no keyword: the existing entry point, the same bytes
    plain = G.typeset_glyphs(pages, atlas, col("page") + [0], *args, angle=0, pivot=(5, 5), **kw)
    assert plain.rows.tobytes() == up.rows.tobytes() and all(np.array_equal(a, b) for a, b in zip(up.to_host(), plain.to_host()))


@pytest.mark.parametrize("r", [0, 12])
def test_a_glyph_across_four_tiles_at_45_degrees(r):
    """Where the frame box of a patch is largest: 45 degrees, the glyph over the corner of four tiles, r = 0 and 12; and the
    other diagonal, and 135."""
    rng = np.random.default_rng(7)
    pages = [rng.integers(0, 256, (96, 192, 3), dtype=np.uint8)]
    maps = [TR.noise(40, 60, 3), TR.glyph(30, 50, 4)]
    layers = [T.tlayer(0, 45, (64, 32), r, (200, 10, 10), (0, 0, 0)), T.tlayer(0, -45, (128, 64), r, (10, 200, 10), (255, 255, 0)),
              T.tlayer(0, 135, (100, 40), r, (1, 2, 3), (250, 251, 252))]
    places = [(0, 0, 34, 12), (1, 1, 103, 49), (2, 1, 80, 30), (2, 0, 90, 20)]
    tp, want_pages, want_rows, written = _run(pages, layers, places, maps)
    _same(tp, want_pages, want_rows, f"r {r}")
    for w in written:                                                    # each layer reaches four tiles or more
        tiles = {(y // 32, x // 64) for y, x in np.argwhere(w)[::7]}
        assert len(tiles) >= 4
    assert (tp.n_fill > 0).all() and ((tp.n_stroke > tp.n_fill).all() if r else (tp.n_stroke == 0).all())


def test_page_edges_a_clip_both_orders_and_a_mixed_call():
    """Layers hanging over each edge of the page, one cut by its clip, two overlapping layers in both orders, and an upright
    layer between tilted ones, on pages of several sizes in one call; in place as well."""
    rng = np.random.default_rng(8)
    pages = [rng.integers(0, 256, s + (3,), dtype=np.uint8) for s in ((70, 130), (1, 1), (129, 67))]
    maps = GR.small_atlas() + [TR.noise(30, 90, 9)]
    big = 10
    L_, P_ = [], []

    def add(ly, run):
        L_.append(ly)
        P_.extend((len(L_) - 1, g, x, y) for g, x, y in run)

    add(T.tlayer(0, 15, (0, 35), 3, (200, 10, 10), (0, 0, 0)), [(big, -40, 20)])                    # over the left edge
    add(T.tlayer(0, -37, (130, 35), 2, (10, 200, 10), (255, 255, 0)), [(big, 90, 20)])               # the right
    add(T.tlayer(0, 3, (65, 0), 5, (10, 10, 200), (0, 255, 255)), [(big, 20, -15)])                  # the top
    add(T.tlayer(0, -3, (65, 70), 12, (9, 9, 9), (240, 0, 240)), [(big, 20, 55)])                    # the bottom
    add(T.tlayer(0, 37, (60, 30), 6, (9, 9, 9), (240, 240, 0), clip=(25, 11, 90, 58)), [(6, 40, 20), (5, 50, 25)])   # its clip
    add(T.tlayer(2, 90, (33, 64), 4, (1, 2, 3), (250, 251, 252)), [(big, -10, 50), (0, 30, 60)])     # a quarter turn, overhanging
    add(T.tlayer(2, 0, (0, 0), 3, (200, 10, 10), (0, 0, 0)), [(5, 20, 10), (8, 30, 12)])             # upright, between tilted ones
    add(T.tlayer(2, 180, (33, 100), 1, (0, 200, 10), (20, 0, 0)), [(1, 20, 95), (2, 40, 97)])
    add(T.tlayer(1, 45, (0, 0), 2, (1, 2, 3), (250, 251, 252)), [(2, -3, -3)])                       # the 1 x 1 page
    add(T.tlayer(0, 20, (500, 500), 12), [(0, 10, 10)])                                              # OUTSIDE: turned off the page
    add(T.tlayer(0, 20, (60, 60), 3), [(3, 10, 10), (7, 12, 10)])                                    # EMPTY: zero-sized glyphs only
    add(T.tlayer(0, -20, (60, 60), 3, (5, 5, 5), (99, 99, 99)), [(3, 50, 50), (0, 55, 50), (7, 60, 50), (9, 70, 58)])  # ... in a run
    tp, want_pages, want_rows, written = _run(pages, L_, P_, maps)
    _same(tp, want_pages, want_rows, "edges")
    L = pkg()._lib
    assert tp.status.tolist() == [L.TYPESET_OK] * 9 + [L.TYPESET_OUTSIDE, L.TYPESET_EMPTY, L.TYPESET_OK]
    assert (tp.n_fill[:9] > 0).all() and tp.n_fill[9] == 0 and tp.n_fill[10] == 0 and tp.n_fill[11] > 0
    for k, col, row in ((0, 0, None), (1, 129, None), (2, None, 0), (3, None, 69)):                  # each reaches its edge
        assert written[k][:, col].any() if col is not None else written[k][row].any()
    assert written[4][11:58, 25:90].any() and written[4].sum() == written[4][11:58, 25:90].sum()
    # in place, on pages with padded rows
    dev = torch.device("cuda:0")
    wide = [torch.zeros((pg.shape[0], pg.shape[1] + 9, 3), dtype=torch.uint8, device=dev) for pg in pages]
    views = [w[:, 4:4 + pg.shape[1]] for w, pg in zip(wide, pages)]
    for v, pg in zip(views, pages):
        v.copy_(torch.from_numpy(pg))
    tq, _, _, _ = _run(pages, L_, P_, maps, into=views)
    assert all(np.array_equal(v.cpu().numpy(), b) for v, b in zip(views, want_pages)) and tq.rows.tobytes() == tp.rows.tobytes()
    assert all(not w[:, :4].any() and not w[:, 4 + pg.shape[1]:].any() for w, pg in zip(wide, pages))

    # two overlapping layers in both orders: each order is the restatement's, and the orders differ
    pg = [pages[0]]
    a = T.tlayer(0, 20, (60, 35), 3, (200, 10, 10), (0, 0, 0))
    b = T.tlayer(0, -25, (60, 35), 2, (10, 200, 10), (255, 255, 0))
    pa, pb = [(5, 40, 20), (6, 50, 30)], [(6, 45, 25), (5, 60, 22)]
    outs = []
    for first, second, p1, p2 in ((a, b, pa, pb), (b, a, pb, pa)):
        places = [(0,) + q for q in p1] + [(1,) + q for q in p2]
        tp, wp, wr, _ = _run(pg, [first, second], places, maps)
        _same(tp, wp, wr, "order")
        outs.append(tp.to_host()[0])
    assert (outs[0] != outs[1]).any()


def test_257_placements_of_one_layer_in_one_tile():
    """More placements of one layer in one tile than a chunk stages (256): the walk goes on, the frame box keeps the max."""
    rng = np.random.default_rng(9)
    pages = [rng.integers(0, 256, (64, 128, 3), dtype=np.uint8)]
    maps = [TR.solid(2, 2, 200), TR.glyph(7, 9, 5), TR.solid(1, 1, 255)]
    places = [(0, int(k % 3), 70 + int(rng.integers(0, 40)), 8 + int(rng.integers(0, 16))) for k in range(257)]
    places += [(1, 1, 75, 12)] * 2 + [(1, 0, 78 + k % 30, 14 + k % 5) for k in range(300)]
    layers = [T.tlayer(0, 15, (90, 16), 2, (200, 10, 10), (0, 0, 0)), T.tlayer(0, -15, (90, 16), 1, (0, 0, 250), (250, 250, 0))]
    tp, want_pages, want_rows, written = _run(pages, layers, places, maps)
    _same(tp, want_pages, want_rows, "257")
    ts = pkg().typeset
    _, pv, cs = ts._tilt_args([15, -15], [(90, 16)] * 2, 2)
    tiles, entries, _ = ts.tilt_tables([(64, 128)], [0, 0], [q[0] for q in places], [maps[q[1]].shape for q in places],
                                       [(q[2], q[3]) for q in places], [2, 1], None, pv, cs)
    per_tile = [entries[a:b] for a, b in zip(tiles["first"][:-1], tiles["first"][1:])]
    assert max((e < 257).sum() for e in per_tile) == 257 and max((e >= 257).sum() for e in per_tile) == 302
    assert (tp.n_fill > 0).all() and (tp.n_stroke > tp.n_fill).all()


def test_the_bitmap_path_is_the_same_rule():
    """`typeset.typeset_pages(angle=, pivot=)`: each bitmap is the one glyph of its layer; against the same restatement.  Angle
    0 everywhere is `ctd_typeset`'s call, byte for byte."""
    p = pkg()
    rng = np.random.default_rng(10)
    pages = [rng.integers(0, 256, s + (3,), dtype=np.uint8) for s in ((70, 130), (129, 67))]
    maps = [TR.glyph(20, 60, 1), TR.noise(18, 26, 2), np.zeros((0, 5), np.uint8), TR.solid(14, 22, 160), TR.glyph(24, 80, 3)]
    layers = [T.tlayer(0, 20, (60, 35), 3, (200, 10, 10), (0, 0, 0)), T.tlayer(1, -25, (30, 60), 0, (10, 200, 10), (255, 255, 0)),
              T.tlayer(0, 45, (10, 10), 2), T.tlayer(0, 0, (0, 0), 5, (10, 10, 200), (0, 255, 255)),
              T.tlayer(1, 90, (33, 64), 12, (1, 2, 3), (250, 251, 252), clip=(5, 5, 60, 120))]
    xy = [(30, 25), (20, 50), (5, 5), (80, 40), (-5, 52)]
    places = [(i, i, x, y) for i, (x, y) in enumerate(xy)]
    tp = p.typeset.typeset_pages(pages, [ly["page"] for ly in layers], maps, xy, fill=[ly["fill"][::-1] for ly in layers],
                                 stroke=[ly["stroke"][::-1] for ly in layers], radius=[ly["r"] for ly in layers],
                                 clip=[ly.get("clip") or (0, 0, pages[ly["page"]].shape[1], pages[ly["page"]].shape[0]) for ly in layers],
                                 angle=[ly["angle"] for ly in layers], pivot=[ly["pivot"] for ly in layers])
    want_pages, want_rows, _ = T.typeset(pages, layers, places, maps)
    _same(tp, want_pages, want_rows, "bitmaps")
    L = p._lib
    assert tp.status.tolist() == [L.TYPESET_OK, L.TYPESET_OK, L.TYPESET_EMPTY, L.TYPESET_OK, L.TYPESET_OK] and tp.n_fill[2] == 0
    kw = dict(fill=(9, 9, 9), stroke=(200, 200, 200), radius=2)
    a = p.typeset.typeset_pages(pages, [0, 1], maps[:2], xy[:2], **kw)
    b = p.typeset.typeset_pages(pages, [0, 1], maps[:2], xy[:2], angle=0, pivot=(7, 7), **kw)
    assert a.rows.tobytes() == b.rows.tobytes() and all(np.array_equal(x, y) for x, y in zip(a.to_host(), b.to_host()))


def test_ctd_typeset_tilted_refuses_bad_arguments_without_a_launch():
    L = pkg()._lib
    dev = torch.device("cuda:0")
    rows = torch.full((64,), 0xA5, dtype=torch.uint8, device=dev)
    tab = torch.zeros((4096,), dtype=torch.uint8, device=dev)
    t = tab.data_ptr()

    def call(prm, **null):
        a = dict(pages=t, layers=t, places=t, glyphs=t, tiles=t, entries=t, atlas=t, rows=rows.data_ptr())
        a.update(null)
        rc = L.lib().ctd_typeset_tilted(a["pages"], a["layers"], a["places"], a["glyphs"], a["tiles"], a["entries"], a["atlas"],
                                        C.byref(prm) if prm is not None else None, a["rows"], None)
        torch.cuda.synchronize()
        return rc

    good = (1, 1, 1, 1, 1, 1, 16)
    assert call(None) != L.OK
    for k in range(7):
        v = list(good)
        v[k] = -1
        assert call(L.CtdGlyphParams(*v)) != L.OK, k
    for null in ("pages", "layers", "places", "glyphs", "tiles", "entries", "atlas", "rows"):
        assert call(L.CtdGlyphParams(*good), **{null: None}) != L.OK, null
    assert call(L.CtdGlyphParams(1, 1, 0, 0, 0, 0, 0)) == L.OK and call(L.CtdGlyphParams(0, 1, 1, 0, 0, 0, 0), layers=None, rows=None) == L.OK
    assert bool((rows == 0xA5).all())                                     # no tiles or no layers: nothing at all


# ---- 3. the chain ----------------------------------------------------------------------------------------------------------------

class _Blk:
    def __init__(self, xyxy, angle):
        self.xyxy, self.angle = list(xyxy), int(angle)


CHAIN_SHAPE = (230, 480)
CHAIN = (((120, 115), (100, 55), 20), ((360, 115), (100, 30), -25))      # centre, semi-axes and turn of each balloon = its block's angle


def chain_page():
    """A grey page with two white elliptic balloons turned by +20 and -25 degrees, each with three bars of text along its long
    axis: (page, mask, blocks)."""
    H, W = CHAIN_SHAPE
    page = np.full((H, W, 3), 120, np.uint8)
    mask = np.zeros((H, W), np.uint8)
    blocks = []
    yy, xx = np.mgrid[0:H, 0:W]
    for centre, semi, turn in CHAIN:
        page[T.ellipse((H, W), centre, semi, turn)] = 255
        t = np.deg2rad(turn)
        a = (xx - centre[0]) * np.cos(t) + (yy - centre[1]) * np.sin(t)
        b = -(xx - centre[0]) * np.sin(t) + (yy - centre[1]) * np.cos(t)
        text = (np.abs(a) <= 40) & (np.abs(b) <= 9) & (np.abs(b) % 7 <= 2)
        mask[text] = 255
        ys, xs = np.nonzero(text)
        blocks.append(_Blk((xs.min(), ys.min(), xs.max() + 1, ys.max() + 1), turn))
    page[mask != 0] = 0
    return page, mask, blocks


def test_the_chain_sets_tilted_text_larger_and_inside_its_balloon():
    """`layout_boxes(tilt=True)` on two slanted balloons: a larger box than upright for both; `typeset_text(shaped=lb.frame)`
    changes no pixel outside a block's upright region (black on white: a pixel with F > 0 or S > 0 changes), and its pages are
    the restatement's on the atlas's own bitmaps; `tilt=False` is the call as it was."""
    p, det = pkg(), TG.detector()
    G = p.glyphs
    page, mask, blocks = chain_page()
    dev = det.net.device
    pages = [torch.from_numpy(page).to(dev)]
    results = [(None, torch.from_numpy(mask).to(dev), blocks)]
    br = det.balloons(pages, results)
    assert br.ok.all() and (br.flags & 15 == 0).all()
    up = det.layout_boxes(pages, results, regions=br, inset=2)
    lb = det.layout_boxes(pages, results, regions=br, inset=2, tilt=True)
    print(f"\nupright areas {up.area.tolist()}, tilted {lb.area.tolist()}; a_area {up.a_area.tolist()} -> {lb.a_area.tolist()}")
    assert lb.ok.all() and (lb.area > up.area).all() and (lb.a_area > up.a_area).all()
    assert lb.angle.tolist() == [20, -25] and np.array_equal(lb.pivot, lb.anchors) and lb.frame.angle.tolist() == [20, -25]
    assert (lb.frame.flags & T.TILTED != 0).all() and up.angle is None and up.frame is None
    # tilt=False: what the call gave before the keyword
    same = det.layout_boxes(pages, results, regions=br, inset=2, tilt=False)
    assert same.rows.tobytes() == up.rows.tobytes() and same.rows.tobytes() == p.layout.layout_boxes(br, up.anchors, inset=2).rows.tobytes()
    # angles given override the blocks'; the frame is the restatement's
    rows, bits = br.to_host()
    for j in range(2):
        w0, n = int(br.word0[j]), int(br.nw[j]) * int(br.windows[j, 3] - br.windows[j, 1])
        want_row, want_words = T.tilt_block(BR.row_dict(rows[j]), bits[w0:w0 + n], tuple(br.windows[j].tolist()), tuple(lb.pivot[j].tolist()),
                                            blocks[j].angle, *CHAIN_SHAPE)
        assert BR.row_dict(lb.frame.rows[j]) == want_row and np.array_equal(lb.frame.to_host()[1][w0:w0 + n], want_words)
    zero = det.layout_boxes(pages, results, regions=br, inset=2, tilt=True, angles=[0, 0])
    assert np.array_equal(zero.rect, up.rect) and np.array_equal(zero.a_rect, up.a_rect) and zero.angle.tolist() == [0, 0]

    font, _ = TRS._font(G)
    rng = np.random.default_rng(21)
    runs = [rng.integers(0, 19, 9), rng.integers(0, 19, 12)]
    sizes = [6, 8, 10, 12, 14, 16, 20, 24]
    kw = dict(fill=(0, 0, 0), stroke=(0, 0, 0), radius=2, gap=1)
    region = [br.mask(j).cpu().numpy() for j in range(2)]
    allowed = np.zeros(CHAIN_SHAPE, bool)
    for j in range(2):
        x1, y1, x2, y2 = br.windows[j].tolist()
        allowed[y1:y2, x1:x2] |= region[j]
    for balance in (False, True):
        atlas = G.GlyphAtlas(device=dev)
        tp = det.typeset_text(pages, lb, font, atlas, runs, sizes, shaped=lb.frame, balance=balance, **kw)
        assert tp.shaped.all() and tp.layer_of.tolist() == [0, 1] and (tp.n_fill > 0).all() and (tp.n_stroke > tp.n_fill).all()
        got = tp.to_host()[0]
        changed = (got != page).any(axis=2)
        assert changed.sum() > 200 and not (changed & ~allowed).any()
        # the restatement on the atlas's own bitmaps and the call's own placements
        cov = atlas._cov[:atlas.nbytes].cpu().numpy()
        maps = [cov[o:o + h * w].reshape(h, w) for o, (h, w) in zip(atlas.offsets.tolist(), atlas.sizes.tolist())]
        layers = [T.tlayer(0, blocks[j].angle, lb.pivot[j], 2, (0, 0, 0), (0, 0, 0)) for j in range(2)]
        places = [(int(l), int(g), int(x), int(y)) for l, g, (x, y) in zip(tp.place_layer, tp.place_glyph, tp.xy)]
        want_pages, want_rows, written = T.typeset([page], layers, places, maps)
        assert np.array_equal(got, want_pages[0]) and np.array_equal(np.stack([tp.n_fill, tp.n_stroke], axis=1), want_rows)
        for j in range(2):
            assert not (written[j] & ~allowed).any()
    upright = det.typeset_text(pages, up, font, G.GlyphAtlas(device=dev), runs, sizes, shaped=br, **kw)
    print(f"sizes upright {upright.size.tolist()}, tilted {tp.size.tolist()}")
    assert (tp.size >= upright.size).all()
    # the bitmap and the glyph calls read the frame from the boxes too
    bm = det.typeset(pages, lb, [np.full((6, 30), 255, np.uint8)] * 2, radius=1)
    want_pages, want_rows, _ = T.typeset([page], [T.tlayer(0, blocks[j].angle, lb.pivot[j], 1) for j in range(2)],
                                         [(j, 0, int(bm.xy[j][0]), int(bm.xy[j][1])) for j in range(2)], [np.full((6, 30), 255, np.uint8)])
    assert np.array_equal(bm.to_host()[0], want_pages[0]) and bm.fits.all()
    # vertical flow keeps working on the rectangle path
    vert = det.typeset_text(pages, lb, font, G.GlyphAtlas(device=dev), runs, sizes, vertical=True, **kw)
    assert (vert.n_fill > 0).all()
    # frames must agree
    for boxes, shaped in ((lb, br), (up, lb.frame)):
        with pytest.raises(ValueError):
            det.typeset_text(pages, boxes, font, G.GlyphAtlas(device=dev), runs, sizes, shaped=shaped, **kw)
    for bad in (dict(tilt=1), dict(angles=[20, -25]), dict(tilt=True, angles=[20]), dict(tilt=True, angles=[20, 181]), dict(tilt=True, angles=[2.5, 1])):
        with pytest.raises(ValueError):
            det.layout_boxes(pages, results, regions=br, **bad)
    with pytest.raises(ValueError):
        det.layout_boxes(pages, results, regions=lb.frame, tilt=True)
