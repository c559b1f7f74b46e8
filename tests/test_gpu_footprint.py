"""-m gpu: footprint regions -- `ctd_balloon_footprints` (csrc/kernels_footprint.hip), `balloons.balloon_regions(footprint=True)`
and `TextDetector.layout_boxes(footprint=True)` -- against the numpy restatement tests/footprint_ref.py, whose closure comes from
per-row and per-column spans on a boolean plane.  The rule is integers only and the smallest orthogonally convex superset has
one answer, so every comparison is EXACT: every field of every row and every word of every bit plane.  One call carries all
pages of a material; the pages are noise, so that the erase rule calls their blocks TEXTURED."""
import ctypes as C

import numpy as np
import pytest
import torch

import balance_ref as BAL
import balloon_ref as BR
import erase_ref as ER
import fit_ref as FIT
import footprint_ref as FR
import layout_ref as LR
import test_gpu_balloons as TB
import test_gpu_fit as TF
import test_gpu_regions as TG
from conftest import pkg

pytestmark = pytest.mark.gpu

_Blk = TB._Blk
TIGHT = dict(reach=0, reach_min=8)                                 # the window is the box grown by 8


# ---- the material ------------------------------------------------------------------------------------------------------------

def noise(H, W, seed):
    page = np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)
    return page, np.zeros((H, W), np.uint8)


def ink(page, mask, pts=(), rects=()):
    """Text pixels (x, y) and rectangles (x1, y1, x2, y2)."""
    for x, y in pts:
        mask[y, x] = 255
    for x1, y1, x2, y2 in rects:
        mask[y1:y2, x1:x2] = 255
    page[mask != 0] = 0


GEOMETRY = ((64, 63), (1, 64), (62, 65), (63, 129), (128, 64), (0, 129), (127, 65), (190, 63), (171, 129))


def word_geometry_pages():
    """One 24 x 300 noise page per window (x origin, width) for reach = 0, reach_min = 8, grow = 0: the box is as high as the
    page, so the window's first and last row are the box's.  Every block: a column whose seeds sit in rows 0 and 23, seeds at
    its box's left and right end; the 129-wide windows also seeds at bits 62, 63, 0 and 1 of a word (window columns 62 .. 65),
    and the last one -- its box ends at the page's edge -- a row with seeds in words 0 and 2 only."""
    out = []
    for k, (origin, width) in enumerate(GEOMETRY):
        page, mask = noise(24, 300, 100 + k)
        x2 = 300 if origin + width == 300 else origin + width - 8
        box = (origin + 8, 0, x2, 24)
        mid = origin + width // 2
        pts = [(mid, 0), (mid, 23), (box[0], 5 + k), (x2 - 1, 9)]
        if width == 129:
            pts += [(origin + 62, 3), (origin + 63, 14), (origin + 64, 7), (origin + 65, 20)]
        if origin + width == 300:
            pts = [(origin + 10, 12), (origin + 128, 12), (origin + 70, 2), (origin + 70, 22)]
        ink(page, mask, pts)
        out.append((page, mask, [box]))
    return out


def chain_pages():
    """The 24-link chain of tests/footprint_ref.py (13 rounds), transposed and mirrored, for TIGHT windows and grow = 0: window
    columns 40 .. 145 (60 .. 133 transposed), across the word boundaries at 64 and 128."""
    plane, _ = FR.chain()
    out = []
    for pl, x0 in ((plane, 40), (plane.T, 60), (plane[:, ::-1], 40), (plane[::-1], 40)):
        h, w = pl.shape
        page, mask = noise(h + 16, x0 + w + 20, 7)
        mask[8:8 + h, x0:x0 + w][pl] = 255
        page[mask != 0] = 0
        out.append((page, mask, [(8, 8, x0 + w + 4, 8 + h)]))
    return out


def corner_page():
    """A 90 x 150 noise page with a block in each corner and one in the middle; the text reaches all four sides of each box."""
    page, mask = noise(90, 150, 11)
    boxes = [(0, 0, 30, 14), (118, 0, 150, 12), (0, 74, 26, 90), (121, 77, 150, 90), (60, 36, 92, 52)]
    for x1, y1, x2, y2 in boxes:
        ink(page, mask, rects=[(x1, y1, x2, y1 + 3), (x1, y2 - 3, x1 + 9, y2), (x2 - 7, y1 + 6, x2, y2)])
    return page, mask, boxes


def holes_page():
    """A 100 x 240 noise page for grow = 2.  Block 0 has text in its box's top corners and along its bottom: the closure fills
    rows 28 and 29 above the box.  Block 1's text lies there (inside the closure, outside the box), block 2's text within 2
    pixels of block 0's text (inside F_0 but not T_0), and mask pixels that no box covers at (120 .. 123, 28 .. 29).  Blocks 3
    and 4 overlap and share text."""
    page, mask = noise(100, 240, 12)
    ink(page, mask, rects=[(40, 30, 60, 40), (140, 30, 160, 40), (60, 50, 140, 60),       # block 0
                           (92, 28, 108, 30), (36, 33, 40, 37), (120, 28, 124, 30),      # block 1, block 2, nobody's
                           (172, 32, 190, 38), (202, 42, 212, 52), (216, 44, 226, 50)])  # 3, shared, 4
    return page, mask, [(40, 30, 160, 60), (90, 26, 110, 30), (30, 32, 40, 38), (170, 30, 215, 60), (200, 40, 235, 70)]


def big_pages():
    """A 1024 x 512 noise page under one box (8192 words: eligible) and a 2731 x 130 one (3 x 2731 = 8193 words: not)."""
    out = []
    for (H, W), seed in (((1024, 512), 13), ((2731, 130), 14)):
        page, mask = noise(H, W, seed)
        ink(page, mask, rects=[(100, 200, 125, 210), (60, 700, 110, 712), (20, 400, 28, 460)])
        out.append((page, mask, [(0, 0, W, H)]))
    return out


def random_pages(n=20, blocks=8):
    """Seeded 110 x 190 noise pages with glyph-like blobs: per block a few short strokes inside its box."""
    out = []
    for s in range(n):
        rng = np.random.default_rng(500 + s)
        page, mask = noise(110, 190, 600 + s)
        boxes = []
        for _ in range(blocks):
            w, h = int(rng.integers(12, 70)), int(rng.integers(8, 40))
            x1, y1 = int(rng.integers(-5, 190 - w + 5)), int(rng.integers(-5, 110 - h + 5))
            boxes.append((x1, y1, x1 + w, y1 + h))
            for _ in range(int(rng.integers(1, 7))):
                sx, sy = int(rng.integers(max(x1, 0), min(x1 + w, 190))), int(rng.integers(max(y1, 0), min(y1 + h, 110)))
                lx, ly = (int(rng.integers(1, 9)), int(rng.integers(1, 3))) if rng.random() < 0.5 else (int(rng.integers(1, 3)), int(rng.integers(1, 9)))
                mask[sy:min(sy + ly, y1 + h), sx:min(sx + lx, x1 + w)] = 255
        page[mask != 0] = 0
        out.append((page, mask, boxes))
    return out


_REF = {}


def run(name, material, **kw):
    """(`balloon_regions(footprint=True)` over the material, the restatement's pages), the latter computed once per name."""
    key = (name, tuple(sorted(kw.items())))
    if key not in _REF:
        _REF[key] = [FR.footprint_page(page, mask, boxes, **kw) for page, mask, boxes in material]
    dev = torch.device("cuda:0")
    pages, masks = [torch.from_numpy(m[0]).to(dev) for m in material], [torch.from_numpy(m[1]).to(dev) for m in material]
    br = pkg().balloons.balloon_regions(pages, masks, [[_Blk(b) for b in m[2]] for m in material], footprint=True, **kw)
    return br, _REF[key]


def flat(ref, what):
    return [x for page in ref for x in page[what]]


def plane_of(br, j):
    x1, y1, x2, y2 = br.windows[j].tolist()
    return br.mask(j).cpu().numpy(), (x1, y1, x2, y2)


# ---- 1. the kernel against the restatement -----------------------------------------------------------------------------------

@pytest.mark.parametrize("pad", [0, 3])
def test_word_geometry(pad):
    material = word_geometry_pages()
    br, ref = run("geometry", material, grow=0, pad=pad, **TIGHT)
    TB._compare(br, material, ref, f"word geometry, pad {pad}")
    ws = br.windows
    assert (ws[:, 2] - ws[:, 0]).tolist() == [w for _, w in GEOMETRY] and ws[:, 0].tolist() == [o for o, _ in GEOMETRY]
    assert set((ws[:4, 0] % 64).tolist()) == {0, 1, 62, 63} and (ws[:, 1] == 0).all() and (ws[:, 3] == 24).all()
    assert br.footprint.all() and br.ok.all() and (br.erase_rows["status"] == ER.TEXTURED).all()
    if pad == 0:
        last, _ = plane_of(br, 8)
        assert last[12, 10:129].all() and not last[12, :10].any() and last[:, 70].sum() >= 21    # words 0 .. 2 of a row; a column
        for j in range(9):
            pl, _ = plane_of(br, j)
            mid = GEOMETRY[j][1] // 2
            if j < 8:
                assert pl[:, mid].all()                              # from the window's first row to its last


def test_the_chain_takes_its_rounds_whichever_way_it_runs():
    material = chain_pages()
    br, ref = run("chain", material, grow=0, pad=0, **TIGHT)
    TB._compare(br, material, ref, "chain")
    assert br.area.tolist() == [339] * 4 and br.rows["n_seed"].tolist() == [26] * 4 and br.footprint.all()
    plane, _ = FR.chain()
    closed, rounds = FR.closure(plane)
    assert rounds == 13
    got, win = plane_of(br, 0)
    assert win[0] == 0 and np.array_equal(got[8:82, 40:146], closed) and got.sum() == 339
    got, _ = plane_of(br, 1)
    assert np.array_equal(got[8:114, 60:134], closed.T)


@pytest.mark.parametrize("grow", [0, 2, 8])
@pytest.mark.parametrize("pad", [0, 1, 4, 16])
def test_pad_and_page_edges(grow, pad):
    material = [corner_page()]
    br, ref = run("corners", material, grow=grow, pad=pad)
    TB._compare(br, material, ref, f"grow {grow}, pad {pad}")
    assert br.footprint.all()
    # default windows (32 or more around the box) hold g + pad <= 24: only the page cuts
    assert (br.flags & 15 == 0).all()
    edge = [0x30, 0x60, 0x90, 0xC0, 0]
    if pad == 0:                                                   # the closure alone touches just its own corner
        assert (br.flags >> 4 & 15).tolist() == [e >> 4 for e in edge]


def test_the_window_cuts_the_region_where_grow_and_pad_exceed_reach_min():
    material = [corner_page()]
    br, ref = run("corners", material, grow=2, pad=16, **TIGHT)
    TB._compare(br, material, ref, "cut")
    L, T, R, B = BR.CUT_LEFT, BR.CUT_TOP, BR.CUT_RIGHT, BR.CUT_BOTTOM
    want = [(L | T) << 4 | R | B, (T | R) << 4 | L | B, (L | B) << 4 | T | R, (R | B) << 4 | L | T, L | T | R | B]
    assert br.flags.tolist() == [w | FR.FOOTPRINT for w in want]
    for j in range(5):                                             # the whole window: the box grown by 8 lies within 2 + 16
        pl, (x1, y1, x2, y2) = plane_of(br, j)
        other = material[0][1] != 0
        bx = material[0][2][j]
        other[bx[1]:bx[3], bx[0]:bx[2]] = False
        assert np.array_equal(pl, ~other[y1:y2, x1:x2])


def test_other_text_is_a_hole_and_overlapping_boxes_share_text():
    material = [holes_page()]
    br, ref = run("holes", material, grow=2, pad=4)
    TB._compare(br, material, ref, "holes")
    assert br.footprint.all()
    page, mask, boxes = material[0]
    full = np.zeros(mask.shape, bool)
    pl, (x1, y1, x2, y2) = plane_of(br, 0)
    full[y1:y2, x1:x2] = pl
    assert full[28:30, 60:92].all() and full[28:30, 108:120].all() and full[28:30, 124:140].all()      # the closure above the box
    assert not full[28:30, 92:108].any() and not full[28:30, 120:124].any()                            # block 1's text, nobody's
    assert not full[33:37, 36:40].any() and full[32, 36:40].all() and full[37, 36:40].all()            # block 2's text, inside F_0
    assert full[30:40, 40:60].all()                                                                    # its own text stays
    a, wa = plane_of(br, 3)
    b, wb = plane_of(br, 4)
    assert a[42 - wa[1]:52 - wa[1], 202 - wa[0]:212 - wa[0]].all() and b[42 - wb[1]:52 - wb[1], 202 - wb[0]:212 - wb[0]].all()
    # block 4's own text next to block 3's box: inside P_3 and a hole
    assert not a[44 - wa[1]:50 - wa[1], 216 - wa[0]:218 - wa[0]].any() and a[43 - wa[1], 216 - wa[0]:218 - wa[0]].all()


def _status_material():
    pages = big_pages()
    return [TB.status_page(), pages[0], pages[1]]


def test_every_status_in_one_call():
    """PLAIN, TEXTURED, NO_RING, NO_MASK, EMPTY, a TEXTURED block of 8193 words and one of exactly 8192 in one call: the PLAIN
    block is byte-identical to the call without the keyword, the ineligible ones keep the balloon call's row."""
    p = pkg()
    material = _status_material()
    br, ref = run("status", material)
    TB._compare(br, material, ref, "statuses")
    assert br.erase_rows["status"].tolist() == [ER.TEXTURED, ER.NO_RING, ER.NO_MASK, ER.EMPTY, ER.EMPTY, ER.PLAIN, ER.TEXTURED, ER.TEXTURED]
    assert br.footprint.tolist() == [True, True, False, False, False, False, True, False]
    assert br.status.tolist() == [BR.OK, BR.OK] + [BR.NOT_PLAIN] * 3 + [BR.OK, BR.OK, BR.NOT_PLAIN]
    assert br.too_large.tolist() == [False] * 7 + [True] and int(br.nw[6] * 1024) == 8192 and int(br.nw[7]) * 2731 == 8193
    dev = torch.device("cuda:0")
    off = p.balloons.balloon_regions([torch.from_numpy(m[0]).to(dev) for m in material], [torch.from_numpy(m[1]).to(dev) for m in material],
                                     [[_Blk(b) for b in m[2]] for m in material])
    assert not off.footprint.any() and off.status.tolist() == [BR.NOT_PLAIN] * 5 + [BR.OK] + [BR.NOT_PLAIN] * 2
    for j in (2, 3, 4, 5, 7):
        assert br.rows[j].tobytes() == off.rows[j].tobytes()
    a, b = br.to_host()[1], off.to_host()[1]
    w0, n = int(br.word0[5]), int(br.nw[5]) * int(br.windows[5, 3] - br.windows[5, 1])
    assert n > 0 and np.array_equal(a[w0:w0 + n], b[w0:w0 + n])
    for j in (2, 3, 4):
        w0, n = int(br.word0[j]), int(br.nw[j]) * int(br.windows[j, 3] - br.windows[j, 1])
        assert not a[w0:w0 + n].any()
    # the keyword left at its default: the bytes of the call before it existed (no second launch)
    again = p.balloons.balloon_regions([m[0] for m in material[:1]], [m[1] for m in material[:1]], [[_Blk(b) for b in material[0][2]]],
                                       footprint=False, pad=16)
    assert again.rows.tobytes() == off.rows[:6].tobytes()


def test_random_pages():
    material = random_pages()
    br, ref = run("random", material)
    want = TB._compare(br, material, ref, "random")
    n_fp = int(br.footprint.sum())
    print(f"\n{len(want)} blocks on {len(material)} pages: {n_fp} footprints, {int(br.ok.sum())} ok, "
          f"{int((br.flags & 0xF0 != 0).sum())} at a page edge")
    assert len(want) == 160 and n_fp >= 100 and (br.flags[br.footprint] & 0xF0 != 0).any()
    again, _ = run("random", material)
    assert again.rows.tobytes() == br.rows.tobytes() and torch.equal(again.bits.view(torch.int64), br.bits.view(torch.int64))


# ---- 2. the entry point with the test's own buffers ------------------------------------------------------------------------------

SENT = np.uint64(0xA5A5A5A5A5A5A5A5)


class _Tables:
    """The tables of a `ctd_balloon_footprints` call laid out by the test: rows and a guarded bit buffer pre-filled with 0xA5,
    the erase rows the restatement's, in another order."""

    def __init__(self, material, **kw):
        p = pkg()
        B, E = p.balloons, p.erase
        dev = torch.device("cuda:0")
        self.kw = dict(FR.DEFAULTS, **kw)
        self.ref = [FR.footprint_page(page, mask, boxes, **kw) for page, mask, boxes in material]
        self.off = [FR.footprint_page(page, mask, boxes, footprint=False, **kw) for page, mask, boxes in material]
        self.pages = [torch.from_numpy(m[0]).to(dev) for m in material]
        self.masks = [torch.from_numpy(m[1]).to(dev) for m in material]
        n = self.n = sum(len(m[2]) for m in material)
        self.n_pages = len(material)
        jobs, erows, pt = np.zeros((n,), B.JOB_DTYPE), np.zeros((n,), E.ROW_DTYPE), np.zeros((len(material),), E.PAGE_DTYPE)
        k, at, self.layout, self.max_words = 0, 3, [], 0
        for i, ((page, mask, boxes), (rows, words, wins, er)) in enumerate(zip(material, self.ref)):
            pt[i]["page_dev"], pt[i]["mask_dev"] = self.pages[i].data_ptr(), self.masks[i].data_ptr()
            pt[i]["H"], pt[i]["W"], pt[i]["pitch"], pt[i]["mask_pitch"] = page.shape[0], page.shape[1], self.pages[i].stride(0), self.masks[i].stride(0)
            for b, row, w, e in zip(boxes, rows, words, er):
                jobs[k]["page"], jobs[k]["xyxy"], jobs[k]["erase_row"], jobs[k]["word0"] = i, b, n - 1 - k, at
                for f in ER.FIELDS:
                    erows[n - 1 - k][f] = e[f]
                self.layout.append((at, w, bool(row["flags"] & FR.FOOTPRINT), row))
                if w is not None:
                    at += len(w) + 1 + k % 3                       # 1 .. 3 guard words behind every block
                    self.max_words = max(self.max_words, len(w))
                k += 1
        self.total = at + 2
        self.tab = torch.from_numpy(np.concatenate([jobs.view(np.uint8), pt.view(np.uint8), erows.view(np.uint8)])).to(dev)
        self.o_pages, self.o_rows = n * 32, n * 32 + len(material) * 72
        self.fill()

    def fill(self):
        dev = self.tab.device
        self.bits = torch.full((self.total * 8,), 0xA5, dtype=torch.uint8, device=dev)
        self.rows_dev = torch.full((64 + self.n * 48 + 64,), 0xA5, dtype=torch.uint8, device=dev)

    def params(self, **kw):
        v = dict(self.kw, max_words=self.max_words)
        v.update(kw)
        return pkg()._lib.CtdFootprintParams(v["grow"], v["pad"], v["reach"], v["reach_min"], v["max_words"])

    def call(self, prm, n=None, **null):
        t = self.tab.data_ptr()
        a = dict(jobs=t, pages=t + self.o_pages, erows=t + self.o_rows, rows=self.rows_dev.data_ptr() + 64, bits=self.bits.data_ptr())
        a.update(null)
        rc = pkg()._lib.lib().ctd_balloon_footprints(a["jobs"], self.n if n is None else n, a["pages"], self.n_pages, a["erows"],
                                                    C.byref(prm) if prm is not None else None, a["rows"], a["bits"], None)
        torch.cuda.synchronize()
        return rc

    def untouched(self):
        return bool((self.bits == 0xA5).all()) and bool((self.rows_dev == 0xA5).all())


def _tables():
    return _Tables([holes_page(), TB.status_page(), corner_page()], **TIGHT)


def test_nothing_but_the_eligible_blocks_rows_and_words_is_touched():
    """`ctd_balloon_footprints` ALONE through ctypes, on rows and a guarded bit buffer that hold 0xA5: every eligible row and
    word is the restatement's; every other row, every word of a block that is not eligible, every guard still holds 0xA5."""
    p = pkg()
    t = _tables()
    p._lib.check(t.call(t.params()), "ctd_balloon_footprints")
    rows = t.rows_dev.cpu().numpy()
    assert (rows[:64] == 0xA5).all() and (rows[-64:] == 0xA5).all()
    rows = rows[64:-64].view(p.balloons.ROW_DTYPE)
    bits = t.bits.cpu().numpy().view(np.uint64)
    guard = np.ones((t.total,), bool)
    seen = [0, 0]
    for k, (at, w, eligible, row) in enumerate(t.layout):
        seen[eligible] += 1
        if eligible:
            assert BR.row_dict(rows[k]) == row, k
            assert np.array_equal(bits[at:at + len(w)], w), k
            guard[at:at + len(w)] = False
        else:
            assert (rows[k:k + 1].view(np.uint8) == 0xA5).all(), k
    assert seen[0] >= 4 and seen[1] >= 10 and guard.sum() >= t.n + 5 and (bits[guard] == SENT).all()
    # a block larger than the call's max_words is not eligible: only the small ones are written
    t.fill()
    p._lib.check(t.call(t.params(max_words=40)), "ctd_balloon_footprints")
    rows = t.rows_dev.cpu().numpy()[64:-64].view(p.balloons.ROW_DTYPE)
    bits = t.bits.cpu().numpy().view(np.uint64)
    guard = np.ones((t.total,), bool)
    small = 0
    for k, (at, w, eligible, row) in enumerate(t.layout):
        if eligible and len(w) <= 40:
            assert BR.row_dict(rows[k]) == row and np.array_equal(bits[at:at + len(w)], w)
            guard[at:at + len(w)] = False
            small += 1
        else:
            assert (rows[k:k + 1].view(np.uint8) == 0xA5).all(), k
    assert small >= 1 and (bits[guard] == SENT).all()


def test_bad_arguments_are_refused_without_a_launch():
    p = pkg()
    L = p._lib
    t = _tables()
    for bad in (dict(pad=17), dict(pad=-1), dict(grow=9), dict(grow=-1), dict(reach=33), dict(reach_min=7), dict(max_words=8193),
                dict(max_words=-1)):
        assert t.call(t.params(**bad)) != L.OK, bad
    assert t.call(t.params(), n=-1) != L.OK
    assert t.call(None) != L.OK
    for null in ("jobs", "pages", "erows", "rows", "bits"):
        assert t.call(t.params(), **{null: None}) != L.OK, null
    prm = t.params()
    assert L.lib().ctd_balloon_footprints(8, 1, 8, 0, 8, C.byref(prm), 8, 8, None) != L.OK           # blocks without pages
    assert t.untouched()
    assert t.call(t.params(), n=0) == L.OK and t.untouched()                                          # n = 0: nothing launched
    assert t.call(t.params(max_words=0), bits=None) == L.OK                                           # nobody owns a word
    assert t.untouched()
    dev = torch.device("cuda:0")
    page, mask = torch.zeros((40, 60, 3), dtype=torch.uint8, device=dev), torch.zeros((40, 60), dtype=torch.uint8, device=dev)
    for bad in (dict(pad=17), dict(pad=-1), dict(pad=True), dict(footprint=1.5), dict(footprint=True, grow=9)):
        with pytest.raises(ValueError):
            p.balloons.balloon_regions([page], [mask], [[_Blk((20, 18, 40, 22))]], **bad)


# ---- 3. downstream, without a change -------------------------------------------------------------------------------------------

def test_layout_boxes_and_shaped_fit_run_on_the_combined_regions():
    """`layout.layout_boxes` and `layout.shaped_fit(balance=True)` on the rows and planes that the two launches left, against
    `layout_ref` / `fit_ref` / `balance_ref` on the restatement's planes: plain blocks and footprints in one table."""
    p = pkg()
    Y = p.layout
    page, mask, box = BR.chamber_page()
    material = [holes_page(), (page, mask, [box]), corner_page()]
    br, ref = run("downstream", material)
    TB._compare(br, material, ref, "downstream")
    rows, words, wins = flat(ref, 0), flat(ref, 1), flat(ref, 2)
    n = len(rows)
    assert br.ok.all() and 0 < br.footprint.sum() < n
    planes = [BR.unpack(w, win[3] - win[1], win[2] - win[0]) for w, win in zip(words, wins)]
    wins = [tuple(int(v) for v in w) for w in wins]
    centre = [[r["sum_x"] // r["area"], r["sum_y"] // r["area"]] for r in rows]
    for inset in (0, 2):
        lb = Y.layout_boxes(br, inset=inset)
        assert [LR.row_dict(r) for r in lb.rows] == [LR.layout_row(pl, win, c, inset=inset) for pl, win, c in zip(planes, wins, centre)]
        assert lb.ok[br.footprint].any()
    texts = [TF._text(10, (3, 5, 8, 12), 80 + j) for j in range(n)]
    cum = [np.stack(t[0]) for t in texts]
    lines = np.array(texts[0][1])
    greedy = [FIT.fit_row(pl, win, c, texts[j][0], texts[j][1], [1] * 4, inset=1) for j, (pl, win, c) in enumerate(zip(planes, wins, centre))]
    want = [BAL.rebalance(g, texts[j][0], None) for j, g in enumerate(greedy)]
    sf = Y.shaped_fit(br, cum, lines, 1, inset=1, balance=True)
    assert [(FIT.row_dict(r), BAL.bal_dict(b)) for r, b in zip(sf.rows, sf.bal_rows)] == want
    assert any(w[0]["status"] == FIT.OK for w, f in zip(want, br.footprint) if f)


def test_the_detector_typesets_a_block_on_noise_only_with_the_keyword():
    """One bar of text on a flat room and one on a noise field: `det.layout_boxes(..., footprint=True)` and `det.typeset` give
    both blocks a layer; without the keyword the second block is skipped."""
    det = TG.detector()
    page, mask = noise(90, 220, 15)
    page[10:80, 10:100] = 240
    ink(page, mask, rects=[(30, 40, 80, 48), (130, 40, 190, 48)])
    boxes = [(28, 38, 82, 50), (128, 38, 192, 50)]
    results = [(None, torch.from_numpy(mask).cuda(), [_Blk(b) for b in boxes])]
    pages = [torch.from_numpy(page).cuda()]
    bitmaps = [np.full((5, 20), 255, np.uint8), np.full((5, 20), 255, np.uint8)]
    lb = det.layout_boxes(pages, results, footprint=True)
    br = det.balloons(pages, results, footprint=True, pad=4)
    assert br.erase_rows["status"].tolist() == [ER.PLAIN, ER.TEXTURED] and br.footprint.tolist() == [False, True] and lb.ok.all()
    tp = det.typeset(pages, lb, bitmaps)
    assert (tp.layer_of >= 0).all() and tp.n_fill[tp.layer_of[1]] > 0
    x1, y1, x2, y2 = lb.rect[1].tolist()
    assert 120 <= x1 < x2 <= 200 and 30 <= y1 < y2 <= 58             # inside the old text's place grown by 2 + 4
    off = det.layout_boxes(pages, results)
    assert off.ok.tolist() == [True, False] and det.typeset(pages, off, bitmaps).layer_of.tolist() == [0, -1]
    assert off.rows[0].tobytes() == lb.rows[0].tobytes()
    with pytest.raises(ValueError):
        det.layout_boxes(pages, results, footprint=True, pad=17)
    with pytest.raises(ValueError):
        det.balloons(pages, results, footprint="yes")
