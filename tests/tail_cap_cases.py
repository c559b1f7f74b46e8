"""TEST INFRASTRUCTURE of tests/test_gpu_tail_caps.py and tests/test_tail_cap_cases.py: cases AT, one BELOW and one ABOVE the
capacities of the native tail's fixed tables (csrc/tail.hip):

  * `kCompCap` = 65 536 components per polarity and page and `kRowCap` = 262 144 row-table entries per page of the DB stage
    (`db_maps`: f_at / f_over, b_at / b_over, r_at / r_over, each followed in raster order by a solid bar and a bar with a hole,
    so that the LAST table slots are the ones a non-zero box comes from);
  * the `kCompCap` statistics rows `undetected_pass` (refine_undetected_mask) labels a page mask with (`undetected_cases`:
    u_at / u_over / u_far -- 4-isolated specks fill the ranking, the blobs that become windows come after them);
  * the "one 8-connected component per 2 x 2 cell" bound that sizes the tables of `refine_canvas` (`canvas_case`: dark single
    pixels at even coordinates, windows of even origin and odd size whose candidate holds exactly that many components).

Everything is deterministic and built without a GPU; the counts are asserted in tests/test_tail_cap_cases.py."""
import functools

import numpy as np

import tail_trace_cases as T
from oracle import cv_ref as cv
from oracle import postproc_ref as R

COMP_CAP, ROW_CAP = T.COMP_CAP, T.ROW_CAP

# ============================================================================================================ DB stage
DB_SHAPE = (520, 1030)              # every DB map here: maps of one shape can share a call
LOW, HIGH = 0.05, 0.9               # below / above the 0.3 of the bitmap; a shape of HIGH pixels scores 0.9 > 0.6
# the two shapes: rows 486 .. 491 (6) and 496 .. 515 (20), hole rows 502 .. 509 (8: 10 row entries with its ring)
BAR, RING, HOLE = (486, 4, 6, 106), (496, 4, 20, 106), (502, 12, 8, 90)        # (y, x, h, w)
SHAPE_ROWS = BAR[2] + RING[2] + HOLE[2] + 2


def _shapes(prob, high=HIGH, low=LOW):
    for (y, x, h, w), v in ((BAR, high), (RING, high), (HOLE, low)):
        prob[y: y + h, x: x + w] = v


def _sites(k, y0, x0, y_end, x_end):
    """(ys, xs) of the first `k` sites of the stride-2 grid from (y0, x0), in raster order."""
    per_row = len(range(x0, x_end, 2))
    assert k <= per_row * len(range(y0, y_end, 2)), (k, per_row)
    i = np.arange(k)
    return y0 + 2 * (i // per_row), x0 + 2 * (i % per_row)


def f_map(n_f):
    """`n_f` foreground components: n_f - 2 single pixels at stride 2 (8-isolated), then the bar, then the ring (the last)."""
    prob = np.full(DB_SHAPE, LOW, np.float32)
    ys, xs = _sites(n_f - 2, 0, 0, 480, DB_SHAPE[1])
    prob[ys, xs] = HIGH
    _shapes(prob)
    return prob


def b_map(n_b):
    """`n_b` background components: the page around the slab (the first), n_b - 2 single background pixels at stride 2 inside
    the slab (4-isolated, off the frame: holes of one row each, 3 row entries with their ring), the ring's hole (the last).
    Three foreground components: slab, bar, ring."""
    prob = np.full(DB_SHAPE, LOW, np.float32)
    prob[1:481, 1: DB_SHAPE[1] - 1] = HIGH
    ys, xs = _sites(n_b - 2, 2, 2, 479, DB_SHAPE[1] - 2)
    prob[ys, xs] = LOW
    _shapes(prob)
    return prob


# r maps: 1-pixel columns at stride 2 from row 0 -- 60 of 480 rows above the shapes, 452 of 516 rows, one of 76 --; with the
# shapes' 36 entries that is 60 * 480 + 452 * 516 + 76 + 36 = 262 144.  Rows 516 .. 519 stay clear: one page background.
R_COLUMNS = [480] * 60 + [516] * 452 + [76]


def r_map(extra):
    """ROW_CAP row entries from 513 columns and the two shapes (515 foreground components, 2 background); `extra`: plus that
    many single pixels under the columns (one entry each)."""
    assert sum(R_COLUMNS) + SHAPE_ROWS == ROW_CAP
    prob = np.full(DB_SHAPE, LOW, np.float32)
    for i, h in enumerate(R_COLUMNS):
        prob[:h, 2 * i] = HIGH
    _shapes(prob)
    for e in range(extra):
        prob[518, 300 + 2 * e] = HIGH
    return prob


def fitting_map(seed):
    """A speckle patch (tests/test_db_compact.py `speckle`: nested holes, islands, diagonal links) on an empty map of DB_SHAPE:
    a page that fits every table, to stand next to one that does not."""
    from test_db_compact import speckle
    prob = np.full(DB_SHAPE, LOW, np.float32)
    sp = speckle(seed)
    prob[40: 40 + sp.shape[0], 300: 300 + sp.shape[1]] = sp
    _shapes(prob)
    return prob


@functools.lru_cache(None)
def db_maps():
    """{name: prob}; *_at fills a table exactly, *_over needs one entry more."""
    return {"f_at": f_map(COMP_CAP), "f_over": f_map(COMP_CAP + 1), "b_at": b_map(COMP_CAP), "b_over": b_map(COMP_CAP + 1),
            "r_at": r_map(0), "r_over": r_map(1), "fits 2": fitting_map(2), "fits 7": fitting_map(7)}


AT, OVER = ("f_at", "b_at", "r_at"), ("f_over", "b_over", "r_over")
# name: (n_f, n_b, rows); rows of the f maps: one per pixel; of the b maps: the slab's 480 and three per hole
DB_COUNTS = {"f_at": (COMP_CAP, 2, COMP_CAP - 2 + SHAPE_ROWS), "f_over": (COMP_CAP + 1, 2, COMP_CAP - 1 + SHAPE_ROWS),
             "b_at": (3, COMP_CAP, 480 + 3 * (COMP_CAP - 2) + SHAPE_ROWS), "b_over": (3, COMP_CAP + 1, 480 + 3 * (COMP_CAP - 1) + SHAPE_ROWS),
             "r_at": (515, 2, ROW_CAP), "r_over": (516, 2, ROW_CAP + 1)}
DB_BATCHES = (("fits 2", "f_over", "r_at"), ("b_over", "fits 7"))


def overflows(name):
    nf, nb, rows = DB_COUNTS[name]
    return nf > COMP_CAP or nb > COMP_CAP or rows > ROW_CAP


@functools.lru_cache(None)
def db_oracle(name):
    """(boxes, scores) of `R.boxes_from_bitmap` on a map (shared, never modified)."""
    prob = db_maps()[name]
    return R.boxes_from_bitmap(prob, prob > 0.3, prob.shape[1], prob.shape[0])


@functools.lru_cache(None)
def db_tables(name):
    """`tail_trace_cases.db_reference` of a map that fits (shared, never modified)."""
    return T.db_reference(db_maps()[name])


def db_rows(prob):
    """Row-table entries of a map from the labellings' statistics alone: a component's height, and a hole's (a background
    component off the frame) plus two."""
    bitmap = prob > 0.3
    H, W = bitmap.shape
    st_f = R.connected_components_with_stats(bitmap.astype(np.uint8), 8)[2][1:]
    st_b = R.connected_components_with_stats((~bitmap).astype(np.uint8), 4)[2][1:]
    hole = (st_b[:, 0] > 0) & (st_b[:, 1] > 0) & (st_b[:, 0] + st_b[:, 2] < W) & (st_b[:, 1] + st_b[:, 3] < H)
    return int(st_f[:, 3].sum()) + int((st_b[:, 3] + 2)[hole].sum())


def erase_last_component(prob):
    """The map without its last foreground component (what a table one entry short loses)."""
    n, lab, _ = R.connected_components_with_stats((prob > 0.3).astype(np.uint8), 8)
    out = prob.copy()
    out[lab == n - 1] = LOW
    return out


# ======================================================================================================= undetected pass
U_SIZE = 512
BLOB = (84, 81)                     # (w, h): 6 804 pixels


def _text_blob(page, mask, x, y, sw, w=BLOB[0], h=BLOB[1]):
    """A mask blob over dark strokes on the light ground (in its left `sw` columns): its window refines to the strokes, not
    to everything."""
    mask[y: y + h, x: x + w] = 255
    for k in range(6, h - 6, 12):
        page[y + k: y + k + 5, x + 6: x + sw - 6] = 30
    for k in range(10, sw - 10, 16):
        page[y + 4: y + h - 4, x + k: x + k + 4] = 30


def undetected_page(n_specks, blobs, sw=BLOB[0]):
    """(page, mask): `n_specks` 4-isolated mask pixels (a checkerboard, raster order) fill the first ranks of the labelling;
    the blobs [(x, y)] lie below them, with strokes in their left `sw` columns.  The ground is flat: a window without strokes
    (a block over the margin) refines to nothing."""
    page = np.full((U_SIZE, U_SIZE, 3), 228, np.uint8)
    mask = np.zeros((U_SIZE, U_SIZE), np.uint8)
    i = np.arange(n_specks)
    ys, j = i // (U_SIZE // 2), i % (U_SIZE // 2)
    mask[ys, 2 * j + (ys & 1)] = 255
    assert ys.max() + 2 < min(y for _, y in blobs)
    for x, y in blobs:
        _text_blob(page, mask, x, y, sw)
    return np.ascontiguousarray(page), np.ascontiguousarray(mask)


FAR_SPECKS = 70400                  # 275 rows of 256
GROW_SPECKS = 90112                 # 352 rows of 256: the blob is component 90 113
# `undetected_pass` sizes the device table of a one-page call for COMP_CAP rows and `DevBuf::get` (csrc/tail.hip) allocates a
# quarter more plus 4 096 bytes; the relabelling of a page asks for 16 + 20 n bytes.  u_over and u_far fit what is there;
# u_grow does not: the buffer is released and allocated again.
FIRST_TABLE_BYTES = (4 + COMP_CAP * 20) + (4 + COMP_CAP * 20) // 4 + 4096


def relabel_bytes(n):
    return 16 + 20 * n


FAR_BLOBS = ((20, 290), (200, 300), (380, 310))
# u_far's blocks reach into a blob's box from the right, over its stroke-free part: exactly half of the second blob's box
# (84 x 81: 42 columns; 0.5 is not < 0.5: no window), one column less than half of the third's
FAR_BLOCKS = ([200 + 42, 294, 350, 390], [380 + 43, 304, 505, 400])


@functools.lru_cache(None)
def undetected_cases():
    """{name: case of `tail_trace_cases._case`} with keep = True: u_at (the blob is component COMP_CAP), u_over (COMP_CAP + 1),
    u_far (three blobs beyond rank 70 000, two of them under a block: one half covered, one a column less), u_grow (90 113
    components: the relabelling's table outgrows the buffer a one-page call has allocated)."""
    out = {}
    for name, n in (("u_at", COMP_CAP - 1), ("u_over", COMP_CAP)):
        page, mask = undetected_page(n, [(200, 300)])
        out[name] = T._case(name, [page], [mask], [[]], keep=True)
    page, mask = undetected_page(FAR_SPECKS, FAR_BLOBS, sw=40)
    out["u_far"] = T._case("u_far", [page], [mask], [[list(b) for b in FAR_BLOCKS]], keep=True)
    page, mask = undetected_page(GROW_SPECKS, [(200, 380)])
    out["u_grow"] = T._case("u_grow", [page], [mask], [[]], keep=True)
    return out


def text_page(seed, shape=(U_SIZE, U_SIZE)):
    """(page, mask, boxes) of a text-like page that fits: `tail_trace_cases.stroke_page` with two blocks."""
    page, mask = T.stroke_page(shape[1], shape[0], seed, 0.6)
    return page, mask, [[30, 40, 200, 150], [shape[1] - 190, shape[0] - 160, shape[1] - 20, shape[0] - 30]]


@functools.lru_cache(None)
def undetected_batches():
    """The two batches around u_over: three pages of one size (one labelling launch for the batch), three of different sizes
    (one launch per page)."""
    u = undetected_cases()["u_over"]
    out = []
    for name, shapes in (("[text, u_over, text] of one size", ((U_SIZE, U_SIZE), (U_SIZE, U_SIZE))),
                         ("[text, u_over, text] of three sizes", ((300, 411), (259, 640)))):
        a, b = text_page(31, shapes[0]), text_page(32, shapes[1])
        out.append(T._case(name, [a[0], u["pages"][0], b[0]], [a[1], u["masks"][0], b[1]], [a[2], [], b[2]], keep=True))
    return out


def single_page(case, b):
    """Page `b` of a case as a call of its own."""
    return T._case(f"{case['name']}: page {b} alone", [case["pages"][b]], [case["masks"][b]], [case["boxes"][b]], keep=case["keep"],
                   mode=case["mode"])


def undetected_truncated(img, mask_pred, mask_refined, boxes, refine_mode, cap=COMP_CAP):
    """`R.refine_undetected_mask` as a tail that keeps only the first `cap` statistics rows computes it (the wrong tail, on
    paper): components of rank > cap never become blocks.  Edits `mask_pred` in place like the original."""
    mask_pred[np.where(mask_refined > 30)] = 0
    n, labels, stats = R.connected_components_with_stats(cv.threshold_binary(mask_pred, 30, 255), 4)
    stats = stats[: cap + 1]                                  # row 0 is the background
    valid = np.where(stats[:, -1] > 50)[0]
    blks = []
    for li in valid[1:]:
        x, y, w, h, area = (int(v) for v in stats[li])
        bbox = [x, y, x + w, y + h]
        if max([R.union_area(b, bbox) for b in boxes] + [-1]) / w / h < 0.5:
            blks.append(R.TextBlock(bbox))
    if blks:
        mask_refined = np.bitwise_or(mask_refined, R.refine_mask(img, mask_pred, blks, refine_mode=refine_mode))
    return mask_refined


def blob_ranks(case):
    """[(rank, box xyxy, covered fraction of the box by the best block)] of the components of more than 50 pixels that the
    undetected pass of a one-page case sees (after pass 0 has cleared what it refined), background left out."""
    img, mask, boxes = case["pages"][0], case["masks"][0].copy(), case["boxes"][0]
    ref = R.refine_mask(img, mask, [R.TextBlock(list(b)) for b in boxes], case["mode"])
    mask[np.where(ref > 30)] = 0
    n, labels, stats = R.connected_components_with_stats(cv.threshold_binary(mask, 30, 255), 4)
    out = []
    for li in np.where(stats[:, -1] > 50)[0][1:]:
        x, y, w, h, area = (int(v) for v in stats[li])
        bbox = [x, y, x + w, y + h]
        out.append((int(li), bbox, max([R.union_area(b, bbox) for b in boxes] + [-1]) / w / h))
    return n - 1, out


# ========================================================================================================== canvas bound
CANVAS_SIZES = ((1, 1), (3, 3), (33, 31), (65, 129))
# [page][(x1, y1, w, h)]: even origins, odd sizes; two pages of different widths (no block pads to 65 x 129 in the open:
# that window stands on the left edge)
CANVAS_PAGES = (((160, 200), [(8, 6, 1, 1), (20, 10, 3, 3), (0, 40, 65, 129)]), ((101, 130), [(30, 20, 33, 31)]))
TEXT_WINDOW = (10, 70, 64, 48)      # on the second page, below the dots: strokes (`canvas_text_case`, a call of its own)


def cell_bound(w, h):
    """`refine_canvas`'s bound on the 8-connected components of a w x h window: one per 2 x 2 cell."""
    return ((w + 1) // 2) * ((h + 1) // 2)


def _canvas_pages():
    pages, masks = [], []
    for k, ((im_w, im_h), wins) in enumerate(CANVAS_PAGES):
        page = np.full((im_h, im_w, 3), 225, np.uint8)
        page[::2, ::2] = 20
        mask = np.zeros((im_h, im_w), np.uint8)
        for x1, y1, w, h in wins:
            assert x1 % 2 == 0 and y1 % 2 == 0 and w % 2 == 1 and h % 2 == 1
            mask[y1: y1 + h: 2, x1: x1 + w: 2] = 255
        if k == 1:                                            # the text-like window of `canvas_text_case`, below the dots
            x1, y1, w, h = TEXT_WINDOW
            page[y1 - 8:] = 225
            for y in range(y1 + 6, y1 + h - 8, 10):
                page[y: y + 4, x1 + 6: x1 + w - 6] = 20
            mask[y1 + 3: y1 + h - 3, x1 + 3: x1 + w - 3] = 255
        pages.append(page), masks.append(mask)
    return pages, masks


@functools.lru_cache(None)
def canvas_case():
    """Dark single pixels at even coordinates on a light ground, the mask set on exactly those pixels inside the windows: every
    candidate of every window has `cell_bound` components, and the call holds nothing but these windows -- `refine_canvas`
    sizes its tables from ONE sum over all bands of all windows of a call, so only then are the tables full."""
    pages, masks = _canvas_pages()
    boxes = [[T.block_for_window(im_w, im_h, wn) for wn in wins] for (im_w, im_h), wins in CANVAS_PAGES]
    return T._case("canvas bound: one component per 2 x 2 cell", pages, masks, boxes)


@functools.lru_cache(None)
def canvas_text_case():
    """The second page of `canvas_case` with its text-like window alone: a call of its own (its three bands have one component
    each and would leave the tables of the dot windows' call a third empty), whose result is not all zero."""
    pages, masks = _canvas_pages()
    (im_w, im_h), _ = CANVAS_PAGES[1]
    return T._case("canvas path: the text window alone", [pages[1]], [masks[1]], [[T.block_for_window(im_w, im_h, TEXT_WINDOW)]])


def candidate_components(img, mask, win):
    """8-connected components of every candidate the oracle makes for a window (colour candidates, then Otsu)."""
    x1, y1, w, h = win
    im = np.ascontiguousarray(img[y1: y1 + h, x1: x1 + w])
    msk = np.ascontiguousarray(mask[y1: y1 + h, x1: x1 + w])
    ml = R.get_topk_masklist(im, msk) + R.get_otsuthresh_masklist(im, msk)
    return [R.connected_components_with_stats(c, 8)[0] - 1 for c, _ in ml]
