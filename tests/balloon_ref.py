"""numpy restatement of the balloon rule (include/ctd_hip.h, "balloon regions"): per block that the erase rule calls PLAIN, the
4-connected region of balloon-coloured pixels around its glyphs inside a window around its box.  Written from the rule's
statement: the erase rows, F_b and med come from tests/erase_ref.py, the open plane is three comparisons, and the connected
components come from a QUEUE flood fill, pixel by pixel (`flood`) -- nothing like the kernel's row and column sweeps over
words (csrc/kernels_balloon.hip).  `scipy.ndimage.label`, where it imports, is a second method (`flood_label`) that the CPU
tests hold against the queue and that the one half-megapixel case uses.  The kernel is compared with `balloon_page` field by
field and word by word (tests/test_gpu_balloons.py); tests/test_balloon_ref.py checks the rule's own promises here."""
from collections import deque

import numpy as np

import erase_ref as ER

OK, NOT_PLAIN, TOO_LARGE = range(3)
MAX_WORDS, MAX_REACH, MIN_REACH_MIN, MAX_REACH_MIN = 8192, 32, 8, 1024
CUT_LEFT, CUT_TOP, CUT_RIGHT, CUT_BOTTOM = 1, 2, 4, 8
FIELDS = ("status", "area", "bbox", "flags", "n_seed", "sum_x", "sum_y")
DEFAULTS = dict(grow=2, tol=12, reach=8, reach_min=32)


def check_params(grow, tol, reach, reach_min):
    if not (0 <= grow <= ER.MAX_GROW and 0 <= tol <= 255 and 0 <= reach <= MAX_REACH and MIN_REACH_MIN <= reach_min <= MAX_REACH_MIN):
        raise ValueError("grow 0..8, tol 0..255, reach 0..32, reach_min 8..1024")


def window(xyxy, H, W, reach, reach_min):
    """(the clipped box or None, (wx1, wy1, wx2, wy2)): the window is empty where the clipped box is."""
    x1, y1, x2, y2 = max(int(xyxy[0]), 0), max(int(xyxy[1]), 0), min(int(xyxy[2]), W), min(int(xyxy[3]), H)
    if x1 >= x2 or y1 >= y2:
        return None, (0, 0, 0, 0)
    ex = max(reach_min, ((x2 - x1) * reach) >> 3)
    ey = max(reach_min, ((y2 - y1) * reach) >> 3)
    return (x1, y1, x2, y2), (max(x1 - ex, 0), max(y1 - ey, 0), min(x2 + ex, W), min(y2 + ey, H))


def n_words(win):
    """(nw, nw * wh) of a window."""
    nw = (win[2] - win[0] + 63) // 64
    return nw, nw * (win[3] - win[1])


def flood(open_, seed):
    """The pixels of `open_` 4-connected to a pixel of `seed` (a subset of open_) through pixels of open_: a queue, one pixel
    at a time."""
    h, w = open_.shape
    reached = np.zeros((h, w), bool)
    free = open_.copy()
    q = deque()
    for y, x in zip(*np.nonzero(seed)):
        q.append((int(y), int(x)))
        reached[y, x] = True
        free[y, x] = False
    while q:
        y, x = q.popleft()
        for yy, xx in ((y - 1, x), (y + 1, x), (y, x - 1), (y, x + 1)):
            if 0 <= yy < h and 0 <= xx < w and free[yy, xx]:
                free[yy, xx] = False
                reached[yy, xx] = True
                q.append((yy, xx))
    return reached


def flood_label(open_, seed):
    """The same set from `scipy.ndimage.label` (its default structure is the 4-neighbourhood); None where scipy is missing."""
    try:
        from scipy import ndimage
    except ImportError:
        return None
    lab, _ = ndimage.label(open_)
    hit = np.unique(lab[seed])
    return np.isin(lab, hit[hit != 0])


def pack(plane):
    """An (h, w) boolean plane as h * ceil(w / 64) u64 words, row by row, bit i of word j = column 64 j + i."""
    h, w = plane.shape
    nw = (w + 63) // 64
    padded = np.zeros((h, nw * 64), np.uint8)
    padded[:, :w] = plane
    return np.packbits(padded.reshape(h, nw, 8, 8), axis=3, bitorder="little").reshape(h * nw, 8).copy().view("<u8").reshape(-1)


def unpack(words, h, w):
    nw = (w + 63) // 64
    bits = np.unpackbits(np.asarray(words, "<u8").reshape(h, nw, 1).view(np.uint8), axis=2, bitorder="little")
    return bits.reshape(h, nw * 64)[:, :w].astype(bool)


def _zero_row(status):
    return dict(status=status, area=0, bbox=[0, 0, 0, 0], flags=0, n_seed=0, sum_x=0, sum_y=0)


def block_region(page, text, xyxy, erow, grow, tol, reach, reach_min, method=flood):
    """(row, words or None, window) of one block.  text = M as a boolean plane; erow: the block's erase row (a dict)."""
    H, W = text.shape
    box, win = window(xyxy, H, W, reach, reach_min)
    nw, words = n_words(win)
    owns = words <= MAX_WORDS
    if erow["status"] != ER.PLAIN:
        return _zero_row(NOT_PLAIN), (np.zeros((words,), np.uint64) if owns else None), win
    if not owns:
        return _zero_row(TOO_LARGE), None, win
    x1, y1, x2, y2 = box
    wx1, wy1, wx2, wy2 = win
    T = np.zeros((H, W), bool)
    T[y1:y2, x1:x2] = text[y1:y2, x1:x2]
    F = ER.dilate(T, grow)
    assert not F[:wy1].any() and not F[wy2:].any() and not F[:, :wx1].any() and not F[:, wx2:].any()    # F_b lies inside the window
    seed = F[wy1:wy2, wx1:wx2]
    px = page[wy1:wy2, wx1:wx2].astype(np.int64)
    near = (np.abs(px - np.array(erow["med"], np.int64)) <= tol).all(axis=2)
    region = method(near | seed, seed)
    ys, xs = np.nonzero(region)
    flags = 0
    for bit, hit, at_edge in ((CUT_LEFT, region[:, 0].any(), wx1 == 0), (CUT_TOP, region[0].any(), wy1 == 0),
                              (CUT_RIGHT, region[:, -1].any(), wx2 == W), (CUT_BOTTOM, region[-1].any(), wy2 == H)):
        if hit:
            flags |= bit << 4 if at_edge else bit
    row = dict(status=OK, area=int(region.sum()), bbox=[int(xs.min()) + wx1, int(ys.min()) + wy1, int(xs.max()) + wx1 + 1,
                                                       int(ys.max()) + wy1 + 1],
               flags=flags, n_seed=int(seed.sum()), sum_x=int(xs.sum()) + wx1 * len(xs), sum_y=int(ys.sum()) + wy1 * len(ys))
    return row, pack(region), win


def balloon_page(page, mask, boxes, erows=None, grow=2, tol=12, reach=8, reach_min=32, method=flood):
    """The rule on one page: (rows, words per block (None where the block owns none), windows, erase rows).  page (H,W,3) u8,
    mask (H,W) u8, boxes: the blocks' xyxy in blk_list order; erows: their erase rows, by default those of
    `erase_ref.erase_page` with the same grow and tol."""
    check_params(grow, tol, reach, reach_min)
    page, mask = np.asarray(page), np.asarray(mask)
    if erows is None:
        erows = ER.erase_page(page, mask, boxes, grow=grow, tol=tol)[0]
    text = mask != 0
    out = [block_region(page, text, b, e, grow, tol, reach, reach_min, method) for b, e in zip(boxes, erows)]
    return [o[0] for o in out], [o[1] for o in out], [o[2] for o in out], erows


def row_dict(row):
    """A record of the kernel's result table as the dict `block_region` returns."""
    return {k: (row[k].tolist() if np.ndim(row[k]) else int(row[k])) for k in FIELDS}


# ---- pages with known answers (tests/test_balloon_ref.py; the GPU test runs the same through the kernel) ---------------------

WHITE, INK, LINE = 255, 0, 60


def chamber_page(shape=(60, 100), room=(20, 10, 80, 50), text=(40, 26, 60, 32), gap=None, bg=200):
    """A grey page with a white room whose 1-pixel outline (value LINE) runs along the inside of `room`'s border, and a bar
    of text in it.  gap: (x, y) of one outline pixel that is left white.  (page, mask, box of the text)."""
    H, W = shape
    page = np.full((H, W, 3), bg, np.uint8)
    x1, y1, x2, y2 = room
    page[y1:y2, x1:x2] = WHITE
    page[y1, x1:x2] = page[y2 - 1, x1:x2] = LINE
    page[y1:y2, x1] = page[y1:y2, x2 - 1] = LINE
    if gap is not None:
        page[gap[1], gap[0]] = WHITE
    mask = np.zeros((H, W), np.uint8)
    tx1, ty1, tx2, ty2 = text
    mask[ty1:ty2, tx1:tx2] = 255
    page[mask != 0] = INK
    return page, mask, text
