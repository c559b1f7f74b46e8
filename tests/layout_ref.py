"""numpy restatement of the layout rule (include/ctd_hip.h, "layout boxes"): per block with a balloon region, the region eroded
by `inset` and clipped at the window, the best rectangle inside it and the best one that contains the block's anchor, by the
order "larger area, then smaller y1, then smaller x1, then smaller y2".  Written from the rule's statement: `best_rect` walks
the plane row by row as a histogram of column heights and takes the rectangles a stack pops (every maximal rectangle is one of
them) -- nothing like the kernel's rows ANDed k deep (csrc/kernels_layout.hip); `best_rect_brute` looks at EVERY rectangle
through a summed-area table, a second method for small planes that tests/test_layout_ref.py holds against the first.  The
kernel is compared with `layout_row` field by field (tests/test_gpu_layout.py)."""
import numpy as np

import balloon_ref as BR
from balloon_ref import pack, unpack  # noqa: F401  (the bit planes' layout is the balloon rule's)

OK, NO_REGION, EMPTY = range(3)
MAX_INSET = 16
FIELDS = ("status", "n_inner", "area", "rect", "a_area", "a_rect")


def check_params(inset):
    if not 0 <= inset <= MAX_INSET:
        raise ValueError("inset 0..16")


def erode(plane, m):
    """The pixels whose (2m + 1)-square lies inside the plane and is all set.  The square is an interval of columns times an
    interval of rows, so the rows are done first and the columns of that after."""
    plane = np.asarray(plane, bool)
    h, w = plane.shape
    out = np.zeros((h, w), bool)
    if h <= 2 * m or w <= 2 * m:
        return out
    rows = np.ones((h, w - 2 * m), bool)
    for d in range(2 * m + 1):
        rows &= plane[:, d:d + w - 2 * m]
    cols = np.ones((h - 2 * m, w - 2 * m), bool)
    for d in range(2 * m + 1):
        cols &= rows[d:d + h - 2 * m]
    out[m:h - m, m:w - m] = cols
    return out


def _key(area, x1, y1, x2, y2):
    return (-area, y1, x1, y2)


def best_rect(plane, anchor=None):
    """(area, [x1, y1, x2, y2]) of the best rectangle of the plane, x2 and y2 exclusive, or (0, [0, 0, 0, 0]); with `anchor` =
    (x, y) the best among those that contain that pixel.  Row r is the bottom row of the candidates: heights[x] counts the set
    pixels from (x, r) upwards, and the stack pops, for every column, the widest rectangle of that column's height."""
    plane = np.asarray(plane, bool)
    h, w = plane.shape
    best = None
    heights = np.zeros((w + 1,), np.int64)                  # the last entry stays 0: it empties the stack
    for r in range(h):
        heights[:w] = np.where(plane[r], heights[:w] + 1, 0)
        if not heights.any():
            continue
        hs = heights.tolist()
        stack = []
        for x in range(w + 1):
            cur = hs[x]
            while stack and hs[stack[-1]] >= cur:
                top = hs[stack.pop()]
                if top == 0:
                    continue
                x1 = stack[-1] + 1 if stack else 0
                y1 = r - top + 1
                if anchor is not None and not (x1 <= anchor[0] < x and y1 <= anchor[1] <= r):
                    continue
                key = _key(top * (x - x1), x1, y1, x, r + 1)
                if best is None or key < best[0]:
                    best = (key, [x1, y1, x, r + 1])
            stack.append(x)
    return (0, [0, 0, 0, 0]) if best is None else (-best[0][0], best[1])


_GRIDS = {}


def best_rect_brute(plane, anchor=None):
    """The same answer from EVERY rectangle of the plane: one is inside when its sum in the summed-area table is its area.
    For planes up to about 12 x 12."""
    plane = np.asarray(plane, bool)
    h, w = plane.shape
    if (h, w) not in _GRIDS:
        y1, y2, x1, x2 = np.meshgrid(np.arange(h), np.arange(1, h + 1), np.arange(w), np.arange(1, w + 1), indexing="ij")
        some = (y1 < y2) & (x1 < x2)
        _GRIDS[(h, w)] = tuple(a[some] for a in (y1, y2, x1, x2))
    y1, y2, x1, x2 = _GRIDS[(h, w)]
    S = np.zeros((h + 1, w + 1), np.int64)
    S[1:, 1:] = plane.cumsum(axis=0).cumsum(axis=1)
    area = (y2 - y1) * (x2 - x1)
    inside = S[y2, x2] - S[y1, x2] - S[y2, x1] + S[y1, x1] == area
    if anchor is not None:
        inside &= (x1 <= anchor[0]) & (anchor[0] < x2) & (y1 <= anchor[1]) & (anchor[1] < y2)
    if not inside.any():
        return 0, [0, 0, 0, 0]
    y1, y2, x1, x2, area = y1[inside], y2[inside], x1[inside], x2[inside], area[inside]
    k = np.lexsort((y2, x1, y1, -area))[0]                  # the last key is the first to decide
    return int(area[k]), [int(x1[k]), int(y1[k]), int(x2[k]), int(y2[k])]


def _zero_row(status):
    return dict(status=status, n_inner=0, area=0, rect=[0, 0, 0, 0], a_area=0, a_rect=[0, 0, 0, 0])


def layout_row(region, win, anchor, inset=2, balloon_status=BR.OK, max_words=BR.MAX_WORDS, method=best_rect):
    """The row of one block.  region: B_b as a boolean (wh, ww) plane over the window `win` = (wx1, wy1, wx2, wy2) (ignored
    where `balloon_status` is not OK); anchor: (x, y) in page coordinates."""
    check_params(inset)
    if balloon_status != BR.OK or BR.n_words(win)[1] > max_words:
        return _zero_row(NO_REGION)
    wx1, wy1, wx2, wy2 = win
    inner = erode(np.asarray(region, bool).reshape(max(wy2 - wy1, 0), max(wx2 - wx1, 0)), inset)
    if not inner.any():
        return _zero_row(EMPTY)

    def page(rect):
        return [rect[0] + wx1, rect[1] + wy1, rect[2] + wx1, rect[3] + wy1]

    area, rect = method(inner)
    a = (int(anchor[0]) - wx1, int(anchor[1]) - wy1)
    a_area, a_rect = 0, None
    if 0 <= a[0] < wx2 - wx1 and 0 <= a[1] < wy2 - wy1 and inner[a[1], a[0]]:
        a_area, a_rect = method(inner, a)
    return dict(status=OK, n_inner=int(inner.sum()), area=area, rect=page(rect), a_area=a_area,
                a_rect=page(a_rect) if a_area else [0, 0, 0, 0])


def row_dict(row):
    """A record of the kernel's result table as the dict `layout_row` returns."""
    return {k: (row[k].tolist() if np.ndim(row[k]) else int(row[k])) for k in FIELDS}


# ---- small planes with answers written out by hand (tests/test_layout_ref.py) ------------------------------------------------

def _plane(rows):
    return np.array([[c == "#" for c in r] for r in rows], bool)


# name: (plane, anchor (x, y) or None, (area, rect), (a_area, a_rect) or None)
NAMED = {
    # two 2 x 2 squares, the right one higher up: the smaller y1 wins although its x1 is larger
    "tie_on_y1": (_plane(["....##.",
                          "....##.",
                          "##.....",
                          "##....."]), None, (4, [4, 0, 6, 2]), None),
    # two 2 x 2 squares on the same rows: the smaller x1 wins
    "tie_on_x1": (_plane([".##.##",
                          ".##.##"]), None, (4, [1, 0, 3, 2]), None),
    # an L with arms of 4 pixels from one corner: same y1, same x1, the flat arm has the smaller y2
    "tie_on_y2": (_plane(["####",
                          "#...",
                          "#...",
                          "#..."]), None, (4, [0, 0, 4, 1]), None),
    # a room and a corridor: the anchor in the corridor gets the corridor's row through the room, not the room
    "anchored_differs": (_plane(["....####",
                                 "....####",
                                 "########",
                                 "....####"]), (1, 2), (16, [4, 0, 8, 4]), (8, [0, 2, 8, 3])),
    # the anchor on a pixel that is not set
    "anchor_outside": (_plane(["###.",
                               "###.",
                               "...."]), (3, 2), (6, [0, 0, 3, 2]), (0, [0, 0, 0, 0])),
    "single_pixel": (_plane(["...",
                             ".#.",
                             "..."]), (1, 1), (1, [1, 1, 2, 2]), (1, [1, 1, 2, 2])),
    "empty": (_plane(["...", "..."]), (1, 1), (0, [0, 0, 0, 0]), (0, [0, 0, 0, 0])),
    # a plus with arms of equal area: the upright arm starts higher
    "plus": (_plane(["..#..",
                     "..#..",
                     "#####",
                     "..#..",
                     "..#.."]), (0, 2), (5, [2, 0, 3, 5]), (5, [0, 2, 5, 3])),
}


# ---- planes for the kernel (tests/test_gpu_layout.py): the shapes that can go wrong -----------------------------------------

def staircase(steps=8, step_w=16, step_h=8):
    """Columns that rise from left to right in `steps` steps, on the floor of a (steps * step_h) x (steps * step_w + 1) plane:
    the rectangle under step i is (steps - i) * step_w wide and (i + 1) * step_h high, best in the middle."""
    a = np.zeros((steps * step_h, steps * step_w + 1), bool)
    for i in range(steps):
        a[steps * step_h - (i + 1) * step_h:, i * step_w:(i + 1) * step_w] = True
    return a


def comb(h=41, w=65, base=6):
    """1-pixel teeth on every other column, standing on a base of `base` rows."""
    a = np.zeros((h, w), bool)
    a[:, ::2] = True
    a[h - base:] = True
    return a


def plus(n=65, arm=10):
    """Two bars of n x arm that cross in the middle: equal areas, the upright one has the smaller y1."""
    a = np.zeros((n, n), bool)
    lo = (n - arm) // 2
    a[lo:lo + arm] = True
    a[:, lo:lo + arm] = True
    return a


def ell(n=60, arm=10):
    """Two bars of n x arm from the top left corner: equal areas, same y1 and x1, the flat one has the smaller y2."""
    a = np.zeros((n, n), bool)
    a[:arm] = True
    a[:, :arm] = True
    return a


def ring(h=50, w=100, hole=(35, 20, 65, 30)):
    """An open room with a neighbour's text as a hole."""
    a = np.ones((h, w), bool)
    a[hole[1]:hole[3], hole[0]:hole[2]] = False
    return a


def corridor():
    """A 40 x 100 room at the right and a corridor 3 pixels high that leads to it from the left edge: 40 x 160."""
    a = np.zeros((40, 160), bool)
    a[:, 60:] = True
    a[18:21, :60] = True
    return a


def band(h=1024, w=512, half=40):
    """A diagonal band: pixel (x, y) is set where |x - y / 2| < half."""
    ys, xs = np.mgrid[:h, :w]
    return np.abs(xs - ys // 2) < half


def material():
    """[(name, plane (wh, ww) bool, anchor (x, y) in WINDOW coordinates, balloon status)]: one call's blocks."""
    rng = np.random.default_rng(20)
    out = []
    for w, h in ((1, 64), (63, 1), (64, 2), (65, 64), (128, 1), (129, 2), (1000, 64), (64, 64), (1000, 2), (1, 1), (128, 64),
                 (63, 64), (129, 64)):
        out.append((f"ones_{w}x{h}", np.ones((h, w), bool), (w // 2, h // 2), BR.OK))
    a = np.zeros((20, 128), bool)
    a[3:15, 50:80] = True
    out.append(("straddle_63_64", a, (63, 8), BR.OK))
    a = np.zeros((20, 200), bool)
    a[3:15, 120:140] = True
    a[5:9, 100:180] = True
    out.append(("straddle_127_128", a, (128, 6), BR.OK))
    a = np.zeros((10, 300), bool)
    a[2:7, 30:270] = True                                   # words 1, 2 and 3 whole, and into words 0 and 4
    out.append(("three_whole_words", a, (150, 4), BR.OK))
    a = np.zeros((30, 70), bool)
    a[17, 65] = True
    out.append(("single_pixel", a, (65, 17), BR.OK))
    out.append(("staircase", staircase(), (70, 60), BR.OK))
    out.append(("comb", comb(), (32, 3), BR.OK))
    out.append(("plus", plus(), (5, 32), BR.OK))
    out.append(("ell", ell(), (30, 4), BR.OK))
    out.append(("ring_anchor_in", ring(), (10, 25), BR.OK))
    out.append(("ring_anchor_on_hole", ring(), (50, 25), BR.OK))
    out.append(("noise_0.9", rng.random((40, 200)) < 0.9, (100, 20), BR.OK))
    out.append(("noise_0.99", rng.random((40, 200)) < 0.99, (100, 20), BR.OK))
    out.append(("anchor_outside_window", np.ones((20, 70), bool), (-5, 3), BR.OK))
    out.append(("anchor_below_window", np.ones((20, 70), bool), (5, 20), BR.OK))
    out.append(("corridor", corridor(), (10, 19), BR.OK))
    out.append(("not_plain", np.ones((9, 70), bool), (3, 3), BR.NOT_PLAIN))
    out.append(("too_large", np.ones((9, 70), bool), (3, 3), BR.TOO_LARGE))
    out.append(("gone_at_16", np.ones((32, 200), bool), (100, 16), BR.OK))
    a = np.zeros((40, 90), bool)
    a[2:35, 10:50] = True                                   # 33 rows: inset 16 leaves one row of 8 pixels
    out.append(("one_row_left_at_16", a, (30, 18), BR.OK))
    return out
