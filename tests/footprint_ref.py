"""numpy restatement of the footprint rule (include/ctd_hip.h, "footprint regions"): per block whose erase row says TEXTURED or
NO_RING, the place where its old text stood -- the orthogonally convex closure of F_b, grown by `pad`, minus other blocks'
text -- as an OK balloon row and a bit plane.  Written from the rule's statement: the erase rows and D_k come from
tests/erase_ref.py, the windows, the packing and the PLAIN blocks from tests/balloon_ref.py, and the closure from per-row and
per-column `flatnonzero` spans on a boolean plane, repeated until nothing changes (`closure`) -- nothing like the kernel's
prefix and suffix ORs over words (csrc/kernels_footprint.hip).  `brute_closures` is a second method for tiny planes, a search
over all supersets, that the CPU tests hold against the spans.  The kernel is compared with `footprint_page` field by field and
word by word (tests/test_gpu_footprint.py); tests/test_footprint_ref.py checks the rule's own promises here."""
import numpy as np

import balloon_ref as BR
import erase_ref as ER

FOOTPRINT, MAX_PAD = 256, 16
DEFAULTS = dict(BR.DEFAULTS, pad=4)


def check_params(grow, tol, reach, reach_min, pad):
    BR.check_params(grow, tol, reach, reach_min)
    if not 0 <= pad <= MAX_PAD:
        raise ValueError("pad 0..16")


def closure(plane):
    """(the orthogonally convex closure of a boolean plane, the rounds that changed it).  A round: every row's span from its
    first to its last pixel is filled, then every column's."""
    q = np.array(plane, bool)
    rounds = 0
    while True:
        before = q.copy()
        for line in list(q) + list(q.T):                     # rows (views of q), then columns
            at = np.flatnonzero(line)
            if len(at):
                line[at[0]:at[-1] + 1] = True
        if np.array_equal(q, before):
            return q, rounds
        rounds += 1


def is_convex(q):
    """Every row and every column of q holds at most one run."""
    for line in list(q) + list(q.T):
        at = np.flatnonzero(line)
        if len(at) and not line[at[0]:at[-1] + 1].all():
            return False
    return True


def brute_closures(h, w):
    """The smallest orthogonally convex superset of EVERY subset of an h x w plane (h * w <= 16) by search: code -> code, a
    plane's code being its pixels as the bits of an integer, row by row.  Every plane is tested for convexity on its own;
    a subset's closure is the smallest convex plane among ALL that contain it (the rule says there is one of that size)."""
    n = h * w
    codes = np.arange(1 << n, dtype=np.int64)
    planes = ((codes[:, None] >> np.arange(n)) & 1).astype(bool).reshape(-1, h, w)
    convex = codes[[is_convex(q) for q in planes]]
    size = planes.reshape(len(codes), -1).sum(axis=1)
    out = np.zeros_like(codes)
    for c in codes:
        over = convex[(convex & c) == c]
        least = over[size[over] == size[over].min()]
        assert len(least) == 1, "the smallest convex superset is unique"
        out[c] = least[0]
    return out, planes


def chain(links=24, dx=8, dy=6):
    """A seed whose closure takes one half-round per link: two pixels in row 0, ten apart; then every link one pixel inside the
    far end of the span that the previous half-round filled -- an odd link below it (a column span of eight), an even link to
    its right (a row span of ten).  (plane, seed pixels as (x, y)); 24 links: 74 x 106, 26 pixels, 339 in the closure, 13
    rounds."""
    pts = [(0, 0), (dx + 1, 0)]
    for k in range(1, links + 1):
        i = (k + 1) // 2
        pts.append((dx * i, dy * (i - 1) + dy + 1) if k % 2 else (dx * i + dx + 1, dy * i))
    w, h = max(p[0] for p in pts) + 1, max(p[1] for p in pts) + 1
    plane = np.zeros((h, w), bool)
    for x, y in pts:
        plane[y, x] = True
    return plane, pts


def region_row(region, win, H, W, n_seed):
    """The OK row of a region (a boolean plane over the window `win` of an H x W page) with the footprint bit."""
    wx1, wy1, wx2, wy2 = win
    ys, xs = np.nonzero(region)
    flags = FOOTPRINT
    if len(xs):
        for bit, hit, at_edge in ((BR.CUT_LEFT, region[:, 0].any(), wx1 == 0), (BR.CUT_TOP, region[0].any(), wy1 == 0),
                                  (BR.CUT_RIGHT, region[:, -1].any(), wx2 == W), (BR.CUT_BOTTOM, region[-1].any(), wy2 == H)):
            if hit:
                flags |= bit << 4 if at_edge else bit
    bbox = [int(xs.min()) + wx1, int(ys.min()) + wy1, int(xs.max()) + wx1 + 1, int(ys.max()) + wy1 + 1] if len(xs) else [0] * 4
    return dict(status=BR.OK, area=len(xs), bbox=bbox, flags=flags, n_seed=n_seed, sum_x=int(xs.sum()) + wx1 * len(xs),
                sum_y=int(ys.sum()) + wy1 * len(ys))


def block_footprint(text, xyxy, erow, grow, reach, reach_min, pad, max_words=BR.MAX_WORDS):
    """(row, words, plane over the window) of one block, or None where it is not eligible.  text = M as a boolean plane."""
    if erow["status"] not in (ER.TEXTURED, ER.NO_RING):
        return None
    H, W = text.shape
    box, win = BR.window(xyxy, H, W, reach, reach_min)
    nw, words = BR.n_words(win)
    if words > min(BR.MAX_WORDS, max_words):
        return None
    x1, y1, x2, y2 = box
    wx1, wy1, wx2, wy2 = win
    T = np.zeros((H, W), bool)
    T[y1:y2, x1:x2] = text[y1:y2, x1:x2]
    F = ER.dilate(T, grow)
    seed = F[wy1:wy2, wx1:wx2]
    assert int(seed.sum()) == int(F.sum()) == erow["n_fill"]
    closed, _ = closure(seed)
    padded = ER.dilate(closed, pad)                             # on the window's plane: clipped to the window
    other = text.copy()
    other[y1:y2, x1:x2] = False
    region = padded & ~other[wy1:wy2, wx1:wx2]
    return region_row(region, win, H, W, int(seed.sum())), BR.pack(region), region


def footprint_page(page, mask, boxes, erows=None, grow=2, tol=12, reach=8, reach_min=32, pad=4, footprint=True, method=BR.flood):
    """Both rules on one page, as `balloons.balloon_regions(..., footprint=True)` leaves the tables: (rows, words per block
    (None where the block owns none), windows, erase rows).  Arguments as `balloon_ref.balloon_page`."""
    check_params(grow, tol, reach, reach_min, pad)
    rows, words, wins, erows = BR.balloon_page(page, mask, boxes, erows, grow, tol, reach, reach_min, method)
    rows, words = list(rows), list(words)
    text = np.asarray(mask) != 0
    for k, (b, e) in enumerate(zip(boxes, erows)):
        fp = block_footprint(text, b, e, grow, reach, reach_min, pad) if footprint else None
        if fp is not None:
            rows[k], words[k] = fp[0], fp[1]
    return rows, words, wins, erows
