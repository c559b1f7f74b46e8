"""The tilted-text rule of include/ctd_hip.h ("tilted text") restated in numpy, sequentially: the two maps between a block's
frame and the page, the tilted region T_b with its row, and the tilted compositor -- U as a max-paste over the frame, F by
four taps per page pixel, and from there on `typeset_ref`'s outline and blend over whole pages.  It shares nothing with the
kernels' LDS planes, ballots, frame boxes or tiles, and nothing with the package beyond the rule.

The (c, s) table is built here WITHOUT a libm: `COS16` pins rint(65536 cos(k degrees)) for k = 0 .. 90, every other angle follows
by symmetry.  tests/test_tilt_ref.py holds the package's table (made with numpy's cos and sin) against it.

A tilted layer is a `glyph_ref.glayer` dict plus `angle` (degrees) and `pivot` (x, y); placements are (layer, glyph, x, y)
with x, y in FRAME coordinates."""
import numpy as np

import balloon_ref as BR
import glyph_ref as GR
import typeset_ref as TR

TILTED, FOOTPRINT = 512, 256

COS16 = (65536, 65526, 65496, 65446, 65376, 65287, 65177, 65048, 64898, 64729, 64540, 64332, 64104, 63856, 63589, 63303, 62997, 62672,
         62328, 61966, 61584, 61183, 60764, 60326, 59870, 59396, 58903, 58393, 57865, 57319, 56756, 56175, 55578, 54963, 54332, 53684,
         53020, 52339, 51643, 50931, 50203, 49461, 48703, 47930, 47143, 46341, 45525, 44695, 43852, 42995, 42126, 41243, 40348, 39441,
         38521, 37590, 36647, 35693, 34729, 33754, 32768, 31772, 30767, 29753, 28729, 27697, 26656, 25607, 24550, 23486, 22415, 21336,
         20252, 19161, 18064, 16962, 15855, 14742, 13626, 12505, 11380, 10252, 9121, 7987, 6850, 5712, 4572, 3430, 2287, 1144, 0)


def cs(angle):
    """(c, s) of an integer angle in -180 .. 180 degrees, from COS16 alone."""
    a = int(angle)
    if not -180 <= a <= 180:
        raise ValueError("angle in -180 .. 180")
    k = abs(a)
    c = COS16[k] if k <= 90 else -COS16[180 - k]
    s = COS16[90 - k] if k <= 90 else COS16[k - 90]
    return c, (s if a >= 0 else -s)


def to_page(qx, qy, pivot, c, s):
    """Frame pixels -> (PX, PY), 16.16, int64 arrays."""
    dx, dy = np.asarray(qx, np.int64) - pivot[0], np.asarray(qy, np.int64) - pivot[1]
    return (pivot[0] << 16) + c * dx - s * dy, (pivot[1] << 16) + s * dx + c * dy


def to_frame(px, py, pivot, c, s):
    """Page pixels -> (u, v), 16.16, int64 arrays."""
    dx, dy = np.asarray(px, np.int64) - pivot[0], np.asarray(py, np.int64) - pivot[1]
    return (pivot[0] << 16) + c * dx + s * dy, (pivot[1] << 16) - s * dx + c * dy


def nearest(P):
    return (np.asarray(P, np.int64) + 32768) >> 16


# ---- tilted regions -------------------------------------------------------------------------------------------------------------

def tilt_plane(region, win, pivot, c, s):
    """T_b: `region` (a boolean plane over the window `win` = x1, y1, x2, y2) turned into the frame, over the same window."""
    wx1, wy1, wx2, wy2 = win
    h, w = wy2 - wy1, wx2 - wx1
    out = np.zeros((h, w), bool)
    for y in range(h):                                       # one frame row after the other
        PX, PY = to_page(np.arange(w) + wx1, np.full((w,), y + wy1), pivot, c, s)
        x, yy = nearest(PX) - wx1, nearest(PY) - wy1
        ok = (x >= 0) & (x < w) & (yy >= 0) & (yy < h)
        out[y, ok] = region[yy[ok], x[ok]]
    return out


def tilt_row(src, plane, win, H, W):
    """The OK row of a tilted plane: the source row's status and n_seed, everything else over T_b, bit 8 kept, bit 9 set."""
    wx1, wy1, wx2, wy2 = win
    ys, xs = np.nonzero(plane)
    flags = (src["flags"] & FOOTPRINT) | TILTED
    if len(xs):
        for bit, hit, at_edge in ((BR.CUT_LEFT, plane[:, 0].any(), wx1 == 0), (BR.CUT_TOP, plane[0].any(), wy1 == 0),
                                  (BR.CUT_RIGHT, plane[:, -1].any(), wx2 == W), (BR.CUT_BOTTOM, plane[-1].any(), wy2 == H)):
            if hit:
                flags |= bit << 4 if at_edge else bit
    bbox = [int(xs.min()) + wx1, int(ys.min()) + wy1, int(xs.max()) + wx1 + 1, int(ys.max()) + wy1 + 1] if len(xs) else [0] * 4
    return dict(status=BR.OK, area=len(xs), bbox=bbox, flags=flags, n_seed=src["n_seed"], sum_x=int(xs.sum()) + wx1 * len(xs),
                sum_y=int(ys.sum()) + wy1 * len(ys))


def tilt_block(src, words, win, pivot, angle, H, W, max_words=BR.MAX_WORDS):
    """(row, words or None) of one block: `src` its balloon row (a dict), `words` its u64 words (None where it owns none)."""
    nw, n = BR.n_words(win)
    owns = win[2] > win[0] and win[3] > win[1] and n <= min(max_words, BR.MAX_WORDS)
    if src["status"] != BR.OK:
        return dict(src), (np.zeros((n,), np.uint64) if owns else None)
    if not owns:
        return dict(status=BR.TOO_LARGE, area=0, bbox=[0] * 4, flags=0, n_seed=0, sum_x=0, sum_y=0), None
    c, s = cs(angle)
    plane = tilt_plane(BR.unpack(words, win[3] - win[1], win[2] - win[0]), win, pivot, c, s)
    return tilt_row(src, plane, win, H, W), BR.pack(plane)


# ---- tilted coverage ------------------------------------------------------------------------------------------------------------

def tlayer(page, angle=0, pivot=(0, 0), r=0, fill=(0, 0, 0), stroke=(255, 255, 255), clip=None):
    d = GR.glayer(page, r, fill, stroke, clip)
    d["angle"], d["pivot"] = int(angle), (int(pivot[0]), int(pivot[1]))
    return d


def upright(li, places, atlas, beyond=()):
    """(U, x1, y1): the max-paste of layer li's valid placements over their bounding rectangle, one glyph after the other."""
    vp = GR.valid_places(li, places, atlas, beyond)
    if not vp:
        return np.zeros((0, 0), np.uint8), 0, 0
    x1, y1 = min(x for _, x, _ in vp), min(y for _, _, y in vp)
    x2, y2 = max(x + b.shape[1] for b, x, _ in vp), max(y + b.shape[0] for b, _, y in vp)
    U = np.zeros((y2 - y1, x2 - x1), np.uint8)
    for b, x, y in vp:
        part = U[y - y1:y - y1 + b.shape[0], x - x1:x - x1 + b.shape[1]]
        np.maximum(part, b, out=part)
    return U, x1, y1


def _tap(U, ux, uy, X, Y):
    h, w = U.shape
    ok = (X >= ux) & (X < ux + w) & (Y >= uy) & (Y < uy + h)
    out = np.zeros(X.shape, np.int64)
    out[ok] = U[Y[ok] - uy, X[ok] - ux]
    return out


def coverage(U, ux, uy, pivot, c, s, x1, y1, x2, y2):
    """F on the page rectangle [x1, x2) x [y1, y2)."""
    py, px = np.mgrid[y1:y2, x1:x2]
    u, v = to_frame(px, py, pivot, c, s)
    x0, y0, fx, fy = u >> 16, v >> 16, (u >> 8) & 255, (v >> 8) & 255
    top = _tap(U, ux, uy, x0, y0) * (256 - fx) + _tap(U, ux, uy, x0 + 1, y0) * fx
    bot = _tap(U, ux, uy, x0, y0 + 1) * (256 - fx) + _tap(U, ux, uy, x0 + 1, y0 + 1) * fx
    return ((top * (256 - fy) + bot * fy + 32768) >> 16).astype(np.uint8)


def layer_planes(li, layer, places, atlas, shape, beyond=()):
    """(F, S, (x1, y1, x2, y2)) of a valid layer on the rectangle it may write: page and clip; None where that is empty."""
    H, W = shape
    cx1, cy1, cx2, cy2 = layer.get("clip") or (0, 0, W, H)
    x1, y1, x2, y2 = max(cx1, 0), max(cy1, 0), min(cx2, W), min(cy2, H)
    if x1 >= x2 or y1 >= y2:
        return None
    r = layer["r"]
    U, ux, uy = upright(li, places, atlas, beyond)
    c, s = cs(layer["angle"])
    Fg = coverage(U, ux, uy, layer["pivot"], c, s, x1 - r, y1 - r, x2 + r, y2 + r)
    return Fg[r:Fg.shape[0] - r, r:Fg.shape[1] - r], TR.dilate(Fg, r), (x1, y1, x2, y2)


def typeset(pages, layers, places, atlas, beyond=()):
    """All layers in order onto copies of `pages`: (pages, rows (n, 2) int32 n_fill and n_stroke, written), `written[i]` a
    boolean plane of layer i's page: the pixels it wrote with F > 0 or S > 0 (None for a layer that draws nothing)."""
    out = [p.copy() for p in pages]
    rows = np.zeros((len(layers), 2), np.int32)
    written = [None] * len(layers)
    for li, ly in enumerate(layers):
        if not (0 <= ly["page"] < len(pages)) or ly["r"] > TR.MAX_RADIUS:
            continue
        page = out[ly["page"]]
        got = layer_planes(li, ly, places, atlas, page.shape[:2], beyond)
        if got is None:
            continue
        F, S, (x1, y1, x2, y2) = got
        P = page[y1:y2, x1:x2].astype(np.int64)
        for ch in range(3):
            P[..., ch] = TR.blend(TR.blend(P[..., ch], ly["stroke"][ch], S), ly["fill"][ch], F)
        page[y1:y2, x1:x2] = P.astype(np.uint8)
        rows[li] = int((F > 0).sum()), int((S > 0).sum())
        written[li] = np.zeros(page.shape[:2], bool)
        written[li][y1:y2, x1:x2] = (F > 0) | (S > 0)
    return out, rows, written


# ---- material -------------------------------------------------------------------------------------------------------------------

def ellipse(shape, centre, semi, turn):
    """A filled ellipse with semi-axes `semi` = (a, b) whose a-axis runs along (cos turn, sin turn) in image coordinates (x right,
    y down) -- where the text lines of a block of angle `turn` run, see `to_frame` -- as a boolean plane of `shape` = (H, W)."""
    H, W = shape
    yy, xx = np.mgrid[0:H, 0:W]
    t = np.deg2rad(turn)
    dx, dy = xx - centre[0], yy - centre[1]
    a = dx * np.cos(t) + dy * np.sin(t)
    b = -dx * np.sin(t) + dy * np.cos(t)
    return (a / semi[0]) ** 2 + (b / semi[1]) ** 2 <= 1.0


def erode(plane, m):
    """The layout rule's inner plane: every pixel of the (2m + 1)-square inside the plane and set."""
    if m == 0:
        return plane.copy()
    h, w = plane.shape
    pad = np.zeros((h + 2 * m, w + 2 * m), bool)
    pad[m:m + h, m:m + w] = plane
    out = np.ones((h, w), bool)
    for dy in range(2 * m + 1):
        for dx in range(2 * m + 1):
            out &= pad[dy:dy + h, dx:dx + w]
    return out
