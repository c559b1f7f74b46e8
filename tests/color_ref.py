"""numpy restatement of the font-colour rule (include/ctd_hip.h, "font colours"): the fill and the surround colour of one text
line from (page, mask, quad), integers only.  Written from the rule's statement, vectorised per line, with Python integers
where products could leave int64.  The product's kernel (csrc/kernels_color.hip) is compared with `line_color` field by field
(tests/test_gpu_colors.py); tests/test_color_ref.py checks the rule's own promises here, without a GPU."""
import numpy as np

OK, EMPTY, NO_MASK, NO_CONTRAST, TOO_LARGE = range(5)
MAX_PIXELS, MAX_COORD = 1 << 24, 1 << 29
FIELDS = ("n_fg", "s_fg", "n_bg", "s_bg", "g_on", "g_off", "n_on", "n_off", "status", "fg", "bg")


def grey(px):
    """(..., 3) u8 BGR -> grey, the formula of csrc/kernels_tail.hip / oracle/cv_ref.py."""
    p = px.astype(np.int64)
    return (p[..., 0] * 3735 + p[..., 1] * 19235 + p[..., 2] * 9798 + 16384) >> 15


def clipped_box(quad, H, W):
    """(x0, y0, x1, y1) of the quad's bounding box clipped to the page, inclusive; x1 < x0 or y1 < y0: nothing."""
    q = np.asarray(quad, np.int64).reshape(4, 2)
    return max(int(q[:, 0].min()), 0), max(int(q[:, 1].min()), 0), min(int(q[:, 0].max()), W - 1), min(int(q[:, 1].max()), H - 1)


def inside(quad, H, W):
    """(x0, y0, bool array over the clipped box) or None: the four cross products all >= 0 or all <= 0."""
    x0, y0, x1, y1 = clipped_box(quad, H, W)
    if x1 < x0 or y1 < y0:
        return None
    q = np.asarray(quad, np.int64).reshape(4, 2)
    ys, xs = np.mgrid[y0:y1 + 1, x0:x1 + 1].astype(np.int64)
    ge = np.ones(xs.shape, bool)
    le = np.ones(xs.shape, bool)
    for k in range(4):
        ex, ey = q[(k + 1) % 4] - q[k]                   # |coordinates| <= 2^29: every product below 2^61
        c = ex * (ys - q[k, 1]) - ey * (xs - q[k, 0])
        ge &= c >= 0
        le &= c <= 0
    return x0, y0, ge | le


def text_like_distance(g, n_on, n_off, g_on, g_off):
    """The definition: |g n_on - g_on| n_off < |g n_off - g_off| n_on, per grey value in Python integers."""
    return np.array([abs(int(v) * n_on - g_on) * n_off < abs(int(v) * n_off - g_off) * n_on for v in np.asarray(g).reshape(-1)],
                    bool).reshape(np.shape(g))


def text_like_threshold(g, n_on, n_off, g_on, g_off):
    """The single-threshold form: 2 g n_on n_off above (ON mean higher) or below g_on n_off + g_off n_on."""
    lhs, rhs = g_on * n_off, g_off * n_on
    D, S = 2 * n_on * n_off, lhs + rhs
    g = np.asarray(g, np.int64)
    if lhs > rhs:
        return g >= S // D + 1
    if lhs < rhs:
        return g <= (S + D - 1) // D - 1
    return np.zeros(g.shape, bool)


def _mean(s, n):
    return [(2 * int(v) + n) // (2 * n) for v in s]


def line_color(page, mask, quad):
    """One row of `ctd_line_colors` as a dict of Python ints / lists (channels in page order, BGR)."""
    page, mask = np.asarray(page), np.asarray(mask)
    H, W = page.shape[:2]
    assert page.dtype == np.uint8 and page.shape == (H, W, 3) and mask.dtype == np.uint8 and mask.shape == (H, W)
    r = dict(n_fg=0, s_fg=[0, 0, 0], n_bg=0, s_bg=[0, 0, 0], g_on=0, g_off=0, n_on=0, n_off=0, status=EMPTY, fg=[0, 0, 0],
             bg=[0, 0, 0])
    q = [int(v) for v in np.asarray(quad).reshape(8)]
    x0, y0, x1, y1 = clipped_box(q, H, W)
    empty_box = x1 < x0 or y1 < y0
    if max(abs(v) for v in q) > MAX_COORD or (not empty_box and (x1 - x0 + 1) * (y1 - y0 + 1) > MAX_PIXELS):
        r["status"] = TOO_LARGE                          # from the quad, H and W alone
        return r
    ins = None if empty_box else inside(q, H, W)
    if ins is None or not ins[2].any():
        return r
    x0, y0, sel = ins
    px = page[y0:y0 + sel.shape[0], x0:x0 + sel.shape[1]][sel]           # (n, 3)
    on = mask[y0:y0 + sel.shape[0], x0:x0 + sel.shape[1]][sel] != 0
    g = grey(px)
    n_on, n_off = int(on.sum()), int((~on).sum())
    g_on, g_off = int(g[on].sum()), int(g[~on].sum())
    r.update(n_on=n_on, n_off=n_off, g_on=g_on, g_off=g_off)
    if n_on == 0:
        r["status"] = NO_MASK
        return r
    if n_off == 0 or g_on * n_off == g_off * n_on:
        r["status"] = NO_CONTRAST
        fg_sel, bg_sel = on, ~on
    else:
        r["status"] = OK
        like = text_like_distance(np.arange(256), n_on, n_off, g_on, g_off)[g]
        fg_sel, bg_sel = on & like, ~like
    r["n_fg"], r["n_bg"] = int(fg_sel.sum()), int(bg_sel.sum())
    r["s_fg"] = [int(v) for v in px[fg_sel].astype(np.int64).sum(0)]
    r["s_bg"] = [int(v) for v in px[bg_sel].astype(np.int64).sum(0)]
    r["fg"] = _mean(r["s_fg"], r["n_fg"])
    r["bg"] = _mean(r["s_bg"], r["n_bg"]) if r["n_bg"] else list(r["fg"])
    return r


def row_dict(row):
    """A record of the product's `colors.OUT_DTYPE` as the dict `line_color` returns."""
    return {k: (row[k].tolist() if np.ndim(row[k]) else int(row[k])) for k in FIELDS}


def pooled(rows):
    """Per-block pooling of `LineColors.blocks()` over the OK / NO_CONTRAST rows of one block: (valid, fg RGB, bg RGB)."""
    use = [r for r in rows if r["status"] in (OK, NO_CONTRAST)]
    n_fg, n_bg = sum(r["n_fg"] for r in use), sum(r["n_bg"] for r in use)
    if n_fg == 0:
        return False, [0, 0, 0], [0, 0, 0]
    fg = _mean([sum(r["s_fg"][c] for r in use) for c in range(3)], n_fg)
    bg = _mean([sum(r["s_bg"][c] for r in use) for c in range(3)], n_bg) if n_bg else list(fg)
    return True, fg[::-1], bg[::-1]


# ---- shared test material ------------------------------------------------------------------------------------------------

def dilate(mask, r):
    """Binary dilation by a (2r+1)-square, numpy only."""
    m = np.pad(mask != 0, r)
    out = np.zeros(mask.shape, bool)
    for dy in range(2 * r + 1):
        for dx in range(2 * r + 1):
            out |= m[dy:dy + mask.shape[0], dx:dx + mask.shape[1]]
    return out.astype(np.uint8) * 255


def flat_page(text_bgr, back_bgr, shape=(96, 160)):
    """A two-colour page with bar 'glyphs' (vertical bars 3 wide every 7 columns in two text rows, plus one tilted band) and
    the tight mask of the glyphs."""
    H, W = shape
    glyph = np.zeros((H, W), bool)
    for y0 in (14, 52):
        for x in range(12, W - 12, 7):
            glyph[y0:y0 + 22, x:x + 3] = True
    yy, xx = np.mgrid[0:H, 0:W]
    glyph |= (np.abs((yy - 40) - (xx - 80) * 0.5) < 2) & (np.abs(xx - 80) < 40)
    page = np.empty((H, W, 3), np.uint8)
    page[:] = np.asarray(back_bgr, np.uint8)
    page[glyph] = np.asarray(text_bgr, np.uint8)
    return page, glyph.astype(np.uint8) * 255


FLAT_COLOURS = [((20, 20, 20), (240, 240, 240)),         # dark on light
                ((250, 250, 250), (30, 40, 50)),         # light on dark
                ((0, 0, 255), (0, 255, 0)),              # red on green (BGR): greys 76 / 150
                ((200, 60, 10), (90, 200, 220))]
FLAT_QUADS = [[10, 12, 150, 12, 150, 38, 10, 38],        # axis-aligned
              [10, 38, 150, 38, 150, 12, 10, 12],        # its reversed winding
              [8, 50, 150, 44, 152, 76, 10, 80],         # tilted
              [-20, 40, 100, -10, 120, 30, 0, 90],       # leaves the page (left and top)
              [100, 60, 200, 50, 205, 110, 105, 120]]    # leaves the page (right and bottom)


def flat_cases():
    """(page, mask, quad, text BGR, background BGR): every colour pair x tight / dilated-by-2 mask x every quad."""
    for text, back in FLAT_COLOURS:
        page, tight = flat_page(text, back)
        for mask in (tight, dilate(tight, 2)):
            for q in FLAT_QUADS:
                yield page, mask, q, list(text), list(back)
