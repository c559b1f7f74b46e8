"""Typeset from a glyph atlas, restated sequentially (the rule: include/ctd_hip.h, the glyph section).  A layer's valid
placements are max-pasted, one glyph after the other, into ONE block bitmap over their bounding rectangle; from there on it is
the existing restatement, `typeset_ref.typeset`, imported and not edited.  So the two oracles of tests/test_gpu_glyphs.py
share the composed bitmaps and nothing else: this file for every byte and row, `typeset.typeset_pages` on the same bitmaps for
the pages.  Also: a brute-force tile table and status (loops over pages, tiles and placements) and a scalar `flow`.
It shares nothing with comic-text-detector_amd/glyphs.py.

A glyph layer here is a dict: page, r, fill and stroke (three ints in the PAGE's channel order), optionally clip.  A placement
is a tuple (layer, glyph, x, y).  The atlas is a list of (h, w) u8 arrays; `beyond` names glyph ids whose record the kernel
must refuse (it does not lie inside atlas_bytes)."""
import numpy as np

import typeset_ref as TR

MAX_COORD = 1 << 29


def glayer(page, r=0, fill=(0, 0, 0), stroke=(255, 255, 255), clip=None):
    d = dict(page=int(page), r=int(r), fill=tuple(fill), stroke=tuple(stroke))
    if clip is not None:
        d["clip"] = tuple(clip)
    return d


def valid_places(li, places, atlas, beyond=()):
    """The placements of layer `li` that contribute, in table order: [(glyph bitmap, x, y)]."""
    out = []
    for lay, g, x, y in places:
        if lay != li or g < 0 or g >= len(atlas) or g in beyond or abs(x) > MAX_COORD or abs(y) > MAX_COORD:
            continue
        if atlas[g].shape[0] == 0 or atlas[g].shape[1] == 0:
            continue
        out.append((atlas[g], int(x), int(y)))
    return out


def compose(li, layer, places, atlas, shape, beyond=()):
    """Layer `li` as ONE bitmap layer of `typeset_ref`: the max-paste of its valid placements over their bounding rectangle,
    cut to the page grown by r + 1 (what lies further out can reach no page pixel).  A layer without such a placement gets a
    bitmap without pixels."""
    H, W = shape
    r = layer["r"]
    vp = valid_places(li, places, atlas, beyond)
    x1 = y1 = x2 = y2 = 0
    if vp:
        x1, y1 = max(min(x for _, x, _ in vp), -r - 1), max(min(y for _, _, y in vp), -r - 1)
        x2, y2 = min(max(x + b.shape[1] for b, x, _ in vp), W + r + 1), min(max(y + b.shape[0] for b, _, y in vp), H + r + 1)
    cov = np.zeros((max(y2 - y1, 0), max(x2 - x1, 0)), np.uint8)
    for b, x, y in vp:                                       # one glyph after the other
        for by in range(b.shape[0]):
            yy = y + by - y1
            if yy < 0 or yy >= cov.shape[0]:
                continue
            a1, a2 = max(x, x1), min(x + b.shape[1], x2)
            if a1 < a2:
                cov[yy, a1 - x1:a2 - x1] = np.maximum(cov[yy, a1 - x1:a2 - x1], b[by, a1 - x:a2 - x])
    return TR.layer(layer["page"], cov, x1, y1, r, layer["fill"], layer["stroke"], layer.get("clip"))


def composed(layers, places, atlas, shapes, beyond=()):
    """Every layer as a bitmap layer.  A layer whose page is none keeps its page, which `typeset_ref.is_valid` refuses."""
    out = []
    for li, ly in enumerate(layers):
        shape = shapes[ly["page"]] if 0 <= ly["page"] < len(shapes) else (1, 1)
        out.append(compose(li, ly, places, atlas, shape, beyond))
    return out


def typeset(pages, layers, places, atlas, beyond=()):
    """(pages, rows, bitmap layers): all layers in order onto copies of `pages`, by `typeset_ref.typeset` on the composed
    bitmaps."""
    bl = composed(layers, places, atlas, [p.shape[:2] for p in pages], beyond)
    out, rows = TR.typeset(pages, bl)
    return out, rows, bl


def _grown(layer, x, y, w, h, H, W):
    r = layer["r"]
    cx1, cy1, cx2, cy2 = layer.get("clip") or (0, 0, W, H)
    return max(x - r, cx1, 0), max(y - r, cy1, 0), min(x + w + r, cx2, W), min(y + h + r, cy2, H)


def status_of(li, layers, places, sizes, shapes):
    """EMPTY: no placement of the layer has a glyph with pixels; OUTSIDE: none of those meets page and clip; OK."""
    H, W = shapes[layers[li]["page"]]
    inked = drawn = 0
    for i, (lay, g, x, y) in enumerate(places):
        h, w = sizes[i]
        if lay != li or h == 0 or w == 0:
            continue
        inked += 1
        x1, y1, x2, y2 = _grown(layers[li], x, y, w, h, H, W)
        drawn += x1 < x2 and y1 < y2
    return TR.EMPTY if not inked else TR.OUTSIDE if not drawn else TR.OK


def tables_brute(shapes, layers, places, sizes, tw, th):
    """The tile table by a loop over pages, tiles and placements: ([(page, tx, ty, first)] + [(0, 0, 0, n_entries)], entries).
    sizes[i] = (h, w) of placement i's glyph."""
    tiles, entries = [], []
    for pg, (H, W) in enumerate(shapes):
        for ty in range((H + th - 1) // th):
            for tx in range((W + tw - 1) // tw):
                mine = []
                for i, (lay, g, x, y) in enumerate(places):
                    h, w = sizes[i]
                    if layers[lay]["page"] != pg or h == 0 or w == 0:
                        continue
                    x1, y1, x2, y2 = _grown(layers[lay], x, y, w, h, H, W)
                    if max(x1, tx * tw) < min(x2, tx * tw + tw) and max(y1, ty * th) < min(y2, ty * th + th):
                        mine.append(i)
                if mine:
                    tiles.append((pg, tx, ty, len(entries)))
                    entries += mine
    return tiles + [(0, 0, 0, len(entries))], entries


def flow_brute(ids, sizes, advance, bearing, rect, line=None, gap=0, vertical=False, breaks=None, align="center"):
    """`glyphs.flow` one glyph at a time.  sizes / advance / bearing: per glyph ID.  ([(x, y)], fits)"""
    x1, y1, x2, y2 = rect
    ax = 1 if vertical else 0
    along, across = (y2 - y1, x2 - x1) if vertical else (x2 - x1, y2 - y1)
    n = len(ids)
    if line is None:
        line = max([sizes[g][ax] for g in ids], default=0)   # sizes are (h, w): the tallest, or for columns the widest
    lines, cur, pen, i = [], [], 0, 0
    while i < n:
        a = advance[ids[i]][ax]
        if cur and pen + a > along:
            end = i
            if breaks is not None:
                for k in range(i - 1, cur[0] - 1, -1):
                    if breaks[k]:
                        end = k + 1
                        break
            lines.append(list(range(cur[0], end)))
            cur, pen, i = [], 0, end
            continue
        cur.append(i)
        pen += a
        i += 1
    if cur:
        lines.append(cur)
    total = len(lines) * line + max(len(lines) - 1, 0) * gap
    lead = (across - total) >> 1
    xy, fits = [None] * n, total <= across
    for c, ln in enumerate(lines):
        length = sum(advance[ids[i]][ax] for i in ln)
        fits = fits and length <= along
        slack = along - length
        pen = {"left": 0, "center": slack >> 1, "right": slack}[align]
        for i in ln:
            g = ids[i]
            if vertical:
                left = x1 + lead + total - line - c * (line + gap)
                xy[i] = (left + ((line - sizes[g][1]) >> 1) + bearing[g][0], y1 + pen + bearing[g][1])
            else:
                xy[i] = (x1 + pen + bearing[g][0], y1 + lead + c * (line + gap) + bearing[g][1])
            pen += advance[ids[i]][ax]
    return xy, bool(fits)


# ---- material -------------------------------------------------------------------------------------------------------------------

def small_atlas():
    """Ten glyphs: glyph-like, noise, solid, a 2 x 2, two without pixels."""
    return [TR.glyph(12, 10, 1), TR.noise(9, 14, 2), TR.solid(8, 8, 255), np.zeros((0, 5), np.uint8), TR.solid(2, 2, 200),
            TR.glyph(24, 24, 3), TR.noise(16, 24, 4), np.zeros((5, 0), np.uint8), TR.glyph(7, 19, 5), TR.solid(1, 1, 255)]


def small_case():
    """(layers, places) over `typeset_ref.SHAPES` and `small_atlas`: see tests/test_gpu_glyphs.py test 1 for what they cover."""
    L, P = [], []

    def add(ly, run):
        L.append(ly)
        P.extend((len(L) - 1, g, x, y) for g, x, y in run)

    # page 0 is 70 x 130 (tile seams at x = 64 and y = 32, 64, 96, 128), page 3 is 129 x 67 (x = 64, 128; y = 32, 64)
    add(glayer(0, 3, (200, 10, 10), (0, 0, 0)), [(0, 58, 26), (1, 57, 60), (8, 50, 90)])          # across the corners 63/64, 31/32
    add(glayer(3, 12, (0, 0, 255), (255, 255, 0)), [(2, 75, 10), (2, 76, 40)])                    # 11 and 12 inside the next tile
    add(glayer(0, 2, (10, 200, 10), (255, 255, 0)), [(5, 10, 90), (6, 20, 95), (5, 14, 92)])      # overlap: max, not sum
    add(glayer(3, 1, (9, 9, 9), (240, 0, 240)), [(4, 3 + 5 * (k % 25), 50 + 7 * (k // 25)) for k in range(50)])   # one id 50 times
    add(glayer(0, 4, (1, 2, 3), (250, 251, 252)), [(0, 5, 5), (3, 16, 5), (1, 20, 5), (7, 35, 5), (8, 36, 5)])   # spaces in a run
    add(glayer(0, 6, (9, 9, 9), (240, 240, 0), clip=(25, 41, 40, 58)), [(6, 20, 44)])             # cut by its clip
    add(glayer(3, 6, (9, 9, 9), (0, 240, 240), clip=(-50, 34, 1000, 1000)), [(6, 20, 30), (5, 100, 40)])
    add(glayer(1, 5, (255, 255, 255), (0, 0, 0)), [(5, -6, -5), (5, 50, 20), (9, 30, 15)])        # the one-tile page, over its edges
    add(glayer(2, 2, (1, 2, 3), (250, 251, 252)), [(1, -1, -1)])                                  # the 1 x 1 page
    add(glayer(0, 12, (0, 0, 0), (255, 255, 255)), [(0, 400, 10), (0, -23, 10)])                  # OUTSIDE: off the page by > r
    add(glayer(0, 3), [(3, 10, 10), (7, 12, 10)])                                                 # EMPTY: spaces only
    add(glayer(0, 3), [])                                                                         # EMPTY: no placement
    add(glayer(0, 0, (255, 0, 0), (0, 255, 255)), [(8, 40, 120), (0, 62, 115), (9, 69, 129)])     # r = 0, the page's last pixel
    return L, P


def overlapping():
    """Two layers that overlap each other on one tile of page 0."""
    return ([glayer(0, 3, (200, 10, 10), (0, 0, 0)), glayer(0, 2, (10, 200, 10), (255, 255, 0))],
            [(0, 5, 10, 70), (0, 6, 22, 72), (1, 6, 14, 76), (1, 5, 30, 70)])
