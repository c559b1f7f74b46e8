"""The typeset rule of include/ctd_hip.h restated in numpy, sequentially: layer by layer over whole pages, the outline S as a
max over one shifted copy of the coverage per offset of the disk.  It shares nothing with the kernel's tiles, its LDS patch
or its running maxima.  Also: a brute-force tile table (a loop over pages, tiles and layers) and the material of the tests.

A layer here is a dict: page, cov (h x w u8 array), x0, y0, fill and stroke (three ints in the PAGE's channel order), r, and
optionally clip = (x1, y1, x2, y2) exclusive (default: the page) and w / h / beyond, which override what the layer table
says without changing `cov` (how the tests state a layer the kernel must refuse)."""
import numpy as np

MAX_SIDE, MAX_RADIUS = 8192, 12
OK, EMPTY, OUTSIDE = range(3)
DISK_SIZES = {1: 5, 2: 13, 3: 29, 4: 49, 5: 81, 6: 113, 7: 149, 8: 197, 9: 253, 10: 317, 11: 377, 12: 441}


def disk(r):
    """The offsets (dx, dy) with dx^2 + dy^2 <= r^2."""
    return [(dx, dy) for dy in range(-r, r + 1) for dx in range(-r, r + 1) if dx * dx + dy * dy <= r * r]


def blend(c, k, a):
    """(c (255 - a) + k a + 127) / 255, integer division; c, k, a ints or int arrays in 0 .. 255."""
    c, k, a = np.asarray(c, np.int64), np.asarray(k, np.int64), np.asarray(a, np.int64)
    return (c * (255 - a) + k * a + 127) // 255


def coverage(layer, x1, y1, x2, y2):
    """F on the page rectangle [x1, x2) x [y1, y2): the bitmap where it lies, 0 elsewhere."""
    cov = layer["cov"]
    h, w = cov.shape
    out = np.zeros((y2 - y1, x2 - x1), np.uint8)
    bx1, by1 = max(x1, layer["x0"]), max(y1, layer["y0"])
    bx2, by2 = min(x2, layer["x0"] + w), min(y2, layer["y0"] + h)
    if bx1 < bx2 and by1 < by2:
        out[by1 - y1:by2 - y1, bx1 - x1:bx2 - x1] = cov[by1 - layer["y0"]:by2 - layer["y0"], bx1 - layer["x0"]:bx2 - layer["x0"]]
    return out


def dilate(Fg, r):
    """S on the inner part of Fg, which carries r extra pixels on every side: the max over the disk, one shifted copy each."""
    H, W = Fg.shape[0] - 2 * r, Fg.shape[1] - 2 * r
    S = np.zeros((H, W), np.uint8)
    if r == 0:
        return S
    for dx, dy in disk(r):
        np.maximum(S, Fg[r + dy:r + dy + H, r + dx:r + dx + W], out=S)
    return S


def is_valid(layer, n_pages):
    h, w = layer.get("h", layer["cov"].shape[0]), layer.get("w", layer["cov"].shape[1])
    return (0 <= layer["page"] < n_pages and 1 <= w <= MAX_SIDE and 1 <= h <= MAX_SIDE and layer["r"] <= MAX_RADIUS and
            not layer.get("beyond", False))


def written_rect(layer, H, W):
    """The rectangle a valid layer writes: page, clip, the bitmap's rectangle grown by r.  (x1, y1, x2, y2), maybe empty."""
    h, w = layer["cov"].shape
    r = layer["r"]
    cx1, cy1, cx2, cy2 = layer.get("clip") or (0, 0, W, H)
    return (max(layer["x0"] - r, cx1, 0), max(layer["y0"] - r, cy1, 0),
            min(layer["x0"] + w + r, cx2, W), min(layer["y0"] + h + r, cy2, H))


def apply_layer(page, layer):
    """One layer onto `page` (H, W, 3 u8, in place).  (n_fill, n_stroke)"""
    H, W = page.shape[:2]
    x1, y1, x2, y2 = written_rect(layer, H, W)
    if x1 >= x2 or y1 >= y2:
        return 0, 0
    r = layer["r"]
    Fg = coverage(layer, x1 - r, y1 - r, x2 + r, y2 + r)
    F = Fg[r:Fg.shape[0] - r, r:Fg.shape[1] - r]
    S = dilate(Fg, r)
    P = page[y1:y2, x1:x2].astype(np.int64)
    for c in range(3):
        P[..., c] = blend(blend(P[..., c], layer["stroke"][c], S), layer["fill"][c], F)
    page[y1:y2, x1:x2] = P.astype(np.uint8)
    return int((F > 0).sum()), int((S > 0).sum())


def typeset(pages, layers):
    """All layers in order onto copies of `pages`.  (pages, rows) with rows (n, 2) int32: n_fill, n_stroke."""
    out = [p.copy() for p in pages]
    rows = np.zeros((len(layers), 2), np.int32)
    for i, ly in enumerate(layers):
        if is_valid(ly, len(pages)):
            rows[i] = apply_layer(out[ly["page"]], ly)
    return out, rows


def status_of(layer, H, W):
    h, w = layer["cov"].shape
    if w == 0 or h == 0:
        return EMPTY
    x1, y1, x2, y2 = written_rect(layer, H, W)
    return OUTSIDE if x1 >= x2 or y1 >= y2 else OK


def tables_brute(shapes, layers, tw, th):
    """The tile table by a loop over pages, tiles and layers: ([(page, tx, ty, first)] + [(0, 0, 0, n_entries)], entries).
    A layer is listed whatever its validity, as long as its rectangle meets the tile: refusing it is the kernel's part."""
    tiles, entries = [], []
    for pg, (H, W) in enumerate(shapes):
        for ty in range((H + th - 1) // th):
            for tx in range((W + tw - 1) // tw):
                mine = []
                for i, ly in enumerate(layers):
                    if ly["page"] != pg or 0 in ly["cov"].shape:
                        continue
                    x1, y1, x2, y2 = written_rect(ly, H, W)
                    if max(x1, tx * tw) < min(x2, tx * tw + tw) and max(y1, ty * th) < min(y2, ty * th + th):
                        mine.append(i)
                if mine:
                    tiles.append((pg, tx, ty, len(entries)))
                    entries += mine
    return tiles + [(0, 0, 0, len(entries))], entries


# ---- material -------------------------------------------------------------------------------------------------------------------

def glyph(h, w, seed=0):
    """Glyph-like coverage: a few strokes with anti-aliased (ramped) edges on an empty ground."""
    rng = np.random.default_rng(seed)
    a = np.zeros((h, w), np.float64)
    yy, xx = np.mgrid[0:h, 0:w]
    for _ in range(3):
        cx, cy, ang = rng.uniform(0, w), rng.uniform(0, h), rng.uniform(0, np.pi)
        d = np.abs((xx - cx) * np.sin(ang) - (yy - cy) * np.cos(ang))
        a = np.maximum(a, np.clip(1.6 - d, 0, 1))
    return np.round(a * 255).astype(np.uint8)


def noise(h, w, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)


def solid(h, w, v=255):
    return np.full((h, w), v, np.uint8)


def layer(page, cov, x0, y0, r=0, fill=(0, 0, 0), stroke=(255, 255, 255), clip=None, **kw):
    d = dict(page=page, cov=np.ascontiguousarray(cov, np.uint8), x0=int(x0), y0=int(y0), r=int(r), fill=tuple(fill), stroke=tuple(stroke))
    if clip is not None:
        d["clip"] = tuple(clip)
    d.update(kw)
    return d


SHAPES = [(130, 70), (32, 64), (1, 1), (67, 129)]            # (H, W): 70 x 130, 64 x 32 (exactly one tile), 1 x 1, 129 x 67


def small_pages(seed=5):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in SHAPES]


def overlapping():
    """Three mutually overlapping layers on page 0."""
    return [layer(0, glyph(20, 30, 1), 20, 60, 3, (200, 10, 10), (0, 0, 0)),
            layer(0, noise(18, 26, 2), 30, 68, 2, (10, 200, 10), (255, 255, 0)),
            layer(0, solid(14, 22, 160), 26, 64, 5, (10, 10, 200), (0, 255, 255))]


def small_layers():
    """About 40 hand-made layers over `SHAPES`: see tests/test_gpu_typeset.py test 1 for what they must cover."""
    out = []
    for r in range(13):                                      # every radius, glyph-like and noise in turn, across page 0 and 3
        cov = glyph(9 + r, 14 + r, r) if r % 2 else noise(7 + r, 11 + r, r)
        pg = 0 if r < 7 else 3
        out.append(layer(pg, cov, (5 + 9 * r) % 50 if pg == 0 else 3 + 18 * (r - 7), 3 + 17 * r if pg == 0 else 5 + 8 * (r - 7), r,
                         (r * 20, 255 - r * 20, 7), (255 - r * 9, r * 9, 200)))
    out += [layer(0, solid(1, 1, 255), 30, 100, 4, (0, 0, 0), (255, 255, 255)),
            layer(0, solid(1, 1, 1), 50, 100, 4, (0, 0, 0), (255, 255, 255)),
            layer(0, solid(5, 5, 255), 60, 5, 0, (255, 255, 255), (0, 0, 0)),
            layer(0, solid(5, 5, 255), 60, 15, 2, (0, 0, 0), (0, 0, 0)),
            layer(0, solid(5, 5, 255), 60, 25, 2, (255, 255, 255), (255, 255, 255))]
    # across each edge and each corner of page 0 and of the one-tile page 1
    for pg, (H, W) in ((0, SHAPES[0]), (1, SHAPES[1])):
        for k, (x, y) in enumerate(((-6, H // 2), (W - 6, H // 2), (W // 2, -5), (W // 2, H - 5),
                                    (-6, -5), (W - 6, -5), (-6, H - 5), (W - 6, H - 5))):
            out.append(layer(pg, glyph(11, 13, 20 + k), x, y, 1 + k % 4, (30 * k, 9, 250 - 30 * k), (250 - 30 * k, 250, 30 * k)))
    out += [layer(2, noise(3, 3, 40), -1, -1, 2, (1, 2, 3), (250, 251, 252)),          # the 1 x 1 page
            layer(0, glyph(8, 8, 41), 400, 10, 12),                                    # wholly off the page
            layer(0, glyph(8, 8, 42), -21, 10, 12),                                    # off by one pixel more than the radius
            layer(0, np.zeros((0, 7), np.uint8), 10, 10, 3),                           # zero size
            layer(0, np.zeros((7, 0), np.uint8), 10, 10, 3),
            layer(0, glyph(8, 8, 43), 20, 40, 3, clip=(30, 30, 30, 60)),               # an empty clip
            layer(0, glyph(8, 8, 44), 20, 40, 3, clip=(60, 0, 70, 130)),               # a clip that misses it
            layer(0, noise(16, 24, 45), 20, 44, 6, (9, 9, 9), (240, 240, 0), clip=(25, 41, 40, 58)),   # cut by its clip
            layer(3, noise(16, 24, 46), 20, 30, 6, (9, 9, 9), (240, 0, 240), clip=(-50, 34, 1000, 1000))]
    # ends exactly on the tile seam x = 64 of page 3 / y = 32 of page 0, and a pixel either side, at r = 12: the outline
    # reaches tiles the bitmap does not
    for k, end in enumerate((63, 64, 65)):
        out.append(layer(3, glyph(10, 20, 50 + k), end - 20, 40 + k, 12, (0, 0, 255), (255, 255, 0)))
        out.append(layer(0, glyph(10, 20, 53 + k), 10 + 3 * k, end - 32 - 10, 12, (255, 0, 0), (0, 255, 255)))
    return out + overlapping()
