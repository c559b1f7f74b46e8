"""Typeset: text layers with outlines composited into pages, on the GPU.

`layout_boxes` gives the box to lay the translated text into; any font engine renders that text into 8-bit coverage bitmaps.
This is the step that puts them into the device pages, with the outline that is the standard manga treatment:

    tp = typeset_pages(fp.pages, page_of, bitmaps, xy, fill=(0, 0, 0), stroke=(255, 255, 255), radius=3)
    tp.pages[i]                                          # or TextDetector.typeset(fp.pages, lb, bitmaps, radius=3)

packs the bitmaps into one buffer, builds the tile table with numpy (`typeset_tables`: the touched 64 x 32 tiles of all pages
and, per tile, its layers in ascending order), uploads coverage and tables once, makes ONE `ctd_typeset` call
(csrc/kernels_typeset.hip: one launch, one workgroup per touched tile, the coverage patch of each layer in LDS) and downloads
one small table.  The rule is integers only and stated in include/ctd_hip.h (restated in numpy in tests/typeset_ref.py;
DESIGN.md section 4.21 has its limits): the outline S is the max of the coverage F over a disk of `radius` pixels, and a
pixel becomes blend(blend(page, stroke, S), fill, F) with blend(c, k, a) = (c (255 - a) + k a + 127) / 255; layers are applied
in the order given.  Glyph rasterisation is not done here (a font engine's job, or `glyphs.GlyphAtlas.rasterise`).  There is no per-layer Python beyond packing the bitmaps
and no CPU fallback: without a GPU it raises `CtdError` like the rest of the package.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import _lib as L
from .pagecall import Page, PageCall, check_pages, device_pages, table_dtype, views

__all__ = ["typeset_pages", "TypesetPages", "typeset_tables", "place", "PAGE_DTYPE", "LAYER_DTYPE", "TILE_DTYPE", "ROW_DTYPE",
           "tilt_tables", "TILT_LAYER_DTYPE"]

# numpy views of `ctd_typeset_page` / `_layer` / `_tile` / `_row` (include/ctd_hip.h)
PAGE_DTYPE = table_dtype(L.CtdTypesetPage)
LAYER_DTYPE = table_dtype(L.CtdTypesetLayer)
TILE_DTYPE = table_dtype(L.CtdTypesetTile)
ROW_DTYPE = table_dtype(L.CtdTypesetRow)

MAX_COORD = 1 << 29


def _ints(a, shape, what) -> np.ndarray:
    """`a` as an int64 array of `shape` (-1: any length); ValueError where it holds anything but whole numbers."""
    a = np.asarray(a)
    if a.dtype.kind not in "iu" and a.size:
        raise ValueError(f"{what}: integers")
    try:
        return a.astype(np.int64).reshape(shape)
    except ValueError:
        raise ValueError(f"{what}: expected shape {shape}") from None


def _per_layer(v, n, width, what) -> np.ndarray:
    """One value (of `width` numbers) for all layers or one per layer -> (n, width) int64."""
    a = np.asarray(v)
    if a.dtype.kind not in "iu" or a.dtype == bool:
        raise ValueError(f"{what}: integers")
    a = a.astype(np.int64)
    if a.shape == ((width,) if width > 1 else ()):
        return np.broadcast_to(a.reshape(1, width), (n, width)).copy()
    if a.shape in ((n, width),) + (((n,),) if width == 1 else ()):
        return a.reshape(n, width)
    raise ValueError(f"{what}: one value for all layers or one per layer")


def _layers(shapes: Sequence, page_of, radius, clip) -> tuple:
    """The per-layer arguments that `typeset_tables` and `glyphs.glyph_tables` share, checked: (H, W, page_of, r, clip) with
    H, W per page, the others per layer, all int64; the default clip is the layer's page."""
    H = _ints([s[0] for s in shapes], (-1,), "shapes")
    W = _ints([s[1] for s in shapes], (-1,), "shapes")
    if len(H) and (min(H.min(), W.min()) < 1 or max(H.max(), W.max()) > L.TYPESET_MAX_SIDE):
        raise ValueError(f"page sides must be 1 .. {L.TYPESET_MAX_SIDE}")
    page_of = _ints(page_of, (-1,), "page_of")
    n = len(page_of)
    r = _per_layer(radius, n, 1, "radius")[:, 0]
    if n and (page_of.min() < 0 or page_of.max() >= len(H)):
        raise ValueError("page_of: an index of `shapes`")
    if n and (r.min() < 0 or r.max() > L.TYPESET_MAX_RADIUS):
        raise ValueError(f"radius in 0 .. {L.TYPESET_MAX_RADIUS}")
    pw, ph = W[page_of], H[page_of]
    if clip is None:
        clip = np.stack([np.zeros_like(pw), np.zeros_like(ph), pw, ph], axis=1)
    clip = _per_layer(clip, n, 4, "clip")
    if n and (clip.min() < -2 ** 31 or clip.max() >= 2 ** 31):
        raise ValueError("clip beyond int32")
    return H, W, page_of, r, clip


def _rects(n: int, sizes, xy, r, clip, pw, ph, what: str) -> tuple:
    """n bitmaps of sizes[i] = (h, w) at xy[i], checked (`what` words the message), and the rectangle of each grown by
    r[i], cut to clip[i] and to its page of pw[i] x ph[i]: (sizes, xy, x1, y1, x2, y2); empty where x1 >= x2 or y1 >= y2."""
    sizes, xy = _ints(sizes, (n, 2), "sizes"), _ints(xy, (n, 2), "xy")
    if n and (sizes.min() < 0 or sizes.max() > L.TYPESET_MAX_SIDE):
        raise ValueError(f"{what} sides must be 0 .. {L.TYPESET_MAX_SIDE}")
    if n and np.abs(xy).max() > MAX_COORD:
        raise ValueError("xy beyond 2^29")
    x1 = np.maximum(np.maximum(xy[:, 0] - r, clip[:, 0]), 0)
    y1 = np.maximum(np.maximum(xy[:, 1] - r, clip[:, 1]), 0)
    x2 = np.minimum(np.minimum(xy[:, 0] + sizes[:, 1] + r, clip[:, 2]), pw)
    y2 = np.minimum(np.minimum(xy[:, 1] + sizes[:, 0] + r, clip[:, 3]), ph)
    return sizes, xy, x1, y1, x2, y2


def _bin_tiles(H, W, page_of_item, x1, y1, x2, y2, items) -> tuple:
    """The tile binner of both typeset calls: (tiles, entries).  `items` (ascending indices) lie on page page_of_item[i] of
    H[p] x W[p] pixels and cover the non-empty rectangle x1[i] .. y2[i], exclusive, within it.  tiles: `TILE_DTYPE`, every
    tile that an item's rectangle meets once, in page-major, row-major order, and a closing row whose `first` is the entry
    count; entries: int32, the items of each tile in ascending order."""
    tw, th = L.TYPESET_TILE_W, L.TYPESET_TILE_H
    tx1, ty1 = x1[items] // tw, y1[items] // th
    nx, ny = (x2[items] - 1) // tw + 1 - tx1, (y2[items] - 1) // th + 1 - ty1
    cnt = nx * ny
    total = int(cnt.sum())
    if total >= 2 ** 31:
        raise ValueError("too many tile entries for one call")
    k = np.arange(total, dtype=np.int64) - np.repeat(np.cumsum(cnt) - cnt, cnt)     # the entry's number within its item
    nxr = np.repeat(nx, cnt)
    tx, ty = np.repeat(tx1, cnt) + k % np.maximum(nxr, 1), np.repeat(ty1, cnt) + k // np.maximum(nxr, 1)
    item = np.repeat(items, cnt)
    pg = page_of_item[item]
    tiles_x = (W + tw - 1) // tw
    per_page = tiles_x * ((H + th - 1) // th)
    key = (np.cumsum(per_page) - per_page)[pg] + ty * tiles_x[pg] + tx
    order = np.argsort(key, kind="stable")                 # stable: the items of a tile stay in ascending order
    first = np.flatnonzero(np.diff(key[order], prepend=-1)) if total else np.zeros((0,), np.int64)
    tiles = np.zeros((len(first) + 1,), TILE_DTYPE)
    at = order[first]
    tiles["page"][:-1], tiles["tx"][:-1], tiles["ty"][:-1], tiles["first"][:-1] = pg[at], tx[at], ty[at], first
    tiles["first"][-1] = total
    return tiles, item[order].astype(np.int32)


# ---- tilted layers (include/ctd_hip.h, "tilted text") -------------------------------------------------------

TILT_LAYER_DTYPE = table_dtype(L.CtdTiltLayer)
TILT_MAX_COORD = 1 << 27                                   # |xy| and |pivot| of a tilted layer: the binner's products fit int64


def _tilt_args(angle, pivot, n: int):
    """The `angle` / `pivot` keywords of the typeset calls, checked: None where no layer is tilted (the call then runs as it
    always did), else (angle (n,) int64 degrees, pivot (n, 2) int64, cs (n, 2) int64 16.16 cosine and sine)."""
    if angle is None:
        if pivot is not None:
            raise ValueError("pivot: only with angle")
        return None
    angle = _per_layer(angle, n, 1, "angle")[:, 0]
    if n and (angle.min() < -180 or angle.max() > 180):
        raise ValueError("angle: -180 .. 180 degrees")
    pivot = _per_layer((0, 0) if pivot is None else pivot, n, 2, "pivot")
    if n and np.abs(pivot).max() > TILT_MAX_COORD:
        raise ValueError("pivot beyond 2^27")
    if not angle.any():
        return None
    from .balloons import cs_of                            # the one table of both calls (balloons imports nothing of this module)
    return angle, pivot, cs_of(angle)


def _tilt_rects(n: int, sizes, xy, r, clip, pw, ph, pivot, cs, what: str) -> tuple:
    """`_rects` for bitmaps in a frame: sizes[i] = (h, w) at FRAME position xy[i], frame pivot[i] and cs[i] = (c, s).  The
    page pixels whose four taps can touch the bitmap are those p with page -> frame (p) inside the bitmap's rectangle grown
    by one pixel to the left and up; d = p - pivot is the exact inverse image 65536 (c a - s b, s a + c b) / (c^2 + s^2) of
    (a, b) = frame point - pivot, linear, so its extremes lie at the rectangle's corners: floor of the least and ceiling of
    the greatest, in integers, then grown by r + 1, cut to clip[i] and the page."""
    sizes, xy = _ints(sizes, (n, 2), "sizes"), _ints(xy, (n, 2), "xy")
    if n and (sizes.min() < 0 or sizes.max() > L.TYPESET_MAX_SIDE):
        raise ValueError(f"{what} sides must be 0 .. {L.TYPESET_MAX_SIDE}")
    if n and np.abs(xy).max() > TILT_MAX_COORD:
        raise ValueError("xy of a tilted call beyond 2^27")
    c, s = cs[:, 0:1], cs[:, 1:2]
    N = (c * c + s * s)[:, 0]
    a = np.stack([xy[:, 0] - 1, xy[:, 0] + sizes[:, 1]], axis=1) - pivot[:, 0:1]
    b = np.stack([xy[:, 1] - 1, xy[:, 1] + sizes[:, 0]], axis=1) - pivot[:, 1:2]
    A, B = a[:, [0, 1, 0, 1]], b[:, [0, 0, 1, 1]]                             # the four corners
    numx, numy = 65536 * (c * A - s * B), 65536 * (s * A + c * B)
    lox, hix = numx.min(axis=1) // N, -((-numx.max(axis=1)) // N)
    loy, hiy = numy.min(axis=1) // N, -((-numy.max(axis=1)) // N)
    x1 = np.maximum(np.maximum(pivot[:, 0] + lox - r - 1, clip[:, 0]), 0)
    y1 = np.maximum(np.maximum(pivot[:, 1] + loy - r - 1, clip[:, 1]), 0)
    x2 = np.minimum(np.minimum(pivot[:, 0] + hix + r + 2, clip[:, 2]), pw)
    y2 = np.minimum(np.minimum(pivot[:, 1] + hiy + r + 2, clip[:, 3]), ph)
    return sizes, xy, x1, y1, x2, y2


def tilt_tables(shapes: Sequence, page_of, layer_of, sizes, xy, radius, clip, pivot, cs) -> tuple:
    """`glyphs.glyph_tables` for tilted layers: (tiles, entries, status).  pivot (n_layers, 2) and cs (n_layers, 2) give
    every layer's frame; xy[i] is placement i's FRAME position.  A placement is entered in every tile that the conservative
    page box of `_tilt_rects` meets; OUTSIDE means that box is empty.  For a bitmap call layer_of is arange(n).  Numpy only."""
    H, W, page_of, r, clip = _layers(shapes, page_of, radius, clip)
    nl = len(page_of)
    layer_of = _ints(layer_of, (-1,), "layer_of")
    n = len(layer_of)
    if n and (layer_of.min() < 0 or layer_of.max() >= nl):
        raise ValueError("layer_of: an index of the layers")
    if n and (np.diff(layer_of) < 0).any():
        raise ValueError("layer_of must be non-decreasing: the placements of a layer are consecutive")
    pg = page_of[layer_of]
    sizes, xy, x1, y1, x2, y2 = _tilt_rects(n, sizes, xy, r[layer_of], clip[layer_of], W[pg], H[pg], pivot[layer_of], cs[layer_of],
                                            "glyph")
    inked = (sizes[:, 0] > 0) & (sizes[:, 1] > 0)
    drawn = inked & (x1 < x2) & (y1 < y2)
    n_inked, n_drawn = np.bincount(layer_of[inked], minlength=nl), np.bincount(layer_of[drawn], minlength=nl)
    status = np.where(n_inked == 0, L.TYPESET_EMPTY, np.where(n_drawn == 0, L.TYPESET_OUTSIDE, L.TYPESET_OK)).astype(np.int32)
    return _bin_tiles(H, W, pg, x1, y1, x2, y2, np.flatnonzero(drawn)) + (status,)


def _tilt_layer_table(page_of, clip4, fill, stroke, r, pivot, cs) -> np.ndarray:
    lt = np.zeros((len(page_of),), TILT_LAYER_DTYPE)
    lt["page"], lt["clip"], lt["fill"], lt["stroke"], lt["radius"] = page_of, clip4, fill, stroke, r
    lt["ax"], lt["ay"], lt["c"], lt["s"] = pivot[:, 0], pivot[:, 1], cs[:, 0], cs[:, 1]
    return lt


def _place_table(layer_of, glyph, xy) -> np.ndarray:
    qt = np.zeros((len(layer_of),), table_dtype(L.CtdGlyphPlace))
    qt["layer"], qt["glyph"], qt["x"], qt["y"] = layer_of, glyph, xy[:, 0], xy[:, 1]
    return qt


def typeset_tables(shapes: Sequence, page_of, sizes, xy, radius=0, clip=None) -> tuple:
    """The tile table and the entry list of a typeset call: (tiles, entries, status).  shapes[p] = (H, W) of page p; per
    layer page_of[i], sizes[i] = (h, w) of its bitmap, xy[i] = (x0, y0) of the bitmap's top-left pixel in page coordinates,
    radius (one for all or one per layer), clip[i] = (x1, y1, x2, y2) exclusive (one for all, one per layer, default: the
    page).  A layer is entered in every tile that its rectangle grown by its radius, cut to the page and the clip, meets.
    tiles: `TILE_DTYPE`, n_tiles + 1 rows, every touched tile once in page-major, row-major order, the last row's `first` the
    entry count.  entries: int32 layer indices, ascending within a tile.  status[i], the first that applies:
    `_lib.TYPESET_EMPTY` (w or h is 0), `TYPESET_OUTSIDE` (that rectangle is empty), `TYPESET_OK`.  Numpy only."""
    H, W, page_of, r, clip = _layers(shapes, page_of, radius, clip)
    sizes, xy, x1, y1, x2, y2 = _rects(len(page_of), sizes, xy, r, clip, W[page_of], H[page_of], "bitmap")
    status = np.where((sizes[:, 0] == 0) | (sizes[:, 1] == 0), L.TYPESET_EMPTY,
                      np.where((x1 >= x2) | (y1 >= y2), L.TYPESET_OUTSIDE, L.TYPESET_OK)).astype(np.int32)
    return _bin_tiles(H, W, page_of, x1, y1, x2, y2, np.flatnonzero(status == L.TYPESET_OK)) + (status,)


def place(rects, sizes, radius=0) -> tuple:
    """Bitmaps of sizes[i] = (h, w) centred in rects[i] = (x1, y1, x2, y2), exclusive: (xy, fits) with xy[i] = (x0, y0),
    x0 = x1 + ((x2 - x1 - w) >> 1) and likewise y0 (the odd pixel of slack goes right and down; a bitmap larger than its box
    overhangs it evenly), and fits[i] where the bitmap plus 2 radius fits the rectangle both ways.  Numpy."""
    rects = _ints(rects, (-1, 4), "rects")
    n = len(rects)
    sizes = _ints(sizes, (n, 2), "sizes")
    r = _per_layer(radius, n, 1, "radius")[:, 0]
    bw, bh = rects[:, 2] - rects[:, 0], rects[:, 3] - rects[:, 1]
    xy = np.stack([rects[:, 0] + ((bw - sizes[:, 1]) >> 1), rects[:, 1] + ((bh - sizes[:, 0]) >> 1)], axis=1)
    return xy, (sizes[:, 1] + 2 * r <= bw) & (sizes[:, 0] + 2 * r <= bh)


class TypesetPages:
    """The result of `typeset_pages`.  `pages[i]` (H,W,3) u8 in the page's channel order, on the device: views of ONE new
    allocation, or the caller's own pages where `inplace` was set.  Per layer: `rows` the kernel's records (`ROW_DTYPE`),
    `n_fill[i]` the pixels written with coverage above 0, `n_stroke[i]` those written with outline above 0, `status[i]` =
    `_lib.TYPESET_OK` / `TYPESET_EMPTY` (a bitmap without pixels) / `TYPESET_OUTSIDE` (nothing of it on the page and in the
    clip), `xy[i]` where the bitmap went.  `TextDetector.typeset` adds `layer_of[j]`, block j's layer or -1, and `fits[i]`."""

    def __init__(self, pages: List[torch.Tensor], rows: np.ndarray, status: np.ndarray, xy: np.ndarray):
        self.pages, self.rows, self.status, self.xy = pages, rows, status, xy
        if len(rows) != len(status) or len(xy) != len(rows):
            raise ValueError("one row, one status and one position per layer")
        self.n_fill, self.n_stroke = rows["n_fill"], rows["n_stroke"]
        self.layer_of = self.fits = None

    def __len__(self) -> int:
        return len(self.rows)

    def to_host(self):
        """The pages as a list of numpy arrays."""
        return [p.cpu().numpy() for p in self.pages]

    def __repr__(self) -> str:
        return f"TypesetPages({len(self.pages)} pages, {len(self)} layers, {int((self.status == L.TYPESET_OK).sum())} drawn)"


def _dense(t) -> bool:
    return t.stride(2) == 1 and t.stride(1) == 3 and t.stride(0) >= 3 * t.shape[1]


def _copies(pages, device):
    """The pages copied into views of ONE new allocation, each on a 256-byte boundary: one device copy where they already lie
    like that in one buffer (as `FilledPages.pages` do), else one copy (or upload) a page."""
    store, out = views([(int(p.shape[0]), int(p.shape[1]), 3) for p in pages], device)
    dev = [p for p in pages if isinstance(p, torch.Tensor) and p.device == device and p.is_contiguous()]
    if len(dev) == len(pages) and all(p.untyped_storage().data_ptr() == dev[0].untyped_storage().data_ptr() and
                                      p.data_ptr() - dev[0].data_ptr() == o.data_ptr() - out[0].data_ptr() for p, o in zip(dev, out)):
        used = out[-1].data_ptr() - out[0].data_ptr() + out[-1].numel()
        src = torch.empty((0,), dtype=torch.uint8, device=device).set_(dev[0].untyped_storage(), dev[0].storage_offset(), (used,))
        store[:used].copy_(src)
    else:
        for o, p in zip(out, pages):
            o.copy_(p if isinstance(p, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(p)))
    return out


def _layer_args(pages, page_of, fill, stroke, radius, inplace: bool) -> tuple:
    """What `typeset_pages` and `glyphs.typeset_glyphs` check first, ValueError where it is wrong: the pages, the per-layer
    columns -> (shapes, page_of, fill (n, 3) BGR, stroke (n, 3) BGR, r)."""
    check_pages(pages, nonempty=False)                    # an empty page is the tables' "page sides" error
    if inplace and not all(isinstance(p, torch.Tensor) and p.is_cuda and _dense(p) for p in pages):
        raise ValueError("inplace=True needs device pages with dense rows")
    shapes = [tuple(int(v) for v in p.shape[:2]) for p in pages]
    page_of = _ints(page_of, (-1,), "page_of")
    n = len(page_of)
    colours = []
    for name, v in (("fill", fill), ("stroke", stroke)):
        c = _per_layer(v, n, 3, name)
        if n and (c.min() < 0 or c.max() > 255):
            raise ValueError(f"{name}: 0 .. 255")
        colours.append(c[:, ::-1])
    return shapes, page_of, colours[0], colours[1], _per_layer(radius, n, 1, "radius")[:, 0]


def _open_pages(pc: PageCall, pages, shapes, page_of, clip, inplace: bool) -> tuple:
    """Behind the tables, which have checked `page_of` and `clip`, inside the call's `PageCall`: (out, pt, clip4).
    out: the pages the kernel writes, the caller's own where `inplace`, else copies (views of one new allocation); pt:
    their `ctd_typeset_page` table; clip4: the clip of every layer, (n, 4), the page where none was given."""
    n = len(page_of)
    clip4 = _per_layer(clip, n, 4, "clip") if clip is not None else np.array([(0, 0, shapes[p][1], shapes[p][0]) for p in page_of],
                                                                            np.int64).reshape(n, 4)
    if not pages:
        out = []
    elif inplace:
        out = device_pages(pages, pc.device, pc.what)[0]       # the caller's own tensors (checked below): nothing to keep
        if any(o.data_ptr() != p.data_ptr() for o, p in zip(out, pages)):
            raise ValueError("inplace=True needs pages on the device the call runs on")
    else:
        out = _copies(pages, pc.device)
    pt = np.zeros((len(out),), PAGE_DTYPE)
    pt["page_dev"] = [o.data_ptr() for o in out]
    pt["H"], pt["W"], pt["pitch"] = [s[0] for s in shapes], [s[1] for s in shapes], [o.stride(0) for o in out]
    return out, pt, clip4


def typeset_pages(pages: Sequence[Page], page_of, bitmaps: Sequence[np.ndarray], xy, fill=(0, 0, 0), stroke=(255, 255, 255),
                  radius=0, clip=None, inplace: bool = False, stream: Optional[torch.cuda.Stream] = None,
                  device=None, angle=None, pivot=None) -> TypesetPages:
    """Composite layers into the pages of a batch by the typeset rule: one upload of coverage and tables, one `ctd_typeset`
    launch, one small download.  pages: uint8 (H,W,3) pages of any mix of sizes, on the device or on the host; per layer
    page_of[i], bitmaps[i] a (h, w) uint8 numpy array of coverage, xy[i] = (x0, y0) of its top-left pixel in page
    coordinates; fill / stroke: RGB, one triple for all layers or one per layer (reversed into the pages' BGR order); radius:
    the outline's, 0 .. 12, one for all or one per layer; clip: (x1, y1, x2, y2) exclusive, one for all or one per layer,
    default the page.  Layers are applied in the order given.  inplace=False composites into a copy, views of one new
    allocation; inplace=True writes the given pages, which must then be device tensors with dense rows (any row pitch).
    Bad arguments raise ValueError before anything is uploaded.  Runs on `stream` (default: the current stream of the pages'
    device) and waits for the result; see `TypesetPages`.
    angle, pivot: per layer (one for all or one per layer) the whole degrees, -180 .. 180, and the page pixel (x, y; default
    (0, 0)) of the layer's frame; xy[i] is then the bitmap's position in that FRAME, and the bitmap is turned about the pivot
    into the page (include/ctd_hip.h, "tilted text": resampled by four taps, the outline a page-space disk).  The launch is
    then `ctd_typeset_tilted`'s: each bitmap is the one glyph of its layer, the packed coverage is the atlas and the record
    table is built here.  Where no layer has a non-zero angle the call is the one above, exactly."""
    shapes, page_of, fill, stroke, r = _layer_args(pages, page_of, fill, stroke, radius, inplace)
    n = len(page_of)
    tilt = _tilt_args(angle, pivot, n)
    if len(bitmaps) != n:
        raise ValueError("one bitmap per layer")
    for b in bitmaps:
        if not isinstance(b, np.ndarray) or b.dtype != np.uint8 or b.ndim != 2:
            raise ValueError("a bitmap is a (h, w) uint8 numpy array")
    sizes = np.array([b.shape for b in bitmaps], np.int64).reshape(n, 2)
    xy = _ints(xy, (n, 2), "xy")
    if tilt is None:
        tiles, entries, status = typeset_tables(shapes, page_of, sizes, xy, r, clip)
    else:
        tiles, entries, status = tilt_tables(shapes, page_of, np.arange(n), sizes, xy, r, clip, tilt[1], tilt[2])
    area = sizes[:, 0] * sizes[:, 1]
    cov0 = np.cumsum(area) - area
    cov = np.concatenate([b.ravel() for b in bitmaps]) if n else np.zeros((0,), np.uint8)
    n_pages, n_tiles = len(pages), len(tiles) - 1
    with PageCall("typesetting runs", pages, stream, device) as pc:
        out, pt, clip4 = _open_pages(pc, pages, shapes, page_of, clip, inplace)
        rows = np.zeros((n,), ROW_DTYPE)
        if tilt is not None and n_tiles:
            rec = np.zeros((n,), table_dtype(L.CtdGlyphRecord))
            rec["off"], rec["w"], rec["h"] = cov0, sizes[:, 1], sizes[:, 0]
            lt = _tilt_layer_table(page_of, clip4, fill, stroke, r, tilt[1], tilt[2])
            # one upload: the tables, the records made here, and the coverage as the atlas
            _, ptr = pc.upload([pt, lt, _place_table(np.arange(n), np.arange(n), xy), rec, tiles, entries, cov])
            rows_dev = torch.empty((n * ROW_DTYPE.itemsize,), dtype=torch.uint8, device=pc.device)
            prm = L.CtdGlyphParams(n, n_pages, n_tiles, len(entries), n, n, len(cov))
            L.check(L.lib().ctd_typeset_tilted(ptr[0], ptr[1], ptr[2], ptr[3], ptr[4], ptr[5], ptr[6] if len(cov) else None,
                                               C.byref(prm), rows_dev.data_ptr(), pc.st.cuda_stream), "ctd_typeset_tilted")
            rows = pc.rows(rows_dev, ROW_DTYPE, n)
        elif tilt is None and n and n_pages:
            lt = np.zeros((n,), LAYER_DTYPE)
            lt["cov0"], lt["page"], lt["x0"], lt["y0"], lt["h"], lt["w"] = cov0, page_of, xy[:, 0], xy[:, 1], sizes[:, 0], sizes[:, 1]
            lt["cov_pitch"], lt["clip"], lt["fill"], lt["stroke"], lt["radius"] = sizes[:, 1], clip4, fill, stroke, r
            _, ptr = pc.upload([pt, lt, tiles, entries, cov])   # one upload: the four tables and the coverage
            rows_dev = torch.empty((n * ROW_DTYPE.itemsize,), dtype=torch.uint8, device=pc.device)
            prm = L.CtdTypesetParams(n, n_pages, n_tiles, len(entries), len(cov), 0)
            L.check(L.lib().ctd_typeset(ptr[0], ptr[1], ptr[2], ptr[3] if len(entries) else None, ptr[4] if len(cov) else None,
                                        C.byref(prm), rows_dev.data_ptr(), pc.st.cuda_stream), "ctd_typeset")
            rows = pc.rows(rows_dev, ROW_DTYPE, n)
    return TypesetPages(out, rows, status, xy)
