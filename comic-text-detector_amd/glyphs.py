"""Typeset from a glyph atlas: glyph runs composited into pages, on the GPU.

`typeset.typeset_pages` takes one coverage bitmap per block; a font engine (FreeType, PIL's `font.getmask`, HarfBuzz plus a
rasteriser) gives one bitmap per GLYPH plus metrics.  Here each distinct glyph is rasterised once, by any engine, into an atlas
that stays on the device across pages, and a call sends only a table of placements, 16 bytes a glyph:

    atlas = GlyphAtlas()
    ids = atlas.add(bitmaps, advance=adv)                  # once per distinct glyph; ids are stable
    xy, fits = flow(run, atlas, rect)                      # where a block's glyph run goes in its box (numpy)
    tp = typeset_glyphs(fp.pages, atlas, page_of, layer_of, glyph, xy, fill=(0, 0, 0), stroke=(255, 255, 255), radius=3)
    tp.pages[i]                                            # or TextDetector.typeset_glyphs(fp.pages, lb, atlas, runs, radius=3)

A layer is a page, two colours, an outline radius and a clip, plus a run of placements (layer, glyph, x, y); its coverage is the
MAX over its placements of the glyph coverage, and from there on the rule is `typeset`'s, unchanged (include/ctd_hip.h;
restated in tests/glyph_ref.py): by definition the result is what `typeset_pages` gives for the
block bitmap that the max-paste of the glyphs produces.  `glyph_tables` builds the tile table with numpy (the touched 64 x 32
tiles and, per tile, its placements in ascending order), tables and placements go up in ONE upload, ONE `ctd_typeset_glyphs`
launch (csrc/kernels_glyphs.hip) assembles each layer's coverage on chip, one small download.  No CPU fallback: without a
GPU `GlyphAtlas` and `typeset_glyphs` raise `CtdError` like the rest of the package.

What this is not: no kerning, no shaping (ligatures, bidi, contextual forms), no hyphenation, no font-size search and no
rasterisation.  `flow` is a greedy breaker on integer advances; anything smarter computes `xy` itself and calls
`typeset_glyphs`.  Overlapping glyphs of a layer combine by max, not by sum; a layer has one colour, so a coloured word is a
layer of its own.
"""
from __future__ import annotations

import contextlib
import ctypes as C
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib as L
from .regions import Page
from .typeset import (MAX_COORD, ROW_DTYPE, TILE_DTYPE, TypesetPages, _bin_tiles, _ints, _layer_args, _layers, _open_pages, _pack,
                      _rects)

__all__ = ["GlyphAtlas", "glyph_tables", "typeset_glyphs", "flow", "LAYER_DTYPE", "PLACE_DTYPE", "RECORD_DTYPE"]

# numpy views of `ctd_glyph_layer` / `_place` / `_record` (include/ctd_hip.h; the _lib.CtdGlyph* mirrors)
LAYER_DTYPE = np.dtype([("page", "<i4"), ("clip", "<i4", (4,)), ("fill", "u1", (3,)), ("stroke", "u1", (3,)), ("radius", "u1"),
                        ("pad_", "u1"), ("pad2_", "<i4")])
PLACE_DTYPE = np.dtype([("layer", "<i4"), ("glyph", "<i4"), ("x", "<i4"), ("y", "<i4")])
RECORD_DTYPE = np.dtype([("off", "<i8"), ("w", "<i4"), ("h", "<i4")])
assert LAYER_DTYPE.itemsize == C.sizeof(L.CtdGlyphLayer) == 32
assert PLACE_DTYPE.itemsize == C.sizeof(L.CtdGlyphPlace) == 16
assert RECORD_DTYPE.itemsize == C.sizeof(L.CtdGlyphRecord) == 16
assert C.sizeof(L.CtdGlyphParams) == 32


class GlyphAtlas:
    """Glyph coverage on the device, kept across calls.  `add(bitmaps, advance=None, bearing=None)` appends (h, w) uint8
    arrays (zero-sized ones are legal: a space) and returns their int32 ids, which never change.  The coverage lives in ONE
    device buffer of dense rows, grown by doubling with a device copy, so only the appended bytes are ever uploaded; the record
    table (`RECORD_DTYPE`: off, w, h) is kept on the device beside it and on the host as `sizes[i] = (h, w)` and `offsets[i]`.
    `advance[i] = (ax, ay)` (default (w, h)) and `bearing[i] = (bx, by)` (default 0) are host-side integer metrics that only
    `flow` reads.  `len(atlas)` glyphs, `nbytes` of coverage; `close()` frees the device buffers."""

    def __init__(self, device=None):
        if not torch.cuda.is_available():
            raise L.CtdError("the glyph atlas lives on the GPU and there is none (no CPU fallback)")
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.sizes = np.zeros((0, 2), np.int64)
        self.offsets = np.zeros((0,), np.int64)
        self.advance = np.zeros((0, 2), np.int64)
        self.bearing = np.zeros((0, 2), np.int64)
        self.nbytes = 0
        self._cov = torch.empty((4096,), dtype=torch.uint8, device=self.device)
        self._rec = torch.empty((256 * RECORD_DTYPE.itemsize,), dtype=torch.uint8, device=self.device)

    def __len__(self) -> int:
        return len(self.offsets)

    @staticmethod
    def _grown(buf, used, need):
        """`buf` with room for `need` bytes: itself, or a buffer of twice the size (or more) holding its first `used` bytes."""
        if need <= buf.numel():
            return buf
        cap = buf.numel()
        while cap < need:
            cap *= 2
        new = torch.empty((cap,), dtype=torch.uint8, device=buf.device)
        new[:used].copy_(buf[:used])
        return new

    def add(self, bitmaps: Sequence[np.ndarray], advance=None, bearing=None) -> np.ndarray:
        if self._cov is None:
            raise L.CtdError("the atlas is closed")
        for b in bitmaps:
            if not isinstance(b, np.ndarray) or b.dtype != np.uint8 or b.ndim != 2:
                raise ValueError("a glyph is a (h, w) uint8 numpy array")
        k = len(bitmaps)
        sizes = np.array([b.shape for b in bitmaps], np.int64).reshape(k, 2)
        if k and sizes.max() > L.TYPESET_MAX_SIDE:
            raise ValueError(f"glyph sides must be 0 .. {L.TYPESET_MAX_SIDE}")
        advance = sizes[:, ::-1].copy() if advance is None else _ints(advance, (k, 2), "advance")
        bearing = np.zeros((k, 2), np.int64) if bearing is None else _ints(bearing, (k, 2), "bearing")
        if k and max(np.abs(advance).max(), np.abs(bearing).max()) > MAX_COORD:
            raise ValueError("advance / bearing beyond 2^29")
        area = sizes[:, 0] * sizes[:, 1]
        off = self.nbytes + np.cumsum(area) - area
        n0, total = len(self), int(area.sum())
        if n0 + k >= 2 ** 31:
            raise ValueError("too many glyphs")
        rec = np.zeros((k,), RECORD_DTYPE)
        rec["off"], rec["h"], rec["w"] = off, sizes[:, 0], sizes[:, 1]
        with torch.cuda.device(self.device):
            self._cov = self._grown(self._cov, self.nbytes, self.nbytes + total)
            self._rec = self._grown(self._rec, n0 * RECORD_DTYPE.itemsize, (n0 + k) * RECORD_DTYPE.itemsize)
            if total:
                new = np.concatenate([b.ravel() for b in bitmaps])
                self._cov[self.nbytes: self.nbytes + total].copy_(torch.from_numpy(new))
            if k:
                self._rec[n0 * RECORD_DTYPE.itemsize: (n0 + k) * RECORD_DTYPE.itemsize].copy_(torch.from_numpy(rec.view(np.uint8).copy()))
        self.sizes, self.offsets = np.concatenate([self.sizes, sizes]), np.concatenate([self.offsets, off])
        self.advance, self.bearing = np.concatenate([self.advance, advance]), np.concatenate([self.bearing, bearing])
        self.nbytes += total
        torch.cuda.current_stream(self.device).synchronize()                # a later call may run on any stream
        return np.arange(n0, n0 + k, dtype=np.int32)

    def close(self) -> None:
        self._cov = self._rec = None

    def __repr__(self) -> str:
        return f"GlyphAtlas({len(self)} glyphs, {self.nbytes} bytes on {self.device})"


def glyph_tables(shapes: Sequence, page_of, layer_of, sizes, xy, radius=0, clip=None) -> tuple:
    """The tile table and the entry list of a `typeset_glyphs` call: (tiles, entries, status).  shapes[p] = (H, W) of page p;
    per LAYER page_of[l], radius (one for all or one per layer) and clip[l] = (x1, y1, x2, y2) exclusive (one for all, one
    per layer, default: the page); per PLACEMENT layer_of[i] (non-decreasing, else ValueError), sizes[i] = (h, w) of its
    glyph and xy[i] = (x, y) of the glyph's top-left pixel in page coordinates.  A placement whose glyph has pixels is entered
    in every tile that its rectangle grown by its layer's radius, cut to the page and the clip, meets.  tiles: `TILE_DTYPE`,
    n_tiles + 1 rows, every touched tile once in page-major, row-major order, the last row's `first` the entry count.
    entries: int32 placement indices, ascending within a tile, so the placements of a layer are consecutive.  status[l], the
    first that applies: `_lib.TYPESET_EMPTY` (no placement has a glyph with pixels), `TYPESET_OUTSIDE` (no such placement's
    rectangle grown by r meets page and clip), `TYPESET_OK`.  Numpy only."""
    H, W, page_of, r, clip = _layers(shapes, page_of, radius, clip)
    nl = len(page_of)
    layer_of = _ints(layer_of, (-1,), "layer_of")
    n = len(layer_of)
    if n and (layer_of.min() < 0 or layer_of.max() >= nl):
        raise ValueError("layer_of: an index of the layers")
    if n and (np.diff(layer_of) < 0).any():
        raise ValueError("layer_of must be non-decreasing: the placements of a layer are consecutive")
    pg = page_of[layer_of]
    sizes, xy, x1, y1, x2, y2 = _rects(n, sizes, xy, r[layer_of], clip[layer_of], W[pg], H[pg], "glyph")
    inked = (sizes[:, 0] > 0) & (sizes[:, 1] > 0)
    drawn = inked & (x1 < x2) & (y1 < y2)
    n_inked, n_drawn = np.bincount(layer_of[inked], minlength=nl), np.bincount(layer_of[drawn], minlength=nl)
    status = np.where(n_inked == 0, L.TYPESET_EMPTY, np.where(n_drawn == 0, L.TYPESET_OUTSIDE, L.TYPESET_OK)).astype(np.int32)
    return _bin_tiles(H, W, pg, x1, y1, x2, y2, np.flatnonzero(drawn)) + (status,)


def flow(ids, atlas, rect, line: Optional[int] = None, gap: int = 0, vertical: bool = False, breaks=None,
         align: str = "center") -> tuple:
    """One block's glyph run `ids` placed in the box rect = (x1, y1, x2, y2), exclusive: (xy, fits), xy[i] the top-left pixel
    of glyph i.  Greedy, integers, numpy.  `atlas` gives `sizes`, `advance` and `bearing` (a `GlyphAtlas` or anything with
    those three arrays).
    Horizontal: the pen starts at the line's left and adds advance[:, 0] per glyph; a line ends before the first glyph whose
    advance would pass the box's width (a glyph wider than the box stands alone on its line).  With `breaks` (bool per glyph:
    a line may end after this one) the line ends at the last allowed break before that glyph, and there where none is
    allowed (a hard break); the default allows a break everywhere, which is right for CJK.  Lines are `line` pixels high
    (default: the run's tallest glyph) and `gap` apart.  `align` shifts each line by its slack: "left" 0, "center"
    slack >> 1, "right" all of it.  The stack of lines is centred vertically as `typeset.place` centres a bitmap (slack >> 1,
    a stack taller than the box overhangs it evenly).  A glyph goes to (pen + bearing_x, line_top + bearing_y).
    vertical=True: the same with the axes swapped.  Columns of width `line` (default: the run's widest glyph), `gap` apart,
    run from right to left, the first one rightmost; the stack of columns is centred horizontally; the pen runs down by
    advance[:, 1]; `align` shifts a column down by its slack ("left" is the top); a glyph is centred in its column:
    (col_left + ((line - w) >> 1) + bearing_x, pen + bearing_y).
    `fits` is True where no line or column passes the box: every line's advances fit its length, and the stack fits across."""
    if align not in ("left", "center", "right"):
        raise ValueError('align: "left", "center" or "right"')
    ids = _ints(ids, (-1,), "ids")
    n = len(ids)
    x1, y1, x2, y2 = (int(v) for v in _ints(rect, (4,), "rect"))
    if n and (ids.min() < 0 or ids.max() >= len(atlas.sizes)):
        raise ValueError("ids: glyphs of the atlas")
    sizes, adv2, bear = np.asarray(atlas.sizes)[ids], np.asarray(atlas.advance)[ids], np.asarray(atlas.bearing)[ids]
    adv = adv2[:, 1 if vertical else 0].astype(np.int64)
    if n and adv.min() < 0:
        raise ValueError("advances must not be negative")
    if line is None:
        line = int(sizes[:, 1 if vertical else 0].max()) if n else 0
    line, gap = int(line), int(gap)
    if line < 0:
        raise ValueError("line: not negative")
    if breaks is not None:
        breaks = np.asarray(breaks)
        if breaks.dtype != bool or breaks.shape != (n,):
            raise ValueError("breaks: one bool per glyph")
    along, across = (y2 - y1, x2 - x1) if vertical else (x2 - x1, y2 - y1)
    cum = np.concatenate([[0], np.cumsum(adv)])
    allowed = None if breaks is None else np.flatnonzero(breaks)
    starts = []
    s = 0
    while s < n:                                           # one step a LINE, not a glyph
        end = int(np.searchsorted(cum, cum[s] + along, side="right")) - 1
        end = min(max(end, s + 1), n)
        if end < n and allowed is not None:
            k = int(np.searchsorted(allowed, end - 1, side="right")) - 1     # the last allowed break in s .. end - 1
            if k >= 0 and allowed[k] >= s:
                end = int(allowed[k]) + 1
        starts.append(s)
        s = end
    starts = np.array(starts, np.int64)
    n_lines = len(starts)
    ends = np.concatenate([starts[1:], [n]]).astype(np.int64)
    length = cum[ends] - cum[starts]
    slack = along - length
    shift = {"left": np.zeros_like(slack), "center": slack >> 1, "right": slack}[align]
    of = np.repeat(np.arange(n_lines), ends - starts)      # the glyph's line
    pen = (cum[:-1] - cum[starts][of]) + shift[of]
    total = n_lines * line + max(n_lines - 1, 0) * gap
    lead = (across - total) >> 1
    if vertical:
        col_left = x1 + lead + total - line - of * (line + gap)
        xy = np.stack([col_left + ((line - sizes[:, 1]) >> 1) + bear[:, 0], y1 + pen + bear[:, 1]], axis=1)
    else:
        xy = np.stack([x1 + pen + bear[:, 0], y1 + lead + of * (line + gap) + bear[:, 1]], axis=1)
    fits = bool((length <= along).all() and total <= across)
    return xy.astype(np.int64).reshape(n, 2), fits


def typeset_glyphs(pages: Sequence[Page], atlas: GlyphAtlas, page_of, layer_of, glyph, xy, fill=(0, 0, 0),
                   stroke=(255, 255, 255), radius=0, clip=None, inplace: bool = False,
                   stream: Optional[torch.cuda.Stream] = None, device=None) -> TypesetPages:
    """Composite glyph layers into the pages of a batch: one upload of tables and placements, one `ctd_typeset_glyphs`
    launch, one small download.  pages: as `typeset.typeset_pages`.  Per LAYER: page_of[l]; fill / stroke (RGB, one triple for
    all or one per layer); radius 0 .. 12 and clip (x1, y1, x2, y2) exclusive (one for all or one per layer; default the
    page).  Per PLACEMENT: layer_of[i] (non-decreasing), glyph[i] an id of `atlas`, xy[i] = (x, y) of the glyph's top-left
    pixel in page coordinates.  A layer's coverage is the max over its placements; layers are applied in order.  `inplace`
    as in `typeset_pages`.  Bad arguments raise ValueError before anything is uploaded.  Runs on `stream` (default: the
    current stream of the atlas's device) and waits for the result: a `TypesetPages` with one row and one status per
    LAYER, whose `xy` is per PLACEMENT and which also carries `place_layer` (= layer_of) and `place_glyph`."""
    shapes, page_of, fill, stroke, r = _layer_args(pages, page_of, fill, stroke, radius, inplace)
    nl = len(page_of)
    layer_of = _ints(layer_of, (-1,), "layer_of")
    n = len(layer_of)
    glyph, xy = _ints(glyph, (n,), "glyph"), _ints(xy, (n, 2), "xy")
    if not isinstance(atlas, GlyphAtlas) or atlas._cov is None:
        raise ValueError("atlas: an open GlyphAtlas")
    if n and (glyph.min() < 0 or glyph.max() >= len(atlas)):
        raise ValueError("glyph: an id of the atlas")
    tiles, entries, status = glyph_tables(shapes, page_of, layer_of, atlas.sizes[glyph], xy, r, clip)
    n_pages, n_tiles = len(pages), len(tiles) - 1
    device = atlas.device if device is None else torch.device(device)
    if device != atlas.device:
        raise ValueError("the atlas lives on another device")
    with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
        with torch.cuda.device(device):
            st = torch.cuda.current_stream(device)
            out, pt, clip4 = _open_pages(pages, shapes, page_of, clip, inplace, device)
            rows = np.zeros((nl,), ROW_DTYPE)
            if n_tiles:
                lt = np.zeros((nl,), LAYER_DTYPE)
                lt["page"], lt["clip"], lt["fill"], lt["stroke"], lt["radius"] = page_of, clip4, fill, stroke, r
                qt = np.zeros((n,), PLACE_DTYPE)
                qt["layer"], qt["glyph"], qt["x"], qt["y"] = layer_of, glyph, xy[:, 0], xy[:, 1]
                blob, at = _pack([pt, lt, qt, tiles, entries])     # one upload: the tables and the placements
                tab = torch.from_numpy(blob).to(device)
                rows_dev = torch.empty((nl * ROW_DTYPE.itemsize,), dtype=torch.uint8, device=device)
                prm = L.CtdGlyphParams(nl, n_pages, n_tiles, len(entries), n, len(atlas), atlas.nbytes)
                ptr = [tab.data_ptr() + int(a) for a in at]
                L.check(L.lib().ctd_typeset_glyphs(ptr[0], ptr[1], ptr[2], atlas._rec.data_ptr(), ptr[3], ptr[4],
                                                   atlas._cov.data_ptr(), C.byref(prm), rows_dev.data_ptr(), st.cuda_stream),
                        "ctd_typeset_glyphs")
                rows = rows_dev.cpu().numpy().view(ROW_DTYPE)           # stream-ordered: behind the launch
            st.synchronize()
    tp = TypesetPages(out, rows, status, np.zeros((nl, 2), np.int64))
    tp.xy, tp.place_layer, tp.place_glyph = xy, layer_of, glyph             # per placement here, not per layer
    return tp
