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

Where the glyphs come from outlines, the atlas fills itself: `OutlineFont` keeps quadratic outlines on the device,
`atlas.rasterise(font, gids, size)` rasterises every (glyph, size) instance it does not hold yet straight into its buffer in ONE
`ctd_rasterise_glyphs` launch (csrc/kernels_raster.hip; an unhinted integer rule, include/ctd_hip.h, tests/raster_ref.py,
DESIGN.md section 4.25), and `fit` picks the largest size whose flow fits a box, on the host, from metrics only.

What this is not: no kerning, no shaping (ligatures, bidi, contextual forms), no hyphenation, no hinting and no cubic
outlines.  `flow` is a greedy breaker on integer advances; anything smarter computes `xy` itself and calls
`typeset_glyphs`.  Overlapping glyphs of a layer combine by max, not by sum; a layer has one colour, so a coloured word is a
layer of its own.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib as L
from .pagecall import Page, PageCall, need_gpu, table_dtype
from .typeset import (MAX_COORD, ROW_DTYPE, TILE_DTYPE, TypesetPages, _bin_tiles, _ints, _layer_args, _layers, _open_pages, _rects,
                      _tilt_args, _tilt_layer_table, tilt_tables)

__all__ = ["GlyphAtlas", "glyph_tables", "typeset_glyphs", "flow", "place_lines", "LAYER_DTYPE", "PLACE_DTYPE", "RECORD_DTYPE", "OutlineFont",
           "segments_from_ops", "outline_boxes", "flow_outlines", "fit", "RASTER_JOB_DTYPE"]

# numpy views of `ctd_glyph_layer` / `_place` / `_record` and `ctd_raster_job` (include/ctd_hip.h)
LAYER_DTYPE = table_dtype(L.CtdGlyphLayer)
PLACE_DTYPE = table_dtype(L.CtdGlyphPlace)
RECORD_DTYPE = table_dtype(L.CtdGlyphRecord)
RASTER_JOB_DTYPE = table_dtype(L.CtdRasterJob)


class GlyphAtlas:
    """Glyph coverage on the device, kept across calls.  `add(bitmaps, advance=None, bearing=None)` appends (h, w) uint8
    arrays (zero-sized ones are legal: a space) and returns their int32 ids, which never change.  The coverage lives in ONE
    device buffer of dense rows, grown by doubling with a device copy, so only the appended bytes are ever uploaded; the record
    table (`RECORD_DTYPE`: off, w, h) is kept on the device beside it and on the host as `sizes[i] = (h, w)` and `offsets[i]`.
    `advance[i] = (ax, ay)` (default (w, h)) and `bearing[i] = (bx, by)` (default 0) are host-side integer metrics that only
    `flow` reads.  `len(atlas)` glyphs, `nbytes` of coverage; `close()` frees the device buffers.
    `rasterise(font, gids, size)` appends instances of an `OutlineFont`'s glyphs without any coverage crossing the bus."""

    def __init__(self, device=None):
        need_gpu("the glyph atlas lives")
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.sizes = np.zeros((0, 2), np.int64)
        self.offsets = np.zeros((0,), np.int64)
        self.advance = np.zeros((0, 2), np.int64)
        self.bearing = np.zeros((0, 2), np.int64)
        self.nbytes = 0
        self._cov = torch.empty((4096,), dtype=torch.uint8, device=self.device)
        self._rec = torch.empty((256 * RECORD_DTYPE.itemsize,), dtype=torch.uint8, device=self.device)
        self._instances = {}                               # (font, gid, S) -> id: what `rasterise` has made

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
        with PageCall("the glyph atlas lives", (), None, self.device):       # waits: a later call may run on any stream
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
        return np.arange(n0, n0 + k, dtype=np.int32)

    def rasterise(self, font: "OutlineFont", gids, size) -> np.ndarray:
        """The atlas ids of the font's glyphs `gids` at `size` pixels an em (one for all or one per gid; S = round(size 65536
        / upem)).  Instances the
        atlas already holds, (font, gid, S), keep their ids; the missing ones are rasterised from the font's device outlines
        straight into the coverage buffer in ONE `ctd_rasterise_glyphs` launch: the buffer is grown first, only the job table
        (40 bytes an instance) and the new records go up, no coverage does.  Records and metrics are appended as `add`
        appends them: `sizes` (h, w) of the rule's box, `advance` (ax, ascent + descent) and the horizontal `bearing`
        (bx, baseline + by) of `font.metrics`.  A box side above `_lib.RASTER_MAX_SIDE` raises ValueError before anything
        changes.  Runs on the current stream of the atlas's device and waits for it, as `add` does."""
        if self._cov is None:
            raise L.CtdError("the atlas is closed")
        if not isinstance(font, OutlineFont):
            raise ValueError("font: an OutlineFont")
        gids = font._gids(gids)
        size = np.asarray(size, np.float64)
        if size.ndim > 1 or (size.ndim == 1 and len(size) != len(gids)):
            raise ValueError("size: one for all gids or one per gid")
        scale_of = {float(v): font.scale(v) for v in np.unique(size)}
        keys = [(font, g, scale_of[float(v)]) for g, v in zip(gids.tolist(), np.broadcast_to(size, gids.shape).tolist())]
        new = [key for key in dict.fromkeys(keys) if key not in self._instances]   # the missing instances, each once, in order
        k = len(new)
        if k:
            new_g, new_S = np.array([key[1] for key in new], np.int64), np.array([key[2] for key in new], np.int64)
            box, adv, bear = np.zeros((k, 4), np.int64), np.zeros((k, 2), np.int64), np.zeros((k, 2), np.int64)
            for S in np.unique(new_S):                     # host metrics, one pass a distinct scale
                at = np.flatnonzero(new_S == S)
                m = font._metrics_at(new_g[at], int(S), False)
                box[at], adv[at], bear[at] = m.box, m.advance, m.bearing
            if box[:, 2:].max() > L.RASTER_MAX_SIDE:
                raise ValueError(f"an instance's box side is above {L.RASTER_MAX_SIDE} pixels")
            if max(np.abs(adv).max(), np.abs(bear).max()) > MAX_COORD:
                raise ValueError("advance / bearing beyond 2^29")
            n0 = len(self)
            if n0 + k >= 2 ** 31:
                raise ValueError("too many glyphs")
            area = box[:, 2] * box[:, 3]
            off = self.nbytes + np.cumsum(area) - area
            total = int(area.sum())
            jobs = np.zeros((k,), RASTER_JOB_DTYPE)
            jobs["off"], jobs["w"], jobs["h"], jobs["bx"], jobs["by"] = off, box[:, 2], box[:, 3], box[:, 0], box[:, 1]
            jobs["seg_first"], jobs["seg_count"], jobs["scale"] = font.seg_first[new_g], font.seg_count[new_g], new_S
            rec = np.zeros((k,), RECORD_DTYPE)
            rec["off"], rec["h"], rec["w"] = off, box[:, 3], box[:, 2]
            segs_dev = font._sync()
            if font.device != self.device:
                raise ValueError("the font's outlines live on another device")
            want = np.where((area == 0) | (font.seg_count[new_g] == 0), L.RASTER_EMPTY, L.RASTER_OK)
            with PageCall("the glyph atlas lives", (), None, self.device) as pc:
                cov = self._grown(self._cov, self.nbytes, self.nbytes + total)
                recs = self._grown(self._rec, n0 * RECORD_DTYPE.itemsize, (n0 + k) * RECORD_DTYPE.itemsize)
                tab, (jobs_ptr, rec_ptr) = pc.upload([jobs, rec])       # one upload: the job table and the new records
                status_dev = torch.empty((k,), dtype=torch.int32, device=self.device)
                L.check(L.lib().ctd_rasterise_glyphs(segs_dev.data_ptr(), font.n_segs, jobs_ptr, k, cov.data_ptr(),
                                                     self.nbytes + total, status_dev.data_ptr(), pc.st.cuda_stream),
                        "ctd_rasterise_glyphs")
                at = rec_ptr - tab.data_ptr()
                recs[n0 * RECORD_DTYPE.itemsize: (n0 + k) * RECORD_DTYPE.itemsize].copy_(tab[at: at + rec.nbytes])
                status = pc.rows(status_dev, np.int32, k)
            if not np.array_equal(status, want):
                raise L.CtdError(f"ctd_rasterise_glyphs: status {status.tolist()} where {want.tolist()} was expected")
            self._cov, self._rec = cov, recs
            self.sizes, self.offsets = np.concatenate([self.sizes, box[:, [3, 2]]]), np.concatenate([self.offsets, off])
            self.advance, self.bearing = np.concatenate([self.advance, adv]), np.concatenate([self.bearing, bear])
            self.nbytes += total
            for i, key in enumerate(new):
                self._instances[key] = n0 + i
        return np.array([self._instances[key] for key in keys], np.int32)

    def close(self) -> None:
        self._cov = self._rec = None
        self._instances = {}

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


def place_lines(fit, count, adv, bearing, align: str = "center", blocks=None) -> np.ndarray:
    """The glyph positions of the blocks of a `layout.ShapedFit`, all blocks at once in numpy: xy (sum(count), 2), the
    top-left pixel of every glyph.  blocks: the blocks of `fit` to place, all of them `ok` (default: every ok block, in
    order); count[i]: the glyphs of blocks[i]'s run; adv and bearing: per glyph, runs one behind the other, the horizontal
    advance and the bearing (x, y) at the size of the block's chosen candidate.  A line's pen starts at its slot's x1 plus
    the shift `flow` gives a line in its box -- "left" 0, "center" slack >> 1, "right" the slack, the slack the slot's width
    less the line's advances -- and a glyph goes to (pen + bearing_x, line top + bearing_y).  ValueError where the runs are
    not the ones the fit was made with (a line record's length is not the sum of its glyphs' advances)."""
    if align not in ("left", "center", "right"):
        raise ValueError('align: "left", "center" or "right"')
    blocks = np.flatnonzero(fit.ok) if blocks is None else _ints(blocks, (-1,), "blocks")
    nb = len(blocks)
    if nb and (blocks.min() < 0 or blocks.max() >= len(fit) or not fit.ok[blocks].all()):
        raise ValueError("blocks: blocks of the fit that are ok")
    count = _ints(count, (nb,), "count")
    total = int(count.sum())
    adv, bearing = _ints(adv, (total,), "adv"), _ints(bearing, (total, 2), "bearing")
    if total == 0:
        return np.zeros((0, 2), np.int64)
    n_lines = fit.n_lines[blocks].astype(np.int64)
    first = np.cumsum(count) - count                       # a block's first glyph
    of_block = np.repeat(np.arange(nb), n_lines)           # per line of all blocks
    k = np.arange(len(of_block)) - np.repeat(np.cumsum(n_lines) - n_lines, n_lines)
    rec = fit.lines[blocks[of_block], k].astype(np.int64)  # start, x1, y, width, length
    start = first[of_block] + rec[:, 0]
    end = np.concatenate([start[1:], [total]])
    end[np.cumsum(n_lines) - 1] = first + count            # a block's last line ends with its run
    before = np.cumsum(adv) - adv                          # the advances in front of a glyph, over all runs
    cum = np.concatenate([before, [before[-1] + adv[-1]]])
    if (end <= start).any() or not np.array_equal(cum[end] - cum[start], rec[:, 4]):
        raise ValueError("the runs are not the ones the fit was made with")
    slack = rec[:, 3] - rec[:, 4]
    shift = {"left": np.zeros_like(slack), "center": slack >> 1, "right": slack}[align]
    of = np.repeat(np.arange(len(start)), end - start)     # the glyph's line
    pen = rec[of, 1] + shift[of] + before - before[start][of]
    return np.stack([pen + bearing[:, 0], rec[of, 2] + bearing[:, 1]], axis=1)


def typeset_glyphs(pages: Sequence[Page], atlas: GlyphAtlas, page_of, layer_of, glyph, xy, fill=(0, 0, 0),
                   stroke=(255, 255, 255), radius=0, clip=None, inplace: bool = False,
                   stream: Optional[torch.cuda.Stream] = None, device=None, angle=None, pivot=None) -> TypesetPages:
    """Composite glyph layers into the pages of a batch: one upload of tables and placements, one `ctd_typeset_glyphs`
    launch, one small download.  pages: as `typeset.typeset_pages`.  Per LAYER: page_of[l]; fill / stroke (RGB, one triple for
    all or one per layer); radius 0 .. 12 and clip (x1, y1, x2, y2) exclusive (one for all or one per layer; default the
    page).  Per PLACEMENT: layer_of[i] (non-decreasing), glyph[i] an id of `atlas`, xy[i] = (x, y) of the glyph's top-left
    pixel in page coordinates.  A layer's coverage is the max over its placements; layers are applied in order.  `inplace`
    as in `typeset_pages`.  Bad arguments raise ValueError before anything is uploaded.  Runs on `stream` (default: the
    current stream of the atlas's device) and waits for the result: a `TypesetPages` with one row and one status per
    LAYER, whose `xy` is per PLACEMENT and which also carries `place_layer` (= layer_of) and `place_glyph`.
    angle, pivot: per LAYER (one for all or one per layer) the whole degrees, -180 .. 180, and the page pixel (x, y; default
    (0, 0)) of the layer's frame; xy is then in FRAME coordinates and the layer is turned about its pivot into the page
    (include/ctd_hip.h, "tilted text"; `typeset.tilt_tables` bins each placement by a conservative page box), in ONE
    `ctd_typeset_tilted` launch (csrc/kernels_tilted.hip) for all layers, tilted or not.  Where no layer has a non-zero
    angle the call is the one above, exactly."""
    shapes, page_of, fill, stroke, r = _layer_args(pages, page_of, fill, stroke, radius, inplace)
    nl = len(page_of)
    tilt = _tilt_args(angle, pivot, nl)
    layer_of = _ints(layer_of, (-1,), "layer_of")
    n = len(layer_of)
    glyph, xy = _ints(glyph, (n,), "glyph"), _ints(xy, (n, 2), "xy")
    if not isinstance(atlas, GlyphAtlas) or atlas._cov is None:
        raise ValueError("atlas: an open GlyphAtlas")
    if n and (glyph.min() < 0 or glyph.max() >= len(atlas)):
        raise ValueError("glyph: an id of the atlas")
    if tilt is None:
        tiles, entries, status = glyph_tables(shapes, page_of, layer_of, atlas.sizes[glyph], xy, r, clip)
    else:
        tiles, entries, status = tilt_tables(shapes, page_of, layer_of, atlas.sizes[glyph], xy, r, clip, tilt[1], tilt[2])
    n_pages, n_tiles = len(pages), len(tiles) - 1
    device = atlas.device if device is None else torch.device(device)
    if device != atlas.device:
        raise ValueError("the atlas lives on another device")
    with PageCall("typesetting runs", pages, stream, device) as pc:
        out, pt, clip4 = _open_pages(pc, pages, shapes, page_of, clip, inplace)
        rows = np.zeros((nl,), ROW_DTYPE)
        if n_tiles:
            if tilt is None:
                lt = np.zeros((nl,), LAYER_DTYPE)
                lt["page"], lt["clip"], lt["fill"], lt["stroke"], lt["radius"] = page_of, clip4, fill, stroke, r
            else:
                lt = _tilt_layer_table(page_of, clip4, fill, stroke, r, tilt[1], tilt[2])
            entry = L.lib().ctd_typeset_glyphs if tilt is None else L.lib().ctd_typeset_tilted
            qt = np.zeros((n,), PLACE_DTYPE)
            qt["layer"], qt["glyph"], qt["x"], qt["y"] = layer_of, glyph, xy[:, 0], xy[:, 1]
            _, ptr = pc.upload([pt, lt, qt, tiles, entries])       # one upload: the tables and the placements
            rows_dev = torch.empty((nl * ROW_DTYPE.itemsize,), dtype=torch.uint8, device=pc.device)
            prm = L.CtdGlyphParams(nl, n_pages, n_tiles, len(entries), n, len(atlas), atlas.nbytes)
            L.check(entry(ptr[0], ptr[1], ptr[2], atlas._rec.data_ptr(), ptr[3], ptr[4], atlas._cov.data_ptr(), C.byref(prm),
                          rows_dev.data_ptr(), pc.st.cuda_stream), "ctd_typeset_glyphs" if tilt is None else "ctd_typeset_tilted")
            rows = pc.rows(rows_dev, ROW_DTYPE, nl)
    tp = TypesetPages(out, rows, status, np.zeros((nl, 2), np.int64))
    tp.xy, tp.place_layer, tp.place_glyph = xy, layer_of, glyph             # per placement here, not per layer
    return tp


# ---- outlines rasterised into the atlas (include/ctd_hip.h, "glyph outlines rasterised into the atlas")

def _sround(v, S):
    """A font-unit length at scale S (16.16 pixels per font unit), rounded to pixels."""
    return (np.asarray(v, np.int64) * int(S) + 32768) >> 16


def _scale_of(size, upem) -> int:
    S = int(round(float(size) * 65536 / upem))
    if not 0 < S <= L.RASTER_MAX_SCALE:
        raise ValueError(f"size: the scale {S} / 65536 pixels per font unit is not in 1 .. 2^22")
    return S


def segments_from_ops(ops) -> np.ndarray:
    """Pen-style operations -> the (n, 6) int32 segment rows (x0, y0, cx, cy, x1, y1) of the raster rule.  `ops` is a sequence
    of (name, points) as a fontTools `RecordingPen` records them (no font library is imported here): `moveTo` ((x, y),),
    `lineTo` ((x, y),), `qCurveTo` (off, ..., off, on) with TrueType's implied on-curve points between consecutive off-curve
    points (a last point of None: a contour of off-curve points only, which starts at the implied point between its last and
    its first), `closePath` / `endPath` (). A line is stored with its control point on its start.  A fill needs closed
    contours, so both `closePath` and `endPath` add the line back to the contour's start where the pen is not there.
    Coordinates are integers; an implied point between a and b is (a + b + 1) >> 1, at most half a font unit from the exact
    one.  `curveTo` raises ValueError: cubics are not accepted, convert them first (cu2qu).  Pure numpy."""
    rows, cur, start = [], None, None

    def pt(p):
        x, y = p
        if int(x) != x or int(y) != y:
            raise ValueError("outline coordinates are integers (font units)")
        if max(abs(int(x)), abs(int(y))) > 1 << 15:
            raise ValueError("outline coordinates beyond 2^15")
        return int(x), int(y)

    def mid(a, b):
        return (a[0] + b[0] + 1) >> 1, (a[1] + b[1] + 1) >> 1

    def close():
        nonlocal cur, start
        if cur is not None and start is not None and cur != start:
            rows.append(cur + cur + start)
        cur = start = None

    for name, args in ops:
        if name == "moveTo":
            close()
            cur = start = pt(args[0])
        elif name == "lineTo":
            if cur is None:
                raise ValueError("lineTo before moveTo")
            p = pt(args[0])
            rows.append(cur + cur + p)
            cur = p
        elif name == "qCurveTo":
            if len(args) < 1:
                raise ValueError("qCurveTo: at least one point")
            if args[-1] is None:                           # off-curve points only: start at an implied point
                off = [pt(a) for a in args[:-1]]
                if not off:
                    raise ValueError("qCurveTo: no points")
                close()
                cur = start = mid(off[-1], off[0])
                last = start
            else:
                if cur is None:
                    raise ValueError("qCurveTo before moveTo")
                off, last = [pt(a) for a in args[:-1]], pt(args[-1])
            for i, c in enumerate(off):
                end = mid(c, off[i + 1]) if i + 1 < len(off) else last
                rows.append(cur + c + end)
                cur = end
            if not off:
                rows.append(cur + cur + last)
                cur = last
        elif name in ("closePath", "endPath"):
            close()
        elif name == "curveTo":
            raise ValueError("curveTo: cubic curves are not accepted; convert them to quadratics first (cu2qu)")
        else:
            raise ValueError(f"unknown pen operation {name!r}")
    close()
    return np.array(rows, np.int32).reshape(-1, 6)


def outline_boxes(points: Sequence[np.ndarray], S: int) -> np.ndarray:
    """The raster rule's box of each outline at scale S: rows (bx, by, w, h), int64.  points[i]: the (n, 6) segments of glyph
    i.  X = (x S + 512) >> 10, Y = (-y S + 512) >> 10 over ALL points, controls included; floor of the minimum, ceil of the
    maximum, in pixels of 64; no segments: zeros."""
    out = np.zeros((len(points), 4), np.int64)
    for i, sg in enumerate(points):
        if len(sg) == 0:
            continue
        sg = np.asarray(sg, np.int64).reshape(-1, 3, 2)
        X, Y = (sg[..., 0] * S + 512) >> 10, (-sg[..., 1] * S + 512) >> 10
        bx, by = int(X.min()) >> 6, int(Y.min()) >> 6
        out[i] = bx, by, ((int(X.max()) + 63) >> 6) - bx, ((int(Y.max()) + 63) >> 6) - by
    return out


class OutlineFont:
    """Quadratic glyph outlines, kept on the device once.  `upem` font units per em; `ascent` and `descent` the line's extent
    above and below the baseline, both >= 0, font units.  `add(segments_list, advance)` appends glyphs ((n, 6) int32 arrays
    as `segments_from_ops` returns them; an empty one is a space) with their horizontal advances in font units and returns
    their gids, which never change.  The segments live in ONE int32 device buffer grown by doubling with a device copy, so
    only appended rows are uploaded; host copies are kept, and everything but `GlyphAtlas.rasterise` works from those,
    without a GPU (the upload then waits for the first `rasterise`)."""

    def __init__(self, upem: int, ascent: int, descent: int, device=None):
        if not (0 < int(upem) <= 1 << 15 and 0 <= int(ascent) <= 1 << 15 and 0 <= int(descent) <= 1 << 15):
            raise ValueError("upem 1 .. 2^15, ascent and descent 0 .. 2^15")
        self.upem, self.ascent, self.descent = int(upem), int(ascent), int(descent)
        self.device = None if device is None else torch.device(device)
        self.segments = []                                 # per gid: (n, 6) int32
        self.seg_first = np.zeros((0,), np.int64)
        self.seg_count = np.zeros((0,), np.int64)
        self.advance = np.zeros((0,), np.int64)
        self.n_segs = 0
        self._dev, self._on_dev = None, 0                  # the device buffer (bytes) and the segment rows it holds
        self._host = None                                  # every segment's points, (n_segs, 3, 2) int64: made when boxes are asked for

    def __len__(self) -> int:
        return len(self.segments)

    def add(self, segments_list: Sequence[np.ndarray], advance) -> np.ndarray:
        k = len(segments_list)
        advance = _ints(advance, (k,), "advance")
        if k and (advance.min() < 0 or advance.max() > 1 << 15):
            raise ValueError("advance: 0 .. 2^15 font units")
        segs = []
        for sg in segments_list:
            sg = np.asarray(sg)
            if sg.dtype.kind not in "iu" or sg.ndim != 2 or sg.shape[1] != 6:
                raise ValueError("a glyph is a (n, 6) integer array of segments")
            if sg.size and np.abs(sg.astype(np.int64)).max() > 1 << 15:
                raise ValueError("outline coordinates beyond 2^15")
            segs.append(np.ascontiguousarray(sg, np.int32))
        count = np.array([len(sg) for sg in segs], np.int64)
        if self.n_segs + int(count.sum()) >= 2 ** 31 or len(self) + k >= 2 ** 31:
            raise ValueError("too many segments")
        n0 = len(self)
        self.seg_first = np.concatenate([self.seg_first, self.n_segs + np.cumsum(count) - count])
        self.seg_count = np.concatenate([self.seg_count, count])
        self.advance = np.concatenate([self.advance, advance])
        self.segments += segs
        self.n_segs += int(count.sum())
        if torch.cuda.is_available():
            self._sync()
        return np.arange(n0, n0 + k, dtype=np.int32)

    def _sync(self):
        """The device buffer with every segment row in it: the rows added since the last call go up, nothing else."""
        if not torch.cuda.is_available():
            raise L.CtdError("the outlines are rasterised on the GPU and there is none (no CPU fallback)")
        if self.device is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        if self._dev is None:
            self._dev = torch.empty((4096 * 24,), dtype=torch.uint8, device=self.device)
        if self._on_dev < self.n_segs:
            with torch.cuda.device(self.device):
                self._dev = GlyphAtlas._grown(self._dev, self._on_dev * 24, self.n_segs * 24)
                g0 = int(np.searchsorted(self.seg_first, self._on_dev, side="left"))   # whole glyphs were uploaded
                new = np.concatenate([sg.ravel() for sg in self.segments[g0:]])
                self._dev[self._on_dev * 24: self.n_segs * 24].copy_(torch.from_numpy(new.view(np.uint8)))
                torch.cuda.current_stream(self.device).synchronize()
            self._on_dev = self.n_segs
        return self._dev

    def scale(self, size) -> int:
        """S = round(size 65536 / upem): the 16.16 scale at which `size` pixels make an em."""
        return _scale_of(size, self.upem)

    def boxes(self, gids, S: int) -> np.ndarray:
        """`outline_boxes` of the font's glyphs `gids` at scale S, all at once: rows (bx, by, w, h)."""
        gids = self._gids(gids)
        out = np.zeros((len(gids), 4), np.int64)
        count = self.seg_count[gids]
        inked = np.flatnonzero(count)
        if len(inked):
            if self._host is None or len(self._host) != self.n_segs:
                self._host = np.concatenate(self.segments).astype(np.int64).reshape(-1, 3, 2)
            c = count[inked]
            starts = np.cumsum(c) - c
            sg = self._host[np.repeat(self.seg_first[gids[inked]] - starts, c) + np.arange(int(c.sum()))]
            X, Y = (sg[..., 0] * int(S) + 512) >> 10, (-sg[..., 1] * int(S) + 512) >> 10
            lo = [np.minimum(np.minimum(v[:, 0], v[:, 1]), v[:, 2]) for v in (X, Y)]      # over a segment's three points
            hi = [np.maximum(np.maximum(v[:, 0], v[:, 1]), v[:, 2]) for v in (X, Y)]
            bx, by = np.minimum.reduceat(lo[0], starts) >> 6, np.minimum.reduceat(lo[1], starts) >> 6
            out[inked, 0], out[inked, 1] = bx, by
            out[inked, 2] = ((np.maximum.reduceat(hi[0], starts) + 63) >> 6) - bx
            out[inked, 3] = ((np.maximum.reduceat(hi[1], starts) + 63) >> 6) - by
        return out

    def _gids(self, gids):
        gids = _ints(gids, (-1,), "gids")
        if len(gids) and (gids.min() < 0 or gids.max() >= len(self)):
            raise ValueError("gids: glyphs of the font")
        return gids

    def metrics(self, gids, size, vertical: bool = False):
        """What `flow` reads, for `gids` at `size` pixels an em, from the outlines by the raster rule, on the host: an object
        with `sizes[i] = (h, w)`, `advance[i] = (ax, ay)` and `bearing[i]` of gids[i] (so a run indexes it by POSITION in
        `gids`), plus `box[i] = (bx, by, w, h)`, `scale`, `baseline` (the scaled ascent) and `line` (the scaled ascent plus
        the scaled descent; vertical: the scaled em, a column's width).  ax = (adv S + 32768) >> 16 and ay = `line` of the
        horizontal case.  Horizontal bearing: (bx, baseline + by), so a line's top is `baseline` above the pen's baseline.
        vertical=True: bearing (0, baseline + by); `flow` centres a glyph in its column."""
        return self._metrics_at(gids, self.scale(size), vertical)

    def _metrics_at(self, gids, S: int, vertical: bool):
        import types
        gids = self._gids(gids)
        box = self.boxes(gids, S)
        base, down = int(_sround(self.ascent, S)), int(_sround(self.descent, S))
        adv = np.stack([_sround(self.advance[gids], S), np.full((len(gids),), base + down, np.int64)], axis=1)
        bear = np.stack([np.zeros((len(gids),), np.int64) if vertical else box[:, 0], base + box[:, 1]], axis=1)
        return types.SimpleNamespace(sizes=box[:, [3, 2]].copy(), advance=adv.reshape(-1, 2), bearing=bear.reshape(-1, 2), box=box,
                                     scale=S, baseline=base, line=int(_sround(self.upem, S)) if vertical else base + down)

    def close(self) -> None:
        self._dev, self._on_dev = None, 0

    def __repr__(self) -> str:
        return f"OutlineFont({len(self)} glyphs, {self.n_segs} segments, upem {self.upem})"


def _run_metrics(run_gids, font, size, vertical):
    run = _ints(run_gids, (-1,), "run")
    uniq, pos = np.unique(run, return_inverse=True)
    return font.metrics(uniq, size, vertical=vertical), uniq, pos.reshape(-1)


def flow_outlines(run_gids, font: OutlineFont, rect, size, **flow_kwargs) -> tuple:
    """`flow` of a run of the FONT's gids at `size`, on `font.metrics`: (xy, fits).  `line` defaults to the metrics' `line`
    (ascent + descent, scaled; vertical: the scaled em), not to the run's tallest glyph: the bearings are measured from it."""
    m, _, pos = _run_metrics(run_gids, font, size, bool(flow_kwargs.get("vertical", False)))
    kw = dict(flow_kwargs)
    if kw.get("line") is None:
        kw["line"] = m.line
    return flow(pos, m, rect, **kw)


def fit(run_gids, font: OutlineFont, rect, sizes, **flow_kwargs) -> tuple:
    """The largest of the ascending `sizes` (pixels an em) at which the run, flowed by `flow_outlines` into `rect`, fits:
    (size, True), or (sizes[0], False) where none does.  Bisection: the greedy breaker's `fits` is monotone in the size on
    these metrics (tests/test_raster_ref.py holds it against a linear scan on seeded cases).  Host only, metrics only:
    nothing is rasterised."""
    sizes = list(sizes)
    if not sizes or any(b <= a for a, b in zip(sizes, sizes[1:])):
        raise ValueError("sizes: ascending, at least one")
    lo, hi = -1, len(sizes)                                # sizes[lo] fits (or lo = -1), sizes[hi] does not (or hi = len)
    while hi - lo > 1:
        k = (lo + hi) >> 1
        if flow_outlines(run_gids, font, rect, sizes[k], **flow_kwargs)[1]:
            lo = k
        else:
            hi = k
    return (sizes[lo], True) if lo >= 0 else (sizes[0], False)
