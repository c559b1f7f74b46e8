"""Font colours: the fill and the surround colour of every text line of a batch, on the GPU.

Every `TextBlock` carries the reference's colour fields (`fg_r/g/b`, `bg_r/g/b`, utils/textblock.py:62-67); in the reference's
ecosystem an OCR model fills them line by line.  The detector already holds what determines them -- the page, the refined text
mask and the line quads -- so

    lc = line_colors(pages, masks, blk_lists)           # or TextDetector.font_colors(pages, results)
    lc.apply(blk_lists)                                 # blk.get_font_colors() / blk.stroke_width now answer

builds one job table with numpy, uploads it once, runs ONE kernel launch (`ctd_line_colors`, csrc/kernels_color.hip: one block
per line) and downloads one small table.  The rule is integers only and stated in include/ctd_hip.h (restated in numpy in
tests/color_ref.py; DESIGN.md section 4.16 has its limits): inside the quad, split the pixels by the mask, call a pixel
text-like when its grey is nearer to the mean under the mask than to the mean off it, fill = mean colour of the text-like
pixels under the mask, surround = mean colour of everything that is not text-like.  There is no per-line Python and no CPU
fallback: without a GPU it raises `CtdError` like the rest of the package.
"""
from __future__ import annotations

from collections import namedtuple
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib as L
from .pagecall import Page, PageCall, blk_lists_of, check_pages, table_dtype
from .regions import batch_lines

__all__ = ["line_colors", "LineColors", "BlockColors", "color_rows", "JOB_DTYPE", "OUT_DTYPE"]

# numpy views of `ctd_color_job` / `ctd_line_color` (include/ctd_hip.h)
JOB_DTYPE = table_dtype(L.CtdColorJob)
OUT_DTYPE = table_dtype(L.CtdLineColor)

BlockColors = namedtuple("BlockColors", "index valid fg bg")
BlockColors.__doc__ = """`LineColors.blocks()`: `index` (m,2) i32 = (page, block) of every block that has lines, in order; `valid[j]`
False where none of the block's lines has status OK / NO_CONTRAST (fg / bg are 0 there); `fg`, `bg` (m,3) u8 RGB."""


def color_rows(pages: Sequence[torch.Tensor], masks: Sequence[torch.Tensor], page_of, quads,
               stream: Optional[torch.cuda.Stream] = None) -> np.ndarray:
    """`ctd_line_colors`: row i = the rule of include/ctd_hip.h on (pages[page_of[i]], masks[page_of[i]], quads[i]).  `pages`
    (H,W,3) / `masks` (H,W): dense uint8 device tensors as `pagecall.device_pages` returns them (any row pitch); quads (n,8)
    i32.  One upload, ONE launch, one download; returns the rows on the host as an `OUT_DTYPE` array (synchronises `stream`,
    default the current stream of the pages' device)."""
    quads = np.ascontiguousarray(np.asarray(quads, np.int32).reshape(-1, 8))
    n = len(quads)
    if n == 0:
        return np.zeros((0,), OUT_DTYPE)
    if not all(isinstance(t, torch.Tensor) and t.is_cuda for t in list(pages) + list(masks)):
        raise L.CtdError("the kernel reads its pages and masks in device memory (no CPU fallback)")
    page_of = np.asarray(page_of, np.int64).reshape(n)
    with PageCall("font colours run", pages, stream) as pc:
        P, M = pc.pages(pages, dense=True), pc.pages(masks, dense=True)
        jobs = np.zeros((n,), JOB_DTYPE)
        jobs["page_dev"], jobs["mask_dev"], jobs["H"], jobs["W"] = P.ptr[page_of], M.ptr[page_of], P.H[page_of], P.W[page_of]
        jobs["pitch"], jobs["mask_pitch"], jobs["quad"] = P.pitch[page_of], M.pitch[page_of], quads
        tab = pc.upload([jobs])[0]
        out = torch.empty((n * OUT_DTYPE.itemsize,), dtype=torch.uint8, device=pc.device)
        L.check(L.lib().ctd_line_colors(tab.data_ptr(), n, out.data_ptr(), pc.st.cuda_stream), "ctd_line_colors")
        rows = pc.rows(out, OUT_DTYPE, n)
    return rows


class LineColors:
    """The colours of `line_colors`, columnar: `index[i] = (page, block, line)` names the line (as in `LineRegions`);
    `status[i]` is `_lib.COLOR_OK` / `COLOR_EMPTY` (no pixel inside the quad) / `COLOR_NO_MASK` (no mask pixel inside) /
    `COLOR_NO_CONTRAST` (the greys under and off the mask tie, e.g. isoluminant text: fill = mean under the mask, surround =
    mean off it) / `COLOR_TOO_LARGE`; `n_on`, `n_off` the mask split of the quad's pixels, `n_fg`, `n_bg` the pixels the fill
    and the surround were averaged over; `fg`, `bg` (n,3) u8 in RGB, the reference's `frgb` order.  `rows`: the kernel's
    records (`OUT_DTYPE`; sums and colours there are in PAGE channel order, BGR)."""

    def __init__(self, index: np.ndarray, rows: np.ndarray):
        self.index = np.asarray(index, np.int32).reshape(-1, 3)
        self.rows = rows
        if len(self.index) != len(rows):
            raise ValueError("one index row per line")
        self.status, self.n_on, self.n_off = rows["status"], rows["n_on"], rows["n_off"]
        self.n_fg, self.n_bg = rows["n_fg"], rows["n_bg"]
        self.fg = np.ascontiguousarray(rows["fg"][:, ::-1])
        self.bg = np.ascontiguousarray(rows["bg"][:, ::-1])

    def __len__(self) -> int:
        return len(self.index)

    def blocks(self) -> BlockColors:
        """Per-block pooled colours: (2 * sum S + sum n) // (2 * sum n) per channel over the block's OK and NO_CONTRAST
        lines, so long lines weigh more and the result stays integer.  Where none of those lines has a surround pixel (all
        are NO_CONTRAST without an off-mask pixel) the surround is the fill, as for a single line."""
        n = len(self)
        if n == 0:
            z = np.zeros((0, 3), np.uint8)
            return BlockColors(np.zeros((0, 2), np.int32), np.zeros((0,), bool), z, z.copy())
        key = self.index[:, :2]
        first = np.ones((n,), bool)
        first[1:] = (key[1:] != key[:-1]).any(axis=1)        # lines come block by block (`regions.batch_lines`)
        starts = np.nonzero(first)[0]
        use = ((self.status == L.COLOR_OK) | (self.status == L.COLOR_NO_CONTRAST)).astype(np.int64)
        pool = lambda col: np.add.reduceat(col * (use if col.ndim == 1 else use[:, None]), starts, axis=0)   # noqa: E731
        n_fg, n_bg = pool(self.n_fg.astype(np.int64)), pool(self.n_bg.astype(np.int64))
        s_fg, s_bg = pool(self.rows["s_fg"][:, ::-1].astype(np.int64)), pool(self.rows["s_bg"][:, ::-1].astype(np.int64))
        valid = n_fg > 0
        mean = lambda s, k: (2 * s + k[:, None]) // np.maximum(2 * k[:, None], 1)                             # noqa: E731
        fg = np.where(valid[:, None], mean(s_fg, n_fg), 0)
        bg = np.where(valid[:, None], np.where((n_bg > 0)[:, None], mean(s_bg, n_bg), fg), 0)
        return BlockColors(key[starts].copy(), valid, fg.astype(np.uint8), bg.astype(np.uint8))

    def apply(self, blk_lists: Sequence) -> BlockColors:
        """`blk.set_font_colors(fg, bg, accumulate=True)` on every valid block of `blk_lists` (per page a list of
        `TextBlock`s, a `BlockList` or a result triple): `blk.get_font_colors()` then returns exactly the pooled colours.
        Blocks without a valid line are left untouched.  Returns `blocks()`."""
        bc = self.blocks()
        lists = blk_lists_of(blk_lists)
        for (pg, b), ok, fg, bg in zip(bc.index.tolist(), bc.valid.tolist(), bc.fg.tolist(), bc.bg.tolist()):
            if ok:
                lists[pg][b].set_font_colors(fg, bg, accumulate=True)
        return bc

    def __repr__(self) -> str:
        return f"LineColors({len(self)} lines, {int((self.status == L.COLOR_OK).sum())} ok)"


def line_colors(pages: Sequence[Page], masks: Sequence[Page], blk_lists: Sequence,
                stream: Optional[torch.cuda.Stream] = None, device=None) -> LineColors:
    """Fill and surround colour of EVERY line of EVERY block of a batch: one table upload, one kernel launch, one small
    download.  pages: uint8 BGR (H,W,3) pages of any mix of sizes, masks: uint8 (H,W) text masks of the same sizes (normally
    each page's `mask_refined`, either refine mode; a pixel counts as text where the mask is not 0), both on the device or on
    the host (uploaded here); blk_lists[b]: page b's blk_list -- a list of `TextBlock`s or a `BlockList` (read from its
    records, no `TextBlock` is built).  Runs on `stream` (default: the current stream of the pages' device) and waits for the
    result; see `LineColors`.
    "Surround" is the colour AROUND the glyphs.  The reference names the field it goes to "stroke" (`srgb`, `stroke_width`):
    it is an outline colour only where the text has an outline; for plain text it is the balloon or page colour.  Text as
    bright as its background (isoluminant) and lettering of three colours are beyond the rule: the first comes back as
    `COLOR_NO_CONTRAST`, the second as the mean of whatever falls on each side of the grey split."""
    if len(pages) != len(blk_lists) or len(masks) != len(pages):
        raise ValueError("one mask and one blk_list per page")
    check_pages(pages, masks, "BGR ", nonempty=False)
    index, quads = batch_lines(blk_lists)[:2]
    if len(index) == 0:
        return LineColors(index, np.zeros((0,), OUT_DTYPE))
    with PageCall("font colours run", pages, stream, device) as pc:
        rows = color_rows(pc.pages(pages).t, pc.pages(masks).t, index[:, 0], quads)
    return LineColors(index, rows)
