"""Fill what erase leaves: a smooth pull-push fill of a hole mask, on the GPU.

`erase_text` cleans a page only where the background is one colour; text on a gradient or a screentone, text that touches the
balloon's outline and text outside every box come back as `er.rest`, "the mask an inpainter still needs".  This is the step
that fills it without leaving the device:

    fp = fill_rest(er.pages, er.rest)                    # or TextDetector.fill_rest(pages, results)
    fp.pages[i]                                          # the page with every hole pixel filled, on the device

builds one small table with numpy, uploads it once, makes ONE `ctd_fill_rest` call (csrc/kernels_fill.hip: a pull launch over
the 64 x 64 tiles of all pages, one workgroup per page for the coarse levels, a push launch over the tiles, no host step
between them) and downloads one small table.  The rule is integers only and stated in include/ctd_hip.h (restated in numpy in
tests/fill_ref.py; DESIGN.md section 4.19 has its limits): pull builds an image pyramid of the known pixels -- a level pixel is
the rounded mean of its known children --, push fills the unknown pixels from coarse to fine by bilinear upsampling with the
weights 9, 3, 3, 1.  A gradient comes back as the gradient, art as its blurred surroundings; texture does not come back
(`texture.texture_fill` starts from this result and puts screentone back by patch matching).
There is no per-page Python and no CPU fallback: without a GPU it raises `CtdError` like the rest of the package.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import _lib as L
from .pagecall import Page, PageCall, check_pages, table_dtype

__all__ = ["fill_rest", "FilledPages", "fill_tables", "level_shapes", "PAGE_DTYPE", "ROW_DTYPE"]

# numpy views of `ctd_fill_page` / `ctd_fill_row` (include/ctd_hip.h)
PAGE_DTYPE = table_dtype(L.CtdFillPage)
ROW_DTYPE = table_dtype(L.CtdFillRow)

STORED_LEVELS = 6          # levels 1 .. 6 pass through the scratch buffer; the coarser ones never leave the chip


def level_shapes(H: int, W: int) -> list:
    """[(H_l, W_l)] for l = 0 .. T: level l + 1 is ceil(H_l / 2) x ceil(W_l / 2), the top level T is the first that is 1 x 1."""
    out = [(int(H), int(W))]
    while out[-1] != (1, 1):
        h, w = out[-1]
        out.append(((h + 1) // 2, (w + 1) // 2))
    return out


def fill_tables(shapes: Sequence) -> tuple:
    """The tile and scratch columns of the page table for pages of `shapes` = (H, W): (tile0, n_tiles, lvl0, scratch_dwords,
    levels) -- the 64 x 64 tiles of the pages before each page, the tiles of all pages, each page's first pyramid dword of
    the scratch buffer (the per-tile hole counts come first, then levels 1 .. 6 of every page), the buffer's size in dwords,
    and the top level T of each page."""
    H = np.array([s[0] for s in shapes], np.int64)
    W = np.array([s[1] for s in shapes], np.int64)
    if len(H) and (min(H.min(), W.min()) < 1 or max(H.max(), W.max()) > L.FILL_MAX_SIDE):
        raise ValueError(f"page sides must be 1 .. {L.FILL_MAX_SIDE}")
    t = L.FILL_TILE
    tiles = ((W + t - 1) // t) * ((H + t - 1) // t)
    n_tiles = int(tiles.sum())
    if n_tiles >= 2 ** 31:
        raise ValueError("too many pixels for one call")
    plane = np.zeros_like(H)
    for l in range(1, STORED_LEVELS + 1):
        plane += ((H + (1 << l) - 1) >> l) * ((W + (1 << l) - 1) >> l)
    lvl0 = n_tiles + np.cumsum(plane) - plane
    side = np.maximum(H, W)
    levels = np.zeros_like(H)
    for l in range(1, 14):                                          # T = ceil(log2(the longer side))
        levels += (side > (1 << (l - 1))).astype(np.int64)
    return np.cumsum(tiles) - tiles, n_tiles, lvl0, int(n_tiles + plane.sum()), levels


class FilledPages:
    """The result of `fill_rest`.  `pages[i]` (H,W,3) u8 in the page's channel order: dense device tensors, views of ONE
    allocation, page i with its hole pixels filled and every other pixel as it was.  Per page: `rows` the kernel's records
    (`ROW_DTYPE`: status, n_hole, levels, top[3] in PAGE channel order), `status[i]` = `_lib.FILL_OK` (filled) /
    `FILL_NO_HOLE` (nothing to fill, a copy) / `FILL_NO_KNOWN` (nothing to fill from, a copy), `n_hole[i]` the number of hole
    pixels, `top[i]` the colour of the pyramid's top pixel -- the mean of means of the known pixels -- in RGB."""

    def __init__(self, pages: List[torch.Tensor], rows: np.ndarray):
        self.pages, self.rows = pages, rows
        if len(pages) != len(rows):
            raise ValueError("one row per page")
        self.status = rows["status"]
        self.n_hole = rows["n_hole"]
        self.top = np.ascontiguousarray(rows["top"][:, ::-1])

    def __len__(self) -> int:
        return len(self.pages)

    def to_host(self):
        """The pages as a list of numpy arrays."""
        return [p.cpu().numpy() for p in self.pages]

    def __repr__(self) -> str:
        return f"FilledPages({len(self.pages)} pages, {int((self.status == L.FILL_OK).sum())} filled)"


def fill_rest(pages: Sequence[Page], holes: Sequence[Page], stream: Optional[torch.cuda.Stream] = None, device=None) -> FilledPages:
    """Fill the hole pixels of EVERY page of a batch by the pull-push rule: one table upload, one `ctd_fill_rest` call (three
    launches), one small download.  pages: uint8 (H,W,3) pages of any mix of sizes, holes: uint8 (H,W) masks of the same
    sizes (normally `ErasedPages.pages` and `.rest`; a pixel is a hole where the mask is not 0), both on the device or on the
    host (uploaded here); row strides beyond the row size are honoured.  Runs on `stream` (default: the current stream of
    the pages' device) and waits for the result; see `FilledPages`."""
    if len(holes) != len(pages):
        raise ValueError("one hole mask per page")
    check_pages(pages, holes, mask="hole mask")
    tile0, n_tiles, lvl0, scratch_dwords, _ = fill_tables([tuple(p.shape[:2]) for p in pages])
    n_pages = len(pages)
    if n_pages == 0:
        return FilledPages([], np.zeros((0,), ROW_DTYPE))
    with PageCall("filling holes runs", pages, stream, device) as pc:
        P, M = pc.pages(pages), pc.pages(holes)
        # one buffer behind all the outputs, each on a 256-byte boundary
        out = pc.outputs([(int(h), int(w), 3) for h, w in zip(P.H, P.W)])
        pt = np.zeros((n_pages,), PAGE_DTYPE)
        pt["page_dev"], pt["hole_dev"], pt["out_dev"] = P.ptr, M.ptr, [o.data_ptr() for o in out]
        pt["H"], pt["W"], pt["pitch"], pt["hole_pitch"], pt["out_pitch"] = P.H, P.W, P.pitch, M.pitch, 3 * P.W
        pt["tile0"], pt["lvl0"] = tile0, lvl0
        tab = pc.upload([pt])[0]
        scratch = torch.empty((scratch_dwords,), dtype=torch.int32, device=pc.device)
        rows_dev = torch.empty((n_pages * ROW_DTYPE.itemsize,), dtype=torch.uint8, device=pc.device)
        prm = L.CtdFillParams(n_tiles)
        L.check(L.lib().ctd_fill_rest(tab.data_ptr(), n_pages, C.byref(prm), scratch.data_ptr(), rows_dev.data_ptr(),
                                      pc.st.cuda_stream), "ctd_fill_rest")
        rows = pc.rows(rows_dev, ROW_DTYPE, n_pages)
    return FilledPages(out, rows)
