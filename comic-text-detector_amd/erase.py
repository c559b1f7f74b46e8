"""Erase text on plain backgrounds: cleaned pages and the mask an inpainter still needs, on the GPU.

Most text of a comic page sits on a flat balloon.  Downstream tools do not run an inpainting network for such a block: they
look at the background next to the glyphs and, where it is one colour, fill the text with it; only the other blocks go to
the expensive inpainter.  The detector already holds what decides that -- the page, the refined text mask and the block
boxes -- so

    er = erase_text(pages, masks, blk_lists)            # or TextDetector.erase_text(pages, results)
    er.pages[i], er.rest[i]                             # the cleaned page and what is left to inpaint, on the device

builds two small tables with numpy, uploads them once, makes ONE `ctd_erase_text` call (csrc/kernels_erase.hip: a stats launch,
one workgroup per block, and a paint launch over the page tiles, no host step between them) and downloads one small table.
The rule is integers only and stated in include/ctd_hip.h (restated in numpy in tests/erase_ref.py; DESIGN.md section 4.17 has
its limits): sample a ring of background around the block's glyphs, away from anybody's glyphs; the block is plain when 15/16 of
the ring lies within `tol` of the ring's median in every channel; a plain block's glyphs, grown by `grow`, are filled with the
median.  There is no per-block Python and no CPU fallback: without a GPU it raises `CtdError` like the rest of the package.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import _lib as L
from .pagecall import Page, PageCall, blk_lists_of, check_pages, check_pitch, table_dtype
from .textblock import BlockList

__all__ = ["erase_text", "ErasedPages", "erase_tables", "JOB_DTYPE", "PAGE_DTYPE", "ROW_DTYPE"]

# numpy views of `ctd_erase_job` / `ctd_erase_page` / `ctd_erase_row` (include/ctd_hip.h)
JOB_DTYPE = table_dtype(L.CtdEraseJob)
PAGE_DTYPE = table_dtype(L.CtdErasePage)
ROW_DTYPE = table_dtype(L.CtdEraseRow)


def check_params(grow, ring, tol, min_ring) -> L.CtdEraseParams:
    vals = (grow, ring, tol, min_ring)
    if not all(isinstance(v, (int, np.integer)) and not isinstance(v, bool) for v in vals):
        raise ValueError("grow, ring, tol and min_ring are integers")
    if not (0 <= grow <= L.ERASE_MAX_GROW and 1 <= ring <= L.ERASE_MAX_RING and 0 <= tol <= 255 and 1 <= min_ring < 2 ** 31):
        raise ValueError("grow in 0..8, ring in 1..16, tol in 0..255, min_ring >= 1")
    return L.CtdEraseParams(int(grow), int(ring), int(tol), int(min_ring), 0)


def _page_boxes(blk_list) -> np.ndarray:
    """(n, 4) i32 xyxy of a page's blocks in order; a `BlockList` is read from its records (no `TextBlock` is built)."""
    if isinstance(blk_list, BlockList):
        return np.asarray(blk_list.records["xyxy"], np.int64).reshape(-1, 4)
    a = np.asarray([b.xyxy for b in blk_list], np.float64).reshape(-1, 4)
    if not np.array_equal(a, np.trunc(a)):
        raise ValueError("block boxes must have integer coordinates (the detector's xyxy)")
    return a.astype(np.int64)


def erase_tables(boxes: Sequence[np.ndarray], shapes: Sequence) -> tuple:
    """The job table and the block / tile columns of the page table for pages of `shapes` = (H, W) with `boxes[i]` (n_i, 4):
    (jobs JOB_DTYPE, block0, n_blocks, tile0, n_tiles)."""
    counts = np.array([len(b) for b in boxes], np.int64)
    n = int(counts.sum())
    jobs = np.zeros((n,), JOB_DTYPE)
    if n:
        xy = np.concatenate([np.asarray(b, np.int64).reshape(-1, 4) for b in boxes])
        jobs["xyxy"] = np.clip(xy, -2 ** 31, 2 ** 31 - 1)          # beyond +-2^29 is TOO_LARGE either way
        jobs["page"] = np.repeat(np.arange(len(boxes)), counts)
    H = np.array([s[0] for s in shapes], np.int64)
    W = np.array([s[1] for s in shapes], np.int64)
    tiles = ((W + L.ERASE_TILE_W - 1) // L.ERASE_TILE_W) * ((H + L.ERASE_TILE_H - 1) // L.ERASE_TILE_H)
    n_tiles = int(tiles.sum())
    if n_tiles >= 2 ** 31 or n >= 2 ** 31:
        raise ValueError("too many pixels or blocks for one call")
    return jobs, np.cumsum(counts) - counts, counts, np.cumsum(tiles) - tiles, n_tiles


def page_table(P, M, block0, counts) -> np.ndarray:
    """The input columns of the `PAGE_DTYPE` table, which `balloons` reads too; P, M: `PageCall.pages` of pages and masks."""
    pt = np.zeros((len(P.t),), PAGE_DTYPE)
    pt["page_dev"], pt["mask_dev"], pt["H"], pt["W"], pt["pitch"], pt["mask_pitch"] = P.ptr, M.ptr, P.H, P.W, P.pitch, M.pitch
    pt["block0"], pt["n_blocks"] = block0, counts
    return pt


class ErasedPages:
    """The result of `erase_text`.  `pages[i]` (H,W,3) u8 BGR and `rest[i]` (H,W) u8: dense device tensors, page i with the
    glyphs of its plain blocks filled, and the mask an inpainter still needs (255 = inpaint; 0 where a plain block was filled).
    Per block, in order: `index[j] = (page, block)`, `rows` the kernel's records (`ROW_DTYPE`: status, n_fill, n_ring, cnt[3],
    med[3], the last two in PAGE channel order), `status[j]` = `_lib.ERASE_PLAIN` (filled) / `ERASE_TEXTURED` (the background
    is not one colour) / `ERASE_NO_RING` (too little background in reach) / `ERASE_NO_MASK` (no text pixel in the box) /
    `ERASE_EMPTY` (the box misses the page) / `ERASE_TOO_LARGE`, `plain[j]` bool, `fill[j]` the fill colour in RGB (the
    ring's median; painted only where `plain`)."""

    def __init__(self, pages: List[torch.Tensor], rest: List[torch.Tensor], index: np.ndarray, rows: np.ndarray):
        self.pages, self.rest = pages, rest
        self.index = np.asarray(index, np.int32).reshape(-1, 2)
        self.rows = rows
        if len(self.index) != len(rows):
            raise ValueError("one index row per block")
        self.status = rows["status"]
        self.plain = self.status == L.ERASE_PLAIN
        self.fill = np.ascontiguousarray(rows["med"][:, ::-1])

    def __len__(self) -> int:
        return len(self.index)

    def to_host(self):
        """(pages, rest) as lists of numpy arrays."""
        return [p.cpu().numpy() for p in self.pages], [r.cpu().numpy() for r in self.rest]

    def __repr__(self) -> str:
        return f"ErasedPages({len(self.pages)} pages, {len(self)} blocks, {int(self.plain.sum())} plain)"


def erase_text(pages: Sequence[Page], masks: Sequence[Page], blk_lists: Sequence, grow: int = 2, ring: int = 4, tol: int = 12,
               min_ring: int = 16, stream: Optional[torch.cuda.Stream] = None, device=None) -> ErasedPages:
    """Decide for EVERY block of EVERY page of a batch whether it stands on a plain background, fill the plain ones and make
    the mask of the rest: one table upload, one `ctd_erase_text` call (two launches), one small download.  pages: uint8 BGR
    (H,W,3) pages of any mix of sizes, masks: uint8 (H,W) text masks of the same sizes (normally each page's `mask_refined`,
    either refine mode; a pixel counts as text where the mask is not 0), both on the device or on the host (uploaded here);
    blk_lists[b]: page b's blk_list -- a list of `TextBlock`s or a `BlockList` (read from its records, no `TextBlock` is
    built).  grow: the fill reaches this far beyond a block's text; ring: width of the background ring that is sampled;
    tol: how far from the ring's median a ring pixel may lie; min_ring: fewer ring pixels than this give no decision.  Runs
    on `stream` (default: the current stream of the pages' device) and waits for the result; see `ErasedPages`."""
    prm = check_params(grow, ring, tol, min_ring)
    if len(pages) != len(blk_lists) or len(masks) != len(pages):
        raise ValueError("one mask and one blk_list per page")
    check_pages(pages, masks, "BGR ")
    boxes = [_page_boxes(b) for b in blk_lists_of(blk_lists)]
    jobs, block0, counts, tile0, n_tiles = erase_tables(boxes, [tuple(p.shape[:2]) for p in pages])
    n, n_pages = len(jobs), len(pages)
    index = np.stack([jobs["page"], np.arange(n) - np.repeat(block0, counts)], axis=1).astype(np.int32) if n else \
        np.zeros((0, 2), np.int32)
    if n_pages == 0:
        return ErasedPages([], [], index, np.zeros((0,), ROW_DTYPE))
    with PageCall("erasing text runs", pages, stream, device) as pc:
        P, M = pc.pages(pages), pc.pages(masks)
        check_pitch(3 * P.W)
        # one buffer behind all the outputs: the pages, then the rest masks, each on a 256-byte boundary
        views = pc.outputs([(int(h), int(w), 3) for h, w in zip(P.H, P.W)] + [(int(h), int(w)) for h, w in zip(P.H, P.W)])
        out, rest = views[:n_pages], views[n_pages:]
        pt = page_table(P, M, block0, counts)
        pt["out_dev"] = [o.data_ptr() for o in out]
        pt["rest_dev"] = [r.data_ptr() for r in rest]
        pt["out_pitch"], pt["rest_pitch"], pt["tile0"] = 3 * P.W, P.W, tile0
        prm.n_tiles = n_tiles
        _, (jobs_ptr, pages_ptr) = pc.upload([jobs, pt])                    # jobs, then pages: one upload
        rows_dev = torch.empty((max(n, 1) * ROW_DTYPE.itemsize,), dtype=torch.uint8, device=pc.device)
        L.check(L.lib().ctd_erase_text(jobs_ptr, n, pages_ptr, n_pages, C.byref(prm), rows_dev.data_ptr(), pc.st.cuda_stream),
                "ctd_erase_text")
        rows = pc.rows(rows_dev, ROW_DTYPE, n) if n else np.zeros((0,), ROW_DTYPE)
    return ErasedPages(out, rest, index, rows)
