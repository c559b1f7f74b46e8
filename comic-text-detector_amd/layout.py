"""Layout boxes: the largest free rectangle in every balloon, on the GPU.

A typesetter lays translated text into a box, not into a bit plane.  `balloons.balloon_regions` leaves every block's free
area on the device as a bit plane; this is the step from that plane to the box:

    br = balloon_regions(pages, masks, blk_lists)           # or TextDetector.balloons(...)
    lb = layout_boxes(br)                                   # or TextDetector.layout_boxes(pages, results)
    lb.ok[j], lb.rect[j], lb.area[j], lb.a_rect[j], lb.a_area[j], lb.n_inner[j]

uploads one small table (the jobs and the balloon rows), makes ONE `ctd_layout_boxes` call (csrc/kernels_layout.hip: one
launch, one workgroup per block, the window's bit planes in LDS) on the planes where they lie, and downloads one small table.
The rule is integers only and stated in include/ctd_hip.h (restated in numpy in tests/layout_ref.py; DESIGN.md section 4.20
has its limits): the region is eroded by `inset` pixels, clipped at the window; `rect` is the largest axis-aligned rectangle
inside what is left, `a_rect` the largest one that contains the block's anchor; at equal area the smaller y1, then x1, then
y2 wins, so the answer is a function of the plane alone.  There is no per-block Python and no CPU fallback: without a GPU it
raises `CtdError` like the rest of the package.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np
import torch

from . import _lib as L
from .balloons import ROW_DTYPE as BALLOON_ROW_DTYPE
from .balloons import BalloonRegions
from .pagecall import PageCall, table_dtype

__all__ = ["layout_boxes", "LayoutBoxes", "box_anchors", "check_params", "JOB_DTYPE", "ROW_DTYPE"]

# numpy views of `ctd_layout_job` / `ctd_layout_row` (include/ctd_hip.h)
JOB_DTYPE = table_dtype(L.CtdLayoutJob)
ROW_DTYPE = table_dtype(L.CtdLayoutRow)


def check_params(inset) -> L.CtdLayoutParams:
    if not isinstance(inset, (int, np.integer)) or isinstance(inset, bool):
        raise ValueError("inset is an integer")
    if not 0 <= inset <= L.LAYOUT_MAX_INSET:
        raise ValueError("inset in 0..16")
    return L.CtdLayoutParams(int(inset), 0, 0, 0)


def box_anchors(boxes, shapes) -> np.ndarray:
    """(n, 2) i64 x, y: the centres ((x1 + x2) >> 1, (y1 + y2) >> 1) of the blocks' boxes clipped to their pages, blocks in
    page order; `boxes[i]` (n_i, 4) xyxy for a page of `shapes[i]` = (H, W)."""
    counts = np.array([len(b) for b in boxes], np.int64)
    if not int(counts.sum()):
        return np.zeros((0, 2), np.int64)
    xy = np.concatenate([np.asarray(b, np.int64).reshape(-1, 4) for b in boxes])
    H = np.repeat(np.array([s[0] for s in shapes], np.int64), counts)
    W = np.repeat(np.array([s[1] for s in shapes], np.int64), counts)
    x1, y1 = np.maximum(xy[:, 0], 0), np.maximum(xy[:, 1], 0)
    x2, y2 = np.minimum(xy[:, 2], W), np.minimum(xy[:, 3], H)
    return np.stack([(x1 + x2) >> 1, (y1 + y2) >> 1], axis=1)


class LayoutBoxes:
    """The result of `layout_boxes`.  Per block, in the order of the `BalloonRegions` it was made from: `index[j] = (page,
    block)`, `rows` the kernel's records (`ROW_DTYPE`), `status[j]` = `_lib.LAYOUT_OK` / `LAYOUT_NO_REGION` (the block has
    no balloon region) / `LAYOUT_EMPTY` (`inset` leaves nothing of the region), `ok[j]` bool, `n_inner[j]` the pixels of the
    region eroded by `inset`, `area[j]` and `rect[j]` x1, y1, x2, y2 in page coordinates (exclusive) of the largest rectangle
    inside it, `a_area[j]` and `a_rect[j]` of the largest one that contains `anchors[j]` (x, y; all 0 where the anchor is no
    pixel of the eroded region).  All 0 where the block is not `ok`."""

    def __init__(self, index, rows, anchors, inset):
        self.index = np.asarray(index, np.int32).reshape(-1, 2)
        self.rows, self.anchors, self.inset = rows, anchors, int(inset)
        if len(self.index) != len(rows) or len(anchors) != len(rows):
            raise ValueError("one index row and one anchor per block")
        self.status = rows["status"]
        self.ok = self.status == L.LAYOUT_OK
        self.n_inner, self.area, self.rect = rows["n_inner"], rows["area"], rows["rect"]
        self.a_area, self.a_rect = rows["a_area"], rows["a_rect"]

    def __len__(self) -> int:
        return len(self.index)

    def __repr__(self) -> str:
        return f"LayoutBoxes({len(self)} blocks, {int(self.ok.sum())} ok, inset {self.inset})"


def layout_boxes(br: BalloonRegions, anchors=None, inset: int = 2, stream: Optional[torch.cuda.Stream] = None) -> LayoutBoxes:
    """The layout boxes of EVERY block of a `BalloonRegions`: one table upload, one `ctd_layout_boxes` launch on `br.bits`
    where they lie, one small download.  anchors: (n, 2) integers, x and y in page coordinates, one per block of `br`; by
    default `br.center`, the centre of mass of the region (-1, -1 where the block is not ok).  inset: the margin to the
    region's outline in pixels, 0 .. 16.  Runs on `stream` (default: the current stream of the bits' device) and waits for the
    result; see `LayoutBoxes`."""
    prm = check_params(inset)
    n = len(br)
    anchors = np.asarray(br.center if anchors is None else anchors)
    if anchors.dtype.kind not in "iu" or anchors.ndim != 2 or anchors.shape != (n, 2):
        raise ValueError("anchors: an (n, 2) integer array, x and y per block")
    anchors = anchors.astype(np.int64)
    if n and (anchors.min() < -2 ** 31 or anchors.max() >= 2 ** 31):
        raise ValueError("anchor beyond int32")
    if n == 0:
        return LayoutBoxes(br.index, np.zeros((0,), ROW_DTYPE), anchors, inset)
    if not torch.cuda.is_available() or not br.bits.is_cuda:
        raise L.CtdError("layout boxes run on the GPU and there is none (no CPU fallback)")
    jobs = np.zeros((n,), JOB_DTYPE)
    jobs["win"], jobs["ax"], jobs["ay"], jobs["word0"] = br.windows, anchors[:, 0], anchors[:, 1], br.word0
    owned = (br.nw * (br.windows[:, 3] - br.windows[:, 1]))[~br.too_large]
    prm.max_words, prm.n_rows = int(owned.max()) if len(owned) else 0, n
    brows = np.ascontiguousarray(br.rows)
    if brows.dtype != BALLOON_ROW_DTYPE:
        raise ValueError("`br.rows` are not balloon rows")
    with PageCall("layout boxes run", (), stream, br.bits.device) as pc:
        # one upload: the jobs, then the balloon rows as the balloon call returned them
        _, (jobs_ptr, brows_ptr) = pc.upload([jobs, brows])
        res = torch.empty((n * ROW_DTYPE.itemsize,), dtype=torch.uint8, device=pc.device)
        L.check(L.lib().ctd_layout_boxes(jobs_ptr, n, brows_ptr, br.bits.data_ptr() if prm.max_words else None, C.byref(prm),
                                         res.data_ptr(), pc.st.cuda_stream), "ctd_layout_boxes")
        rows = pc.rows(res, ROW_DTYPE, n)
    return LayoutBoxes(br.index, rows, anchors, inset)
