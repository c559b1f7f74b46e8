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

`shaped_fit(br, cum, line, gap)` is the step beyond the box: per block the largest candidate size at which its glyph run sets
in line slots that follow the balloon region, ONE `ctd_layout_fit` launch (csrc/kernels_fit.hip) on the same planes; the rule
is stated in include/ctd_hip.h ("shaped fit"), restated in tests/fit_ref.py, DESIGN.md section 4.31 has its limits.  With
`balance=True` the same launch (`ctd_layout_fit_balanced`) also spreads the slack evenly over the lines by a dynamic program in
the block: the header's "balanced lines", restated in tests/balance_ref.py, DESIGN.md section 4.32.
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

__all__ = ["layout_boxes", "LayoutBoxes", "shaped_fit", "ShapedFit", "box_anchors", "check_params", "JOB_DTYPE", "ROW_DTYPE",
           "FIT_JOB_DTYPE", "FIT_CAND_DTYPE", "FIT_ROW_DTYPE", "FIT_BALANCE_DTYPE"]

# numpy views of `ctd_layout_job` / `ctd_layout_row` (include/ctd_hip.h)
JOB_DTYPE = table_dtype(L.CtdLayoutJob)
ROW_DTYPE = table_dtype(L.CtdLayoutRow)
# ... and of `ctd_fit_job` / `ctd_fit_cand` / `ctd_fit_row`
FIT_JOB_DTYPE = table_dtype(L.CtdFitJob)
FIT_CAND_DTYPE = table_dtype(L.CtdFitCand)
FIT_ROW_DTYPE = table_dtype(L.CtdFitRow)
FIT_BALANCE_DTYPE = table_dtype(L.CtdFitBalance)


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
        # set by `TextDetector.layout_boxes(tilt=True)`: per block the frame's angle and pivot, and the tilted regions; `rect`
        # and `a_rect` are then frame coordinates
        self.angle = self.pivot = self.frame = None

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


# ---- shaped fit: text lines that follow each balloon's outline (include/ctd_hip.h, "shaped fit") ------

class ShapedFit:
    """The result of `shaped_fit`.  Per block, in the order of the `BalloonRegions` it was made from: `index[j] = (page,
    block)`, `rows` the kernel's records (`FIT_ROW_DTYPE`), `status[j]` = `_lib.FIT_OK` / `FIT_NO_REGION` / `FIT_NO_TEXT` (no
    run or no candidate) / `FIT_NO_ANCHOR` (`anchors[j]` is no pixel of the region eroded by `inset`) / `FIT_NO_FIT` (no
    candidate sets in 32 lines), `ok[j]` bool, `cand[j]` the index of the largest candidate that fits, `n_lines[j]` its
    lines, `n_inner[j]` the pixels of the eroded region, and `lines[j]` (32, 5) int32: per line the start glyph, the slot's
    x1 and the line's top row in page coordinates, the slot's width and the length of the line's advances; 0 beyond
    `n_lines[j]`.  All 0 where the block is not `ok`.  `balanced[j]` bool: the block's lines are the balanced ones
    (`shaped_fit(balance=True)` and an admissible vector exists), `cost[j]` int64 the sum of the squared slacks of the lines
    written; all False and 0 from a call without `balance`, where `bal_rows` (`FIT_BALANCE_DTYPE`) is None."""

    def __init__(self, index, rows, anchors, inset, bal_rows=None):
        self.index = np.asarray(index, np.int32).reshape(-1, 2)
        self.rows, self.anchors, self.inset, self.bal_rows = rows, anchors, int(inset), bal_rows
        if len(self.index) != len(rows) or len(anchors) != len(rows) or (bal_rows is not None and len(bal_rows) != len(rows)):
            raise ValueError("one index row and one anchor per block")
        self.balanced = np.zeros((len(rows),), bool) if bal_rows is None else bal_rows["balanced"] != 0
        self.cost = np.zeros((len(rows),), np.int64) if bal_rows is None else bal_rows["cost"].astype(np.int64)
        self.status = rows["status"]
        self.ok = self.status == L.FIT_OK
        self.cand, self.n_lines, self.n_inner = rows["cand"], rows["n_lines"], rows["n_inner"]
        self.lines = np.ascontiguousarray(rows["lines"]).view(np.int32).reshape(len(rows), L.FIT_MAX_LINES, 5)

    def __len__(self) -> int:
        return len(self.index)

    def __repr__(self) -> str:
        return f"ShapedFit({len(self)} blocks, {int(self.ok.sum())} ok, inset {self.inset})"


def _per_cand(v, counts, what) -> np.ndarray:
    """`line` / `gap` of `shaped_fit` as one int64 per candidate row: an integer for all, a 1-D array shared by every block
    that has candidates, or one sequence per block."""
    n, total = len(counts), int(counts.sum())
    if isinstance(v, (int, np.integer)) and not isinstance(v, bool):
        return np.full((total,), int(v), np.int64)
    if isinstance(v, np.ndarray) and v.ndim == 1 and v.dtype.kind in "iu":
        if (counts[counts > 0] != len(v)).any():
            raise ValueError(f"{what}: a shared array has one entry per candidate of every block")
        return np.tile(v.astype(np.int64), int((counts > 0).sum()))
    if isinstance(v, np.ndarray) or not isinstance(v, (list, tuple)) or len(v) != n:
        raise ValueError(f"{what}: an integer, a 1-D integer array for all blocks, or one sequence per block")
    parts = [np.zeros((0,), np.int64) if c == 0 else np.asarray(x) for x, c in zip(v, counts)]
    if any(x.ndim != 1 or len(x) != c or (c and x.dtype.kind not in "iu") for x, c in zip(parts, counts)):
        raise ValueError(f"{what}: one integer per candidate of the block")
    return np.concatenate(parts).astype(np.int64) if parts else np.zeros((0,), np.int64)


def fit_tables(cum, line, gap, breaks=None) -> tuple:
    """The tables of a `ctd_layout_fit` call for n blocks, numpy only: (fit jobs `FIT_JOB_DTYPE`, candidates `FIT_CAND_DTYPE`,
    cumulative advances int32, break bytes uint8).  cum[j]: a (C_j, G_j + 1) integer array, row c the run's cumulative
    advances at candidate c (from 0, not decreasing), candidates in ascending order of size -- or None: no text.  line, gap:
    per candidate the line height (>= 1) and the rows between two lines (>= 0); an integer for all, a 1-D array shared by
    every block, or one sequence per block.  breaks: None, or per block None / one truth value per glyph (a line may end
    after this glyph).  ValueError for anything else."""
    n = len(cum)
    arrs = [np.zeros((0, 1), np.int64) if c is None else np.asarray(c) for c in cum]
    if any(a.ndim != 2 or a.shape[1] < 1 or (a.size and a.dtype.kind not in "iu") for a in arrs):
        raise ValueError("cum: per block a (C, G + 1) integer array or None")
    C_ = np.array([a.shape[0] for a in arrs], np.int64).reshape(n)
    G = np.array([a.shape[1] - 1 for a in arrs], np.int64).reshape(n)
    G[C_ == 0] = 0
    if n and (C_.max() > L.FIT_MAX_CANDS or G.max() > L.FIT_MAX_GLYPHS):
        raise ValueError(f"at most {L.FIT_MAX_CANDS} candidates and {L.FIT_MAX_GLYPHS} glyphs a block")
    flat = np.concatenate([a.reshape(-1) for a in arrs]).astype(np.int64) if n else np.zeros((0,), np.int64)
    row_len = np.repeat(G + 1, C_)                          # one entry per candidate row
    row0 = np.cumsum(row_len) - row_len
    if len(flat):
        step = np.diff(flat)
        step[row0[1:] - 1] = 0                              # from one row to the next
        if flat[row0].any() or (step < 0).any() or flat.max() >= 2 ** 31:
            raise ValueError("cum: every row starts at 0, does not decrease and fits int32")
    line, gap = _per_cand(line, C_, "line"), _per_cand(gap, C_, "gap")
    if len(line) and (line.min() < 1 or gap.min() < 0 or line.max() >= 2 ** 31 or gap.max() >= 2 ** 31):
        raise ValueError("line >= 1, gap >= 0")
    jobs, cands = np.zeros((n,), FIT_JOB_DTYPE), np.zeros((len(row_len),), FIT_CAND_DTYPE)
    jobs["n_glyphs"], jobs["n_cands"], jobs["cand0"], jobs["break0"] = G, C_, np.cumsum(C_) - C_, -1
    cands["line"], cands["gap"], cands["cum0"] = line, gap, row0
    brk = np.zeros((0,), np.uint8)
    if breaks is not None:
        if len(breaks) != n:
            raise ValueError("breaks: None, or one entry per block")
        has = np.array([b is not None for b in breaks], bool).reshape(n)
        parts = [np.asarray(b).astype(bool) for b in breaks if b is not None]
        if any(p.shape != (g,) for p, g in zip(parts, G[has])):
            raise ValueError("breaks: one truth value per glyph of the block")
        size = G[has]
        jobs["break0"][has] = np.cumsum(size) - size
        brk = np.concatenate(parts).astype(np.uint8) if parts else brk
    return jobs, cands, flat.astype(np.int32), brk


def shaped_fit(br: BalloonRegions, cum, line, gap, breaks=None, anchors=None, inset: int = 2,
               stream: Optional[torch.cuda.Stream] = None, balance: bool = False) -> ShapedFit:
    """The shaped fit of EVERY block of a `BalloonRegions`: per block the largest candidate size at which its glyph run sets
    in line slots that follow the balloon region, symmetric about the anchor's column -- one table upload, one
    `ctd_layout_fit` launch on `br.bits` where they lie, one small download.  cum, line, gap, breaks: one entry per block
    of `br`, see `fit_tables`.  anchors and inset as `layout_boxes`; add the text's stroke radius to `inset`.  Runs on `stream`
    (default: the current stream of the bits' device) and waits for the result; see `ShapedFit`.  balance=True: the launch
    is `ctd_layout_fit_balanced`'s, which keeps every block's size, line count and slots and moves the line ends to the
    admissible breaks of least summed squared slack (the greedy lines stand where there are none); its scratch is one
    allocation of `ctd_layout_fit_work_bytes` on the call's stream."""
    check_params(inset)
    if not isinstance(balance, (bool, np.bool_)):
        raise ValueError("balance is a bool")
    n = len(br)
    if len(cum) != n:
        raise ValueError("cum: one entry per block")
    anchors = np.asarray(br.center if anchors is None else anchors)
    if anchors.dtype.kind not in "iu" or anchors.ndim != 2 or anchors.shape != (n, 2):
        raise ValueError("anchors: an (n, 2) integer array, x and y per block")
    anchors = anchors.astype(np.int64)
    if n and (anchors.min() < -2 ** 31 or anchors.max() >= 2 ** 31):
        raise ValueError("anchor beyond int32")
    fjobs, cands, flat, brk = fit_tables(cum, line, gap, breaks)
    if n == 0:
        return ShapedFit(br.index, np.zeros((0,), FIT_ROW_DTYPE), anchors, inset,
                         np.zeros((0,), FIT_BALANCE_DTYPE) if balance else None)
    if not torch.cuda.is_available() or not br.bits.is_cuda:
        raise L.CtdError("the shaped fit runs on the GPU and there is none (no CPU fallback)")
    jobs = np.zeros((n,), JOB_DTYPE)
    jobs["win"], jobs["ax"], jobs["ay"], jobs["word0"] = br.windows, anchors[:, 0], anchors[:, 1], br.word0
    owned = (br.nw * (br.windows[:, 3] - br.windows[:, 1]))[~br.too_large]
    prm = L.CtdFitParams(int(inset), int(owned.max()) if len(owned) else 0, n, len(cands), len(flat), len(brk))
    brows = np.ascontiguousarray(br.rows)
    if brows.dtype != BALLOON_ROW_DTYPE:
        raise ValueError("`br.rows` are not balloon rows")
    with PageCall("the shaped fit runs", (), stream, br.bits.device) as pc:
        # one upload: the two job tables, the balloon rows as the balloon call returned them, candidates, advances, breaks
        _, ptr = pc.upload([jobs, fjobs, brows, cands, flat, brk])
        args = (ptr[0], ptr[1], n, ptr[2], br.bits.data_ptr() if prm.max_words else None, ptr[3] if len(cands) else None,
                ptr[4] if len(flat) else None, ptr[5] if len(brk) else None, C.byref(prm))
        if not balance:
            res = torch.empty((n * FIT_ROW_DTYPE.itemsize,), dtype=torch.uint8, device=pc.device)
            L.check(L.lib().ctd_layout_fit(*args, res.data_ptr(), pc.st.cuda_stream), "ctd_layout_fit")
            rows, bal_rows = pc.rows(res, FIT_ROW_DTYPE, n), None
        else:
            need = int(L.lib().ctd_layout_fit_work_bytes(fjobs.ctypes.data, n))
            if need < 0:
                raise L.CtdError("ctd_layout_fit_work_bytes refused the job table")
            # one allocation: the rows, the balance rows right behind them (656 n is a multiple of 8), the scratch
            at = n * FIT_ROW_DTYPE.itemsize
            res, work = pc.outputs([(at + n * FIT_BALANCE_DTYPE.itemsize,), (need,)])
            L.check(L.lib().ctd_layout_fit_balanced(*args, res.data_ptr(), res.data_ptr() + at, work.data_ptr() if need else None,
                                                    need, pc.st.cuda_stream), "ctd_layout_fit_balanced")
            both = pc.rows(res, np.uint8, len(res))         # one download for both tables
            rows, bal_rows = both[:at].view(FIT_ROW_DTYPE), both[at:].view(FIT_BALANCE_DTYPE)
    return ShapedFit(br.index, rows, anchors, inset, bal_rows)
