"""Balloon regions: the free area around every block that stands on a plain background, on the GPU.

After the original text is erased, a comic-translation caller puts the translated text back, and for that it needs the
extent of the area the old text stood in: the balloon.  Downstream tools flood-fill on the host, page by page and block by
block, from the text outwards over pixels of the balloon's colour and read the fill's bounding box, area and centre.  The
detector already holds what decides the region -- the page, the refined text mask, the block boxes and, since `erase_text`,
per block "this background is one colour" and that colour -- so

    br = balloon_regions(pages, masks, blk_lists)       # or TextDetector.balloons(pages, results[, erased=er])
    br.ok[j], br.area[j], br.bbox[j], br.center[j], br.flags[j], br.mask(j)

builds the tables with numpy, uploads them once, makes ONE `ctd_balloon_regions` call (csrc/kernels_balloon.hip: one launch,
one workgroup per block, the window's bit planes in LDS) -- after the erase stats launch on the same stream where no
`ErasedPages` is passed in -- and downloads one small table; the regions themselves stay on the device as bit planes.  The
rule is integers only and stated in include/ctd_hip.h (restated in numpy with a queue flood fill in tests/balloon_ref.py;
DESIGN.md section 4.18 has its limits): in a window around the block's box, the pixels within `tol` of the erase row's median
in every channel, plus the block's own filled glyphs, are open; the region is what is 4-connected to the glyphs through open
pixels.  There is no per-block Python and no CPU fallback: without a GPU it raises `CtdError` like the rest of the package.

A block that does not stand on a plain background -- a caption on screentone, narration over artwork, a sound effect -- has no
balloon: it comes back `BALLOON_NOT_PLAIN`, and layout and typeset skip it although the fill calls removed its text.  With
`footprint=True` a second launch (`ctd_balloon_footprints`, csrc/kernels_footprint.hip) follows the balloon launch on the same
stream, with the same uploaded tables, and gives every such block (erase row TEXTURED or NO_RING) the place where its old text
stood as its region: the orthogonally convex closure of its filled glyphs, grown by `pad`, minus other blocks' text -- written
into the same rows and the same bit buffer as an OK row with `_lib.BALLOON_FOOTPRINT` in its flags, so `layout_boxes`,
`shaped_fit` and the typeset calls run on it unchanged (`BalloonRegions.footprint[j]`).

A block set at an angle wants its box in its own frame, not the small upright one inside a slanted balloon:
`tilt_regions(br, angles)` turns every region into its block's frame in ONE `ctd_balloon_tilt` launch (csrc/kernels_tilt.hip)
-- the same windows and word layout in a second bit buffer, an ordinary `BalloonRegions` that the layout calls take as it
stands -- and the typeset calls turn the text back (`TextDetector.layout_boxes(tilt=True)`).
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib as L
from . import erase as E
from .pagecall import Page, PageCall, blk_lists_of, check_pages, check_pitch, table_dtype

__all__ = ["balloon_regions", "BalloonRegions", "balloon_tables", "check_params", "check_footprint", "JOB_DTYPE", "ROW_DTYPE",
           "tilt_regions", "cs_of", "check_angles", "TILT_JOB_DTYPE"]

# numpy views of `ctd_balloon_job` / `ctd_balloon_row` (include/ctd_hip.h); the page table is `erase.PAGE_DTYPE`
JOB_DTYPE = table_dtype(L.CtdBalloonJob)
ROW_DTYPE = table_dtype(L.CtdBalloonRow)
TILT_JOB_DTYPE = table_dtype(L.CtdTiltJob)


def check_params(grow, tol, reach, reach_min) -> L.CtdBalloonParams:
    vals = (grow, tol, reach, reach_min)
    if not all(isinstance(v, (int, np.integer)) and not isinstance(v, bool) for v in vals):
        raise ValueError("grow, tol, reach and reach_min are integers")
    if not (0 <= grow <= L.ERASE_MAX_GROW and 0 <= tol <= 255 and 0 <= reach <= L.BALLOON_MAX_REACH
            and L.BALLOON_MIN_REACH_MIN <= reach_min <= L.BALLOON_MAX_REACH_MIN):
        raise ValueError("grow in 0..8, tol in 0..255, reach in 0..32, reach_min in 8..1024")
    return L.CtdBalloonParams(int(grow), int(tol), int(reach), int(reach_min), 0)


def check_footprint(footprint, pad) -> None:
    """`footprint` is a bool and `pad` an integer in 0 .. `FOOTPRINT_MAX_PAD`, whether or not footprints are asked for."""
    if not isinstance(footprint, (bool, np.bool_)):
        raise ValueError("footprint is a bool")
    if not isinstance(pad, (int, np.integer)) or isinstance(pad, (bool, np.bool_)) or not 0 <= pad <= L.FOOTPRINT_MAX_PAD:
        raise ValueError("pad is an integer in 0..16")


def balloon_tables(boxes: Sequence[np.ndarray], shapes: Sequence, reach: int = 8, reach_min: int = 32) -> tuple:
    """What the host decides from the boxes alone, for pages of `shapes` = (H, W) with `boxes[i]` (n_i, 4), blocks in page
    order: (windows (n, 4) i64 x1, y1, x2, y2 in page coordinates, x2 and y2 exclusive, all 0 where the clipped box is empty;
    nw (n,) words a window row; word0 (n,) the block's first word of the bit buffer; the buffer's word count; too_large (n,)
    bool: the window holds more than `BALLOON_MAX_WORDS` words and the block owns none)."""
    check_params(0, 0, reach, reach_min)
    counts = np.array([len(b) for b in boxes], np.int64)
    n = int(counts.sum())
    win = np.zeros((n, 4), np.int64)
    if n:
        xy = np.concatenate([np.asarray(b, np.int64).reshape(-1, 4) for b in boxes])
        H = np.repeat(np.array([s[0] for s in shapes], np.int64), counts)
        W = np.repeat(np.array([s[1] for s in shapes], np.int64), counts)
        x1, y1 = np.maximum(xy[:, 0], 0), np.maximum(xy[:, 1], 0)
        x2, y2 = np.minimum(xy[:, 2], W), np.minimum(xy[:, 3], H)
        some = (x1 < x2) & (y1 < y2)
        ex = np.maximum(reach_min, ((x2 - x1) * reach) >> 3)
        ey = np.maximum(reach_min, ((y2 - y1) * reach) >> 3)
        win = np.stack([np.maximum(x1 - ex, 0), np.maximum(y1 - ey, 0), np.minimum(x2 + ex, W), np.minimum(y2 + ey, H)], axis=1)
        win[~some] = 0
    nw = (win[:, 2] - win[:, 0] + 63) >> 6
    words = nw * (win[:, 3] - win[:, 1])
    too_large = words > L.BALLOON_MAX_WORDS
    owned = np.where(too_large, 0, words)
    return win, nw, np.cumsum(owned) - owned, int(owned.sum()), too_large


class BalloonRegions:
    """The result of `balloon_regions`.  Per block, in order: `index[j] = (page, block)`, `rows` the kernel's records
    (`ROW_DTYPE`), `status[j]` = `_lib.BALLOON_OK` / `BALLOON_NOT_PLAIN` (the erase rule does not call the block's background
    one colour: no region) / `BALLOON_TOO_LARGE` (the window holds more than 8192 words), `ok[j]` bool, `area[j]` pixels,
    `bbox[j]` x1, y1, x2, y2 in page coordinates (exclusive), `center[j]` = (sum_x // area, sum_y // area) where `ok`, else
    -1, `flags[j]`: bits 0..3 (`_lib.BALLOON_CUT_LEFT / TOP / RIGHT / BOTTOM`) the region reaches that side of its window --
    it was cut by the window, or it leaked through a gap in the balloon's outline -- bits 4..7 the same where that side is
    the page's edge; bit 8 (`_lib.BALLOON_FOOTPRINT`) the region is the block's footprint, not a balloon: `footprint[j]` bool
    (`balloon_regions(..., footprint=True)`: where the old text stood, for a block off a plain background; `erase_rows[j]` says
    TEXTURED or NO_RING there).  `windows[j]` x1, y1, x2, y2 of the block's window, `nw[j]`, `word0[j]`: its words in
    `bits`, the device
    u64 buffer of all regions (window row y, columns 64 k .. 64 k + 63 in word `word0 + y * nw + k`, least significant bit
    first); `mask(j)` unpacks one.  `erase_rows`: the blocks' `erase.ROW_DTYPE` rows that decided plain / not plain."""

    def __init__(self, index, rows, windows, nw, word0, too_large, bits, erase_rows):
        self.index = np.asarray(index, np.int32).reshape(-1, 2)
        self.rows, self.windows, self.nw, self.word0, self.too_large = rows, windows, nw, word0, too_large
        self.bits, self.erase_rows = bits, erase_rows
        if len(self.index) != len(rows):
            raise ValueError("one index row per block")
        self.status = rows["status"]
        self.ok = self.status == L.BALLOON_OK
        self.area, self.bbox, self.flags = rows["area"], rows["bbox"], rows["flags"]
        self.footprint = (self.flags & L.BALLOON_FOOTPRINT) != 0
        self.shapes = None                                     # (H, W) per page, where `balloon_regions` made the regions
        self.angle = self.pivot = self.cs = None               # set by `tilt_regions`: the regions are in the blocks' frames
        den = np.where(self.ok, np.maximum(rows["area"], 1), 1).astype(np.int64)
        self.center = np.where(self.ok[:, None], np.stack([rows["sum_x"] // den, rows["sum_y"] // den], axis=1), -1)

    def __len__(self) -> int:
        return len(self.index)

    def mask(self, j: int) -> torch.Tensor:
        """Block j's region as a (wh, ww) bool device tensor over its window (all False where the block is not `ok`)."""
        x1, y1, x2, y2 = (int(v) for v in self.windows[j])
        if self.too_large[j]:
            raise ValueError("the block's window is too large: it has no bits")
        nw, w0 = int(self.nw[j]), int(self.word0[j])
        words = self.bits.view(torch.int64)[w0: w0 + nw * (y2 - y1)].view(y2 - y1, nw, 1)
        shifts = torch.arange(64, device=words.device, dtype=torch.int64)
        return ((words >> shifts) & 1).bool().view(y2 - y1, nw * 64)[:, : x2 - x1]

    def to_host(self):
        """(rows, bits) as numpy arrays; bits is u64."""
        return self.rows, self.bits.view(torch.int64).cpu().numpy().view(np.uint64)

    def __repr__(self) -> str:
        return f"BalloonRegions({len(self)} blocks, {int(self.ok.sum())} ok)"


def balloon_regions(pages: Sequence[Page], masks: Sequence[Page], blk_lists: Sequence, erased: Optional[E.ErasedPages] = None,
                    grow: int = 2, tol: int = 12, reach: int = 8, reach_min: int = 32,
                    stream: Optional[torch.cuda.Stream] = None, device=None, footprint: bool = False,
                    pad: int = L.FOOTPRINT_DEFAULT_PAD) -> BalloonRegions:
    """The balloon region of EVERY block of EVERY page of a batch: one table upload, one `ctd_balloon_regions` launch, one
    small download.  pages, masks, blk_lists as for `erase.erase_text`.  erased: the `ErasedPages` of an `erase_text` call
    on the same pages, masks and blocks with the same `grow` (its rows are uploaded); without it the erase rule's stats launch
    runs first on the same stream, with `grow`, `tol` and the erase defaults, and its rows never leave the device in between.
    grow: as in `erase_text`; tol: how far from the block's background colour an open pixel may lie, per channel; reach: the
    window is the box grown by reach / 8 of its side, but at least by reach_min pixels.  footprint: a second launch,
    `ctd_balloon_footprints`, follows on the same stream with the same tables and gives every block whose erase row is
    TEXTURED or NO_RING the place where its old text stood as its region (OK, `BALLOON_FOOTPRINT` in its flags), grown by
    `pad` pixels (0 .. 16); off, the call launches and returns what it always did.  Runs on `stream` (default: the current
    stream of the pages' device) and waits for the result; see `BalloonRegions`."""
    prm = check_params(grow, tol, reach, reach_min)
    check_footprint(footprint, pad)
    if len(pages) != len(blk_lists) or len(masks) != len(pages):
        raise ValueError("one mask and one blk_list per page")
    check_pages(pages, masks, "BGR ")
    boxes = [E._page_boxes(b) for b in blk_lists_of(blk_lists)]
    shapes = [tuple(p.shape[:2]) for p in pages]
    ejobs, block0, counts, _, _ = E.erase_tables(boxes, shapes)
    n, n_pages = len(ejobs), len(pages)
    index = np.stack([ejobs["page"], np.arange(n) - np.repeat(block0, counts)], axis=1).astype(np.int32) if n else \
        np.zeros((0, 2), np.int32)
    if erased is not None and (len(erased) != n or not np.array_equal(erased.index, index)):
        raise ValueError("`erased` is not the result of erase_text on these pages and blocks")
    win, nw, word0, total, too_large = balloon_tables(boxes, shapes, reach, reach_min)
    if total >= 2 ** 31:
        raise ValueError("too many window words for one call")
    if n_pages == 0:
        return BalloonRegions(index, np.zeros((0,), ROW_DTYPE), win, nw, word0, too_large, torch.zeros((0,), dtype=torch.uint64),
                              np.zeros((0,), E.ROW_DTYPE))
    rs = E.ROW_DTYPE.itemsize
    with PageCall("balloon regions run", pages, stream, device) as pc:
        P, M = pc.pages(pages), pc.pages(masks)
        check_pitch(3 * P.W)
        jt = np.zeros((n,), JOB_DTYPE)
        jt["page"], jt["xyxy"], jt["erase_row"], jt["word0"] = ejobs["page"], ejobs["xyxy"], np.arange(n), word0
        erows_up = np.ascontiguousarray(erased.rows) if erased is not None else np.zeros((0,), E.ROW_DTYPE)
        # one upload: erase jobs, balloon jobs, pages, and the erase rows where the caller has them
        _, (ejobs_ptr, jobs_ptr, pages_ptr, erows_ptr) = pc.upload([ejobs, jt, E.page_table(P, M, block0, counts), erows_up])
        # one buffer behind both row tables: balloon rows, then erase rows
        res = torch.empty((max(n, 1) * (ROW_DTYPE.itemsize + rs),), dtype=torch.uint8, device=pc.device)
        bits = torch.empty((max(total, 1),), dtype=torch.int64, device=pc.device)[:total].view(torch.uint64)
        if n:
            lib = L.lib()
            if erased is None:
                eprm = E.check_params(grow, 4, tol, 16)             # n_tiles = 0: the stats launch alone
                erows_ptr = res.data_ptr() + n * ROW_DTYPE.itemsize
                L.check(lib.ctd_erase_text(ejobs_ptr, n, pages_ptr, n_pages, C.byref(eprm), erows_ptr, pc.st.cuda_stream),
                        "ctd_erase_text")
            owned = (nw * (win[:, 3] - win[:, 1]))[~too_large]
            prm.max_words = int(owned.max()) if len(owned) else 0
            L.check(lib.ctd_balloon_regions(jobs_ptr, n, pages_ptr, n_pages, erows_ptr, C.byref(prm), res.data_ptr(),
                                            bits.data_ptr() if total else None, pc.st.cuda_stream), "ctd_balloon_regions")
            if footprint:                                           # the same tables, rows and bits, no host step between
                fprm = L.CtdFootprintParams(prm.grow, int(pad), prm.reach, prm.reach_min, prm.max_words)
                L.check(lib.ctd_balloon_footprints(jobs_ptr, n, pages_ptr, n_pages, erows_ptr, C.byref(fprm), res.data_ptr(),
                                                   bits.data_ptr() if total else None, pc.st.cuda_stream),
                        "ctd_balloon_footprints")
        host = pc.rows(res, np.uint8, n * (ROW_DTYPE.itemsize + rs))
    rows = host[: n * ROW_DTYPE.itemsize].view(ROW_DTYPE)
    erows = erased.rows if erased is not None else host[n * ROW_DTYPE.itemsize: n * (ROW_DTYPE.itemsize + rs)].view(E.ROW_DTYPE)
    if erased is not None and not np.array_equal(rows["n_seed"][rows["status"] == L.BALLOON_OK],
                                                 erows["n_fill"][rows["status"] == L.BALLOON_OK]):
        raise ValueError("`erased` was made with another `grow`, or from other pages, masks or blocks")
    out = BalloonRegions(index, rows, win, nw, word0, too_large, bits, erows)
    out.shapes = shapes
    return out


# ---- tilted regions (include/ctd_hip.h, "tilted text") ------------------------------------------------------

def check_angles(angles, n: int, what: str = "angles") -> np.ndarray:
    """`angles` as (n,) int64: one whole number of degrees in -180 .. 180 per item; ValueError otherwise."""
    a = np.asarray(angles)
    if a.dtype.kind not in "iu" or a.dtype == bool or a.shape != (n,):
        raise ValueError(f"{what}: one integer per block")
    a = a.astype(np.int64)
    if n and (a.min() < -180 or a.max() > 180):
        raise ValueError(f"{what}: -180 .. 180 degrees")
    return a


def cs_of(angles) -> np.ndarray:
    """(n, 2) int64: c = rint(cos 65536), s = rint(sin 65536) of whole degrees.  No product lies nearer than 0.004 to a
    rounding tie, so the table does not depend on the libm (tests/test_tilt_ref.py pins it)."""
    t = np.deg2rad(np.asarray(angles, np.float64))
    return np.stack([np.rint(np.cos(t) * 65536), np.rint(np.sin(t) * 65536)], axis=-1).astype(np.int64).reshape(-1, 2)


def tilt_regions(br: BalloonRegions, angles, pivots=None, stream: Optional[torch.cuda.Stream] = None) -> BalloonRegions:
    """The regions of a `BalloonRegions` turned into their blocks' own frames: one table upload, one `ctd_balloon_tilt`
    launch (csrc/kernels_tilt.hip) on `br.bits` where they lie, one small download.  angles: one integer per block, degrees,
    -180 .. 180 (a detected block's `angle`); pivots: (n, 2) integers, x and y in page coordinates, about which each block
    turns (default: the centre of its window).  `br.shapes[p]` = (H, W) of page p, as `balloon_regions` leaves it, decides
    whether a cut flag names a window side or the page's edge (None: the right and bottom sides are never one).  The result is an ordinary
    `BalloonRegions` in FRAME coordinates -- the same index, windows, nw, word0, too_large and erase_rows, new rows and a new
    bit buffer, `_lib.BALLOON_TILTED` in the flags of every ok row -- so `layout.layout_boxes` and `layout.shaped_fit` take
    it as it stands; it also carries `angle`, `pivot` and `cs` (the 16.16 pairs), which the typeset calls need to turn the
    text back.  Frame pixel q of a window is set iff the page pixel nearest to frame -> page (q) is in the window and in the
    region.  Bad arguments raise ValueError before anything is uploaded."""
    n = len(br)
    angles = check_angles(angles, n)
    if pivots is None:
        pivots = np.stack([(br.windows[:, 0] + br.windows[:, 2]) >> 1, (br.windows[:, 1] + br.windows[:, 3]) >> 1], axis=1)
    pivots = np.asarray(pivots)
    if pivots.dtype.kind not in "iu" or pivots.shape != (n, 2):
        raise ValueError("pivots: an (n, 2) integer array, x and y per block")
    pivots = pivots.astype(np.int64)
    if n and np.abs(pivots).max() > 1 << 29:
        raise ValueError("pivot beyond 2^29")
    WH = np.full((n, 2), -1, np.int64)                           # no window side is a page's right or bottom edge
    shapes = getattr(br, "shapes", None)
    if shapes is not None:
        hw = np.asarray([tuple(s[:2]) for s in shapes], np.int64).reshape(-1, 2)
        if n and (br.index[:, 0].min() < 0 or br.index[:, 0].max() >= len(hw)):
            raise ValueError("shapes: one (H, W) per page of the regions")
        WH = hw[br.index[:, 0]][:, ::-1] if n else WH
    brows = np.ascontiguousarray(br.rows)
    if brows.dtype != ROW_DTYPE:
        raise ValueError("`br.rows` are not balloon rows")
    cs = cs_of(angles)

    def result(rows, bits):
        out = BalloonRegions(br.index, rows, br.windows, br.nw, br.word0, br.too_large, bits, br.erase_rows)
        out.angle, out.pivot, out.cs, out.shapes = angles, pivots, cs, shapes
        return out

    if n == 0:
        return result(np.zeros((0,), ROW_DTYPE), br.bits)
    if not torch.cuda.is_available() or not br.bits.is_cuda:
        raise L.CtdError("tilted regions run on the GPU and there is none (no CPU fallback)")
    jobs = np.zeros((n,), TILT_JOB_DTYPE)
    jobs["win"], jobs["ax"], jobs["ay"], jobs["c"], jobs["s"] = br.windows, pivots[:, 0], pivots[:, 1], cs[:, 0], cs[:, 1]
    jobs["W"], jobs["H"], jobs["word0"] = WH[:, 0], WH[:, 1], br.word0
    owned = (br.nw * (br.windows[:, 3] - br.windows[:, 1]))[~br.too_large]
    prm = L.CtdTiltParams(int(owned.max()) if len(owned) else 0)
    with PageCall("tilted regions run", (), stream, br.bits.device) as pc:
        _, (jobs_ptr, brows_ptr) = pc.upload([jobs, brows])     # one upload: the jobs, then the balloon rows
        res = torch.empty((n * ROW_DTYPE.itemsize,), dtype=torch.uint8, device=pc.device)
        bits = torch.empty((max(br.bits.numel(), 1),), dtype=torch.int64, device=pc.device)[: br.bits.numel()].view(torch.uint64)
        L.check(L.lib().ctd_balloon_tilt(jobs_ptr, n, brows_ptr, br.bits.data_ptr() if prm.max_words else None, C.byref(prm),
                                         res.data_ptr(), bits.data_ptr() if prm.max_words else None, pc.st.cuda_stream),
                "ctd_balloon_tilt")
        rows = pc.rows(res, ROW_DTYPE, n)
    return result(rows, bits)
