"""OCR line crops on the GPU: the reference's `TextBlock.get_transformed_region` (utils/textblock.py:162-194), batched.

The OCR stage downstream of the detector takes one perspective-rectified crop per text line, `textheight` pixels high.
The reference makes them one at a time with cv2 on the host (findHomography + warpPerspective [+ rotate for vertical
blocks]).  Here the pages are already in HBM and the line quads already in the batch's record arrays, so

    regs = line_regions(pages, blk_lists, textheight=48)        # or TextDetector.line_regions(pages, results)

computes every line's crop size and homography in ONE native host call (`ctd_region_transforms`, csrc/host_region.cpp),
builds a job table with numpy, uploads it once and warps all crops in ONE kernel launch (`ctd_warp_regions`,
csrc/kernels_region.hip) into one packed device buffer: crops back to back, each (textheight, width_i, C) contiguous.
Packed, not padded: one 2000-px line would otherwise size every crop of the batch; `LineRegions.padded(width)` makes the
(N, textheight, width, C) tensor an OCR network wants when asked.  There is no per-line Python in this path and no CPU
fallback: without a GPU it raises `CtdError` like the rest of the package.

An OCR network reads float tensors (N, C, textheight, W), normalised, the lines sorted by width and cut into chunks, each
chunk padded to its own widest line.  `line_batches` writes exactly those tensors in the same single launch
(`ctd_warp_region_batches`): warp, value table, layout and padding fused, no packed intermediate; `batch_plan` is the
bucketing (host, numpy).

What is restated from cv2 here (four-point homography, the fixed-point linear warp) is listed in DESIGN.md section 5.
"""
from __future__ import annotations

from collections import namedtuple
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import _lib as L
from .pagecall import Page, PageCall, table_dtype
from .pagecall import align as _align, check_pages as _check_pages, device_pages as _device_pages, views as _views  # noqa: F401
# (the underscore names: plain aliases, kept for the tests that import them)
from .textblock import LANGCLS2IDX, BlockList, TextBlock

__all__ = ["line_regions", "LineRegions", "transforms", "warp", "JOB_DTYPE", "line_batches", "LineBatches", "batch_plan",
           "BatchPlan", "value_tables", "warp_batches", "BATCH_JOB_DTYPE"]

# numpy views of `ctd_region_job` / `ctd_region_batch_job` (include/ctd_hip.h)
JOB_DTYPE = table_dtype(L.CtdRegionJob)
BATCH_JOB_DTYPE = table_dtype(L.CtdRegionBatchJob)


def transforms(quads, language, vertical, font_size, im_w, im_h, textheight=48):
    """Crop size and homography of n text lines (`ctd_region_transforms`; host code, needs no GPU).  quads (n,4,2) or (n,8)
    integers; language (0 eng / 1 ja / 2 unknown), vertical, font_size: per line, from the line's block; im_w / im_h: per
    line or one for all.  Returns wh (n,2) i32 = (w, h) of the warp before the rotation of vertical lines, M (n,3,3) f64
    page -> crop, Minv (n,3,3) f64, status (n) i32 (`_lib.REGION_OK` / `_lib.REGION_DEGENERATE`)."""
    q = np.ascontiguousarray(np.asarray(quads, np.int32).reshape(-1, 8))
    n = len(q)
    lang = np.ascontiguousarray(np.broadcast_to(np.asarray(language, np.int32), (n,)))
    vert = np.ascontiguousarray(np.broadcast_to(np.asarray(vertical).astype(np.int32), (n,)))
    fs = np.ascontiguousarray(np.broadcast_to(np.asarray(font_size, np.float64), (n,)))
    iw = np.ascontiguousarray(np.broadcast_to(np.asarray(im_w, np.int32), (n,)))
    ih = np.ascontiguousarray(np.broadcast_to(np.asarray(im_h, np.int32), (n,)))
    wh = np.zeros((n, 2), np.int32)
    M = np.zeros((n, 3, 3), np.float64)
    Minv = np.zeros((n, 3, 3), np.float64)
    status = np.zeros((n,), np.int32)
    L.check(L.lib().ctd_region_transforms(q.ctypes.data, lang.ctypes.data, vert.ctypes.data, fs.ctypes.data, iw.ctypes.data,
                                          ih.ctypes.data, n, float(textheight), wh.ctypes.data, M.ctypes.data,
                                          Minv.ctypes.data, status.ctypes.data), "ctd_region_transforms")
    return wh, M, Minv, status


class LineRegions:
    """The crops of `line_regions`: `packed` is ONE uint8 device buffer holding crop i at `offsets[i]` as a contiguous
    (textheight, widths[i], C) array; `index[i] = (page, block, line)` names the line (block = position in the page's
    blk_list, line = position in the block's `lines`); `valid[i]` is False for a degenerate line (the reference raises on it:
    zero size, non-finite ratio, singular homography), which has width 0 and no bytes.  `regs[i]` is the device view of crop i;
    `len(regs)` the number of lines."""

    def __init__(self, packed: torch.Tensor, index: np.ndarray, widths: np.ndarray, offsets: np.ndarray, valid: np.ndarray,
                 textheight: int, channels: int, keep=None):
        self.packed, self.index, self.widths, self.offsets, self.valid = packed, index, widths, offsets, valid
        self.textheight, self.channels = int(textheight), int(channels)
        self._keep = keep                                # the pages the launch reads, alive until the crops are dropped

    def __len__(self) -> int:
        return len(self.widths)

    def __getitem__(self, i) -> torch.Tensor:
        i = range(len(self))[i]                          # negative indices, IndexError
        w, o = int(self.widths[i]), int(self.offsets[i])
        return self.packed[o: o + self.textheight * w * self.channels].view(self.textheight, w, self.channels)

    def __iter__(self):
        return (self[i] for i in range(len(self)))

    def padded(self, width: Optional[int] = None) -> torch.Tensor:
        """(N, textheight, width, C) uint8 on the device: every crop in the top-left corner, zeros on its right; a crop wider
        than `width` loses its right end.  Default width: the widest crop.  A handful of launches, whatever N is."""
        n, th, ch = len(self), self.textheight, self.channels
        width = int(self.widths.max()) if (width is None and n) else int(width or 0)
        out = torch.zeros((n, th, width, ch), dtype=torch.uint8, device=self.packed.device)
        if n == 0 or width == 0 or self.packed.numel() == 0:
            return out
        dev = self.packed.device
        nbytes = torch.from_numpy(self.widths.astype(np.int64) * (th * ch)).to(dev)
        crop = torch.repeat_interleave(torch.arange(n, device=dev), nbytes)                  # crop of every packed byte
        row_b = torch.from_numpy(self.widths.astype(np.int64) * ch).to(dev)[crop]            # bytes per row of that crop
        local = torch.arange(self.packed.numel(), device=dev) - torch.from_numpy(self.offsets.astype(np.int64)).to(dev)[crop]
        r, rem = local // row_b, local % row_b
        keep = rem < width * ch
        dst = crop * (th * width * ch) + r * (width * ch) + rem
        out.view(-1)[dst[keep]] = self.packed[keep]
        return out

    def to_host(self) -> List[np.ndarray]:
        """Every crop as a (textheight, width_i, C) numpy array: one download, the arrays are views of it."""
        buf = self.packed.cpu().numpy()
        th, ch = self.textheight, self.channels
        return [buf[o: o + th * w * ch].reshape(th, w, ch) for o, w in zip(self.offsets.tolist(), self.widths.tolist())]

    def __repr__(self) -> str:
        return (f"LineRegions({len(self)} lines, {int((~self.valid).sum())} invalid, textheight {self.textheight}, "
                f"{self.packed.numel()} bytes)")


def warp(pages: Sequence[torch.Tensor], page_of: np.ndarray, wh: np.ndarray, Minv: np.ndarray, rotate: np.ndarray,
         channels: int, stream: Optional[torch.cuda.Stream] = None):
    """`ctd_warp_regions`: crop i = cv2.warpPerspective(pages[page_of[i]], inverse of Minv[i], wh[i]) (INTER_LINEAR, constant
    border 0), turned by 90 degrees counter-clockwise where rotate[i]; crops with wh[i] = (0, 0) are skipped.  `pages`: dense
    uint8 device tensors as `_device_pages` returns them.  ONE launch.  Returns (packed device buffer, offsets, sizes (n,2) =
    (rows, cols) of the stored crops)."""
    n = len(wh)
    wh = np.asarray(wh, np.int64).reshape(n, 2)
    rotate = np.asarray(rotate).astype(bool).reshape(n)
    if n and (wh.min() < 0 or wh.max() > L.REGION_MAX_SIDE or ((wh[:, 0] == 0) != (wh[:, 1] == 0)).any()):
        raise ValueError("crop sizes must be (0, 0) or 1 ... REGION_MAX_SIDE a side")
    pix = wh[:, 0] * wh[:, 1]
    nbytes = pix * channels
    offsets = np.cumsum(nbytes) - nbytes
    total = int(nbytes.sum())
    sizes = np.where(rotate[:, None], wh, wh[:, ::-1])
    tiles = (pix + L.REGION_TILE - 1) // L.REGION_TILE
    n_tiles = int(tiles.sum())
    if n_tiles >= 2 ** 31:
        raise ValueError("too many pixels for one launch")
    with PageCall("line crops run", pages, stream, sync=False) as pc:
        packed = torch.empty((total,), dtype=torch.uint8, device=pc.device)
        if n_tiles == 0:
            return packed, offsets, sizes
        jobs = np.zeros((n,), JOB_DTYPE)
        _fill_jobs(jobs, pc.pages(pages, dense=True), page_of, channels, Minv, wh, rotate)
        jobs["out_off"] = offsets
        _, (jobs_ptr, prefix_ptr) = pc.upload([jobs, _tile_prefix(tiles)])           # jobs, then the tile prefix: one upload
        L.check(L.lib().ctd_warp_regions(jobs_ptr, n, prefix_ptr, n_tiles, packed.data_ptr(), pc.st.cuda_stream),
                "ctd_warp_regions")
    return packed, offsets, sizes


def _fill_jobs(jobs, P, page_of, channels, Minv, wh, rotate) -> None:
    """The page and warp columns of `JOB_DTYPE` rows, which both warp calls fill alike; P: `PageCall.pages` of the pages."""
    page_of = np.asarray(page_of, np.int64).reshape(len(jobs))
    jobs["page_dev"], jobs["H"], jobs["W"], jobs["pitch"], jobs["C"] = P.ptr[page_of], P.H[page_of], P.W[page_of], P.pitch[page_of], channels
    jobs["Minv"] = np.asarray(Minv, np.float64).reshape(len(jobs), 9)
    jobs["w"], jobs["h"], jobs["rotate"] = wh[:, 0], wh[:, 1], rotate


def _tile_prefix(tiles) -> np.ndarray:
    return np.concatenate(([0], np.cumsum(tiles))).astype(np.int32)


def _page_lines(blk_list):
    """Every line of a page in block order, as columns: quads (n,8) i32, language, vertical, font_size of the line's block,
    block index, line index inside the block.  A `BlockList` is read from its record arrays (no `TextBlock` is built)."""
    if isinstance(blk_list, BlockList):
        r = blk_list.records
        nl = r["n_lines"].astype(np.int64)
        blk = np.repeat(np.arange(len(r)), nl)
        within = np.arange(int(nl.sum())) - np.repeat(np.cumsum(nl) - nl, nl)
        quads = blk_list.line_quads.reshape(-1, 8)[r["line_off"].astype(np.int64)[blk] + within]
        # `TextBlock.font_size` is a Python int unless a merge made it a float (textblock.blocks_from_records)
        fs = np.where(r["font_is_float"] != 0, r["font_size"], np.trunc(r["font_size"]))
        return quads.astype(np.int32), r["language"][blk], r["vertical"][blk], fs[blk], blk, within
    quads, lang, vert, fs, counts = [], [], [], [], []
    for b in blk_list:                                   # per BLOCK (a caller's own list of objects), never per line
        q = np.asarray(b.lines, np.float64).reshape(-1, 8)
        if not np.array_equal(q, np.trunc(q)):
            raise ValueError("text lines must have integer coordinates (the detector's quads)")
        quads.append(q.astype(np.int32))
        counts.append(len(q))
        lang.append(LANGCLS2IDX.get(b.language, 1))      # only 'eng' / 'unknown' get the margin (textblock.py:167)
        vert.append(bool(b.vertical))
        fs.append(float(b.font_size))
    counts = np.asarray(counts, np.int64)
    blk = np.repeat(np.arange(len(counts)), counts)
    within = np.arange(int(counts.sum())) - np.repeat(np.cumsum(counts) - counts, counts)
    quads = np.concatenate(quads) if quads else np.zeros((0, 8), np.int32)
    return (quads, np.asarray(lang, np.int32)[blk], np.asarray(vert, bool)[blk], np.asarray(fs, np.float64)[blk], blk, within)


def batch_lines(blk_lists):
    """The lines of every page of a batch as columns: index (n,3) i32 = (page, block, line), quads, language, vertical,
    font_size."""
    cols = [_page_lines(b) for b in blk_lists]
    counts = [len(c[0]) for c in cols]
    cat = lambda k, dt: (np.concatenate([c[k] for c in cols]).astype(dt) if cols else np.zeros((0,), dt))   # noqa: E731
    index = np.stack([np.repeat(np.arange(len(cols)), counts), cat(4, np.int64), cat(5, np.int64)], axis=1).astype(np.int32) \
        if cols else np.zeros((0, 3), np.int32)
    quads = np.concatenate([c[0] for c in cols]) if cols else np.zeros((0, 8), np.int32)
    return index, quads, cat(1, np.int32), cat(2, np.int32), cat(3, np.float64)


def _regions(P, index, quads, lang, vert, fs, textheight) -> LineRegions:
    """Inside the caller's `PageCall`, on its stream; P: its `pages`."""
    pg = index[:, 0]
    wh, _, Minv, status = transforms(quads, lang, vert, fs, P.W[pg] if len(pg) else 0, P.H[pg] if len(pg) else 0, textheight)
    vert = np.asarray(vert).astype(bool)
    packed, offsets, sizes = warp(P.t, pg, wh, Minv, vert, P.C)
    return LineRegions(packed, index, sizes[:, 1].astype(np.int64), offsets, status == L.REGION_OK, int(textheight), P.C,
                       keep=P.t)


def line_regions(pages: Sequence[Page], blk_lists: Sequence, textheight: int = 48,
                 stream: Optional[torch.cuda.Stream] = None, device=None) -> LineRegions:
    """The `get_transformed_region` crops of EVERY line of EVERY block of a batch: one native host call for the transforms,
    one upload, one kernel launch.  pages: uint8 BGR (H,W,3) or grey (H,W) pages of any mix of sizes, on the device or on the
    host (uploaded here); blk_lists[b]: page b's blk_list -- a list of `TextBlock`s or a `BlockList`.  Asynchronous on `stream`
    (default: the current stream of the pages' device); see `LineRegions`."""
    if len(pages) != len(blk_lists):
        raise ValueError("one blk_list per page")
    if textheight < 1 or int(textheight) > L.REGION_MAX_SIDE:
        raise ValueError("textheight out of range")
    with PageCall("line crops run", pages, stream, device, sync=False) as pc:
        return _regions(pc.pages(pages), *batch_lines(blk_lists), textheight)


def transformed_region(blk: TextBlock, img: Page, idx: int, textheight):
    """`TextBlock.get_transformed_region`: one line's crop, a numpy array for a numpy image, a device tensor for a device
    tensor (no host round trip, asynchronous on the current stream)."""
    host = not isinstance(img, torch.Tensor)
    if not host and not img.is_cuda:
        raise L.CtdError("get_transformed_region takes a numpy image or a CUDA tensor (there is no CPU path)")
    with PageCall("line crops run", [img], sync=False) as pc:
        P = pc.pages([img])
        q = np.asarray(blk.lines[idx], np.float64).reshape(1, 8)
        if not np.array_equal(q, np.trunc(q)):
            raise ValueError("text lines must have integer coordinates (the detector's quads)")
        regs = _regions(P, np.zeros((1, 3), np.int32), q.astype(np.int32), [LANGCLS2IDX.get(blk.language, 1)],
                        [bool(blk.vertical)], [float(blk.font_size)], textheight)
        if not regs.valid[0]:
            raise ValueError(f"degenerate text line {blk.lines[idx]}: no region of height {textheight} (zero size, non-finite "
                             "aspect ratio or singular homography)")
        out = regs[0] if P.t[0].dim() == 3 else regs[0][:, :, 0]
        return out.cpu().numpy() if host else out


# ---- OCR input batches ------------------------------------------------------------------------------------------------------

BatchPlan = namedtuple("BatchPlan", "order bounds batch_width cut")
BatchPlan.__doc__ = """`batch_plan`'s record: `order` (M,) i64 the lines in batch order; batch k holds
order[bounds[k]: bounds[k + 1]] and is `batch_width[k]` columns wide; `cut[j]` = the columns kept of line order[j]."""

_NP_DTYPE = {torch.uint8: np.uint8, torch.float16: np.float16, torch.float32: np.float32}
_ABI_DTYPE = {torch.uint8: L.REGION_U8, torch.float16: L.REGION_F16, torch.float32: L.REGION_F32}
_LAYOUT = {"nchw": L.LAYOUT_NCHW, "nhwc": L.LAYOUT_NHWC}


def batch_plan(widths, valid, max_batch: Optional[int] = 16, width_multiple: int = 8, max_width: Optional[int] = None) -> BatchPlan:
    """Width buckets of the lines of a batch (host, numpy, needs no GPU).  The valid lines of width >= 1, sorted by width
    with a STABLE sort (ties keep line order; the sort is on the uncut widths), cut into consecutive runs of at most
    `max_batch` lines (None: one run).  Run k is `batch_width[k]` columns wide: its largest min(width, max_width), rounded up
    to a multiple of `width_multiple`; `cut` = min(width, max_width) per line of `order` (the right end of a longer line is
    lost, as in `LineRegions.padded(width)`).  No valid line: no batch."""
    widths = np.asarray(widths, np.int64).reshape(-1)
    valid = np.asarray(valid).astype(bool).reshape(-1)
    if len(widths) != len(valid):
        raise ValueError("one width and one valid flag per line")
    width_multiple = int(width_multiple)
    if width_multiple < 1 or (max_batch is not None and int(max_batch) < 1) or (max_width is not None and int(max_width) < 1):
        raise ValueError("max_batch, width_multiple and max_width must be >= 1")
    if max_width is not None and int(max_width) % width_multiple:
        raise ValueError("max_width must be a multiple of width_multiple")
    lines = np.nonzero(valid & (widths >= 1))[0].astype(np.int64)
    order = lines[np.argsort(widths[lines], kind="stable")]
    m = len(order)
    cut = widths[order] if max_width is None else np.minimum(widths[order], int(max_width))
    if m == 0:
        return BatchPlan(order, np.zeros((1,), np.int64), np.zeros((0,), np.int64), cut)
    step = m if max_batch is None else int(max_batch)
    bounds = np.append(np.arange(0, m, step, dtype=np.int64), m)
    widest = cut[bounds[1:] - 1]                          # `cut` is non-decreasing along `order`
    return BatchPlan(order, bounds, (widest + width_multiple - 1) // width_multiple * width_multiple, cut)


def value_tables(dtype, channels: int, mean=127.5, std=127.5) -> np.ndarray:
    """(channels, 256) array of `dtype`: table[c][v] = ((v - mean[c]) / std[c]) in float32, converted to `dtype` --
    `((np.arange(256, dtype=np.float32) - mean[c]) / std[c]).astype(dtype)`.  mean / std: a scalar or one value per output
    channel, taken as float32.  uint8: the identity (any other mean / std is a ValueError)."""
    if isinstance(dtype, torch.dtype) and dtype not in _NP_DTYPE:
        raise ValueError("dtype must be uint8, float16 or float32")
    npdt = np.dtype(_NP_DTYPE.get(dtype, dtype))
    if npdt not in (np.dtype(np.uint8), np.dtype(np.float16), np.dtype(np.float32)):
        raise ValueError("dtype must be uint8, float16 or float32")
    mean = np.asarray(mean, np.float32).reshape(-1)
    std = np.asarray(std, np.float32).reshape(-1)
    if len(mean) not in (1, channels) or len(std) not in (1, channels):
        raise ValueError("mean / std: a scalar or one value per output channel")
    if npdt == np.uint8:
        if (mean != np.float32(127.5)).any() or (std != np.float32(127.5)).any():
            raise ValueError("uint8 batches are not normalised: leave mean / std at their defaults")
        return np.tile(np.arange(256, dtype=np.uint8), (channels, 1))
    mean, std = np.broadcast_to(mean, (channels,)), np.broadcast_to(std, (channels,))
    return np.stack([((np.arange(256, dtype=np.float32) - mean[c]) / std[c]).astype(npdt) for c in range(channels)])


def warp_batches(pages: Sequence[torch.Tensor], page_of, wh, Minv, rotate, channels: int, batch_of, slot, cut, batch_n,
                 batch_width, textheight, dtype=torch.float16, layout: str = "nchw", tables: Optional[np.ndarray] = None,
                 rgb: bool = False, pad: int = 0, stream: Optional[torch.cuda.Stream] = None):
    """`ctd_warp_region_batches`: the crops of `warp` (same arguments up to `channels`) written straight into K batch tensors
    in ONE launch.  Job i fills slot `slot[i]` of batch `batch_of[i]` (-1: the job is in no batch) with the first `cut[i]`
    columns of its stored crop; batch k holds `batch_n[k]` slots of `textheight` (one value, or one per batch) rows and
    `batch_width[k]` columns, laid out `layout` with `dtype` elements = tables[c][u8 value] (`value_tables`; channel order
    reversed where `rgb`), `tables[c][pad]` outside the crop.  Returns (storage, offsets): ONE device tensor of `dtype` and
    the element offset of every batch in it, each on a 16-byte boundary.  One upload (jobs, tile prefix, tables)."""
    if not all(isinstance(p, torch.Tensor) and p.is_cuda for p in pages):
        raise L.CtdError("the kernel reads its pages in device memory: CPU tensors cannot be warped (no CPU fallback)")
    n = len(wh)
    wh = np.asarray(wh, np.int64).reshape(n, 2)
    rotate = np.asarray(rotate).astype(bool).reshape(n)
    batch_of = np.asarray(batch_of, np.int64).reshape(n)
    slot = np.asarray(slot, np.int64).reshape(n)
    cut = np.asarray(cut, np.int64).reshape(n)
    batch_n = np.asarray(batch_n, np.int64).reshape(-1)
    batch_width = np.asarray(batch_width, np.int64).reshape(-1)
    K = len(batch_n)
    th = np.broadcast_to(np.asarray(textheight, np.int64), (K,))
    if dtype not in _ABI_DTYPE or layout not in _LAYOUT:
        raise ValueError("dtype: torch.uint8 / float16 / float32; layout: 'nchw' / 'nhwc'")
    if not 0 <= int(pad) <= 255:
        raise ValueError("pad is a uint8 page value")
    if n and (wh.min() < 0 or wh.max() > L.REGION_MAX_SIDE or ((wh[:, 0] == 0) != (wh[:, 1] == 0)).any()):
        raise ValueError("crop sizes must be (0, 0) or 1 ... REGION_MAX_SIDE a side")
    if len(batch_width) != K or (K and (batch_n.min() < 1 or batch_width.min() < 1 or th.min() < 1 or
                                        (th * batch_width).max() >= 2 ** 31)):
        raise ValueError("every batch needs >= 1 slot, >= 1 row and >= 1 column (rows * columns within int32)")
    used = batch_of >= 0
    sizes = np.where(rotate[:, None], wh, wh[:, ::-1])   # (rows, cols) of the stored crops
    bk = batch_of[used]
    if len(bk) and (bk.max() >= K or (slot[used] < 0).any() or (slot[used] >= batch_n[bk]).any() or (cut[used] < 0).any() or
                    (cut[used] > np.minimum(sizes[used, 1], batch_width[bk])).any() or (sizes[used, 0] > th[bk]).any()):
        raise ValueError("a slot outside its batch, or a crop larger than its slot")
    item = torch.empty((), dtype=dtype).element_size()
    elems = batch_n * channels * th * batch_width
    align = 16 // item
    offsets = np.zeros((K,), np.int64)
    total = 0
    for k in range(K):                                   # per BATCH: every batch starts on a 16-byte boundary
        offsets[k] = (total + align - 1) // align * align
        total = int(offsets[k] + elems[k])
    tiles = np.zeros((n,), np.int64)
    tiles[used] = (th[bk] * batch_width[bk] + L.REGION_TILE - 1) // L.REGION_TILE
    n_tiles = int(tiles.sum())
    if n_tiles >= 2 ** 31:
        raise ValueError("too many pixels for one launch")
    with PageCall("line crops run", pages, stream, sync=False) as pc:
        storage = torch.empty((total,), dtype=dtype, device=pc.device)
        if n_tiles == 0:
            return storage, offsets
        P = pc.pages(pages, dense=True)
        if dtype == torch.uint8:
            tables = np.zeros((0,), np.uint8)
        else:
            if tables is None:
                tables = value_tables(dtype, channels)
            tables = np.ascontiguousarray(tables, _NP_DTYPE[dtype])
            if tables.shape != (channels, 256):
                raise ValueError("tables: (channels, 256)")
        rows = np.zeros((n,), BATCH_JOB_DTYPE)
        _fill_jobs(rows["warp"], P, page_of, channels, Minv, wh, rotate)
        safe = np.where(used, batch_of, 0)
        rows["warp"]["out_off"] = np.where(used, offsets[safe] if K else 0, 0)
        rows["slot"] = np.where(used, slot, 0)
        rows["rows"] = np.where(used, th[safe] if K else 0, 0)
        rows["Wk"] = np.where(used, batch_width[safe] if K else 0, 0)
        rows["cut"] = np.where(used, cut, 0)
        _, ptr = pc.upload([rows, _tile_prefix(tiles), tables])       # jobs, the tile prefix, the value tables: one upload
        L.check(L.lib().ctd_warp_region_batches(ptr[0], n, ptr[1], n_tiles, ptr[2] if tables.size else None, storage.data_ptr(),
                                                _ABI_DTYPE[dtype], _LAYOUT[layout], int(bool(rgb)), int(pad),
                                                pc.st.cuda_stream), "ctd_warp_region_batches")
    return storage, offsets


class LineBatches:
    """The OCR input of `line_batches`: K width buckets in ONE device tensor `storage`.  `lb[k]` = (x, lines): x the
    (n_k, C, textheight, W_k) view ('nhwc': (n_k, textheight, W_k, C)) of batch k, `lines` the rows of `index` its slots hold,
    in order.  `index` (N,3) = (page, block, line), `valid`, `widths`: `LineRegions`' arrays of the same call (all N lines;
    a degenerate line is in no batch); `order`, `bounds`, `batch_width`, `cut`: the `batch_plan`; `offsets`: the element
    offset of every batch in `storage` (16-byte aligned).  `ready` is recorded behind the launch: `wait()` before use on
    another stream.  `page0`: the first page of the work item inside its batch (`detect_stream`)."""

    def __init__(self, storage: torch.Tensor, offsets: np.ndarray, index: np.ndarray, valid: np.ndarray, widths: np.ndarray,
                 plan: BatchPlan, textheight: int, channels: int, layout: str, ready: Optional[torch.cuda.Event], keep=None):
        self.storage, self.offsets, self.index, self.valid, self.widths = storage, offsets, index, valid, widths
        self.order, self.bounds, self.batch_width, self.cut = plan
        self.textheight, self.channels, self.dtype, self.layout = int(textheight), int(channels), storage.dtype, layout
        self.ready = ready
        self.page0 = 0
        self._keep = keep                                # the pages the launch reads, alive until the batches are dropped

    def __len__(self) -> int:
        return len(self.batch_width)

    def __getitem__(self, k):
        k = range(len(self))[k]
        lines = self.order[self.bounds[k]: self.bounds[k + 1]]
        n, th, ch, wk, o = len(lines), self.textheight, self.channels, int(self.batch_width[k]), int(self.offsets[k])
        shape = (n, ch, th, wk) if self.layout == "nchw" else (n, th, wk, ch)
        return self.storage[o: o + n * ch * th * wk].view(shape), lines

    def __iter__(self):
        return (self[k] for k in range(len(self)))

    def wait(self, stream: Optional[torch.cuda.Stream] = None) -> "LineBatches":
        """Orders `stream` (default: the current stream of the batches' device) behind the launch and tells the allocator
        that the storage is in use there."""
        st = stream if stream is not None else torch.cuda.current_stream(self.storage.device)
        if self.ready is not None:
            st.wait_event(self.ready)
        if self.storage.numel():
            self.storage.record_stream(st)
        return self

    def __repr__(self) -> str:
        return (f"LineBatches({len(self)} batches of {len(self.order)} lines, widths {self.batch_width.tolist()}, textheight "
                f"{self.textheight}, {self.layout} {self.dtype}, {self.storage.numel()} elements)")


def line_batches(pages: Sequence[Page], blk_lists: Sequence, textheight: int = 48, max_batch: Optional[int] = 16,
                 width_multiple: int = 8, max_width: Optional[int] = None, dtype=torch.float16, layout: str = "nchw",
                 mean=127.5, std=127.5, rgb: bool = False, pad: int = 0, stream: Optional[torch.cuda.Stream] = None,
                 device=None) -> LineBatches:
    """The lines of `line_regions(pages, blk_lists, textheight)` as the input tensors of an OCR network: sorted by width, cut
    into batches of at most `max_batch` lines (`batch_plan`), every batch padded to its own widest line, normalised
    ((v - mean[c]) / std[c] through a 256-entry table per output channel, `value_tables`), channel order reversed where `rgb`
    (BGR pages to RGB planes), padding = normalise(`pad`), laid out `layout` in `dtype` (torch.uint8: values unchanged).  One
    native host call for the transforms, one upload, ONE kernel launch writing one allocation; no packed intermediate and
    no torch kernel.  Asynchronous on `stream` (default: the current stream of the pages' device); see `LineBatches`."""
    if len(pages) != len(blk_lists):
        raise ValueError("one blk_list per page")
    if textheight < 1 or int(textheight) > L.REGION_MAX_SIDE:
        raise ValueError("textheight out of range")
    if dtype not in _ABI_DTYPE or layout not in _LAYOUT:
        raise ValueError("dtype: torch.uint8 / float16 / float32; layout: 'nchw' / 'nhwc'")
    if any(isinstance(p, torch.Tensor) and not p.is_cuda for p in pages):
        raise L.CtdError("line_batches takes numpy pages or CUDA tensors (there is no CPU path for CPU tensors)")
    with PageCall("line crops run", pages, stream, device, sync=False) as pc:
        P = pc.pages(pages)
        tables = value_tables(dtype, P.C, mean, std)
        index, quads, lang, vert, fs = batch_lines(blk_lists)
        pg = index[:, 0]
        wh, _, Minv, status = transforms(quads, lang, vert, fs, P.W[pg] if len(pg) else 0, P.H[pg] if len(pg) else 0, textheight)
        vert = np.asarray(vert).astype(bool)
        valid = status == L.REGION_OK
        widths = np.where(vert, wh[:, 1], wh[:, 0]).astype(np.int64)          # columns of the stored crops
        plan = batch_plan(widths, valid, max_batch, width_multiple, max_width)
        n, m = len(widths), len(plan.order)
        batch_of, slot, cut = np.full((n,), -1, np.int64), np.zeros((n,), np.int64), np.zeros((n,), np.int64)
        counts = np.diff(plan.bounds)
        batch_of[plan.order] = np.repeat(np.arange(len(counts)), counts)
        slot[plan.order] = np.arange(m) - np.repeat(plan.bounds[:-1], counts)
        cut[plan.order] = plan.cut
        storage, offsets = warp_batches(P.t, pg, wh, Minv, vert, P.C, batch_of, slot, cut, counts, plan.batch_width,
                                        int(textheight), dtype, layout, tables, rgb, pad)
        ready = torch.cuda.Event()
        ready.record(pc.st)
    return LineBatches(storage, offsets, index, valid, widths, plan, int(textheight), P.C, layout, ready, keep=P.t)
