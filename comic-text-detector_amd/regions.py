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

What is restated from cv2 here (four-point homography, the fixed-point linear warp) is listed in DESIGN.md section 5.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence, Union

import numpy as np
import torch

from . import _lib as L
from .textblock import LANGCLS2IDX, BlockList, TextBlock

__all__ = ["line_regions", "LineRegions", "transforms", "warp", "JOB_DTYPE"]

# numpy view of `ctd_region_job` (include/ctd_hip.h; _lib.CtdRegionJob)
JOB_DTYPE = np.dtype([("page_dev", "<u8"), ("H", "<i4"), ("W", "<i4"), ("C", "<i4"), ("pitch", "<i4"), ("Minv", "<f8", (9,)),
                      ("w", "<i4"), ("h", "<i4"), ("rotate", "<i4"), ("pad_", "<i4"), ("out_off", "<i8")])
assert JOB_DTYPE.itemsize == C.sizeof(L.CtdRegionJob)

Page = Union[np.ndarray, torch.Tensor]


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


def _device_pages(pages: Sequence[Page], device=None):
    """Pages as uint8 device tensors (H,W) / (H,W,C) whose rows are dense (any row pitch): host pages are uploaded, tensors
    on the device pass through.  Returns (tensors, C, device)."""
    if not torch.cuda.is_available():
        raise L.CtdError("line crops run on the GPU and there is none (no CPU fallback)")
    if device is None:
        device = next((p.device for p in pages if isinstance(p, torch.Tensor) and p.is_cuda), torch.device("cuda", 0))
    device = torch.device(device)
    out, ch = [], None
    for p in pages:
        if isinstance(p, torch.Tensor):
            t = p.to(device)
        else:
            a = np.asarray(p)
            if a.dtype != np.uint8:
                raise ValueError("pages must be uint8")
            t = torch.from_numpy(np.ascontiguousarray(a)).to(device)
        if t.dtype != torch.uint8 or t.dim() not in (2, 3) or (t.dim() == 3 and t.shape[2] not in (1, 3)):
            raise ValueError("pages must be uint8 (H,W) or (H,W,3)")
        c = 1 if t.dim() == 2 else int(t.shape[2])
        dense = t.stride(1) == c and (t.dim() == 2 or t.stride(2) == 1) and t.stride(0) >= t.shape[1] * c
        if t.shape[0] < 1 or t.shape[1] < 1:
            raise ValueError("empty page")
        if not dense:
            t = t.contiguous()
        if ch is not None and c != ch:
            raise ValueError("the pages of one call must have the same number of channels")
        ch = c
        out.append(t)
    return out, (ch or 3), device


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
    dev = pages[0].device if pages else torch.device("cuda", 0)
    tiles = (pix + L.REGION_TILE - 1) // L.REGION_TILE
    n_tiles = int(tiles.sum())
    if n_tiles >= 2 ** 31:
        raise ValueError("too many pixels for one launch")
    with torch.cuda.stream(stream) if stream is not None else torch.cuda.device(dev):
        st = torch.cuda.current_stream(dev)
        packed = torch.empty((total,), dtype=torch.uint8, device=dev)
        if n_tiles == 0:
            return packed, offsets, sizes
        page_of = np.asarray(page_of, np.int64).reshape(n)
        ptr = np.array([p.data_ptr() for p in pages], np.uint64)
        H = np.array([p.shape[0] for p in pages], np.int32)
        W = np.array([p.shape[1] for p in pages], np.int32)
        pitch = np.array([p.stride(0) for p in pages], np.int64)
        if pitch.max() >= 2 ** 31:
            raise ValueError("row pitch beyond int32")
        table = np.zeros((n * JOB_DTYPE.itemsize + (n + 1) * 4,), np.uint8)          # jobs, then the tile prefix: one upload
        jobs = table[: n * JOB_DTYPE.itemsize].view(JOB_DTYPE)
        jobs["page_dev"], jobs["H"], jobs["W"], jobs["C"], jobs["pitch"] = ptr[page_of], H[page_of], W[page_of], channels, pitch[page_of]
        jobs["Minv"] = np.asarray(Minv, np.float64).reshape(n, 9)
        jobs["w"], jobs["h"], jobs["rotate"], jobs["out_off"] = wh[:, 0], wh[:, 1], rotate, offsets
        table[n * JOB_DTYPE.itemsize:].view(np.int32)[:] = np.concatenate(([0], np.cumsum(tiles)))
        tab = torch.from_numpy(table).to(dev)
        L.check(L.lib().ctd_warp_regions(tab.data_ptr(), n, tab.data_ptr() + n * JOB_DTYPE.itemsize, n_tiles, packed.data_ptr(),
                                         st.cuda_stream), "ctd_warp_regions")
    return packed, offsets, sizes


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


def _regions(pages, ch, index, quads, lang, vert, fs, textheight, stream) -> LineRegions:
    H = np.array([p.shape[0] for p in pages], np.int32)
    W = np.array([p.shape[1] for p in pages], np.int32)
    pg = index[:, 0]
    wh, _, Minv, status = transforms(quads, lang, vert, fs, W[pg] if len(pg) else 0, H[pg] if len(pg) else 0, textheight)
    vert = np.asarray(vert).astype(bool)
    packed, offsets, sizes = warp(pages, pg, wh, Minv, vert, ch, stream)
    return LineRegions(packed, index, sizes[:, 1].astype(np.int64), offsets, status == L.REGION_OK, int(textheight), ch,
                       keep=pages)


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
    pages, ch, device = _device_pages(pages, device)
    cols = [_page_lines(b) for b in blk_lists]
    counts = [len(c[0]) for c in cols]
    cat = lambda k, dt: (np.concatenate([c[k] for c in cols]).astype(dt) if cols else np.zeros((0,), dt))   # noqa: E731
    index = np.stack([np.repeat(np.arange(len(cols)), counts), cat(4, np.int64), cat(5, np.int64)], axis=1).astype(np.int32) \
        if cols else np.zeros((0, 3), np.int32)
    quads = np.concatenate([c[0] for c in cols]) if cols else np.zeros((0, 8), np.int32)
    return _regions(pages, ch, index, quads, cat(1, np.int32), cat(2, np.int32), cat(3, np.float64), textheight, stream)


def transformed_region(blk: TextBlock, img: Page, idx: int, textheight):
    """`TextBlock.get_transformed_region`: one line's crop, a numpy array for a numpy image, a device tensor for a device
    tensor (no host round trip, asynchronous on the current stream)."""
    host = not isinstance(img, torch.Tensor)
    if not host and not img.is_cuda:
        raise L.CtdError("get_transformed_region takes a numpy image or a CUDA tensor (there is no CPU path)")
    pages, ch, _ = _device_pages([img])
    q = np.asarray(blk.lines[idx], np.float64).reshape(1, 8)
    if not np.array_equal(q, np.trunc(q)):
        raise ValueError("text lines must have integer coordinates (the detector's quads)")
    regs = _regions(pages, ch, np.zeros((1, 3), np.int32), q.astype(np.int32), [LANGCLS2IDX.get(blk.language, 1)],
                    [bool(blk.vertical)], [float(blk.font_size)], textheight, None)
    if not regs.valid[0]:
        raise ValueError(f"degenerate text line {blk.lines[idx]}: no region of height {textheight} (zero size, non-finite "
                         "aspect ratio or singular homography)")
    out = regs[0] if pages[0].dim() == 3 else regs[0][:, :, 0]
    return out.cpu().numpy() if host else out
