"""What the page calls share: argument checks, device pages, tables, one upload, the stream, one download.

`regions`, `colors`, `erase`, `balloons`, `layout`, `fill`, `typeset` and `glyphs` each make one native call on a batch of
pages.  The kernels differ; the Python around them is this module: `table_dtype` (the numpy view of a `_lib` structure),
`blk_lists_of`, `check_pages`, `device_pages`, `views`, `pack` and `PageCall`, the body of a call.  Nothing here knows any
one call.
"""
from __future__ import annotations

import math
from collections import namedtuple
from typing import Optional, Sequence, Union

import numpy as np
import torch

from . import _lib as L

__all__ = ["table_dtype", "blk_lists_of", "check_pages", "device_pages", "views", "align", "pack", "PageCall", "Pages", "Page"]

Page = Union[np.ndarray, torch.Tensor]

Pages = namedtuple("Pages", "t C ptr H W pitch")
Pages.__doc__ = """`PageCall.pages`: `t` the dense uint8 device tensors, `C` their channel count (1 for (H,W) pages; 3 where
there is no page), and per page `ptr` u64, `H`, `W` and the row `pitch` in bytes, i64 (every pitch is below 2^31)."""


def table_dtype(struct) -> np.dtype:
    """The numpy record of a `_lib` ctypes structure: same names, offsets and size, so a table built with it is the C table.
    (The ctypes mirrors are held to include/ctd_hip.h by the compiled-header tests.)"""
    return np.dtype(struct)


def blk_lists_of(results: Sequence) -> list:
    """Per page the blk_list: `results` holds (mask, mask_refined, blk_list) triples or the blk_lists themselves."""
    return [r[2] if isinstance(r, tuple) and len(r) == 3 else r for r in results]


def _shape_of(a):
    return tuple(a.shape), (a.dtype == torch.uint8 if isinstance(a, torch.Tensor) else np.asarray(a).dtype == np.uint8)


def check_pages(pages: Sequence[Page], masks: Optional[Sequence[Page]] = None, order: str = "", mask: str = "mask",
                nonempty: bool = True) -> None:
    """The page arguments of the tail calls, on the host or on the device: ValueError unless every page is uint8 (H,W,3),
    its mask (where masks are given, one a page) uint8 (H,W) of the page's size and, with `nonempty`, no side is 0.  `order`
    ("BGR ") and `mask` ("hole mask") only word the message."""
    for i, p in enumerate(pages):
        ps, pu8 = _shape_of(p)
        if not pu8 or len(ps) != 3 or ps[2] != 3:
            raise ValueError(f"pages must be uint8 {order}(H,W,3)")
        if masks is not None:
            ms, mu8 = _shape_of(masks[i])
            if not mu8 or ms != ps[:2]:
                raise ValueError(f"a {mask} must be uint8 and have the shape of its page")
        if nonempty and (ps[0] < 1 or ps[1] < 1):
            raise ValueError("empty page")


def align(n: int, a: int = 256) -> int:
    return (n + a - 1) // a * a


def views(shapes: Sequence[tuple], device) -> tuple:
    """Uninitialised uint8 device tensors of `shapes`: views of ONE new allocation, in the order given, each on a 256-byte
    boundary.  Returns (store, views)."""
    sizes = [math.prod(s) for s in shapes]
    offs = np.cumsum([0] + [align(n) for n in sizes]).tolist()
    store = torch.empty((offs[-1],), dtype=torch.uint8, device=device)
    return store, [store[o: o + n].view(s) for o, n, s in zip(offs, sizes, shapes)]


def need_gpu(what: str) -> None:
    """CtdError, worded by `what` ("line crops run"), where there is no GPU."""
    if not torch.cuda.is_available():
        raise L.CtdError(f"{what} on the GPU and there is none (no CPU fallback)")


def _scan_pages(pages: Sequence[Page], device, what: str) -> tuple:
    """`device_pages` and, read on the way, the columns of a page table: (tensors, C, device, (ptr, H, W, pitch) as lists)."""
    need_gpu(what)
    if device is None:
        device = next((p.device for p in pages if isinstance(p, torch.Tensor) and p.is_cuda), torch.device("cuda", 0))
    device = torch.device(device)
    out, ch, ptr, H, W, pitch = [], None, [], [], [], []
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
        h, w, s0 = t.shape[0], t.shape[1], t.stride(0)
        dense = t.stride(1) == c and (t.dim() == 2 or t.stride(2) == 1) and s0 >= w * c
        if h < 1 or w < 1:
            raise ValueError("empty page")
        if not dense:
            t = t.contiguous()
            s0 = t.stride(0)
        if ch is not None and c != ch:
            raise ValueError("the pages of one call must have the same number of channels")
        ch = c
        out.append(t), ptr.append(t.data_ptr()), H.append(h), W.append(w), pitch.append(s0)
    return out, (ch or 3), device, (ptr, H, W, pitch)


def device_pages(pages: Sequence[Page], device=None, what: str = "line crops run"):
    """Pages as uint8 device tensors (H,W) / (H,W,C) whose rows are dense (any row pitch): host pages are uploaded, tensors
    on the device pass through, others are copied -- all on the current stream.  Returns (tensors, C, device)."""
    return _scan_pages(pages, device, what)[:3]


def check_pitch(pitch: np.ndarray) -> None:
    """ValueError where a row pitch does not fit the int32 fields of the page tables."""
    if len(pitch) and pitch.max() >= 2 ** 31:
        raise ValueError("row pitch beyond int32")


def pack(parts) -> tuple:
    """The tables of a call as ONE byte array for one upload, each part on an 8-byte boundary: (blob, offsets)."""
    parts = [x.reshape(-1).view(np.uint8) for x in parts]
    at = [0]
    for x in parts:
        at.append(at[-1] + align(len(x), 8))
    blob = np.zeros((at[-1],), np.uint8)
    for a, x in zip(at, parts):
        blob[a: a + len(x)] = x
    return blob, at


class PageCall:
    """The body of one page call, a context manager:

        with PageCall("erasing text runs", pages, stream, device) as pc:
            P, M = pc.pages(pages), pc.pages(masks)            # dense device tensors + ptr / H / W / pitch columns
            out = pc.outputs(shapes)                           # views of one allocation
            tab, (jobs_ptr, pages_ptr) = pc.upload([jobs, pt]) # one blob, one upload
            L.check(L.lib().ctd_...(jobs_ptr, ..., pc.st.cuda_stream), "ctd_...")
            rows = pc.rows(rows_dev, ROW_DTYPE, n)             # one stream-ordered download

    Entering raises the no-GPU `CtdError` worded by `what`, enters `stream` where one is given, resolves the device (the
    argument, else the first CUDA tensor of `pages`, else cuda:0), enters it and sets `st`, its current stream: every
    allocation, copy and launch of the body is then on `st`.  Leaving synchronises `st` unless `sync=False` (or the body
    raised).

    LIFETIMES ARE THIS CLASS'S JOB.  A launch reads device memory that Python owns: host pages uploaded by `pages`, the
    `.contiguous()` copies it makes of tensors that are not dense, the table blob of `upload`, the buffer `rows` downloads.
    The object holds a reference to each of them until it is left, that is until `st` has been synchronised, so no caller
    can drop one early by reusing a name.  With `sync=False` nothing has been waited for when the object is left; that is
    sound only because all of the above were allocated on `st` inside the block, so the caching allocator hands their memory
    to nobody but later work on `st`, behind the launch.  Allocate a kernel input outside the block, or on another stream,
    and the same code becomes a use-after-free on the device: this is the one place where moving a line turns correct code
    into that.  Tensors the CALLER owns (device pages passed in) are the caller's to keep; the asynchronous results keep
    them themselves (`LineRegions` / `LineBatches` `keep=`)."""

    def __init__(self, what: str, pages: Sequence = (), stream: Optional[torch.cuda.Stream] = None, device=None,
                 sync: bool = True):
        self.what, self._pages, self._stream, self.device, self.sync = what, pages, stream, device, sync
        self.st, self._keep, self._ctx = None, [], []

    def __enter__(self) -> "PageCall":
        need_gpu(self.what)
        try:
            if self._stream is not None:
                self._open(torch.cuda.stream(self._stream))
            if self.device is None:
                self.device = next((p.device for p in self._pages if isinstance(p, torch.Tensor) and p.is_cuda),
                                   torch.device("cuda", 0))
            self.device = torch.device(self.device)
            self._open(torch.cuda.device(self.device))
            self.st = torch.cuda.current_stream(self.device)
        except BaseException:
            self._close()
            raise
        return self

    def _open(self, cm) -> None:
        cm.__enter__()
        self._ctx.append(cm)

    def _close(self) -> None:
        self._keep = []
        while self._ctx:
            self._ctx.pop().__exit__(None, None, None)

    def __exit__(self, exc_type, exc, tb):
        try:
            if exc_type is None and self.sync:
                self.st.synchronize()
        finally:
            self._close()
        return False

    def pages(self, seq: Sequence[Page], dense: bool = False) -> Pages:
        """`device_pages` of `seq` on the call's device and stream, kept until the call is left, with the columns a page
        table wants.  dense=True: `seq` already holds such tensors (`warp`, `color_rows`) and is taken as it is."""
        if dense:
            t = list(seq)
            ch = 3 if not t else 1 if t[0].dim() == 2 else int(t[0].shape[2])
            cols = [p.data_ptr() for p in t], [p.shape[0] for p in t], [p.shape[1] for p in t], [p.stride(0) for p in t]
        else:
            t, ch, _, cols = _scan_pages(seq, self.device, self.what)
        self._keep.append(t)
        ptr, H, W, pitch = (np.array(c, dt) for c, dt in zip(cols, (np.uint64, np.int64, np.int64, np.int64)))
        check_pitch(pitch)
        return Pages(t, ch, ptr, H, W, pitch)

    def outputs(self, shapes: Sequence[tuple]) -> list:
        """`views`: uninitialised uint8 device tensors of `shapes` in one new allocation (the result owns them)."""
        return views(shapes, self.device)[1]

    def upload(self, parts) -> tuple:
        """`pack` and ONE upload: (the device blob, the device pointer of every part), parts on 8-byte boundaries."""
        blob, at = pack(parts)
        tab = torch.from_numpy(blob).to(self.device)
        self._keep.append(tab)
        return tab, [tab.data_ptr() + a for a in at[:-1]]

    def rows(self, dev_buf: torch.Tensor, dtype, n: int) -> np.ndarray:
        """The first `n` records of `dev_buf` on the host as `dtype`: one download, stream-ordered behind the launches."""
        self._keep.append(dev_buf)
        return dev_buf.cpu().numpy().view(dtype)[:n]
