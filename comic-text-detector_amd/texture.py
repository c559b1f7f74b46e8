"""Texture fill: rebuild screentone in a hole mask by patch matching, on the GPU.

`fill_rest` gives a hole its smooth surroundings: a gradient comes back, screentone comes back as its local mean.  This is
the step that starts from that result and puts the texture back without leaving the device:

    tx = texture_fill(er.pages, er.rest)                 # or TextDetector.texture_fill(pages, results)
    tx.pages[i]                                          # the page with every hole pixel filled from its surroundings' patches

builds one small table with numpy, uploads it once, makes ONE `ctd_texture_fill` call (csrc/kernels_texture.hip: a prepare
launch over the 64 x 64 tiles of all pages, `iterations * sweeps + 1` sweep launches and `iterations` vote launches over
the tiles, one workgroup per page for the rows; no host step between them) and downloads one small table.  The rule is
integers only and stated in include/ctd_hip.h (restated in numpy in tests/texture_ref.py; DESIGN.md section 4.30 has its
limits and what it gains): every pixel whose 7 x 7 patch touches the hole looks for the most similar patch that touches no
hole, within `radius` pixels, by Jacobi sweeps of propagation and random search driven by a hash of (pixel, sweep, draw,
seed); a hole pixel then becomes the rounded mean of what the patches covering it vote for.  It works at one scale: lines
and panel borders wider than a patch are not continued.  There is no per-page Python and no CPU fallback: without a GPU it
raises `CtdError` like the rest of the package.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import _lib as L
from .fill import fill_rest
from .pagecall import Page, PageCall, check_pages, table_dtype

__all__ = ["texture_fill", "TexturedPages", "texture_tables", "PAGE_DTYPE", "ROW_DTYPE"]

# numpy views of `ctd_texture_page` / `ctd_texture_row` (include/ctd_hip.h)
PAGE_DTYPE = table_dtype(L.CtdTexturePage)
ROW_DTYPE = table_dtype(L.CtdTextureRow)


def texture_tables(shapes: Sequence) -> tuple:
    """The tile and scratch columns of the page table for pages of `shapes` = (H, W): (tile0, n_tiles, fld0, cls0,
    scratch_bytes) -- the 64 x 64 tiles of the pages before each page, the tiles of all pages, the byte offsets of each page's
    two field planes and of its class plane in the scratch buffer (16 bytes a tile first, then 8 bytes a pixel of every page,
    then 1 byte a pixel of every page), and the buffer's size."""
    H = np.array([s[0] for s in shapes], np.int64)
    W = np.array([s[1] for s in shapes], np.int64)
    if len(H) and (min(H.min(), W.min()) < 1 or max(H.max(), W.max()) > L.TEXTURE_MAX_SIDE):
        raise ValueError(f"page sides must be 1 .. {L.TEXTURE_MAX_SIDE}")
    t = L.TEXTURE_TILE
    tiles = ((W + t - 1) // t) * ((H + t - 1) // t)
    n_tiles = int(tiles.sum())
    if n_tiles >= 2 ** 31:
        raise ValueError("too many pixels for one call")
    px = H * W
    before, total = np.cumsum(px) - px, int(px.sum())
    return np.cumsum(tiles) - tiles, n_tiles, 16 * n_tiles + 8 * before, 16 * n_tiles + 8 * total + before, 16 * n_tiles + 9 * total


class TexturedPages:
    """The result of `texture_fill`.  `pages[i]` (H,W,3) u8 in the page's channel order: dense device tensors, views of ONE
    allocation, each on a 256-byte boundary, page i with its hole pixels filled and every other pixel as it was.  Per page:
    `rows` the kernel's records (`ROW_DTYPE`), `status[i]` = `_lib.TEXTURE_OK` / `TEXTURE_NO_HOLE` (nothing to fill, a copy)
    / `TEXTURE_NO_SOURCE` (no 7 x 7 patch free of holes: the page with `init` on its holes), `n_hole[i]` the hole pixels,
    `n_target[i]` the pixels whose patch touches a hole, `n_source[i]` the patch centres to copy from, `n_unmatched[i]` the
    targets that found no source within the radius (their votes are missing; a hole pixel nobody votes for keeps `init`)."""

    def __init__(self, pages: List[torch.Tensor], rows: np.ndarray):
        self.pages, self.rows = pages, rows
        if len(pages) != len(rows):
            raise ValueError("one row per page")
        self.status = rows["status"]
        self.n_hole, self.n_target = rows["n_hole"], rows["n_target"]
        self.n_source, self.n_unmatched = rows["n_source"], rows["n_unmatched"]

    def __len__(self) -> int:
        return len(self.pages)

    def to_host(self):
        """The pages as a list of numpy arrays."""
        return [p.cpu().numpy() for p in self.pages]

    def __repr__(self) -> str:
        return f"TexturedPages({len(self.pages)} pages, {int((self.status == L.TEXTURE_OK).sum())} filled)"


def texture_fill(pages: Sequence[Page], holes: Sequence[Page], init: Optional[Sequence[Page]] = None, radius: int = 32,
                 iterations: int = 5, sweeps: int = 2, seed: int = 0, stream: Optional[torch.cuda.Stream] = None, device=None,
                 n_init: int = 8) -> TexturedPages:
    """Fill the hole pixels of EVERY page of a batch by the patch-matching rule: one table upload, one `ctd_texture_fill`
    call, one small download.  pages: uint8 (H,W,3) pages of any mix of sizes, holes: uint8 (H,W) masks of the same sizes
    (normally `ErasedPages.pages` and `.rest`; a pixel is a hole where the mask is not 0), init: the pages the search starts
    from, uint8 (H,W,3), read on hole pixels only (default: `fill.fill_rest(pages, holes)`, made here on the same stream and
    device); all on the device or on the host (uploaded here); row strides beyond the row size are honoured.  radius 1 ..
    127: how far a patch may come from; iterations 1 .. 16: rounds of `sweeps` (1 .. 8) search sweeps and one vote; n_init
    1 .. 16: random candidates of the first sweep; seed: any u32.  The result is a function of these and the page alone.
    Runs on `stream` (default: the current stream of the pages' device) and waits for the result; see `TexturedPages`."""
    if len(holes) != len(pages) or (init is not None and len(init) != len(pages)):
        raise ValueError("one hole mask (and one init page) per page")
    check_pages(pages, holes, mask="hole mask")
    if init is not None:
        check_pages(init)
        if any(tuple(a.shape) != tuple(p.shape) for a, p in zip(init, pages)):
            raise ValueError("an init page must have the shape of its page")
    for name, v, hi in (("radius", radius, L.TEXTURE_MAX_RADIUS), ("iterations", iterations, 16), ("sweeps", sweeps, 8), ("n_init", n_init, 16)):
        if not 1 <= int(v) <= hi:
            raise ValueError(f"{name} must be 1 .. {hi}")
    if not 0 <= int(seed) < 2 ** 32:
        raise ValueError("seed must be a u32")
    tile0, n_tiles, fld0, cls0, scratch_bytes = texture_tables([tuple(p.shape[:2]) for p in pages])
    n_pages = len(pages)
    if n_pages == 0:
        return TexturedPages([], np.zeros((0,), ROW_DTYPE))
    with PageCall("texture fill runs", pages, stream, device) as pc:
        P, M = pc.pages(pages), pc.pages(holes)
        # the default start: the pull-push fill of the same pages, on this call's stream and device
        S = pc.pages(fill_rest(P.t, M.t, device=pc.device).pages if init is None else init)
        # one buffer behind all the outputs, each on a 256-byte boundary
        out = pc.outputs([(int(h), int(w), 3) for h, w in zip(P.H, P.W)])
        pt = np.zeros((n_pages,), PAGE_DTYPE)
        pt["page_dev"], pt["hole_dev"], pt["init_dev"], pt["out_dev"] = P.ptr, M.ptr, S.ptr, [o.data_ptr() for o in out]
        pt["H"], pt["W"], pt["pitch"], pt["hole_pitch"], pt["init_pitch"], pt["out_pitch"] = P.H, P.W, P.pitch, M.pitch, S.pitch, 3 * P.W
        pt["tile0"], pt["fld0"], pt["cls0"] = tile0, fld0, cls0
        tab = pc.upload([pt])[0]
        scratch = torch.empty((scratch_bytes,), dtype=torch.uint8, device=pc.device)
        rows_dev = torch.empty((n_pages * ROW_DTYPE.itemsize,), dtype=torch.uint8, device=pc.device)
        prm = L.CtdTextureParams(n_tiles, int(radius), int(iterations), int(sweeps), int(n_init), int(seed), scratch_bytes)
        L.check(L.lib().ctd_texture_fill(tab.data_ptr(), n_pages, C.byref(prm), scratch.data_ptr(), rows_dev.data_ptr(),
                                         pc.st.cuda_stream), "ctd_texture_fill")
        rows = pc.rows(rows_dev, ROW_DTYPE, n_pages)
    return TexturedPages(out, rows)
