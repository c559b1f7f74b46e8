"""TEST INFRASTRUCTURE.  Float64 per-op reference of the lowered op program with an error bound derived from each
engine's arithmetic (used by tests/test_layer_ref.py on the CPU and tests/test_gpu_layers.py on the GPU).

For one op of a program, `LayerCheck.check(i)` takes the op's inputs AS THE ENGINE STORED THEM (`read_tensor`, or the
page for the first layer), recomputes the op in float64 from the program blob's folded weights and returns
max |engine - ref| / bound over the checked elements.  A ratio above 1 is a kernel, packing or dispatch bug.

In-place writes.  The lowering lets a C3 bottleneck write its result into the channel slice it reads as residual, and
the merged cv1+cv2 conv writes a slice the bottleneck later overwrites: after a forward that slice holds only its last
version.  `snapshot_program` appends, right after every op whose output is overwritten later, a 1x1 conv with identity
weights (no bias, no activation) that copies the op's output into a fresh tensor.  The copy is exact on every engine
(one product by 1.0 per output, the other products are 0 * x = 0; fp16 values stay fp16, the split engine's weight 1.0
splits exactly and hi + lo is what it stored), and the original ops keep their kernels (asserted on the GPU).

The bound.  u = 2^-24, S = sum |w x| + |b| in f64 over the K products of an output, lambda = 4 (the probabilistic
accumulation bound of Higham & Mary, one value for every kernel).  Pre-activation allowance A:

  fp32   lambda sqrt(K) u S                                        (f32-operand MFMA, f32 accumulate)
  fp32s  lambda sqrt(K) u S + sum |w| max(2^-22 |x|, 2^-25) + 2^-21 S + 2^-33 max|w_n| sum |x|
         (activations split hi + lo with fp16's subnormal floor 2^-25 -- activations are NOT scaled; weight hi + lo after
         the per-channel power-of-two scaling and the dropped wl xl term; the last term is the subnormal floor of a weight
         lo half 2^-34 below the channel's scaled maximum, doubled)
  fp16   lambda sqrt(K) u S + 2^-11 S + 2^-25 sum |x|
         (weights packed as an fp16 rounding of the blob, with fp16's subnormal floor; activations read back are exact
         fp16.  The first layer (STEM) reads the page: float input is rounded to fp16, + 2^-11 S + 2^-25 sum |w|, and the
         u8 variant packs w 128/255, whose subnormal floor is counted twice: 2^-24 sum |x|)

  K = Cin k^2 for a conv, Cin (k / s)^2 for a ConvTranspose.  Inputs the engine took from the page instead of a stored
  tensor (the fp32s first layer) add u S for the f32 rounding of u8 / 255.

On top of A:
  activation, propagated    sup |phi'| over [v - A, v + A] times A (SiLU: 1.1; sigmoid: sigma'(max(|v| - A, 0)))
  activation, own           SiLU / sigmoid (|v| + 8) u |phi(v)| + 2^-120: ctd_act_fast is __expf (1 ulp of v_exp_f32 plus
                            the rounding of v log2 e, |v| u relative) + rcp (1 ulp) + 1 + e and the product (1 ulp each),
                            and ctd_silu_f32 (~2 ulp) is inside it; the absolute term covers denormal flushing; leaky u |phi|
  residual add              u |y|, and for fp32s the residual read as hi + lo: max(2^-22 |r|, 2^-25)
  storage                   fp32 u |y|; fp32s (split plane or fp32, either) max(2^-22 |y|, 2^-25); fp16 max(2^-11 |y|, 2^-25),
                            with |y| the reference plus everything above (the engine rounds its own value)

Other ops: AVGPOOL2 (a + b) + (c + d) times 0.25: 0.5 u sum |x| + storage.  DETECT (expf, IEEE division: sigma to 6 u
relative): xy (2 sigma - 0.5 + g) s within s (12 u sigma + u (2 sigma + |2 sigma - 0.5| + 2 |2 sigma - 0.5 + g|)),
wh (2 sigma)^2 a within 15 u |wh|, scores within 6 u sigma.  DB_UP: the hidden ConvT's output h gets the conv bound,
the relu and the engine's storage of h (fp16 on the fp16 engine, f32 otherwise); the second ConvT adds sum |w2| E_h.
SEG_FINAL: the ConvT bound + sigmoid + f32 storage.

Exact ops stay exact: MAXPOOL is bit-identical to the max of the engine's own input; EXPORT copies; on the engine's own
outputs bitmap == (lines[:, 0] > thresh) and mask_u8 == (mask * float32(255)).astype(uint8) (reference inference.py).

Sampling.  Maps larger than 128 x 128 per page are checked on 16 x 16 output windows, all channels.  The windows follow the
kernels' geometry (`EDGES`, one row per patch / tile shape with the kernel it comes from): for every row of the table the
windows straddle the first, one interior (nearest the middle) and the LAST interior multiple of the edge, in both axes and
crossed with each other -- corners of four patches, 3 x 3 per row of the table.  `LINEAR_BLOCKS` adds, in a late row, the two
ends of a row wrap and the block edge nearest to it for the kernels that walk the map in linear blocks of pixels.  On top of
that the earlier set stays as it was: the four corners, the middle of each edge, the seams at 16, 32, 64, 128 and 256 on
the diagonal and on two crosses, and four seeded random windows.  The reference of a window is computed from a zero-padded
crop of the input.  Smaller maps are checked in full.

Pages.  Without `pages`: the sampled maps on pages 0 and B - 1, the smaller maps on every page.  With `pages`: every op on
exactly those pages; the checker then keeps only those pages of every tensor it reads (`read_tensor` hands out all B), and
`check_all` drops a tensor once no later op's check reads it.  What a sampled check leaves out is stated as a condition (every
row of `EDGES`, every requested page, for every op); the share of elements it looked at is reported (`n` of `total`), no
number is asserted for it.

Programs built by hand.  `direct_program` is a small program no lowering of the network produces: channel counts and
offsets that no vector path can take, so that every engine runs it on its direct (VALU) kernels -- the universal fallback,
and the yardstick of the native selftest.  It has no Detect / seg-final / DB ops: `outs` may be {} for such a program, and
the INPUT op is left out through `check_all(ops=...)` where the engine stores the page in fp16 (the network's fp16 program
has a STEM op instead, so the checker has no fp16 INPUT bound).
"""
from __future__ import annotations

import copy
import importlib
import math
from typing import Callable, Dict, List, Optional

import numpy as np
import torch
import torch.nn.functional as F

L = importlib.import_module("comic-text-detector_amd._lib")

U = 2.0 ** -24
LAMBDA = 4.0
ENGINES = ("fp32", "fp32s", "fp16")
WIN = 16
FULL_MAX = 128
SEAMS = (16, 32, 64, 128, 256)
# (rows, columns) of a patch / tile in OUTPUT pixels, and the kernels that cut the map that way (their own constants, as
# tests/c3_emul.py, tests/stem2_emul.py, tests/test_halo3_emul.py and tests/test_split_halo_emul.py restate them)
EDGES = (
    (16, 16, "conv_halo_kernel, conv_halo3_kernel (kernels_halo*.hip TWP x THP = 16 x 16), conv_split_halo_kernel THP = 16, "
             "stem_split_kernel (kernels_split_stem.hip ST = 16), kernels_fused.hip SF_T = 16"),
    (8, 16, "c3_fused_kernel (C3_TW x C3_TH = 16 x 8), c3b_kernel (BW = 16, BH = 8), stem_conv2_kernel (S2_TW x S2_TH = 16 x 8), "
            "conv_split_halo_kernel THP = 8"),
    (8, 32, "the first layer of kernels_fused.hip (SM_TW x SM_TH = 32 x 8 outputs)"),
    (32, 32, "a ConvTranspose 4x4 / stride 2 through conv_halo_kernel / conv_halo3_kernel / conv_split_halo_kernel (a 16 x 16 "
             "input patch writes 32 x 32) and seg_final_mfma_kernel / seg_final_gather_kernel (SF_T = 16 input pixels, 2 x 2 each)"),
    (4, 128, "db_up_mfma_kernel: a group of 32 quarter-resolution pixels writes 4 rows of 128 outputs"),
    (64, 64, "a 16 x 16 patch two stride-2 ConvTransposes below the map (the heads' last two layers)"),
    (128, 128, "conv_f32_kernel (FBM = 128), conv_igemm_kernel / conv_split_kernel BM = 128: block edges of a map whose width "
               "is a multiple of 128, and a block of whole rows"),
    (256, 256, "conv_igemm_kernel / conv_split_kernel BM = 256 (SBM): likewise"),
)
LINEAR_BLOCKS = (128, 256)          # pixels per block of kernels_f32.hip / kernels_igemm.hip / kernels_split.hip
INF = float("inf")


# ---------------------------------------------------------------------------------------------------------------------
# which op wrote what
# ---------------------------------------------------------------------------------------------------------------------

def _writes(o) -> Optional[tuple]:
    k = o["kind"]
    if k == L.OP_INPUT:
        return None if o["dst"] < 0 else (o["dst"], 0, -1)
    if k in (L.OP_STEM, L.OP_CONV, L.OP_CONVT):
        return o["dst"], o["dst_coff"], o["cout"]
    if k in (L.OP_MAXPOOL, L.OP_AVGPOOL2):
        return o["dst"], o["dst_coff"], o["src0_c"]
    return None


def _write_range(prog, o):
    w = _writes(o)
    if w is None:
        return None
    tid, lo, c = w
    return tid, lo, (prog.tensors[tid][0] if c < 0 else lo + c)


def snapshot_program(prog):
    """-> (program with identity-copy ops after every op whose output is overwritten later, {original op index: index in
    the new program}, {original op index: snapshot tensor id})."""
    rng = [_write_range(prog, o) for o in prog.ops]
    snap = copy.copy(prog)
    snap.tensors = list(prog.tensors)
    snap.ops = []
    snap._params = list(prog._params)
    snap.taps = dict(prog.taps)
    index, snaps = {}, {}
    for i, o in enumerate(prog.ops):
        index[i] = len(snap.ops)
        snap.ops.append(dict(o))
        r = rng[i]
        if r is None:
            continue
        tid, lo, hi = r
        if any(q is not None and q[0] == tid and q[1] < hi and lo < q[2] for q in rng[i + 1:]):
            c = hi - lo
            t = snap.tensor(c, prog.tensors[tid][1], prog.tensors[tid][2])
            snap.op(L.OP_CONV, src0=tid, src0_coff=lo, src0_c=c, dst=t, dst_coff=0, cout=c, k=1, stride=1, pad=0,
                    act=L.ACT["none"], w_off=snap.param(np.eye(c, dtype=np.float32).reshape(c, c, 1, 1)),
                    b_off=snap.param(np.zeros(c, np.float32)), name=(o["name"] or f"op{i}") + ".snapshot")
            snaps[i] = t
    return snap, index, snaps


def direct_program(prec: int, seed: int = 0):
    """-> (program, indices of the ops to check).  B x 192 x 320 pages, two average pools, then seven conv ops around a
    24 x 40 map with cin = 24 / 40 / 48 and cout = 20 / 24 (no multiple of 16 or 32 among the sources, channel offsets 3 and
    23 in a 44-channel tensor): a 3x3 / s2 conv (padding on the top and left only) twice, a residual add into a channel offset
    of a wider tensor, a two-source conv with one source through the x2 upsample, ConvTranspose 4x4 / s2 / p1 and 2x2 / s2 /
    p0, and silu, leaky, relu and none.  Weights ~ N(0, gain^2 / fan_in) with synth's gains: activations stay O(1)."""
    G = importlib.import_module("comic-text-detector_amd.graph")
    r = np.random.RandomState(4000 + seed)
    P = G.Program(prec)
    P.meta = dict(no=1)                                   # no Detect op: blks is (B, 0, 1)

    def w(shape, fan_in, gain=1.0):
        return (r.standard_normal(shape) * gain / math.sqrt(fan_in)).astype(np.float32)

    def b(c):
        return (0.1 * r.standard_normal(c)).astype(np.float32)

    t_in = P.tensor(4, 0, 0, "input")
    P.op(L.OP_INPUT, dst=t_in, name="input")
    cur = t_in
    for d in (1, 2):
        t = P.tensor(4, d, 0, f"d.pool{d}")
        P.op(L.OP_AVGPOOL2, src0=cur, src0_coff=0, src0_c=4, dst=t, name=f"d.pool{d}")
        cur = t
    first = len(P.ops)
    w0 = w((24, 4, 3, 3), 27, 1.25)
    w0[:, 3] = 0                                          # the page's zero 4th channel
    A = P.conv([G.View(cur, 0, 4, 2)], w0, b(24), 3, 2, 1, "silu", name="d.stem")                  # 24 x 40, 24 channels
    wide = P.tensor(44, 3, 0, "d.wide")
    P.conv([A], w((20, 24, 1, 1), 24), b(20), 1, 1, 0, "leaky", dst=G.View(wide, 3, 20, 3), name="d.pw")
    P.conv([A], w((20, 24, 3, 3), 216), b(20), 3, 1, 1, "relu", dst=G.View(wide, 23, 20, 3), res=G.View(wide, 3, 20, 3),
           name="d.res")
    D = P.conv([G.View(wide, 3, 40, 3)], w((24, 40, 3, 3), 360), None, 3, 2, 1, "none", name="d.down")     # 12 x 20
    E = P.conv([A, G.View(D.tid, 0, 24, 3, up=1)], w((20, 48, 3, 3), 432, 1.25), b(20), 3, 1, 1, "silu", name="d.cat")
    P.convt(D, w((24, 20, 4, 4), 96), b(20), 4, 2, 1, "leaky", name="d.up4")                       # 12 x 20 -> 24 x 40
    P.convt(E, w((20, 24, 2, 2), 20), b(24), 2, 2, 0, "relu", name="d.up2")                        # 24 x 40 -> 48 x 80
    return P, list(range(first, len(P.ops)))


# ---------------------------------------------------------------------------------------------------------------------
# float64 pieces
# ---------------------------------------------------------------------------------------------------------------------

def _t(a) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a, np.float64))


def _sig(v):
    return 1.0 / (1.0 + np.exp(-np.clip(v, -700, 700)))


def _act(v, act):
    if act == L.ACT["silu"]:
        return v * _sig(v)
    if act == L.ACT["leaky"]:
        return np.where(v > 0, v, 0.1 * v)
    if act == L.ACT["relu"]:
        return np.maximum(v, 0.0)
    if act == L.ACT["sigmoid"]:
        return _sig(v)
    return v


def _act_err(v, A, act, y):
    """sup |phi'| over [v - A, v + A] * A + the activation's own error at v (see the module docstring)."""
    if act == L.ACT["silu"]:
        return 1.1 * A + (np.abs(v) + 8) * U * np.abs(y) + 2.0 ** -120
    if act == L.ACT["sigmoid"]:
        m = np.maximum(np.abs(v) - A, 0.0)
        s = _sig(m)
        return s * (1 - s) * A + (np.abs(v) + 8) * U * np.abs(y) + 2.0 ** -120
    if act == L.ACT["leaky"]:
        return np.where(v + A > 0, 1.0, 0.1) * A + U * np.abs(y)
    if act == L.ACT["relu"]:
        return np.where(v + A > 0, 1.0, 0.0) * A
    return A


def _split_err(x):
    return np.where(x == 0, 0.0, np.maximum(2.0 ** -22 * np.abs(x), 2.0 ** -25))


def storage_err(engine: str, y, f32: bool = False):
    if engine == "fp32" or (engine == "fp16" and f32):
        return U * np.abs(y)
    if engine == "fp32s":
        return np.maximum(2.0 ** -22 * np.abs(y), 2.0 ** -25)
    return np.maximum(2.0 ** -11 * np.abs(y), 2.0 ** -25)


def _ratio(got, ref, bound) -> float:
    d = np.abs(np.asarray(got, np.float64) - ref)
    if not np.all(np.isfinite(got)):
        return INF
    over = d[bound <= 0]
    if over.size and over.max() > 0:
        return INF
    b = np.where(bound > 0, bound, 1.0)
    return float((np.where(bound > 0, d, 0.0) / b).max()) if d.size else 0.0


def _ratio_pages(got, ref, bound):
    """-> (worst ratio, index along axis 0 where it is)."""
    r = [_ratio(got[b], ref[b], bound[b]) for b in range(len(ref))]
    j = int(np.argmax(r)) if r else 0
    return (r[j] if r else 0.0), j


def seam_positions(e: int, n: int):
    """The first, the interior (nearest n / 2) and the last multiple of e inside (0, n)."""
    if e >= n:
        return []
    last = (n - 1) // e * e
    mid = min(max(int(round(n / 2 / e)) * e, e), last)
    return sorted({e, mid, last})


def legacy_positions(Ho: int, Wo: int, seed: int, salt: int):
    """Window origins of the earlier sampling (before clamping): corners, edge middles, SEAMS on the diagonal and two crosses,
    four seeded random windows."""
    pos = [(0, 0), (0, Wo), (Ho, 0), (Ho, Wo), (0, Wo // 2 - 8), (Ho, Wo // 2 - 8), (Ho // 2 - 8, 0), (Ho // 2 - 8, Wo)]
    for m in SEAMS:
        if m < Ho or m < Wo:
            pos.append((m - 8, m - 8))
            pos.append((m - 8, Wo // 2 + 3))
            pos.append((Ho // 2 + 5, m - 8))
    r = np.random.RandomState(seed * 7919 + salt)
    pos += [(int(r.randint(0, Ho - WIN + 1)), int(r.randint(0, Wo - WIN + 1))) for _ in range(4)]
    return pos


def geometry_positions(Ho: int, Wo: int):
    """Window origins (before clamping) that straddle, crossed in both axes, the first / interior / last seam of every row of
    EDGES, and the row wraps and late block edges of LINEAR_BLOCKS."""
    h = WIN // 2
    pos = []
    for eh, ew, _ in EDGES:
        ys, xs = seam_positions(eh, Ho), seam_positions(ew, Wo)
        pos += [(y - h, x - h) for y in ys for x in xs]
    late = max(Ho - WIN - h, 0)                           # rows [late, late + WIN): the ends of 16 rows and the starts of the next
    pos += [(late, Wo), (late, 0)]
    for lb in LINEAR_BLOCKS:
        if Ho * Wo > lb:
            p = ((late + h) * Wo + Wo // 2) // lb * lb   # a block edge in a late row (on a column seam when lb divides Wo)
            pos.append((p // Wo - h, p % Wo - h))
    return pos


# ---------------------------------------------------------------------------------------------------------------------
# the checker
# ---------------------------------------------------------------------------------------------------------------------

class LayerCheck:
    """prog: the lowered program (NOT the snapshot one); snaps: `snapshot_program`'s third result (or {} when nothing is
    overwritten); engine: "fp32" / "fp32s" / "fp16"; get(tid) -> engine tensor (B,H,W,C) f32 (`read_tensor` layout);
    outs: dict(blks, mask, lines, mask_u8, bitmap) numpy; page: (B,3,H,W) what the network sees (u8 / 255 or the float
    input); u8: the page came in as uint8; kernels: per original op the kernel name (None: every op wrote its tensor);
    pages: the pages to check (None: see the module docstring) -- everything the checker keeps is cut down to them, and
    results name the page of the batch, not its position in `pages`; legacy_windows: the earlier window set only (kept so
    that a test can show what that set misses)."""

    def __init__(self, prog, snaps: Dict[int, int], engine: str, get: Callable, outs: dict, page, u8: bool = False,
                 kernels: Optional[List[str]] = None, seed: int = 0, pages=None, legacy_windows: bool = False):
        assert engine in ENGINES
        self.p, self.snaps, self.engine, self._get = prog, snaps, engine, get
        self.B_all = len(page)
        self.pages = None if pages is None else sorted({int(b) for b in pages})
        assert self.pages is None or (self.pages and 0 <= self.pages[0] and self.pages[-1] < self.B_all), pages
        self.real = list(range(self.B_all)) if self.pages is None else self.pages      # kept position -> page of the batch
        self.page = np.asarray(page if self.pages is None else page[self.pages], np.float64)   # (anything with len and [list])
        self.outs = outs if self.pages is None else {k: np.asarray(v)[self.pages] for k, v in outs.items()}
        self.u8, self.kernels, self.seed, self.legacy = u8, kernels, seed, legacy_windows
        self.blob = prog.blob().astype(np.float64)
        self.B, _, self.H, self.W = self.page.shape
        self.rng = [_write_range(prog, o) for o in prog.ops]
        self._cache: Dict[int, np.ndarray] = {}
        self.peak_cached_bytes = 0

    # -- engine values ------------------------------------------------------------------------------------------------
    def get(self, tid: int) -> np.ndarray:
        if tid not in self._cache:
            a = self._get(tid)
            assert len(a) == self.B_all, (tid, a.shape)
            self._cache[tid] = np.asarray(a, np.float32) if self.pages is None else np.ascontiguousarray(a[self.pages], np.float32)
            del a
            self.peak_cached_bytes = max(self.peak_cached_bytes, sum(v.nbytes for v in self._cache.values()))
        return self._cache[tid]

    def _fused(self, i: int) -> bool:
        return self.kernels is not None and self.kernels[i] == "(fused)"

    def _segments(self, tid: int, coff: int, c: int, t: int):
        """Where channels [coff, coff + c) of tensor `tid`, as they were right before op t, are to be read: a list of
        ("page", writer op, ch, end) / ("tensor", tensor id, first channel there, ch, end)."""
        segs = []
        ch = coff
        while ch < coff + c:
            w = max((j for j in range(t) if self.rng[j] is not None and self.rng[j][0] == tid
                     and self.rng[j][1] <= ch < self.rng[j][2]), default=None)
            if w is None:
                raise ValueError(f"tensor {tid} channel {ch} is read before any op writes it")
            end = min(coff + c, self.rng[w][2])
            final = not any(q is not None and q[0] == tid and q[1] <= ch < q[2] for q in self.rng[w + 1:])
            if self.p.ops[w]["kind"] == L.OP_INPUT and self._fused(w):
                segs.append(("page", w, ch, end))
            elif final:
                segs.append(("tensor", tid, ch, ch, end))
            else:
                segs.append(("tensor", self.snaps[w], ch - self.rng[w][1], ch, end))
            ch = end
        return segs

    def value(self, tid: int, coff: int, c: int, t: int, f64: bool = True) -> np.ndarray:
        """Channels [coff, coff + c) of tensor `tid` as they were right before op t (B,H,W,c) f64 -- or, with f64 = False, as
        stored (f32, a view where one tensor holds them all): for callers that cut windows out before they compute."""
        parts = []
        for seg in self._segments(tid, coff, c, t):
            if seg[0] == "page":
                _, w, ch, end = seg
                x = self.page.transpose(0, 2, 3, 1)
                x = np.concatenate([x, np.zeros(x.shape[:3] + (self.rng[w][2] - 3,))], 3)
                parts.append(x[..., ch: end])
            else:
                _, src, first, ch, end = seg
                a = self.get(src)[..., first: first + end - ch]
                parts.append(a.astype(np.float64) if f64 else a)
        return np.concatenate(parts, 3) if len(parts) > 1 else parts[0]

    def reads(self, i: int) -> set:
        """Ids of the engine tensors that check(i) fetches."""
        o = self.p.ops[i]
        want = []
        if self.rng[i] is not None and not (o["kind"] == L.OP_INPUT and self._fused(i)):
            tid, lo, hi = self.rng[i]
            want.append((tid, lo, hi - lo, i + 1))
        if o["kind"] not in (L.OP_INPUT, L.OP_STEM):
            if o["src0"] >= 0:
                want.append((o["src0"], o["src0_coff"], o["src0_c"], i))
            if o["src1"] >= 0:
                want.append((o["src1"], o["src1_coff"], o["src1_c"], i))
            if o["kind"] in (L.OP_CONV, L.OP_CONVT) and o["res"] >= 0:
                want.append((o["res"], o["res_coff"], o["cout"], i))
        ids = set()
        for tid, coff, c, t in want:           # (more channels than the check reads does no harm: a tensor stays longer)
            ids |= {seg[1] for seg in self._segments(tid, coff, max(c, 1), t) if seg[0] == "tensor"}
        return ids

    def from_page(self, tid: int, t: int) -> bool:
        w = max((j for j in range(t) if self.rng[j] is not None and self.rng[j][0] == tid), default=None)
        return w is not None and self.p.ops[w]["kind"] == L.OP_INPUT and self._fused(w)

    def sources(self, o, t: int):
        """[(array (B,h,w,c), up)] of the op's (concatenated) sources."""
        s = [(self.value(o["src0"], o["src0_coff"], o["src0_c"], t, f64=False), o["src0_up"])]
        if o["src1"] >= 0:
            s.append((self.value(o["src1"], o["src1_coff"], o["src1_c"], t, f64=False), o["src1_up"]))
        return s

    # -- windows ------------------------------------------------------------------------------------------------------
    def windows(self, Ho: int, Wo: int, B: int, salt: int = 0, legacy: Optional[bool] = None):
        """(kept page position, y0, x0, h, w) of the output windows of a (B, Ho, Wo) map."""
        legacy = self.legacy if legacy is None else legacy
        if Ho <= FULL_MAX and Wo <= FULL_MAX:
            return [(b, 0, 0, Ho, Wo) for b in range(B)]
        ys = lambda v: min(max(v, 0), Ho - WIN)      # noqa: E731
        xs = lambda v: min(max(v, 0), Wo - WIN)      # noqa: E731
        pos = legacy_positions(Ho, Wo, self.seed, salt)
        if not legacy:
            pos = pos + geometry_positions(Ho, Wo)
        pos = sorted({(ys(y), xs(x)) for y, x in pos})
        on = sorted({0, B - 1}) if (self.pages is None or legacy) else range(B)
        return [(b, y, x, WIN, WIN) for b in on for y, x in pos]

    @staticmethod
    def crop(a: np.ndarray, b: int, r0: int, r1: int, c0: int, c1: int, up: int = 0) -> np.ndarray:
        """Rows [r0, r1) x cols [c0, c1) of page b of NHWC `a` seen through a nearest x2^up upsample, zero outside ->
        (C, r1 - r0, c1 - c0)."""
        Hl, Wl = a.shape[1] << up, a.shape[2] << up
        rr, cc = np.arange(r0, r1), np.arange(c0, c1)
        vr, vc = (rr >= 0) & (rr < Hl), (cc >= 0) & (cc < Wl)
        x = a[b][np.clip(rr, 0, Hl - 1) >> up][:, np.clip(cc, 0, Wl - 1) >> up]
        x = x * (vr[:, None, None] & vc[None, :, None])
        return np.ascontiguousarray(x.transpose(2, 0, 1), np.float64)

    def _par(self, off: int, n: int) -> np.ndarray:
        return self.blob[off: off + n]

    # -- one linear layer on a batch of windows ---------------------------------------------------------------------
    def _linear(self, x: torch.Tensor, w: np.ndarray, b, transposed: bool, s: int, K: int, *, stem: bool = False,
                paged: bool = False):
        """x (N,Cin,h,w) crops -> (v, A): the f64 pre-activation and its allowance for this engine."""
        op = F.conv_transpose2d if transposed else F.conv2d
        wt = _t(w)
        v = op(x, wt, None, s)
        S = op(x.abs(), wt.abs(), None, s)
        if b is not None:
            bt = _t(b).view(1, -1, 1, 1)
            v, S = v + bt, S + bt.abs()
        A = LAMBDA * math.sqrt(K) * U * S
        e = self.engine
        sumx = lambda: op(x.abs(), torch.ones_like(wt), None, s)                  # noqa: E731
        if e == "fp32s":
            A = A + op(_t(_split_err(x.numpy())), wt.abs(), None, s) + 2.0 ** -21 * S
            wmax = wt.abs().amax(dim=(0, 2, 3) if transposed else (1, 2, 3)).view(1, -1, 1, 1)
            A = A + 2.0 ** -33 * wmax * sumx()
        elif e == "fp16":
            A = A + 2.0 ** -11 * S + (2.0 ** -24 if (stem and self.u8) else 2.0 ** -25) * sumx()
            if stem:
                sw = op(torch.ones_like(x), wt.abs(), None, s)
                A = A + 2.0 ** -11 * S + 2.0 ** -25 * sw
        if paged:
            A = A + U * S
        return v.numpy(), A.numpy(), S.numpy()

    # -- per op -------------------------------------------------------------------------------------------------------
    def check(self, i: int) -> dict:
        o = self.p.ops[i]
        k = o["kind"]
        fn = {L.OP_INPUT: self._input, L.OP_STEM: self._conv, L.OP_CONV: self._conv, L.OP_CONVT: self._conv,
              L.OP_MAXPOOL: self._maxpool, L.OP_AVGPOOL2: self._avgpool, L.OP_DETECT: self._detect,
              L.OP_EXPORT: self._export, L.OP_SEG_FINAL: self._seg_final, L.OP_DB_UP: self._db_up}[k]
        r = fn(i, o)
        r.setdefault("name", o["name"])
        r["page"] = self.real[r["page"]] if r.get("page") is not None else None     # where the worst ratio is
        r.setdefault("win", None)
        r["total"] = r.pop("per_page", 0) * self.B_all                              # elements the op wrote, all pages
        return r

    def out_value(self, i: int, f64: bool = True) -> np.ndarray:
        tid, lo, hi = self.rng[i]
        return self.value(tid, lo, hi - lo, i + 1, f64)

    def _input(self, i, o):
        if self._fused(i):
            return dict(ratio=0.0, n=0, skipped=True)
        got = self.out_value(i)
        ref = np.concatenate([self.page.transpose(0, 2, 3, 1), np.zeros(got.shape[:3] + (got.shape[3] - 3,))], 3)
        ratio, pg = _ratio_pages(got, ref, U * np.abs(ref))
        return dict(ratio=ratio, page=pg, n=got.size, per_page=got[0].size)

    def conv_bounds(self, i: int, wins):
        """[(window, f64 reference (C,h,w), bound (C,h,w))] of conv op i on the given windows (kept page positions)."""
        out = []
        self._conv(i, self.p.ops[i], wins=wins, collect=out)
        return out

    def _conv(self, i, o, wins=None, collect=None):
        k, s, p = o["k"], o["stride"], o["pad"]
        kind = o["kind"]
        transposed = kind == L.OP_CONVT
        got_all = self.out_value(i, f64=False)
        Ho, Wo = got_all.shape[1:3]
        cout = o["cout"]
        if kind == L.OP_STEM:
            srcs = [(self.page.transpose(0, 2, 3, 1), 0)]
            paged = False
        else:
            srcs = self.sources(o, i)
            paged = any(self.from_page(t, i) for t in (o["src0"], o["src1"]) if t >= 0)
        cin = sum(a.shape[3] for a, _ in srcs)
        if transposed:
            w = self._par(o["w_off"], cin * cout * k * k).reshape(cin, cout, k, k)
            K = cin * (k // s) ** 2
        else:
            w = self._par(o["w_off"], cout * cin * k * k).reshape(cout, cin, k, k)
            K = cin * k * k
        b = self._par(o["b_off"], cout) if o["b_off"] >= 0 else None
        res = self.value(o["res"], o["res_coff"], cout, i, f64=False) if o["res"] >= 0 else None
        f32 = self.p.tensors[o["dst"]][2] == 1
        worst, n, at = 0.0, 0, None
        wins = self.windows(Ho, Wo, self.B, salt=i) if wins is None else wins
        for (h, ww), group in _by_size(wins).items():
            crops, offs = [], []
            for bb, y0, x0, _, _ in group:
                if transposed:
                    i0r, i0c = (y0 + p - k + 1) // s, (x0 + p - k + 1) // s       # a fixed-size crop that holds every
                    i1r, i1c = i0r + (h + k - 2) // s + 1, i0c + (ww + k - 2) // s + 1   # input of the window
                    crops.append(np.concatenate([self.crop(a, bb, i0r, i1r + 1, i0c, i1c + 1, up) for a, up in srcs], 0))
                    offs.append((y0 - (i0r * s - p), x0 - (i0c * s - p)))
                else:
                    r0, c0 = y0 * s - p, x0 * s - p
                    crops.append(np.concatenate([self.crop(a, bb, r0, r0 + (h - 1) * s + k, c0, c0 + (ww - 1) * s + k, up)
                                                 for a, up in srcs], 0))
                    offs.append((0, 0))
            v, A, _ = self._linear(_t(np.stack(crops)), w, b, transposed, s, K, stem=kind == L.OP_STEM, paged=paged)
            for j, (bb, y0, x0, _, _) in enumerate(group):
                oy, ox = offs[j]
                vj, Aj = v[j, :, oy: oy + h, ox: ox + ww], A[j, :, oy: oy + h, ox: ox + ww]
                y = _act(vj, o["act"])
                D = _act_err(vj, Aj, o["act"], y)
                if res is not None:
                    r = res[bb, y0: y0 + h, x0: x0 + ww].transpose(2, 0, 1).astype(np.float64)
                    y = y + r
                    D = D + U * np.abs(y) + (_split_err(r) if self.engine == "fp32s" else 0.0)
                D = D + storage_err(self.engine, np.abs(y) + D, f32)   # rounds the value the engine had
                got = got_all[bb, y0: y0 + h, x0: x0 + ww].transpose(2, 0, 1)
                if collect is not None:
                    collect.append(((bb, y0, x0, h, ww), y, D))
                r = _ratio(got, y, D)
                if at is None or r > worst:
                    worst, at = r, (bb, y0, x0)
                n += got.size
        return dict(ratio=worst, n=n, page=at[0], win=at[1:], per_page=got_all[0].size)

    def _maxpool(self, i, o):
        a = self.value(o["src0"], o["src0_coff"], o["src0_c"], i).astype(np.float32)
        ref = F.max_pool2d(torch.from_numpy(a.transpose(0, 3, 1, 2).copy()), o["k"], 1, o["k"] // 2).numpy()
        got = self.out_value(i).transpose(0, 3, 1, 2).astype(np.float32)
        bad = [b for b in range(len(ref)) if not np.array_equal(got[b], ref[b])]
        return dict(ratio=INF if bad else 0.0, page=bad[0] if bad else 0, n=got.size, exact=True, per_page=got[0].size)

    def _avgpool(self, i, o):
        a = self.value(o["src0"], o["src0_coff"], o["src0_c"], i)
        B, H, W, C = a.shape
        q = a.reshape(B, H // 2, 2, W // 2, 2, C)
        ref = q.mean(axis=(2, 4))
        D = 0.5 * U * np.abs(q).sum(axis=(2, 4))
        D = D + storage_err(self.engine, np.abs(ref) + D, self.p.tensors[o["dst"]][2] == 1)
        ratio, pg = _ratio_pages(self.out_value(i), ref, D)
        return dict(ratio=ratio, page=pg, n=ref.size, per_page=ref[0].size)

    def _detect(self, i, o):
        stride, row_unit, na, no = o["aux"][:4]
        raw = self.value(o["src0"], o["src0_coff"], na * no, i)            # (B, ny, nx, na*no)
        B, ny, nx, _ = raw.shape
        z = raw.reshape(B, ny, nx, na, no).transpose(0, 3, 1, 2, 4)      # (B, na, ny, nx, no)
        sg = _sig(z)
        es = 6 * U * sg
        gx = np.arange(nx).reshape(1, 1, 1, nx)
        gy = np.arange(ny).reshape(1, 1, ny, 1)
        anc = np.asarray(o["faux"][: 2 * na], np.float64).reshape(1, na, 1, 1, 2)
        ref, D = sg.copy(), es.copy()
        for j, g in ((0, gx), (1, gy)):
            t = 2 * sg[..., j] - 0.5 + g
            ref[..., j] = t * stride
            D[..., j] = stride * (2 * es[..., j] + U * (2 * sg[..., j] + np.abs(2 * sg[..., j] - 0.5) + 2 * np.abs(t)))
        for j in (2, 3):
            ref[..., j] = (2 * sg[..., j]) ** 2 * anc[..., j - 2]
            D[..., j] = 15 * U * np.abs(ref[..., j])
        unit = (self.H // 64) * (self.W // 64)
        r0 = row_unit * unit
        got = self.outs["blks"][:, r0: r0 + na * ny * nx]
        ratio, pg = _ratio_pages(got, ref.reshape(B, -1, no), D.reshape(B, -1, no))
        return dict(ratio=ratio, page=pg, n=got.size, per_page=got[0].size)

    def _export(self, i, o):
        a = self.value(o["src0"], o["src0_coff"], 1, i)[..., 0].astype(np.float32)
        which, plane = o["aux"][0], o["aux"][1]
        if which == L.OUT_MASK:
            ok = np.array_equal(self.outs["mask"][:, 0], a) and self._mask_u8_ok()
        else:
            ok = np.array_equal(self.outs["lines"][:, plane], a) and (plane != 0 or self._bitmap_ok(o))
        return dict(ratio=0.0 if ok else INF, page=0, n=a.size, exact=True, per_page=a[0].size)

    def _mask_u8_ok(self) -> bool:
        m = np.asarray(self.outs["mask"][:, 0], np.float32)
        return np.array_equal(self.outs["mask_u8"], (m * np.float32(255)).astype(np.uint8))

    def _bitmap_ok(self, o) -> bool:
        return np.array_equal(self.outs["bitmap"].astype(bool), self.outs["lines"][:, 0] > np.float32(o["faux"][0]))

    def _seg_final(self, i, o):
        a = self.value(o["src0"], o["src0_coff"], o["src0_c"], i, f64=False)
        cin = a.shape[3]
        w = self._par(o["w_off"], cin * 16).reshape(cin, 1, 4, 4)
        got_all = self.outs["mask"]
        worst, n, at = 0.0, 0, None
        for (h, ww), group in _by_size(self.windows(self.H, self.W, self.B, salt=i)).items():
            crops, offs = [], []
            for bb, y0, x0, _, _ in group:
                i0r, i0c = (y0 - 2) // 2, (x0 - 2) // 2                      # as in _conv: k = 4, s = 2, p = 1
                i1r, i1c = i0r + (h + 2) // 2 + 1, i0c + (ww + 2) // 2 + 1
                crops.append(self.crop(a, bb, i0r, i1r + 1, i0c, i1c + 1))
                offs.append((y0 - (i0r * 2 - 1), x0 - (i0c * 2 - 1)))
            v, A, _ = self._linear(_t(np.stack(crops)), w, None, True, 2, cin * 4)
            for j, (bb, y0, x0, _, _) in enumerate(group):
                oy, ox = offs[j]
                vj, Aj = v[j, 0, oy: oy + h, ox: ox + ww], A[j, 0, oy: oy + h, ox: ox + ww]
                y = _sig(vj)
                D = _act_err(vj, Aj, L.ACT["sigmoid"], y) + U * y
                r = _ratio(got_all[bb, 0, y0: y0 + h, x0: x0 + ww], y, D)
                if at is None or r > worst:
                    worst, at = r, (bb, y0, x0)
                n += h * ww
        return dict(ratio=worst if self._mask_u8_ok() else INF, n=n, page=at[0], win=at[1:], per_page=self.H * self.W)

    def _db_up(self, i, o):
        a = self.value(o["src0"], o["src0_coff"], o["src0_c"], i, f64=False)
        q = o["aux"][1]
        nbr = o["aux"][2] or 2
        pb = q * q * 4 + q + q * 4 + 1
        worst, n, at = 0.0, 0, None
        wins = _by_size(self.windows(self.H, self.W, self.B, salt=i))
        for br in range(nbr):
            prm = self._par(o["w_off"] + br * pb, pb)
            w1 = prm[: q * q * 4].reshape(q, q, 2, 2)
            b1 = prm[q * q * 4: q * q * 4 + q]
            w2 = prm[q * q * 4 + q: q * q * 4 + q + q * 4].reshape(q, 1, 2, 2)
            b2 = prm[q * q * 4 + q + q * 4:]
            got_all = self.outs["lines"][:, br]
            for (h, ww), group in wins.items():
                crops = [self.crop(a[..., br * q: (br + 1) * q], bb, y0 // 4, y0 // 4 + (h + 2) // 4 + 1, x0 // 4,
                                   x0 // 4 + (ww + 2) // 4 + 1) for bb, y0, x0, _, _ in group]
                vh, Ah, _ = self._linear(_t(np.stack(crops)), w1, b1, True, 2, q)
                hh = np.maximum(vh, 0.0)
                Eh = _act_err(vh, Ah, L.ACT["relu"], hh)
                Eh = Eh + storage_err(self.engine, hh + Eh)
                v, A, _ = self._linear(_t(hh), w2, b2, True, 2, q)
                A = A + F.conv_transpose2d(_t(Eh), _t(np.abs(w2)), None, 2).numpy()
                for j, (bb, y0, x0, _, _) in enumerate(group):
                    oy, ox = y0 - (y0 // 4) * 4, x0 - (x0 // 4) * 4
                    vj, Aj = v[j, 0, oy: oy + h, ox: ox + ww], A[j, 0, oy: oy + h, ox: ox + ww]
                    y = _sig(vj)
                    D = _act_err(vj, Aj, L.ACT["sigmoid"], y) + U * y
                    r = _ratio(got_all[bb, y0: y0 + h, x0: x0 + ww], y, D)
                    if at is None or r > worst:
                        worst, at = r, (bb, y0, x0)
                    n += h * ww
        return dict(ratio=worst if self._bitmap_ok(o) else INF, n=n, page=at[0], win=at[1:], per_page=nbr * self.H * self.W)

    def check_all(self, ops=None) -> Dict[int, dict]:
        """Checks the ops in program order; a tensor is dropped from the cache once no later op of `ops` reads it."""
        ops = sorted(range(len(self.p.ops)) if ops is None else ops)
        last = {}
        for i in ops:
            for tid in self.reads(i):
                last[tid] = i
        res = {}
        for i in ops:
            res[i] = self.check(i)
            for tid in [t for t in self._cache if last.get(t, -1) <= i]:
                del self._cache[tid]
        return res


def _by_size(wins):
    g: Dict[tuple, list] = {}
    for wdw in wins:
        g.setdefault((wdw[3], wdw[4]), []).append(wdw)
    return g
