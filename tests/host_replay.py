"""TEST INFRASTRUCTURE of tests/test_host_sanitizers.py: records calls of the native host entry points as case files for the
host-only replay harness (tests/native/host_replay.cpp) and reads its result files.

`Recorder` stands in for the loaded library (`_lib.lib()`) while one of the suite's existing generators drives the product's
own wrappers: every call of a host entry point goes to the SHIPPED library as before, and its raw argument buffers plus what the
library returned are kept as one case.  Input buffers are recorded at exactly the size the entry point may read, output
capacities as the caller passed them -- the wrappers pass the documented minimum of include/ctd_hip.h.

File format (cases and results; little endian):
    file = b"CTDRPLY1" case*          case = str name, str entry, u32 n_items, item*          str = u32 length, bytes
    item = str tag, u8 dtype code (b h i l I L f d), u8 present (0 = a NULL pointer), u32 ndim, u64 dims[ndim], bytes
Items tagged `exp.*` are the shipped library's results; the harness ignores them."""
import contextlib
import ctypes as C
import struct

import numpy as np

from conftest import pkg

MAGIC = b"CTDRPLY1"
CODES = {"b": np.uint8, "h": np.int16, "i": np.int32, "l": np.int64, "I": np.uint32, "L": np.uint64, "f": np.float32, "d": np.float64}
_CODE_OF = {np.dtype(v): k for k, v in CODES.items()}


class Absent:
    """A NULL pointer argument of element type `code`."""
    def __init__(self, code):
        self.code = code


def _wstr(f, s):
    b = s.encode()
    f.write(struct.pack("<I", len(b)) + b)


def write_cases(path, cases):
    with open(path, "wb") as f:
        f.write(MAGIC)
        for c in cases:
            _wstr(f, c["name"])
            _wstr(f, c["entry"])
            items = list(c["items"].items()) + [("exp." + k, v) for k, v in c.get("expected", {}).items()]
            f.write(struct.pack("<I", len(items)))
            for tag, v in items:
                _wstr(f, tag)
                if isinstance(v, Absent):
                    f.write(struct.pack("<cBIQ", v.code.encode(), 0, 1, 0))
                    continue
                a = np.ascontiguousarray(v)
                a = a.reshape(1) if a.ndim == 0 else a
                f.write(struct.pack("<cBI", _CODE_OF[a.dtype].encode(), 1, a.ndim) + struct.pack(f"<{a.ndim}Q", *a.shape))
                f.write(a.tobytes())


def read_results(path):
    """[(name, entry, {tag: array})] of a result (or case) file."""
    out = []
    with open(path, "rb") as f:
        buf = f.read()
    assert buf[:8] == MAGIC, "not a replay file"
    pos = 8

    def rstr():
        nonlocal pos
        n, = struct.unpack_from("<I", buf, pos)
        pos += 4 + n
        return buf[pos - n: pos].decode()

    while pos < len(buf):
        name, entry = rstr(), rstr()
        n_items, = struct.unpack_from("<I", buf, pos)
        pos += 4
        items = {}
        for _ in range(n_items):
            tag = rstr()
            code, present, ndim = struct.unpack_from("<cBI", buf, pos)
            pos += 6
            dims = struct.unpack_from(f"<{ndim}Q", buf, pos)
            pos += 8 * ndim
            dt = np.dtype(CODES[code.decode()])
            n = int(np.prod(dims)) if present else 0
            items[tag] = np.frombuffer(buf, dt, n, pos).reshape(dims if present else (0,)).copy()
            pos += n * dt.itemsize
        out.append((name, entry, items))
    return out


# ------------------------------------------------------------------------------------------------------------------ recorder

def _addr(a):
    if a is None:
        return None
    if isinstance(a, int):
        return a or None
    if hasattr(a, "_obj"):                     # ctypes.byref(x)
        return C.addressof(a._obj)
    if isinstance(a, C.c_void_p):
        return a.value
    return C.addressof(a)


def _read(a, code, count):
    """`count` elements of type `code` at pointer argument `a` (a copy), or `Absent`."""
    p = _addr(a)
    if p is None:
        return Absent(code)
    dt = np.dtype(CODES[code])
    return np.frombuffer(C.string_at(p, int(count) * dt.itemsize), dt).copy()


def _i32(v):
    return np.array([int(v)], np.int32)


def _f64(v):
    return np.array([float(v)], np.float64)


ERR_NOMEM = -4           # CTD_ERR_NOMEM (include/ctd_hip.h)
BLK_BYTES = 96          # sizeof(ctd_blk); checked against the package's ctypes struct in Recorder.__init__


def _rec_group_output(fn, a):
    (blines, cls, nb, lines, nl, im_w, im_h, mask, pitch, recs, blk_cap, lout, line_cap, dout, dist_cap, n_b, n_l, n_d) = a
    items = dict(blines=_read(blines, "i", 4 * nb), cls=_read(cls, "i", nb), n_blk=_i32(nb), lines=_read(lines, "i", 8 * nl),
                 n_lines=_i32(nl), im_w=_i32(im_w), im_h=_i32(im_h),
                 mask=_read(mask, "b", (im_h - 1) * pitch + im_w),          # the last row ends at the page's width
                 mask_pitch=_i32(pitch), blk_cap=_i32(blk_cap), line_cap=_i32(line_cap), dist_cap=_i32(dist_cap))
    rc = fn(*a)
    exp = dict(rc=_i32(rc))
    if rc == 0:
        cb, cl, cd = (int(_read(x, "i", 1)[0]) for x in (n_b, n_l, n_d))
        exp.update(n_blk_out=_i32(cb), n_lines_out=_i32(cl), n_dist_out=_i32(cd), blks=_read(recs, "b", BLK_BYTES * cb),
                   lines_out=_read(lout, "i", 8 * cl), dist_out=_read(dout, "d", 3 * cd))
    return rc, items, exp


def _exp_boxes(rc, boxes, scores, n):
    exp = dict(rc=_i32(rc))
    if rc == 0:
        k = int(_read(n, "i", 1)[0])
        exp.update(n_out=_i32(k), boxes=_read(boxes, "h", 8 * k), scores=_read(scores, "f", k))
    return exp


def _rec_db_boxes(fn, a):
    prob, lab_f, st_f, n_f, lab_b, st_b, n_b, W, H, cap, unclip, boxes, scores, n = a
    items = dict(prob=_read(prob, "f", W * H), lab_f=_read(lab_f, "i", W * H), st_f=_read(st_f, "i", 5 * n_f), n_f=_i32(n_f),
                 lab_b=_read(lab_b, "i", W * H), st_b=_read(st_b, "i", 5 * n_b), n_b=_i32(n_b), W=_i32(W), H=_i32(H),
                 max_candidates=_i32(cap), unclip_ratio=_f64(unclip))
    rc = fn(*a)
    return rc, items, _exp_boxes(rc, boxes, scores, n)


def _rec_db_boxes_compact(fn, a):
    (W, H, n_f, st_f, first_f, par_f, off_f, sum_f, n_b, st_b, first_b, par_b, off_b, sum_b, ring_sum, ring_cnt, row_lo, row_hi,
     cap, unclip, boxes, scores, n) = a
    items = dict(W=_i32(W), H=_i32(H), n_f=_i32(n_f), st_f=_read(st_f, "i", 5 * n_f), first_f=_read(first_f, "i", n_f),
                 par_f=_read(par_f, "i", n_f), off_f=_read(off_f, "i", n_f), sum_f=_read(sum_f, "d", n_f), n_b=_i32(n_b),
                 st_b=_read(st_b, "i", 5 * n_b), first_b=_read(first_b, "i", n_b), par_b=_read(par_b, "i", n_b),
                 off_b=_read(off_b, "i", n_b), sum_b=_read(sum_b, "d", n_b), ring_sum=_read(ring_sum, "d", n_b),
                 ring_cnt=_read(ring_cnt, "i", n_b), max_candidates=_i32(cap), unclip_ratio=_f64(unclip))
    # row tables: exactly the rows the component tables address (h rows per component, h + 2 per hole's ring)
    rows = 0
    if n_f:
        rows = max(rows, int((items["off_f"] + items["st_f"].reshape(-1, 5)[:, 3]).max()))
    if n_b:
        hole = items["par_b"] > 0
        if hole.any():
            rows = max(rows, int((items["off_b"] + items["st_b"].reshape(-1, 5)[:, 3] + 2)[hole].max()))
    items.update(row_lo=_read(row_lo, "i", rows), row_hi=_read(row_hi, "i", rows))
    rc = fn(*a)
    return rc, items, _exp_boxes(rc, boxes, scores, n)


def _rec_topk(fn, a):
    items = dict(hist=_read(a[0], "l", 256))
    rc = fn(*a)
    return rc, items, dict(rc=_i32(rc), colors=_read(a[1], "d", 3))


def _rec_otsu(fn, a):
    items = dict(hist=_read(a[0], "l", 256))
    rc = fn(*a)
    return rc, items, dict(rc=_i32(rc))


def _rec_inrange(fn, a):
    fn(*a)
    return None, dict(lo=_f64(a[0]), hi=_f64(a[1])), dict(lb=_read(a[2], "i", 1), ub=_read(a[3], "i", 1))


def _rec_gather(fn, a):
    dst, srcs, sizes, n, threads = a
    sz = _read(sizes, "L", n)
    items = dict(n=_i32(n), threads=_i32(threads), sizes=sz, dst_null=_i32(_addr(dst) is None))
    total = 0
    if not isinstance(sz, Absent):
        ptrs = np.frombuffer(C.string_at(_addr(srcs), 8 * n), np.uint64)
        for i in range(n):
            items[f"src{i}"] = _read(int(ptrs[i]), "b", int(sz[i]))
            total += int(sz[i])
    rc = fn(*a)
    return rc, items, dict(rc=_i32(rc), dst=_read(dst, "b", total) if rc == 0 and _addr(dst) else np.zeros(0, np.uint8))


_RECORDERS = {"ctd_group_output": _rec_group_output, "ctd_db_boxes": _rec_db_boxes, "ctd_db_boxes_compact": _rec_db_boxes_compact,
              "ctd_topk_colors": _rec_topk, "ctd_otsu_from_hist": _rec_otsu, "ctd_inrange_bounds": _rec_inrange,
              "ctd_host_gather": _rec_gather}


class Recorder:
    """Stands in for the ctypes library object: host entry points are recorded, everything else passes through."""

    def __init__(self):
        self._L = pkg()._lib
        self._real = self._L.lib()
        assert C.sizeof(self._L.CtdBlk) == BLK_BYTES
        self.cases = []
        self.label, self.tied = "", False

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        rec = _RECORDERS.get(name)
        if rec is None:
            return fn

        def call(*a):
            rc, items, exp = rec(fn, a)
            self.add(name, items, exp)
            return rc
        return call

    def add(self, entry, items, expected, tied=None):
        self.cases.append(dict(name=f"{len(self.cases):04d} {self.label}", entry=entry, items=items, expected=expected,
                               tied=self.tied if tied is None else tied))

    @contextlib.contextmanager
    def recording(self, label, tied=False):
        """Calls made through the package inside this block are recorded under `label`; `tied`: the generator CONSTRUCTS ties
        (lines of one row, histogram bins of equal count), so numpy's arccos / argsort may order the results differently from
        libm / a stable sort."""
        old = self._L._lib
        self._L._lib, self.label, self.tied = self, label, tied
        try:
            yield self
        finally:
            self._L._lib = old


# ------------------------------------------------------------------------------------------------------------------ case set

def _labels(prob):
    from oracle import postproc_ref as R
    bitmap = prob > 0.3
    _, lab_f, st_f = R.connected_components_with_stats(bitmap.astype(np.uint8), 8)
    _, lab_b, st_b = R.connected_components_with_stats((~bitmap).astype(np.uint8), 4)
    return bitmap, lab_f, st_f[1:], lab_b, st_b[1:]


def _db_cases(rec, label, prob, caps=(1000,), compact=True):
    """`ctd_db_boxes` at every capacity of `caps`, plus at EXACTLY the contour count and one below it (truncation), and the
    same map through the compact tables.  Every case carries what must come out (`intent`): n_out = min(cap, contours), the
    contour count taken from the label images (components + background regions off the frame), not from the library."""
    import dbc_emul
    p = pkg()
    prob = np.ascontiguousarray(prob, np.float32)
    H, W = prob.shape
    bitmap, lab_f, st_f, lab_b, st_b = _labels(prob)
    holes = sum(1 for x, y, w, h, _ in st_b if x > 0 and y > 0 and x + w < W and y + h < H)
    n_contours = len(st_f) + holes
    all_caps = list(caps) + sorted({n_contours, max(n_contours - 1, 0)})
    for cap in all_caps:
        with rec.recording(f"{label} cap {cap} (contours {n_contours})"):
            p.postproc.SegRepresenter(max_candidates=cap)._page(prob, lab_f, st_f, lab_b, st_b, W, H)
        rec.cases[-1]["intent"] = dict(rc=0, n_out=min(cap, n_contours), contours=n_contours)
    if compact:
        t = dbc_emul.dbc_tables(prob, bitmap)
        for cap in all_caps:
            with rec.recording(f"{label} compact cap {cap} (contours {n_contours})"):
                dbc_emul.boxes_from_tables(p, t, max_candidates=cap)
            rec.cases[-1]["intent"] = dict(rc=0, n_out=min(cap, n_contours), contours=n_contours)


def _group_case(rec, label, blks, lines, im_w, im_h, mask, tied=False, tight=False):
    """One `group_output` call through the product's wrapper (capacities = the documented minimum); with `tight` also at
    EXACTLY what the page needs, and at one below that in each of the three pools (CTD_ERR_NOMEM)."""
    p = pkg()
    with rec.recording(label, tied):
        recs, lout, dout = p.textblock.group_output_native(blks[0], blks[1], lines, im_w, im_h, mask)
    rec.cases[-1]["py"] = (blks, lines, im_w, im_h, mask)          # for the oracle (tests/test_host_sanitizers.py)
    if not tight:
        return
    need = (len(recs), len(lout), len(dout))
    src = rec.cases[-1]["items"]
    for which in (None, 0, 1, 2):
        caps = list(need)
        if which is not None:
            if need[which] == 0:
                continue
            caps[which] -= 1
        _group_raw(rec, f"{label} caps {caps} (needs {list(need)})", src, caps, tied)
        # what must come out: one below the need in any pool is CTD_ERR_NOMEM, exactly the need is enough
        rec.cases[-1]["intent"] = dict(rc=0, counts=list(need)) if which is None else dict(rc=ERR_NOMEM)


def _group_raw(rec, label, src, caps, tied=False, mask=None, pitch=None):
    """`ctd_group_output` on the recorded inputs `src` with the given capacities (and optionally another mask / pitch)."""
    L = pkg()._lib
    arr = lambda k: None if isinstance(src[k], Absent) else src[k]                                   # noqa: E731
    ptr = lambda a: None if a is None else a.ctypes.data                                            # noqa: E731
    mask = arr("mask") if mask is None else mask
    pitch = int(src["mask_pitch"][0]) if pitch is None else pitch
    recs = (L.CtdBlk * max(caps[0], 1))()
    lout, dout = np.zeros((max(caps[1], 1), 8), np.int32), np.zeros((max(caps[2], 1), 3), np.float64)
    n = [C.c_int32(), C.c_int32(), C.c_int32()]
    with rec.recording(label, tied):
        return rec.ctd_group_output(ptr(arr("blines")), ptr(arr("cls")), int(src["n_blk"][0]), ptr(arr("lines")),
                                    int(src["n_lines"][0]), int(src["im_w"][0]), int(src["im_h"][0]), ptr(mask), pitch, recs,
                                    caps[0], lout.ctypes.data, caps[1], dout.ctypes.data, caps[2], *(C.byref(x) for x in n))


def refine_rules_expected(hist4):
    """`refine_rules` (csrc/host_refine.h) from the oracle's restatements: np.histogram(bins=255) + get_topk_color, the
    cv2.inRange bounds around each colour (textmask.py:63-69), Otsu per channel."""
    from oracle import cv_ref as cv
    from oracle import postproc_ref as R
    px = np.repeat(np.arange(256, dtype=np.uint8), hist4[0].astype(np.int64))
    counts, edges = np.histogram(px, bins=255)
    rules = np.zeros((6, 3), np.int32)
    rules[:3, 0] = -1
    for k, color in enumerate(R.get_topk_color(edges, counts, k=3, color_var=10)):
        c_top = min(color + 30, 255)
        lo, hi = cv.in_range_bounds(c_top - 60, c_top)
        rules[k] = (0, lo, hi) if lo <= hi else (0, 1, 0)
    for ch in range(3):
        cpx = np.repeat(np.arange(256, dtype=np.uint8), hist4[1 + ch].astype(np.int64))
        rules[3 + ch] = (1 + ch, cv.otsu_threshold_value(cpx) if len(cpx) else 0, 0)
    return rules.reshape(-1)


def refine_windows(n=120):
    """(label, image (h,w,3) u8, predicted mask (h,w) u8) of small text-block windows: noise, strokes on a flat background,
    grey images (B = G = R: the three Otsu channels tie, the first wins), constant images, empty and full masks."""
    rng = np.random.RandomState(29)
    kinds = ("noise", "dark strokes on a flat background", "grey image", "constant image", "empty mask", "full mask")
    for i in range(n):
        h, w = int(rng.randint(6, 40)), int(rng.randint(6, 48))
        kind = i % 6
        msk = (rng.rand(h, w) < rng.uniform(0.1, 0.6)).astype(np.uint8) * int(rng.randint(128, 256))
        img = rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
        if kind == 1:
            img = np.broadcast_to(rng.randint(150, 256, 3), (h, w, 3)).astype(np.uint8).copy()
            img[msk > 0] = rng.randint(0, 90, 3)
            img = np.clip(img.astype(np.int64) + rng.randint(-6, 7, img.shape), 0, 255).astype(np.uint8)
        elif kind == 2:
            img[..., 1] = img[..., 2] = img[..., 0]
        elif kind == 3:
            img[:] = rng.randint(0, 256)
        elif kind == 4:
            msk[:] = 0
        elif kind == 5:
            msk[:] = 255
        yield f"window {i} ({kinds[kind]}) {h}x{w}", img, np.ascontiguousarray(msk)


def refine_window_expected(img, msk, libm_side=True):
    """(hist4, rules, sums, npix, expected candidates) of one window from the ORACLE's restatement of reference
    utils/textmask.py, with numpy on the libm side as in the harness (`libm_side=False`: numpy as it is, which is what the
    product inside a Python process calls, csrc/np_dispatch.h -- tests/tail_trace_cases.py): the colour candidates of `get_topk_masklist` and the
    Otsu candidate of `get_otsuthresh_masklist` -- each through `minxor_thresh` -- in the order `merge_mask_list` sorts them.
    The lists are rebuilt here from the same oracle calls only to know WHICH rule each candidate is; the distances are
    checked against the oracle's own functions."""
    from oracle import cv_ref as cv
    from oracle import postproc_ref as R
    with numpy_on_the_libm_side() if libm_side else contextlib.nullcontext():
        grey = cv.cvt_bgr2gray(img)
        sel = grey[np.where(cv.erode(msk, cv.RECT3, 1) > 127)]
        hist4 = np.stack([np.bincount(sel, minlength=256)] + [np.bincount(img[..., c].ravel(), minlength=256) for c in range(3)])
        hist4 = hist4.astype(np.uint32)
        rules = refine_rules_expected(hist4)
        sums, cands, otsu = np.zeros(6, np.uint64), [], []
        bin_, his = np.histogram(sel, bins=255)
        for k, color in enumerate(R.get_topk_color(his, bin_, color_var=10, k=3)):
            c_top = min(color + 30, 255)
            threshed = cv.in_range(grey, c_top - 60, c_top)
            sums[k] = np.bitwise_xor(threshed, msk).sum(dtype=np.uint64)
            chosen, xor_sum = R.minxor_thresh(threshed, msk)
            cands.append([k, int(chosen is not threshed), xor_sum])
        for c in range(3):
            _, threshed = cv.threshold_otsu(np.ascontiguousarray(img[..., c]))
            sums[3 + c] = np.bitwise_xor(threshed, msk).sum(dtype=np.uint64)
            chosen, xor_sum = R.minxor_thresh(threshed, msk)
            otsu.append([3 + c, int(chosen is not threshed), xor_sum])
        otsu.sort(key=lambda x: x[2])
        cands.append(otsu[0])
        cands.sort(key=lambda x: x[2])
        whole = R.get_topk_masklist(img, msk) + R.get_otsuthresh_masklist(img, msk)
        whole.sort(key=lambda x: x[1])
    assert [x[1] for x in whole] == [c[2] for c in cands]
    rule, inv, dist = np.zeros(4, np.int32), np.zeros(4, np.int32), np.zeros(4, np.uint64)
    for i, (k, v, d) in enumerate(cands):
        rule[i], inv[i], dist[i] = k, v, d
    return hist4, rules, sums, img.shape[0] * img.shape[1], dict(rc=_i32(len(cands)), cand_rule=rule, cand_invert=inv, cand_dist=dist)


@contextlib.contextmanager
def numpy_on_the_libm_side():
    """numpy's `arccos` / default-kind `argsort` replaced by what a process without numpy has in csrc/np_dispatch.h: libm's
    acos, a stable sort.  For the ORACLE: what the reference's code gives where numpy takes neither SVML nor x86-simd-sort."""
    import math
    acos, argsort = np.arccos, np.argsort

    def arccos_libm(x, *a, **k):
        x = np.asarray(x, np.float64)
        return np.array([math.acos(v) if -1.0 <= v <= 1.0 else math.nan for v in x.reshape(-1).tolist()]).reshape(x.shape)

    def argsort_stable(a, *args, **kw):
        kw.setdefault("kind", "stable")
        return argsort(a, *args, **kw)
    np.arccos, np.argsort = arccos_libm, argsort_stable
    try:
        yield
    finally:
        np.arccos, np.argsort = acos, argsort


def topk_by_the_oracle(px, libm_side=False):
    from oracle import postproc_ref as R
    counts, edges = np.histogram(px, bins=255)
    with numpy_on_the_libm_side() if libm_side else contextlib.nullcontext():
        return [float(c) for c in R.get_topk_color(edges, counts, k=3, color_var=10)]


def _refine_inputs():
    """(pixels, bound pairs) of `test_refine_host_decisions_match_oracle`: its own generator."""
    import test_post_host as TP
    return TP.refine_decision_inputs()


def histograms():
    """(label, pixels u8, tied) of the 300 histograms above and of `sweep_cases.tied_sweep`.  Of the 300, `tied` is decided
    from the oracle alone: a histogram whose colour pick depends on the order numpy's argsort gives bins of EQUAL count (the
    empty bins of a sparse histogram tie, and the pick reaches them whenever no bin falls below the 0.1 % cut first) differs
    between the oracle with numpy's own sort and the oracle with a stable one."""
    import sweep_cases as S
    for it, px in enumerate(_refine_inputs()[0]):
        yield f"histogram {it}", px, topk_by_the_oracle(px) != topk_by_the_oracle(px, libm_side=True)
    for case, px, what in S.tied_sweep():
        yield what, px, True


def build_case_set():
    """The case set of tests/test_host_sanitizers.py; returns the `Recorder` (`.cases`)."""
    import test_group_native as TG
    import test_post_host as TP
    p = pkg()
    rec = Recorder()

    # ---- ctd_group_output
    for seed in range(20):
        blks, lines, im_w, im_h, mask = TG.random_page(seed)
        _group_case(rec, f"random_page {seed}", blks, lines, im_w, im_h, mask if seed % 5 else None, tight=seed % 4 == 1)
    for seed in range(10):
        blks, lines, im_w, im_h, mask = TG.grid_page(seed)
        # no exact-capacity variants here: where the order of tied lines decides a split, what a page NEEDS differs between
        # numpy's order (the record) and a stable sort (the harness)
        _group_case(rec, f"grid_page {seed}", blks, lines, im_w, im_h, mask, tied=True)
    blks, lines, W, H, mask = TP.hand_built_scene()
    _group_case(rec, "hand-built scene", blks, lines, W, H, mask, tight=True)
    _group_case(rec, "hand-built scene, no mask", blks, lines, W, H, None)
    none = (np.zeros((0, 4), np.int32), np.zeros((0,), np.int32), np.zeros((0,)))
    _group_case(rec, "empty inputs", none, [], W, H, mask, tight=True)
    _group_case(rec, "no blocks, one line, no mask", none, np.array([[[10, 10], [100, 10], [100, 30], [10, 30]]], np.int32), 640,
                480, None, tight=True)
    _group_case(rec, "blocks without lines", (np.array([[5, 5, 60, 40], [-20, 300, 80, 420]], np.int32), np.array([1, 0], np.int32),
                                              np.ones(2)), [], W, H, None, tight=True)
    blks, lines, im_w, im_h, mask = TG.random_page(3, im_w=1800, im_h=900)
    _group_case(rec, "random_page 3 wide (two-page reading order)", blks, lines, im_w, im_h, mask)
    # a mask whose pitch exceeds its width: the same page from a wider allocation
    blks, lines, im_w, im_h, mask = TG.random_page(7)
    _group_case(rec, "random_page 7", blks, lines, im_w, im_h, mask)
    src = rec.cases[-1]
    wide = np.full((im_h, im_w + 37), 255, np.uint8)
    wide[:, :im_w] = mask
    need = [int(src["expected"][k][0]) for k in ("n_blk_out", "n_lines_out", "n_dist_out")]
    _group_raw(rec, "random_page 7, mask pitch = width + 37", src["items"], need, mask=wide.reshape(-1)[: (im_h - 1) * (im_w + 37) + im_w],
               pitch=im_w + 37)
    rec.cases[-1]["same_as"] = src["name"]

    # ---- ctd_db_boxes / ctd_db_boxes_compact
    # seed 226: one of the pages of the round-6 seed sweep (tests/test_post_host.py) -- two lines of one text row tie.  Seed 1
    # is left out on purpose: two of the 42 lines of one of its blocks have EXACTLY equal distances (359.5), and numpy's argsort
    # hands the pair's (c, d) operands back in the other order than a stable sort -- a tie no generator constructed
    for seed, tied in ((0, False), (2, False), (3, False), (226, True)):
        page, mask_u8, prob, blks = TP.fake_outputs(seed)
        _db_cases(rec, f"fake_outputs {seed}", prob, compact=seed in (0, 226))
        bitmap, lab_f, st_f, lab_b, st_b = _labels(prob)
        boxes, scores = p.postproc.SegRepresenter()._page(prob, lab_f, st_f, lab_b, st_b, prob.shape[1], prob.shape[0])
        _group_case(rec, f"fake_outputs {seed} lines", blks, boxes[scores > 0.6].astype(np.int32), prob.shape[1], prob.shape[0],
                    mask_u8, tied=tied, tight=seed == 2)
    for case in TP.EDGE_CASES:
        pr, cap = TP.edge_case_map(case)
        _db_cases(rec, f"edge case {case}", pr, caps=(1000,) if cap == 1000 else (cap, 1000))
    for seed in range(12):
        _db_cases(rec, f"speckle {seed}", TP.speckle_map(seed))
    import os
    gold = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "db_short_side_ties.npz"))
    for key in ("map0", "map1"):
        _db_cases(rec, f"short side of two pixels {key}", gold[key])
    # components that touch each page edge, a hole whose first pixel lies in column 1 (the `fx - 1` read), a hole in the
    # last-but-one column and row, single pixels in the four corners
    pr = np.full((40, 56), 0.05, np.float32)
    pr[0:6, 10:30] = 0.9
    pr[34:40, 10:30] = 0.8
    pr[10:30, 0:8] = 0.9
    pr[12:28, 1:5] = 0.1
    pr[10:30, 48:56] = 0.7
    pr[12:28, 51:55] = 0.1
    pr[33:40, 40:56] = 0.9
    pr[35:39, 42:55] = 0.2
    pr[0, 0] = pr[0, 55] = pr[39, 0] = 0.95
    _db_cases(rec, "components on every page edge, holes in column 1 and next to the last column / row", pr)

    # ---- histograms: ctd_topk_colors, ctd_otsu_from_hist, refine_rules, refine_candidates
    rng = np.random.RandomState(17)
    hists = []
    for i, (label, px, tied) in enumerate(histograms()):
        hist = np.bincount(px, minlength=256).astype(np.int64)
        hists.append(hist)
        out = np.zeros(3, np.float64)
        with rec.recording(label, tied):
            rec.ctd_topk_colors(hist.ctypes.data, out.ctypes.data)
            rec.cases[-1]["py"] = px
            rec.ctd_otsu_from_hist(hist.ctypes.data)
        # the window's 4 histograms: this one for the selected grey pixels, the three before it for B, G, R
        hist4 = np.stack([hists[max(len(hists) - 1 - k, 0)] for k in range(4)]).astype(np.uint32)
        # expected on the harness's side of csrc/np_dispatch.h (libm, a stable sort): the oracle with numpy put there
        with numpy_on_the_libm_side():
            rules = refine_rules_expected(hist4)
        rec.label = label
        rec.add("refine_rules", dict(hist4=hist4.reshape(-1)), dict(rules=rules), tied=tied)
        # xor sums that tie (no values to expect: what `refine_candidates` must return is checked on the windows below; these
        # run under the sanitizers and must come out the same in every flavour)
        npix = int(rng.randint(1, 1 << 20))
        sums = rng.randint(0, 255 * npix + 1, 6).astype(np.uint64)
        if i % 3 == 0:
            sums[4] = sums[3]
        if i % 5 == 0:
            sums[0] = 255 * npix - sums[0] if i % 2 else sums[5]
        if i % 7 == 0:
            sums[1] = 255 * npix // 2 + (255 * npix) % 2 * (i % 2)
        rec.add("refine_candidates", dict(rules=rules, sums=sums, npix=np.array([npix], np.int64)), {}, tied=False)
    for label, img, msk in refine_windows():
        hist4, rules, sums, npix, want = refine_window_expected(img, msk)
        rec.label = label
        rec.add("refine_rules", dict(hist4=hist4.reshape(-1)), dict(rules=rules), tied=False)
        rec.add("refine_candidates", dict(rules=rules, sums=sums, npix=np.array([npix], np.int64)), want, tied=False)
    for lo, hi in _refine_inputs()[1]:
        lb, ub = C.c_int32(), C.c_int32()
        with rec.recording(f"inrange {lo!r} {hi!r}"):
            rec.ctd_inrange_bounds(float(lo), float(hi), C.byref(lb), C.byref(ub))

    # ---- ctd_host_gather
    g = np.random.RandomState(23)
    for label, sizes, threads in [("zero buffers", [], 4), ("one buffer", [4097], 4), ("sizes 0 and 1 mixed in", [0, 1, 300, 0, 1, 0, 77], 3),
                                  ("more threads than buffers", [64, 1, 5000], 16), ("one thread", [10, 20, 30], 1),
                                  ("threads 0", [3, 0, 9], 0), ("eight pages", [196608] * 8, 8)]:
        bufs = [g.randint(0, 256, s).astype(np.uint8) for s in sizes]
        n = len(bufs)
        dst = np.zeros(sum(sizes), np.uint8)
        ptrs = (C.c_void_p * max(n, 1))(*[b.ctypes.data if b.size else None for b in bufs])
        sz = (C.c_size_t * max(n, 1))(*sizes)
        with rec.recording(f"gather: {label}"):
            rc = rec.ctd_host_gather(dst.ctypes.data if n else None, ptrs if n else None, sz if n else None, n, threads)
        assert rc == 0 and np.array_equal(dst, np.concatenate(bufs) if n else dst), label
    return rec
