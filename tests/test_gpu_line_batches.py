"""-m gpu: OCR input batches -- `ctd_warp_region_batches` (csrc/kernels_region.hip `region_batch_kernel`),
`regions.line_batches` / `TextDetector.line_batches` and `detect_stream(line_batches=...)`.  Every comparison is EXACT: the
warp arithmetic is the restatement's (tests/region_ref.py), the value map a table numpy builds, so expected elements are
`table[c][warp]` inside a slot's crop and `table[c][pad]` elsewhere, compared as bit patterns."""
import numpy as np
import pytest
import torch

import region_ref as R
import test_gpu_regions as TG
from conftest import pkg

pytestmark = pytest.mark.gpu

TH = TG.TH
TBITS = {torch.uint8: torch.uint8, torch.float16: torch.int16, torch.float32: torch.int32}


def bits(t: torch.Tensor) -> np.ndarray:
    """The bit patterns of a device tensor, on the host."""
    return t.contiguous().view(TBITS[t.dtype]).cpu().numpy()


def expect(u8: np.ndarray, tables: np.ndarray, rgb: bool, layout: str) -> np.ndarray:
    """(n, th, W, C) uint8 page values -> the batch tensor: channel order, value table, layout (numpy, bit patterns)."""
    ch = u8.shape[3]
    src = u8[..., ::-1] if rgb else u8
    out = np.stack([tables[c][src[..., c]] for c in range(ch)], axis=3)
    if layout == "nchw":
        out = out.transpose(0, 3, 1, 2)
    return np.ascontiguousarray(out).view({1: np.uint8, 2: np.int16, 4: np.int32}[out.dtype.itemsize])


# ---- 1. the kernel ---------------------------------------------------------------------------------------------------------

_KERNEL = {}


def kernel_case(channels):
    """Pages, jobs, their restated crops and the slots (shared by every parametrisation; the reference is computed once)."""
    if channels in _KERNEL:
        return _KERNEL[channels]
    RG = pkg().regions
    rng = np.random.default_rng(channels)
    shapes = [(61, 83), (120, 97), (33, 150)]
    imgs = [rng.integers(0, 256, s + ((3,) if channels == 3 else ()), dtype=np.uint8) for s in shapes]
    dev = torch.device("cuda:0")
    wide = torch.zeros((120, 131) + ((3,) if channels == 3 else ()), dtype=torch.uint8, device=dev)
    wide[:, 17:17 + 97] = torch.from_numpy(imgs[1]).to(dev)
    pages = [torch.from_numpy(imgs[0]).to(dev), wide[:, 17:17 + 97], torch.from_numpy(imgs[2]).to(dev)]
    pages, ch, _ = RG._device_pages(pages, dev)
    assert ch == channels and not pages[1].is_contiguous()       # the pitched view is read through its pitch
    base = TG._kernel_jobs(imgs)
    ref = [None if w == 0 else R.warp(imgs[pi], Minv, w, h, rot).reshape((w, h, ch) if rot else (h, w, ch))
           for pi, Minv, w, h, rot in base]
    size = lambda k: ref[k].shape[:2]                            # noqa: E731  (rows, cols) of the stored crop

    # job rows of the launch: (base job, batch, slot, cut); batches: (n, rows, Wk).  Jobs without a slot have batch -1.
    rows_of, batches = [], []

    def add_batch(members, rows, Wk, cuts=None):
        k = len(batches)
        batches.append((len(members), rows, Wk))
        for s, j in enumerate(members):
            rows_of.append((j, k, s, min(size(j)[1], Wk) if cuts is None else cuts[s]))

    groups = {}
    for j, r in enumerate(ref):
        if r is None:
            rows_of.append((j, -1, 0, 0))                        # empty jobs: first, in the middle, last
        else:
            groups.setdefault(size(j)[0], []).append(j)
    for rows, members in sorted(groups.items()):                 # every job once: batches of <= 3 crops of one height,
        for a in range(0, len(members), 3):                      # as wide as the widest (cut == Wk there, padding elsewhere)
            part = members[a: a + 3]
            add_batch(part, rows, max(size(j)[1] for j in part))
    find = lambda rows, cols: [j for j in range(len(base)) if ref[j] is not None and size(j) == (rows, cols)][:3]   # noqa: E731
    sq = find(32, 32)
    assert len(sq) == 3
    add_batch(sq, 32, 32)                                        # a slot of exactly one tile
    add_batch(sq, 32, 33)                                        # one tile plus one column
    odd = find(17, 33)
    assert len(odd) == 3
    add_batch(odd, 17, 33)                                       # odd rows x odd Wk x odd C: slots 1, 2 at odd element offsets
    add_batch(find(13, 21), 13, 22)                              # cut == Wk - 1
    big = find(48, 64)
    assert len(big) == 3
    add_batch(big, 48, 41, cuts=[40, 41, 17])                    # cut < w (truncated), with and without padding
    add_batch(big[:2], 48, 40)                                   # truncated, cut == Wk
    add_batch(find(1, 1), 1, 1)                                  # 1 x 1 crops in 1 x 1 slots
    add_batch(find(1, 1)[:2], 3, 5)                              # a slot higher than its crop: rows below it are padding
    add_batch([0, sq[0]], 32, 35, cuts=[0, 32])                             # an EMPTY job given a slot: all padding
    rows_of.insert(len(rows_of) // 2, (0, -1, 0, 0))
    rows_of.append((len(base) - 1, -1, 0, 0))
    _KERNEL[channels] = (pages, imgs, base, ref, rows_of, batches)
    return _KERNEL[channels]


@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
@pytest.mark.parametrize("dtype", [torch.uint8, torch.float16, torch.float32], ids=["u8", "f16", "f32"])
@pytest.mark.parametrize("channels", [3, 1])
def test_batch_kernel_equals_the_restatement_on_every_element(channels, dtype, layout):
    """`ctd_warp_region_batches` given explicit jobs and slots: EVERY element of every batch tensor equals
    table[c][restated warp] inside the slot's kept columns and table[c][pad] elsewhere, for rgb False / True and pad 0 / 200."""
    p = pkg()
    RG = p.regions
    pages, imgs, base, ref, rows_of, batches = kernel_case(channels)
    ch = channels
    if dtype == torch.uint8:
        tables = RG.value_tables(dtype, ch)
    else:                                                        # a different table per channel: a swapped channel shows
        tables = RG.value_tables(dtype, ch, [10.0, 120.5, 200.0][:ch], [50.0, 60.25, 70.0][:ch])
    jb = [base[r[0]] for r in rows_of]
    wh = np.array([[j[2], j[3]] for j in jb])
    n_el = n_bad = 0
    for rgb, pad in ((False, 0), (True, 200), (False, 200), (True, 0)):
        storage, offsets = RG.warp_batches(pages, [j[0] for j in jb], wh, np.array([j[1] for j in jb]), [j[4] for j in jb], ch,
                                           [r[1] for r in rows_of], [r[2] for r in rows_of], [r[3] for r in rows_of],
                                           [b[0] for b in batches], [b[2] for b in batches], [b[1] for b in batches],
                                           dtype, layout, tables, rgb, pad)
        torch.cuda.synchronize()
        assert storage.dtype == dtype and storage.dim() == 1
        item = storage.element_size()
        assert all((int(o) * item) % 16 == 0 for o in offsets) and storage.data_ptr() % 16 == 0
        buf = bits(storage)
        odd_f16 = 0
        for k, (n, rows, Wk) in enumerate(batches):
            u8 = np.full((n, rows, Wk, ch), pad, np.uint8)
            for j, kk, s, cut in rows_of:
                if kk == k and ref[j] is not None:
                    rr = min(rows, ref[j].shape[0])
                    u8[s, :rr, :cut] = ref[j][:rr, :cut]
            want = expect(u8, tables, rgb, layout)
            got = buf[int(offsets[k]): int(offsets[k]) + want.size].reshape(want.shape)
            bad = int((got != want).sum())
            n_el, n_bad = n_el + want.size, n_bad + bad
            assert bad == 0, f"batch {k} ({n} x {rows} x {Wk}, rgb {rgb}, pad {pad}): {bad} of {want.size} elements differ"
            odd_f16 += int(n > 1 and (ch * rows * Wk) % 2 == 1)
        assert odd_f16 >= 2                                      # slots at odd element offsets inside their batch
        assert int(offsets[-1]) + batches[-1][0] * ch * batches[-1][1] * batches[-1][2] == storage.numel()
    print(f"\nC={ch} {dtype} {layout}: {len(rows_of)} jobs in {len(batches)} batches x 4 (rgb, pad) launches, "
          f"{n_el} elements compared, {n_bad} differ")
    # the translation IS the source window (job 1: T(7, 3), 21 x 13 of page 0), whatever the slot
    k = next(r[1] for r in rows_of if r[0] == 1)
    s = next(r[2] for r in rows_of if r[0] == 1)
    n, rows, Wk = batches[k]
    storage, offsets = RG.warp_batches(pages, [j[0] for j in jb], wh, np.array([j[1] for j in jb]), [j[4] for j in jb], ch,
                                       [r[1] for r in rows_of], [r[2] for r in rows_of], [r[3] for r in rows_of],
                                       [b[0] for b in batches], [b[2] for b in batches], [b[1] for b in batches],
                                       torch.uint8, "nhwc")
    view = storage[int(offsets[k]): int(offsets[k]) + n * rows * Wk * ch].view(n, rows, Wk, ch)[s, :13, :21].cpu().numpy()
    assert np.array_equal(view, imgs[0][3:16, 7:28].reshape(13, 21, ch))


# ---- 2 - 5. the batch ---------------------------------------------------------------------------------------------------------

_MIX = {}


def mix():
    """The five-page mix of `test_line_regions_equal_the_single_line_calls`: two 512 x 512 tail pages (vertical 'ja' blocks,
    horizontal 'eng' blocks; `BlockList`s), a detected 256 x 256 page, an empty page, a page whose 'ja' block holds a
    degenerate line.  With its `LineRegions` (the shipped path), computed once."""
    if not _MIX:
        p, det = pkg(), TG.detector()
        TB = p.textblock
        page_a, lazy_a = TG.tail_page(1, lazy=True)
        page_b, lazy_b = TG.tail_page(2, lazy=True)
        page_c = p.synth.text_like_page((256, 256), 3, n_blocks=4)
        res_c = det(page_c)
        page_d = p.synth.text_like_page((200, 300), 4, n_blocks=2)
        odd = TB.TextBlock([20, 20, 260, 120], language="ja", font_size=21, vertical=False,
                           lines=[[[20, 20], [260, 22], [258, 58], [19, 55]], [[30, 70], [30, 70], [30, 110], [30, 110]],
                                  [[5, 150], [290, 160], [288, 195], [4, 186]]])
        eng = TB.TextBlock([20, 20, 260, 120], language="eng", font_size=21, vertical=False,
                           lines=[[[30, 70], [30, 70], [30, 110], [30, 110]], [[5, 150], [290, 160], [288, 195], [4, 186]]])
        pages = [page_a, page_b, page_c, np.full((90, 120, 3), 200, np.uint8), page_d]
        lists = [lazy_a.to_list(), lazy_b.to_list(), res_c[2], [], [odd, eng]]
        lazy = [lazy_a, lazy_b, res_c[2], [], [odd, eng]]
        regs = det.line_regions(pages, lists, TH)
        torch.cuda.synchronize()
        _MIX.update(pages=pages, lists=lists, lazy=lazy, regs=regs, padded={})
    return _MIX


def padded(width=None) -> np.ndarray:
    """`LineRegions.padded(width)` of the mix on the host, one call per width."""
    m = mix()
    if width not in m["padded"]:
        m["padded"][width] = m["regs"].padded(width).cpu().numpy()
    return m["padded"][width]


def plans_equal(a, b):
    for f in ("order", "bounds", "batch_width", "cut", "index", "valid", "widths", "offsets"):
        assert np.array_equal(getattr(a, f), getattr(b, f)), f
    assert (a.textheight, a.channels, a.dtype, a.layout, len(a)) == (b.textheight, b.channels, b.dtype, b.layout, len(b))


def batches_equal(a, b):
    plans_equal(a, b)
    for (xa, la), (xb, lb) in zip(a, b):
        assert xa.shape == xb.shape and np.array_equal(la, lb) and torch.equal(xa, xb)


def test_one_uint8_batch_is_the_padded_tensor_of_the_shipped_path():
    m = mix()
    det, regs = TG.detector(), m["regs"]
    lb = det.line_batches(m["pages"], m["lists"], textheight=TH, dtype=torch.uint8, layout="nhwc", max_batch=None, width_multiple=1)
    lb.wait()
    torch.cuda.synchronize()
    assert np.array_equal(lb.index, regs.index) and lb.index.dtype == regs.index.dtype
    assert np.array_equal(lb.valid, regs.valid) and np.array_equal(lb.widths, regs.widths) and lb.widths.dtype == regs.widths.dtype
    assert len(lb) == 1 and (lb.textheight, lb.channels, lb.dtype, lb.layout) == (TH, 3, torch.uint8, "nhwc")
    x, lines = lb[0]
    assert np.array_equal(lines, lb.order) and x.data_ptr() == lb.storage.data_ptr() and x.numel() == lb.storage.numel()
    n_invalid = int((~regs.valid).sum())
    assert n_invalid == 1 and len(lines) == len(regs) - 1 and regs.valid[lines].all()
    assert int(np.nonzero(~regs.valid)[0][0]) not in lines.tolist()          # the degenerate line is in no batch
    want = regs.padded()[torch.from_numpy(lb.order).to(x.device)]
    assert x.shape == want.shape == (len(lines), TH, int(regs.widths.max()), 3)
    assert torch.equal(x, want)
    print(f"\n{len(lines)} lines of {len(regs)}, one batch {tuple(x.shape)}: equal to padded()[order]")


@pytest.mark.parametrize("kw", [dict(), dict(width_multiple=1, dtype=torch.float32, mean=[123.675, 116.28, 103.53],
                                             std=[58.395, 57.12, 57.375], rgb=True, pad=200),
                                dict(max_width=64), dict(layout="nhwc", max_width=64, width_multiple=4, pad=255)],
                         ids=["defaults", "f32-rgb-per-channel", "max_width", "nhwc-max_width"])
def test_buckets_and_normalisation(kw):
    """max_batch = 4: every batch is table[padded(W_k)[lines]] in the asked layout, bit for bit; shapes and lines follow
    `batch_plan`; every view starts 16-byte aligned inside ONE storage."""
    m = mix()
    RG, regs = pkg().regions, m["regs"]
    lb = RG.line_batches(m["pages"], m["lists"], textheight=TH, max_batch=4, **kw)
    lb.wait()
    torch.cuda.synchronize()
    dtype, layout = kw.get("dtype", torch.float16), kw.get("layout", "nchw")
    plan = RG.batch_plan(regs.widths, regs.valid, 4, kw.get("width_multiple", 8), kw.get("max_width"))
    for f in ("order", "bounds", "batch_width", "cut"):
        assert np.array_equal(getattr(lb, f), getattr(plan, f)), f
    assert len(lb) == len(plan.batch_width) >= 8 and lb.dtype == dtype and lb.storage.dtype == dtype and lb.storage.dim() == 1
    tables = RG.value_tables(dtype, 3, kw.get("mean", 127.5), kw.get("std", 127.5))
    lo, hi = lb.storage.data_ptr(), lb.storage.data_ptr() + lb.storage.numel() * lb.storage.element_size()
    n_el = n_bad = n_pad = 0
    end = lo
    for k, (x, lines) in enumerate(lb):
        Wk = int(plan.batch_width[k])
        assert np.array_equal(lines, plan.order[plan.bounds[k]: plan.bounds[k + 1]])
        assert tuple(x.shape) == ((len(lines), 3, TH, Wk) if layout == "nchw" else (len(lines), TH, Wk, 3)) and x.is_contiguous()
        assert x.data_ptr() % 16 == 0 and end <= x.data_ptr() and x.data_ptr() + x.numel() * x.element_size() <= hi
        end = x.data_ptr() + x.numel() * x.element_size()
        u8 = padded(Wk)[lines].copy()
        if kw.get("pad", 0):                                     # padded() fills with 0: the columns right of every crop
            for s, w in enumerate(np.minimum(regs.widths[lines], Wk)):
                assert not u8[s, :, w:].any()
                u8[s, :, w:] = kw["pad"]
                n_pad += u8[s, :, w:].size
        want = expect(u8, tables, kw.get("rgb", False), layout)
        bad = int((bits(x) != want).sum())
        n_el, n_bad = n_el + want.size, n_bad + bad
        assert bad == 0, f"batch {k} {tuple(x.shape)}: {bad} of {want.size} elements differ"
    assert end == hi
    if "max_width" in kw:
        assert int(plan.batch_width.max()) == 64 and (regs.widths > 64).any()
    print(f"\n{kw}: {len(lb)} batches, widths {plan.batch_width.tolist()}, {n_el} elements compared, {n_bad} differ")


def test_entry_forms_agree():
    """Host pages and device pages, result triples and blk_lists, `TextBlock` lists and `BlockList`s, the detector's method
    and the module's function: the same tensors and the same plan.  The `BlockList` path builds no `TextBlock`s; a grey page
    gives one channel."""
    m = mix()
    p, det = pkg(), TG.detector()
    kw = dict(textheight=TH, max_batch=5)
    first = det.line_batches(m["pages"], m["lists"], **kw)
    dev_pages = [torch.from_numpy(x).cuda() for x in m["pages"]]
    for other in (det.line_batches(dev_pages, m["lists"], **kw),
                  det.line_batches(m["pages"], [(None, None, bl) for bl in m["lists"]], **kw),
                  det.line_batches(dev_pages, m["lazy"], **kw),
                  p.regions.line_batches(dev_pages, m["lazy"], **kw),
                  p.regions.line_batches(m["pages"], m["lists"], **kw)):
        torch.cuda.synchronize()
        batches_equal(other, first)
        assert torch.equal(other.storage, first.storage)         # textheight 48: no alignment gaps between the batches
    page, lazy = TG.tail_page(2, lazy=True)
    assert lazy._built is None
    a = p.regions.line_batches([page], [lazy], **kw)
    assert lazy._built is None and len(a.index) == lazy.n_lines
    b = p.regions.line_batches([page], [lazy.to_list()], **kw)
    torch.cuda.synchronize()
    batches_equal(a, b)
    grey = np.ascontiguousarray(page[:, :, 1])
    g = p.regions.line_batches([grey], [lazy], mean=0.0, std=255.0, **kw)
    c = p.regions.line_batches([page], [lazy], mean=0.0, std=255.0, **kw)
    torch.cuda.synchronize()
    assert g.channels == 1 and len(g) == len(c) > 0
    for (xg, lg), (xc, lc) in zip(g, c):
        assert tuple(xg.shape) == (len(lg), 1, TH, xc.shape[3]) and np.array_equal(lg, lc)
        assert torch.equal(xg[:, 0], xc[:, 1])


def test_nothing_to_do_and_refusals():
    p, det = pkg(), TG.detector()
    RG, L = p.regions, p._lib
    TB = p.textblock
    blank = np.full((90, 120, 3), 200, np.uint8)
    flat = TB.TextBlock([30, 70, 30, 110], language="ja", font_size=21, vertical=False,
                        lines=[[[30, 70], [30, 70], [30, 110], [30, 110]], [[40, 10], [40, 10], [40, 10], [40, 10]]])
    for lb in (RG.line_batches([], []), det.line_batches([blank], [[]]), RG.line_batches([blank], [[flat]], dtype=torch.uint8)):
        lb.wait()
        assert len(lb) == 0 and lb.storage.numel() == 0 and list(lb) == [] and len(lb.order) == 0
        assert lb.bounds.tolist() == [0] and lb.ready is not None
        with pytest.raises(IndexError):
            lb[0]
    assert len(lb.index) == 2 and not lb.valid.any() and not lb.widths.any()
    assert L.lib().ctd_warp_region_batches(None, 0, None, 0, None, None, L.REGION_F16, L.LAYOUT_NCHW, 0, 0, None) == L.OK
    assert L.lib().ctd_warp_region_batches(None, 3, None, 0, None, None, L.REGION_U8, L.LAYOUT_NHWC, 1, 255, None) == L.OK
    assert L.lib().ctd_warp_region_batches(None, 0, None, 0, None, None, 7, L.LAYOUT_NCHW, 0, 0, None) < 0
    assert L.lib().ctd_warp_region_batches(None, 0, None, 0, None, None, L.REGION_U8, L.LAYOUT_NCHW, 0, 256, None) < 0
    assert L.lib().ctd_warp_region_batches(None, 1, None, 1, None, None, L.REGION_U8, L.LAYOUT_NCHW, 0, 0, None) < 0
    assert b"null" in L.lib().ctd_last_error()
    with pytest.raises(ValueError):
        RG.line_batches([blank], [[flat]], dtype=torch.uint8, mean=0.0)
    with pytest.raises(ValueError):
        RG.line_batches([blank], [[flat]], dtype=torch.float64)
    with pytest.raises(ValueError):
        RG.line_batches([blank], [[flat]], max_width=60)
    with pytest.raises(L.CtdError):
        RG.line_batches([torch.zeros((64, 64, 3), dtype=torch.uint8)], [[flat]])
    with pytest.raises(L.CtdError):
        RG.warp_batches([torch.zeros((64, 64, 3), dtype=torch.uint8)], [0], [[4, 4]], np.eye(3)[None], [False], 3, [0], [0], [4],
                        [1], [4], 4)


# ---- 6. the stream ---------------------------------------------------------------------------------------------------------

def blocks_equal(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert [int(v) for v in x.xyxy] == [int(v) for v in y.xyxy]
        assert np.array_equal(np.asarray(x.lines), np.asarray(y.lines))
        assert (x.language, bool(x.vertical), int(x.angle), float(x.font_size)) == \
            (y.language, bool(y.vertical), int(y.angle), float(y.font_size))


@pytest.mark.parametrize("lazy", [False, True])
def test_detect_stream_yields_the_batches_of_every_work_item(lazy):
    """`detect_stream(line_batches={})`: (results, batches) per batch; `results` are the plain stream's; the work items'
    `LineBatches` hold, line for line, what `TextDetector.line_batches` gives for the item's pages; page numbers are
    batch-relative; `line_batches=None` still yields plain lists."""
    p, det = pkg(), TG.detector()
    pages = [[p.synth.text_like_page((256, 256), 3 + 2 * k + j, n_blocks=4) for j in range(2)] for k in range(3)]
    plain = list(det.detect_stream(pages, workers=2, depth=2, tail_split=2, lazy=lazy, line_batches=None))
    assert all(isinstance(r, list) and all(isinstance(x, tuple) and len(x) == 3 for x in r) for r in plain)
    got = list(det.detect_stream(pages, workers=2, depth=2, tail_split=2, lazy=lazy, line_batches={}))
    assert len(got) == len(plain) == 3
    n_lines = 0
    for batch, item, want in zip(pages, got, plain):
        assert isinstance(item, tuple) and len(item) == 2
        results, batches = item
        assert len(results) == len(want) == 2 and isinstance(batches, list) and len(batches) == 2
        for (m, r, bl), (m1, r1, bl1) in zip(results, want):
            assert np.array_equal(m, m1) and np.array_equal(r, r1)
            assert isinstance(bl, p.textblock.BlockList) == lazy
            blocks_equal(list(bl), list(bl1))
        starts = [lb.page0 for lb in batches] + [len(batch)]
        assert starts == [0, 1, 2]
        for lb, lo, hi in zip(batches, starts[:-1], starts[1:]):
            assert lb.wait() is lb
            ref = det.line_batches(batch[lo:hi], results[lo:hi])
            torch.cuda.synchronize()
            assert ((lb.index[:, 0] >= lo) & (lb.index[:, 0] < hi)).all()
            rel = lb.index.copy()
            rel[:, 0] -= lb.page0
            assert np.array_equal(rel, ref.index)
            lb.index, keep = rel, lb.index
            batches_equal(lb, ref)
            lb.index = keep
            assert (lb.dtype, lb.layout, lb.textheight) == (torch.float16, "nchw", 48)
            n_lines += len(lb.order)
    assert n_lines > 0
    # keywords pass through; records= and PageResult triples keep working
    kw = dict(textheight=32, dtype=torch.uint8, layout="nhwc", max_batch=3, width_multiple=1)
    for results, batches in det.detect_stream(pages[:1], workers=2, depth=2, tail_split=1, lazy=lazy, records=(64, 256),
                                              line_batches=kw):
        assert len(batches) == 1 and batches[0].page0 == 0 and results[0].record is not None
        ref = det.line_batches(pages[0], results, **kw)
        batches[0].wait()
        torch.cuda.synchronize()
        batches_equal(batches[0], ref)
