"""-m gpu: the forms of input that the shared call layer (`pagecall.PageCall`) handles for every page call -- host arrays,
dense device tensors, device views with a row pitch beyond the row, device views that are not dense and must be made
contiguous -- each on the current stream and on a side stream, through `line_colors`, `erase_text`, `balloon_regions`,
`fill_rest`, `typeset_pages(inplace=False)` and `line_regions`.  Expected values are the numpy restatements that each
module's own GPU test compares against (color_ref, erase_ref, balloon_ref, fill_ref, typeset_ref, region_ref), as exactly
as those tests compare: every field and every byte, and for the warp every pixel outside the restatement's tie band, one of
its candidates inside.  Nothing here is compared with another run of the code under test."""
import numpy as np
import pytest
import torch

import balloon_ref as BR
import color_ref as CR
import erase_ref as ER
import fill_ref as FR
import region_ref as RR
import test_gpu_balloons as TGB
import test_gpu_colors as TGC
import test_gpu_fill as TGF
import test_gpu_typeset as TGT
import typeset_ref as TR
from conftest import pkg

pytestmark = pytest.mark.gpu

TH = 24
FORMS = ("host", "dense", "pitched", "strided")
SYNC_CALLS = ("line_colors", "erase_text", "balloon_regions", "fill_rest", "typeset_pages")
CALLS = SYNC_CALLS + ("line_regions",)
_M = {}


def _quad(x1, y1, x2, y2):
    return [[x1, y1], [x2, y1], [x2, y2], [x1, y2]]


def material():
    """Two pages of different sizes, 48 x 72 and 40 x 150 (a row of the second spans three 64-bit words), three blocks with
    their text mask and one line each: a bar in a white room; a bar that crosses the word seams at x = 64 and 128 in a room on
    noise; a bar in a room that the page's right edge cuts, whose box and line reach beyond the page.  Plus three typeset
    layers in the same places.  Built once; nothing writes to it."""
    if "m" not in _M:
        TB = pkg().textblock.TextBlock
        rng = np.random.default_rng(7)
        p0, m0 = np.full((48, 72, 3), (200, 190, 180), np.uint8), np.zeros((48, 72), np.uint8)
        TGB._room(p0, m0, 4, 4, 68, 44, (16, 20, 56, 26))
        p1, m1 = rng.integers(0, 256, (40, 150, 3), dtype=np.uint8), np.zeros((40, 150), np.uint8)
        TGB._room(p1, m1, 6, 4, 135, 36, (20, 16, 131, 22))
        TGB._room(p1, m1, 137, 8, 150, 32, (140, 16, 150, 22))
        lists = [[TB([12, 16, 60, 30], lines=[_quad(16, 20, 56, 26)], language="eng", font_size=6)],
                 [TB([16, 12, 134, 26], lines=[_quad(20, 16, 131, 22)], language="ja", font_size=6),
                  TB([138, 12, 170, 28], lines=[_quad(140, 16, 162, 22)], language="eng", font_size=6)]]
        layers = [TR.layer(0, TR.glyph(12, 20, 1), 10, 10, 2, (3, 2, 1), (0, 128, 250)),
                  TR.layer(1, TR.glyph(14, 90, 2), 50, 12, 3, (250, 250, 250), (5, 5, 5)),
                  TR.layer(1, TR.noise(10, 30, 3), 135, 20, 1, (0, 0, 0), (255, 255, 255))]
        _M["m"] = ([p0, p1], [m0, m1], lists, layers)
    return _M["m"]


def reference(name):
    """The restatement's answer for call `name` on the material: computed once, shared, never changed."""
    if name not in _M:
        pages, masks, lists, layers = material()
        boxes = [[tuple(b.xyxy) for b in blks] for blks in lists]
        if name == "line_colors":
            _M[name] = TGC._reference(pages, masks, lists)
        elif name == "erase_text":
            _M[name] = [ER.erase_page(pg, mk, bx) for pg, mk, bx in zip(pages, masks, boxes)]
        elif name == "balloon_regions":
            _M[name] = [BR.balloon_page(pg, mk, bx) for pg, mk, bx in zip(pages, masks, boxes)]
        elif name == "fill_rest":
            _M[name] = [FR.fill_vec(pg, mk) for pg, mk in zip(pages, masks)]
        elif name == "typeset_pages":
            _M[name] = TR.typeset(pages, layers)
        else:
            _M[name] = [[RR.get_transformed_region(pg, ln, b.language, b.vertical, b.font_size, TH) for b in blks for ln in b.lines]
                        for pg, blks in zip(pages, lists)]
    return _M[name]


def as_form(arrs, form, dev):
    """The arrays in one of the four forms the layer takes."""
    if form == "host":
        return list(arrs)
    out = []
    for a in arrs:
        t = torch.from_numpy(a).to(dev)
        H, W, c = t.shape[0], t.shape[1], (t.shape[2] if t.dim() == 3 else 1)
        if form == "pitched":                                # rows are slices of a wider buffer: dense, read through the pitch
            wide = torch.full((H, W + 29) + tuple(t.shape[2:]), 77, dtype=torch.uint8, device=dev)
            wide[:, 13:13 + W] = t
            t = wide[:, 13:13 + W]
            assert t.stride(0) == (W + 29) * c and t.stride(1) == c and not t.is_contiguous()
        elif form == "strided":                              # every second column of a buffer twice as wide: not dense
            wide = torch.full((H, 2 * W) + tuple(t.shape[2:]), 77, dtype=torch.uint8, device=dev)
            wide[:, ::2] = t
            t = wide[:, ::2]
            assert t.stride(1) == 2 * c and not t.is_contiguous()
        out.append(t)
    return out


def run(name, pages, masks, stream):
    p = pkg()
    _, _, lists, layers = material()
    if name == "line_colors":
        return p.colors.line_colors(pages, masks, lists, stream=stream)
    if name == "erase_text":
        return p.erase.erase_text(pages, masks, lists, stream=stream)
    if name == "balloon_regions":
        return p.balloons.balloon_regions(pages, masks, lists, stream=stream)
    if name == "fill_rest":
        return p.fill.fill_rest(pages, masks, stream=stream)
    if name == "typeset_pages":
        return TGT._api(p, pages, layers, inplace=False, stream=stream)
    return p.regions.line_regions(pages, lists, textheight=TH, stream=stream)


def check(name, got):
    pages, masks, lists, layers = material()
    want = reference(name)
    boxes = [[tuple(b.xyxy) for b in blks] for blks in lists]
    if name == "line_colors":
        index, rows = want
        assert got.index.tolist() == [list(i) for i in index] and got.rows.dtype == pkg().colors.OUT_DTYPE
        TGC._compare(got.rows, rows, lambda i: index[i])
        assert {r["status"] for r in rows} == {CR.OK}
    elif name == "erase_text":
        assert [ER.row_dict(r) for r in got.rows] == [r for rows, _, _ in want for r in rows] and not got.rows["pad_"].any()
        assert got.index.tolist() == [[0, 0], [1, 0], [1, 1]]
        for i, (_, out, rest) in enumerate(want):
            assert np.array_equal(got.pages[i].cpu().numpy(), out) and np.array_equal(got.rest[i].cpu().numpy(), rest), i
            assert got.pages[i].is_contiguous() and got.rest[i].is_contiguous()
        assert got.plain.any() and (want[0][1] != pages[0]).any()
    elif name == "balloon_regions":
        TGB._compare(got, [(pg, mk, bx) for pg, mk, bx in zip(pages, masks, boxes)], want)
        assert got.ok.any()
    elif name == "fill_rest":
        TGF._compare(got, pages, masks, want)
        assert (got.status == pkg()._lib.FILL_OK).all()
    elif name == "typeset_pages":
        assert not TGT._same(got.to_host(), want[0]), "typeset pages differ"
        assert np.array_equal(np.stack([got.n_fill, got.n_stroke], axis=1), want[1]) and want[1].all()
    else:
        host, k = got.to_host(), 0
        assert got.channels == 3 and got.valid.all() and len(got) == 3
        for pg, lines in enumerate(want):
            for ref, band, cands in lines:
                crop = host[k]
                assert crop.shape == ref.shape and crop.shape[0] == TH and got.index[k, 0] == pg
                assert not ((crop != ref) & ~band[:, :, None]).any(), f"line {k}: a pixel outside the tie band differs"
                one_of = np.zeros(band.shape, bool)
                for c in cands:
                    one_of |= (crop == c).all(axis=2)
                assert not (~one_of & band).any(), f"line {k}: a tie-band pixel is none of the candidates"
                assert band.mean() <= 0.02
                k += 1


def test_the_material_is_what_the_cases_need():
    pages, masks, lists, layers = material()
    assert [pg.shape for pg in pages] == [(48, 72, 3), (40, 150, 3)] and pages[1].shape[1] > 128
    assert sum(len(b) for b in lists) == 3 and all(m.any() for m in masks)
    x1, _, x2, _ = lists[1][1].xyxy
    assert x1 < pages[1].shape[1] < x2                       # the block that straddles the page's edge


@pytest.mark.parametrize("side", (False, True), ids=("current", "side"))
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", CALLS)
def test_every_input_form_on_either_stream_equals_the_restatement(name, form, side):
    dev = torch.device("cuda:0")
    pages, masks = material()[:2]
    pages, masks = as_form(pages, form, dev), as_form(masks, form, dev)
    stream = None
    if side:
        stream = torch.cuda.Stream(dev)
        stream.wait_stream(torch.cuda.current_stream(dev))   # the inputs were written on the current stream
    got = run(name, pages, masks, stream)
    if side:
        stream.synchronize()                                  # `line_regions` returns without waiting
    check(name, got)


@pytest.mark.parametrize("name", SYNC_CALLS)
def test_inputs_may_be_dropped_and_their_memory_reused_once_a_call_has_returned(name):
    """The observable form of the layer's lifetime rule, ordinary valid use: a call that waits has finished with its
    inputs -- and with the contiguous copies, the tables and the rows buffer it made of them on the side stream -- when it
    returns.  The caller drops the inputs, fresh allocations of the same sizes are overwritten on the default stream, and
    the result still equals the restatement."""
    dev = torch.device("cuda:0")
    pages, masks = material()[:2]
    pages, masks = as_form(pages, "strided", dev), as_form(masks, "strided", dev)
    sizes = [t._base.numel() if t._base is not None else t.numel() for t in pages + masks] + [t.numel() for t in pages + masks]
    stream = torch.cuda.Stream(dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    got = run(name, pages, masks, stream)
    del pages, masks
    fresh = [torch.full((n,), 0xA5, dtype=torch.uint8, device=dev) for n in sizes]
    torch.cuda.current_stream(dev).synchronize()
    assert all(bool((f == 0xA5).all()) for f in fresh)
    check(name, got)
