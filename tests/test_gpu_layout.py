"""-m gpu: layout boxes -- `ctd_layout_boxes` (csrc/kernels_layout.hip), `layout.layout_boxes` and `TextDetector.layout_boxes`
-- against the numpy restatement tests/layout_ref.py, whose rectangles come from a stack over column heights.  The rule is
integers only and its order is total, so every comparison is EXACT: every field of every row.  Most cases drive the entry
point through ctypes on hand-made bit planes and hand-made balloon rows: that is how the shapes that can go wrong are
reached."""
import ctypes as C

import numpy as np
import pytest
import torch

import balloon_ref as BR
import layout_ref as LR
import test_gpu_regions as TG
from conftest import pkg

pytestmark = pytest.mark.gpu

GUARD = 0xA5


def _tables(p, cases, gap=0):
    """The job table, the balloon rows and the bit buffer of one call.  cases: (plane or None, win, anchor in page coordinates,
    balloon status); a block's words lie `gap` guard words (0xA5...) behind the block before it.  (jobs, balloon rows, words,
    max_words)"""
    n = len(cases)
    jobs, brows = np.zeros((n,), p.layout.JOB_DTYPE), np.zeros((n,), p.balloons.ROW_DTYPE)
    words, at, max_words = [], 0, 0
    for k, (plane, win, anchor, status) in enumerate(cases):
        jobs[k]["win"], jobs[k]["ax"], jobs[k]["ay"], jobs[k]["word0"] = win, anchor[0], anchor[1], at
        brows[k]["status"] = status
        if plane is not None:
            assert plane.shape == (win[3] - win[1], win[2] - win[0])
            w = BR.pack(plane)
            words += [w, np.full((gap,), 0xA5A5A5A5A5A5A5A5, np.uint64)]
            at += len(w) + gap
            if len(w) <= BR.MAX_WORDS:
                max_words = max(max_words, len(w))
    return jobs, brows, (np.concatenate(words) if words else np.zeros((0,), np.uint64)), max_words


def _run(p, cases, inset, n_rows=None, max_words=None, lead=0):
    """One `ctd_layout_boxes` call on the current stream: (rows, kernel milliseconds by HIP events).  The row table starts
    `lead` bytes into a buffer filled with 0xA5 and has 64 guard bytes behind it; the guards and every word of the bit buffer
    are checked after the call."""
    L, Y = p._lib, p.layout
    dev = torch.device("cuda:0")
    jobs, brows, words, mw = _tables(p, cases, gap=1)
    n = len(cases)
    tab = torch.from_numpy(np.concatenate([jobs.view(np.uint8), brows.view(np.uint8)])).to(dev)
    bits = torch.from_numpy(np.concatenate([np.full((1,), 0xA5A5A5A5A5A5A5A5, np.uint64), words]).view(np.int64)).to(dev)
    out = torch.full((lead + n * 48 + 64,), GUARD, dtype=torch.uint8, device=dev)
    prm = L.CtdLayoutParams(inset, mw if max_words is None else max_words, n if n_rows is None else n_rows)
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    st = torch.cuda.current_stream(dev)
    t0.record(st)
    rc = L.lib().ctd_layout_boxes(tab.data_ptr(), n, tab.data_ptr() + n * 32, bits.data_ptr() + 8, C.byref(prm),
                                  out.data_ptr() + lead, st.cuda_stream)
    t1.record(st)
    L.check(rc, "ctd_layout_boxes")
    st.synchronize()
    host = out.cpu().numpy()
    assert (host[:lead] == GUARD).all() and (host[lead + n * 48:] == GUARD).all(), "a byte outside the row table was written"
    assert np.array_equal(bits.cpu().numpy().view(np.uint64)[1:], words), "the bit buffer was written"
    return host[lead: lead + n * 48].copy().view(Y.ROW_DTYPE), t0.elapsed_time(t1)


def _placed():
    """The material at windows of its own in page coordinates, plus one block whose index lies beyond the balloon row table."""
    cases, names = [], []
    for i, (name, plane, anchor, status) in enumerate(LR.material()):
        h, w = plane.shape
        x0, y0 = 7 * i, 3 * i
        cases.append((plane, (x0, y0, x0 + w, y0 + h), (anchor[0] + x0, anchor[1] + y0), status))
        names.append(name)
    cases.append((np.ones((9, 70), bool), (4, 4, 74, 13), (10, 8), BR.OK))
    names.append("beyond_the_row_table")
    return cases, names


_REF = {}


def _reference(inset):
    """`layout_ref.layout_row` of every block of the material, computed once per inset."""
    if inset not in _REF:
        cases, names = _placed()
        want = [LR.layout_row(plane, win, anchor, inset=inset, balloon_status=status) for plane, win, anchor, status in cases]
        want[-1] = LR._zero_row(LR.NO_REGION)
        _REF[inset] = want
    return _REF[inset]


# ---- 1. the kernel -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("inset", [0, 2, 16])
def test_kernel_equals_the_restatement_in_every_field(inset):
    """One call over the whole material (tests/layout_ref.py `material`: window widths 1 .. 1000 around the word boundaries,
    heights 1, 2 and 64, all-ones planes, runs across one, two and three words, ties, holes, noise, the anchor cases, balloon
    rows that are not OK) and one block beyond the balloon row table (n_rows = n - 1); the same call twice gives the same
    bytes."""
    p = pkg()
    cases, names = _placed()
    want = _reference(inset)
    rows, ms = _run(p, cases, inset, n_rows=len(cases) - 1)
    bad = [(nm, LR.row_dict(r), w) for nm, r, w in zip(names, rows, want) if LR.row_dict(r) != w]
    assert not bad, f"inset {inset}: {len(bad)} rows differ, first: {bad[:3]}"
    counts = [sum(w["status"] == s for w in want) for s in range(3)]
    print(f"\ninset {inset}: {len(cases)} blocks, status counts {counts}, kernel {ms * 1e3:.0f} us")
    assert counts[LR.NO_REGION] == 3 and counts[LR.OK] >= (11 if inset == 16 else 20) and (inset == 0 or counts[LR.EMPTY] >= 6)
    by = dict(zip(names, zip(cases, want)))
    for nm, ((plane, win, anchor, _), w) in by.items():
        if nm.startswith("ones_"):                          # the rectangle is the window shrunk by the inset, or nothing is left
            x1, y1, x2, y2 = win
            if x2 - x1 > 2 * inset and y2 - y1 > 2 * inset:
                assert w["rect"] == [x1 + inset, y1 + inset, x2 - inset, y2 - inset] and w["area"] == w["n_inner"], nm
            else:
                assert w == LR._zero_row(LR.EMPTY), nm
    assert by["gone_at_16"][1]["status"] == (LR.EMPTY if inset == 16 else LR.OK)
    assert (by["one_row_left_at_16"][1]["area"] == 8) == (inset == 16)
    if inset == 0:
        assert by["corridor"][1]["area"] == 4000 and by["corridor"][1]["a_area"] == 480
        assert by["ring_anchor_on_hole"][1]["a_area"] == 0 and by["ring_anchor_in"][1]["a_area"] == 35 * 50
        assert by["anchor_outside_window"][1]["a_area"] == by["anchor_below_window"][1]["a_area"] == 0
        assert by["three_whole_words"][1]["rect"][2] - by["three_whole_words"][1]["rect"][0] == 240
        assert by["single_pixel"][1]["area"] == by["single_pixel"][1]["a_area"] == 1
    again, _ = _run(p, cases, inset, n_rows=len(cases) - 1)
    assert again.tobytes() == rows.tobytes()


# ---- 2. the capacity shapes ------------------------------------------------------------------------------------------------------

def _capacity(name):
    """(plane or None, window, anchor, the row written out by hand or None) at inset 2."""
    if name == "ones_64x8192":                              # nw = 1: 8192 top rows, up to 8192 steps each
        return np.ones((8192, 64), bool), (3, 5, 67, 8197), (30, 4000), dict(
            status=LR.OK, n_inner=60 * 8188, area=60 * 8188, rect=[5, 7, 65, 8195], a_area=60 * 8188, a_rect=[5, 7, 65, 8195])
    if name == "ones_8192x64":                              # nw = 128: 64 top rows of 128 words
        return np.ones((64, 8192), bool), (3, 5, 8195, 69), (4000, 30), dict(
            status=LR.OK, n_inner=8188 * 60, area=8188 * 60, rect=[5, 7, 8193, 67], a_area=8188 * 60, a_rect=[5, 7, 8193, 67])
    if name == "band_512x1024":
        return LR.band(), (3, 5, 515, 1029), (103, 205), None
    return None, (0, 0, 64, 8193), (3, 3), LR._zero_row(LR.NO_REGION)   # 8193 words: no plane, nothing is read


@pytest.mark.parametrize("name", ["ones_64x8192", "ones_8192x64", "band_512x1024", "words_8193"])
def test_the_largest_windows_and_one_beyond(name):
    """8192 words as 64 x 8192, as 8192 x 64 and as 512 x 1024, each in a call of its own at inset 2, and a window of 8193
    words, which has no region.  The all-ones answers are written out; the band's comes from the restatement."""
    p = pkg()
    plane, win, anchor, want = _capacity(name)
    if want is None:
        want = LR.layout_row(plane, win, anchor, inset=2)
        assert want["status"] == LR.OK and 0 < want["a_area"] <= want["area"]
    _run(p, [(np.ones((1, 1), bool), (0, 0, 1, 1), (0, 0), BR.OK)], 0)           # the first launch loads the code
    rows, ms = _run(p, [(plane, win, anchor, BR.OK)], 2, max_words=BR.MAX_WORDS)
    print(f"\n{name}: kernel {ms * 1e3:.0f} us")
    assert LR.row_dict(rows[0]) == want


# ---- 3. the caller's buffers ----------------------------------------------------------------------------------------------------

def test_rows_at_an_odd_offset_and_untouched_guards():
    """The row table 4 bytes off an 8-byte boundary, 68 bytes into its buffer, the bits one word into theirs: the rows are the
    same as at offset 0, every byte around the table and every word of the bits (guard words between the blocks included) is
    as it was (`_run` checks both)."""
    p = pkg()
    cases, names = _placed()
    want = _reference(2)
    rows, _ = _run(p, cases, 2, n_rows=len(cases) - 1, lead=68)
    assert [LR.row_dict(r) for r in rows] == want
    # a block larger than the call's max_words is refused, not computed
    rows, _ = _run(p, cases, 2, n_rows=len(cases) - 1, max_words=16, lead=4)
    for nm, r, w, (plane, win, _, status) in zip(names, rows, want, cases):
        small = BR.n_words(win)[1] <= 16
        assert LR.row_dict(r) == (w if small else LR._zero_row(LR.NO_REGION)), nm


# ---- 4. behind the balloon launch ---------------------------------------------------------------------------------------------

class _Blk:
    def __init__(self, xyxy):
        self.xyxy = list(xyxy)


def _chambers():
    """[(page, mask, boxes)]: a closed room, a room with a gap in its outline on a page of its own colour, two rooms."""
    out = []
    page, mask, box = BR.chamber_page()
    out.append((page, mask, [box]))
    page, mask, box = BR.chamber_page(bg=255, gap=(20, 30))
    out.append((page, mask, [box]))
    page, mask, box = BR.chamber_page(shape=(60, 200))
    page2, mask2, box2 = BR.chamber_page(shape=(60, 200), room=(110, 5, 190, 55), text=(130, 26, 160, 32))
    page[:, 100:], mask[:, 100:] = page2[:, 100:], mask2[:, 100:]
    out.append((page, mask, [box, box2]))
    return out


def _restate(material, ref, anchors, inset):
    """`layout_ref.layout_row` on the planes of `balloon_ref.balloon_page` results."""
    want, k = [], 0
    for (page, mask, boxes), (rows, words, wins, _) in zip(material, ref):
        for row, w, win in zip(rows, words, wins):
            plane = None if w is None else BR.unpack(w, win[3] - win[1], win[2] - win[0])
            want.append(LR.layout_row(plane, win, anchors[k], inset=inset, balloon_status=row["status"]))
            k += 1
    return want


def test_layout_boxes_behind_balloon_regions():
    p = pkg()
    B, Y = p.balloons, p.layout
    material = _chambers()
    ref = [BR.balloon_page(*m) for m in material]
    lists = [[_Blk(b) for b in m[2]] for m in material]
    br = B.balloon_regions([m[0] for m in material], [m[1] for m in material], lists)
    before = br.bits.view(torch.int64).clone()
    centers = [[r["sum_x"] // r["area"], r["sum_y"] // r["area"]] if r["status"] == BR.OK else [-1, -1] for rf in ref for r in rf[0]]
    assert br.center.tolist() == centers and br.ok.all() and len(br) == 4
    for inset in (2, 0, 5):
        lb = Y.layout_boxes(br, inset=inset)
        assert [LR.row_dict(r) for r in lb.rows] == _restate(material, ref, centers, inset), inset
        assert lb.inset == inset and np.array_equal(lb.index, br.index) and lb.anchors.tolist() == centers
    lb = Y.layout_boxes(br)
    # the closed room: 60 x 40 with a 1-pixel outline, so the region is its 58 x 38 interior, and the box is that shrunk by 2
    assert lb.rect[0].tolist() == lb.a_rect[0].tolist() == [23, 13, 77, 47] and lb.area[0] == lb.n_inner[0] == 54 * 34
    assert lb.ok.all() and lb.status.tolist() == [LR.OK] * 4 and repr(lb) == "LayoutBoxes(4 blocks, 4 ok, inset 2)"
    # the leaked region holds far more than the room (the balloon row's flags say so); the room is still its largest rectangle
    assert br.flags[1] == 0xA5 and lb.n_inner[1] == 3500 and lb.rect[1].tolist() == [23, 13, 77, 47]
    assert lb.rect[3].tolist() == [113, 8, 187, 52]
    # anchors of the caller's: one in the margin, one outside every window
    own = np.array([[22, 30], [50, 30], [-7, -7], [150, 30]])
    lb = Y.layout_boxes(br, own, inset=2, stream=torch.cuda.Stream())
    assert [LR.row_dict(r) for r in lb.rows] == _restate(material, ref, own.tolist(), 2)
    assert lb.a_area[0] == 0 and lb.a_area[2] == 0 and lb.a_area[3] > 0
    assert torch.equal(br.bits.view(torch.int64), before)


# ---- 5. through the detector ---------------------------------------------------------------------------------------------------

def test_detector_layout_boxes_equals_the_restatement():
    """`det.layout_boxes(pages, det.detect_batch(pages))` against the restatement fed with the same regions and the centres of
    the blocks' boxes; the same with `regions=` passed in."""
    p, det = pkg(), TG.detector()
    pages = [p.synth.text_like_page((256, 256), 3, n_blocks=4), p.synth.text_like_page((200, 300), 4, n_blocks=2)]
    results = det.detect_batch(pages)
    boxes = [[[int(v) for v in b.xyxy] for b in r[2]] for r in results]
    assert sum(len(b) for b in boxes) >= 3
    anchors = [[(max(x1, 0) + min(x2, pg.shape[1])) >> 1, (max(y1, 0) + min(y2, pg.shape[0])) >> 1]
               for pg, bx in zip(pages, boxes) for x1, y1, x2, y2 in bx]
    br = det.balloons(pages, results)
    rows, bits = br.to_host()
    want = []
    for k in range(len(br)):
        win = tuple(int(v) for v in br.windows[k])
        plane = None
        if not br.too_large[k]:
            w0, nwords = int(br.word0[k]), int(br.nw[k]) * (win[3] - win[1])
            plane = BR.unpack(bits[w0: w0 + nwords], win[3] - win[1], win[2] - win[0])
        want.append(LR.layout_row(plane, win, anchors[k], inset=2, balloon_status=int(rows["status"][k])))
    lb = det.layout_boxes(pages, results)
    assert [LR.row_dict(r) for r in lb.rows] == want and lb.anchors.tolist() == anchors
    print(f"\nstatuses {lb.status.tolist()}, areas {lb.area.tolist()}, anchored {lb.a_area.tolist()}")
    assert lb.ok.sum() >= 1
    other = det.layout_boxes(pages, results, regions=br)
    assert other.rows.tobytes() == lb.rows.tobytes() and np.array_equal(other.index, lb.index)
    wide = det.layout_boxes([torch.from_numpy(x).cuda() for x in pages], results, inset=0, reach=4)
    assert (wide.n_inner[wide.ok] >= wide.area[wide.ok]).all() and len(wide) == len(lb)
    with pytest.raises(ValueError):
        det.layout_boxes(pages, results, inset=17)
    if len(boxes[1]):                                       # regions of two pages, blocks of one
        with pytest.raises(ValueError):
            det.layout_boxes(pages[:1], results[:1], regions=br)


# ---- 6. bad arguments --------------------------------------------------------------------------------------------------------

def test_bad_arguments_are_refused_without_a_launch():
    p = pkg()
    B, Y, L = p.balloons, p.layout, p._lib
    page, mask, box = BR.chamber_page()
    br = B.balloon_regions([page], [mask], [[_Blk(box)]])
    for bad in (-1, 17, 2.5, True):
        with pytest.raises(ValueError):
            Y.layout_boxes(br, inset=bad)
    for anchors in (np.zeros((2,), np.int64), np.zeros((2, 2), np.int64), np.zeros((1, 3), np.int64), np.zeros((1, 2), np.float32),
                    np.zeros((1, 2), bool), np.full((1, 2), -2 ** 31 - 1), [50, 30]):
        with pytest.raises(ValueError):
            Y.layout_boxes(br, anchors)
    assert Y.layout_boxes(br, [[50, 30]]).a_area.tolist() == [54 * 34]
    none = Y.layout_boxes(B.balloon_regions([page], [mask], [[]]))              # a page without blocks: nothing launched
    assert len(none) == 0
    lib = L.lib()
    prm = L.CtdLayoutParams(2, 8, 1)
    assert lib.ctd_layout_boxes(8, 1, 8, None, C.byref(prm), 8, None) != L.OK                  # words to read and no buffer
    assert lib.ctd_layout_boxes(8, 1, None, 8, C.byref(prm), 8, None) != L.OK
    assert lib.ctd_layout_boxes(8, 1, 8, 8, C.byref(L.CtdLayoutParams(17, 8, 1)), 8, None) != L.OK
    torch.cuda.synchronize()
