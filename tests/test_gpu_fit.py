"""-m gpu: the shaped fit -- `ctd_layout_fit` (csrc/kernels_fit.hip), `layout.shaped_fit`, `glyphs.place_lines` and
`TextDetector.typeset_text(shaped=)` -- against the numpy restatement tests/fit_ref.py, which finds axis runs from the
positions of a row's zeros and breaks lines glyph by glyph.  The rule is integers only, so every comparison is EXACT: every
field of every row, every line record.  Most cases drive the entry point through ctypes on hand-made bit planes, hand-made
balloon rows and raw tables, in the manner of tests/test_gpu_layout.py: that is how the shapes that can go wrong are reached."""
import ctypes as C

import numpy as np
import pytest
import torch

import balloon_ref as BR
import fit_ref as FR
import glyph_ref as GR
import layout_ref as LR
import raster_ref as RR
import test_gpu_layout as TL
import test_gpu_raster as TRS
import test_gpu_regions as TG
from conftest import pkg

pytestmark = pytest.mark.gpu

GUARD = 0xA5
ROW = 656


def _text(G, sizes, seed, zero=False):
    """(cums, lines, gaps of 0): a run of G glyphs at `sizes`, advances about half a size (some 0 with `zero`)."""
    rng = np.random.default_rng(seed)
    base = rng.integers(0 if zero else 1, 7, G)
    return [np.concatenate([[0], np.cumsum(base * s // 6)]).astype(np.int64) for s in sizes], [s + 1 for s in sizes], [0] * len(sizes)


def case(plane, win, anchor, text, status=BR.OK, breaks=None, gap=None):
    cums, lines, gaps = text
    return dict(plane=plane, win=tuple(win), anchor=tuple(anchor), status=status, cums=cums, lines=list(lines),
                gaps=list(gaps) if gap is None else [gap] * len(lines), breaks=breaks)


def _ones(h, w, ax, ay, text, x0=0, y0=0, **kw):
    return case(np.ones((h, w), bool), (x0, y0, x0 + w, y0 + h), (x0 + ax, y0 + ay), text, **kw)


def _cases():
    """[(name, case)]: the layout material with text, then the shapes the fit can go wrong at."""
    out = []
    for i, (name, plane, anchor, status) in enumerate(LR.material()):
        h, w = plane.shape
        x0, y0 = 7 * i, 3 * i
        G = 40 if i % 4 else 9
        brk = (None, np.arange(G) % 2 == 1, np.zeros((G,), bool))[i % 3]       # no table, every second break, no break allowed
        out.append((name, case(plane, (x0, y0, x0 + w, y0 + h), (anchor[0] + x0, anchor[1] + y0), _text(G, (3, 5, 8, 12), i),
                               status=status, breaks=brk, gap=(0, 3)[i % 2])))
    small = _text(12, (2, 4), 50)
    zeros = ([np.zeros((6,), np.int64)], [3], [0])
    # window widths around the word boundary, the anchor on the first and last column of a word and of the window
    for w in (1, 63, 64, 65, 130):
        for ax in sorted({0, min(63, w - 1), min(64, w - 1), w - 1, w // 2}):
            out.append((f"w{w}_ax{ax}", _ones(40, w, ax, 20, small, x0=3, y0=5)))
            out.append((f"w{w}_ax{ax}_zero_advances", _ones(40, w, ax, 20, zeros, x0=3, y0=5)))
    out.append(("one_row_high", _ones(1, 65, 32, 0, ([np.arange(5) * 3, np.arange(5) * 20], [1, 1], [0, 0]))))
    out.append(("one_row_high_line_2", _ones(1, 65, 32, 0, ([np.arange(5) * 3], [2], [0]))))
    tall = np.zeros((2048, 64), bool)
    tall[5:2040, 3:61] = FR.ellipse(2035, 58)
    out.append(("tall_64x2048", case(tall, (9, 1, 73, 2049), (9 + 32, 1 + 1000), _text(200, (4, 9, 14, 30), 51), gap=3)))
    out.append(("tall_64x2048_off_axis", case(tall, (9, 1, 73, 2049), (9 + 20, 1 + 300), _text(60, (2, 4, 9), 52))))
    # the stack against the window's top and bottom: only the low candidate stays inside, and only with one line
    one_line = ([np.arange(4) * 3, np.arange(4) * 3], [3, 6], [0, 0])
    out.append(("stack_at_the_top", _ones(30, 40, 20, 2, one_line)))
    out.append(("stack_at_the_bottom", _ones(30, 40, 20, 28, one_line)))
    out.append(("stack_past_the_top", _ones(30, 40, 20, 2, ([np.arange(30) * 3], [3], [0]))))
    out.append(("stack_past_the_bottom", _ones(30, 40, 20, 28, ([np.arange(30) * 3], [3], [0]))))
    # runs: none, one glyph, a glyph wider than every slot
    out.append(("no_glyph", _ones(80, 200, 100, 40, ([np.zeros((1,), np.int64)] * 2, [3, 4], [0, 0]))))
    out.append(("no_candidate", _ones(80, 200, 100, 40, ([], [], []))))
    out.append(("one_glyph", _ones(80, 200, 100, 40, ([np.array([0, 5]), np.array([0, 9])], [5, 9], [1, 1]))))
    out.append(("glyph_wider_than_every_slot", _ones(80, 200, 100, 40, ([np.array([0, 3, 500, 503])], [4], [0]))))
    # 32 lines and 33: slots of 20 (inset 0), two glyphs of 10 a line, lines of 3 in 200 rows
    out.append(("needs_32_lines", _ones(200, 21, 10, 100, ([np.arange(65) * 10], [3], [0]))))
    out.append(("needs_33_lines", _ones(200, 21, 10, 100, ([np.arange(67) * 10], [3], [0]))))
    out.append(("needs_32_lines_gap_3", _ones(200, 21, 10, 100, ([np.arange(65) * 10], [3], [3]))))
    # candidates: one; sixteen of which the middle ones' lines are taller than the window and the last one is small again
    out.append(("one_candidate", _ones(60, 90, 45, 30, _text(30, (5,), 53))))
    c16, l16, g16 = _text(30, tuple(range(3, 19)), 54)
    for c in range(6, 15):
        l16[c] = 61 + c
    c16[15] = c16[2]
    l16[15] = l16[2]
    out.append(("sixteen_candidates_not_monotone", _ones(60, 90, 45, 30, (c16, l16, g16))))
    out.append(("sixteen_candidates_gap_3", _ones(60, 90, 45, 30, _text(30, tuple(range(3, 19)), 55), gap=3)))
    # break tables on an ellipse
    e = FR.ellipse(70, 110)
    for nm, brk in (("no_break_allowed", np.zeros((40,), bool)), ("every_second_break", np.arange(40) % 2 == 1),
                    ("words", np.arange(40) % 5 == 4)):
        out.append((f"ellipse_{nm}", case(e, (11, 13, 121, 83), (11 + 55, 13 + 35), _text(40, (3, 5, 8, 12), 56), breaks=brk)))
    out.append(("ellipse_off_centre", case(e, (11, 13, 121, 83), (11 + 30, 13 + 25), _text(40, (3, 5, 8, 12), 57, zero=True), gap=3)))
    out.append(("beyond_the_row_table", _ones(9, 70, 6, 4, small, x0=4, y0=4)))
    return out


def _upload(p, cases, lead=0):
    """The device tables of one call: the layout jobs, the fit jobs, the balloon rows, candidates, advances, breaks in one
    buffer, the bits (a guard word in front, one behind every block) in another, the rows `lead` bytes into a third."""
    Y = p.layout
    n = len(cases)
    jobs, brows = np.zeros((n,), Y.JOB_DTYPE), np.zeros((n,), p.balloons.ROW_DTYPE)
    words, at, max_words = [np.full((1,), 0xA5A5A5A5A5A5A5A5, np.uint64)], 0, 0
    for k, c in enumerate(cases):
        jobs[k]["win"], jobs[k]["ax"], jobs[k]["ay"], jobs[k]["word0"] = c["win"], c["anchor"][0], c["anchor"][1], at
        brows[k]["status"] = c["status"]
        assert c["plane"].shape == (c["win"][3] - c["win"][1], c["win"][2] - c["win"][0])
        w = BR.pack(c["plane"])
        words += [w, np.full((1,), 0xA5A5A5A5A5A5A5A5, np.uint64)]
        at += len(w) + 1
        max_words = max(max_words, len(w))
    cum = [np.stack(c["cums"]) if c["cums"] else None for c in cases]
    fjobs, cands, flat, brk = Y.fit_tables(cum, [c["lines"] for c in cases], [c["gaps"] for c in cases],
                                           breaks=[c["breaks"] for c in cases])
    blob, offs = p.pagecall.pack([jobs, fjobs, brows, cands, flat, brk])
    dev = torch.device("cuda:0")
    tab = torch.from_numpy(blob).to(dev)
    words = np.concatenate(words)
    bits = torch.from_numpy(words.view(np.int64)).to(dev)
    out = torch.full((lead + n * ROW + 64,), GUARD, dtype=torch.uint8, device=dev)
    ptr = [tab.data_ptr() + o for o in offs[:-1]]
    counts = (len(cands), len(flat), len(brk))
    return tab, bits, words, out, ptr, counts, max_words


def _run(p, cases, inset, n_rows=None, lead=0):
    """One `ctd_layout_fit` call on the current stream: the rows.  The guards around the row table and every word of the bit
    buffer are checked after the call."""
    L, Y = p._lib, p.layout
    n = len(cases)
    tab, bits, words, out, ptr, (nc, ncum, nbrk), mw = _upload(p, cases, lead)
    prm = L.CtdFitParams(inset, mw, n if n_rows is None else n_rows, nc, ncum, nbrk)
    st = torch.cuda.current_stream()
    L.check(L.lib().ctd_layout_fit(ptr[0], ptr[1], n, ptr[2], bits.data_ptr() + 8, ptr[3] if nc else None, ptr[4] if ncum else None,
                                   ptr[5] if nbrk else None, C.byref(prm), out.data_ptr() + lead, st.cuda_stream), "ctd_layout_fit")
    st.synchronize()
    host = out.cpu().numpy()
    assert (host[:lead] == GUARD).all() and (host[lead + n * ROW:] == GUARD).all(), "a byte outside the row table was written"
    assert np.array_equal(bits.cpu().numpy().view(np.uint64), words), "the bit buffer was written"
    return host[lead: lead + n * ROW].copy().view(Y.FIT_ROW_DTYPE)


def _want(c, inset):
    return FR.fit_row(c["plane"], c["win"], c["anchor"], c["cums"], c["lines"], c["gaps"], breaks=c["breaks"], inset=inset,
                      balloon_status=c["status"])


_REF = {}


def _reference(inset):
    """`fit_ref.fit_row` of every case, computed once per inset; the last block lies beyond the balloon row table."""
    if inset not in _REF:
        want = [_want(c, inset) for _, c in _cases()]
        want[-1] = FR._zero_row(FR.NO_REGION)
        _REF[inset] = want
    return _REF[inset]


# ---- 1. the kernel -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("inset", [0, 2, 16])
def test_kernel_equals_the_restatement_in_every_field(inset):
    """One call over all cases (`_cases`: every shape of the layout material with a run of 9 or 40 glyphs at four sizes, with no
    break table, every second break and no break allowed, gaps 0 and 3; windows 1, 63, 64, 65 and 130 wide with the anchor on
    columns 0, 63, 64 and the last; a window one row high; a 64 x 2048 window; stacks at and past the window's top and bottom;
    runs of 0 and 1 glyphs and a glyph wider than every slot; 32 lines and 33; 1 and 16 candidates, not monotone; advances of
    0) and one block beyond the balloon row table.  Every status occurs under the restatement alone, at every inset."""
    p = pkg()
    names, cases = [nm for nm, _ in _cases()], [c for _, c in _cases()]
    want = _reference(inset)
    counts = [sum(w["status"] == s for w in want) for s in range(5)]
    assert all(counts), f"inset {inset}: a status does not occur under the restatement: {counts}"
    rows = _run(p, cases, inset, n_rows=len(cases) - 1)
    bad = [(nm, FR.row_dict(r), w) for nm, r, w in zip(names, rows, want) if FR.row_dict(r) != w]
    assert not bad, f"inset {inset}: {len(bad)} of {len(rows)} rows differ, first: {bad[0]}"
    print(f"\ninset {inset}: {len(cases)} blocks, status counts {counts}")
    by = dict(zip(names, want))
    if inset == 0:
        assert (by["needs_32_lines"]["status"], by["needs_32_lines"]["n_lines"]) == (FR.OK, 32)
        assert (by["needs_32_lines_gap_3"]["status"], by["needs_32_lines_gap_3"]["n_lines"]) == (FR.OK, 32)
        assert by["needs_33_lines"]["status"] == FR.NO_FIT and by["glyph_wider_than_every_slot"]["status"] == FR.NO_FIT
        assert by["no_glyph"]["status"] == by["no_candidate"]["status"] == FR.NO_TEXT
        assert (by["one_glyph"]["cand"], by["one_glyph"]["n_lines"]) == (1, 1)
        assert by["sixteen_candidates_not_monotone"]["cand"] == 15 and by["one_candidate"]["status"] == FR.OK
        assert (by["stack_at_the_top"]["cand"], by["stack_at_the_top"]["n_lines"]) == (0, 1)
        assert (by["stack_at_the_bottom"]["cand"], by["stack_at_the_bottom"]["n_lines"]) == (0, 1)
        assert by["stack_past_the_top"]["status"] == by["stack_past_the_bottom"]["status"] == FR.NO_FIT
        assert by["w65_ax0_zero_advances"]["lines"][0] == [0, 3, 5 + 20 - 1, 0, 0] and by["w65_ax0"]["status"] == FR.NO_FIT
        assert by["w130_ax64"]["lines"][0][3] == 128 and by["w1_ax0"]["status"] == FR.NO_FIT
        assert all((by[k]["n_lines"], by[k]["lines"][0][3]) == (6, 2) for k in ("w65_ax64", "w64_ax63"))   # half = 1 at the last column
        assert by["w130_ax65"]["lines"][0][3] == 130 and by["one_row_high"]["cand"] == 0 and by["one_row_high_line_2"]["status"] == FR.NO_FIT
        assert by["tall_64x2048"]["status"] == by["tall_64x2048_off_axis"]["status"] == FR.OK and by["tall_64x2048"]["n_lines"] > 8
        assert by["ring_anchor_on_hole"]["status"] == by["anchor_outside_window"]["status"] == FR.NO_ANCHOR
        assert by["not_plain"]["status"] == by["too_large"]["status"] == by["beyond_the_row_table"]["status"] == FR.NO_REGION
    again = _run(p, cases, inset, n_rows=len(cases) - 1)
    assert again.tobytes() == rows.tobytes()


def test_rows_at_an_odd_offset_and_untouched_guards():
    """The row table 4 bytes off an 8-byte boundary, 68 bytes into its buffer, the bits one word into theirs with a guard word
    behind every block: the rows are the same, every byte around the table and every word of the bits is as it was (`_run`
    checks both)."""
    p = pkg()
    cases = [c for _, c in _cases()]
    rows = _run(p, cases, 2, n_rows=len(cases) - 1, lead=68)
    assert [FR.row_dict(r) for r in rows] == _reference(2)


# ---- 2. bad arguments ---------------------------------------------------------------------------------------------------------

def test_bad_arguments_are_refused_without_a_launch():
    """Every refusal of the entry point's: the row buffer keeps its guard bytes, so nothing was launched."""
    p = pkg()
    L, Y = p._lib, p.layout
    lib = L.lib()
    good = [_ones(40, 65, 32, 20, _text(12, (2, 4), 50), breaks=np.arange(12) % 2 == 1), _ones(9, 70, 6, 4, _text(5, (2, 4, 6), 1))]
    tab, bits, words, out, ptr, (nc, ncum, nbrk), mw = _upload(p, good)
    st = torch.cuda.current_stream()
    host = tab.cpu().numpy()
    base = tab.data_ptr()

    def call(prm=None, n=2, edit=None, **null):
        """rc of a call with one thing wrong: a parameter, a null table, or a field of a device table."""
        t, q = tab, list(ptr)
        if edit is not None:
            which, k, field, value = edit
            h = host.copy()
            off, dt = (ptr[1] - base, Y.FIT_JOB_DTYPE) if which == "job" else (ptr[3] - base, Y.FIT_CAND_DTYPE)
            h[off:].view(np.uint8)[: dt.itemsize * (k + 1)].view(dt)[k][field] = value
            t = torch.from_numpy(h).cuda()
            q = [t.data_ptr() + (x - base) for x in ptr]
        a = dict(jobs=q[0], fjobs=q[1], brows=q[2], bits=bits.data_ptr() + 8, cands=q[3], cum=q[4], brk=q[5], rows=out.data_ptr())
        a.update(null)
        prm = L.CtdFitParams(2, mw, 2, nc, ncum, nbrk) if prm is None else prm
        rc = lib.ctd_layout_fit(a["jobs"], a["fjobs"], n, a["brows"], a["bits"], a["cands"], a["cum"], a["brk"], C.byref(prm),
                                a["rows"], st.cuda_stream)
        st.synchronize()
        return rc

    bad = [call(n=-1), call(L.CtdFitParams(17, mw, 2, nc, ncum, nbrk)), call(L.CtdFitParams(-1, mw, 2, nc, ncum, nbrk)),
           call(L.CtdFitParams(2, 8193, 2, nc, ncum, nbrk)), call(L.CtdFitParams(2, mw, -1, nc, ncum, nbrk)),
           call(L.CtdFitParams(2, mw, 2, -1, ncum, nbrk)), call(L.CtdFitParams(2, mw, 2, nc, -1, nbrk)),
           call(L.CtdFitParams(2, mw, 2, nc, ncum, -1)),
           call(jobs=None), call(fjobs=None), call(brows=None), call(bits=None), call(cands=None), call(cum=None), call(brk=None),
           call(rows=None),
           call(L.CtdFitParams(2, mw, 2, nc - 1, ncum, nbrk)),                # the last job's candidates lie beyond the table
           call(L.CtdFitParams(2, mw, 2, nc, ncum - 1, nbrk)),                # the last candidate's advances
           call(L.CtdFitParams(2, mw, 2, nc, ncum, nbrk - 1)),                # the first job's breaks
           call(edit=("job", 0, "n_glyphs", L.FIT_MAX_GLYPHS + 1)), call(edit=("job", 0, "n_glyphs", -1)),
           call(edit=("job", 0, "n_glyphs", 13)),                             # one more than its tables hold
           call(edit=("job", 1, "n_cands", L.FIT_MAX_CANDS + 1)), call(edit=("job", 1, "n_cands", -1)),
           call(edit=("job", 1, "cand0", 3)), call(edit=("job", 1, "cand0", -1)),
           call(edit=("job", 0, "break0", 1)), call(edit=("job", 0, "break0", -2)),
           call(edit=("cand", 1, "line", 0)), call(edit=("cand", 2, "gap", -1)),
           call(edit=("cand", 4, "cum0", ncum - 5)), call(edit=("cand", 0, "cum0", -1))]
    assert all(rc != L.OK for rc in bad), bad
    assert (out.cpu().numpy() == GUARD).all(), "a refused call wrote rows"
    assert call(n=0) == L.OK and (out.cpu().numpy() == GUARD).all()          # n = 0 launches nothing
    assert call() == L.OK
    rows = out.cpu().numpy()[: 2 * ROW].copy().view(Y.FIT_ROW_DTYPE)
    assert [FR.row_dict(r) for r in rows] == [_want(c, 2) for c in good] and rows["status"].tolist() == [FR.OK, FR.OK]
    assert call(edit=("job", 0, "break0", -1)) == L.OK                       # -1 is the legal "no table"
    # the Python layer refuses before anything is uploaded
    page, mask, box = BR.chamber_page()
    br = p.balloons.balloon_regions([page], [mask], [[TL._Blk(box)]])
    cum = [np.array([[0, 3, 6]])]
    for kw in (dict(inset=17), dict(inset=-1), dict(inset=2.5), dict(anchors=np.zeros((2, 2), np.int64)), dict(anchors=[[1.5, 2.0]]),
               dict(breaks=[[True]])):
        with pytest.raises(ValueError):
            Y.shaped_fit(br, cum, 4, 0, **kw)
    for args in ((cum * 2, 4, 0), (cum, 0, 0), (cum, 4, -1), ([np.array([[0, 3, 2]])], 4, 0)):
        with pytest.raises(ValueError):
            Y.shaped_fit(br, *args)
    none = Y.shaped_fit(p.balloons.balloon_regions([page], [mask], [[]]), [], 4, 0)   # a page without blocks: nothing launched
    assert len(none) == 0


# ---- 3. behind the balloon launch ---------------------------------------------------------------------------------------------

def _chamber_planes(material):
    """Per block of the chamber pages (window, plane, balloon status) from `balloon_ref.balloon_page`."""
    out = []
    for page, mask, boxes in material:
        rows, words, wins, _ = BR.balloon_page(page, mask, boxes)
        for row, w, win in zip(rows, words, wins):
            out.append((tuple(int(v) for v in win), None if w is None else BR.unpack(w, win[3] - win[1], win[2] - win[0]),
                        row["status"]))
    return out


def test_shaped_fit_behind_balloon_regions():
    p = pkg()
    B, Y = p.balloons, p.layout
    material = TL._chambers()
    lists = [[TL._Blk(b) for b in m[2]] for m in material]
    br = B.balloon_regions([m[0] for m in material], [m[1] for m in material], lists)
    before = br.bits.view(torch.int64).clone()
    planes = _chamber_planes(material)
    assert len(br) == len(planes) == 4 and br.ok.all()
    texts = [_text(14, (3, 5, 8, 12, 17), 60 + j) for j in range(4)]
    brk = [None, np.arange(14) % 3 == 2, None, np.zeros((14,), bool)]
    cum = [np.stack(t[0]) for t in texts]
    lines = np.array(texts[0][1])
    for inset, anchors in ((2, None), (5, None), (0, np.array([[22, 30], [50, 30], [-7, -7], [150, 30]]))):
        sf = Y.shaped_fit(br, cum, lines, 1, breaks=brk, anchors=anchors, inset=inset,
                          stream=None if inset else torch.cuda.Stream())
        use = br.center if anchors is None else anchors
        want = [FR.fit_row(pl, win, use[j], texts[j][0], texts[j][1], [1] * 5, breaks=brk[j], inset=inset, balloon_status=st)
                for j, (win, pl, st) in enumerate(planes)]
        assert [FR.row_dict(r) for r in sf.rows] == want, inset
        assert sf.inset == inset and np.array_equal(sf.index, br.index) and sf.anchors.tolist() == np.asarray(use).tolist()
        assert sf.lines.shape == (4, 32, 5) and np.array_equal(sf.lines[:, :, 3], sf.rows["lines"]["width"])
    assert sf.status.tolist()[2] == FR.NO_ANCHOR and sf.ok[3] and repr(sf).startswith("ShapedFit(4 blocks")
    sf = Y.shaped_fit(br, [cum[0], None, cum[2][:, :1], cum[3]], lines, 1)    # no run, a run without a glyph
    assert sf.status.tolist()[1:3] == [FR.NO_TEXT, FR.NO_TEXT] and sf.ok[0] and sf.ok[3]
    assert torch.equal(br.bits.view(torch.int64), before)


# ---- 4. through the detector --------------------------------------------------------------------------------------------------

def test_typeset_text_shaped_equals_the_restatements():
    """`det.typeset_text(..., shaped=br)` on the chamber pages: the sizes, the line counts and the glyph positions are those of
    `fit_ref.fit_row` and `fit_ref.place` on the restated balloon planes with the font's metrics, and the pages are
    `glyph_ref.typeset` (the typeset restatement on composed bitmaps) of those placements with the raster restatement's
    bitmaps.  `shaped=None` gives what the chain done by hand gives, byte for byte; a block whose anchor is forced off its
    region takes the rectangle path."""
    p, det = pkg(), TG.detector()
    G, Y, B = p.glyphs, p.layout, p.balloons
    material = TL._chambers()
    pages = [m[0] for m in material]
    br = B.balloon_regions(pages, [m[1] for m in material], [[TL._Blk(b) for b in m[2]] for m in material])
    lb = Y.layout_boxes(br)
    font, outlines = TRS._font(G)
    rng = np.random.default_rng(21)
    runs = [rng.integers(0, 20, 7 + 2 * j) for j in range(4)]
    runs[1] = None
    sizes = [6, 8, 10, 12, 14, 16]
    kw = dict(fill=(10, 10, 10), stroke=(250, 250, 250), radius=1, gap=1)
    atlas = G.GlyphAtlas(device=det.net.device)
    tp = det.typeset_text(pages, lb, font, atlas, runs, sizes, shaped=br, **kw)
    idx = [0, 2, 3]
    assert tp.layer_of.tolist() == [0, -1, 1, 2] and tp.shaped.all() and tp.fits.all()
    planes = _chamber_planes(material)
    bitmaps, places, layers, xy_all = [], [], [], []
    for i, j in enumerate(idx):
        uniq, pos = np.unique(runs[j], return_inverse=True)
        ms = [font.metrics(uniq, s) for s in sizes]
        cums = [np.concatenate([[0], np.cumsum(m.advance[pos, 0])]) for m in ms]
        win, plane, st = planes[j]
        row = FR.fit_row(plane, win, lb.anchors[j], cums, [m.line for m in ms], [1] * len(sizes), inset=lb.inset + 1, balloon_status=st)
        assert row["status"] == FR.OK and FR.row_dict(tp.fit.rows[j]) == row
        c = row["cand"]
        assert tp.size[i] == sizes[c] and tp.n_lines[i] == row["n_lines"]
        xy = FR.place(row, ms[c].advance[pos, 0], ms[c].bearing[pos])
        xy_all.append(xy)
        first = len(bitmaps)
        bitmaps += [RR.rasterise(outlines[g], font.scale(sizes[c]))[0] for g in uniq]
        places += [(i, first + int(q), int(x), int(y)) for q, (x, y) in zip(pos, xy)]
        layers.append(GR.glayer(int(lb.index[j, 0]), 1, (10, 10, 10), (250, 250, 250)))
    assert np.array_equal(np.concatenate(xy_all), tp.xy)
    want_pages, want_rows, _ = GR.typeset(pages, layers, places, bitmaps)
    got = tp.to_host()
    assert all(np.array_equal(a, b) for a, b in zip(got, want_pages))
    assert np.array_equal(np.stack([tp.n_fill, tp.n_stroke], axis=1), want_rows)
    assert tp.n_fill.sum() > 0
    print(f"\nshaped sizes {tp.size.tolist()}, lines {tp.n_lines.tolist()}")

    # shaped=None: the chain done by hand, as before
    plain = det.typeset_text(pages, lb, font, G.GlyphAtlas(device=det.net.device), runs, sizes, **kw)
    hand = G.GlyphAtlas(device=det.net.device)
    chosen = [G.fit(runs[j], font, lb.a_rect[j] if lb.a_area[j] > 0 else lb.rect[j], sizes, gap=1) for j in idx]
    ids = hand.rasterise(font, np.concatenate([runs[j] for j in idx]), np.repeat([float(c[0]) for c in chosen], [len(runs[j]) for j in idx]))
    xy = np.concatenate([G.flow_outlines(runs[j], font, lb.a_rect[j] if lb.a_area[j] > 0 else lb.rect[j], c[0], gap=1)[0]
                         for j, c in zip(idx, chosen)])
    by_hand = G.typeset_glyphs(pages, hand, lb.index[idx, 0], np.repeat(np.arange(3), [len(runs[j]) for j in idx]), ids, xy,
                               fill=(10, 10, 10), stroke=(250, 250, 250), radius=1, device=det.net.device)
    assert all(np.array_equal(a, b) for a, b in zip(plain.to_host(), by_hand.to_host())) and plain.rows.tobytes() == by_hand.rows.tobytes()
    assert np.array_equal(plain.xy, xy) and plain.size.tolist() == [c[0] for c in chosen] and not hasattr(plain, "shaped")

    # block 0's anchor forced off its region: NO_ANCHOR, and the block is set as the rectangle path sets it
    anchors = lb.anchors.copy()
    anchors[0] = (-7, -7)
    moved = Y.LayoutBoxes(lb.index, lb.rows, anchors, lb.inset)
    only = [runs[0], None, None, None]
    forced = det.typeset_text(pages, moved, font, G.GlyphAtlas(device=det.net.device), only, sizes, shaped=br, **kw)
    rect = det.typeset_text(pages, lb, font, G.GlyphAtlas(device=det.net.device), only, sizes, **kw)
    assert forced.fit.status[0] == FR.NO_ANCHOR and forced.shaped.tolist() == [False] and forced.n_lines.tolist() == [0]
    assert np.array_equal(forced.xy, rect.xy) and forced.size.tolist() == rect.size.tolist() and forced.fits.tolist() == rect.fits.tolist()
    assert all(np.array_equal(a, b) for a, b in zip(forced.to_host(), rect.to_host())) and forced.rows.tobytes() == rect.rows.tobytes()
    with pytest.raises(ValueError):
        det.typeset_text(pages, lb, font, atlas, runs, sizes, shaped=br, vertical=True, **kw)
    with pytest.raises(ValueError):
        det.typeset_text(pages, lb, font, atlas, runs, list(range(6, 40)), shaped=br, **kw)
