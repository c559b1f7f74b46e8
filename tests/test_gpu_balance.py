"""-m gpu: the balanced breaker -- `ctd_layout_fit_balanced` (csrc/kernels_fit.hip), `layout.shaped_fit(balance=True)` and
`TextDetector.typeset_text(shaped=, balance=True)` -- against the numpy restatement tests/balance_ref.py, which fills the whole
table g(k, s) from the rule's statement.  Integers only, so every comparison is EXACT: every field of both rows.  The block
lists, the device tables and the references of the unbalanced rows are tests/test_gpu_fit.py's."""
import ctypes as C

import numpy as np
import pytest
import torch

import balance_ref as BAL
import balloon_ref as BR
import fit_ref as FR
import glyph_ref as GR
import raster_ref as RR
import test_gpu_fit as TF
import test_gpu_layout as TL
import test_gpu_raster as TRS
import test_gpu_regions as TG
from conftest import pkg

pytestmark = pytest.mark.gpu

GUARD, ROW, BAL_ROW = TF.GUARD, TF.ROW, 16


def _waist(G):
    """A 21 x 60 window whose rows 27 .. 33 are 11 wide about the anchor's column: lines of 5 rows, 5 apart, stand clear of
    the waist only as the first and the third of three.  Glyphs of 5, breaks allowed after glyphs 1 and 2 only: the greedy
    stack ends line 0 at glyph 3 and has to break line 1 hard inside the waist."""
    plane = np.ones((60, 21), bool)
    plane[27:34, :5] = plane[27:34, 16:] = False
    brk = np.zeros((G,), bool)
    brk[1:3] = True
    return TF.case(plane, (2, 3, 23, 63), (2 + 10, 3 + 30), ([np.arange(G + 1) * 5], [5], [5]), breaks=brk)


def _worst():
    """A 64 x 8192 window, lines of 1 row 1 apart, 4096 glyphs: 32 units of 127 glyphs of advance 0 (a few 1) and one of 40.
    Two of those never share a slot of 64 or 60, so 32 lines are needed and suffice; every cut between two of them is open."""
    rng = np.random.default_rng(77)
    adv = (rng.random(4096) < 0.06).astype(np.int64)
    adv[127::128] = 40
    return TF._ones(8192, 64, 32, 4096, ([np.concatenate([[0], np.cumsum(adv)])], [1], [1]), x0=1, y0=2)


def _extra():
    """[(name, case)]: the shapes the balanced breaker can go wrong at."""
    out = [("one_glyph_G1", TF._ones(80, 200, 100, 40, ([np.array([0, 5])], [5], [1]))),
           ("one_glyph_a_line", TF._ones(200, 21, 10, 100, ([np.arange(6) * 15], [3], [0]))),
           ("monospace_ties", TF._ones(200, 41, 20, 100, ([np.arange(10) * 6], [3], [0]))),
           ("monospace_ties_4_lines", TF._ones(200, 41, 20, 100, ([np.arange(21) * 6], [3], [2]))),
           ("zero_advances_only", TF._ones(40, 65, 32, 20, ([np.zeros((7,), np.int64)], [3], [0]))),
           ("zero_advances_between", TF._ones(60, 41, 20, 30, ([np.cumsum([0, 9, 0, 0, 9, 0, 9, 9, 0, 0, 0, 9, 9, 0, 9])], [3], [1]))),
           ("hard_break_with_a_vector", _waist(6)), ("hard_break_without_a_vector_at_inset_2", _waist(7)),
           ("worst_64x8192", _worst())]
    rng = np.random.default_rng(78)
    for w in (63, 64, 65):                                  # about 3.6 lines of small glyphs: wide bands, 200 glyphs
        adv = rng.integers(0, 3, 200)
        out.append((f"w{w}_200_glyphs", TF._ones(40, w, w // 2, 20, ([np.concatenate([[0], np.cumsum(adv)])], [3], [0]), x0=5, y0=1,
                                                 breaks=BAL.word_breaks(200, rng) if w == 64 else None)))
    return out


def _cases():
    """test_gpu_fit's blocks, the extra ones in front of its last: that one lies beyond the balloon row table."""
    base = TF._cases()
    return base[:-1] + _extra() + base[-1:]


_REF = {}


def _reference(inset):
    """Per case (row, balance row) under the restatement, computed once per inset; the unbalanced rows of test_gpu_fit's
    blocks are its own reference's."""
    if inset not in _REF:
        cases = [c for _, c in _cases()]
        base = TF._reference(inset)
        rows = base[:-1] + [TF._want(c, inset) for _, c in _extra()] + base[-1:]
        _REF[inset] = [BAL.rebalance(r, c["cums"], c["breaks"]) for r, c in zip(rows, cases)]
    return _REF[inset]


def _run(p, cases, inset, n_rows=None, lead=0, bal_lead=0, work_lead=0, slack=0):
    """One `ctd_layout_fit_balanced` call on the current stream: (rows, balance rows, whether a byte of the workspace was
    written).  The workspace is `ctd_layout_fit_work_bytes` + `slack` bytes; the guards around the three buffers and every
    word of the bit buffer are checked after the call."""
    L, Y = p._lib, p.layout
    n = len(cases)
    tab, bits, words, out, ptr, (nc, ncum, nbrk), mw = TF._upload(p, cases, lead)
    fjobs = tab.cpu().numpy()[ptr[1] - tab.data_ptr():][: n * Y.FIT_JOB_DTYPE.itemsize].copy()
    need = L.lib().ctd_layout_fit_work_bytes(fjobs.ctypes.data, n)
    assert need == sum(256 * (len(c["cums"][0]) if c["cums"] and len(c["cums"][0]) > 1 else 0) for c in cases)
    dev = out.device
    bal = torch.full((bal_lead + n * BAL_ROW + 64,), GUARD, dtype=torch.uint8, device=dev)
    work = torch.full((work_lead + need + slack + 256,), GUARD, dtype=torch.uint8, device=dev)
    assert out.data_ptr() % 8 == 0 and bal.data_ptr() % 8 == 0 and work.data_ptr() % 256 == 0
    prm = L.CtdFitParams(inset, mw, n if n_rows is None else n_rows, nc, ncum, nbrk)
    st = torch.cuda.current_stream()
    L.check(L.lib().ctd_layout_fit_balanced(ptr[0], ptr[1], n, ptr[2], bits.data_ptr() + 8, ptr[3] if nc else None,
                                            ptr[4] if ncum else None, ptr[5] if nbrk else None, C.byref(prm), out.data_ptr() + lead,
                                            bal.data_ptr() + bal_lead, work.data_ptr() + work_lead, need + slack, st.cuda_stream),
            "ctd_layout_fit_balanced")
    st.synchronize()
    host, hbal, hwork = out.cpu().numpy(), bal.cpu().numpy(), work.cpu().numpy()
    assert (host[:lead] == GUARD).all() and (host[lead + n * ROW:] == GUARD).all(), "a byte outside the row table was written"
    assert (hbal[:bal_lead] == GUARD).all() and (hbal[bal_lead + n * BAL_ROW:] == GUARD).all(), "a byte outside the balance table"
    assert (hwork[:work_lead] == GUARD).all() and (hwork[work_lead + need + slack:] == GUARD).all(), "a byte outside the workspace"
    assert np.array_equal(bits.cpu().numpy().view(np.uint64), words), "the bit buffer was written"
    return (host[lead: lead + n * ROW].copy().view(Y.FIT_ROW_DTYPE), hbal[bal_lead: bal_lead + n * BAL_ROW].copy().view(Y.FIT_BALANCE_DTYPE),
            bool((hwork[work_lead: work_lead + need] != GUARD).any()))


def _compare(names, rows, bals, want, what):
    bad = [(nm, FR.row_dict(r), BAL.bal_dict(b), w) for nm, r, b, w in zip(names, rows, bals, want)
           if (FR.row_dict(r), BAL.bal_dict(b)) != w]
    assert not bad, f"{what}: {len(bad)} of {len(rows)} blocks differ, first: {bad[0]}"


# ---- 1. the kernel -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("inset", [0, 2])
def test_kernel_equals_the_restatement_in_every_field_of_both_rows(inset):
    """One call over test_gpu_fit's blocks and `_extra`'s: G = 1, one glyph a line, monospace advances whose vectors tie,
    advances of 0, a greedy stack that breaks hard with and without an admissible vector, the 64 x 8192 window with 4096
    glyphs in 32 lines, windows 63, 64 and 65 wide, and one block beyond the balloon row table.  Every status and both values
    of `balanced` occur under the restatement alone; the largest window sizes the LDS of the call, so every table of states
    lies there and no byte of the workspace is touched."""
    p = pkg()
    names, cases = [nm for nm, _ in _cases()], [c for _, c in _cases()]
    want = _reference(inset)
    counts = [sum(w[0]["status"] == s for w in want) for s in range(5)]
    ok = [w for w in want if w[0]["status"] == FR.OK]
    kinds = [sum(w[1]["balanced"] == v for w in ok) for v in (0, 1)]
    assert all(counts) and all(kinds), f"inset {inset}: statuses {counts}, balanced 0 / 1 among the OK blocks {kinds}"
    assert all(w[1] == dict(balanced=0, cost=0) for w in want if w[0]["status"] != FR.OK)
    by = dict(zip(names, want))
    greedy = dict(zip(names, TF._reference(inset)[:-1] + [None] * len(_extra())))
    moved = [nm for nm in names if greedy.get(nm) and by[nm][0] != greedy[nm]]
    assert len(moved) >= 5, moved                            # the balanced lines differ from the greedy ones on several blocks
    assert (by["one_glyph_G1"][0]["n_lines"], by["one_glyph_G1"][1]["balanced"]) == (1, 1)
    assert (by["one_glyph_a_line"][0]["n_lines"], by["one_glyph_a_line"][1]["balanced"]) == (5, 1)
    assert by["worst_64x8192"][0]["n_lines"] == 32 and by["worst_64x8192"][1]["balanced"] == 1
    assert by["hard_break_with_a_vector"][1]["balanced"] == 1
    assert [r[0] for r in by["hard_break_with_a_vector"][0]["lines"][:3]] == [0, 2, 3]
    assert by["hard_break_without_a_vector_at_inset_2"][1]["balanced"] == (1 if inset == 0 else 0)
    assert by["ellipse_no_break_allowed"][1]["balanced"] == 0 and by["ellipse_no_break_allowed"][0]["n_lines"] > 1
    if inset == 0:
        assert [r[0] for r in by["monospace_ties"][0]["lines"][:2]] == [0, 5]       # 4 + 5 and 5 + 4 glyphs cost the same
    rows, bals, touched = _run(p, cases, inset, n_rows=len(cases) - 1)
    _compare(names, rows, bals, want, f"inset {inset}")
    assert not touched
    print(f"\ninset {inset}: {len(cases)} blocks, statuses {counts}, balanced 0 / 1 {kinds}, {len(moved)} blocks' lines moved")


def _small():
    """The OK blocks in windows of at most 65 x 40 pixels, the 200-glyph runs last: their tables of states do not fit the LDS
    that the largest of these windows sizes, so they lie in the workspace, behind the parts of the blocks in front of them."""
    keep = [(nm, c) for nm, c in _cases()[:-1] if c["plane"].size <= 65 * 40 and c["status"] == BR.OK]
    assert [nm for nm, _ in keep][-3:] == ["w63_200_glyphs", "w64_200_glyphs", "w65_200_glyphs"] and len(keep) > 20
    return keep


def test_buffers_at_odd_offsets_and_untouched_guards():
    """The row table 68 bytes and the balance table 12 bytes into their buffers (4 off an 8-byte boundary), the workspace 8
    bytes into its own with 40 spare bytes behind what is needed; the tables of states of the 200-glyph runs lie in the
    workspace.  Both rows are the restatement's, and every byte around the three buffers is as it was (`_run` checks)."""
    p = pkg()
    names, cases = [nm for nm, _ in _small()], [c for _, c in _small()]
    full = dict(zip([nm for nm, _ in _cases()], _reference(2)))
    rows, bals, touched = _run(p, cases, 2, lead=68, bal_lead=12, work_lead=8, slack=40)
    _compare(names, rows, bals, [full[nm] for nm in names], "odd offsets")
    assert touched, "no table of states went to the workspace"
    assert all(full[f"w{w}_200_glyphs"][1]["balanced"] == 1 and full[f"w{w}_200_glyphs"][0]["n_lines"] >= 3 for w in (63, 64, 65))


# ---- 2. bad arguments ---------------------------------------------------------------------------------------------------------

def test_bad_arguments_are_refused_without_a_launch():
    """Every refusal of `ctd_layout_fit`'s, a short, missing or misaligned workspace and a NULL balance table: the rows, the
    balance rows and the workspace keep their guard bytes, so nothing was launched."""
    p = pkg()
    L, Y = p._lib, p.layout
    lib = L.lib()
    good = [TF._ones(40, 65, 32, 20, TF._text(12, (2, 4), 50), breaks=np.arange(12) % 2 == 1), TF._ones(9, 70, 6, 4, TF._text(5, (2, 4, 6), 1))]
    tab, bits, words, out, ptr, (nc, ncum, nbrk), mw = TF._upload(p, good)
    st = torch.cuda.current_stream()
    host, base = tab.cpu().numpy(), tab.data_ptr()
    need = 256 * (13 + 6)
    fj = host[ptr[1] - base:][: 2 * Y.FIT_JOB_DTYPE.itemsize].copy()
    assert lib.ctd_layout_fit_work_bytes(fj.ctypes.data, 2) == need and lib.ctd_layout_fit_work_bytes(fj.ctypes.data, 1) == 256 * 13
    assert lib.ctd_layout_fit_work_bytes(None, 0) == 0 and lib.ctd_layout_fit_work_bytes(None, 1) == -1
    assert lib.ctd_layout_fit_work_bytes(fj.ctypes.data, -1) == -1
    bal = torch.full((2 * BAL_ROW + 64,), GUARD, dtype=torch.uint8, device=out.device)
    work = torch.full((need + 256,), GUARD, dtype=torch.uint8, device=out.device)

    def call(prm=None, n=2, edit=None, work_bytes=need, **null):
        """rc of a call with one thing wrong: a parameter, a null table, a field of a device table, or the workspace."""
        t, q = tab, list(ptr)
        if edit is not None:
            which, k, field, value = edit
            h = host.copy()
            off, dt = (ptr[1] - base, Y.FIT_JOB_DTYPE) if which == "job" else (ptr[3] - base, Y.FIT_CAND_DTYPE)
            h[off:].view(np.uint8)[: dt.itemsize * (k + 1)].view(dt)[k][field] = value
            t = torch.from_numpy(h).cuda()
            q = [t.data_ptr() + (x - base) for x in ptr]
        a = dict(jobs=q[0], fjobs=q[1], brows=q[2], bits=bits.data_ptr() + 8, cands=q[3], cum=q[4], brk=q[5], rows=out.data_ptr(),
                 bal=bal.data_ptr(), work=work.data_ptr())
        a.update(null)
        prm = L.CtdFitParams(2, mw, 2, nc, ncum, nbrk) if prm is None else prm
        rc = lib.ctd_layout_fit_balanced(a["jobs"], a["fjobs"], n, a["brows"], a["bits"], a["cands"], a["cum"], a["brk"], C.byref(prm),
                                         a["rows"], a["bal"], a["work"], work_bytes, st.cuda_stream)
        st.synchronize()
        return rc

    bad = [call(work_bytes=need - 1), call(work_bytes=0), call(work_bytes=-1), call(work=None), call(work=work.data_ptr() + 4),
           call(bal=None),
           call(n=-1), call(L.CtdFitParams(17, mw, 2, nc, ncum, nbrk)), call(L.CtdFitParams(-1, mw, 2, nc, ncum, nbrk)),
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

    def untouched():
        return all((t.cpu().numpy() == GUARD).all() for t in (out, bal, work))

    assert untouched(), "a refused call wrote"
    assert call(n=0) == L.OK and call(n=0, bal=None, work=None, work_bytes=0) == L.OK and untouched()   # n = 0 launches nothing
    assert call() == L.OK
    rows = out.cpu().numpy()[: 2 * ROW].copy().view(Y.FIT_ROW_DTYPE)
    bals = bal.cpu().numpy()[: 2 * BAL_ROW].copy().view(Y.FIT_BALANCE_DTYPE)
    want = [BAL.rebalance(TF._want(c, 2), c["cums"], c["breaks"]) for c in good]
    _compare(["a", "b"], rows, bals, want, "the good call")
    assert (bal.cpu().numpy()[2 * BAL_ROW:] == GUARD).all() and (work.cpu().numpy()[need:] == GUARD).all()
    # the Python layer refuses before anything is uploaded
    page, mask, box = BR.chamber_page()
    br = p.balloons.balloon_regions([page], [mask], [[TL._Blk(box)]])
    for balance in (1, "yes", None):
        with pytest.raises(ValueError):
            Y.shaped_fit(br, [np.array([[0, 3, 6]])], 4, 0, balance=balance)
    none = Y.shaped_fit(p.balloons.balloon_regions([page], [mask], [[]]), [], 4, 0, balance=True)   # a page without blocks
    assert len(none) == 0 and none.balanced.shape == (0,) and none.cost.dtype == np.int64


# ---- 3. behind the balloon launch ---------------------------------------------------------------------------------------------

def test_shaped_fit_balanced_behind_balloon_regions_and_unbalanced_as_before():
    """`shaped_fit(balance=True)` on the planes a real `balloon_regions` call left on the device, against the restatement on
    the restated planes; `balance=False` and no keyword give the bytes `ctd_layout_fit` gives, with `balanced` all False."""
    p = pkg()
    B, Y = p.balloons, p.layout
    material = TL._chambers()
    lists = [[TL._Blk(b) for b in m[2]] for m in material]
    br = B.balloon_regions([m[0] for m in material], [m[1] for m in material], lists)
    before = br.bits.view(torch.int64).clone()
    planes = TF._chamber_planes(material)
    assert len(br) == len(planes) == 4 and br.ok.all()
    texts = [TF._text(14, (3, 5, 8, 12, 17), 60 + j) for j in range(4)]
    brk = [None, np.arange(14) % 3 == 2, None, np.zeros((14,), bool)]
    cum = [np.stack(t[0]) for t in texts]
    lines = np.array(texts[0][1])
    moved = flags = 0
    for inset, anchors in ((2, None), (0, np.array([[22, 30], [50, 30], [-7, -7], [150, 30]]))):
        use = br.center if anchors is None else anchors
        greedy = [FR.fit_row(pl, win, use[j], texts[j][0], texts[j][1], [1] * 5, breaks=brk[j], inset=inset, balloon_status=st)
                  for j, (win, pl, st) in enumerate(planes)]
        want = [BAL.rebalance(g, texts[j][0], brk[j]) for j, g in enumerate(greedy)]
        moved += sum(w[0] != g for w, g in zip(want, greedy))
        flags += sum(w[1]["balanced"] for w in want)
        sf = Y.shaped_fit(br, cum, lines, 1, breaks=brk, anchors=anchors, inset=inset, balance=True,
                          stream=None if inset else torch.cuda.Stream())
        assert [(FR.row_dict(r), BAL.bal_dict(b)) for r, b in zip(sf.rows, sf.bal_rows)] == want, inset
        assert sf.balanced.tolist() == [bool(w[1]["balanced"]) for w in want] and sf.cost.tolist() == [w[1]["cost"] for w in want]
        assert sf.cost.dtype == np.int64 and sf.balanced.dtype == bool and sf.lines.shape == (4, 32, 5)
        plain, off = Y.shaped_fit(br, cum, lines, 1, breaks=brk, anchors=anchors, inset=inset), \
            Y.shaped_fit(br, cum, lines, 1, breaks=brk, anchors=anchors, inset=inset, balance=False)
        assert plain.rows.tobytes() == off.rows.tobytes() and [FR.row_dict(r) for r in off.rows] == greedy
        assert not off.balanced.any() and not off.cost.any() and off.bal_rows is None and not plain.balanced.any()
    assert moved and flags, "balancing moved no line of any block: the test shows nothing"
    assert torch.equal(br.bits.view(torch.int64), before)


# ---- 4. through the detector --------------------------------------------------------------------------------------------------

def test_typeset_text_balanced_equals_the_restatements():
    """`det.typeset_text(..., shaped=br, balance=True)` on the chamber pages: sizes and line counts are the unbalanced call's,
    the glyph positions are `fit_ref.place` of the restatement's balanced rows with the font's metrics, and the pages are
    `glyph_ref.typeset` of those placements with the raster restatement's bitmaps.  `balance=True` without `shaped` is
    refused; without `balance` the result has no `balanced`."""
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
    tp = det.typeset_text(pages, lb, font, G.GlyphAtlas(device=det.net.device), runs, sizes, shaped=br, balance=True, **kw)
    greedy = det.typeset_text(pages, lb, font, G.GlyphAtlas(device=det.net.device), runs, sizes, shaped=br, **kw)
    idx = [0, 2, 3]
    assert tp.layer_of.tolist() == [0, -1, 1, 2] and tp.shaped.all() and not hasattr(greedy, "balanced")
    assert tp.size.tolist() == greedy.size.tolist() and tp.n_lines.tolist() == greedy.n_lines.tolist()
    planes = TF._chamber_planes(material)
    bitmaps, places, layers, xy_all, flags = [], [], [], [], []
    for i, j in enumerate(idx):
        uniq, pos = np.unique(runs[j], return_inverse=True)
        ms = [font.metrics(uniq, s) for s in sizes]
        cums = [np.concatenate([[0], np.cumsum(m.advance[pos, 0])]) for m in ms]
        win, plane, st = planes[j]
        row, bal = BAL.balance_row(plane, win, lb.anchors[j], cums, [m.line for m in ms], [1] * len(sizes), inset=lb.inset + 1,
                                   balloon_status=st)
        assert row["status"] == FR.OK and (FR.row_dict(tp.fit.rows[j]), BAL.bal_dict(tp.fit.bal_rows[j])) == (row, bal)
        flags.append(bool(bal["balanced"]))
        c = row["cand"]
        xy = FR.place(row, ms[c].advance[pos, 0], ms[c].bearing[pos])
        xy_all.append(xy)
        first = len(bitmaps)
        bitmaps += [RR.rasterise(outlines[g], font.scale(sizes[c]))[0] for g in uniq]
        places += [(i, first + int(q), int(x), int(y)) for q, (x, y) in zip(pos, xy)]
        layers.append(GR.glayer(int(lb.index[j, 0]), 1, (10, 10, 10), (250, 250, 250)))
    assert tp.balanced.tolist() == flags and all(flags)
    assert np.array_equal(np.concatenate(xy_all), tp.xy)
    want_pages, want_rows, _ = GR.typeset(pages, layers, places, bitmaps)
    assert all(np.array_equal(a, b) for a, b in zip(tp.to_host(), want_pages))
    assert np.array_equal(np.stack([tp.n_fill, tp.n_stroke], axis=1), want_rows)
    assert not np.array_equal(tp.xy, greedy.xy), "balancing moved no glyph: the test shows nothing"
    with pytest.raises(ValueError):
        det.typeset_text(pages, lb, font, G.GlyphAtlas(device=det.net.device), runs, sizes, balance=True, **kw)
