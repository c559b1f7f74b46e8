"""Layout boxes without a GPU: the two methods of the numpy restatement (tests/layout_ref.py) against each other and against
answers written out by hand, what the named material promises, argument checks of `layout.layout_boxes`, and the layout of
the ABI structs against the header.  The kernel itself is compared with the restatement in tests/test_gpu_layout.py."""
import ctypes as C

import numpy as np
import pytest

import balloon_ref as BR
import layout_ref as LR
from c_layout import compiled_flat
from conftest import pkg


# ---- the rule ----------------------------------------------------------------------------------------------------------

def test_the_stack_and_every_rectangle_agree():
    """Several hundred random planes up to 10 x 12 at mixed densities, free and anchored, and the named planes: the stack's
    maximal rectangles and the summed-area table over every rectangle give the same answer under the order."""
    rng = np.random.default_rng(11)
    differs = n = 0
    for i in range(400):
        h, w = int(rng.integers(1, 11)), int(rng.integers(1, 13))
        plane = rng.random((h, w)) < (0.5, 0.7, 0.85, 0.95)[i % 4]
        free = LR.best_rect(plane)
        assert free == LR.best_rect_brute(plane), plane
        x1, y1, x2, y2 = free[1]
        assert free[0] == (x2 - x1) * (y2 - y1) and (free[0] == 0 or plane[y1:y2, x1:x2].all())
        for ax, ay in ((int(rng.integers(0, w)), int(rng.integers(0, h))) for _ in range(3)):
            got = LR.best_rect(plane, (ax, ay))
            assert got == LR.best_rect_brute(plane, (ax, ay)), (plane, ax, ay)
            assert (got[0] > 0) == bool(plane[ay, ax])
            if got[0]:
                assert got[1][0] <= ax < got[1][2] and got[1][1] <= ay < got[1][3] and got[0] <= free[0]
                n += 1
                differs += got != free
    assert n > 500 and differs > 100                         # the anchored answer is a different question
    for name, (plane, anchor, want, a_want) in LR.NAMED.items():
        for method in (LR.best_rect, LR.best_rect_brute):
            assert method(plane) == want, name
            if anchor is not None:
                assert method(plane, anchor) == a_want, name


def test_the_named_planes_hold_what_their_names_promise():
    N = LR.NAMED
    # each tie is decided by the key its name says: the loser has the same area and loses on exactly that key
    for name, loser, key in (("tie_on_y1", [0, 2, 2, 4], 1), ("tie_on_x1", [4, 0, 6, 2], 0), ("tie_on_y2", [0, 0, 1, 4], 3)):
        plane, _, (area, rect), _ = N[name]
        x1, y1, x2, y2 = loser
        assert plane[y1:y2, x1:x2].all() and (x2 - x1) * (y2 - y1) == area, name
        order = (1, 0, 3)                                    # y1, then x1, then y2
        for k in order[:order.index(key)]:
            assert rect[k] == loser[k], name
        assert rect[key] < loser[key], name
    plane, anchor, want, a_want = N["anchored_differs"]
    assert a_want != want and 0 < a_want[0] < want[0] and plane[anchor[1], anchor[0]]
    plane, anchor, want, a_want = N["anchor_outside"]
    assert not plane[anchor[1], anchor[0]] and a_want == (0, [0, 0, 0, 0]) and want[0] > 0
    # the kernel's material: the staircase's best step is in the middle, the plus and the L tie, the corridor is thin
    st = LR.staircase()
    assert LR.best_rect(st) == (5 * 16 * 4 * 8, [64, 24, 128, 64])              # steps 3 and 4 tie: step 4 starts higher up
    assert LR.best_rect(LR.plus()) == (650, [27, 0, 37, 65]) and LR.best_rect(LR.ell()) == (600, [0, 0, 60, 10])
    co = LR.corridor()
    assert LR.best_rect(co) == (4000, [60, 0, 160, 40]) and LR.best_rect(co, (10, 19)) == (480, [0, 18, 160, 21])
    assert LR.best_rect(LR.comb()) == (65 * 6, [0, 35, 65, 41]) and LR.best_rect(LR.comb(), (32, 3)) == (41, [32, 0, 33, 41])
    rg = LR.ring()
    assert LR.best_rect(rg) == (100 * 20, [0, 0, 100, 20]) and LR.best_rect(rg, (50, 25))[0] == 0
    names = [m[0] for m in LR.material()]
    assert len(set(names)) == len(names)
    widths = {m[1].shape[1] for m in LR.material()}
    heights = {m[1].shape[0] for m in LR.material()}
    assert {1, 63, 64, 65, 128, 129, 1000} <= widths and {1, 2, 64} <= heights
    assert {m[3] for m in LR.material()} == {BR.OK, BR.NOT_PLAIN, BR.TOO_LARGE}


def test_erosion_and_rows():
    """`erode` against the rule's statement pixel by pixel; `layout_row` in page coordinates, its statuses, the window's edge."""
    rng = np.random.default_rng(3)
    for m in (0, 1, 2, 5):
        plane = rng.random((17, 23)) < 0.97
        want = np.zeros_like(plane)
        for y in range(17):
            for x in range(23):
                want[y, x] = y - m >= 0 and x - m >= 0 and y + m < 17 and x + m < 23 and plane[y - m:y + m + 1, x - m:x + m + 1].all()
        assert np.array_equal(LR.erode(plane, m), want)
    assert np.array_equal(LR.erode(plane, 0), plane) and not LR.erode(np.ones((32, 200), bool), 16).any()
    assert LR.erode(np.ones((33, 40), bool), 16).sum() == 8
    # a 60 x 40 room of ones in a window at (8, 5): the window's edge erodes like an outline
    room = np.ones((40, 60), bool)
    win = (8, 5, 68, 45)
    assert LR.layout_row(room, win, (30, 20), inset=2) == dict(status=LR.OK, n_inner=56 * 36, area=56 * 36, rect=[10, 7, 66, 43],
                                                               a_area=56 * 36, a_rect=[10, 7, 66, 43])
    assert LR.layout_row(room, win, (9, 20), inset=2)["a_area"] == 0         # the anchor is in the margin
    assert LR.layout_row(room, win, (9, 20), inset=0)["a_rect"] == [8, 5, 68, 45]
    assert LR.layout_row(room, win, (7, 20), inset=0)["a_area"] == 0         # ... and outside the window
    assert LR.layout_row(room, win, (30, 20), inset=16) == dict(status=LR.OK, n_inner=28 * 8, area=28 * 8, rect=[24, 21, 52, 29],
                                                                a_area=0, a_rect=[0, 0, 0, 0])
    assert LR.layout_row(room[:30], (8, 5, 68, 35), (30, 20), inset=16) == LR._zero_row(LR.EMPTY)
    assert LR.layout_row(room, win, (30, 20), balloon_status=BR.NOT_PLAIN) == LR._zero_row(LR.NO_REGION)
    assert LR.layout_row(room, win, (30, 20), balloon_status=BR.TOO_LARGE) == LR._zero_row(LR.NO_REGION)
    assert LR.layout_row(None, (0, 0, 64, 8193), (3, 3)) == LR._zero_row(LR.NO_REGION)
    assert LR.layout_row(room, win, (30, 20), max_words=39) == LR._zero_row(LR.NO_REGION)
    for bad in (-1, 17):
        with pytest.raises(ValueError):
            LR.layout_row(room, win, (30, 20), inset=bad)
    # the brute method through layout_row on a small plane
    small = rng.random((9, 11)) < 0.9
    for anchor in ((3, 4), (13, 9)):
        assert LR.layout_row(small, (3, 2, 14, 11), anchor, inset=0) == \
            LR.layout_row(small, (3, 2, 14, 11), anchor, inset=0, method=LR.best_rect_brute)


# ---- the Python layer ------------------------------------------------------------------------------------------------------

def _regions(p, n=2):
    """A hand-made `BalloonRegions` of n blocks with host bits: enough for the argument checks."""
    B = p.balloons
    import torch
    rows = np.zeros((n,), B.ROW_DTYPE)
    win = np.array([(0, 0, 70, 9)] * n, np.int64)
    nw = np.full((n,), 2, np.int64)
    return B.BalloonRegions(np.stack([np.zeros(n), np.arange(n)], axis=1), rows, win, nw, np.arange(n) * 18, np.zeros((n,), bool),
                            torch.zeros((18 * n,), dtype=torch.int64).view(torch.uint64), np.zeros((n,), p.erase.ROW_DTYPE))


def test_layout_boxes_argument_checks_need_no_gpu():
    p = pkg()
    Y = p.layout
    br = _regions(p)
    for bad in (-1, 17, 2.0, True, None):
        with pytest.raises(ValueError):
            Y.check_params(bad)
        with pytest.raises(ValueError):
            Y.layout_boxes(br, inset=bad)
    for ok in (0, 2, 16, np.int64(3)):
        assert Y.check_params(ok).inset == int(ok)
    for anchors in (np.zeros((2,), np.int64), np.zeros((3, 2), np.int64), np.zeros((2, 3), np.int64), np.zeros((2, 2), np.float32),
                    np.zeros((2, 2), bool), np.full((2, 2), 2 ** 31), [[0, 0]], [[0.5, 1], [2, 3]]):
        with pytest.raises(ValueError):
            Y.layout_boxes(br, anchors)
    none = Y.layout_boxes(_regions(p, 0))                                # no block: nothing to launch
    assert len(none) == 0 and none.rect.shape == (0, 4) and none.a_rect.shape == (0, 4) and none.anchors.shape == (0, 2)
    assert none.index.shape == (0, 2) and none.inset == 2 and repr(none) == "LayoutBoxes(0 blocks, 0 ok, inset 2)"
    assert Y.layout_boxes(p.balloons.balloon_regions([], [], []), inset=0).rows.dtype == Y.ROW_DTYPE
    import torch
    if not torch.cuda.is_available():
        with pytest.raises(p._lib.CtdError):
            Y.layout_boxes(br)
    # the anchors of the detector's wrapper: the centres of the boxes clipped to the page
    a = Y.box_anchors([np.array([(10, 20, 31, 41), (-10, -4, 7, 9), (90, 50, 130, 70)]), np.zeros((0, 4)), np.array([(0, 0, 5, 5)])],
                      [(60, 100), (10, 10), (8, 4)])
    assert a.tolist() == [[20, 30], [3, 4], [95, 55], [2, 2]] and Y.box_anchors([], []).shape == (0, 2)


# ---- ABI -------------------------------------------------------------------------------------------------------------------

def test_layout_structs_have_the_c_layout():
    """`layout.JOB_DTYPE` / `ROW_DTYPE` and the `_lib` mirrors against the header, compiled: sizes, every field's offset, the
    constants; the entry point is exported and bound, and refuses bad arguments before it launches anything."""
    p = pkg()
    L, Y = p._lib, p.layout
    fields = {"ctd_layout_job": ("win", "ax", "ay", "word0"),
              "ctd_layout_params": ("inset", "max_words", "n_rows", "pad_"),
              "ctd_layout_row": ("status", "n_inner", "area", "rect", "a_area", "a_rect")}
    consts = ("CTD_LAYOUT_OK", "CTD_LAYOUT_NO_REGION", "CTD_LAYOUT_EMPTY", "CTD_LAYOUT_MAX_INSET", "CTD_ABI_VERSION")
    vals = compiled_flat(fields, consts)
    mirrors = {"ctd_layout_job": (L.CtdLayoutJob, Y.JOB_DTYPE, 32), "ctd_layout_params": (L.CtdLayoutParams, None, 16),
               "ctd_layout_row": (L.CtdLayoutRow, Y.ROW_DTYPE, 48)}
    k = 0
    for s, fs in fields.items():
        ct, dt, size = mirrors[s]
        assert vals[k] == C.sizeof(ct) == size and (dt is None or dt.itemsize == size), s
        assert vals[k + 1:k + 1 + len(fs)] == [getattr(ct, f).offset for f in fs], s
        assert [f for f, _ in ct._fields_] == list(fs)
        if dt is not None:
            assert vals[k + 1:k + 1 + len(fs)] == [dt.fields[f][1] for f in fs] and dt.names == fs, s
        k += 1 + len(fs)
    assert vals[k:] == [L.LAYOUT_OK, L.LAYOUT_NO_REGION, L.LAYOUT_EMPTY, L.LAYOUT_MAX_INSET, L.ABI_VERSION]
    assert vals[k:k + 4] == [LR.OK, LR.NO_REGION, LR.EMPTY, LR.MAX_INSET] == [0, 1, 2, 16]
    assert Y.ROW_DTYPE.names == LR.FIELDS
    assert "ctd_layout_boxes" in L.SYMBOLS and hasattr(L.lib(), "ctd_layout_boxes")
    # the entry point refuses parameters outside their bounds before anything else (nothing is launched: no GPU is needed)
    lib = L.lib()
    for vals in ((-1, 8, 1), (17, 8, 1), (2, -1, 1), (2, 8193, 1), (2, 8, -1)):
        prm = L.CtdLayoutParams(*vals)
        assert lib.ctd_layout_boxes(8, 1, 8, 8, C.byref(prm), 8, None) != L.OK, vals
    prm = L.CtdLayoutParams(2, 8, 1)
    assert lib.ctd_layout_boxes(8, -1, 8, 8, C.byref(prm), 8, None) != L.OK
    assert lib.ctd_layout_boxes(8, 1, 8, 8, None, 8, None) != L.OK
    assert lib.ctd_layout_boxes(None, 1, 8, 8, C.byref(prm), 8, None) != L.OK
    assert lib.ctd_layout_boxes(8, 1, None, 8, C.byref(prm), 8, None) != L.OK
    assert lib.ctd_layout_boxes(8, 1, 8, None, C.byref(prm), 8, None) != L.OK                # words to read and no buffer
    assert lib.ctd_layout_boxes(8, 1, 8, 8, C.byref(prm), None, None) != L.OK
    assert b"null" in lib.ctd_last_error()
    assert lib.ctd_layout_boxes(None, 0, None, None, C.byref(prm), None, None) == L.OK       # nothing to do
