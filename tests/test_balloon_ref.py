"""Balloon regions without a GPU: the rule's own promises on its numpy restatement (tests/balloon_ref.py) -- answers written
out by hand, 4-connectivity, a closed outline against one with a gap -- the host's tables (`balloons.balloon_tables`) against
the restatement's windows, argument checks of `balloons.balloon_regions`, and the layout of the ABI structs against the
header.  The kernel itself is compared with the restatement in tests/test_gpu_balloons.py."""
import ctypes as C

import numpy as np
import pytest

import balloon_ref as BR
import erase_ref as ER
from c_layout import compiled_flat
from conftest import pkg


def _plain(med, n_fill=0):
    return dict(status=ER.PLAIN, n_fill=n_fill, n_ring=0, cnt=[0, 0, 0], med=list(med))


# ---- the rule ----------------------------------------------------------------------------------------------------------

def test_diagonal_contact_does_not_join():
    """A black 9 x 9 page, one text pixel at (4, 4), g = 0, white pixels placed by hand; the erase row is given."""
    page = np.zeros((9, 9, 3), np.uint8)
    mask = np.zeros((9, 9), np.uint8)
    mask[4, 4] = 255
    page[5, 5] = page[3, 3] = page[3, 5] = page[5, 3] = 255                    # the four diagonal neighbours
    page[6, 5] = 255                                                            # hangs on a diagonal neighbour
    box = (4, 4, 5, 5)
    for method in (BR.flood, BR.flood_label):
        if method(np.ones((1, 1), bool), np.ones((1, 1), bool)) is None:
            continue                                                            # no scipy here: the queue alone
        rows, words, wins, _ = BR.balloon_page(page, mask, [box], erows=[_plain((255, 255, 255))], grow=0, tol=0, reach_min=8,
                                               method=method)
        assert wins == [(0, 0, 9, 9)]
        assert rows == [dict(status=BR.OK, area=1, bbox=[4, 4, 5, 5], flags=0, n_seed=1, sum_x=4, sum_y=4)]
        assert words[0].tolist() == [0, 0, 0, 0, 1 << 4, 0, 0, 0, 0]
        # one 4-neighbour (x = 5, y = 4) joins what hangs on it, and only that: (5, 3), (5, 5) and through it (5, 6)
        page2 = page.copy()
        page2[4, 5] = 255
        rows, words, _, _ = BR.balloon_page(page2, mask, [box], erows=[_plain((255, 255, 255))], grow=0, tol=0, reach_min=8,
                                            method=method)
        assert rows == [dict(status=BR.OK, area=5, bbox=[4, 3, 6, 7], flags=0, n_seed=1, sum_x=4 + 5 * 4, sum_y=3 + 4 + 4 + 5 + 6)]
        assert words[0].tolist() == [0, 0, 0, 1 << 5, 3 << 4, 1 << 5, 1 << 5, 0, 0]


def test_a_closed_outline_holds_the_region_and_a_gap_leaks_it():
    """A 60 x 40 room with a 1-pixel outline on a page of the balloon's own colour: closed, the region is the 58 x 38 interior;
    with ONE outline pixel missing it is the whole window but the outline, and the flags say where it left."""
    page, mask, box = BR.chamber_page(bg=255)
    rows, words, wins, erows = BR.balloon_page(page, mask, [box])
    assert erows[0]["status"] == ER.PLAIN and erows[0]["med"] == [255] * 3 and erows[0]["n_fill"] == 24 * 10
    assert wins == [(8, 0, 92, 60)]
    assert rows == [dict(status=BR.OK, area=58 * 38, bbox=[21, 11, 79, 49], flags=0, n_seed=240, sum_x=38 * (21 + 78) * 58 // 2,
                         sum_y=58 * (11 + 48) * 38 // 2)]
    plane = BR.unpack(words[0], 60, 84)
    want = np.zeros((60, 84), bool)
    want[11:49, 21 - 8:79 - 8] = True
    assert np.array_equal(plane, want) and len(words[0]) == 2 * 60
    page, mask, box = BR.chamber_page(bg=255, gap=(20, 30))
    rows, words, _, _ = BR.balloon_page(page, mask, [box])
    outline = 2 * 60 + 2 * 40 - 4
    assert rows[0]["area"] == 84 * 60 - outline + 1 and rows[0]["bbox"] == [8, 0, 92, 60] and rows[0]["n_seed"] == 240
    assert rows[0]["flags"] == BR.CUT_LEFT | BR.CUT_RIGHT | (BR.CUT_TOP | BR.CUT_BOTTOM) << 4 == 0xA5
    plane = BR.unpack(words[0], 60, 84)
    assert plane[30, 20 - 8] and not plane[29, 20 - 8] and not plane[10, 30] and plane[0, 0] and plane[59, 83]
    # on a page of another colour the gap lets out one pixel, the gap itself, and nothing is cut
    page, mask, box = BR.chamber_page(bg=200, gap=(20, 30))
    rows = BR.balloon_page(page, mask, [box])[0]
    assert rows[0]["area"] == 58 * 38 + 1 and rows[0]["bbox"] == [20, 11, 79, 49] and rows[0]["flags"] == 0


def test_statuses_holes_and_the_word_cap():
    page, mask, box = BR.chamber_page(bg=255)
    # another block's text inside the room is a hole; its own box reports its own region
    mask[38:42, 30:50] = 255
    page[38:42, 30:50] = 0
    rows, words, wins, erows = BR.balloon_page(page, mask, [box, (30, 38, 50, 42), (0, 0, 5, 5), (-9, 0, 0, 5)])
    assert [r["status"] for r in rows] == [BR.OK, BR.OK, BR.NOT_PLAIN, BR.NOT_PLAIN]
    assert [e["status"] for e in erows] == [ER.PLAIN, ER.PLAIN, ER.NO_MASK, ER.EMPTY]
    # F of the other block (its text grown by 2) is not open for this one, except where it is white anyway
    assert rows[0]["area"] == 58 * 38 - 20 * 4 and rows[1]["area"] == 58 * 38 - 20 * 6
    assert rows[2] == BR._zero_row(BR.NOT_PLAIN) and not words[2].any() and len(words[2]) == 37 and wins[2] == (0, 0, 37, 37)
    assert wins[3] == (0, 0, 0, 0) and len(words[3]) == 0
    # 8192 words are computed, 8193 are not: 64 x 8192 and 192 x 2731 pixels
    for (H, W), status in (((8192, 64), BR.OK), ((2731, 192), BR.TOO_LARGE), ((1024, 512), BR.OK), ((1024, 513), BR.TOO_LARGE)):
        win = BR.window((0, 0, W, H), H, W, 8, 32)[1]
        assert win == (0, 0, W, H) and (BR.n_words(win)[1] <= BR.MAX_WORDS) == (status == BR.OK)
    flat = np.full((2731, 192, 3), 9, np.uint8)
    m = np.zeros((2731, 192), np.uint8)
    m[5:8, 5:20] = 1
    rows, words, _, _ = BR.balloon_page(flat, m, [(0, 0, 192, 2731)], erows=[_plain((9, 9, 9))])
    assert rows == [BR._zero_row(BR.TOO_LARGE)] and words == [None]
    for bad in (dict(grow=-1), dict(grow=9), dict(tol=-1), dict(tol=256), dict(reach=-1), dict(reach=33), dict(reach_min=7),
                dict(reach_min=1025)):
        with pytest.raises(ValueError):
            BR.balloon_page(page, mask, [box], **bad)


def test_the_queue_and_the_labelling_agree():
    rng = np.random.default_rng(5)
    if BR.flood_label(np.ones((1, 1), bool), np.ones((1, 1), bool)) is None:
        return                                                                  # no scipy on this machine: nothing to hold against
    for dens in (0.3, 0.55, 0.62, 0.8):
        open_ = rng.random((40, 70)) < dens
        seed = open_ & (rng.random((40, 70)) < 0.01)
        assert np.array_equal(BR.flood(open_, seed), BR.flood_label(open_, seed))
    plane = rng.random((7, 131)) < 0.5
    assert np.array_equal(BR.unpack(BR.pack(plane), 7, 131), plane) and BR.pack(plane).shape == (7 * 3,)
    assert BR.pack(np.ones((1, 65), bool)).tolist() == [2 ** 64 - 1, 1]


# ---- the host's tables -------------------------------------------------------------------------------------------------

def test_balloon_tables_equal_the_restatements_windows():
    p = pkg()
    B = p.balloons
    shapes = [(60, 100), (300, 40), (1024, 512), (1024, 513), (8192, 64), (2731, 192), (50, 70)]
    H, W = 60, 100
    boxes = [np.array([(0, 0, 12, 9), (W - 11, 0, W, 8), (0, H - 9, 13, H), (W - 12, H - 8, W, H), (40, 20, 60, 30), (-10, 5, 15, 14),
                       (W - 8, 5, W + 22, 14), (5, -6, 25, 5), (5, H - 4, 25, H + 7), (-30, 5, -10, 14), (W, 5, W + 20, 14),
                       (10, 10, 10, 20), (30, 20, 10, 5), (0, 0, W, H), (-W, -H, 2 * W, 2 * H), (45, 25, 46, 26)]),
             np.array([(10, 100, 30, 200), (0, 0, 40, 300), (39, 299, 40, 300)]), np.array([(0, 0, 512, 1024), (100, 100, 400, 900)]),
             np.array([(0, 0, 513, 1024)]), np.array([(0, 0, 64, 8192)]), np.array([(0, 0, 192, 2731)]), np.zeros((0, 4), np.int64)]
    for reach, reach_min in ((8, 32), (0, 8), (32, 1024), (3, 9)):
        win, nw, word0, total, too_large = B.balloon_tables(boxes, shapes, reach, reach_min)
        k, at = 0, 0
        for bx, (h, w) in zip(boxes, shapes):
            for b in bx:
                want = BR.window(b, h, w, reach, reach_min)[1]
                wnw, words = BR.n_words(want)
                assert tuple(win[k]) == want and nw[k] == wnw and too_large[k] == (words > BR.MAX_WORDS), (reach, reach_min, b)
                assert word0[k] == at
                at += 0 if words > BR.MAX_WORDS else words
                k += 1
        assert k == len(win) and total == at
    win, nw, word0, total, too_large = B.balloon_tables(boxes, shapes, 8, 32)
    assert too_large.tolist() == [False] * 19 + [False, False, True, False, True]
    assert tuple(win[4]) == (8, 0, 92, 60) and tuple(win[11]) == (0, 0, 0, 0) and nw[11] == 0
    assert B.balloon_tables([], [])[3] == 0
    for bad in (dict(reach=-1), dict(reach=33), dict(reach_min=7), dict(reach_min=1025)):
        with pytest.raises(ValueError):
            B.balloon_tables(boxes, shapes, **bad)


# ---- the Python layer ------------------------------------------------------------------------------------------------------

def test_balloon_regions_argument_checks_need_no_gpu():
    p = pkg()
    B = p.balloons
    page, mask = np.zeros((20, 30, 3), np.uint8), np.zeros((20, 30), np.uint8)
    blk = p.textblock.TextBlock([2, 3, 20, 15], lines=[[[2, 3], [20, 3], [20, 15], [2, 15]]])
    for pg, mk in ((page[:, :, 0], mask), (page.astype(np.int32), mask), (page, mask[:, :29]), (page, mask.astype(bool)),
                   (page, np.zeros((20, 30, 1), np.uint8)), (page[:0], mask[:0])):
        with pytest.raises(ValueError):
            B.balloon_regions([pg], [mk], [[blk]])
    with pytest.raises(ValueError):
        B.balloon_regions([page], [mask, mask], [[blk]])
    with pytest.raises(ValueError):
        B.balloon_regions([page], [mask], [])
    for bad in (dict(grow=-1), dict(grow=9), dict(tol=-1), dict(tol=256), dict(reach=-1), dict(reach=33), dict(reach_min=7),
                dict(reach_min=1025), dict(grow=1.5), dict(tol=True)):
        with pytest.raises(ValueError):
            B.balloon_regions([page], [mask], [[blk]], **bad)
    none = B.balloon_regions([], [], [])                                # no page: nothing to launch
    assert len(none) == 0 and none.index.shape == (0, 2) and none.center.shape == (0, 2) and none.bbox.shape == (0, 4)
    import torch
    if not torch.cuda.is_available():
        with pytest.raises(p._lib.CtdError):
            B.balloon_regions([page], [mask], [[blk]])
        with pytest.raises(p._lib.CtdError):
            B.balloon_regions([page], [mask], [[]])


# ---- ABI -------------------------------------------------------------------------------------------------------------------

def test_balloon_structs_have_the_c_layout():
    """`balloons.JOB_DTYPE` / `ROW_DTYPE` and the `_lib` mirrors against the header, compiled: sizes, every field's offset, the
    constants; the entry point is exported and bound."""
    p = pkg()
    L, B = p._lib, p.balloons
    fields = {"ctd_balloon_job": ("page", "xyxy", "erase_row", "word0"),
              "ctd_balloon_params": ("grow", "tol", "reach", "reach_min", "max_words", "pad_"),
              "ctd_balloon_row": ("status", "area", "bbox", "flags", "n_seed", "sum_x", "sum_y")}
    consts = ("CTD_BALLOON_OK", "CTD_BALLOON_NOT_PLAIN", "CTD_BALLOON_TOO_LARGE", "CTD_BALLOON_MAX_WORDS", "CTD_BALLOON_MAX_REACH",
              "CTD_BALLOON_MIN_REACH_MIN", "CTD_BALLOON_MAX_REACH_MIN", "CTD_BALLOON_CUT_LEFT", "CTD_BALLOON_CUT_TOP",
              "CTD_BALLOON_CUT_RIGHT", "CTD_BALLOON_CUT_BOTTOM", "CTD_ABI_VERSION")
    vals = compiled_flat(fields, consts)
    mirrors = {"ctd_balloon_job": (L.CtdBalloonJob, B.JOB_DTYPE, 32), "ctd_balloon_params": (L.CtdBalloonParams, None, 32),
               "ctd_balloon_row": (L.CtdBalloonRow, B.ROW_DTYPE, 48)}
    k = 0
    for s, fs in fields.items():
        ct, dt, size = mirrors[s]
        assert vals[k] == C.sizeof(ct) == size and (dt is None or dt.itemsize == size), s
        assert vals[k + 1:k + 1 + len(fs)] == [getattr(ct, f).offset for f in fs], s
        assert [f for f, _ in ct._fields_] == list(fs)
        if dt is not None:
            assert vals[k + 1:k + 1 + len(fs)] == [dt.fields[f][1] for f in fs] and dt.names == fs, s
        k += 1 + len(fs)
    assert vals[k:] == [L.BALLOON_OK, L.BALLOON_NOT_PLAIN, L.BALLOON_TOO_LARGE, L.BALLOON_MAX_WORDS, L.BALLOON_MAX_REACH,
                        L.BALLOON_MIN_REACH_MIN, L.BALLOON_MAX_REACH_MIN, L.BALLOON_CUT_LEFT, L.BALLOON_CUT_TOP, L.BALLOON_CUT_RIGHT,
                        L.BALLOON_CUT_BOTTOM, L.ABI_VERSION]
    assert vals[k:k + 11] == [BR.OK, BR.NOT_PLAIN, BR.TOO_LARGE, BR.MAX_WORDS, BR.MAX_REACH, BR.MIN_REACH_MIN, BR.MAX_REACH_MIN,
                              BR.CUT_LEFT, BR.CUT_TOP, BR.CUT_RIGHT, BR.CUT_BOTTOM]
    assert "ctd_balloon_regions" in L.SYMBOLS and hasattr(L.lib(), "ctd_balloon_regions")
    # the entry point refuses parameters outside their bounds before anything else (nothing is launched: no GPU is needed)
    lib = L.lib()
    for vals in ((-1, 12, 8, 32, 0), (9, 12, 8, 32, 0), (2, -1, 8, 32, 0), (2, 256, 8, 32, 0), (2, 12, -1, 32, 0), (2, 12, 33, 32, 0),
                 (2, 12, 8, 7, 0), (2, 12, 8, 1025, 0), (2, 12, 8, 32, -1), (2, 12, 8, 32, 8193)):
        prm = L.CtdBalloonParams(*vals)
        assert lib.ctd_balloon_regions(8, 1, 8, 1, 8, C.byref(prm), 8, 8, None) != L.OK, vals
    prm = L.CtdBalloonParams(2, 12, 8, 32, 0)
    assert lib.ctd_balloon_regions(8, -1, 8, 1, 8, C.byref(prm), 8, 8, None) != L.OK
    assert lib.ctd_balloon_regions(8, 1, 8, 0, 8, C.byref(prm), 8, 8, None) != L.OK          # blocks without pages
    assert lib.ctd_balloon_regions(8, 1, 8, 1, 8, None, 8, 8, None) != L.OK
    assert lib.ctd_balloon_regions(None, 1, 8, 1, 8, C.byref(prm), 8, 8, None) != L.OK
    assert lib.ctd_balloon_regions(None, 0, None, 0, None, C.byref(prm), None, None, None) == L.OK   # nothing to do
