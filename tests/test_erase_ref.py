"""Erasing text without a GPU: the rule's own promises on its numpy restatement (tests/erase_ref.py) -- known answers on flat
pages, both sides of every boundary of the decision -- argument checks of `erase.erase_text`, and the layout of the ABI
structs against the header.  The kernels themselves are compared with the restatement in tests/test_gpu_erase.py."""
import ctypes as C

import numpy as np
import pytest

import erase_ref as R
from c_layout import compiled_flat
from conftest import pkg


# ---- the rule ----------------------------------------------------------------------------------------------------------

def test_a_two_colour_page_comes_back_as_one_colour():
    for page, mask, boxes, balloon in R.flat_cases():
        rows, out, rest = R.erase_page(page, mask, boxes)
        assert rows[0]["status"] == R.PLAIN and rows[0]["med"] == balloon, rows
        assert rows[0]["cnt"] == [rows[0]["n_ring"]] * 3 and rows[0]["n_ring"] >= 16 and rows[0]["n_fill"] > int((mask != 0).sum())
        assert (out == np.array(balloon, np.uint8)).all() and not rest.any()


def one_bar(w=30, h=4, balloon=200, shape=(40, 70), at=(20, 18)):
    """A grey page with ONE w x h bar of text at `at`: (page, mask, box, ring mask).  With g = 2 and r = 4 and the bar more
    than 6 pixels from the page's edges the ring is the 6-dilation minus the 2-dilation of a rectangle:
    (w + 12)(h + 12) - (w + 4)(h + 4) = 8 (w + h + 16) pixels."""
    page = np.full(shape + (3,), balloon, np.uint8)
    mask = np.zeros(shape, np.uint8)
    x, y = at
    mask[y:y + h, x:x + w] = 255
    page[mask != 0] = 0
    ring = np.zeros(shape, bool)
    ring[y - 6:y + h + 6, x - 6:x + w + 6] = True
    ring[y - 2:y + h + 2, x - 2:x + w + 2] = False
    assert int(ring.sum()) == 8 * (w + h + 16)
    return page, mask, (x, y, x + w, y + h), ring


def _spoil(page, ring, k, value, channel):
    """k ring pixels (the first in raster order) of one channel set to `value`."""
    out = page.copy()
    ys, xs = np.nonzero(ring)
    out[ys[:k], xs[:k], channel] = value
    return out


def test_both_sides_of_the_fifteen_sixteenths():
    page, mask, box, ring = one_bar()                              # 400 ring pixels: 15/16 of them are 375
    for channel in range(3):
        row = R.erase_page(_spoil(page, ring, 25, 0, channel), mask, [box])[0][0]
        want = [400, 400, 400]
        want[channel] = 375
        assert row["status"] == R.PLAIN and row["n_ring"] == 400 and row["cnt"] == want and row["med"] == [200] * 3, row
        rows, out, rest = R.erase_page(_spoil(page, ring, 26, 0, channel), mask, [box])
        want[channel] = 374
        assert rows[0]["status"] == R.TEXTURED and rows[0]["cnt"] == want and rows[0]["n_fill"] == 34 * 8
        # a textured block is left alone and its fill region goes to the inpainter
        assert np.array_equal(out, _spoil(page, ring, 26, 0, channel))
        assert int((rest != 0).sum()) == 34 * 8 and rest[16:24, 18:52].all()


def test_a_deviation_of_tol_counts_and_one_more_does_not():
    page, mask, box, ring = one_bar()
    for sign in (1, -1):
        at = R.erase_page(_spoil(page, ring, 26, 200 + sign * 12, 1), mask, [box])[0][0]
        beyond = R.erase_page(_spoil(page, ring, 26, 200 + sign * 13, 1), mask, [box])[0][0]
        assert at["status"] == R.PLAIN and at["cnt"] == [400, 400, 400] and at["med"] == [200] * 3
        assert beyond["status"] == R.TEXTURED and beyond["cnt"] == [400, 374, 400]
    zero = R.erase_page(_spoil(page, ring, 26, 201, 1), mask, [box], tol=0)[0][0]
    assert zero["status"] == R.TEXTURED and zero["cnt"] == [400, 374, 400]
    assert R.erase_page(_spoil(page, ring, 25, 201, 1), mask, [box], tol=0)[0][0]["status"] == R.PLAIN
    # the range is cut at the ends of the value scale
    white = R.erase_page(_spoil(one_bar(balloon=250)[0], ring, 26, 255, 2), mask, [box])[0][0]
    assert white["status"] == R.PLAIN and white["med"] == [250] * 3


def test_min_ring_is_the_first_count_with_a_decision():
    page, mask, box, ring = one_bar()
    rows, out, rest = R.erase_page(page, mask, [box], min_ring=400)
    assert rows[0]["status"] == R.PLAIN and rows[0]["n_ring"] == 400 and not rest.any()
    rows, out, rest = R.erase_page(page, mask, [box], min_ring=401)
    assert rows[0]["status"] == R.NO_RING and rows[0]["n_ring"] == 400 and rows[0]["med"] == [200] * 3 and rows[0]["cnt"] == [400] * 3
    assert np.array_equal(out, page) and int((rest != 0).sum()) == rows[0]["n_fill"] == 34 * 8


def test_the_median_is_the_lower_one():
    page, mask, box, ring = one_bar(balloon=110)
    row = R.erase_page(_spoil(page, ring, 200, 100, 0), mask, [box])[0][0]       # 200 x 100 and 200 x 110: the lower of the two
    assert row["med"] == [100, 110, 110] and row["status"] == R.PLAIN and row["cnt"] == [400] * 3
    row = R.erase_page(_spoil(page, ring, 199, 100, 0), mask, [box])[0][0]
    assert row["med"] == [110, 110, 110]
    rows, out, _ = R.erase_page(_spoil(page, ring, 200, 100, 0), mask, [box])
    assert out[19, 30].tolist() == [100, 110, 110]                              # the fill is the median


def overlapping_pair():
    """Two bars three pixels apart on backgrounds of two near colours (both within tol of each other): both blocks are PLAIN,
    with different medians, and their fill regions share the column between them."""
    page = np.full((40, 100, 3), 100, np.uint8)
    page[:, 42:] = 108
    mask = np.zeros((40, 100), np.uint8)
    mask[15:20, 10:40] = 255
    mask[15:20, 43:73] = 255
    page[mask != 0] = 0
    return page, mask, [(10, 15, 40, 20), (43, 15, 73, 20)]


def test_the_higher_index_wins_where_two_plain_blocks_overlap():
    page, mask, boxes = overlapping_pair()
    rows, out, rest = R.erase_page(page, mask, boxes)
    assert [r["status"] for r in rows] == [R.PLAIN, R.PLAIN] and rows[0]["med"] == [100] * 3 and rows[1]["med"] == [108] * 3
    assert (out[13:22, 8:41] == 100).all() and (out[13:22, 41:75] == 108).all() and not rest.any()
    rows, out, rest = R.erase_page(page, mask, boxes[::-1])
    assert (out[13:22, 8:42] == 100).all() and (out[13:22, 42:75] == 108).all()
    assert (out[:13] == page[:13]).all() and (out[22:] == page[22:]).all()


def test_rest_keeps_the_mask_outside_every_block_and_the_other_statuses():
    page, mask, box, ring = one_bar()
    mask[2:5, 60:66] = 7                                           # text no block claims, far from the bar
    rows, out, rest = R.erase_page(page, mask, [box, (0, 30, 12, 40), (-20, -20, 0, 5), (70, 0, 90, 9), (5, 5, 5, 30),
                                                (0, 0, R.MAX_COORD + 1, 10)])
    assert [r["status"] for r in rows] == [R.PLAIN, R.NO_MASK, R.EMPTY, R.EMPTY, R.EMPTY, R.TOO_LARGE]
    assert all(r == dict(status=r["status"], n_fill=0, n_ring=0, cnt=[0] * 3, med=[0] * 3) for r in rows[1:])
    want = np.zeros_like(mask)
    want[2:5, 60:66] = 255
    assert np.array_equal(rest, want)
    assert (out[16:24, 18:52] == 200).all() and np.array_equal(out[:10], page[:10])
    # at the coordinate cap a box is computed; the pixel cap is on the box grown by g + r
    assert R.erase_page(page, mask, [(0, 0, R.MAX_COORD, 40)])[0][0]["status"] == R.PLAIN
    assert R.box_status((0, 0, 4096 - 12, 4096 - 12), 5000, 5000, 2, 4) == (None, (0, 0, 4084, 4084))
    assert R.box_status((0, 0, 4096 - 12, 4096 - 11), 5000, 5000, 2, 4)[0] == R.TOO_LARGE
    # limits of the rule: a gradient is TEXTURED; a ring swallowed by the neighbours' text is NO_RING
    grad = page.copy()
    grad[:, :, :] = np.where(mask[..., None] != 0, 0, (np.arange(70) * 3)[None, :, None]).astype(np.uint8)
    assert R.erase_page(grad, mask, [box])[0][0]["status"] == R.TEXTURED
    crowded = np.zeros((40, 70), np.uint8)
    crowded[::4, :] = 255                                          # a text row every 4 pixels: everything is within 2 of text
    row = R.erase_page(page, crowded, [(20, 16, 50, 17)])[0][0]
    assert row["status"] == R.NO_RING and row["n_ring"] == 0 and row["n_fill"] == 34 * 5
    for bad in (dict(grow=-1), dict(grow=9), dict(ring=0), dict(ring=17), dict(tol=-1), dict(tol=256), dict(min_ring=0)):
        with pytest.raises(ValueError):
            R.erase_page(page, mask, [box], **bad)


def test_dilation_is_the_chebyshev_ball_clipped_to_the_page():
    s = np.zeros((9, 12), bool)
    s[0, 0] = s[8, 11] = s[4, 6] = True
    for k in (0, 1, 3, 20):
        ys, xs = np.mgrid[0:9, 0:12]
        want = np.zeros_like(s)
        for y, x in zip(*np.nonzero(s)):
            want |= np.maximum(abs(ys - y), abs(xs - x)) <= k
        assert np.array_equal(R.dilate(s, k), want), k


# ---- the Python layer ------------------------------------------------------------------------------------------------------

def test_erase_text_argument_checks_need_no_gpu():
    p = pkg()
    E = p.erase
    page, mask = np.zeros((20, 30, 3), np.uint8), np.zeros((20, 30), np.uint8)
    blk = p.textblock.TextBlock([2, 3, 20, 15], lines=[[[2, 3], [20, 3], [20, 15], [2, 15]]])
    for pg, mk in ((page[:, :, 0], mask), (page.astype(np.int32), mask), (page, mask[:, :29]), (page, mask.astype(bool)),
                   (np.zeros((20, 30, 1), np.uint8), mask), (page, np.zeros((20, 30, 1), np.uint8)), (page[:0], mask[:0])):
        with pytest.raises(ValueError):
            E.erase_text([pg], [mk], [[blk]])
    with pytest.raises(ValueError):
        E.erase_text([page], [mask, mask], [[blk]])
    with pytest.raises(ValueError):
        E.erase_text([page], [mask], [])
    for bad in (dict(grow=-1), dict(grow=9), dict(ring=0), dict(ring=17), dict(tol=-1), dict(tol=256), dict(min_ring=0),
                dict(grow=1.5), dict(tol=True)):
        with pytest.raises(ValueError):
            E.erase_text([page], [mask], [[blk]], **bad)
    none = E.erase_text([], [], [])                                     # no page: nothing to launch
    assert len(none) == 0 and none.pages == [] and none.rest == [] and none.fill.shape == (0, 3) and none.index.shape == (0, 2)
    import torch
    if not torch.cuda.is_available():
        with pytest.raises(p._lib.CtdError):
            E.erase_text([page], [mask], [[blk]])
    # the tables: blocks of a page are consecutive rows, tiles are counted per page
    jobs, block0, counts, tile0, n_tiles = E.erase_tables([np.array([[1, 2, 3, 4], [5, 6, 7, 8]]), np.zeros((0, 4)), np.array([[9, 9, 9, 9]])],
                                                          [(33, 64), (1, 65), (32, 1)])
    assert jobs["page"].tolist() == [0, 0, 2] and jobs["xyxy"].tolist() == [[1, 2, 3, 4], [5, 6, 7, 8], [9, 9, 9, 9]]
    assert block0.tolist() == [0, 2, 2] and counts.tolist() == [2, 0, 1] and tile0.tolist() == [0, 2, 4] and n_tiles == 5


# ---- ABI -------------------------------------------------------------------------------------------------------------------

def test_erase_structs_have_the_c_layout():
    """`erase.JOB_DTYPE` / `PAGE_DTYPE` / `ROW_DTYPE` and the `_lib` mirrors against the header, compiled: sizes and every
    field's offset; the constants."""
    p = pkg()
    L, E = p._lib, p.erase
    fields = {"ctd_erase_job": ("page", "xyxy", "pad_"),
              "ctd_erase_page": ("page_dev", "mask_dev", "out_dev", "rest_dev", "H", "W", "pitch", "mask_pitch", "out_pitch",
                                 "rest_pitch", "block0", "n_blocks", "tile0", "pad_"),
              "ctd_erase_params": ("grow", "ring", "tol", "min_ring", "n_tiles", "pad_"),
              "ctd_erase_row": ("status", "n_fill", "n_ring", "cnt", "med", "pad_")}
    consts = ("CTD_ERASE_PLAIN", "CTD_ERASE_TEXTURED", "CTD_ERASE_NO_RING", "CTD_ERASE_NO_MASK", "CTD_ERASE_EMPTY",
              "CTD_ERASE_TOO_LARGE", "CTD_ERASE_MAX_PIXELS", "CTD_ERASE_MAX_COORD", "CTD_ERASE_MAX_GROW", "CTD_ERASE_MAX_RING",
              "CTD_ERASE_TILE_W", "CTD_ERASE_TILE_H", "CTD_ABI_VERSION")
    vals = compiled_flat(fields, consts)
    mirrors = {"ctd_erase_job": (L.CtdEraseJob, E.JOB_DTYPE, 32), "ctd_erase_page": (L.CtdErasePage, E.PAGE_DTYPE, 72),
               "ctd_erase_params": (L.CtdEraseParams, None, 32), "ctd_erase_row": (L.CtdEraseRow, E.ROW_DTYPE, 32)}
    k = 0
    for s, fs in fields.items():
        ct, dt, size = mirrors[s]
        assert vals[k] == C.sizeof(ct) == size and (dt is None or dt.itemsize == size), s
        assert vals[k + 1:k + 1 + len(fs)] == [getattr(ct, f).offset for f in fs], s
        assert [f for f, _ in ct._fields_] == list(fs)
        if dt is not None:
            assert vals[k + 1:k + 1 + len(fs)] == [dt.fields[f][1] for f in fs] and dt.names == fs, s
        k += 1 + len(fs)
    assert vals[k:] == [L.ERASE_PLAIN, L.ERASE_TEXTURED, L.ERASE_NO_RING, L.ERASE_NO_MASK, L.ERASE_EMPTY, L.ERASE_TOO_LARGE,
                        L.ERASE_MAX_PIXELS, L.ERASE_MAX_COORD, L.ERASE_MAX_GROW, L.ERASE_MAX_RING, L.ERASE_TILE_W, L.ERASE_TILE_H,
                        L.ABI_VERSION]
    assert vals[k:k + 10] == [R.PLAIN, R.TEXTURED, R.NO_RING, R.NO_MASK, R.EMPTY, R.TOO_LARGE, R.MAX_PIXELS, R.MAX_COORD, R.MAX_GROW,
                              R.MAX_RING]
    assert "ctd_erase_text" in L.SYMBOLS and hasattr(L.lib(), "ctd_erase_text")
