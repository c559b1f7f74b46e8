"""The dual labelling on row runs as tests/ccl_runs_emul.py spells it out (the kernels of `launch_ccl_dual` in numpy) against
the oracle's `connected_components_with_stats`, 8-connected for the foreground and 4-connected for the background: label
plane, counts, statistics and first pixels, exactly.  Widths 1..131 put a page in one word, in whole words and in a partial
last word; heights 1..65 put a band boundary nowhere, after the last row and inside the page.  The single-class form
(`launch_ccl`: conn 8 keeps the foreground class, conn 4 the background class of the flipped page) on the same pages against
`connected_components_with_stats(img, conn)`.  No GPU is needed."""
import os
import re

import numpy as np
import pytest

import ccl_runs_emul as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def check_page(name, fg, cap=E.RB_CAP, max_labels=None):
    t = E.label_runs(fg, cap)
    ref = E.reference(fg)
    cap_l = max_labels if max_labels is not None else max(1, t["n_f"], t["n_b"])
    plane, st, first, seg = E.paint(t, cap_l)
    for sign, n in ((1, t["n_f"]), (-1, t["n_b"])):
        nref, lref, sref = ref[sign]
        assert n == nref, f"{name}: {n} components of class {sign}, the oracle has {nref}"
        np.testing.assert_array_equal(np.maximum(sign * plane, 0), lref, err_msg=name)
        k = min(n, cap_l)
        np.testing.assert_array_equal(st[sign][:k], sref[:k], err_msg=name)
        flat = lref.ravel()
        for l in range(k):                                            # the component's first pixel in raster order
            assert first[sign][l] == int(np.argmax(flat == l + 1)), f"{name}: first pixel of {sign * (l + 1)}"
        assert (st[sign][k:] == -1).all() and (first[sign][k:] == -1).all(), f"{name}: rows beyond the labels that exist"
    # run ids are in raster order of the runs' first pixels, and a root is its component's smallest run
    assert all(t["rparent"][r] <= r for r in range(t["R"])), name
    return t


def test_the_emulation_has_the_kernels_constants():
    src = open(os.path.join(ROOT, "comic-text-detector_amd", "csrc", "kernels_post.hip")).read()
    assert int(re.search(r"constexpr int RB_ROWS = (\d+);", src).group(1)) == E.RB_ROWS
    assert int(re.search(r"constexpr int RB_CAP = (\d+);", src).group(1)) == E.RB_CAP


@pytest.mark.parametrize("H", E.HEIGHTS)
def test_every_kind_of_page_at_every_width(H):
    for (h, W), pages in E.small_calls():
        if h != H:
            continue
        for name, fg in pages:
            check_page(f"{name}, {H} x {W}", fg)


def test_the_pages_hold_what_they_are_for():
    """Every pixel a run on the checkerboard; diagonal pairs join for the foreground and not for the background; rows that
    are one run across all words."""
    pages = dict(E.pages_for(65, 131))
    t = E.label_runs(pages["checkerboard"])
    assert t["R"] == 65 * 131 and t["n_f"] == 1 and t["n_b"] == (65 * 131) // 2
    t = E.label_runs(pages["diagonal pairs"])
    assert t["n_f"] == 8 and pages["diagonal pairs"].sum() == 16                # eight pairs, each one component
    t = E.label_runs(pages["diagonal pairs of background"])
    assert t["n_b"] == 16                                                       # ... and two for the background
    t = E.label_runs(pages["rows"])
    assert t["R"] == 65 and t["n_f"] == 33 and t["n_b"] == 32 and all(popc <= 1 for popc in map(E.popc, t["starts"]))


def test_small_tables_send_bands_through_global_memory():
    """The same pages with a table of 64 runs: most bands are over it, the result is the same."""
    n_over = 0
    for H, W in ((65, 131), (33, 65), (65, 33)):
        for name, fg in E.pages_for(H, W):
            t = check_page(f"{name}, {H} x {W}, table of 64", fg, cap=64)
            n_over += len(t["over"])
            under = E.label_runs(fg)
            assert not under["over"] and under["rparent"] == t["rparent"] and under["rlabel"] == t["rlabel"], name
    assert n_over > 50


def test_a_band_over_the_capacity_between_two_under_it():
    fg = E.over_capacity_page(W=1024)
    t = check_page("alternating band between sparse bands", fg)
    assert t["over"] == [1]
    assert t["base"][64 * 32] - t["base"][32 * 32] == 32 * 1024 > E.RB_CAP


def test_max_labels_below_the_component_count_drops_the_rows_beyond():
    fg = E.noise(33, 65, 0.3, 9)
    t = E.label_runs(fg)
    assert min(t["n_f"], t["n_b"]) > 7
    check_page("noise, max_labels 7", fg, max_labels=7)


# ---------------------------------------------------------------------------------------------------------------------------
# launch_ccl: one class of the same engine
# ---------------------------------------------------------------------------------------------------------------------------
def check_single(name, fg, conn, cap=E.RB_CAP, max_labels=None, other=0):
    from oracle import postproc_ref as R
    nref, lref, sref = R.connected_components_with_stats(fg.astype(np.uint8) * 255, conn)
    nref, sref = nref - 1, sref[1:]
    cap_l = max_labels if max_labels is not None else max(1, nref)
    t, n, plane, st, first = E.label_single(fg, conn, cap_l, other, cap)
    name = f"{name}, conn {conn}"
    assert n == nref, f"{name}: {n} components, the oracle has {nref}"
    np.testing.assert_array_equal(plane, np.where(lref > 0, lref, other), err_msg=name)
    k = min(n, cap_l)
    np.testing.assert_array_equal(st[:k], sref[:k], err_msg=name)
    flat = lref.ravel()
    for l in range(k):
        assert first[l] == int(np.argmax(flat == l + 1)), f"{name}: first pixel of {l + 1}"
    assert (st[k:] == -1).all() and (first[k:] == -1).all(), f"{name}: rows beyond the labels that exist"
    return t


@pytest.mark.parametrize("conn", (4, 8))
@pytest.mark.parametrize("H", E.HEIGHTS)
def test_one_class_of_every_kind_of_page_at_every_width(H, conn):
    for (h, W), pages in E.small_calls():
        if h != H:
            continue
        for i, (name, fg) in enumerate(pages):
            check_single(f"{name}, {H} x {W}", fg, conn, other=-(i % 2))     # both background values of the plane


@pytest.mark.parametrize("conn", (4, 8))
def test_one_class_with_small_tables_and_with_a_band_over_the_capacity(conn):
    n_over = 0
    for H, W in ((65, 131), (33, 65), (65, 33)):
        for name, fg in E.pages_for(H, W):
            n_over += len(check_single(f"{name}, {H} x {W}, table of 64", fg, conn, cap=64)["over"])
    assert n_over > 50
    t = check_single("alternating band between sparse bands", E.over_capacity_page(W=1024), conn, other=-1)
    assert t["over"] == [1]


@pytest.mark.parametrize("conn", (4, 8))
@pytest.mark.parametrize("other", (0, -1))
def test_one_class_with_max_labels_below_the_component_count(conn, other):
    fg = E.noise(33, 65, 0.3, 9)
    t, n, *_ = E.label_single(fg, conn, 7)
    assert n > 7
    check_single("noise, max_labels 7", fg, conn, max_labels=7, other=other)
