"""-m gpu: seeded sweeps of the post-network half of the step -- NMS, the DB stage, the labelling kernels, the resize kernel,
the whole native tail at B = 32, pages of different sizes in one batch, and the two host decisions that tie -- each EXACT against
the oracle (oracle/postproc_ref.py, oracle/cv_ref.py, scipy).  The cases come from tests/sweep_cases.py (the generators of
scripts/gpu_*_stress.py, which run thousands of them by hand); tests/test_sweep_cases.py checks without a GPU that the ranges are
not vacuous and that every compare helper below reports a perturbed case.

A sweep collects mismatches (`collect_mismatches`: AssertionError only) and lists every one in its assertion message; any other
exception -- `CtdError`, a HIP error through torch, a timeout -- ends the test at once, so nothing is launched after a GPU error."""
import copy

import numpy as np
import pytest
import torch

import sweep_cases as S
from conftest import checkpoint, pkg
from oracle import cv_ref as cv
from oracle import postproc_ref as R
from test_post_host import blocks_equal

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------- compare helpers (no GPU)

def collect_mismatches(cases, compare):
    """`cases` yields (description, got, ref); returns "description: first difference" of every case on which
    `compare(got, ref)` raises AssertionError.  Anything else that `cases` or `compare` raises passes through: no case is
    produced (nothing is launched) after it."""
    bad = []
    for what, got, ref in cases:
        try:
            compare(got, ref)
        except AssertionError as e:
            bad.append(f"{what}: {' '.join(str(e).split())[:240]}")
    return bad


def report(name, n_cases, bad):
    print(f"\n{name}: {n_cases} cases, {len(bad)} mismatches")
    assert not bad, f"{name}: {len(bad)} of {n_cases} cases differ from the oracle:\n" + "\n".join(bad)


def sweep(name, n_cases, cases, compare):
    """Runs a whole sweep: every case of `cases` through `compare`, exactly `n_cases` of them, every mismatch listed."""
    seen = []

    def counted():
        for case in cases:
            seen.append(case[0])
            yield case
    bad = collect_mismatches(counted(), compare)
    assert len(seen) == n_cases, f"{name}: {len(seen)} cases ran, {n_cases} expected"
    report(name, n_cases, bad)


def compare_detections(got, ref):
    """NMS: lists (one entry per page) of (n,6) [xyxy, conf, cls] f32 -- counts first, then bit for bit in order."""
    assert len(got) == len(ref), f"pages: {len(got)} vs {len(ref)}"
    for i, (g, r) in enumerate(zip(got, ref)):
        assert len(g) == len(r), f"page {i}: {len(g)} vs {len(r)} detections"
        np.testing.assert_array_equal(g, r, err_msg=f"page {i}: detections")


def compare_boxes(got, ref):
    """DB stage: (boxes (n,4,2), scores (n,)) -- boxes equal, scores to 1e-6 (a float32 mean; tests/test_post_host.py)."""
    (gb, gs), (rb, rs) = got, ref
    assert len(gb) == len(rb), f"{len(gb)} vs {len(rb)} boxes"
    np.testing.assert_array_equal(np.asarray(gb).reshape(len(rb), 4, 2), np.asarray(rb).reshape(len(rb), 4, 2), err_msg="boxes")
    np.testing.assert_allclose(np.asarray(gs), np.asarray(rs), rtol=0, atol=1e-6, err_msg="scores")


def compare_labelling(got, ref):
    """Labelling: (n, labels (H,W), stats (n,5) [x,y,w,h,area], first pixels (n,) or None) against
    `R.connected_components_with_stats` = (nref incl. background, labels, stats incl. background row)."""
    n, lab, stats, firsts = got
    nref, lref, sref = ref
    assert int(n) == nref - 1, f"{int(n)} vs {nref - 1} components"
    np.testing.assert_array_equal(lab, lref, err_msg="labels")
    np.testing.assert_array_equal(np.asarray(stats)[: nref - 1], sref[1:], err_msg="stats")
    if firsts is not None:
        flat = lref.ravel()
        firsts = np.asarray(firsts)[: nref - 1]
        assert np.array_equal(flat[firsts], np.arange(1, nref)), "first pixels: not one of every component"
        assert np.array_equal(firsts, np.sort(firsts)) and all(flat[f] not in flat[:f] for f in firsts[:50]), "first pixels: not the first"


def compare_images(got, ref):
    assert got.shape == ref.shape, f"shape {got.shape} vs {ref.shape}"
    np.testing.assert_array_equal(got, ref, err_msg="pixels")


def compare_tail(got, ref):
    """(mask, refined mask, blocks) of the native tail against `R.detector_tail`: masks bit for bit, blocks by `blocks_equal`
    (box, lines in order, language, direction, angle, font size)."""
    np.testing.assert_array_equal(got[0], ref[0], err_msg="mask")
    try:
        blocks_equal(got[2], ref[2])
    except AssertionError as e:
        raise AssertionError(f"blocks ({len(got[2])} vs {len(ref[2])}): {e}") from None
    np.testing.assert_array_equal(got[1], ref[1], err_msg="refined mask")


def compare_refine_decisions(got, ref):
    """(top colours list, Otsu threshold or None)."""
    assert len(got[0]) == len(ref[0]), f"colours: {list(got[0])} vs {list(ref[0])}"
    np.testing.assert_array_equal(np.asarray(got[0], np.float64), np.asarray(ref[0], np.float64), err_msg="colours")
    assert got[1] == ref[1], f"otsu: {got[1]} vs {ref[1]}"


def compare_groups(got, ref):
    from test_reference_pin import same_blocks
    try:
        same_blocks(got, ref)
    except AssertionError as e:
        raise AssertionError(f"blocks ({len(got)} vs {len(ref)}): {e}") from None


def oracle_labelling(img_u8, conn):
    return R.connected_components_with_stats(img_u8, conn)


def oracle_refine_decisions(px):
    counts, edges = np.histogram(px, bins=255)
    return R.get_topk_color(edges, counts, k=3, color_var=10), (cv.otsu_threshold_value(px) if len(px) else None)


def oracle_resize(img, dst_hw, canvas):
    ref = cv.resize_linear_u8(img, (dst_hw[1], dst_hw[0]))
    if canvas is None:
        return ref
    out = np.zeros(tuple(canvas) + ref.shape[2:], np.uint8)
    out[: dst_hw[0], : dst_hw[1]] = ref
    return out


def oracle_tail(case, size, keep, dw=0, dh=0):
    """`R.detector_tail` on a case of `S.tail_case` / `S.tail_batch32` (dw = dh = 0) or `S.letterbox_tail_case`."""
    page, bt, mask, lines_map = case
    return R.detector_tail(page, bt, mask, lines_map, input_size=(size, size), dw=dw, dh=dh,
                           refine_mode=1 if keep else 0, keep_undetected_mask=keep)


# ------------------------------------------------------------------------------------------------------------------ sweeps

def test_nms_sweep():
    """100 cases of `S.nms_case`; every 4th with other thresholds than the detector's 0.4 / 0.35 / 300, two on 32 pages."""
    p = pkg()

    def cases():
        for case, b, (conf, iou, max_det), what in S.nms_sweep():
            dets, counts = p.backend.nms(torch.from_numpy(b).cuda(), conf, iou, max_det)
            torch.cuda.synchronize()
            dets, counts = dets.cpu().numpy(), counts.cpu().numpy()
            yield what, [dets[i, : int(counts[i])] for i in range(len(b))], R.non_max_suppression(b, conf, iou, max_det)
    sweep("nms sweep", 100, cases(), compare_detections)


def test_db_stage_sweep():
    """200 maps of `S.db_map` that are not text-like, the last 24 in calls on 8 maps of one size (batch-wide labelling + tables)."""
    rep = pkg().postproc.SegRepresenter()

    def cases():
        for call in S.db_sweep():
            t = torch.from_numpy(np.stack([pr for _, pr, _ in call])).cuda()
            boxes, scores = rep(t, (t > 0.3).to(torch.uint8))
            for i, (case, pr, what) in enumerate(call):
                H, W = pr.shape
                yield f"{what} ({len(call)} maps in the call)", (boxes[i], scores[i]), R.boxes_from_bitmap(pr, pr > 0.3, W, H)
    sweep("db stage sweep", 200, cases(), compare_boxes)


def test_ccl_sweep():
    """100 images x (4-connected, 8-connected, dual), shapes 1 x 1, 1 x N, N x 1 and 31 / 32 / 33 a side forced first."""
    bk = pkg().backend
    cap = 1 << 17

    def cases():
        for case, img, what in S.ccl_sweep():
            u8 = img.astype(np.uint8) * 255
            dev = torch.from_numpy(u8).cuda()
            refs = {8: oracle_labelling(u8, 8), 4: oracle_labelling(u8, 4), -4: oracle_labelling(255 - u8, 4)}
            for conn in (8, 4):
                lab, n, stats = bk.connected_components(dev, 0, conn, max_labels=cap)
                yield f"{what} conn {conn}", (int(n[0]), lab[0].cpu().numpy(), stats[0].cpu().numpy(), None), refs[conn]
            lab, (nf, nb), (sf, sb), (ff, fb) = bk.connected_components_dual(dev, 0, max_labels=cap)
            lab = lab[0].cpu().numpy()
            yield f"{what} dual foreground", (int(nf[0]), np.maximum(lab, 0), sf[0].cpu().numpy(), ff[0].cpu().numpy()), refs[8]
            yield f"{what} dual background", (int(nb[0]), np.maximum(-lab, 0), sb[0].cpu().numpy(), fb[0].cpu().numpy()), refs[-4]
    sweep("ccl sweep", 400, cases(), compare_labelling)


def test_resize_sweep():
    """150 cases of `S.resize_case`; 1 x 1 sources, 1-pixel destinations, equal size and > 16x up / down forced first."""
    bk = pkg().backend

    def cases():
        for case, img, dst_hw, canvas, what in S.resize_sweep():
            got = bk.resize_linear_u8(torch.from_numpy(img).cuda(), dst_hw, canvas).cpu().numpy()
            yield what, got, oracle_resize(img, dst_hw, canvas)
    sweep("resize sweep", 150, cases(), compare_images)


def test_tail_on_32_different_pages_per_call():
    """One native tail call on 32 DIFFERENT pages (seeds 7000 .. 7063 at 512), one call per tail configuration: the batch-wide
    GPU stages and the one-thread-per-page host stages at the benchmark's batch size, page by page against `R.detector_tail`."""
    from test_gpu_e2e import detector
    size = 512
    det = detector(size)

    def cases():
        for call in range(2):
            keep = bool(call & 1)
            pages = S.tail_batch32(call, 7000, size)
            prob = torch.from_numpy(np.stack([c[3] for c in pages])).cuda()
            got = det.tail_batch([c[0] for c in pages], torch.from_numpy(np.concatenate([c[1] for c in pages])).cuda(),
                                 torch.from_numpy(np.stack([c[2] for c in pages])).cuda(), prob, (prob > 0.3).to(torch.uint8),
                                 refine_mode=1 if keep else 0, keep_undetected_mask=keep)
            for i, c in enumerate(pages):
                yield c[6], got[i], oracle_tail((c[0], c[1], c[4], c[5]), size, keep)
    sweep("tail on 32 different pages per call", 64, cases(), compare_tail)


def test_mixed_size_batch_equals_single_calls():
    """`TextDetector.detect_batch` on 2 .. 6 pages of DIFFERENT sizes (letterbox per page, one forward, per-page inverse mapping)
    against the same detector one page at a time: masks, refined masks and blocks identical."""
    det = pkg().detector.TextDetector(checkpoint(), input_size=256, device="cuda", precision="fp32s")
    n_pages = []

    def cases():
        for case, pages, mode, keep in S.mixed_size_batches():
            batch = det.detect_batch(pages, mode, keep)
            n_pages.append(len(pages))
            for i, pg in enumerate(pages):
                yield f"batch {case} page {i} {pg.shape} mode {mode} keep {keep}", batch[i], det(pg, mode, keep)
    sweep("mixed-size batch against single calls", sum(len(pages) for _, pages, _, _ in S.mixed_size_batches()), cases(), compare_tail)
    assert len(n_pages) == 6 and all(2 <= n <= 6 for n in n_pages)


def test_refine_decisions_on_tied_histograms():
    """`ctd_topk_colors` and `ctd_otsu_from_hist` (csrc/host_refine.cpp; no GPU work) on 200 histograms that TIE, on THIS host:
    the colour pick is an argsort of the bin counts with numpy's default kind, which csrc/np_dispatch.h takes from numpy at run
    time and replaces by a stable sort where it cannot -- on the machine the product is measured on, this test is what notices."""
    lib = pkg()._lib.lib()

    def cases():
        for case, px, what in S.tied_sweep():
            hist = np.bincount(px, minlength=256).astype(np.int64)
            out = np.zeros(3, np.float64)
            n = lib.ctd_topk_colors(hist.ctypes.data, out.ctypes.data)
            otsu = lib.ctd_otsu_from_hist(hist.ctypes.data) if len(px) else None
            yield what, (out[:n].tolist(), otsu), oracle_refine_decisions(px)
    sweep("refine decisions on tied histograms", 200, cases(), compare_refine_decisions)


def test_grouping_on_tie_grids_on_this_host():
    """`ctd_group_output` (csrc/host_group.cpp; no GPU work) on grids of equal boxes (tests/test_group_native.py `grid_page`,
    seeds 0 .. 59), on THIS host: lines of one row tie in `TextBlock.distance`, their order is numpy's argsort on values whose
    last bit is numpy's arccos -- both resolved at run time by csrc/np_dispatch.h, with a silent fallback."""
    from test_group_native import grid_page
    p = pkg()

    def cases():
        for seed in range(60):
            blks, lines, im_w, im_h, mask = grid_page(seed)
            got = p.textblock.group_output(copy.deepcopy(blks), lines.copy(), im_w, im_h, mask)
            yield (f"grid page seed {seed}: {len(lines)} lines, {len(blks[0])} blocks, {im_h}x{im_w}", got,
                   R.group_output(copy.deepcopy(blks), lines.copy(), im_w, im_h, mask))
    sweep("grouping on tie grids", 60, cases(), compare_groups)
