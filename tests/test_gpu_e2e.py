"""-m gpu: the whole `TextDetector.__call__` mirror (network outputs -> NMS -> DB boxes ->
block grouping -> mask refinement) against the oracle's restatement of reference
inference.py:148-178, (a) on rendered text-like network outputs at 1024x1024 and
(b) driven by the real HIP forward with seeded random weights at 256x256."""
import os

import numpy as np
import pytest
import torch

from conftest import checkpoint, pkg
from oracle import postproc_ref as R
from sweep_cases import blks_tensor, letterbox_tail_case, tail_case   # noqa: F401 (blks_tensor: imported from here by other tests)
from sweep_cases import equal_up_to_tied_lines as _equal_up_to_tied_lines
from test_post_host import blocks_equal, fake_outputs

pytestmark = pytest.mark.gpu

_DET = {}


def detector(size):
    if size not in _DET:
        _DET[size] = pkg().detector.TextDetector(checkpoint(0), input_size=size, device="cuda", half=True)
    return _DET[size]


_FULL = {}


def full_outputs(det, x):
    """The seam's full contract (blks, mask f32, lines_map with both planes) for the pages `x` from the detector's
    engine -- and the check that a trimmed engine (outputs="detector", `TextDetector(trim_outputs=True)`: no
    threshold branch, no f32 mask) produces the very same blocks, u8 mask, shrink map and bitmap."""
    if "net" not in _FULL:
        _FULL["net"] = pkg().backend.HipTextDetBackend(checkpoint(0), device="cuda", precision=det.net.precision,
                                                       outputs="detector")
    trim = _FULL["net"]
    blks, mask, lines_map = det.net.forward_u8(x)
    side = (det.net.mask_u8.clone(), det.net.bitmap.clone())
    b2, m2, l2 = trim.forward_u8(x)
    torch.cuda.synchronize()
    assert m2 is None and l2.shape[1] == 1 and lines_map.shape[1] == 2
    assert torch.equal(b2, blks) and torch.equal(l2[:, 0], lines_map[:, 0])
    assert torch.equal(trim.mask_u8, side[0]) and torch.equal(trim.bitmap, side[1])
    return blks, mask, lines_map


@pytest.mark.parametrize("seed,keep", [(0, False), (1, True), (2, True)])
def test_tail_on_text_like_outputs_matches_oracle(seed, keep):
    size = 1024
    page, mask_u8, prob, blks = fake_outputs(seed, size)
    det = detector(size)
    bt = blks_tensor(blks)
    bitmap = (prob > 0.3).astype(np.uint8)
    got = det.tail_batch([page], torch.from_numpy(bt).cuda(), torch.from_numpy(mask_u8)[None].cuda(),
                         torch.from_numpy(prob)[None].cuda(), torch.from_numpy(bitmap)[None].cuda(),
                         refine_mode=1 if keep else 0, keep_undetected_mask=keep)[0]
    mask_f = (mask_u8.astype(np.float32) + 0.5) / 255            # postprocess_mask truncates back to mask_u8
    lines_map = np.stack([prob, np.zeros_like(prob)])[None]
    ref = R.detector_tail(page, bt, mask_f[None, None], lines_map, input_size=(size, size),
                          refine_mode=1 if keep else 0, keep_undetected_mask=keep)
    np.testing.assert_array_equal(got[0], ref[0])                # mask (after the in-place edit when keep=True)
    blocks_equal(got[2], ref[2])
    np.testing.assert_array_equal(got[1], ref[1])                # refined mask, bit exact
    assert len(got[2]) > 3 and (got[1] > 0).mean() > 0.005


def _tail_sweep(name, cases, strict):
    """Runs (seed, keep, got, ref) of `cases` through the three assertions of the test above.  A page whose ONLY difference is the
    order of lines with tied distances is counted apart (see `_equal_up_to_tied_lines`); anything else fails -- and with `strict`
    (the default range, run by the suite) a page of the first kind fails too."""
    bad, tied = [], []
    for what, keep, got, ref in cases:
        try:
            np.testing.assert_array_equal(got[0], ref[0])
            blocks_equal(got[2], ref[2])
            np.testing.assert_array_equal(got[1], ref[1])
        except AssertionError as e:
            if np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]) and _equal_up_to_tied_lines(got[2], ref[2]):
                tied.append(what)
            else:
                bad.append((what, keep, str(e)[:200]))
    print(f"\n{name}: {len(bad)} mismatching pages {bad[:5]}; {len(tied)} pages equal up to the order of tied lines {tied}")
    assert not bad, bad
    if strict:
        assert not tied, f"equal up to the order of tied lines only (the numeric fallback of csrc/np_dispatch.h?): {tied}"


TAIL_SWEEP_DEFAULT = (1000, 1023, 1024)
LETTERBOX_SWEEP_DEFAULT = (2000, 2023)


def test_tail_seed_sweep():
    """The whole-tail parity of the test above over a range of seeds, alternating the two configurations: seeds 1000 .. 1023 at
    1024, or CTD_TAIL_SWEEP="first:last[:size]" by hand.  A page whose ONLY difference is the order of lines with tied distances
    is counted apart (see `_equal_up_to_tied_lines`) and fails the default range only; anything else fails.  Round 6: the first
    sweep (120 pages) found four mismatching pages -- numpy's default argsort (x86-simd-sort on this host) on blocks of more than
    16 tied lines, numpy's SVML arccos against glibc's acos ordering lines of one text row (the product now calls numpy's own
    functions for both, csrc/np_dispatch.h), and two hull edges bounding rectangles of equal area told apart by rounding noise
    (both `min_area_box` use a relative margin).  545 pages at seven sizes since: 0 mismatches, 0 tie-order differences."""
    spec = os.environ.get("CTD_TAIL_SWEEP", "")
    parts = [int(v) for v in spec.split(":")] if spec else list(TAIL_SWEEP_DEFAULT)
    first, last, size = parts[0], parts[1], (parts[2] if len(parts) > 2 else 1024)
    det = detector(size)

    def cases():
        for seed in range(first, last + 1):
            keep = bool(seed & 1)
            page, bt, mask_u8, prob, mask_f, lines_map, what = tail_case(seed, size)
            bitmap = (prob > 0.3).astype(np.uint8)
            got = det.tail_batch([page], torch.from_numpy(bt).cuda(), torch.from_numpy(mask_u8)[None].cuda(),
                                 torch.from_numpy(prob)[None].cuda(), torch.from_numpy(bitmap)[None].cuda(),
                                 refine_mode=1 if keep else 0, keep_undetected_mask=keep)[0]
            ref = R.detector_tail(page, bt, mask_f, lines_map, input_size=(size, size),
                                  refine_mode=1 if keep else 0, keep_undetected_mask=keep)
            yield seed, keep, got, ref
    _tail_sweep(f"tail sweep: seeds {first}..{last} at {size}", cases(), strict=not spec)


def test_letterboxed_tail_sweep():
    """Pages of RANDOM sizes and aspect ratios (200 .. 1500 pixels a side) with network outputs consistent with their letterbox
    at 512 (tests/sweep_cases.py `letterbox_tail_case`): the native tail's inverse mapping (mask crop + resize to the page, box /
    line rescale with the reference's truncations) and everything after it against `R.detector_tail`, both configurations.
    Seeds 2000 .. 2023, or CTD_LETTERBOX_SWEEP="first:last" by hand (tied-line order fails the default range only)."""
    spec = os.environ.get("CTD_LETTERBOX_SWEEP", "")
    first, last = [int(v) for v in spec.split(":")[:2]] if spec else LETTERBOX_SWEEP_DEFAULT
    size = 512
    det = detector(size)

    def cases():
        for seed in range(first, last + 1):
            keep = bool(seed & 1)
            page, bt, mask, lines_map, (dw, dh), what = letterbox_tail_case(seed, size)
            prob = np.ascontiguousarray(lines_map[0, 0])
            mask_u8 = (mask[0, 0] * 255).astype(np.uint8)                 # postprocess_mask's truncation
            bitmap = (prob > 0.3).astype(np.uint8)
            got = det.tail_batch([page], torch.from_numpy(bt).cuda(), torch.from_numpy(mask_u8)[None].cuda(),
                                 torch.from_numpy(prob)[None].cuda(), torch.from_numpy(bitmap)[None].cuda(),
                                 refine_mode=1 if keep else 0, keep_undetected_mask=keep,
                                 metas=[(page.shape[0], page.shape[1], dw, dh)])[0]
            ref = R.detector_tail(page, bt, mask, lines_map, input_size=(size, size), dw=dw, dh=dh,
                                  refine_mode=1 if keep else 0, keep_undetected_mask=keep)
            yield (seed, page.shape[:2]), keep, got, ref
    _tail_sweep(f"letterbox sweep: seeds {first}..{last}", cases(), strict=not spec)


def test_full_detector_on_network_outputs_matches_oracle():
    """The real forward (random weights -> noisy maps: many tiny contours, the worst case for
    the contour/box code) feeding the tail; the oracle tail runs on the same network outputs."""
    size = 256
    p = pkg()
    page = p.synth.text_like_page((size, size), 5, n_blocks=4)
    det = detector(size)
    m, refined, blk_list = det(page, refine_mode=0, keep_undetected_mask=True)
    blks, mask, lines_map = full_outputs(det, torch.from_numpy(page)[None].cuda())
    ref = R.detector_tail(page, blks.cpu().numpy(), mask.cpu().numpy(), lines_map.cpu().numpy(),
                          input_size=(size, size), refine_mode=0, keep_undetected_mask=True)
    np.testing.assert_array_equal(m, ref[0])
    blocks_equal(blk_list, ref[2])
    np.testing.assert_array_equal(refined, ref[1])


def test_detect_batch_equals_single_calls():
    size = 256
    p = pkg()
    pages = [p.synth.text_like_page((size, size), s, n_blocks=4) for s in (7, 8, 9)]
    det = detector(size)
    batch = det.detect_batch(pages)
    for pg, (m, r, bl) in zip(pages, batch):
        m1, r1, bl1 = det(pg)
        np.testing.assert_array_equal(m, m1)
        np.testing.assert_array_equal(r, r1)
        blocks_equal(bl, bl1)


def test_resize_kernel_matches_opencv_restatement():
    """ctd_resize_linear_u8 vs the oracle's restatement of cv2.resize(INTER_LINEAR) (bit exact)."""
    from oracle import cv_ref as cv
    p = pkg()
    rng = np.random.RandomState(0)
    for (sh, sw), (dh, dw) in [((117, 165), (72, 102)), ((300, 200), (1024, 683)), ((64, 64), (64, 64)),
                               ((1654, 1170), (1024, 724)), ((50, 70), (333, 97))]:
        img = rng.randint(0, 256, (sh, sw, 3)).astype(np.uint8)
        got = p.backend.resize_linear_u8(torch.from_numpy(img).cuda(), (dh, dw)).cpu().numpy()
        np.testing.assert_array_equal(got, cv.resize_linear_u8(img, (dw, dh)))
        m = img[..., 0].copy()
        got = p.backend.resize_linear_u8(torch.from_numpy(m).cuda(), (dh, dw), (dh + 5, dw + 9)).cpu().numpy()
        ref = np.zeros((dh + 5, dw + 9), np.uint8)
        ref[:dh, :dw] = cv.resize_linear_u8(m, (dw, dh))
        np.testing.assert_array_equal(got, ref)


def test_detector_on_page_of_another_size_matches_oracle():
    """A portrait page larger than the network input: letterbox (GPU) -> net -> tail with the
    inverse mapping (mask crop + resize, box / line rescale), reference inference.py:143-172."""
    from oracle import cv_ref as cv
    size = 256
    p = pkg()
    page = p.synth.text_like_page((413, 292), 11, n_blocks=5)        # 1654x1170 / 4, like the reference's example
    det = detector(size)
    m, refined, blk_list = det(page, refine_mode=1, keep_undetected_mask=True)
    lb, ratio, (dw, dh) = cv.letterbox(page, (size, size))
    x = torch.from_numpy(lb)[None].cuda()
    blks, mask, lines_map = full_outputs(det, x)
    ref = R.detector_tail(page, blks.cpu().numpy(), mask.cpu().numpy(), lines_map.cpu().numpy(),
                          input_size=(size, size), dw=dw, dh=dh, refine_mode=1, keep_undetected_mask=True)
    assert m.shape == page.shape[:2]
    np.testing.assert_array_equal(m, ref[0])
    blocks_equal(blk_list, ref[2])
    np.testing.assert_array_equal(refined, ref[1])


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_refine_mask_gpu_merge_stage_on_adversarial_windows(seed):
    """`refine_mask` through the native tail (tw_hist / xor / render, ccl, tw_accept / dilate / holes /
    commit) against the oracle on pages built to stress it: noisy colours (many small
    components per candidate), blob masks, and text blocks that overlap each other, touch the page
    border or are a few pixels thin -- the cases the text-like pages do not reach."""
    p = pkg()
    rng = np.random.RandomState(seed)
    H, W = 384, 512
    page = rng.randint(0, 256, (H, W, 3)).astype(np.uint8)
    page[:, : W // 2] = (page[:, : W // 2] // 64) * 64                  # flat-ish colour regions on one half
    mask = np.zeros((H, W), np.uint8)
    for _ in range(60):
        y, x = rng.randint(0, H), rng.randint(0, W)
        hh, ww = rng.randint(2, 40), rng.randint(2, 60)
        mask[y: y + hh, x: x + ww] = rng.randint(40, 256)
    boxes = [[0, 0, 90, 70], [60, 40, 220, 160], [200, 100, 330, 230], [W - 120, H - 90, W, H],
             [10, 300, 400, 306], [430, 5, 436, 200], [100, 100, 180, 150]]
    for _ in range(5):
        x1, y1 = rng.randint(0, W - 40), rng.randint(0, H - 40)
        boxes.append([x1, y1, min(W, x1 + rng.randint(12, 200)), min(H, y1 + rng.randint(12, 150))])
    blks = [p.textblock.TextBlock(b) for b in boxes]
    rblks = [R.TextBlock(b) for b in boxes]
    for mode in (0, 1):
        got = p.textmask.refine_mask(page, mask, blks, mode, "cuda")
        ref = R.refine_mask(page, mask, rblks, mode)
        np.testing.assert_array_equal(got, ref)
    m1, m2 = mask.copy(), mask.copy()
    got = p.textmask.refine_undetected_mask(page, m1, p.textmask.refine_mask(page, mask, blks[:4], 0, "cuda"), blks[:4], 0, "cuda")
    ref = R.refine_undetected_mask(page, m2, R.refine_mask(page, mask, rblks[:4], 0), rblks[:4], 0)
    np.testing.assert_array_equal(got, ref)
    np.testing.assert_array_equal(m1, m2)


def test_refine_mask_batch_equals_single_pages():
    """`refine_mask_batch` packs the windows of several pages (of different sizes) into shared canvases
    and launches; every page must come out as from its own call, and as from the oracle."""
    p = pkg()
    pages, masks, blks = [], [], []
    for seed in range(3):
        page, mask_u8, prob, b = fake_outputs(seed, 384 + 64 * seed)
        boxes = [p.textblock.TextBlock([int(v) for v in bb]) for bb in b[0]]
        pages.append(page)
        masks.append(mask_u8)
        blks.append(boxes)
    blks.append([])                                               # a page without blocks
    pages.append(pages[0])
    masks.append(masks[0])
    together = p.textmask.refine_mask_batch(pages, masks, blks, 0, "cuda")
    for a, m, bl, pg in zip(together, masks, blks, pages):
        np.testing.assert_array_equal(a, p.textmask.refine_mask(pg, m, bl, 0, "cuda"))
        np.testing.assert_array_equal(a, R.refine_mask(pg, m, [R.TextBlock(x.xyxy) for x in bl], 0))
    assert not together[3].any()


def test_db_stage_on_device_tables_matches_oracle_and_falls_back_on_overflow():
    """`SegRepresenter` (two labelling passes + contour tables on the GPU, geometry on the host) against the
    oracle's contour walk on speckle maps; a map with more components than the compact tables hold takes
    the label-image path (the overflow flag of the trace is asserted) and must give the same answer -- here on a map whose
    boxes all score 0; tests/test_gpu_tail_caps.py checks that path on maps whose last components decide boxes that score."""
    from scipy import ndimage
    p = pkg()
    rep = p.postproc.SegRepresenter()
    probs = []
    for seed in range(4):
        rng = np.random.RandomState(200 + seed)
        pr = ndimage.uniform_filter(rng.rand(192, 256), 1 + seed).astype(np.float32)
        probs.append((pr - pr.min()) / (pr.max() - pr.min()) * 0.62)
    prob = torch.from_numpy(np.stack(probs)).cuda()
    boxes, scores = rep(prob, (prob > 0.3).to(torch.uint8))
    for b in range(4):
        rb, rs = R.boxes_from_bitmap(probs[b], probs[b] > 0.3, 256, 192)
        np.testing.assert_array_equal(boxes[b], rb)
        np.testing.assert_allclose(scores[b], rs, rtol=0, atol=1e-6)
    # > 65536 single-pixel components + one solid block: `tail_trace_cases.overflow_map`, 524 a side (67 259 components; the
    # 516-a-side map this test had has 65 179 and fits).  `rep` runs on the calling thread's tail: its trace shows the flag.
    from tail_trace_cases import COMP_CAP, db_counts, overflow_map
    big = overflow_map()
    side = big.shape[0]
    assert big.shape == (side, side) and db_counts(big)[0] > COMP_CAP
    bt = torch.from_numpy(big)[None].cuda()
    tail = p.tail.thread_tail(bt.device)
    tail.set_trace(True)
    try:
        boxes, scores = rep(bt, (bt > 0.3).to(torch.uint8))
        (page,) = tail.trace_db()
    finally:
        tail.set_trace(False)
    assert int(page["hdr"][3]) == 1 and int(page["hdr"][0]) == COMP_CAP, page["hdr"]
    rb, rs = R.boxes_from_bitmap(big, big > 0.3, side, side)
    np.testing.assert_array_equal(boxes[0], rb)
    np.testing.assert_allclose(scores[0], rs, rtol=0, atol=1e-6)


def test_detect_stream_equals_detect_batch():
    """The pipelined form (tails on worker threads under the next forward) returns what detect_batch returns."""
    size = 256
    p = pkg()
    det = detector(size)
    batches = [[p.synth.text_like_page((size, size), 30 + 3 * k + j, n_blocks=4) for j in range(3)] for k in range(4)]
    want = [det.detect_batch(b) for b in batches]
    for engines, split in ((1, 1), (2, 1), (1, 2), (1, 8)):   # 2 engines: batches alternate over two engine copies /
        # streams; split: a batch's tail as that many page-range work items (8 > pages per batch: one page each)
        got = list(det.detect_stream(batches, workers=2, depth=3, engines=engines, tail_split=split))
        assert len(got) == len(want)
        for gb, wb in zip(got, want):
            for (m, r, bl), (m1, r1, bl1) in zip(gb, wb):
                np.testing.assert_array_equal(m, m1)
                np.testing.assert_array_equal(r, r1)
                blocks_equal(bl, bl1)


@pytest.mark.parametrize("lds", [1, 0])
def test_detect_stream_equals_detect_batch_under_every_tail_chain(lds):
    """`tail_chain` = 0 / 1 / 2 (stage 1 of concurrent work items side by side / one after the other on the GPU / the refine
    stage's big enqueue too): three workers on four work items per batch return what detect_batch returns.  Once more with
    every window through the canvases (`tail_lds` = 0), where `refine_canvas`' chained section at 2 is what runs."""
    size = 256
    p = pkg()
    det = detector(size)
    batches = [[p.synth.text_like_page((size, size), 30 + 3 * k + j, n_blocks=4) for j in range(3)] for k in range(3)]
    want = [det.detect_batch(b) for b in batches]
    assert sum(len(bl) for wb in want for _, _, bl in wb) >= 9 and any((r > 0).any() for wb in want for _, r, _ in wb)
    list(det.detect_stream(batches[:1], workers=3, depth=3, tail_split=4))       # (the pool of three workers and their tails exist)
    tails = p.tail.live_tails()
    for chain in (0, 1, 2):
        with p._lib.tuning(tail_chain=chain, tail_lds=lds):
            got = list(det.detect_stream(batches, workers=3, depth=3, tail_split=4))
        assert len(got) == len(want)
        for gb, wb in zip(got, want):
            for (m, r, bl), (m1, r1, bl1) in zip(gb, wb):
                np.testing.assert_array_equal(m, m1, err_msg=f"tail_chain = {chain}")
                np.testing.assert_array_equal(r, r1, err_msg=f"tail_chain = {chain}")
                blocks_equal(bl, bl1)
    assert p.tail.live_tails() == tails


@pytest.mark.parametrize("priority", [0, 1, 2])
def test_tail_created_under_every_stream_priority_refines_exactly(priority):
    """`tail_priority` = 0 / 1 / 2 (highest / the device's default / lowest, read when a tail is created): a tail object
    created under the key runs the call of big, tiny, overlapping and repeated windows exactly as the oracle has it."""
    import tail_trace_cases as T
    from test_gpu_sweeps import report
    from test_gpu_tail_trace import check_call, traced_refine
    p = pkg()
    start = p.tail.live_tails()
    with p._lib.tuning(tail_priority=priority):
        tail = p.tail.Tail(torch.device("cuda", torch.cuda.current_device()))
    try:
        case = T.refine_cases()[2]
        n, bad = check_call(case, traced_refine(case, tail=tail), f" [tail_priority = {priority}]")
    finally:
        tail.__del__()
        del tail
    assert p.tail.live_tails() == start
    report(f"refine on a tail of priority {priority}", n, bad)


def test_model2annotations_batch_driver_writes_the_reference_files(tmp_path):
    """`model2annotations` (batched detect + threaded decode / write) leaves exactly the files the
    reference's loop writes (inference.py:19-70), with the contents of single-page detector calls."""
    from PIL import Image
    p = pkg()
    ann = p.annotations
    src, out = tmp_path / "pages", tmp_path / "out"
    src.mkdir()
    names = ["p0.png", "p1.PNG", "scan.2.bmp"]
    for i, nm in enumerate(names):
        page = p.synth.text_like_page((512 + 64 * i, 448), seed=20 + i, n_blocks=6)
        Image.fromarray(page[:, :, ::-1]).save(src / nm)
    (src / "readme.txt").write_text("not an image")
    ck = checkpoint(0)
    det = p.detector.TextDetector(ck, input_size=512, device="cuda")
    n = ann.model2annotations(ck, str(src), str(out), save_json=True, batch_size=2, detector=det)
    assert n == 3
    expect = {}
    for nm in names:
        img = ann.imread(str(src / nm))
        mask, refined, blks = det(img, refine_mode=p.textmask.REFINEMASK_ANNOTATION, keep_undetected_mask=True)
        expect.update(ann.page_files(str(out), nm, img, refined, blks, save_json=True))
    assert sorted(os.listdir(out)) == sorted(os.path.basename(k) for k in expect)
    for path, content in expect.items():
        got = open(path, "rb").read()
        assert got == (content if isinstance(content, bytes) else content.encode("utf8")), path


@pytest.mark.parametrize("keep", [0, 1])
def test_tail_on_the_reference_example_page_matches_reference_code_golden(keep):
    """The reference's real example page (1654x1170 spread, letterboxed to 1024) through the native tail,
    against the results of the reference's OWN `TextDetector.__call__` for it (tests/golden/real_page.npz,
    oracle/gen_golden_real.py): masks bit for bit, block records byte for byte."""
    import json
    from conftest import GOLDEN
    from oracle.gen_golden_real import SIZE, load_fixture
    p = pkg()
    page, blks, mask_u8, prob, (dw, dh), g = load_fixture(os.path.join(GOLDEN, "real_page.npz"))
    det = detector(SIZE)
    im_h, im_w = page.shape[:2]
    bitmap = (prob > 0.3).astype(np.uint8)
    m, r, b = det.tail_batch([page], torch.from_numpy(blks).cuda(), torch.from_numpy(mask_u8)[None].cuda(),
                             torch.from_numpy(prob)[None].cuda(), torch.from_numpy(bitmap)[None].cuda(), refine_mode=keep,
                             keep_undetected_mask=bool(keep), metas=[(im_h, im_w, dw, dh)])[0]
    assert m.shape == (1170, 1654)
    np.testing.assert_array_equal(m, g[f"mask{keep}"])
    np.testing.assert_array_equal(np.packbits(r > 0), g[f"refined{keep}"])
    rec = p.annotations.blocks_json(b)
    assert rec.encode("utf8") == g[f"records{keep}"].tobytes()


def test_trimmed_detector_returns_the_same_results():
    """`TextDetector(trim_outputs=True)`: same masks and blocks as the full-network detector."""
    p = pkg()
    page = p.synth.text_like_page((256, 256), 9, n_blocks=4)
    a = detector(256)(page, refine_mode=0, keep_undetected_mask=True)
    b = p.detector.TextDetector(checkpoint(0), input_size=256, device="cuda", half=True, trim_outputs=True)(
        page, refine_mode=0, keep_undetected_mask=True)
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1], b[1])
    blocks_equal(a[2], b[2])


def test_host_pages_are_staged_through_pinned_memory():
    """numpy pages (what the reference's callers hand over) go through `_stage`: one pinned buffer and one async
    copy per batch, from loader threads in `detect_stream`; results equal those of device-resident pages, mixed
    page sizes included."""
    p = pkg()
    det = detector(256)
    batches = [[p.synth.text_like_page((256, 256), 50 + 3 * k + j, n_blocks=4) for j in range(3)] for k in range(3)]
    batches[1][1] = p.synth.text_like_page((200, 144), 77, n_blocks=3)
    want = [det.detect_batch([torch.from_numpy(pg).cuda() for pg in b]) for b in batches]
    got_batch = [det.detect_batch(b) for b in batches]
    got_stream = list(det.detect_stream(batches, workers=2, depth=2, loaders=2))
    for got in (got_batch, got_stream):
        for gb, wb in zip(got, want):
            for (m, r, bl), (m1, r1, bl1) in zip(gb, wb):
                np.testing.assert_array_equal(m, m1)
                np.testing.assert_array_equal(r, r1)
                blocks_equal(bl, bl1)


@pytest.mark.parametrize("keep", [False, True])
def test_pageable_result_arrays_of_small_pages(keep):
    """`ctd_tail_run` promises to fill "host arrays": a C caller's malloc'ed masks are PAGEABLE.  Pages under 256 KB
    (`tail_dma_min`) are downloaded by segments of the stage's copy kernel when the arrays are page-locked -- a kernel
    store into pageable memory would be a memory fault, so such arrays must take the hipMemcpyAsync path.
    Small pages, not back to back (separate numpy arrays), B = 3, both the same-size and the letterboxed (resized) form."""
    p = pkg()
    size = 256
    det = detector(size)
    for shapes in ([(size, size)] * 3, [(200, 180), (256, 256), (300, 212)]):
        pages = [p.synth.text_like_page(sh, 40 + i, n_blocks=4) for i, sh in enumerate(shapes)]
        job = det._forward(pages)
        torch.cuda.synchronize()
        tl = p.tail.thread_tail(det.net.device)
        args = (job["gpu"], job["metas"], job["blks"], job["mask_u8"], job["lines_map"], job["bitmap"], det.conf_thresh,
                det.nms_thresh, 0.6, True, 1 if keep else 0, keep, job["ev"])
        ref = tl.run(*args)
        got = tl.run(*args, pinned=False)
        for (m0, r0, b0), (m1, r1, b1) in zip(ref, got):
            np.testing.assert_array_equal(m0, m1)
            np.testing.assert_array_equal(r0, r1)
            blocks_equal(b0, b1)
        assert any((r > 0).any() for _, r, _ in got)


def _speckle_page(H, W, seed):
    """7x7 dark squares on an 8-pixel grid (60 % of the cells): thousands of separate components per window that the merge
    stage ACCEPTS (a square survives the 3x3 erosion as 5x5 > half of it); the raw mask misses 15 % of them."""
    rng = np.random.RandomState(seed)
    on = rng.rand(H // 8, W // 8) < 0.6
    dark = np.zeros((H, W), bool)
    for dy in range(7):
        for dx in range(7):
            dark[dy::8, dx::8][: on.shape[0], : on.shape[1]] |= on
    page = np.full((H, W, 3), 235, np.uint8)
    page[dark] = 20
    page = (page.astype(int) + rng.randint(-12, 13, (H, W, 3))).clip(0, 255).astype(np.uint8)
    mask = np.where(dark, 220, 0).astype(np.uint8)
    drop = rng.rand(H // 8, W // 8) < 0.15
    for dy in range(8):
        for dx in range(8):
            mask[dy::8, dx::8][: on.shape[0], : on.shape[1]][drop] = 0
    return page, mask


def test_canvas_path_equals_the_oracle_on_speckle_pages():
    """The canvas path (`tail_lds` = 0: every window through `tw_accept_count_kernel` / `tw_accept_apply_kernel` /
    `tw_holes_kernel`, many blocks per window) on pages built to overflow the count kernel's per-block LDS table:
    page-sized windows over a speckle of 7x7 squares give every candidate mask thousands of components (more keys per block
    than its 1024 slots, probe failures), i.e. the global-atomic spill inside the kernel -- a branch the text-like pages of
    the other tests never reach.  Both refine modes, byte-identical to the oracle's refine_mask on both pages."""
    p = pkg()
    for H, W in ((320, 448), (960, 1024)):
        page, mask = _speckle_page(H, W, 5)
        boxes = [[2, 2, W - 2, H - 2], [0, 0, W // 2, H // 2], [W // 3, H // 4, W - 5, H - 9], [5, H // 2, W // 2, H - 1]]
        blks = [p.textblock.TextBlock(b) for b in boxes]
        got, paths = _refine_under(p, {"tail_lds": 0}, page, mask, blks)
        assert paths["lds"] == 0 and paths["canvas"] == len(boxes), paths
        assert (got[0] > 0).mean() > 0.2
        rblks = [R.TextBlock(b) for b in boxes]
        for mode in (0, 1):
            np.testing.assert_array_equal(got[mode], R.refine_mask(page, mask, rblks, mode))


def _refine_under(p, key_values, page, mask, blks, dev="cuda"):
    """refine_mask (both modes) under tuning keys, the keys restored afterwards; returns (masks, paths of the last call)"""
    with p._lib.tuning(key_values):
        out = [p.textmask.refine_mask(page, mask, blks, mode, dev) for mode in (0, 1)]
        paths = p.tail.thread_tail(torch.device("cuda", 0)).refine_paths()
    return out, paths


def test_window_local_merge_kernel_equals_the_canvas_path_and_the_oracle():
    """`tw_lds_kernel` (round 6: merge_mask_list of a window as one block on bit planes in LDS) on text-like pages, on a
    speckle of 7x7 squares (hundreds of runs per row band), and on windows chosen for its edges -- narrower than a word,
    exactly 32 / 33 / 64 / 65 wide, one or two pixels high, overlapping, clipped at the page border: byte-identical to
    (a) the canvas path (`tail_lds` = 0), (b) the FORCED OVERFLOW path (`tail_lds_rcap` = 8: every window's run table
    overflows on the device, the host re-does it through the canvases), (c) the oracle's refine_mask."""
    p = pkg()
    cases = []
    page, _, mask, _, _ = p.synth.text_like_outputs(11, 512, n_blocks=8)       # ink + a mask a trained detector would give
    rng = np.random.RandomState(4)
    mask = (mask * (rng.rand(512, 512) > 0.1)).astype(np.uint8)                  # ... with a tenth of its pixels knocked out
    boxes = [[10, 10, 200, 150], [180, 100, 500, 380], [0, 0, 42, 30], [300, 5, 332, 60], [301, 70, 334, 130],
             [100, 200, 164, 300], [99, 301, 164, 380], [400, 10, 406, 300], [5, 350, 500, 352], [20, 360, 400, 361],
             [450, 300, 511, 383], [40, 390, 480, 505]]
    cases.append((page, mask, boxes))
    spage, smask = _speckle_page(256, 320, 7)
    cases.append((spage, smask, [[4, 4, 150, 120], [100, 60, 310, 250], [0, 130, 90, 255]]))
    for page, mask, boxes in cases:
        blks = [p.textblock.TextBlock(b) for b in boxes]
        lds, paths = _refine_under(p, {}, page, mask, blks)
        assert paths["lds"] == len(boxes) and paths["canvas"] == 0 and paths["overflow"] == 0, paths
        canvas, pc = _refine_under(p, {"tail_lds": 0}, page, mask, blks)
        assert pc["lds"] == 0 and pc["canvas"] == len(boxes), pc
        forced, pf = _refine_under(p, {"tail_lds_rcap": 8}, page, mask, blks)
        assert pf["overflow"] >= len(boxes) - 3 and pf["canvas"] == pf["overflow"], pf       # (a near-empty window may fit 8 runs)
        rblks = [R.TextBlock(b) for b in boxes]
        for mode in (0, 1):
            want = R.refine_mask(page, mask, rblks, mode)
            np.testing.assert_array_equal(lds[mode], want)
            np.testing.assert_array_equal(canvas[mode], want)
            np.testing.assert_array_equal(forced[mode], want)
        assert (lds[0] > 0).mean() > 0.005


def test_windows_split_between_the_lds_kernel_and_the_canvas_path_by_size():
    """A page whose blocks give one window beyond the LDS limit (canvas path) next to small ones (window-local kernel), and
    the three LDS launch classes by footprint (`tail_lds_max_bytes` lowered so that mid-sized windows change class)."""
    p = pkg()
    page = p.synth.text_like_page((768, 1024), 5, n_blocks=10)
    mask = np.where(page.min(2) < 128, 230, 10).astype(np.uint8)
    boxes = [[20, 20, 1000, 740], [30, 30, 130, 100], [200, 100, 460, 330], [500, 400, 800, 640], [600, 50, 760, 200]]
    blks = [p.textblock.TextBlock(b) for b in boxes]
    want = [R.refine_mask(page, mask, [R.TextBlock(b) for b in boxes], mode) for mode in (0, 1)]
    got, paths = _refine_under(p, {}, page, mask, blks)
    assert paths["canvas"] == 1 and paths["lds"] == len(boxes) - 1, paths
    small, ps = _refine_under(p, {"tail_lds_max_bytes": 60 << 10}, page, mask, blks)
    assert 0 < ps["lds"] < len(boxes) - 1 and ps["lds"] + ps["canvas"] == len(boxes), ps
    for mode in (0, 1):
        np.testing.assert_array_equal(got[mode], want[mode])
        np.testing.assert_array_equal(small[mode], want[mode])


def test_window_local_merge_kernel_random_stress_against_the_oracle():
    """Seeded stress of `tw_lds_kernel`: pages of random texture (flat areas, strokes, speckle, gradients), random
    predictions, random blocks of every aspect (1 .. 300 pixels, clipped at the borders, overlapping) -- refine_mask in both
    modes against the oracle, every window on the window-local path."""
    p = pkg()
    # CTD_TWLDS_STRESS_SEED / _CASES: longer runs by hand (round 6, at HEAD: 30 seeds x 100 cases = 15 131 windows in LDS +
    # 1 396 re-done after a run-table overflow, 0 mismatches against the oracle in either mode)
    rng = np.random.RandomState(int(os.environ.get("CTD_TWLDS_STRESS_SEED", "20260930")))
    n_cases = int(os.environ.get("CTD_TWLDS_STRESS_CASES", "12"))
    n_windows = n_over = 0
    for case in range(n_cases):
        H, W = int(rng.randint(40, 420)), int(rng.randint(40, 520))
        page = np.full((H, W, 3), rng.randint(150, 255), np.uint8)
        kind = case % 4
        ink = np.zeros((H, W), bool)
        for _ in range(rng.randint(20, 200)):
            y, x = rng.randint(0, H), rng.randint(0, W)
            if kind == 0:
                ink[y: y + rng.randint(1, 4), x: x + rng.randint(2, 40)] = True          # horizontal strokes
            elif kind == 1:
                ink[y: y + rng.randint(2, 40), x: x + rng.randint(1, 4)] = True          # vertical strokes
            elif kind == 2:
                ink[y: y + rng.randint(1, 3), x: x + rng.randint(1, 3)] = True           # speckle
            else:
                ink[y: y + rng.randint(3, 30), x: x + rng.randint(3, 30)] = True         # blobs
        page[ink] = rng.randint(0, 90)
        page = (page.astype(int) + rng.randint(-25, 26, page.shape)).clip(0, 255).astype(np.uint8)
        if case % 3 == 0:
            page[:, : W // 2] = 255 - page[:, : W // 2]                                  # light text on dark in one half
        from scipy import ndimage
        mask = (ndimage.maximum_filter(ink.astype(np.uint8), size=3) * rng.randint(100, 255)).astype(np.uint8)
        mask[rng.rand(H, W) < 0.05] = rng.randint(0, 255)
        boxes = []
        for _ in range(rng.randint(3, 9)):
            x1, y1 = int(rng.randint(0, W - 2)), int(rng.randint(0, H - 2))
            boxes.append([x1, y1, int(min(W - 1, x1 + rng.randint(1, 300))), int(min(H - 1, y1 + rng.randint(1, 300)))])
        blks = [p.textblock.TextBlock(b) for b in boxes]
        got, paths = _refine_under(p, {}, page, mask, blks)
        # (a candidate of pure speckle has more runs than the run table holds: those windows raise the overflow flag and are
        # re-done through the canvases -- same results; the pages here are small, so nothing is too LARGE for the LDS)
        assert paths["canvas"] == paths["overflow"] and paths["lds"] + paths["canvas"] == len(boxes), (case, paths)
        n_windows += paths["lds"]
        n_over += paths["overflow"]
        rblks = [R.TextBlock(b) for b in boxes]
        for mode in (0, 1):
            np.testing.assert_array_equal(got[mode], R.refine_mask(page, mask, rblks, mode), err_msg=f"case {case} mode {mode}")
    print(f"\nstress: {n_windows} windows merged in LDS, {n_over} re-done after a run-table overflow")
    assert n_windows >= 40
