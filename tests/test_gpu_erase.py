"""-m gpu: erasing text on plain backgrounds -- `ctd_erase_text` (csrc/kernels_erase.hip), `erase.erase_text`,
`TextDetector.erase_text` and the `erase=True` option of `model2annotations` -- against the numpy restatement
tests/erase_ref.py.  The rule is integers only, so every comparison is EXACT: every field of every row, every byte of every
cleaned page and of every rest mask."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import erase_ref as R
import test_gpu_regions as TG
from conftest import pkg
from sweep_cases import blks_tensor
from test_erase_ref import _spoil, one_bar, overlapping_pair

pytestmark = pytest.mark.gpu


# ---- 1. the kernels --------------------------------------------------------------------------------------------------------

def _edge_boxes(H, W):
    """Boxes at the four edges and corners, partly and wholly outside the page, without area, and the whole page."""
    return [(0, 0, 12, 9), (W - 11, 0, W, 8), (0, H - 9, 13, H), (W - 12, H - 8, W, H), (W // 3, 0, W // 3 + 20, 7),
            (W // 3, H - 7, W // 3 + 20, H), (0, H // 3, 9, H // 3 + 15), (W - 9, H // 3, W, H // 3 + 15),
            (-10, 5, 15, 14), (W - 8, 5, W + 22, 14), (5, -6, 25, 5), (5, H - 4, 25, H + 7), (-7, -5, 8, 7), (W - 6, -5, W + 9, 7),
            (-7, H - 5, 8, H + 7), (W - 6, H - 5, W + 9, H + 7), (-30, 5, -10, 14), (W, 5, W + 20, 14), (5, -20, 25, 0),
            (5, H, 25, H + 11), (-40, -40, -10, -10), (W + 3, H + 3, W + 33, H + 33), (10, 10, 10, 20), (10, 10, 30, 10),
            (30, 20, 10, 5), (0, 0, W, H), (-W, -H, 2 * W, 2 * H), (0, 0, R.MAX_COORD + 1, 10), (-R.MAX_COORD - 1, 0, 10, 10),
            (0, 0, R.MAX_COORD, H)]


def _runs_page():
    """40 x 300, flat: text runs of 63, 64 and 65 pixels and boxes that start at x = 62, 63, 0 and 1 (mod 64); boxes across the
    tile edges of both kernels (x = 64, 128, 192, 256; y = 32)."""
    page = np.full((40, 300, 3), (180, 200, 220), np.uint8)
    mask = np.zeros((40, 300), np.uint8)
    boxes = []
    for y, x, n in ((8, 62, 63), (14, 63, 64), (20, 64, 65), (26, 65, 63), (32, 126, 65), (3, 190, 64), (29, 1, 63), (35, 200, 90)):
        mask[y:y + 2, x:x + n] = 255
        boxes.append((x, y, x + n, y + 2))
    boxes += [(60, 6, 130, 30), (120, 28, 200, 36), (0, 0, 300, 40), (63, 13, 64, 16), (127, 20, 129, 22)]
    page[mask != 0] = (10, 20, 30)
    return page, mask, boxes


def _three_overlapping():
    """One long bar of text on a background of three near levels, claimed by three overlapping boxes: all PLAIN, different
    medians, every pair of fill regions overlaps and so do all three."""
    page = np.full((44, 110, 3), 100, np.uint8)
    page[:, 40:] = 106
    page[:, 70:] = 112
    mask = np.zeros((44, 110), np.uint8)
    mask[18:24, 8:100] = 255
    page[mask != 0] = 0
    return page, mask, [(8, 18, 50, 24), (40, 15, 75, 27), (60, 18, 100, 24)]


def _plain_over_textured():
    """A bar of text that runs from a flat area into noise: the box on the flat part is PLAIN, the overlapping box on the
    noise is TEXTURED, in both orders."""
    rng = np.random.default_rng(3)
    page = np.full((40, 130, 3), 150, np.uint8)
    page[:, 60:] = rng.integers(60, 256, (40, 70, 3), dtype=np.uint8)
    mask = np.zeros((40, 130), np.uint8)
    mask[17:22, 10:120] = 255
    page[mask != 0] = 5
    return page, mask, [(10, 17, 50, 22), (44, 17, 120, 22), (12, 17, 48, 22)]


def _material():
    """[(page, mask, boxes)]: the pages of ONE call."""
    rng = np.random.default_rng(33)
    out = []
    # random pages (TEXTURED) of the issue's sizes at mask densities 0.02, 0.5, 0, 1; boxes at every edge
    for (H, W), dens in (((61, 83), 0.02), ((120, 97), 0.02), ((33, 150), 0.5), ((61, 83), 0.0), ((33, 150), 1.0)):
        page = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        mask = (rng.random((H, W)) < dens).astype(np.uint8) * rng.integers(1, 256, (H, W), dtype=np.uint8)
        boxes = _edge_boxes(H, W) + [(20, 12, 60, 30), (50, 5, 80, 33), (3, 3, W - 3, H - 3)]
        if H == 120:
            boxes += [(30, 20, 90, 110), (60, 60, 70, 70), (0, 30, 97, 66), (62, 0, 66, 120)]
        out.append((page, mask, boxes))
    out.append(_runs_page())
    # a page of one colour: whatever the mask, the ring has one value
    mask = (rng.random((50, 70)) < 0.02).astype(np.uint8) * 255
    out.append((np.full((50, 70, 3), 117, np.uint8), mask, _edge_boxes(50, 70) + [(20, 10, 50, 40)]))
    out.append(_three_overlapping())
    out.append(_plain_over_textured())
    out.append(overlapping_pair())
    for page, mask, boxes, _ in R.flat_cases():
        out.append((page, mask, boxes))
    page, mask, box, ring = one_bar()
    for k in (25, 26):                                            # the two sides of 15/16
        out.append((_spoil(page, ring, k, 0, 1), mask, [box]))
    out.append((_spoil(page, ring, 26, 212, 2), mask, [box]))     # at tol
    out.append((_spoil(page, ring, 26, 213, 2), mask, [box]))     # beyond it
    out.append((_spoil(one_bar(balloon=110)[0], ring, 200, 100, 0), mask, [box]))   # the lower median of an even count
    out.append((page, mask, []))                                  # a page without blocks in the middle of the call
    m2 = mask.copy()
    m2[2:5, 60:66] = 7
    out.append((page, m2, [box, (0, 30, 12, 40)]))                # mask that belongs to no block; NO_MASK
    return out


def _compare(er, material, kw, what=""):
    """Every row, every byte of out and rest against the restatement; returns the reference rows."""
    want_rows, k, bad = [], 0, []
    for i, (page, mask, boxes) in enumerate(material):
        rows, out, rest = R.erase_page(page, mask, boxes, **kw)
        for b, ref in enumerate(rows):
            assert er.index[k].tolist() == [i, b]
            got = R.row_dict(er.rows[k])
            if got != ref or er.rows[k]["pad_"].any():
                bad.append((i, b, boxes[b], {f: (got[f], ref[f]) for f in R.FIELDS if got[f] != ref[f]}))
            k += 1
        want_rows += rows
        g_out, g_rest = er.pages[i].cpu().numpy(), er.rest[i].cpu().numpy()
        assert g_out.shape == page.shape and g_rest.shape == mask.shape and er.pages[i].is_contiguous() and er.rest[i].is_contiguous()
        if not np.array_equal(g_out, out):
            bad.append((i, "out", int((g_out != out).any(axis=2).sum()), np.argwhere((g_out != out).any(axis=2))[:4].tolist()))
        if not np.array_equal(g_rest, rest):
            bad.append((i, "rest", int((g_rest != rest).sum()), np.argwhere(g_rest != rest)[:4].tolist()))
    assert k == len(er) == len(er.rows)
    assert not bad, f"{what}: {len(bad)} differences, first: {bad[:4]}"
    return want_rows


def _device_inputs(material, dev):
    """Device tensors of the material; page 1 (120 x 97) is a view with a row pitch beyond its width whose mask has another
    pitch."""
    pages = [torch.from_numpy(m[0]).to(dev) for m in material]
    masks = [torch.from_numpy(m[1]).to(dev) for m in material]
    wide = torch.zeros((120, 131, 3), dtype=torch.uint8, device=dev)
    wide[:, 17:17 + 97] = pages[1]
    pages[1] = wide[:, 17:17 + 97]
    wm = torch.zeros((120, 160), dtype=torch.uint8, device=dev)
    wm[:, 40:40 + 97] = masks[1]
    masks[1] = wm[:, 40:40 + 97]
    assert pages[1].stride(0) == 393 and masks[1].stride(0) == 160 and not pages[1].is_contiguous()
    return pages, masks


class _Blk:
    def __init__(self, xyxy):
        self.xyxy = list(xyxy)


@pytest.mark.parametrize("kw", [dict(), dict(grow=0, ring=3, tol=0, min_ring=1), dict(grow=8, ring=16, tol=40, min_ring=300)],
                         ids=["defaults", "g0", "g8r16"])
def test_kernels_equal_the_restatement_in_every_field_and_byte(kw):
    """One `ctd_erase_text` call over pages of different sizes (61 x 83, 120 x 97 pitched, 33 x 150, 40 x 300, ...) against
    `erase_ref.erase_page`: all fields of all rows, all bytes of `out` and `rest`; with the default parameters, with g = 0 and
    with g + r = 24.  The same call twice gives identical bytes."""
    p = pkg()
    E = p.erase
    dev = torch.device("cuda:0")
    material = _material()
    pages, masks = _device_inputs(material, dev)
    lists = [[_Blk(b) for b in m[2]] for m in material]
    er = E.erase_text(pages, masks, lists, **kw)
    want = _compare(er, material, kw, str(kw))
    counts = [sum(w["status"] == s for w in want) for s in range(6)]
    print(f"\n{kw}: {len(want)} blocks on {len(material)} pages, status counts {counts}")
    assert all(counts), "all six statuses occur"
    if not kw:
        by_page = {}
        for (pg, b), w in zip(er.index.tolist(), want):
            by_page.setdefault(pg, []).append(w)
        n = len(material)
        three, mixed = by_page[7], by_page[8]
        assert [w["status"] for w in three] == [R.PLAIN] * 3 and len({tuple(w["med"]) for w in three}) == 3
        assert [w["status"] for w in mixed] == [R.PLAIN, R.TEXTURED, R.PLAIN]
        flat = [by_page[i][0] for i in range(10, 14)]
        assert [w["med"] for w in flat] == [c[3] for c in R.flat_cases()] and all(w["status"] == R.PLAIN for w in flat)
        assert [by_page[i][0]["status"] for i in range(14, 18)] == [R.PLAIN, R.TEXTURED, R.PLAIN, R.TEXTURED]
        assert by_page[18][0]["med"] == [100, 110, 110] and (n - 2) not in by_page
        assert er.plain.tolist() == [w["status"] == R.PLAIN for w in want] and er.fill.tolist() == [w["med"][::-1] for w in want]
    again = E.erase_text(pages, masks, lists, **kw)
    assert again.rows.tobytes() == er.rows.tobytes()
    assert all(torch.equal(a, b) for a, b in zip(again.pages + again.rest, er.pages + er.rest))


def test_no_blocks_copies_the_pages_and_no_pages_launches_nothing():
    p = pkg()
    E, L = p.erase, p._lib
    rng = np.random.default_rng(4)
    material = [(rng.integers(0, 256, (h, w, 3), dtype=np.uint8), (rng.random((h, w)) < 0.3).astype(np.uint8) * 9, [])
                for h, w in ((61, 83), (33, 150), (1, 1), (32, 64), (65, 129))]
    er = E.erase_text([m[0] for m in material], [m[1] for m in material], [[] for _ in material])
    assert len(er) == 0 and er.rows.shape == (0,)
    for (page, mask, _), out, rest in zip(material, *er.to_host()):
        assert np.array_equal(out, page) and np.array_equal(rest, np.where(mask != 0, 255, 0))
    _compare(er, material, {})
    prm = L.CtdEraseParams(2, 4, 12, 16, 0)
    assert L.lib().ctd_erase_text(None, 0, None, 0, C.byref(prm), None, None) == L.OK        # nothing to do, nothing launched
    assert len(E.erase_text([], [], [])) == 0


def test_a_box_over_the_cap_is_too_large_and_reads_nothing():
    """One block whose box grown by g + r holds more than 2^24 pixels, declared over a real allocation of 4097 x 4096:
    TOO_LARGE, the rest of the row 0, the page is copied; decided from xyxy, H and W before any load.  A box at the cap is
    computed."""
    p = pkg()
    E, L = p.erase, p._lib
    dev = torch.device("cuda:0")
    page = torch.zeros((4097, 4096, 3), dtype=torch.uint8, device=dev)
    mask = torch.zeros((4097, 4096), dtype=torch.uint8, device=dev)
    boxes = [(0, 0, 4096, 4097), (0, 0, 4096 - 12, 4096 - 11), (0, 0, 4096 - 12, 4096 - 12)]
    assert [R.box_status(b, 4097, 4096, 2, 4)[0] for b in boxes] == [R.TOO_LARGE, R.TOO_LARGE, None]
    er = E.erase_text([page], [mask], [[_Blk(b) for b in boxes]])
    assert er.status.tolist() == [L.ERASE_TOO_LARGE, L.ERASE_TOO_LARGE, L.ERASE_NO_MASK]
    assert not er.rows.view(np.uint8).reshape(3, -1)[:, 4:].any()
    assert not bool(er.pages[0].any()) and not bool(er.rest[0].any())


# ---- 2. erase_text on the tail's own results -------------------------------------------------------------------------------

def balloon_page(seed, size=256):
    """A small page for these tests: flat grey background, a noise panel (values 100 .. 255: no ink), three blocks of
    stroke-like glyphs -- two on white balloons with 12-pixel margins, one straight on the noise panel."""
    rng = np.random.RandomState(seed)
    img = np.full((size, size, 3), 230, np.uint8)
    half = size // 2
    img[half:, half:] = rng.randint(100, 256, (size - half, size - half, 3))
    fs = 14
    for x0, y0, nl, ln, balloon in ((20, 20, 2, 6, True), (24, half + 24, 3, 5, True), (half + 20, half + 30, 2, 5, False)):
        bw, bh = ln * fs, nl * int(fs * 1.5)
        if balloon:
            img[y0 - 12:y0 + bh + 12, x0 - 12:x0 + bw + 12] = 255
        for li in range(nl):
            for ci in range(ln):
                cx, cy = x0 + ci * fs, y0 + li * int(fs * 1.5) + fs // 4
                for _s in range(4):                               # a few strokes per glyph, as synth.text_like_page draws them
                    sx, sy = cx + rng.randint(0, fs - 4), cy + rng.randint(0, fs - 4)
                    if rng.rand() < 0.5:
                        img[sy:sy + max(2, fs // 8), sx:min(sx + fs // 2, cx + fs - 2)] = rng.randint(0, 40)
                    else:
                        img[sy:min(sy + fs // 2, cy + fs - 2), sx:sx + max(2, fs // 8)] = rng.randint(0, 40)
    return img


def outputs_for(page, seed):
    """Network outputs rendered from the page's ink, as tests/test_post_host.py `fake_outputs` renders them for its own page:
    (blks (1,rows,7), mask_u8, prob, mask f32 (1,1,H,W), lines_map (1,2,H,W))."""
    from oracle import cv_ref as cv, postproc_ref as P
    ink = page.min(axis=2) < 60
    mask_u8 = (cv.dilate((ink * 255).astype(np.uint8), cv.RECT3, 1).astype(np.float32) / 255 * 0.9 * 255).astype(np.uint8)
    prob = (cv.dilate((ink * 255).astype(np.uint8), cv.RECT3, 4) / 255.0 * 0.85 + 0.05).astype(np.float32)
    n, lab, stats = P.connected_components_with_stats(cv.dilate((ink * 255).astype(np.uint8), cv.RECT3, 10), 8)
    rng = np.random.RandomState(seed)
    blines = np.array([[x, y, x + w, y + h] for x, y, w, h, a in stats[1:]], np.int32).reshape(-1, 4)
    cls = rng.randint(0, 2, len(blines)).astype(np.int32)
    confs = np.round(rng.uniform(0.5, 1, len(blines)), 3)
    mask_f = (mask_u8.astype(np.float32) + 0.5) / 255
    return blks_tensor((blines, cls, confs)), mask_u8, prob, mask_f[None, None], np.stack([prob, np.zeros_like(prob)])[None]


_PAGES = {}


def tail_pages(size=256):
    """Two `balloon_page`s with what the ORACLE's tail makes of them on the CPU -- (page, mask_refined, boxes) -- chosen so
    that the restatement alone reports at least 2 PLAIN and at least 1 other block on them (asserted)."""
    if "cpu" not in _PAGES:
        from oracle import postproc_ref as P
        out, statuses = [], []
        for seed in (1, 3):
            page = balloon_page(seed, size)
            bt, mask_u8, prob, mask_f, lines_map = outputs_for(page, seed)
            _, refined, blks = P.detector_tail(page, bt, mask_f, lines_map, input_size=(size, size))
            boxes = [[int(v) for v in b.xyxy] for b in blks]
            statuses += [r["status"] for r in R.erase_page(page, refined, boxes)[0]]
            out.append((page, refined, boxes, (bt, mask_u8, prob)))
        assert sum(s == R.PLAIN for s in statuses) >= 2 and sum(s != R.PLAIN for s in statuses) >= 1, statuses
        _PAGES["cpu"] = out
    return _PAGES["cpu"]


def native_tail(size=256):
    """The native tail's (mask_refined, BlockList) of the pages of `tail_pages`."""
    if "gpu" not in _PAGES:
        p, det = pkg(), TG.detector()
        dev = det.net.device
        res = []
        for page, _, _, (bt, mask_u8, prob) in tail_pages(size):
            bitmap = (prob > 0.3).astype(np.uint8)
            gpu = [torch.from_numpy(page).to(dev)]
            torch.cuda.current_stream(dev).synchronize()
            r = p.tail.thread_tail(dev).run(gpu, [(size, size, 0, 0)], torch.from_numpy(bt).to(dev),
                                            torch.from_numpy(mask_u8)[None].to(dev), torch.from_numpy(prob)[None].to(dev),
                                            torch.from_numpy(bitmap)[None].to(dev), det.conf_thresh, det.nms_thresh, 0.6, True, 0,
                                            False, None, lazy=True)[0]
            res.append((r[1].copy(), r[2]))
        _PAGES["gpu"] = res
    return _PAGES["gpu"]


def test_erase_text_on_the_tails_blocks_equals_the_restatement():
    """`erase.erase_text` with the native tail's `mask_refined` and blk_lists of two pages: rows, pages and rest equal the
    restatement for `BlockList` (no `TextBlock` built) and list input, host and device pages and masks, and on a side
    stream; at least 2 PLAIN blocks and 1 other."""
    p = pkg()
    E, L = p.erase, p._lib
    cpu = tail_pages()
    gpu = native_tail()
    pages, masks, lazies = [c[0] for c in cpu], [g[0] for g in gpu], [g[1] for g in gpu]
    assert all(m.any() for m in masks)
    built = [z._built is not None for z in lazies]
    er = E.erase_text(pages, masks, lazies)
    assert all(b or z._built is None for b, z in zip(built, lazies))            # read from the records
    lists = [z.to_list() for z in lazies]
    material = [(pg, m, [[int(v) for v in b.xyxy] for b in bl]) for pg, m, bl in zip(pages, masks, lists)]
    want = _compare(er, material, {})
    statuses = [w["status"] for w in want]
    print(f"\n{len(want)} blocks, statuses {statuses}")
    assert sum(s == R.PLAIN for s in statuses) >= 2 and sum(s != R.PLAIN for s in statuses) >= 1
    assert er.status.tolist() == statuses and er.plain.tolist() == [s == R.PLAIN for s in statuses]
    assert er.fill.tolist() == [w["med"][::-1] for w in want]                   # RGB
    # the filled pixels are the plain blocks' glyphs, and what is left to inpaint is the other block
    host_pages, host_rest = er.to_host()
    for (pg, m, _), out, rest in zip(material, host_pages, host_rest):
        changed = (out != pg).any(axis=2)
        assert changed.any() and rest.any() and not (changed & (rest != 0)).any()
    dev = torch.device("cuda:0")
    dp, dm = [torch.from_numpy(x).to(dev) for x in pages], [torch.from_numpy(x).to(dev) for x in masks]
    for other in (E.erase_text(pages, masks, lists), E.erase_text(dp, dm, lists), E.erase_text(dp, masks, lazies),
                  E.erase_text(pages, dm, lists, stream=torch.cuda.Stream(dev)),
                  E.erase_text(pages, masks, [(None, None, bl) for bl in lists])):
        assert np.array_equal(other.rows, er.rows) and np.array_equal(other.index, er.index)
        assert all(torch.equal(a, b) for a, b in zip(other.pages + other.rest, er.pages + er.rest))


# ---- 3. through the detector ---------------------------------------------------------------------------------------------------

def test_detector_erase_text_equals_the_restatement():
    """`det.erase_text(pages, det.detect_batch(pages))` against the restatement on the same masks and boxes, for list and lazy
    results and device pages."""
    p, det = pkg(), TG.detector()
    pages = [p.synth.text_like_page((256, 256), 3, n_blocks=4), p.synth.text_like_page((200, 300), 4, n_blocks=2),
             p.synth.text_like_page((256, 256), 5, n_blocks=3)]
    results = det.detect_batch(pages)
    assert sum(len(r[2]) for r in results) >= 4
    er = det.erase_text(pages, results)
    material = [(pg, r[1], [[int(v) for v in b.xyxy] for b in r[2]]) for pg, r in zip(pages, results)]
    want = _compare(er, material, {})
    assert len(want) == sum(len(r[2]) for r in results)
    print(f"\nstatuses {[w['status'] for w in want]}")
    other = det.erase_text([torch.from_numpy(x).cuda() for x in pages], results, grow=3, ring=5)
    _compare(other, material, dict(grow=3, ring=5))
    with pytest.raises(ValueError):
        det.erase_text(pages, results, ring=0)


def test_model2annotations_writes_the_erased_pages_on_request(tmp_path):
    """`model2annotations(erase=True)` writes `clean-<name>.png` and `rest-<name>.png` that decode to `.pages` and `.rest` of
    `erase_text` on the same detection; the default writes the file set it always wrote."""
    p, det = pkg(), TG.detector()
    A = p.annotations
    src = tmp_path / "pages"
    src.mkdir()
    pages = {"a.png": p.synth.text_like_page((256, 256), 3, n_blocks=4), "b.png": p.synth.text_like_page((256, 256), 5, n_blocks=3)}
    for name, img in pages.items():
        (src / name).write_bytes(A.png_bytes(img))
    sets = {}
    for flag in (False, True):
        out = tmp_path / f"out{int(flag)}"
        assert A.model2annotations(None, str(src), str(out), save_json=True, batch_size=2, detector=det, erase=flag) == 2
        sets[flag] = sorted(os.listdir(out))
    assert sets[True] == sorted(sets[False] + ["clean-a.png", "clean-b.png", "rest-a.png", "rest-b.png"])
    for name in pages:                                            # today's files: what `page_files` lists, nothing else
        stem = name[:-4]
        assert {f"{stem}.txt", f"{stem}.json", f"{stem}.png", f"mask-{stem}.png"} <= set(sets[False])
    assert not any(f.startswith(("clean-", "rest-")) for f in sets[False])
    imgs = list(pages.values())
    results = det.detect_batch(imgs, refine_mode=p.textmask.REFINEMASK_ANNOTATION, keep_undetected_mask=True)
    er = det.erase_text(imgs, results)
    for name, img, clean, rest in zip(pages, imgs, *er.to_host()):
        got_clean = A.imread(str(tmp_path / "out1" / f"clean-{name}"))
        from PIL import Image
        got_rest = np.asarray(Image.open(tmp_path / "out1" / f"rest-{name}"))
        assert np.array_equal(got_clean, clean) and np.array_equal(got_rest, rest)
    for f in sets[False]:                                         # the files both runs write are the same bytes
        assert (tmp_path / "out0" / f).read_bytes() == (tmp_path / "out1" / f).read_bytes()


# ---- 4. bad arguments --------------------------------------------------------------------------------------------------------

def test_bad_arguments_are_refused_without_a_launch():
    p = pkg()
    E, L = p.erase, p._lib
    dev = torch.device("cuda:0")
    page = torch.zeros((20, 30, 3), dtype=torch.uint8, device=dev)
    mask = torch.zeros((20, 30), dtype=torch.uint8, device=dev)
    blk = _Blk((2, 3, 20, 15))
    for bad in (dict(grow=-1), dict(grow=9), dict(ring=0), dict(ring=17), dict(tol=-1), dict(tol=256), dict(min_ring=0)):
        with pytest.raises(ValueError):
            E.erase_text([page], [mask], [[blk]], **bad)
    for pg, mk in ((page[:, :, 0], mask), (page, mask[:, :29]), (page.int(), mask), (page, mask[:19])):
        with pytest.raises(ValueError):
            E.erase_text([pg], [mk], [[blk]])
    with pytest.raises(ValueError):
        E.erase_text([page, page], [mask], [[blk], []])
    with pytest.raises(ValueError):
        E.erase_text([page], [mask], [[_Blk((1.5, 2, 3, 4))]])
    # the entry point itself: an error rc, nothing launched (the tables it is given do not exist)
    lib = L.lib()
    ok = (2, 4, 12, 16, 1)
    for vals in ((-1, 4, 12, 16, 1), (9, 4, 12, 16, 1), (2, 0, 12, 16, 1), (2, 17, 12, 16, 1), (2, 4, -1, 16, 1), (2, 4, 256, 16, 1),
                 (2, 4, 12, 0, 1), (2, 4, 12, 16, -1)):
        prm = L.CtdEraseParams(*vals)
        assert lib.ctd_erase_text(8, 1, 8, 1, C.byref(prm), 8, None) != L.OK, vals
    prm = L.CtdEraseParams(*ok)
    assert lib.ctd_erase_text(8, -1, 8, 1, C.byref(prm), 8, None) != L.OK
    assert lib.ctd_erase_text(8, 1, 8, -1, C.byref(prm), 8, None) != L.OK
    assert lib.ctd_erase_text(8, 1, 8, 0, C.byref(prm), 8, None) != L.OK                  # blocks without pages
    assert lib.ctd_erase_text(8, 1, 8, 1, None, 8, None) != L.OK
    assert lib.ctd_erase_text(None, 1, 8, 1, C.byref(prm), 8, None) != L.OK
    assert lib.ctd_erase_text(8, 1, None, 1, C.byref(prm), 8, None) != L.OK
    assert lib.ctd_erase_text(8, 1, 8, 1, C.byref(prm), None, None) != L.OK
    torch.cuda.synchronize()
