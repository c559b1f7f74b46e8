"""-m gpu: font colours -- `ctd_line_colors` (csrc/kernels_color.hip), `colors.line_colors`, `TextDetector.font_colors` and
the `font_colors=True` option of `detect_batch` / `detect_stream` -- against the numpy restatement tests/color_ref.py.  The rule
is integers only, so every comparison is EXACT: every field of every row."""
import numpy as np
import pytest
import torch

import color_ref as R
import test_gpu_regions as TG
from conftest import pkg
from sweep_cases import tail_case

pytestmark = pytest.mark.gpu


# ---- 1. the kernel ---------------------------------------------------------------------------------------------------------

def _rect(x, y, w, h):
    """Axis-aligned quad covering w x h pixels from (x, y), detector order (clockwise from the top left)."""
    return [x, y, x + w - 1, y, x + w - 1, y + h - 1, x, y + h - 1]


def _kernel_material():
    """(images, (image index, mask) pairs, jobs = (pair index, quad)).  Pages of different sizes; masks all zero, all on and
    random at densities 0.02 / 0.5 / 0.98; a constant page and a random grey page (B = G = R); the flat pages of the CPU test."""
    rng = np.random.default_rng(21)
    shapes = [(61, 83), (120, 97), (33, 150), (40, 300)]          # the last: room for rows of 255 .. 257 pixels
    imgs = [rng.integers(0, 256, s + (3,), dtype=np.uint8) for s in shapes]
    imgs.append(np.full((50, 70, 3), 117, np.uint8))              # 4: every pixel equal: the means tie
    imgs.append(np.repeat(rng.integers(0, 256, (50, 70, 1), dtype=np.uint8), 3, axis=2))       # 5: B = G = R, random
    pairs = []
    for i, im in enumerate(imgs):
        h, w = im.shape[:2]
        pairs.append((i, (rng.random((h, w)) < 0.5).astype(np.uint8) * rng.integers(1, 256, (h, w), dtype=np.uint8)))
    base = len(pairs)
    for i in (0, 1, 2):
        h, w = imgs[i].shape[:2]
        pairs += [(i, np.zeros((h, w), np.uint8)), (i, np.full((h, w), 255, np.uint8)),
                  (i, (rng.random((h, w)) < 0.02).astype(np.uint8) * 255), (i, (rng.random((h, w)) < 0.98).astype(np.uint8))]
    away = [-500, -400, -450, -400, -450, -380, -500, -380]
    jobs = [(0, away)]
    for pi in range(len(imgs)):                                   # per page with its half-density mask
        H, W = imgs[pi].shape[:2]
        jobs += [(pi, _rect(5, 7, 1, 1)), (pi, _rect(3, 2, 1, H - 4)), (pi, _rect(2, 3, W - 4, 1))]
        jobs += [(pi, _rect(1 + k, 1 + k, k, 9)) for k in range(1, 10)]                        # rows of 1 .. 9 pixels
        jobs += [(pi, _rect(2, 4, k, 5)) for k in (63, 64, 65) if k + 2 <= W]
        jobs += [(pi, _rect(1, 6, k, 3)) for k in (255, 256, 257) if k + 1 <= W]
        jobs.append((pi, _rect(0, 0, W, H)))                      # the whole page
        q = _rect(4, 3, W - 9, H - 7)
        jobs += [(pi, q), (pi, q[6:8] + q[4:6] + q[2:4] + q[0:2])]                             # both windings
        # outside: partly and wholly beyond every edge and corner
        jobs += [(pi, _rect(-10, 5, 25, 9)), (pi, _rect(W - 8, 5, 30, 9)), (pi, _rect(5, -6, 20, 11)), (pi, _rect(5, H - 4, 20, 11)),
                 (pi, _rect(-7, -5, 15, 12)), (pi, _rect(W - 6, -5, 15, 12)), (pi, _rect(-7, H - 5, 15, 12)),
                 (pi, _rect(W - 6, H - 5, 15, 12)), (pi, _rect(-30, 5, 20, 9)), (pi, _rect(W, 5, 20, 9)), (pi, _rect(5, -20, 20, 11)),
                 (pi, _rect(5, H, 20, 11)), (pi, _rect(-40, -40, 30, 30)), (pi, _rect(W + 3, H + 3, 30, 30)),
                 (pi, _rect(-W, -H, 3 * W, 3 * H))]
        # tilted: a band of half-width t about a centre line at several angles (45 degrees among them), both windings by sign
        cx, cy = W / 2, H / 2
        for deg, half_len, t in ((45, 0.6 * min(H, W), 6), (20, 0.45 * W, 4), (-33, 0.5 * W, 9), (80, 0.6 * H, 5), (135, 40, 3),
                                 (7, 0.7 * W, 0.3), (45, 30, 0.2)):                            # the last two: thinner than a pixel
            a = np.deg2rad(deg)
            u, v = np.array([np.cos(a), np.sin(a)]) * half_len, np.array([-np.sin(a), np.cos(a)]) * t
            c = np.array([cx, cy])
            jobs.append((pi, np.rint(np.array([c - u - v, c + u - v, c + u + v, c - u + v])).astype(int).reshape(8).tolist()))
        jobs.append((pi, [10, 5, 10, 5, 40, 30, 40, 30]))         # degenerate: two points twice, a segment
        jobs.append((pi, [5, 5, 40, 30, 40, 5, 5, 30]))           # self-intersecting
        if pi == 2:
            jobs.append((0, away))                                # an empty job in the middle
    for k in range(base, len(pairs)):                             # the other masks
        H, W = pairs[k][1].shape
        jobs += [(k, _rect(3, 4, W - 7, H - 9)), (k, [2, H // 2, W // 2, 1, W - 3, H // 2, W // 2, H - 2]), (k, _rect(-3, -3, 20, 20))]
    # a grey EXACTLY at the midpoint of the two means (ON greys 110 / 90 / 75 / 125 in equal numbers: mean 100; OFF all 50:
    # midpoint 75; OFF all 150: midpoint 125) is not text-like: the comparison is strict, in both directions
    mm = np.zeros((20, 40), np.uint8)
    mm[:, :20] = 1
    for off in (50, 150):
        mid = np.full((20, 40, 3), off, np.uint8)
        mid[:, :20] = np.tile(np.array([110, 90, 75, 125], np.uint8), 5)[None, :, None]
        imgs.append(mid)
        pairs.append((len(imgs) - 1, mm))
        jobs += [(len(pairs) - 1, _rect(0, 0, 40, 20)), (len(pairs) - 1, _rect(2, 1, 33, 17))]
    jobs.append((1, _rect(3, 5, 90, 30)))                         # 2700 pixels, more than 256 x 8; one round of the 512 x 8 kernel
    jobs.append((1, _rect(2, 3, 93, 100)))                        # 9300 box pixels: three rounds, pass 2 re-seeks past the first
    jobs.append((1, [4, 20, 80, 2, 94, 60, 18, 116]))             # tilted, box 91 x 115 = 10465: rounds with pixels outside the quad
    jobs.append((0, [0, 0, R.MAX_COORD + 1, 0, 50, 50, 0, 50]))   # a coordinate beyond the cap: TOO_LARGE, nothing read
    jobs.append((0, [0, 0, R.MAX_COORD, 0, 50, 50, 0, 50]))       # at the cap: computed
    flat = {}
    for page, mask, quad, _, _ in R.flat_cases():                 # the flat pages of tests/test_color_ref.py
        key = (page.tobytes(), mask.tobytes())
        if key not in flat:
            imgs.append(page)
            pairs.append((len(imgs) - 1, mask))
            flat[key] = len(pairs) - 1
        jobs.append((flat[key], quad))
    jobs.append((2, away))
    return imgs, pairs, jobs


def _compare(rows, want, what):
    bad = []
    for i, (row, ref) in enumerate(zip(rows, want)):
        got = R.row_dict(row)
        if got != ref or row["pad_"].any():
            bad.append((i, what(i), {k: (got[k], ref[k]) for k in R.FIELDS if got[k] != ref[k]}))
    assert not bad, f"{len(bad)} of {len(want)} rows differ, first: {bad[:3]}"


def test_kernel_rows_equal_the_restatement_in_every_field():
    """`ctd_line_colors` against `color_ref.line_color`: all fields of all rows, one launch over pages of different sizes, one
    of them a view with a row pitch beyond its width whose mask has another pitch."""
    p = pkg()
    CO, L = p.colors, p._lib
    dev = torch.device("cuda:0")
    imgs, pairs, jobs = _kernel_material()
    pages_dev = [torch.from_numpy(im).to(dev) for im in imgs]
    wide = torch.zeros((120, 131, 3), dtype=torch.uint8, device=dev)
    wide[:, 17:17 + 97] = pages_dev[1]
    pages_dev[1] = wide[:, 17:17 + 97]
    pages, masks = [], []
    for i, m in pairs:
        pages.append(pages_dev[i])
        md = torch.from_numpy(m).to(dev)
        if i == 1:
            wm = torch.zeros((120, 160), dtype=torch.uint8, device=dev)
            wm[:, 40:40 + 97] = md
            md = wm[:, 40:40 + 97]
        masks.append(md)
    pages = p.regions._device_pages(pages, dev)[0]
    masks = p.regions._device_pages(masks, dev)[0]
    assert not pages[1].is_contiguous() and pages[1].stride(0) == 393 and masks[1].stride(0) == 160   # read through the pitch
    rows = CO.color_rows(pages, masks, [j[0] for j in jobs], [j[1] for j in jobs])
    assert rows.dtype == CO.OUT_DTYPE and len(rows) == len(jobs)
    want = [R.line_color(imgs[pairs[k][0]], pairs[k][1], q) for k, q in jobs]
    _compare(rows, want, lambda i: jobs[i])
    seen = {w["status"] for w in want}
    assert seen == {R.OK, R.EMPTY, R.NO_MASK, R.NO_CONTRAST, R.TOO_LARGE}
    assert want[0]["status"] == want[-1]["status"] == R.EMPTY
    print(f"\n{len(jobs)} jobs on {len(pairs)} page / mask pairs, {sum(w['n_on'] + w['n_off'] for w in want)} inside pixels, "
          f"status counts {[sum(w['status'] == s for w in want) for s in range(5)]}")
    # the flat pages come back as their two colours
    k = len(jobs) - 1 - len(list(R.flat_cases()))
    for row, (_, _, _, text, back) in zip(rows[k:], R.flat_cases()):
        assert row["status"] == L.COLOR_OK and row["fg"].tolist() == text and row["bg"].tolist() == back
    # n = 0 launches nothing; only empty jobs
    assert L.lib().ctd_line_colors(None, 0, None, None) == L.OK
    assert L.lib().ctd_line_colors(None, -1, None, None) != L.OK
    assert len(CO.color_rows(pages, masks, [], np.zeros((0, 8)))) == 0
    only = CO.color_rows(pages, masks, [0, 2], [jobs[0][1], jobs[0][1]])
    assert (only["status"] == L.COLOR_EMPTY).all() and not only.view(np.uint8).reshape(2, -1)[:, :80].any()


def test_a_box_over_the_cap_is_too_large_and_reads_nothing():
    """One job whose clipped box holds 4097 x 4096 > 2^24 pixels, declared over a real allocation of that size: TOO_LARGE,
    the rest of the row 0 -- decided from the quad, H and W before any load."""
    p = pkg()
    dev = torch.device("cuda:0")
    page = torch.zeros((4097, 4096, 3), dtype=torch.uint8, device=dev)
    mask = torch.zeros((4097, 4096), dtype=torch.uint8, device=dev)
    quads = [[0, 0, 4095, 0, 4095, 4096, 0, 4096]]
    rows = p.colors.color_rows([page], [mask], [0], quads)
    ref = R.line_color(np.lib.stride_tricks.as_strided(np.zeros((1, 1, 3), np.uint8), (4097, 4096, 3), (0, 0, 1)),
                       np.lib.stride_tricks.as_strided(np.zeros((1, 1), np.uint8), (4097, 4096), (0, 0)), quads[0])
    assert ref["status"] == R.TOO_LARGE
    _compare(rows, [ref], lambda i: quads[i])
    # one row fewer is exactly the cap: computed (a page of zeros without a mask: NO_MASK)
    rows = p.colors.color_rows([page], [mask], [0], [[0, 0, 4095, 0, 4095, 4095, 0, 4095]])
    assert rows["status"][0] == p._lib.COLOR_NO_MASK and rows["n_off"][0] == 1 << 24 and rows["g_off"][0] == 0


# ---- 2. line_colors on the tail's own blocks -------------------------------------------------------------------------------

_TAIL = {}


def tail_result(seed, size=512):
    """(page, mask_refined, BlockList) of the native tail on rendered network outputs, as tests/test_gpu_regions.py
    `tail_page` runs it: seeds 1 and 2 at 512 give vertical and horizontal blocks."""
    if seed not in _TAIL:
        p, det = pkg(), TG.detector()
        dev = det.net.device
        page, bt, mask_u8, prob = tail_case(seed, size)[:4]
        bitmap = (prob > 0.3).astype(np.uint8)
        gpu = [torch.from_numpy(page).to(dev)]
        torch.cuda.current_stream(dev).synchronize()
        r = p.tail.thread_tail(dev).run(gpu, [(size, size, 0, 0)], torch.from_numpy(bt).to(dev), torch.from_numpy(mask_u8)[None].to(dev),
                                        torch.from_numpy(prob)[None].to(dev), torch.from_numpy(bitmap)[None].to(dev),
                                        det.conf_thresh, det.nms_thresh, 0.6, True, 0, False, None, lazy=True)[0]
        _TAIL[seed] = (page, r[1].copy(), r[2])
    return _TAIL[seed]


def _reference(pages, masks, lists):
    """(index, rows) of the restatement for lists of `TextBlock`s, in `line_colors`' order."""
    index, rows = [], []
    for pg, (page, mask, blks) in enumerate(zip(pages, masks, lists)):
        for b, blk in enumerate(blks):
            for ln, quad in enumerate(blk.lines):
                index.append((pg, b, ln))
                rows.append(R.line_color(page, mask, np.asarray(quad).reshape(8)))
    return index, rows


def _pooled_reference(index, rows):
    out = {}
    for (pg, b, _), r in zip(index, rows):
        out.setdefault((pg, b), []).append(r)
    return {k: R.pooled(v) for k, v in out.items()}


def _check_blocks(lists, pooled):
    """Every block's `get_font_colors()` is the pooled reference; a block without a valid line is all zero."""
    n = 0
    for (pg, b), (ok, fg, bg) in pooled.items():
        blk = lists[pg][b]
        if ok:
            got_fg, got_bg = blk.get_font_colors()
            assert got_fg.tolist() == fg and got_bg.tolist() == bg, (pg, b, got_fg, fg, got_bg, bg)
            want_sw = blk.default_stroke_width if sum(abs(x - y) for x, y in zip(fg, bg)) * len(blk.lines) > 40 else 0
            assert blk.stroke_width == want_sw
            n += 1
        else:
            assert [blk.fg_r, blk.fg_g, blk.fg_b, blk.bg_r, blk.bg_g, blk.bg_b] == [0] * 6
    return n


def test_line_colors_on_the_tails_blocks_equal_the_restatement():
    """`colors.line_colors` with the tail's `mask_refined` and blk_lists of two pages: all columns equal the restatement for
    list and `BlockList` input (no `TextBlock` built for the latter) and for host and device pages and masks; after `apply`
    every block's `get_font_colors()` is the pooled reference."""
    p = pkg()
    CO, L = p.colors, p._lib
    (page_a, mask_a, lazy_a), (page_b, mask_b, lazy_b) = tail_result(1), tail_result(2)
    pages, masks = [page_a, page_b], [mask_a, mask_b]
    assert mask_a.any() and mask_b.any()
    built = lazy_a._built is not None
    lc = CO.line_colors(pages, masks, [lazy_a, lazy_b])
    assert built or lazy_a._built is None                         # read from the records
    lists = [lazy_a.to_list(), lazy_b.to_list()]
    index, want = _reference(pages, masks, lists)
    assert len(lc) == len(want) >= 40 and lc.index.tolist() == [list(i) for i in index]
    _compare(lc.rows, want, lambda i: index[i])
    assert lc.fg.tolist() == [w["fg"][::-1] for w in want] and lc.bg.tolist() == [w["bg"][::-1] for w in want]   # RGB
    for col in ("status", "n_on", "n_off", "n_fg", "n_bg"):
        assert getattr(lc, col).tolist() == [w[col] for w in want]
    n_ok = sum(w["status"] == R.OK for w in want)
    kinds = {(b.language, bool(b.vertical)) for bl in lists for b in bl}
    print(f"\n{len(want)} lines, {n_ok} OK, status counts {[sum(w['status'] == s for w in want) for s in range(5)]}, kinds {sorted(kinds)}")
    assert n_ok >= len(want) // 2 and any(v for _, v in kinds) and any(not v for _, v in kinds)
    dev = torch.device("cuda:0")
    dp, dm = [torch.from_numpy(x).to(dev) for x in pages], [torch.from_numpy(x).to(dev) for x in masks]
    for other in (CO.line_colors(pages, masks, lists), CO.line_colors(dp, dm, lists), CO.line_colors(dp, masks, [lazy_a, lazy_b]),
                  CO.line_colors(pages, dm, lists, stream=torch.cuda.Stream(dev))):
        assert np.array_equal(other.rows, lc.rows) and np.array_equal(other.index, lc.index)
    pooled = _pooled_reference(index, want)
    bc = lc.apply(lists)
    assert [tuple(k) for k in bc.index.tolist()] == list(pooled) and bc.valid.tolist() == [v[0] for v in pooled.values()]
    assert _check_blocks(lists, pooled) >= 4
    with pytest.raises(ValueError):
        CO.line_colors(dp, [dm[0], dm[1][:, :500]], lists)
    with pytest.raises(ValueError):
        CO.line_colors([dp[0], dp[1][:, :, 0]], dm, lists)


# ---- 3. through the detector ---------------------------------------------------------------------------------------------------

def _colour_fields(results):
    return [[int(getattr(b, k)) for k in ("fg_r", "fg_g", "fg_b", "bg_r", "bg_g", "bg_b")] for r in results for b in r[2]]


def test_detector_font_colors_option():
    """`detect_batch(font_colors=True)` and `detect_stream(font_colors=True)` fill the blocks with what
    `font_colors(pages, plain results, apply=False).blocks()` and the restatement give on the same masks; the default leaves
    every colour field 0; `lazy=True` with `font_colors=True` raises."""
    p, det = pkg(), TG.detector()
    pages = [p.synth.text_like_page((256, 256), 3, n_blocks=4), p.synth.text_like_page((200, 300), 4, n_blocks=2),
             p.synth.text_like_page((256, 256), 5, n_blocks=3)]
    plain = det.detect_batch(pages)
    assert sum(len(r[2]) for r in plain) >= 4
    assert all(v == [0] * 6 for v in _colour_fields(plain))                       # exactly as today
    lc = det.font_colors(pages, plain, apply=False)
    assert all(v == [0] * 6 for v in _colour_fields(plain)) and len(lc) == sum(len(b.lines) for r in plain for b in r[2])
    bc = lc.blocks()
    index, want = _reference(pages, [r[1] for r in plain], [r[2] for r in plain])
    _compare(lc.rows, want, lambda i: index[i])
    pooled = _pooled_reference(index, want)
    assert [tuple(k) for k in bc.index.tolist()] == list(pooled)
    assert [(bool(v), f, b) for v, f, b in zip(bc.valid.tolist(), bc.fg.tolist(), bc.bg.tolist())] == list(pooled.values())
    n_valid = sum(v[0] for v in pooled.values())
    assert n_valid >= 3

    def same(results):
        assert len(results) == len(plain)
        for r, q in zip(results, plain):
            assert np.array_equal(r[0], q[0]) and np.array_equal(r[1], q[1]) and len(r[2]) == len(q[2])
            assert [b.lines for b in r[2]] == [b.lines for b in q[2]]
        assert _check_blocks([r[2] for r in results], pooled) == n_valid

    same(det.detect_batch(pages, font_colors=True))
    got = list(det.detect_stream([pages], workers=2, depth=2, tail_split=2, tune=False, font_colors=True))
    assert len(got) == 1
    same(got[0])
    (res, batches), = list(det.detect_stream([pages], workers=2, depth=2, tail_split=2, tune=False, font_colors=True, line_batches={}))
    same(res)
    assert len(batches) == 2
    stream_plain = list(det.detect_stream([pages], workers=2, depth=2, tail_split=2, tune=False))[0]
    assert all(v == [0] * 6 for v in _colour_fields(stream_plain))
    with pytest.raises(ValueError):
        list(det.detect_stream([pages], workers=2, lazy=True, font_colors=True))
    # apply=True on the plain results: the same colours, host or device pages
    det.font_colors([torch.from_numpy(x).cuda() for x in pages], plain)
    same(plain)


def test_model2annotations_writes_the_colours_on_request(tmp_path):
    """`model2annotations(font_colors=True)`: the JSON records carry the colour sums `detect_batch(font_colors=True)` stores,
    in the detector's refine mode for annotations; the default writes zeros."""
    import json
    p, det = pkg(), TG.detector()
    A = p.annotations
    src = tmp_path / "pages"
    src.mkdir()
    pages = {"a.png": p.synth.text_like_page((256, 256), 3, n_blocks=4), "b.png": p.synth.text_like_page((256, 256), 5, n_blocks=3)}
    for name, img in pages.items():
        (src / name).write_bytes(A.png_bytes(img))
    keys = ("fg_r", "fg_g", "fg_b", "bg_r", "bg_g", "bg_b")
    for flag in (False, True):
        out = tmp_path / f"out{int(flag)}"
        assert A.model2annotations(None, str(src), str(out), save_json=True, batch_size=2, detector=det, font_colors=flag) == 2
        n = 0
        for name, img in pages.items():
            recs = json.loads((out / name.replace(".png", ".json")).read_text())
            want = det.detect_batch([img], refine_mode=p.textmask.REFINEMASK_ANNOTATION, keep_undetected_mask=True, font_colors=flag)[0][2]
            assert len(recs) == len(want) >= 1
            assert [[r[k] for k in keys] for r in recs] == [[int(getattr(b, k)) for k in keys] for b in want]
            n += sum(any(r[k] for k in keys) for r in recs)
        assert (n >= 2) if flag else (n == 0)
