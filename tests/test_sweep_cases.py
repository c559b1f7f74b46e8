"""The case generators of the GPU sweeps (tests/sweep_cases.py) checked WITHOUT a GPU, from the oracle alone: the same
(case, seed) gives the same bytes, the ranges that tests/test_gpu_sweeps.py and tests/test_gpu_e2e.py run are not vacuous
(floors on blocks, lines, boxes, candidates, ties -- a later edit of a generator cannot quietly empty a sweep), and the compare
helpers of the sweeps report a case whose result is the oracle's own with ONE perturbation, and only that case."""
import copy
import functools

import numpy as np
import pytest

import sweep_cases as S
import test_gpu_sweeps as G
from oracle import postproc_ref as R


def _bytes(x):
    if isinstance(x, np.ndarray):
        return x.dtype.str.encode() + repr(x.shape).encode() + x.tobytes()
    if isinstance(x, (tuple, list)):
        return b"|".join(_bytes(v) for v in x)
    return repr(x).encode()


@pytest.mark.parametrize("gen,cases", [(S.nms_case, (0, 5, 7)), (S.db_map, (0, 1, 2, 3)), (S.ccl_image, (0, 1, 2, 3)),
                                       (S.resize_case, (0, 1, 2)), (S.tied_pixels, tuple(range(12)))])
def test_generators_are_deterministic(gen, cases):
    for case in cases:
        a, b = gen(case, np.random.RandomState(11 + case)), gen(case, np.random.RandomState(11 + case))
        assert _bytes(a) == _bytes(b)
        assert _bytes(a) != _bytes(gen(case, np.random.RandomState(12 + case))) or gen is S.tied_pixels   # the seed matters


def test_seeded_cases_and_whole_sweeps_are_deterministic():
    assert _bytes(S.tail_case(1000, 256)) == _bytes(S.tail_case(1000, 256))
    assert _bytes(S.letterbox_tail_case(2000)) == _bytes(S.letterbox_tail_case(2000))
    assert _bytes(S.tail_batch32(0, 7000, 256)[:2]) == _bytes(S.tail_batch32(0, 7000, 256)[:2])
    for sweep in (S.ccl_sweep, S.tied_sweep, functools.partial(S.db_sweep, 32), functools.partial(S.resize_sweep, 20),
                  functools.partial(S.mixed_size_batches, 2)):
        assert _bytes(list(sweep())) == _bytes(list(sweep()))


# ------------------------------------------------------------------------------------------------------------- the floors

@functools.lru_cache(None)
def _tail_sweep_refs():
    from test_gpu_e2e import TAIL_SWEEP_DEFAULT
    first, last, size = TAIL_SWEEP_DEFAULT
    out = []
    for seed in range(first, last + 1):
        page, bt, mask_u8, prob, mask_f, lines_map, what = S.tail_case(seed, size)
        out.append(G.oracle_tail((page, bt, mask_f, lines_map), size, bool(seed & 1)))
    return out


def test_tail_sweep_default_range_is_not_vacuous():
    """Seeds 1000 .. 1023 at 1024 (measured: 220 blocks, 1 904 lines, no page below 4 blocks)."""
    refs = _tail_sweep_refs()
    blocks = [len(r[2]) for r in refs]
    lines = sum(len(b.lines) for r in refs for b in r[2])
    assert len(refs) == 24 and min(blocks) >= 1 and sum(blocks) >= 150 and lines >= 1500, (blocks, lines)
    assert all((r[1] > 0).any() for r in refs)                       # every page refines some mask


@functools.lru_cache(None)
def _letterbox_sweep_refs():
    from test_gpu_e2e import LETTERBOX_SWEEP_DEFAULT
    first, last = LETTERBOX_SWEEP_DEFAULT
    out = []
    for seed in range(first, last + 1):
        page, bt, mask, lines_map, (dw, dh), what = S.letterbox_tail_case(seed)
        out.append((page.shape[:2], G.oracle_tail((page, bt, mask, lines_map), S.LETTERBOX_SIZE, bool(seed & 1), dw, dh)))
    return out


def test_letterbox_sweep_default_range_is_not_vacuous():
    """Seeds 2000 .. 2023 (measured: 181 blocks, 825 lines, 11 portrait pages, 2 smaller than the network input)."""
    refs = _letterbox_sweep_refs()
    blocks = [len(r[2]) for _, r in refs]
    portrait = sum(h > w for (h, w), _ in refs)
    landscape = sum(w > h for (h, w), _ in refs)
    upscaled = sum(max(h, w) < S.LETTERBOX_SIZE for (h, w), _ in refs)
    assert len(refs) == 24 and min(blocks) >= 1 and sum(blocks) >= 120, blocks
    assert portrait >= 8 and landscape >= 8 and upscaled >= 1, (portrait, landscape, upscaled)


@functools.lru_cache(None)
def _db_sweep_refs():
    out = []
    for call in S.db_sweep():
        for case, pr, what in call:
            out.append((case, what, pr, R.boxes_from_bitmap(pr, pr > 0.3, pr.shape[1], pr.shape[0])))
    return out


def test_db_sweep_is_not_vacuous():
    """200 maps: every one yields a box; the two sparse kinds (rotated bars, blobs with holes) at least 100 each in total."""
    refs = _db_sweep_refs()
    assert [c for c, _, _, _ in refs] == list(range(200))
    per_kind = [0, 0, 0, 0]
    for case, what, pr, (boxes, scores) in refs:
        assert len(boxes) >= 1, what
        per_kind[case % 4] += len(boxes)
    assert per_kind[1] >= 100 and per_kind[2] >= 100, per_kind
    calls = list(S.db_sweep())
    batched = [c for c in calls if len(c) > 1]
    assert sum(len(c) for c in batched) >= 20 and all(len(c) == 8 and len({m.shape for _, m, _ in c}) == 1 for c in batched)
    assert {case % 4 for c in batched for case, _, _ in c} == {0, 1, 2, 3}


def test_tail_batch32_pages_are_not_vacuous():
    """16 of the 64 pages of `test_tail_on_32_different_pages_per_call` (measured: 133 blocks, 996 lines); the floor of 400
    blocks over 64 pages scaled to 100 over 16."""
    size = 512
    pages = S.tail_batch32(0, 7000, size)[:16]
    refs = [G.oracle_tail((c[0], c[1], c[4], c[5]), size, False) for c in pages]
    assert sum(len(r[2]) for r in refs) >= 100 and sum(len(b.lines) for r in refs for b in r[2]) >= 700
    assert len({c[1].shape for c in S.tail_batch32(1, 7000, 256)}) == 1            # one row count per call


@functools.lru_cache(None)
def _nms_sweep_refs():
    return [(case, b, thr, what, R.non_max_suppression(b, *thr)) for case, b, thr, what in S.nms_sweep()]


def test_nms_sweep_reaches_every_cut():
    """100 cases with `NMS_SWEEP_SEED`: the `max_det` cut, pages without a candidate, the `max_nms` cut, other thresholds than
    the detector's, and two calls on 32 pages -- by the oracle's own results."""
    refs = _nms_sweep_refs()
    assert len(refs) == 100
    cand = [(b[..., 4] > np.float32(thr[0])).sum(1) for _, b, thr, _, _ in refs]
    assert sum(thr[2] == 300 and any(len(r) == 300 for r in ref) for _, _, thr, _, ref in refs) >= 10
    assert sum(thr[2] < 300 and any(len(r) == thr[2] for r in ref) for _, _, thr, _, ref in refs) >= 3
    assert sum(bool((c == 0).all()) for c in cand) >= 5
    assert sum(bool((c > 30000).any()) for c in cand) >= 5
    assert sum(len(b) == 32 for _, b, _, _, _ in refs) == 2
    assert all(sum(len(r) for r in ref) > 32 for _, b, _, _, ref in refs if len(b) == 32)
    others = {thr for _, _, thr, _, _ in refs if thr != (S.NMS_CONF, S.NMS_IOU, S.NMS_MAX_DET)}
    assert sum(case % 4 == 3 for case, *_ in refs) == 25 and len(others) >= 12
    assert {b.shape[2] for _, b, _, _, _ in refs} == {6, 7, 8}
    assert min(b.shape[1] for _, b, _, _, _ in refs) <= 300 and max(b.shape[1] for _, b, _, _, _ in refs) >= 64512


def test_ccl_and_resize_sweeps_hold_their_forced_cases():
    shapes = [img.shape for _, img, _ in S.ccl_sweep()]
    assert len(shapes) == 100 and shapes[:12] == S.CCL_FORCED
    for want in [(1, 1)] + [(a, b) for a in (31, 32, 33) for b in (31, 32, 33) if a == b]:
        assert want in shapes[:12]
    assert any(h == 1 and w > 1 for h, w in shapes[:12]) and any(w == 1 and h > 1 for h, w in shapes[:12])
    assert all(img.any() or img.size < 4 for _, img, _ in list(S.ccl_sweep())[12:])
    res = list(S.resize_sweep())
    assert len(res) == 150
    geo = [(img.shape[:2], dst) for _, img, dst, _, _ in res[:len(S.RESIZE_FORCED)]]
    assert any(s == (1, 1) for s, d in geo) and any(d == (1, 1) and s != (1, 1) for s, d in geo) and any(s == d and s != (1, 1) for s, d in geo)
    assert any(1 in d and s != (1, 1) and d != (1, 1) for s, d in geo)
    assert any(d[0] > 16 * s[0] and d[1] > 16 * s[1] and s != (1, 1) for s, d in geo)
    assert any(s[0] > 16 * d[0] and s[1] > 16 * d[1] and d != (1, 1) for s, d in geo)
    assert {img.ndim for _, img, _, _, _ in res} == {2, 3} and {c is None for _, _, _, c, _ in res} == {True, False}


def colour_pick_tie(px):
    """(is the colour pick decided among tied bins, size of the largest such tie) recomputed from the pixels: the counts of the
    255-bin histogram that `get_topk_color` looks at before it stops; a tie = two of them equal, its size = the number of bins of
    the whole histogram with that count (what the argsort has to order)."""
    counts, edges = np.histogram(px, bins=255)
    idx = np.argsort(counts * -1)
    colors, bins = edges[idx], counts[idx]
    top, seen, tol = [colors[0]], [bins[0]], np.sum(bins) * 0.001
    for color, bin_ in zip(colors[1:], bins[1:]):
        seen.append(bin_)
        if np.abs(np.array(top) - color).min() > 10:
            top.append(color)
        if len(top) >= 3 or bin_ < tol:
            break
    vals, n = np.unique(seen, return_counts=True)
    return bool((n >= 2).any()), max([int((counts == v).sum()) for v in vals[n >= 2]], default=0)


def otsu_tie(px):
    """Two thresholds with the same, maximal between-class variance (the arithmetic of `cv_ref.otsu_threshold_value`)."""
    if not len(px):
        return False
    h = np.bincount(px, minlength=256).astype(np.float64)
    scale = 1.0 / float(px.size)
    mu = float(np.dot(np.arange(256, dtype=np.float64), h)) * scale
    mu1 = q1 = 0.0
    eps = float(np.finfo(np.float32).eps)
    sig = []
    for i in range(256):
        p_i = h[i] * scale
        mu1 *= q1
        q1 += p_i
        q2 = 1.0 - q1
        if min(q1, q2) < eps or max(q1, q2) > 1.0 - eps:
            continue
        mu1 = (mu1 + i * p_i) / q1
        mu2 = (mu - q1 * mu1) / q2
        sig.append(q1 * q2 * (mu1 - mu2) * (mu1 - mu2))
    return len(sig) >= 2 and max(sig) > 0 and sig.count(max(sig)) >= 2


def test_tied_pixels_tie_where_the_oracle_decides():
    cases = list(S.tied_sweep())
    assert len(cases) == 200
    colour = [colour_pick_tie(px) for _, px, _ in cases]
    decided_by_tie = sum(c[0] or otsu_tie(px) for c, (_, px, _) in zip(colour, cases))
    assert decided_by_tie >= 100, decided_by_tie
    assert sum(c[1] > 16 for c in colour) >= 20
    assert sum(otsu_tie(px) for _, px, _ in cases) >= 20
    kinds = [what.split("kind ")[1][0] for _, _, what in cases]
    assert set(kinds) == set("0123456")
    for (_, px, what), k in zip(cases, kinds):                        # the kinds are what they say, in the reference's 255 bins
        counts, _ = np.histogram(px, bins=255)
        if k == "4":
            assert len(px) == 0
        if k == "5":
            assert set(px.tolist()) == {0, 255}
        if k == "6":
            assert px.min() == 0 and px.max() == 255 and len(set(counts[counts > 0].tolist())) == 1, what
        if k == "3":
            top = np.sort(counts)[::-1]
            assert (counts == top[1]).sum() > 16, what


# --------------------------------------------------------- the sweeps can fail: the oracle's own result with one perturbation

def _only(bad, what):
    assert len(bad) == 1 and bad[0].startswith(what + ":"), (what, bad)
    return bad[0]


def test_compare_boxes_reports_one_coordinate_off_by_one():
    refs = _db_sweep_refs()[4:12]
    target = next(i for i, r in enumerate(refs) if len(r[3][0]) >= 2)
    cases = []
    for i, (case, what, pr, (boxes, scores)) in enumerate(refs):
        got = (np.array(boxes).copy(), np.array(scores).copy())
        if i == target:
            got[0][1, 2, 0] += 1
        cases.append((what, got, (boxes, scores)))
    assert "boxes" in _only(G.collect_mismatches(cases, G.compare_boxes), refs[target][1])
    cases[target][1][0][1, 2, 0] -= 1
    assert G.collect_mismatches(cases, G.compare_boxes) == []
    cases[target][1][1][0] += 3e-6                                     # a score beyond 1e-6
    assert "scores" in _only(G.collect_mismatches(cases, G.compare_boxes), refs[target][1])
    cases[target] = (cases[target][0], (cases[target][2][0][:-1], cases[target][2][1][:-1]), cases[target][2])   # a box dropped
    _only(G.collect_mismatches(cases, G.compare_boxes), refs[target][1])


def test_compare_detections_reports_one_dropped_detection():
    refs = _nms_sweep_refs()[:12]
    target = next(i for i, r in enumerate(refs) if len(r[4][-1]) >= 3)
    cases = [(what, [a.copy() for a in ref], ref) for _, _, _, what, ref in refs]
    assert G.collect_mismatches(cases, G.compare_detections) == []
    cases[target][1][-1] = np.delete(cases[target][1][-1], 1, axis=0)
    assert "detections" in _only(G.collect_mismatches(cases, G.compare_detections), refs[target][3])
    cases[target][1][-1] = refs[target][4][-1][[1, 0] + list(range(2, len(refs[target][4][-1])))]       # two swapped
    _only(G.collect_mismatches(cases, G.compare_detections), refs[target][3])


def test_compare_labelling_reports_one_swapped_label_pair():
    cases = []
    for case, img, what in list(S.ccl_sweep())[12:20]:
        ref = G.oracle_labelling(img.astype(np.uint8) * 255, 8)
        firsts = np.array([np.flatnonzero(ref[1].ravel() == l)[0] for l in range(1, ref[0])], np.int64)
        cases.append([what, (ref[0] - 1, ref[1].copy(), ref[2][1:].copy(), firsts), ref])
    assert G.collect_mismatches(cases, G.compare_labelling) == []
    target = next(i for i, c in enumerate(cases) if c[1][0] >= 2)
    lab = cases[target][1][1]
    one, two = lab == 1, lab == 2
    lab[one], lab[two] = 2, 1
    assert "labels" in _only(G.collect_mismatches(cases, G.compare_labelling), cases[target][0])
    lab[one], lab[two] = 1, 2
    cases[target][1][2][0, 4] += 1                                     # one area
    assert "stats" in _only(G.collect_mismatches(cases, G.compare_labelling), cases[target][0])
    cases[target][1][2][0, 4] -= 1
    cases[target][1][3][0] = np.flatnonzero(cases[target][2][1].ravel() == 1)[-1]      # a pixel of the component, not its first
    assert "first pixels" in _only(G.collect_mismatches(cases, G.compare_labelling), cases[target][0])


def test_compare_images_reports_one_changed_pixel():
    cases = [(what, G.oracle_resize(img, dst, canvas), G.oracle_resize(img, dst, canvas)) for _, img, dst, canvas, what in list(S.resize_sweep(16))]
    assert G.collect_mismatches(cases, G.compare_images) == []
    cases[11][1][-1, -1] ^= 1
    assert "pixels" in _only(G.collect_mismatches(cases, G.compare_images), cases[11][0])


def _swap_tied_lines(blocks):
    """Swaps two lines of equal `distance` inside one block (any two lines of a block where none tie); returns a copy."""
    blocks = copy.deepcopy(blocks)
    for need_tie in (True, False):
        for b in blocks:
            d = None if b.distance is None else np.asarray(b.distance).reshape(-1)
            d = d if d is not None and len(d) == len(b.lines) else None
            for i in range(len(b.lines) - 1):
                if (not need_tie or (d is not None and d[i] == d[i + 1])) and not np.array_equal(b.lines[i], b.lines[i + 1]):
                    lines = np.array(b.lines).copy()
                    lines[[i, i + 1]] = lines[[i + 1, i]]
                    b.lines = lines if isinstance(b.lines, np.ndarray) else lines.tolist()
                    return blocks, need_tie
    raise AssertionError("no block with two lines")


def test_compare_tail_reports_a_changed_pixel_and_two_swapped_lines():
    from test_gpu_e2e import _equal_up_to_tied_lines, _tail_sweep
    refs = _tail_sweep_refs()[:6]
    cases = [[f"page {i}", (r[0].copy(), r[1].copy(), copy.deepcopy(r[2])), r] for i, r in enumerate(refs)]
    assert G.collect_mismatches(cases, G.compare_tail) == []
    ys, xs = np.nonzero(refs[2][1])
    cases[2][1][1][ys[0], xs[0]] ^= 255
    assert "refined mask" in _only(G.collect_mismatches(cases, G.compare_tail), "page 2")
    cases[2][1][1][ys[0], xs[0]] ^= 255
    cases[4][1][0][0, 0] ^= 1
    assert "mask" in _only(G.collect_mismatches(cases, G.compare_tail), "page 4")
    cases[4][1][0][0, 0] ^= 1
    swapped, _ = _swap_tied_lines(refs[3][2])
    cases[3][1] = (cases[3][1][0], cases[3][1][1], swapped)
    assert "blocks" in _only(G.collect_mismatches(cases, G.compare_tail), "page 3")
    # the sweeps of tests/test_gpu_e2e.py: the same page fails a by-hand range only if more than tied order differs; the
    # default range fails either way
    sweep = [(c[0], False, c[1], c[2]) for c in cases]
    if _equal_up_to_tied_lines(swapped, refs[3][2]):
        _tail_sweep("by hand", sweep, strict=False)
    with pytest.raises(AssertionError, match="page 3"):
        _tail_sweep("default", sweep, strict=True)
    dropped = copy.deepcopy(refs[3][2])[:-1]
    with pytest.raises(AssertionError, match="page 3"):
        _tail_sweep("by hand", [(c[0], False, (c[1][0], c[1][1], dropped) if c[0] == "page 3" else c[1], c[2]) for c in cases], strict=False)


def test_compare_groups_reports_two_tied_lines_swapped():
    from test_group_native import grid_page
    cases = []
    for seed in range(6):
        blks, lines, im_w, im_h, mask = grid_page(seed)
        ref = R.group_output(copy.deepcopy(blks), lines.copy(), im_w, im_h, mask)
        cases.append([f"grid page seed {seed}", copy.deepcopy(ref), ref])
    assert G.collect_mismatches(cases, G.compare_groups) == []
    cases[3][1], tied = _swap_tied_lines(cases[3][2])
    assert tied                                                        # the grids do tie
    assert "blocks" in _only(G.collect_mismatches(cases, G.compare_groups), "grid page seed 3")


def test_compare_refine_decisions_reports_one_changed_decision():
    cases = [[what, G.oracle_refine_decisions(px), G.oracle_refine_decisions(px)] for _, px, what in list(S.tied_sweep(24))]
    assert G.collect_mismatches(cases, G.compare_refine_decisions) == []
    cols, otsu = cases[7][1]
    cases[7][1] = (list(cols[:-1]) + [cols[-1] + 1.0], otsu)
    assert "colours" in _only(G.collect_mismatches(cases, G.compare_refine_decisions), cases[7][0])
    cases[7][1] = cases[7][2]
    cols, otsu = cases[9][2]
    cases[9][1] = (cols, otsu + 1)
    assert "otsu" in _only(G.collect_mismatches(cases, G.compare_refine_decisions), cases[9][0])


def test_collect_mismatches_lets_everything_but_an_assertion_through():
    """A GPU error (`CtdError`, a RuntimeError from torch) ends a sweep where it happens: no later case is produced."""
    produced = []

    def cases():
        for i in range(5):
            produced.append(i)
            if i == 2:
                raise RuntimeError("HIP error")
            yield f"case {i}", np.zeros(2), np.zeros(2)
    with pytest.raises(RuntimeError):
        G.collect_mismatches(cases(), G.compare_images)
    assert produced == [0, 1, 2]
    with pytest.raises(AssertionError, match="case 1: "):
        G.report("x", 2, G.collect_mismatches([("case 0", np.zeros(2), np.zeros(2)), ("case 1", np.ones(2), np.zeros(2))], G.compare_images))
    with pytest.raises(AssertionError, match="2 cases ran, 3 expected"):
        G.sweep("x", 3, [("case 0", np.zeros(2), np.zeros(2)), ("case 1", np.zeros(2), np.zeros(2))], G.compare_images)
    G.sweep("x", 2, [("case 0", np.zeros(2), np.zeros(2)), ("case 1", np.zeros(2), np.zeros(2))], G.compare_images)
