"""-m gpu: the native tail's fixed tables at, below and above their capacity (csrc/tail.hip: `kCompCap` = 65 536 components per
polarity and page, `kRowCap` = 262 144 row entries per page, the one-component-per-2 x 2-cell bound of `refine_canvas`).  The
cases are tests/tail_cap_cases.py, checked without a GPU in tests/test_tail_cap_cases.py; every comparison is exact except the
DB scores (atol 1e-6, as everywhere in the suite).

  * DB stage, *_at maps (n_f = 65 536 | n_b = 65 536 | rows = 262 144, every guard of `dbc_prep / scan / accum_kernel` with
    equality): header [n_f, n_b, rows, 0], every table against `dbc_emul` (`tail_trace_cases.compare_db_tables`), boxes and
    scores against `R.boxes_from_bitmap`.
  * DB stage, *_over maps (one entry more): overflow flag 1, and the boxes and scores of `db_collect`'s label-image path
    against the oracle -- the first check of that path's RESULT (the row table overflows here for the first time, and so does
    the background count next to three foreground components).
  * DB stage, batches [fits, f_over, r_at] and [b_over, fits]: an overflowed page between pages that fit -- the batch-wide
    maxima of `db_collect`, the per-page skip of its `parallel_for` and the serial loop behind it --, every page against its
    single-page call and the oracle, the pages that fit through their tables too.
  * undetected pass (`refine_undetected_mask`): u_at / u_over / u_far / u_grow -- the blob that becomes a window is component
    65 536, 65 537, 70 401 .. 70 403, 90 113 of the page mask's labelling --, both refine modes, window records, refined masks and masks after
    against the oracle; u_over between two text-like pages of one size (one labelling launch for the batch) and of three sizes
    (one per page), each page against its single-page call; `Tail.run` on u_over with no detections against `R.detector_tail`.
  * canvas bound: a call of nothing but windows whose every candidate holds exactly ((w + 1) / 2) * ((h + 1) / 2) components
    (1, 4, 272, 2 145; two bands each: the labelling of the canvas returns 4 844 = cap1 - 1 labels, asserted on the CPU)
    through the canvases (`tail_lds` = 0) and at the defaults; both equal the oracle and each other.  The masks are all zero
    either way (the test's docstring says what that can and cannot see); a text-like window runs the same two paths in a
    call of its own.
  * history, on a tail of its own: u_at, u_grow (90 113 components: the relabelling's table outgrows the buffer and is
    allocated again), the largest batch, u_at again -- the same bytes both times.

FOUND: `undetected_pass` labelled with `max_labels` = 65 536 and walked min(n, 65 536) statistics rows, so a left-over component
ranked beyond that never became a window: on u_over and u_far the refined mask came back all zero where the oracle refines
4 650 (u_over, mode 0) and 15 748 (u_far, mode 0) pixels.  It now labels a page over the capacity again with a table of all its
rows; pages within it take the path they took.  The label-image path, the *_at maps and the canvas bound agreed with the oracle
as they were.

MEASURED on the MI355X (wall time per test, the oracle side included; the whole file 16 s, 25 tests): DB at the capacity f_at
1.1 s, b_at 1.5 s, r_at 1.1 s; over it f_over 0.2 s, b_over 0.4 s, r_over 0.6 s; the two batches 0.13 s each (their single-page
calls are shared with the tests before); undetected pass 0.5 - 0.8 s per case and mode; its batches 1.4 s (303 windows) and
0.9 s (139); `Tail.run` 0.2 s; canvas bound 0.02 - 0.1 s, the text window under 0.01 s; history 0.3 s.  The `Tail.db_boxes` call
itself: 2.8 / 3.4 / 3.9 ms on f_at / b_at / r_at, 2.9 / 3.0 / 5.4 ms on f_over / b_over / r_over -- the host fallback (label
image to the host, statistics again, `ctd_db_boxes` on 65 537 components, of which `max_candidates` = 1 000 are walked) costs
no more than a millisecond or two; 10 ms for each of the batches.  Headers seen: f_over [65 536, 2, 65 551, 1], b_over [3,
65 536, 197 111, 1], r_over [516, 2, 262 145, 1].  On the library before the fix the u_over, u_far, batch and `Tail.run` tests
fail and the u_at ones pass (u_grow came later and was run on the fixed library only).
"""
import time

import numpy as np
import pytest
import torch

import tail_cap_cases as K
import tail_trace_cases as T
from conftest import pkg
from oracle import postproc_ref as R
from test_gpu_sweeps import collect_mismatches, compare_boxes, compare_tail, report, sweep
from test_gpu_tail_trace import check_call, in_mode, traced_refine

pytestmark = pytest.mark.gpu


def the_tail():
    return pkg().tail.thread_tail(torch.device("cuda", torch.cuda.current_device()))


# ------------------------------------------------------------------------------------------------------------ DB stage

def db_call(names):
    """One `Tail.db_boxes` call on the maps `names` with the trace on: [(trace page, (boxes, scores))] per map, and the
    seconds the call took (the host fallback of an overflowed page is inside it)."""
    tail = the_tail()
    prob = torch.from_numpy(np.stack([K.db_maps()[n] for n in names])).cuda()
    bitmap = (prob > 0.3).to(torch.uint8)
    torch.cuda.synchronize()
    tail.set_trace(True)
    try:
        t0 = time.perf_counter()
        boxes, scores = tail.db_boxes(prob, bitmap)
        dt = time.perf_counter() - t0
        pages = tail.trace_db()
    finally:
        tail.set_trace(False)
    assert len(pages) == len(boxes) == len(scores) == len(names), f"{names}: {len(pages)} pages traced, {len(boxes)} returned"
    print(f"  db_boxes{list(names)}: {dt * 1e3:.1f} ms; hdr {[[int(v) for v in p['hdr']] for p in pages]}")
    return [(p, (b, s)) for p, b, s in zip(pages, boxes, scores)]


_SINGLE = {}


def single(name):
    """A map's single-page call, made once (its results are only read)."""
    if name not in _SINGLE:
        _SINGLE[name] = db_call([name])[0]
    return _SINGLE[name]


def compare_hdr(got, name):
    if name in K.DB_COUNTS:
        nf, nb, rows = K.DB_COUNTS[name]
    else:                                                      # a map that fits: the emulation's counts
        t = K.db_tables(name)
        nf, nb, rows = int(t["n_f"]), int(t["n_b"]), int(t["rows"])
    hdr = [int(v) for v in got["hdr"]]
    if name in K.DB_COUNTS and K.overflows(name):
        assert hdr[3] == 1, f"hdr {hdr}: overflow flag {hdr[3]} vs 1"
        assert hdr[:2] == [min(nf, K.COMP_CAP), min(nb, K.COMP_CAP)], f"hdr {hdr}: counts beyond the capacity"
    else:
        assert hdr == [nf, nb, rows, 0], f"hdr {hdr} vs {[nf, nb, rows, 0]}"


def page_checks(what, name, page, result):
    """The comparisons one page of a DB call takes: (description, got, ref, compare) each."""
    out = [(f"{what}: boxes and scores against the oracle", result, K.db_oracle(name), compare_boxes),
           (f"{what}: header", page, name, compare_hdr)]
    if not (name in K.DB_COUNTS and K.overflows(name)):
        out.append((f"{what}: tables", page, K.db_tables(name), T.compare_db_tables))
    return out


def run_checks(name, checks, n):
    sweep(name, n, ((what, (got, compare), ref) for what, got, ref, compare in checks), lambda gc, ref: gc[1](gc[0], ref))


@pytest.mark.parametrize("name", K.AT)
def test_db_stage_at_the_capacity(name):
    """f_at / b_at / r_at alone: header [n_f, n_b, rows, 0] with the count under test EQUAL to its capacity, all tables, boxes
    and scores."""
    print()
    page, result = single(name)
    assert (K.db_oracle(name)[1] > 0.6).sum() == 2
    run_checks(f"db stage at the capacity, {name}", page_checks(name, name, page, result), 3)


@pytest.mark.parametrize("name", K.OVER)
def test_db_stage_over_the_capacity_takes_the_label_image_path(name):
    """f_over / b_over / r_over alone: the overflow flag, and the boxes and scores of the host fallback against the oracle."""
    print()
    page, result = single(name)
    assert (K.db_oracle(name)[1] > 0.6).sum() == 2
    run_checks(f"db stage over the capacity, {name}", page_checks(name, name, page, result), 2)


@pytest.mark.parametrize("index", range(len(K.DB_BATCHES)))
def test_db_stage_overflowed_page_next_to_pages_that_fit(index):
    """[fits, f_over, r_at] and [b_over, fits] in one call each: every page against the oracle, its header and (where it
    fits) its tables, and against its own single-page call."""
    print()
    names = K.DB_BATCHES[index]
    got = db_call(names)
    checks = []
    for b, (name, (page, result)) in enumerate(zip(names, got)):
        what = f"page {b} ({name}) of {list(names)}"
        checks += page_checks(what, name, page, result)
        checks.append((f"{what}: boxes and scores against its single-page call", result, single(name)[1], compare_boxes))
        checks.append((f"{what}: header against its single-page call", [int(v) for v in page["hdr"]],
                       [int(v) for v in single(name)[0]["hdr"]], lambda g, r: np.testing.assert_array_equal(g, r)))
    # per page: oracle, header and (where it fits) tables, then two comparisons with its single-page call
    run_checks(f"db batch {list(names)}", checks, ((3 + 2 + 3) + 2 * 3, (2 + 3) + 2 * 2)[index])


# ------------------------------------------------------------------------------------------------------- undetected pass

def both_sides(case, refined):
    """Every blob of a one-page case that becomes a window has refined pixels, and pixels that are not."""
    _, blobs = K.blob_ranks(case)
    for rank, (x1, y1, x2, y2), covered in blobs:
        inside = refined[0][y1:y2, x1:x2]
        if covered < 0.5:
            assert 500 < (inside > 0).sum() < inside.size - 500, f"{case['name']}: component {rank} refined to {(inside > 0).sum()} pixels"
        else:
            assert not inside.any(), f"{case['name']}: component {rank} is covered by a block and was refined"


@pytest.mark.parametrize("mode", (0, 1))
@pytest.mark.parametrize("name", ("u_at", "u_over", "u_far", "u_grow"))
def test_undetected_pass_beyond_the_capacity(name, mode):
    """u_at / u_over / u_far / u_grow, both refine modes: the second pass's window records, the refined mask and the mask after the
    call against the oracle; the blobs' windows are refined on both sides."""
    case = in_mode(K.undetected_cases()[name], mode)
    got = traced_refine(case)
    n, bad = check_call(case, got)
    assert n == {"u_at": 1, "u_over": 1, "u_far": 4, "u_grow": 1}[name], f"{n} windows"      # u_far: two blocks, two of the three blobs
    bad += collect_mismatches([(f"{case['name']}: refined on both sides", case, got[2])], both_sides)
    report(f"undetected pass, {case['name']}", n, bad)


@pytest.mark.parametrize("index", (0, 1))
def test_undetected_pass_overflowed_page_between_pages_that_fit(index):
    """[text, u_over, text]: of one size (one labelling launch for the batch) and of three sizes (one per page): the call
    against the oracle, and every page against its single-page call."""
    case = K.undetected_batches()[index]
    got = traced_refine(case)
    n, bad = check_call(case, got)
    assert n == (303, 139)[index], f"{n} windows"             # four of the blocks, the rest left-over components (u_over's: one)
    pairs = []
    for b in range(3):
        alone = traced_refine(K.single_page(case, b))
        pairs.append((f"{case['name']}: refined mask of page {b} against its single-page call", got[2][b], alone[2][0]))
        pairs.append((f"{case['name']}: mask after, page {b}, against its single-page call", got[3][b], alone[3][0]))
    bad += collect_mismatches(pairs, lambda g, r: np.testing.assert_array_equal(g, r))
    u = K.undetected_cases()["u_over"]
    bad += collect_mismatches([(f"{case['name']}: u_over refined on both sides", u, [got[2][1]])], both_sides)
    report(f"undetected pass, {case['name']}", n, bad)


@pytest.mark.parametrize("mode", (0, 1))
def test_whole_tail_on_u_over_without_detections(mode):
    """`Tail.run(..., keep_undetected_mask=True)` on u_over with an empty Detect tensor and an empty line map against
    `R.detector_tail`: the page mask goes through the crop / resize stage (same size: a copy) into the undetected pass."""
    case = K.undetected_cases()["u_over"]
    page, mask = case["pages"][0], case["masks"][0]
    H, W = mask.shape
    blks = np.zeros((1, 64, 7), np.float32)
    prob = np.zeros((1, H, W), np.float32)
    dev = torch.device("cuda", torch.cuda.current_device())
    pt = torch.from_numpy(prob).to(dev)
    got = the_tail().run([torch.from_numpy(page).to(dev)], [(H, W, 0, 0)], torch.from_numpy(blks).to(dev),
                         torch.from_numpy(mask[None].copy()).to(dev), pt, (pt > 0.3).to(torch.uint8), refine_mode=mode,
                         keep_undetected_mask=True)
    mask_f = (mask.astype(np.float32) + 0.5) / 255
    ref = R.detector_tail(page, blks, mask_f[None, None], np.stack([prob[0], prob[0]])[None], input_size=(W, H), refine_mode=mode,
                          keep_undetected_mask=True)
    assert (ref[1] > 0).sum() > 500 and not len(ref[2])
    sweep(f"whole tail on u_over, refine mode {mode}", 1, [("u_over", [np.array(got[0][0]), np.array(got[0][1]), got[0][2]], ref)], compare_tail)


# ---------------------------------------------------------------------------------------------------------- canvas bound

CANVAS_RUNS = [(" [tail_lds = 0]", {"tail_lds": 0}), (" [defaults]", {})]


def on_the_two_merge_paths(case, n_windows):
    """A case under `CANVAS_RUNS`: every run against the oracle (records, path counts, masks) and the runs against each other."""
    total, bad, before, masks = 0, [], [], []
    for what, tune in CANVAS_RUNS:
        got = traced_refine(case, tune)
        n, b = check_call(case, got, what)
        assert n == n_windows, f"{n} windows"
        if tune:
            assert dict(got[1]) == {"lds": 0, "canvas": n, "overflow": 0}, got[1]
        print(f"  {case['name']}{what}: paths {dict(got[1])}")
        total, bad = total + n, bad + b
        before.append(T.before_merge(got[0]))
        masks.append([m.tobytes() for m in got[2] + got[3]])
    assert before[0] == before[1], "the records before the merge stage differ between the merge paths"
    assert masks[0] == masks[1], "the masks differ between the merge paths"
    return total, bad


@pytest.mark.parametrize("mode", (0, 1))
def test_canvas_tables_at_their_bound(mode):
    """The dot-grid pages, and nothing else in the call: every candidate of the 1 x 1, 3 x 3, 33 x 31 and 65 x 129 windows
    holds exactly one component per 2 x 2 cell, so the canvas labelling returns `cap1` - 1 = 4 844 labels and the last row of
    `cstats` and of the counter table is used (summed on the CPU in tests/test_tail_cap_cases.py; the device does not report
    the count).  Every window through the canvases (`tail_lds` = 0), and at the defaults.

    What this can see: a fault, or a non-zero mask, if a table a few rows short lets the labelling's statistics or the
    counters run into what lies behind them.  What it cannot: the dots are single pixels, all refused by the `w * h >= 3`
    rule, and `ccl_label_body` writes no statistics for an id above `max_labels`; so a bound that is short, with a
    `max_labels` that is short with it, still gives the all-zero masks of the oracle."""
    total, bad = on_the_two_merge_paths(in_mode(K.canvas_case(), mode), 4)
    report(f"canvas bound, refine mode {mode}", total, bad)


@pytest.mark.parametrize("mode", (0, 1))
def test_canvas_path_on_the_text_window_alone(mode):
    """The text-like window of the second dot page in a call of its own on the same two paths: a result that is not all
    zero (2 672 pixels in mode 0) from the canvases."""
    total, bad = on_the_two_merge_paths(in_mode(K.canvas_text_case(), mode), 1)
    report(f"canvas path, text window, refine mode {mode}", total, bad)


# --------------------------------------------------------------------------------------------------------------- history

def test_u_at_before_and_after_the_largest_batch():
    """On a tail of its own, so that its buffers start empty: the u_at call (the statistics table of a one-page call is
    allocated: 1.64 MB), u_grow (90 113 components: the relabelling asks for 1.80 MB, the buffer is released and allocated
    again -- the one allocation the relabelling can make), the batch of three 512 x 512 pages with u_over in the middle, the
    u_at call again.  u_at returns the same bytes both times and the oracle's; u_grow equals the oracle."""
    p = pkg()
    u = K.undetected_cases()
    tail = p.tail.Tail(torch.device("cuda", torch.cuda.current_device()))
    try:
        first = traced_refine(u["u_at"], tail=tail)
        grown = traced_refine(u["u_grow"], tail=tail)
        traced_refine(K.undetected_batches()[0], tail=tail)
        second = traced_refine(u["u_at"], tail=tail)
    finally:
        tail.__del__()
    for a, b in zip(first[2] + first[3], second[2] + second[3]):
        assert a.tobytes() == b.tobytes(), "u_at differs after the batch"
    assert first[0].tobytes() == second[0].tobytes(), "u_at's window records differ after the batch"
    n, bad = check_call(u["u_at"], second)
    k, b = check_call(u["u_grow"], grown)
    bad += b + collect_mismatches([("u_grow: refined on both sides", u["u_grow"], grown[2])], both_sides)
    report("u_at after a grown table and the largest batch", n + k, bad)
