"""-m gpu: the DB stage with the segment skip of `dbc_accum_kernel` (csrc/kernels_tail.hip; the flags come from the label
pass of `launch_ccl_dual`, csrc/kernels_post.hip) on the maps of tests/db_runs_cases.py, through `ctd_tail_db_boxes` with the
trace on: every integer table exact against tests/dbc_emul.py, the f64 sums within the bounds `tail_trace_cases.db_reference`
derives (a skipped wave added nothing before, so the addends and their grouping into runs are what they were), boxes and
scores against the oracle's contour walk.  Pages whose background -1 is a hole -- where the skip must be off -- share a call
with pages where it is on, and pages with holes share it with pages that have none (`hole_rows` = 0: no ring test, no `par_b`
gather).  That the maps are what this needs is checked without a GPU in tests/test_db_runs_cases.py."""
import numpy as np
import pytest
import torch

import db_runs_cases as D
import tail_trace_cases as T
from conftest import pkg
from oracle import postproc_ref as R
from test_gpu_sweeps import collect_mismatches, compare_boxes, report

pytestmark = pytest.mark.gpu

_REF = {}


def reference(name, prob):
    """(tables with bounds, oracle boxes and scores) of a map, computed once and shared (only read)."""
    if name not in _REF:
        H, W = prob.shape
        _REF[name] = (T.db_reference(prob), R.boxes_from_bitmap(prob, prob > 0.3, W, H, max_candidates=1000))
    return _REF[name]


def traced_call(maps, tune=()):
    """One `Tail.db_boxes` call on `maps` = [(name, prob)] with the trace on: ([trace page], [boxes], [scores])."""
    p = pkg()
    tail = p.tail.thread_tail(torch.device("cuda", torch.cuda.current_device()))
    prob = torch.from_numpy(np.stack([pr for _, pr in maps])).cuda()
    tail.set_trace(True)
    try:
        with p._lib.tuning(dict(tune)):
            boxes, scores = tail.db_boxes(prob, (prob > 0.3).to(torch.uint8))
            pages = tail.trace_db()
    finally:
        tail.set_trace(False)
    assert len(pages) == len(boxes) == len(scores) == len(maps), f"{len(pages)} pages traced, {len(boxes)} returned, {len(maps)} sent"
    return pages, boxes, scores


def check_call(call_name, tune, maps):
    pages, boxes, scores = traced_call(maps, tune)
    bad = []
    for (name, prob), page, bx, sc in zip(maps, pages, boxes, scores):
        tables, oracle = reference(name, prob)
        bad += collect_mismatches([(f"{name} ({call_name}): tables", page, tables)], T.compare_db_tables)
        bad += collect_mismatches([(f"{name} ({call_name}): boxes and scores", (bx, sc), oracle)], compare_boxes)
    return 2 * len(maps), bad


@pytest.mark.parametrize("index", range(len(D.calls())))
def test_db_tables_and_boxes_with_the_segment_skip(index):
    """One call of `db_runs_cases.calls`: pages that skip (outer background -1), pages that must not (a frame, nested rings, a
    slotted bar along the top edge: -1 is a hole) and pages with nothing to skip (all foreground) side by side."""
    call_name, tune, maps = D.calls()[index]
    n, bad = check_call(call_name, tune, maps)
    report(f"db stage, {call_name}", n, bad)


def test_a_page_gives_the_same_tables_alone_and_between_pages_of_the_other_kind():
    """The text page and the frame page alone and in the mixed call: every table the same bytes (the f64 sums are sums of the
    same runs, added by atomics in any order: within twice their bound of each other, each being within it of the emulation)."""
    _, _, maps = D.calls()[0]
    together = dict(zip((n for n, _ in maps), traced_call(maps)[0]))
    for name in ("text", "frame"):
        (alone,), _, _ = traced_call([m for m in maps if m[0] == name])
        for k in ("hdr",) + T._INT_TABLES + ("row_lo", "row_hi"):
            np.testing.assert_array_equal(alone[k], together[name][k], err_msg=f"{name}: {k}")
        ref = reference(name, dict(maps)[name])[0]
        for k in ("sum_f", "sum_b", "ring_sum"):
            assert (np.abs(alone[k] - together[name][k]) <= 2 * ref["bound_" + k]).all(), f"{name}: {k}"


def test_one_1024_page():
    """A 1024 x 1024 text-like page: 4 096 blocks' worth of segments, most of them skipped."""
    n, bad = check_call("1024 x 1024", {}, [("big", D.big_map())])
    report("db stage, 1024 x 1024", n, bad)
