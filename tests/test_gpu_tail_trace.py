"""-m gpu: the tables the tail's kernels WRITE, not only the decisions the host draws from them (`Tail.set_trace`, ABI v9).

Mask refinement: per window the four histograms of `tw_hist_kernel`, the rules, the six xor sums of `tw_xor_kernel` and the
candidates with their distances -- exact against the oracle on the window's crop (`tail_trace_cases.refine_reference`), every
window of every call; the path counts against `ctd_tail_refine_paths`; the final masks still against `R.refine_mask` /
`R.refine_undetected_mask`.  DB stage: every table of `dbc_prep / scan / init / accum_kernel` through `ctd_tail_db_boxes` --
integers exact against `dbc_emul.dbc_tables`, the f64 sums within the bound derived in `tail_trace_cases.db_reference`.

Cases and their coverage are checked without a GPU in tests/test_tail_trace_cases.py.  Mismatches are collected per window /
per map as in tests/test_gpu_sweeps.py (AssertionError only: any other exception ends the test, nothing is launched after it)."""
import numpy as np
import pytest
import torch

import tail_trace_cases as T
from conftest import pkg
from test_gpu_sweeps import collect_mismatches, report

pytestmark = pytest.mark.gpu

_REF = {}


def reference(case):
    """A case's reference, computed once and shared (never modified: the records are compared, the masks only read)."""
    if case["name"] not in _REF:
        _REF[case["name"]] = T.refine_reference(case)
    return _REF[case["name"]]


def traced_refine(case, tune=()):
    """One `Tail.refine` call with the trace on (the calling thread's tail; off again afterwards), under the case's tuning
    keys and `tune` = {key: value}, put back afterwards.  Returns (records, path counts, refined masks, masks after)."""
    p = pkg()
    tail = p.tail.thread_tail(torch.device("cuda", torch.cuda.current_device()))
    pages = [torch.from_numpy(img).cuda() for img in case["pages"]]
    tail.set_trace(True)
    try:
        with p._lib.tuning({**case["tune"], **dict(tune)}):
            refined, after = tail.refine(pages, [m.copy() for m in case["masks"]], case["boxes"], case["mode"], case["keep"])
            recs, paths = tail.trace_windows(), tail.refine_paths()
    finally:
        tail.set_trace(False)
    return recs, paths, [np.array(r) for r in refined], [np.array(a) for a in after]


def check_call(case, got, what=""):
    """Every window record, the path counts and the final masks of one call against the reference; returns the mismatches."""
    recs, paths, refined, after = got
    ref_recs, ref_refined, ref_after = reference(case)
    assert len(recs) == len(ref_recs), f"{case['name']}{what}: {len(recs)} windows traced, {len(ref_recs)} expected"

    def cases():
        for i, (g, r) in enumerate(zip(recs, ref_recs)):
            yield f"{case['name']}{what}, window {i} (page {r['page']}, pass {r['pass_']}, {r['w']} x {r['h']} at {r['x1']},{r['y1']})", g, r
    bad = collect_mismatches(cases(), T.compare_window)
    bad += collect_mismatches([(f"{case['name']}{what}: paths", recs, paths)], T.compare_paths)
    masks = [(f"{case['name']}{what}: refined mask of page {b}", refined[b], ref_refined[b]) for b in range(len(refined))]
    masks += [(f"{case['name']}{what}: mask after the call, page {b}", after[b], ref_after[b]) for b in range(len(after))]
    bad += collect_mismatches(masks, lambda g, r: np.testing.assert_array_equal(g, r))
    return len(recs), bad


def test_refine_tables_of_every_width_class_on_the_three_merge_paths():
    """The width-class pages (every width 1 .. 17, 31 .. 33, 63 .. 65 at heights 1, 2, 3 and >= 8, four image kinds) three
    times: default path, every window through the canvases (`tail_lds` = 0), and with a run table of 8 (`tail_lds_rcap`:
    overflows re-done through the canvases).  The records before the merge stage must be the same bytes in all three."""
    case = T.width_class_case()
    runs = [("", {}), (" [tail_lds = 0]", {"tail_lds": 0}), (" [tail_lds_rcap = 8]", {"tail_lds_rcap": 8})]
    n, bad, before = 0, [], []
    for what, tune in runs:
        got = traced_refine(case, tune)
        k, b = check_call(case, got, what)
        n, bad = n + k, bad + b
        before.append(T.before_merge(got[0]))
        if what == " [tail_lds = 0]":
            assert got[1]["lds"] == 0 and got[1]["canvas"] == k, got[1]
    assert before[0] == before[1] == before[2], "the records before the merge stage differ between the merge paths"
    report("refine tables, width classes", n, bad)


@pytest.mark.parametrize("index", range(6))
def test_refine_tables(index):
    """The other calls of `tail_trace_cases.refine_cases`: windows of two and of four blocks with grid-stride trips, those
    next to 1 x 1 and 3 x 2 windows, overlapping and repeated ones, the same under a lowered `tail_max_blocks`, three pages of
    different widths, and a `keep_undetected_mask` call whose second-pass windows are compared as well."""
    case = T.refine_cases()[index]
    n, bad = check_call(case, traced_refine(case))
    report(f"refine tables, {case['name']}", n, bad)


def test_db_tables():
    """Every table `db_collect` hands to `ctd_db_boxes_compact`, per page of every call of `tail_trace_cases.db_calls`; on
    the map whose EMULATED component count exceeds the capacity only the overflow flag."""
    p = pkg()
    tail = p.tail.thread_tail(torch.device("cuda", torch.cuda.current_device()))
    n_maps = sum(len(call) for _, call in T.db_calls())

    def cases():
        for call_name, call in T.db_calls():
            prob = torch.from_numpy(np.stack([pr for _, pr in call])).cuda()
            tail.db_boxes(prob, (prob > 0.3).to(torch.uint8))
            pages = tail.trace_db()
            assert len(pages) == len(call), f"{call_name}: {len(pages)} pages traced, {len(call)} expected"
            for (name, pr), got in zip(call, pages):
                if name == "overflow":
                    nf, nb = T.db_counts(pr)
                    ref = dict(n_f=nf, n_b=nb, rows=0)
                    assert nf > T.COMP_CAP
                else:
                    ref = T.db_reference(pr)
                yield f"{name} ({call_name})", got, ref
    tail.set_trace(True)
    try:
        bad = collect_mismatches(cases(), T.compare_db_tables)
    finally:
        tail.set_trace(False)
    report("db tables", n_maps, bad)


def test_trace_is_off_by_default_and_per_tail():
    """A tail that was never switched on records nothing; switching off drops what was recorded."""
    p = pkg()
    tail = p.tail.thread_tail(torch.device("cuda", torch.cuda.current_device()))
    case = T.refine_cases()[0]
    pages = [torch.from_numpy(img).cuda() for img in case["pages"]]
    tail.refine(pages, [m.copy() for m in case["masks"]], case["boxes"], 0, False)
    assert len(tail.trace_windows()) == 0 and tail.trace_db() == []
    tail.set_trace(True)
    tail.refine(pages, [m.copy() for m in case["masks"]], case["boxes"], 0, False)
    tail.refine(pages, [m.copy() for m in case["masks"]], case["boxes"], 0, False)      # cleared at the start of every call
    assert len(tail.trace_windows()) == 1
    tail.set_trace(False)
    assert len(tail.trace_windows()) == 0
