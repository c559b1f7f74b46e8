"""-m gpu: the tables the tail's kernels WRITE, not only the decisions the host draws from them (`Tail.set_trace`, ABI v9).

Mask refinement: per window the four histograms of `tw_hist_kernel`, the rules, the six xor sums of `tw_xor_kernel` and the
candidates with their distances -- exact against the oracle on the window's crop (`tail_trace_cases.refine_reference`), every
window of every call; the path counts against `ctd_tail_refine_paths`; the final masks still against `R.refine_mask` /
`R.refine_undetected_mask`.  DB stage: every table of `dbc_prep / scan / init / accum_kernel` through `ctd_tail_db_boxes` --
integers exact against `dbc_emul.dbc_tables`, the f64 sums within the bound derived in `tail_trace_cases.db_reference`.

The merge stage's launch-shape keys (`tail_lds_threads`, `tail_lds_cls0 / cls1`, `tail_lds_runs_x10`): the same exact
comparison under every value, plus the LAUNCH LOG of the trace (`Tail.trace_lds_launches`: windows, max_words, rcap, threads
and LDS bytes of every `tw_lds_kernel` launch, as the launcher clamped them) against `tail_trace_cases.lds_launches`, a plain
restatement of the host's sizing checked on the CPU against hand-computed rows, and the path counts against it (and, where run
tables overflow, against the emulation's run counts).  Measured (windows, max_words, rcap, bytes per launch): block_size_case
18 windows in two launches (17, 1 026, 2 565, 34 964) + (1, 2 080, 5 200, 70 800) at 256 / 512 / 1024 threads, {lds 18, canvas 0,
overflow 0}; the width-class pages one launch (392, 33, 1 024, 8 736); class_case 11 windows in 1 to 3 launches per setting of
`class_settings` (defaults (8, 1 197, 2 992, 40 776) + (2, 2 080, 5 200, 70 800) + (1, 4 515, 11 287, 153 588); one class
(11, 4 515, ..); limits one byte below two needs (7, 600) + (2, 1 302) + (2, 4 515)), all in LDS; `tail_lds_runs_x10` = 1 / 25 /
160 / 1000 on class_case: {lds 9 | 8, overflow 2 | 3} (refine mode 0 | 1), {lds 11}, {lds 7, canvas 4}, {lds 4, canvas 7};
the 2 080-word window (1, 2 080, 1 024, 37 520) at 1; the speckle window overflows at rcap 1 024, not at 1 560 / 9 984.

Cases and their coverage are checked without a GPU in tests/test_tail_trace_cases.py.  Mismatches are collected per window /
per map as in tests/test_gpu_sweeps.py (AssertionError only: any other exception ends the test, nothing is launched after it)."""
import functools

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


def traced_launches(case, tune=(), tail=None):
    """One `Tail.refine` call with the trace on (the calling thread's tail unless one is given; off again afterwards), under
    the case's tuning keys and `tune` = {key: value}, put back afterwards.  Returns ((records, path counts, refined masks,
    masks after), the launch log of the window-local merge kernel)."""
    p = pkg()
    if tail is None:
        tail = p.tail.thread_tail(torch.device("cuda", torch.cuda.current_device()))
    pages = [torch.from_numpy(img).cuda() for img in case["pages"]]
    tail.set_trace(True)
    try:
        with p._lib.tuning({**case["tune"], **dict(tune)}):
            refined, after = tail.refine(pages, [m.copy() for m in case["masks"]], case["boxes"], case["mode"], case["keep"])
            recs, paths, launches = tail.trace_windows(), tail.refine_paths(), tail.trace_lds_launches()
    finally:
        tail.set_trace(False)
    return (recs, paths, [np.array(r) for r in refined], [np.array(a) for a in after]), launches


def traced_refine(case, tune=(), tail=None):
    """`traced_launches` without the launch log: (records, path counts, refined masks, masks after)."""
    return traced_launches(case, tune, tail)[0]


def in_mode(case, mode):
    """The case in the other refine mode (a case of its own: the reference is kept per name)."""
    return case if mode == case["mode"] else {**case, "mode": mode, "name": f"{case['name']} [refine mode {mode}]"}


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
    assert len(tail.trace_windows()) == 0 and tail.trace_db() == [] and tail.trace_lds_launches() == []
    tail.set_trace(True)
    tail.refine(pages, [m.copy() for m in case["masks"]], case["boxes"], 0, False)
    tail.refine(pages, [m.copy() for m in case["masks"]], case["boxes"], 0, False)      # cleared at the start of every call
    assert len(tail.trace_windows()) == 1
    words = T.case_words(case)
    ((_, mw, rcap, nbytes, _),) = T.launches_of_setting(words)[1]
    assert tail.trace_lds_launches() == [dict(windows=1, max_words=mw, rcap=rcap, threads=T.key_defaults()["tail_lds_threads"],
                                              bytes=nbytes, refused=0)]
    other = p.tail.Tail(tail.device)                     # per tail: a second object, never switched on, records nothing
    try:
        other.refine(pages, [m.copy() for m in case["masks"]], case["boxes"], 0, False)
        assert len(other.trace_windows()) == 0 and other.trace_lds_launches() == []
        assert len(tail.trace_lds_launches()) == 1
    finally:
        other.__del__()
    tail.set_trace(False)
    assert len(tail.trace_windows()) == 0 and tail.trace_lds_launches() == []


# ----------------------------------------------------------------------------------------- the merge stage's launch-shape keys

def _show(what, launches, paths):
    print(f"  {what}: paths {dict(paths)}; launches (windows, max_words, rcap, threads, bytes) "
          f"{[(g['windows'], g['max_words'], g['rcap'], g['threads'], g['bytes']) + (('REFUSED',) if g['refused'] else ()) for g in launches]}")


def _run_keyed(case, tune, what, want_paths=None):
    """One traced call under `tune`: results against the oracle, the launch log against the restatement of the host's sizing
    (`tail_trace_cases.lds_launches`, at the thread count `tune` asks for), the routing against it too; returns
    (windows, mismatches, records before the merge stage, launch log)."""
    got, launches = traced_launches(case, tune)
    _show(f"{case['name']}{what}", launches, got[1])
    n, bad = check_call(case, got, what)
    canvas, want = T.launches_of_setting(T.case_words(case), {**case["tune"], **dict(tune)})
    nt = T.clamped_threads({**T.key_defaults(), **case["tune"], **dict(tune)}["tail_lds_threads"])
    bad += collect_mismatches([(f"{case['name']}{what}: launch log", launches, (want, nt))], T.compare_launches)
    paths = got[1]
    if want_paths is None:                               # by the restatement alone: what is not LDS up front is canvas; overflows on top
        ok = paths["canvas"] - paths["overflow"] == len(canvas) and paths["lds"] + paths["canvas"] == n
    else:
        ok = dict(paths) == want_paths
    if not ok:
        bad.append(f"{case['name']}{what}: paths {dict(paths)}, expected {want_paths or ('canvas up front', len(canvas))}")
    return n, bad, T.before_merge(got[0]), launches


def test_block_size_case_at_every_block_size():
    """`tail_lds_threads` = 256 / 512 / 1024 on windows whose word counts lie on both sides of each block size (one and
    three words per row, a 257-word row, a 1 x 1 and a 33 x 2 window, 2 080 words), both refine modes: every record and mask
    byte against the oracle, every launch at the block size asked for, no overflow and nothing through the canvases, and the
    records before the merge stage the same bytes at the three sizes."""
    print()
    total, bad = 0, []
    for mode in (0, 1):
        case, before = in_mode(T.block_size_case(), mode), []
        for nt in T.BLOCK_SIZES:
            n, b, bm, _ = _run_keyed(case, {"tail_lds_threads": nt}, f" [tail_lds_threads = {nt}]", {"lds": 18, "canvas": 0, "overflow": 0})
            total, bad = total + n, bad + b
            before.append(bm)
        assert before[0] == before[1] == before[2], "the records before the merge stage differ between the block sizes"
    report("block_size_case x block sizes x refine modes", total, bad)


def test_width_classes_and_mixed_windows_at_every_block_size():
    """The width-class pages and the call of big, tiny, overlapping and repeated windows at the three block sizes."""
    print()
    total, bad = 0, []
    for case in (T.width_class_case(), T.refine_cases()[2], in_mode(T.refine_cases()[2], 1)):
        before = []
        for nt in T.BLOCK_SIZES:
            n, b, bm, _ = _run_keyed(case, {"tail_lds_threads": nt}, f" [tail_lds_threads = {nt}]")
            total, bad = total + n, bad + b
            before.append(bm)
        assert before[0] == before[1] == before[2], "the records before the merge stage differ between the block sizes"
    report("width classes, mixed windows x block sizes", total, bad)


def test_block_size_key_is_clamped_to_256_512_1024():
    """`tail_lds_threads` = 0, 300, 513, 4096 launch 256, 256, 512, 1024 threads (the log shows what the launcher used, not
    what the key said), on the smallest call: one window."""
    print()
    case, total, bad = T.refine_cases()[0], 0, []
    for value, nt in ((0, 256), (300, 256), (513, 512), (4096, 1024)):
        assert T.clamped_threads(value) == nt
        n, b, _, launches = _run_keyed(case, {"tail_lds_threads": value}, f" [tail_lds_threads = {value}]")
        assert [g["threads"] for g in launches] == [nt], (value, launches)
        total, bad = total + n, bad + b
    report("block size clamp", total, bad)


def test_launch_classes():
    """`tail_lds_cls0 / cls1` on windows of 1 to 4 515 words, both refine modes: under every setting of
    `tail_trace_cases.class_settings` the logged launches are those of the restatement (the 1 x 1 window in the LDS layout
    of the largest one included), every window is merged in LDS without overflow, and the results equal the oracle."""
    print()
    total, bad = 0, []
    for mode in (0, 1):
        case = in_mode(T.class_case(), mode)
        for what, tune in T.class_settings():
            n, b, _, _ = _run_keyed(case, tune, f" [{what}]", {"lds": 11, "canvas": 0, "overflow": 0})
            total, bad = total + n, bad + b
    report("class_case x class limits x refine modes", total, bad)


@functools.lru_cache(None)
def speckle_case():
    """One window (164 x 104: 624 words) over the 7 x 7 squares of test_gpu_e2e's speckle page: about two runs per word."""
    from test_gpu_e2e import _speckle_page
    page, mask = _speckle_page(256, 320, 7)
    return T._case("speckle window", [page], [mask], [[[100, 60, 250, 150]]])


def test_run_capacity():
    """`tail_lds_runs_x10` = 1 / 25 / 160 / 1000 (floor 1 024, 2.5, 16 and 100 runs per word): the logged rcap and LDS bytes
    and the routing are the restatement's -- windows move to the canvases as the need grows --, the overflows are exactly the
    windows whose run count by the emulation exceeds their launch's rcap, the speckle window does not overflow at 16 per
    word, the 2 080-word window completes in LDS at 0.1 per word in a layout with rlay > rcap, and all results equal the
    oracle and, before the merge stage, each other."""
    print()
    total, bad = 0, []
    runs = (1, 25, 160, 1000)
    for fn in (T.class_case, T.large_window_case, speckle_case):
        for mode in (0, 1):
            case, before = in_mode(fn(), mode), []
            for r in runs:
                want = T.expected_paths(fn, mode, {"tail_lds_runs_x10": r})
                n, b, bm, launches = _run_keyed(case, {"tail_lds_runs_x10": r}, f" [tail_lds_runs_x10 = {r}]", want)
                total, bad = total + n, bad + b
                before.append(bm)
                if fn is speckle_case and r == 160:
                    assert want == {"lds": 1, "canvas": 0, "overflow": 0}
                if fn is T.large_window_case and r == 1:
                    (g,) = launches
                    assert (g["max_words"] + 1) // 2 > g["rcap"] == 1024 and want == {"lds": 1, "canvas": 0, "overflow": 0}, (g, want)
            assert all(bm == before[0] for bm in before), "the records before the merge stage differ between run capacities"
    report("run capacity", total, bad)
