"""-m gpu: every batch of a long `TextDetector.detect_stream` against the unpipelined run.  The kernels behind the pipeline are
held against references all over the suite; here it is the hand-overs between them -- `job["ev"]` into `ctd_tail_run`,
`main.wait_event(ev)` behind `_stage`, `slot["ev"].synchronize()` before a pinned slot is used again, `st.wait_stream(main)` of
the lanes, the job dict that keeps a forward's outputs and the staged pages alive -- at steady state: streams longer than
`depth` and the pinned rings (tests/stream_cases.py, checked in tests/test_stream_cases.py), whose consecutive batches give
different answers (blank, dense, blank, ...), so bytes left over from the batch before or after are wrong bytes.

REFERENCE: `detect_batch` on device-resident pages, batch after batch, on a second `TextDetector` (its engine; the main thread's
tail) that never streams, computed for every sequence and option before the first stream of this file starts (`refs()`), and
never written to afterwards.  What is asserted on it alone, before any comparison: every blank batch has 0 blocks and all-zero
refined masks, every dense batch at least 6 blocks and a refined mask that is not, every sparse batch at least 6 blocks, no two
consecutive batches have equal masks.  COMPARISON: after the generator is exhausted, with every yielded result still held;
`mask` and `mask_refined` with `assert_array_equal`, the blocks with `test_post_host.blocks_equal`.

The checkpoint is `stream_cases.stream_checkpoint()`: the suite's random checkpoints answer a flat page with 6 .. 41 blocks.

SIZES OF THE LAPPING CASES (test 4).  Measured on the MI355X in the sequential reference run (`refs()`): a batch's forward between
two events around `net.forward_u8`, a work item's tail from `thread_tail(dev).timings()["total"]` (one item = one batch:
`tail_split` = 1), medians over the twelve batches.
  * forward_heavy: 8 pages of 512 x 512 gave forward 1.84 ms, tail 1.07 ms (0.7 on the blank batches, 1.3 on the sparse ones):
    1.72, short of 2.  The forward is bound by its ~100 launches at these sizes, so the next sizes gain little; at the cap,
    8 pages of 1024 x 1024 -- what runs --: forward 3.02 / 3.03 ms, tail 1.31 / 1.47 ms (1.0 blank, 1.5 sparse) in two runs:
    forward / tail = 2.30 / 2.06 over all batches, 3.0 on the blank and 2.0 on the sparse ones.
  * tail_heavy: 3 dense pages of 256 x 256 (`n_blocks` 12, ~110 blocks a page) gave forward 1.48 ms, tail 1.96 ms: 1.3, short
    of 2.  4 pages of 512 x 512 with `n_blocks` 16 -- what runs --: forward 1.57 / 1.58 ms, tail 4.20 / 4.83 ms:
    tail / forward = 2.7 / 3.1.
The test prints both times of every batch of its run; it asserts none of them.

SEEN / NOT SEEN, with one hand-over taken out of detector.py at a time (each edit run twice, never committed):
  * `None` for `job["ev"]` in `_tail`: 18 of the 26 tests of the first version of this file fail -- every stream of real pages
    but `tail_heavy`, where the tail starts long after its forward has ended; 2 .. 26 of 26 batches differ.
  * no `slot["ev"].synchronize()` in `_stage`: the host streams with ONE loader fail (alternating: batches 3, 4, 5 of 26;
    mixed_sizes: batch 3 of 20 in one of the two runs) -- the loader refills a slot whose upload has not read it yet.
  * no `main.wait_event(ev)`, no `st.wait_stream(main)`: NOT seen, in either run.  The host streams were meant to see both (the
    second through `engines` = 2), the 25-MB uploads of `forward_heavy` in particular: pages are staged `depth` batches
    ahead, and their upload has ended by the time their forward is launched.

WALL TIME on the MI355X: the whole file 16 s, 28 tests.  The first test that runs makes all the references and the six
detectors: 5.4 s; the three calls on device pages 0.6 - 0.7 s per case; the host streams 0.1 - 0.3 s, those of `forward_heavy`
0.7 s; the options 0.1 - 0.3 s; `forward_heavy` 0.4 s, `tail_heavy` 0.6 s; the stubs 0.05 - 0.5 s.
"""
import threading
import time

import numpy as np
import pytest
import torch

import stream_cases as SC
from conftest import pkg
from test_gpu_line_batches import batches_equal
from test_post_host import blocks_equal

pytestmark = pytest.mark.gpu

RECORDS = (64, 256)
BOOKKEEPING = dict(n=12, pages=4, depth=3, workers=3)

# Every `detect_stream` call of this file on real pages: (sequence, keywords).  tests/test_stream_cases.py holds each against
# `depth` + the pinned slots of its loaders.
DEVICE_RUNS = [("alternating", dict(workers=3, depth=4, tail_split=split, engines=engines)) for split in (1, 4) for engines in (1, 2)]
HOST_RUNS = [(name, dict(workers=3, depth=4, loaders=loaders)) for name in ("alternating", "mixed_sizes") for loaders in (1, 2)] + \
            [("alternating", dict(workers=3, depth=1, loaders=2)), ("alternating", dict(workers=3, depth=6, loaders=2)),
             ("alternating", dict(workers=3, depth=4, loaders=2, engines=2)),   # the lanes' `wait_stream(main)` carries the upload
             # uploads of 25 MB a batch: the copy of a batch takes as long as a third of its forward
             ("forward_heavy", dict(workers=3, depth=4, loaders=1, tail_split=1)),
             ("forward_heavy", dict(workers=3, depth=4, loaders=2, tail_split=1, engines=2))]
OPTION_RUNS = [("alternating", dict(workers=3, depth=4, lazy=True)),
               ("alternating", dict(workers=3, depth=4, records=RECORDS)),
               ("alternating", dict(workers=3, depth=4, keep_undetected_mask=True, refine_mode=1)),
               ("alternating", dict(workers=3, depth=4, font_colors=True)),
               ("alternating", dict(workers=3, depth=4, tail_split=2, line_batches={}))]
LAPPING_RUNS = [("forward_heavy", dict(workers=3, depth=4, tail_split=1)),
                ("tail_heavy", dict(workers=1, depth=4, keep_undetected_mask=True, refine_mode=1))]
STUB_RUNS = [("stubs", dict(workers=BOOKKEEPING["workers"], depth=BOOKKEEPING["depth"], tail_split=s)) for s in (1, 2, 5, 9)]
STREAMS = DEVICE_RUNS + HOST_RUNS + OPTION_RUNS + LAPPING_RUNS + STUB_RUNS


def _id(run):
    return run[0] + "-" + "-".join(f"{k}{v}" for k, v in run[1].items() if k != "workers")


# ---------------------------------------------------------------------------------------------------------------- the two sides

_DET = {}


def detectors(size):
    """(the detector that streams, the one that makes the references) at `size`."""
    if size not in _DET:
        ck = SC.stream_checkpoint()
        _DET[size] = tuple(pkg().detector.TextDetector(ck, input_size=size, device="cuda", half=True) for _ in range(2))
    return _DET[size]


def size_of(name):
    return {"forward_heavy": SC.FORWARD_HEAVY["size"], "tail_heavy": SC.TAIL_HEAVY["size"]}.get(name, 256)


_REFS = {}


def _reference(name, seq, timed=False, refine_mode=None, keep_undetected_mask=False, font_colors=False, records=None):
    """`detect_batch` of every batch of `seq` on device pages, one after the other, on the reference detector -- its two halves
    (`_forward`, then `_tail` / `_tail_colors`) with the device idle in between.  `timed`: also the forward (two events around
    `net.forward_u8`) and the tail (`timings()["total"]`) of every batch, in ms."""
    _, ref = detectors(size_of(name))
    dev = ref.net.device
    mode, keep = pkg().textmask.REFINEMASK_INPAINT if refine_mode is None else refine_mode, keep_undetected_mask
    run_tail = ref._tail_colors if font_colors else (lambda job, mode, keep: ref._tail(job, mode, keep, records=records))
    tail = pkg().tail.thread_tail(dev)
    inner, marks = ref.net.forward_u8, []

    def forward_u8(x):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(torch.cuda.current_stream(dev))
        out = inner(x)
        e1.record(torch.cuda.current_stream(dev))
        marks.append((e0, e1))
        return out

    if timed:
        ref.net.forward_u8 = forward_u8
    try:
        out, tails = [], []
        for _, pages in seq:
            job = ref._forward([torch.from_numpy(p).to(dev) for p in pages])
            torch.cuda.synchronize(dev)                               # the reference leans on none of the waits under test
            out.append(run_tail(job, mode, keep))
            tails.append(tail.timings()["total"])
    finally:
        if timed:
            del ref.net.forward_u8
    torch.cuda.synchronize(dev)
    return out, ([a.elapsed_time(b) for a, b in marks], tails)


def _not_vacuous(name, seq, want, undetected=False):
    """The conditions on the reference alone.  `undetected`: the run keeps the undetected mask, which refines what the UNet's
    mask holds outside every block -- on a blank page too; the blocks are what a blank batch must not have."""
    for k, ((kind, _), res) in enumerate(zip(seq, want)):
        blocks, refined = sum(len(r[2]) for r in res), sum(int(r[1].any()) for r in res)
        if kind == SC.BLANK:
            assert blocks == 0 and (refined == 0 or undetected), \
                f"{name}: blank batch {k} has {blocks} blocks, {refined} pages with a refined mask"
        elif kind == SC.SPARSE:                                       # (two patches a page refine nothing on many a page: with the
            assert blocks >= 6, f"{name}: sparse batch {k} has {blocks} blocks"       # oracle, none of the 8 pages of one batch)
        else:
            assert blocks >= 6 and refined >= 1, f"{name}: {kind} batch {k} has {blocks} blocks, {refined} pages with a refined mask"
    for k, (a, b) in enumerate(zip(want, want[1:])):
        same = len(a) == len(b) and all(x[0].shape == y[0].shape and np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1])
                                        for x, y in zip(a, b))
        assert not same, f"{name}: batches {k} and {k + 1} have equal masks"


def refs():
    """Every reference of this file, made once, before the first stream: `plain` per sequence, the option variants of
    `alternating`, the tail-heavy options of `tail_heavy`; `times` = (forward ms, tail ms) per batch of the lapping cases."""
    if _REFS:
        return _REFS
    seqs = {name: make() for name, make in SC.SEQUENCES.items()}
    out = dict(seqs=seqs, plain={}, times={})
    for name in ("alternating", "mixed_sizes", "forward_heavy"):
        if name == "forward_heavy":
            _reference(name, seqs[name][:2])                          # (the engine's plan and the tail's tables at this size exist)
        out["plain"][name], out["times"][name] = _reference(name, seqs[name], timed=True)
        _not_vacuous(name, seqs[name], out["plain"][name])
    heavy = dict(keep_undetected_mask=True, refine_mode=1)
    out["keep"] = _reference("alternating", seqs["alternating"], **heavy)[0]
    _reference("tail_heavy", seqs["tail_heavy"][:2], **heavy)         # (plan and tables at this size, as above)
    out["tail_heavy"], out["times"]["tail_heavy"] = _reference("tail_heavy", seqs["tail_heavy"], timed=True, **heavy)
    out["colors"] = _reference("alternating", seqs["alternating"], font_colors=True)[0]
    for key, name in (("keep", "alternating"), ("tail_heavy", "tail_heavy"), ("colors", "alternating")):
        _not_vacuous(f"{name} ({key})", seqs[name], out[key], undetected=key != "colors")
    out["records"] = _reference("alternating", seqs["alternating"], records=RECORDS)[0]
    assert all(r.record[0] == len(r[2]) for res in out["records"] for r in res) and \
        any(r.record[0] > 0 for res in out["records"] for r in res)
    _REFS.update(out)
    return _REFS


def device_batches(name):
    dev = detectors(size_of(name))[0].net.device
    return [[torch.from_numpy(p).to(dev) for p in pages] for _, pages in refs()["seqs"][name]]


def host_batches(name):
    return [pages for _, pages in refs()["seqs"][name]]


def compare(got, want, what, extra=None):
    """Every batch of a finished stream against the reference; reports ALL batches that differ."""
    assert len(got) == len(want), f"{what}: {len(got)} batches yielded, {len(want)} expected"
    bad = []
    for k, (gb, wb) in enumerate(zip(got, want)):
        try:
            assert len(gb) == len(wb)
            for (m, r, bl), (m1, r1, bl1) in zip(gb, wb):
                np.testing.assert_array_equal(m, m1)
                np.testing.assert_array_equal(r, r1)
                blocks_equal(list(bl), list(bl1))
            if extra is not None:
                extra(k, gb, wb)
        except AssertionError as e:
            bad.append((k, str(e).strip().splitlines()[0][:120] if str(e).strip() else "blocks"))
    assert not bad, f"{what}: {len(bad)} of {len(want)} batches differ from detect_batch: {bad[:6]}"


# ---- 1. device pages; pools, leases and lanes used again by later calls ---------------------------------------------------------

@pytest.mark.parametrize("run", DEVICE_RUNS, ids=_id)
def test_alternating_device_pages_three_calls_on_one_detector(run):
    name, kw = run
    want = refs()["plain"][name]
    det, _ = detectors(256)
    batches = device_batches(name)
    first = list(det.detect_stream(batches, tune=False, **kw))
    tails = pkg().tail.live_tails()
    again = [list(det.detect_stream(batches, tune=False, **kw)) for _ in range(2)]
    assert pkg().tail.live_tails() == tails
    for i, got in enumerate([first] + again):
        compare(got, want, f"{_id(run)}, call {i}")


# ---- 2. host pages through the pinned rings -----------------------------------------------------------------------------------

@pytest.mark.parametrize("run", HOST_RUNS, ids=_id)
def test_host_pages_through_the_pinned_rings(run):
    name, kw = run
    want = refs()["plain"][name]
    det, _ = detectors(size_of(name))
    got = list(det.detect_stream(host_batches(name), tune=False, **kw))
    compare(got, want, _id(run))


# ---- 3. the options of the benchmark's sub-runs -------------------------------------------------------------------------------

COLOUR_FIELDS = ("fg_r", "fg_g", "fg_b", "bg_r", "bg_g", "bg_b")


def _colours(res):
    return [[int(getattr(b, k)) for k in COLOUR_FIELDS] for r in res for b in r[2]]


@pytest.mark.parametrize("run", OPTION_RUNS, ids=_id)
def test_options_of_the_benchmark_sub_runs(run):
    name, kw = run
    R = refs()
    det, ref = detectors(256)
    batches = device_batches(name)
    got = list(det.detect_stream(batches, tune=False, **kw))
    if kw.get("lazy"):
        assert all(isinstance(r[2], pkg().textblock.BlockList) for res in got for r in res)     # materialised by `compare`, now
        compare(got, R["plain"][name], _id(run))
    elif kw.get("records"):
        def records(k, gb, wb):
            for g, w in zip(gb, wb):
                np.testing.assert_array_equal(g.record, w.record)
        compare(got, R["records"], _id(run), records)
    elif kw.get("keep_undetected_mask"):
        compare(got, R["keep"], _id(run))
    elif kw.get("font_colors"):
        def colours(k, gb, wb):
            assert _colours(gb) == _colours(wb)
        assert any(any(v) for res in R["colors"] for v in _colours(res))
        compare(got, R["colors"], _id(run), colours)
    else:
        results = [res for res, _ in got]
        for _, lbs in got:
            for lb in lbs:
                assert lb.wait() is lb
        compare(results, R["plain"][name], _id(run))
        lines = 0
        for k, ((res, lbs), pages, want) in enumerate(zip(got, batches, R["plain"][name])):
            starts = [lb.page0 for lb in lbs] + [len(pages)]
            assert starts == [lo for lo, _ in det._split(len(pages), kw["tail_split"])] + [len(pages)]
            for lb, lo, hi in zip(lbs, starts[:-1], starts[1:]):
                expect = ref.line_batches(pages[lo:hi], want[lo:hi])
                torch.cuda.synchronize()
                rel = lb.index.copy()
                rel[:, 0] -= lb.page0
                assert np.array_equal(rel, expect.index), f"batch {k}"
                lb.index, keep = rel, lb.index
                try:
                    batches_equal(lb, expect)
                finally:
                    lb.index = keep
                lines += len(lb.order)
        assert lines > 0


# ---- 4. one side clearly longer than the other ----------------------------------------------------------------------------------

@pytest.mark.parametrize("run", LAPPING_RUNS, ids=_id)
def test_forward_and_tail_lap_each_other(run):
    name, kw = run
    R = refs()
    want = R["plain"][name] if name == "forward_heavy" else R[name]
    fwd, tail = (float(np.median(v)) for v in R["times"][name])
    print(f"\n{name}: forward {fwd:.2f} ms, tail {tail:.2f} ms per batch in the sequential run "
          f"(forward / tail = {fwd / max(tail, 1e-9):.2f}); per batch {np.round(R['times'][name][0], 2).tolist()} / "
          f"{np.round(R['times'][name][1], 2).tolist()}")
    det, _ = detectors(size_of(name))
    got = list(det.detect_stream(device_batches(name), tune=False, **kw))
    compare(got, want, _id(run))


# ---- 5. the generator's own bookkeeping (no kernel is launched) -----------------------------------------------------------------

class Stubs:
    """Recording stand-ins for `_stage`, `_forward` and `_tail` on ONE detector instance; a batch is a list of its own number."""

    def __init__(self, det, seed, fail=None):
        self.det, self.fail, self.lock = det, fail, threading.Lock()
        self.delay = np.random.RandomState(seed).uniform(0.0, 0.020, (BOOKKEEPING["n"], BOOKKEEPING["pages"] + 1))
        self.started, self.yielded, self.worst, self.tails_in, self.tails_out = 0, 0, 0, 0, 0

    def __enter__(self):
        self.det._stage, self.det._forward, self.det._tail = self.stage, self.forward, self.tail
        return self

    def __exit__(self, *exc):
        del self.det._stage, self.det._forward, self.det._tail

    def stage(self, pages):
        return list(pages), None

    def forward(self, pages, net=None):
        with self.lock:
            self.started += 1
            self.worst = max(self.worst, self.started - self.yielded)
        return dict(k=pages[0], metas=[None] * len(pages))

    def tail(self, job, refine_mode, keep_undetected_mask, lo=None, hi=None, records=None, lazy=False):
        with self.lock:
            self.tails_in += 1
        try:
            time.sleep(float(self.delay[job["k"], lo]))
            if self.fail == (job["k"], lo):
                raise RuntimeError(f"work item {lo} of batch {job['k']}")
            return [(job["k"], lo, hi)]
        finally:
            with self.lock:
                self.tails_out += 1

    def consume(self, gen, limit=None):
        out = []
        for item in gen:
            with self.lock:
                self.yielded += 1
            out.append(item)
            if limit is not None and len(out) == limit:
                break
        return out


def stub_batches():
    return [[k] * BOOKKEEPING["pages"] for k in range(BOOKKEEPING["n"])]


def tiles(item, k, pages, parts):
    """The (k, lo, hi) records of one yielded batch tile [0, pages) in order, in min(parts, pages) pieces."""
    assert [r[0] for r in item] == [k] * min(parts, pages), item
    assert item[0][1] == 0 and item[-1][2] == pages and all(a[2] == b[1] for a, b in zip(item, item[1:])), item
    assert all(r[1] < r[2] for r in item), item


@pytest.mark.parametrize("run", STUB_RUNS, ids=_id)
def test_generator_bookkeeping_order_tiling_and_depth(run):
    _, kw = run
    det, _ = detectors(256)
    n, pages = BOOKKEEPING["n"], BOOKKEEPING["pages"]
    with Stubs(det, seed=kw["tail_split"]) as s:
        got = s.consume(det.detect_stream(stub_batches(), tune=False, **kw))
        assert len(got) == n and s.started == n
        for k, item in enumerate(got):
            tiles(item, k, pages, kw["tail_split"])
        assert 1 <= s.worst <= kw["depth"], s.worst
        assert s.tails_in == s.tails_out == n * min(kw["tail_split"], pages)


def test_generator_bookkeeping_an_exception_surfaces_at_its_batch():
    _, kw = STUB_RUNS[1]
    det, _ = detectors(256)
    n, pages = BOOKKEEPING["n"], BOOKKEEPING["pages"]
    with Stubs(det, seed=7, fail=(5, 2)) as s:
        gen = det.detect_stream(stub_batches(), tune=False, **kw)
        got = [next(gen) for _ in range(5)]
        with pytest.raises(RuntimeError, match="work item 2 of batch 5"):
            next(gen)
        with pytest.raises(StopIteration):
            next(gen)                                               # the generator has ended; its queued items are done
        assert s.tails_in == s.tails_out
        for k, item in enumerate(got):
            tiles(item, k, pages, kw["tail_split"])
    tails = pkg().tail.live_tails()
    with Stubs(det, seed=8) as s:                                   # a fresh call on the same detector
        got = s.consume(det.detect_stream(stub_batches(), tune=False, **kw))
        assert len(got) == n
        for k, item in enumerate(got):
            tiles(item, k, pages, kw["tail_split"])
    assert pkg().tail.live_tails() == tails


def test_generator_bookkeeping_closing_early_leaves_nothing_behind():
    _, kw = STUB_RUNS[1]
    det, _ = detectors(256)
    n, pages = BOOKKEEPING["n"], BOOKKEEPING["pages"]
    with Stubs(det, seed=11) as s:                                  # (the pool of three workers and their tails exist)
        assert len(s.consume(det.detect_stream(stub_batches(), tune=False, **kw))) == n
    tails = pkg().tail.live_tails()
    with Stubs(det, seed=9) as s:
        gen = det.detect_stream(stub_batches(), tune=False, **kw)
        got = s.consume(gen, limit=3)
        gen.close()
        assert [item[0][0] for item in got] == [0, 1, 2]
        assert s.tails_in == s.tails_out                            # every queued item has finished or was cancelled
        assert s.started <= 3 + kw["depth"]
    assert pkg().tail.live_tails() <= tails
    with Stubs(det, seed=10) as s:
        got = s.consume(det.detect_stream(stub_batches(), tune=False, **kw))
        assert len(got) == n and s.worst <= kw["depth"]
        for k, item in enumerate(got):
            tiles(item, k, pages, kw["tail_split"])
    # and the real thing after the stubs are gone
    want = refs()["plain"]["alternating"]
    compare(list(det.detect_stream(device_batches("alternating"), tune=False, **DEVICE_RUNS[1][1])), want, "after the stubs")


# ---- 6. depth < 1 -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("depth", [0, -1])
def test_depth_below_one_is_a_value_error_before_any_work(depth):
    det, _ = detectors(256)
    touched = []

    def batches():
        touched.append(1)
        yield from device_batches("alternating")

    pools = dict(det._pools)
    with pytest.raises(ValueError, match="depth"):
        next(det.detect_stream(batches(), depth=depth, tune=False))
    assert not touched and det._pools == pools
    # no detector and no GPU is needed to see it: the check is among the first statements of the generator
    bare = object.__new__(pkg().detector.TextDetector)
    with pytest.raises(ValueError, match="depth"):
        next(pkg().detector.TextDetector.detect_stream(bare, [], depth=depth))
