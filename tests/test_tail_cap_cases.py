"""No GPU: every case of tests/tail_cap_cases.py is what it claims, and the comparisons of tests/test_gpu_tail_caps.py would see
the faults the cases are there for.

  * `COMP_CAP` / `ROW_CAP` are the `kCompCap` / `kRowCap` of csrc/tail.hip, read from the source: a changed capacity fails here
    instead of making the cases vacuous.
  * DB maps: n_f, n_b and the row entries of f_at / f_over (65 536 / 65 537, 2, 65 570 / 65 571), b_at / b_over (3, 65 536 /
    65 537, 197 118 / 197 121) and r_at / r_over (515 / 516, 2, 262 144 / 262 145) by the oracle's labelling; the bar and the
    ring are the last two foreground components, the ring's hole the last background one, both score above 0.6 in
    `R.boxes_from_bitmap`; f_over without its last component gives other boxes, and `compare_boxes` reports it.
  * undetected pass: the blob of u_at is component 65 536 of 65 536, that of u_over 65 537 of 65 537, those of u_far 70 401 ..
    70 403 with covered fractions none / exactly 0.5 / 0.488; the oracle's pass with its statistics cut to the first 65 536 rows
    (the wrong tail, on paper) equals the full one on u_at and differs on u_over and u_far, in both refine modes; every blob
    that becomes a window refines to some of its pixels and not to all.
  * canvas bound: the windows are the ones asked for (even origin, odd size), every candidate of every window has exactly
    ((w + 1) / 2) * ((h + 1) / 2) components (1, 4, 2 145 and 272), the call holds no other window, and so the components of
    all its bands together (4 844) are `refine_canvas`'s `cap1` - 1; the text-like window is a call of its own.
  * u_grow: 90 113 components; the relabelling's table (1.8 MB) is larger than what a one-page call has allocated (1.64 MB),
    those of u_over and u_far are not."""
import os
import re

import numpy as np
import pytest

import tail_cap_cases as K
import tail_trace_cases as T
from conftest import ROOT
from oracle import postproc_ref as R
from test_gpu_sweeps import collect_mismatches, compare_boxes


def test_capacities_are_those_of_the_source():
    src = open(os.path.join(ROOT, "comic-text-detector_amd", "csrc", "tail.hip")).read()
    got = {}
    for name in ("kCompCap", "kRowCap"):
        m = re.findall(r"constexpr\s+int\s+%s\s*=\s*1\s*<<\s*(\d+)\s*;" % name, src)
        assert len(m) == 1, f"{name}: {len(m)} definitions of the form `constexpr int {name} = 1 << n;` in csrc/tail.hip"
        got[name] = 1 << int(m[0])
    assert (K.COMP_CAP, K.ROW_CAP) == (T.COMP_CAP, T.ROW_CAP) == (got["kCompCap"], got["kRowCap"])


@pytest.mark.parametrize("name", K.AT + K.OVER)
def test_db_map_counts(name):
    prob = K.db_maps()[name]
    assert prob.shape == K.DB_SHAPE and prob.dtype == np.float32
    nf, nb, rows = K.DB_COUNTS[name]
    assert T.db_counts(prob) == (nf, nb) and K.db_rows(prob) == rows
    want = {"f_at": (K.COMP_CAP, 2), "f_over": (K.COMP_CAP + 1, 2), "b_at": (3, K.COMP_CAP), "b_over": (3, K.COMP_CAP + 1),
            "r_at": (515, 2), "r_over": (516, 2)}[name]
    assert (nf, nb) == want
    if name[0] == "r":
        assert rows == K.ROW_CAP + (name == "r_over") and nf < 2000 and nb < 2000
    else:
        assert rows < K.ROW_CAP                                # only the count under test is at its capacity
    assert K.overflows(name) == (name in K.OVER)
    if name in K.AT:                                           # the emulation the tables are compared with counts the same
        t = K.db_tables(name)
        assert (int(t["n_f"]), int(t["n_b"]), int(t["rows"])) == (nf, nb, rows)


@pytest.mark.parametrize("name", K.AT + K.OVER + ("fits 2", "fits 7"))
def test_the_two_shapes_come_last_and_score(name):
    """Bar and ring are the last foreground components in raster order (r_over: before its extra pixel), the ring's hole the
    last background component; the oracle gives both a box with a score above 0.6."""
    prob = K.db_maps()[name]
    bitmap = (prob > 0.3).astype(np.uint8)
    n, _, st = R.connected_components_with_stats(bitmap, 8)
    last = st[-3:-1] if name == "r_over" else st[-2:]
    for s, (y, x, h, w) in zip(last, (K.BAR, K.RING)):
        assert [int(v) for v in s[:4]] == [x, y, w, h] and h >= 3
    assert int(st[-2 if name == "r_over" else -1][4]) == K.RING[2] * K.RING[3] - K.HOLE[2] * K.HOLE[3]
    nb, _, sb = R.connected_components_with_stats(1 - bitmap, 4)
    y, x, h, w = K.HOLE
    assert [int(v) for v in sb[-1]] == [x, y, w, h, w * h]
    boxes, scores = K.db_oracle(name)
    assert (scores > 0.6).sum() == 2, scores[scores > 0]
    if name in K.DB_COUNTS:                                    # the specks themselves give no box: the shapes decide the result
        assert (scores > 0).sum() <= 3


def test_a_table_one_entry_short_changes_the_boxes_of_f_over():
    prob = K.db_maps()["f_over"]
    cut = K.erase_last_component(prob)
    assert T.db_counts(cut) == (K.COMP_CAP, 1)
    got = R.boxes_from_bitmap(cut, cut > 0.3, prob.shape[1], prob.shape[0])
    full = K.db_oracle("f_over")
    assert (got[1] > 0.6).sum() == 1 and (full[1] > 0.6).sum() == 2
    assert len(collect_mismatches([("f_over, last component lost", got, full)], compare_boxes)) == 1
    assert not collect_mismatches([("f_over", K.db_oracle("f_over"), full)], compare_boxes)


def test_db_batches():
    maps = K.db_maps()
    assert [len(b) for b in K.DB_BATCHES] == [3, 2]
    for batch in K.DB_BATCHES:
        assert len({maps[n].shape for n in batch}) == 1
    assert [K.overflows(n) if n in K.DB_COUNTS else False for n in K.DB_BATCHES[0]] == [False, True, False]
    assert K.DB_BATCHES[1][0] == "b_over"
    for n in ("fits 2", "fits 7"):
        t = K.db_tables(n)
        assert 10 < t["n_f"] < 1000 and 10 < t["n_b"] < 1000 and t["rows"] < 10000


# ------------------------------------------------------------------------------------------------------- undetected pass

def test_blob_ranks():
    u = K.undetected_cases()
    assert all(c["keep"] and len(c["pages"]) == 1 and c["pages"][0].shape == (K.U_SIZE, K.U_SIZE, 3) for c in u.values())
    n, blobs = K.blob_ranks(u["u_at"])
    assert n == K.COMP_CAP and [b[0] for b in blobs] == [K.COMP_CAP] and not u["u_at"]["boxes"][0]
    n, blobs = K.blob_ranks(u["u_over"])
    assert n == K.COMP_CAP + 1 and [b[0] for b in blobs] == [K.COMP_CAP + 1] and not u["u_over"]["boxes"][0]
    n, blobs = K.blob_ranks(u["u_far"])
    assert n == K.FAR_SPECKS + 3 and [b[0] for b in blobs] == [K.FAR_SPECKS + 1, K.FAR_SPECKS + 2, K.FAR_SPECKS + 3] and K.FAR_SPECKS >= 70000
    assert all(b[1][2] - b[1][0] == K.BLOB[0] and b[1][3] - b[1][1] == K.BLOB[1] for b in blobs)
    assert blobs[0][2] < 0 and blobs[1][2] == 0.5 and 0.4 < blobs[2][2] < 0.5          # the `< 0.5` rule on both sides
    n, blobs = K.blob_ranks(u["u_grow"])
    assert n == K.GROW_SPECKS + 1 and [b[0] for b in blobs] == [n]
    # the relabelling's table: within the buffer a one-page call has allocated for u_over and u_far, beyond it for u_grow
    assert K.relabel_bytes(K.COMP_CAP + 1) < K.relabel_bytes(K.FAR_SPECKS + 3) <= K.FIRST_TABLE_BYTES < K.relabel_bytes(n)


@pytest.mark.parametrize("mode", (0, 1))
@pytest.mark.parametrize("name", ("u_at", "u_over", "u_far", "u_grow"))
def test_a_tail_that_keeps_only_the_first_rows_is_seen(name, mode):
    case = K.undetected_cases()[name]
    img, mask, boxes = case["pages"][0], case["masks"][0], case["boxes"][0]
    blks = [R.TextBlock(list(b)) for b in boxes]
    first = R.refine_mask(img, mask, blks, mode)
    full = R.refine_undetected_mask(img, mask.copy(), first.copy(), blks, mode)
    cut = K.undetected_truncated(img, mask.copy(), first.copy(), boxes, mode)
    assert np.array_equal(full, cut) == (name == "u_at")
    _, blobs = K.blob_ranks({**case, "mode": mode})
    for rank, (x1, y1, x2, y2), covered in blobs:
        inside = full[y1:y2, x1:x2]
        if covered < 0.5:                                      # a window: refined pixels on both sides
            assert 500 < (inside > 0).sum() < inside.size - 500, (name, rank)
            if rank > K.COMP_CAP:
                assert not cut[y1:y2, x1:x2].any()
        else:
            assert not inside.any(), (name, rank)


def test_undetected_batches():
    same, mixed = K.undetected_batches()
    u = K.undetected_cases()["u_over"]
    for case in (same, mixed):
        assert len(case["pages"]) == 3 and case["keep"] and case["masks"][1] is u["masks"][0] and case["boxes"][1] == []
        assert all(len(b) == 2 for b in (case["boxes"][0], case["boxes"][2]))
    sizes = [m.shape for m in same["masks"]]
    assert len(set(sizes)) == 1 and sizes[0][0] * sizes[0][1] % 256 == 0           # back to back: one labelling launch
    assert len({m.shape for m in mixed["masks"]}) == 3
    for case in (same, mixed):                                 # the pages next to u_over have something to refine
        _, refined, _ = T.refine_reference(K.single_page(case, 0))
        assert (refined[0] > 0).sum() > 500


# ---------------------------------------------------------------------------------------------------------- canvas bound

def test_canvas_windows_hold_one_component_per_cell():
    case = K.canvas_case()
    assert [m.shape[1] for m in case["masks"]] == [160, 101]
    recs, refined, _ = T.refine_reference(case)
    seen, labels, cap1, k = [], 0, 1, 0
    for img, mask, boxes, (size, wins) in zip(case["pages"], case["masks"], case["boxes"], K.CANVAS_PAGES):
        assert T.windows_of(img.shape, boxes) == wins                     # nothing but the dot windows in the call
        for x1, y1, w, h in wins:
            assert x1 % 2 == 0 and y1 % 2 == 0 and w % 2 == 1 and h % 2 == 1
            counts = K.candidate_components(img, mask, (x1, y1, w, h))
            assert counts and all(c == K.cell_bound(w, h) for c in counts), (w, h, counts)
            assert len(counts) == int(recs[k]["n_cand"])                  # one band of the canvas per candidate
            labels, cap1, k = labels + sum(counts), cap1 + len(counts) * K.cell_bound(w, h), k + 1
            seen.append((w, h))
    assert sorted(seen) == sorted(K.CANVAS_SIZES) and [K.cell_bound(w, h) for w, h in K.CANVAS_SIZES] == [1, 4, 272, 2145]
    # `refine_canvas`: cap1 = 1 + the sum of the bounds over all bands of the call; the canvas labelling returns cap1 - 1 labels
    assert k == len(recs) == 4 and labels == cap1 - 1 == 2 * (1 + 4 + 272 + 2145)
    assert not refined[0].any() and not refined[1].any()      # dots alone are refused (w * h < 3)


def test_canvas_text_case_is_a_call_of_its_own_and_refines_to_something():
    case = K.canvas_text_case()
    assert T.windows_of(case["pages"][0].shape, case["boxes"][0]) == [K.TEXT_WINDOW]
    counts = K.candidate_components(case["pages"][0], case["masks"][0], K.TEXT_WINDOW)
    assert sum(counts) < K.cell_bound(*K.TEXT_WINDOW[2:])                 # far from the bound: why it is kept out of the dots' call
    _, refined, _ = T.refine_reference(case)
    assert (refined[0] > 0).sum() > 500
