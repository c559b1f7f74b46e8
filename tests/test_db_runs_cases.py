"""The maps of tests/db_runs_cases.py do what tests/test_gpu_db_runs.py needs them to, checked without a GPU on the emulated
tables (tests/dbc_emul.py): where the segment skip of `dbc_accum_kernel` must be off it would lose something, where it is on
it has segments to skip and segments to keep, and a skipped segment never held a contribution."""
import numpy as np

import db_runs_cases as D
from dbc_emul import dbc_tables


def _pages():
    seen = set()
    for _, _, maps in D.calls():
        for name, prob in maps:
            if name not in seen:
                seen.add(name)
                yield name, prob, dbc_tables(prob, prob > 0.3)
    yield "big", D.big_map(), None


def test_background_one_is_a_hole_exactly_where_the_cases_say():
    n_hole = 0
    for name, prob, t in _pages():
        if t is None or t["n_b"] == 0:
            assert name not in D.HOLE_FIRST
            continue
        hole_first = bool(t["par_b"][0] > 0)
        assert hole_first == (name in D.HOLE_FIRST), name
        flags = D.segment_flags(t)
        if hole_first:
            n_hole += 1
            clear = np.repeat(~flags, 64)[: prob.size].reshape(prob.shape)
            if name in ("frame", "frame 257 x 131"):     # a skip taken here by mistake drops a good part of the hole's sum
                assert prob[clear].sum() > 0.2 * t["sum_b"][0] > 0, name
            elif name != "frame 33 x 65":                # (65 wide: every segment holds a frame pixel)
                assert clear.any() and t["sum_b"][0] > 0, name
    assert n_hole == len(D.HOLE_FIRST)


def test_skipped_segments_hold_no_contribution_and_both_kinds_of_segment_occur():
    mixed = 0
    for name, prob, t in _pages():
        if t is None or t["n_b"] == 0 or t["par_b"][0] > 0:
            continue
        flags = D.segment_flags(t)
        clear = np.repeat(~flags, 64)[: prob.size]
        lab_f, lab_b = t["lab_f"].ravel(), t["lab_b"].ravel()
        assert not lab_f[clear].any() and (lab_b[clear] == 1).all(), name
        # a foreground pixel next to a hole (a ring pixel) and every hole pixel sit in kept segments
        hole_px = np.isin(lab_b, 1 + np.nonzero(t["par_b"] > 0)[0])
        assert not hole_px[clear].any(), name
        mixed += bool(flags.any() and (~flags).any())
    assert mixed >= 4                                    # the text pages at the three shapes and the late background


def test_segments_straddle_rows_and_pages_end_in_partial_segments():
    shapes = {prob.shape for _, _, maps in D.calls() for _, prob in maps}
    assert any(w % 64 for _, w in shapes) and any((h * w) % 64 for h, w in shapes) and (64, 64) in shapes
    assert {(1, 70), (70, 1), (33, 65), (96, 160), (257, 131)} <= shapes
    ink = D.big_map() > 0.3
    assert 0.01 < ink.mean() < 0.08


def test_pages_with_and_without_holes_share_a_call():
    """`hole_rows` = 0 switches the ring test off per page: both kinds, each with ink, in the mixed calls."""
    for index in (0, 2):
        _, _, maps = D.calls()[index]
        holes = {name: int((dbc_tables(prob, prob > 0.3)["par_b"] > 0).sum()) for name, prob in maps if (prob > 0.3).any()}
        assert any(v > 0 for v in holes.values()) and any(v == 0 for v in holes.values()), holes
    solid = dict(D.calls()[2][2])["solid 257 x 131"]
    t = dbc_tables(solid, solid > 0.3)
    assert t["n_f"] >= 4 and t["n_b"] == 1
