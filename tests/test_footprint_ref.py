"""The footprint rule's own promises, on the numpy restatement tests/footprint_ref.py (no GPU): the closure is idempotent,
contains its seed, is orthogonally convex and stays inside the seed's bounding box; on every subset of a 3 x 4 plane it is what
a search over all supersets finds; the 24-link chain takes 13 rounds; and the Python entry points refuse a bad `pad` or
`footprint` before they touch a GPU."""
import numpy as np
import pytest

import balloon_ref as BR
import erase_ref as ER
import footprint_ref as FR
from conftest import pkg


def _planes():
    rng = np.random.default_rng(33)
    for k in range(40):
        h, w = int(rng.integers(1, 40)), int(rng.integers(1, 90))
        yield rng.random((h, w)) < (0.002, 0.02, 0.2)[k % 3]
    yield np.zeros((5, 7), bool)
    yield np.ones((5, 7), bool)
    yield FR.chain()[0]


def test_closure_is_idempotent_convex_contains_the_seed_and_stays_in_its_box():
    for seed in _planes():
        q, _ = FR.closure(seed)
        assert (q | seed).sum() == q.sum() and FR.is_convex(q)
        again, rounds = FR.closure(q)
        assert rounds == 0 and np.array_equal(again, q)
        ys, xs = np.nonzero(seed)
        if len(xs):
            box = np.zeros_like(seed)
            box[ys.min():ys.max() + 1, xs.min():xs.max() + 1] = True
            assert not (q & ~box).any()
        else:
            assert not q.any()


def test_closure_equals_the_search_on_every_subset_of_a_3_by_4_plane():
    least, planes = FR.brute_closures(3, 4)
    assert len(planes) == 4096
    moved = 0
    for code in range(4096):
        q, _ = FR.closure(planes[code])
        assert np.array_equal(q, planes[least[code]]), code
        moved += int(least[code] != code)
    assert moved > 1000                                          # most subsets are not convex: the search did something


def test_closure_of_two_pieces_without_a_common_row_or_column_stays_two_pieces():
    seed = np.zeros((9, 9), bool)
    seed[0:3, 0:3] = seed[5:9, 4:9] = True
    assert np.array_equal(FR.closure(seed)[0], seed)


def test_the_chain_of_24_links_takes_13_rounds():
    plane, pts = FR.chain()
    q, rounds = FR.closure(plane)
    assert plane.shape == (74, 106) and len(pts) == 26 == int(plane.sum()) and int(q.sum()) == 339 and rounds == 13
    for other in (plane.T, plane[::-1], plane[:, ::-1]):           # transposed and mirrored: the same set, moved
        assert int(FR.closure(other)[0].sum()) == 339
    assert np.array_equal(FR.closure(plane.T)[0], q.T) and np.array_equal(FR.closure(plane[:, ::-1])[0], q[:, ::-1])
    # every link matters: without one, the chain stops there
    for drop in (2, 13, 25):
        less = plane.copy()
        less[pts[drop][1], pts[drop][0]] = False
        assert int(FR.closure(less)[0].sum()) < 339


def test_a_textured_block_gets_its_footprint_and_a_plain_one_keeps_its_balloon():
    """One page, a bar of text on a flat room and one on a noise field: the restatement's combined tables."""
    rng = np.random.default_rng(4)
    page = np.full((80, 200, 3), 230, np.uint8)
    page[:, 100:] = rng.integers(0, 256, (80, 100, 3), dtype=np.uint8)
    mask = np.zeros((80, 200), np.uint8)
    mask[30:34, 20:70] = mask[40:44, 30:60] = 255                  # two lines, plain
    mask[30:34, 120:170] = mask[40:44, 130:160] = 255              # two lines, on noise
    page[mask != 0] = 0
    boxes = [(18, 28, 72, 46), (118, 28, 172, 46)]
    rows, words, wins, erows = FR.footprint_page(page, mask, boxes)
    assert [e["status"] for e in erows] == [ER.PLAIN, ER.TEXTURED]
    assert rows[0]["flags"] & FR.FOOTPRINT == 0 and rows[1]["flags"] == FR.FOOTPRINT and rows[1]["status"] == BR.OK
    plain = BR.balloon_page(page, mask, boxes)
    assert rows[0] == plain[0][0] and np.array_equal(words[0], plain[1][0]) and not plain[1][1].any()
    # F_b: two bars grown by 2; the closure fills the gap between the lines over the shorter line's columns; pad 4 around it
    got = BR.unpack(words[1], wins[1][3] - wins[1][1], wins[1][2] - wins[1][0])
    want = np.zeros((80, 200), bool)
    want[28:36, 118:172] = want[36:46, 128:162] = True
    want = ER.dilate(want, 4)
    assert np.array_equal(got, want[wins[1][1]:wins[1][3], wins[1][0]:wins[1][2]])
    assert rows[1]["n_seed"] == erows[1]["n_fill"] == 8 * 54 + 8 * 34 and rows[1]["area"] == int(want.sum())
    off = FR.footprint_page(page, mask, boxes, footprint=False)
    assert off[0] == plain[0] and all(np.array_equal(a, b) for a, b in zip(off[1], plain[1]))


@pytest.mark.parametrize("bad", [dict(pad=17), dict(pad=-1), dict(pad=True), dict(footprint=1.5), dict(pad=2.0),
                                 dict(footprint=1, pad=4)])
def test_bad_pad_or_footprint_is_refused_without_a_gpu(bad):
    p = pkg()
    page, mask = np.zeros((8, 8, 3), np.uint8), np.zeros((8, 8), np.uint8)
    with pytest.raises(ValueError):
        p.balloons.balloon_regions([page], [mask], [[]], **bad)
    with pytest.raises(ValueError):
        p.balloons.check_footprint(bad.get("footprint", False), bad.get("pad", 4))
    p.balloons.check_footprint(True, 0), p.balloons.check_footprint(False, 16), p.balloons.check_footprint(np.bool_(True), np.int64(4))
    assert p._lib.BALLOON_FOOTPRINT == FR.FOOTPRINT and p._lib.FOOTPRINT_MAX_PAD == FR.MAX_PAD
