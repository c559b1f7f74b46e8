"""The texture fill rule (include/ctd_hip.h, `ctd_texture_fill`) on the CPU: the two numpy restatements of
tests/texture_ref.py agree to the byte, the hash has its pinned values, the rule has the properties the header states, and it
gains what DESIGN.md section 4.30 records over the pull-push fill it starts from.  No GPU, no library."""
import hashlib

import numpy as np
import pytest

import fill_ref
import texture_ref as T


def test_hash_pins():
    pins = (((0, 0, 0, 0, 0), 0), ((1, 0, 0, 0, 0), 0x6d523710), ((0, 1, 0, 0, 0), 0xc4a0e45c), ((5, 9, 3, 7, 0), 0x8956b9f4),
            ((8191, 8191, 88, 31, 12345), 0xbe08f714))
    for (x, y, s, k, seed), want in pins:
        assert T.hash32(x, y, s, k, seed) == want
        assert int(T.hash32(np.array([x]), np.array([y]), s, k, seed)[0]) == want
    x, y = np.arange(50), np.arange(50)[::-1]
    for rho in (1, 2, 32, 127):
        d = T.draw(x, y, 3, 4, 99, rho)
        assert d.min() >= -rho and d.max() <= rho
        assert d.tolist() == [T.draw(int(a), int(b), 3, 4, 99, rho) for a, b in zip(x, y)]
    assert T.radii(32) == [32, 16, 8, 4, 2, 1] and T.radii(127) == [127, 63, 31, 15, 7, 3, 1] and T.radii(1) == [1]


def _small_cases():
    """(name, page, hole, init, parameters) on pages of up to 40 x 50: every path of the rule at a size the loops can walk."""
    rng = np.random.default_rng(7)
    out = []

    def add(name, page, hole, init=None, **kw):
        out.append((name, page, hole, T.pull_push(page, hole) if init is None else init, kw))

    hole = np.zeros((30, 44), np.uint8)
    hole[9:17, 14:30] = 255
    add("tone-rect", T.tone_page(30, 44, 4), hole, n_em=2)
    add("diag-text", T.diag_page(40, 50), T.text_holes(40, 50), n_em=2, n_sweep=1, radius=12)
    hole = np.zeros((24, 31), np.uint8)
    hole[:9, 20:] = 3                                                # flush with a corner
    hole[20:, :4] = 1
    add("noise-corners", rng.integers(0, 256, (24, 31, 3), dtype=np.uint8), hole, n_em=2, radius=127, seed=4242)
    add("ramp-random0.02", fill_ref.ramp_page(26, 33), T._random(26, 33, 0.02, rng), n_em=1, n_sweep=1, n_init=1)
    add("noise-random0.04", rng.integers(0, 256, (25, 40, 3), dtype=np.uint8), T._random(25, 40, 0.04, rng), n_em=2, radius=2)
    add("noise-random0.5", rng.integers(0, 256, (12, 15, 3), dtype=np.uint8), T._random(12, 15, 0.5, rng))
    add("none", rng.integers(0, 256, (9, 12, 3), dtype=np.uint8), np.zeros((9, 12), np.uint8))
    add("all", rng.integers(0, 256, (9, 12, 3), dtype=np.uint8), np.full((9, 12), 9, np.uint8))
    add("6x9", rng.integers(0, 256, (6, 9, 3), dtype=np.uint8), T._random(6, 9, 0.2, rng))
    hole = np.zeros((7, 8), np.uint8)
    hole[0, 7] = 1
    add("7x8", fill_ref.ramp_page(7, 8), hole, radius=1)
    add("1x1", np.full((1, 1, 3), 5, np.uint8), np.ones((1, 1), np.uint8))
    hole = np.zeros((20, 28), np.uint8)
    hole[6:12, 8:19] = 255
    page = T.tone_page(20, 28, 6)
    add("tone-own-init", page, hole, init=rng.integers(0, 256, page.shape, dtype=np.uint8), n_em=3, radius=1)
    return out


SMALL = _small_cases()


@pytest.mark.parametrize("case", SMALL, ids=[c[0] for c in SMALL])
def test_loops_equal_vec_in_every_byte_and_field(case):
    _, page, hole, init, kw = case
    a, ra = T.texture_loops(page, hole, init, **kw)
    b, rb = T.texture_vec(page, hole, init, **kw)
    assert ra == rb
    assert np.array_equal(a, b), np.argwhere((a != b).any(axis=2))[:4].tolist()


def test_the_three_statuses_and_what_out_is():
    rows = {c[0]: T.texture_vec(*c[1:4], **c[4]) for c in SMALL}
    by = {c[0]: c for c in SMALL}
    for name in ("none",):
        out, row = rows[name]
        assert row["status"] == T.NO_HOLE and row["n_hole"] == row["n_target"] == row["n_unmatched"] == 0
        assert np.array_equal(out, by[name][1])
    for name in ("all", "6x9", "1x1", "noise-random0.5"):
        out, row = rows[name]
        _, page, hole, init, _ = by[name]
        assert row["status"] == T.NO_SOURCE and row["n_source"] == 0 and row["n_unmatched"] == row["n_target"] > 0
        assert np.array_equal(out, np.where((hole != 0)[:, :, None], init, page))
    out, row = rows["7x8"]
    # the one centre is (3, 3); with R = 1 only the targets (2, 4) and (3, 4) can reach it
    assert {f: row[f] for f in T.FIELDS[:4]} == {"status": T.OK, "n_hole": 1, "n_target": 16, "n_source": 1} and row["n_unmatched"] >= 14
    out, row = rows["noise-random0.04"]
    assert row["status"] == T.OK and 0 < row["n_unmatched"] < row["n_target"]
    assert rows["tone-rect"][1]["n_unmatched"] == 0 and rows["tone-rect"][1]["status"] == T.OK
    # a 7 x 7 page without a hole has exactly one centre
    assert T.texture_vec(np.zeros((7, 7, 3), np.uint8), np.zeros((7, 7), np.uint8), np.zeros((7, 7, 3), np.uint8))[1] == \
        {"status": T.NO_HOLE, "n_hole": 0, "n_target": 0, "n_source": 1, "n_unmatched": 0}


@pytest.mark.parametrize("case", SMALL, ids=[c[0] for c in SMALL])
def test_known_pixels_stay_and_filled_values_stay_in_range(case):
    _, page, hole, init, kw = case
    out, _ = T.texture_vec(page, hole, init, **kw)
    h = hole != 0
    assert np.array_equal(out[~h], page[~h])
    pool = np.concatenate([page[~h], init[h]])
    assert (out[h] >= pool.min(axis=0)).all() and (out[h] <= pool.max(axis=0)).all()


def test_one_colour_in_one_colour_out():
    rng = np.random.default_rng(3)
    colour = (17, 250, 133)
    page = np.full((30, 41, 3), colour, np.uint8)
    hole = T._random(30, 41, 0.03, rng)
    hole[10:16, 20:30] = 1
    out, row = T.texture_vec(page, hole, page.copy(), n_em=2)
    assert row["status"] == T.OK and np.array_equal(out, page)


def test_the_result_does_not_depend_on_what_stands_under_the_hole_or_beside_the_page():
    """`out` is a function of (page, mask, init, parameters): the page's own bytes under the hole are never read, and the
    mask's non-zero values are all alike."""
    _, page, hole, init, kw = SMALL[0]
    a = T.texture_vec(page, hole, init, **kw)[0]
    other = page.copy()
    other[hole != 0] = 123
    b = T.texture_vec(other, (hole != 0).astype(np.uint8), init, **kw)[0]
    assert np.array_equal(a[hole != 0], b[hole != 0])


def test_quality_texture_fill_quarters_the_error_of_the_pull_push_fill():
    """The condition of DESIGN.md section 4.30 on the rule: on each of the six screentone cases the mean error over the hole
    is at most a quarter of the pull-push fill's.  The figures are printed; the first case's bytes are pinned."""
    print()
    for name, page, hole in T.quality_cases():
        init = T.pull_push(page, hole)
        out, row = T.texture_vec(page, hole, init)
        e0, e1 = T.hole_error(init, page, hole), T.hole_error(out, page, hole)
        print(f"{name}: pull-push {e0:.2f}, texture fill {e1:.2f}, ratio {e1 / e0:.2f}, row {row}")
        if name == "tone4-rect":
            assert hashlib.sha256(out.tobytes()).hexdigest()[:16] == "f45237fdb2a0780a"
        assert row["status"] == T.OK and row["n_unmatched"] == 0
        assert e1 <= e0 / 4, name
