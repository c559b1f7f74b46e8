"""`ctd_group_output` (native host code, csrc/host_group.cpp; runs without a GPU) against the oracle's
restatement of reference utils/textblock.py:421-508 -- and against the reference's own `group_output`
(live where the reference tree is present, else its stored results: tests/refcode.py) -- on randomised pages: rotated / vertical / horizontal line quads in
clusters, yolo blocks around some clusters (all three languages), lines outside every block, blocks
without lines, boxes reaching outside the page, empty inputs.  Strict comparison: every detection
field of the record, `distance` / `vec` / `norm` / `weight` bit for bit, Python type of `font_size`."""
import copy

import numpy as np
import pytest

from conftest import pkg
from oracle import postproc_ref as R
from refcode import reference_post, reference_results


def random_page(seed, im_w=None, im_h=None):
    rng = np.random.RandomState(seed)
    im_w = im_w or int(rng.choice([640, 1024, 1400]))
    im_h = im_h or int(rng.choice([480, 1024, 1654]))
    lines, blines, cls = [], [], []
    for _ in range(rng.randint(0, 14)):
        vertical = rng.rand() < 0.5
        fs = rng.randint(8, 40)
        n = rng.randint(1, 7)
        length = rng.randint(30, 300)
        x0, y0 = rng.randint(0, im_w - 40), rng.randint(0, im_h - 40)
        ang = np.deg2rad(rng.choice([0, 0, 0, rng.uniform(-25, 25)]))
        c, s = np.cos(ang), np.sin(ang)
        quads = []
        for i in range(n):
            if rng.rand() < 0.15:
                continue                                   # a gap -> split candidates
            if vertical:
                ox, oy, w, h = x0 - i * fs * rng.uniform(1.1, 2.8), y0 + rng.randint(-5, 5), fs, length * rng.uniform(0.5, 1)
            else:
                ox, oy, w, h = x0 + rng.randint(-5, 5), y0 + i * fs * rng.uniform(1.1, 2.8), length * rng.uniform(0.5, 1), fs
            q = np.array([[0, 0], [w, 0], [w, h], [0, h]], np.float64)
            q = q @ np.array([[c, s], [-s, c]]) + [ox, oy]
            q[:, 0] = np.clip(q[:, 0], 0, im_w)
            q[:, 1] = np.clip(q[:, 1], 0, im_h)
            q = q.astype(np.int32)
            if np.linalg.norm(q[1] - q[0]) < 4 or np.linalg.norm(q[3] - q[0]) < 4 or \
               np.linalg.norm(q[2] - q[1]) < 4 or np.linalg.norm(q[3] - q[2]) < 4:
                continue                                   # clipped flat at the page border: font size 0 crashes the reference
            quads.append(q)
        if not quads:
            continue
        lines += quads
        if rng.rand() < 0.65:                               # a yolo block around (most of) the cluster
            pts = np.concatenate(quads)
            lo, hi = pts.min(0) + rng.randint(-12, 12, 2), pts.max(0) + rng.randint(-12, 12, 2)
            blines.append([lo[0], lo[1], hi[0], hi[1]])
            cls.append(rng.randint(0, 3))
    for _ in range(rng.randint(0, 3)):                      # blocks without lines, partly outside the page
        x, y = rng.randint(-30, im_w - 20), rng.randint(-30, im_h - 20)
        blines.append([x, y, x + rng.randint(10, 200), y + rng.randint(10, 200)])
        cls.append(rng.randint(0, 3))
    order = rng.permutation(len(lines))
    lines = np.array([lines[i] for i in order], np.int32).reshape(-1, 4, 2)
    mask = np.zeros((im_h, im_w), np.uint8)
    for q in lines:
        if rng.rand() < 0.8:
            lo, hi = q.min(0), q.max(0)
            mask[lo[1]: hi[1], lo[0]: hi[0]] = rng.randint(20, 256)
    for b in blines:
        if rng.rand() < 0.5:
            mask[max(b[1], 0): max(b[3], 0), max(b[0], 0): max(b[2], 0)] = rng.randint(20, 256)
    blks = (np.array(blines, np.int32).reshape(-1, 4), np.array(cls, np.int32), np.ones(len(cls)))
    return blks, lines, im_w, im_h, mask


def same_blocks(ours, theirs):
    assert len(ours) == len(theirs)
    for a, b in zip(ours, theirs):
        assert [int(v) for v in a.xyxy] == [int(v) for v in b.xyxy]
        assert np.array_equal(np.asarray(a.lines), np.asarray(b.lines))
        assert (a.language, bool(a.vertical), int(a.angle), bool(a.merged)) == \
               (b.language, bool(b.vertical), int(b.angle), bool(b.merged))
        assert float(a.font_size) == float(b.font_size)
        assert isinstance(a.font_size, float) == isinstance(b.font_size, float)
        np.testing.assert_array_equal(np.asarray(a.distance), np.asarray(b.distance))
        np.testing.assert_array_equal(np.asarray(a.vec), np.asarray(b.vec))
        assert float(a.norm) == float(b.norm) and float(a.weight) == float(b.weight)


@pytest.mark.parametrize("seed", range(60))
def test_native_group_output_equals_oracle(seed):
    p = pkg()
    blks, lines, im_w, im_h, mask = random_page(seed)
    use_mask = mask if seed % 5 else None
    got = p.textblock.group_output(copy.deepcopy(blks), lines.copy(), im_w, im_h, use_mask)
    ref = R.group_output(copy.deepcopy(blks), lines.copy(), im_w, im_h, use_mask)
    same_blocks(got, ref)


def grid_page(seed):
    """Clusters of axis-aligned integer quads on a grid (rows x columns of equal boxes, some missing), shuffled: lines of one row
    or column tie MATHEMATICALLY in `TextBlock.distance`, blocks reach 60 lines -- what the random quads above never produce
    (round 6: the seed sweep of the whole-tail test found the ties)."""
    rng = np.random.RandomState(seed)
    im_w, im_h = int(rng.choice([640, 1024, 1400])), int(rng.choice([640, 1024, 1654]))
    lines, blines, cls = [], [], []
    for _ in range(rng.randint(1, 6)):
        vertical = rng.rand() < 0.5
        fs, gap = int(rng.randint(10, 36)), int(rng.randint(2, 14))
        nrow, ncol = int(rng.randint(1, 9)), int(rng.randint(1, 9))
        x0, y0, length = int(rng.randint(0, im_w - 200)), int(rng.randint(0, im_h - 200)), int(rng.randint(20, 90))
        quads = []
        for r in range(nrow):
            for c in range(ncol):
                if rng.rand() < 0.2:
                    continue
                x, y, w, h = (x0 + c * (fs + gap), y0 + r * (length + gap), fs, length) if vertical else \
                             (x0 + c * (length + gap), y0 + r * (fs + gap), length, fs)
                if x + w < im_w and y + h < im_h:
                    quads.append(np.array([[x, y], [x + w, y], [x + w, y + h], [x, y + h]], np.int32))
        if not quads:
            continue
        lines += quads
        if rng.rand() < 0.7:
            pts = np.concatenate(quads)
            lo, hi = pts.min(0) - rng.randint(0, 10, 2), pts.max(0) + rng.randint(0, 10, 2)
            blines.append([lo[0], lo[1], hi[0], hi[1]])
            cls.append(int(rng.randint(0, 3)))
    if not lines:
        return grid_page(seed + 100000)
    order = rng.permutation(len(lines))
    lines = np.array([lines[i] for i in order], np.int32).reshape(-1, 4, 2)
    mask = np.zeros((im_h, im_w), np.uint8)
    for q in lines:
        if rng.rand() < 0.8:
            mask[q[0, 1]: q[2, 1], q[0, 0]: q[2, 0]] = rng.randint(20, 256)
    blks = (np.array(blines, np.int32).reshape(-1, 4), np.array(cls, np.int32), np.ones(len(cls)))
    return blks, lines, im_w, im_h, mask


@pytest.mark.parametrize("seed", range(40))
def test_native_group_output_equals_oracle_on_tied_lines(seed):
    """Grids of equal boxes: every distance ties with others.  `TextBlock.sort_lines` is `np.argsort` with numpy's default kind --
    x86-simd-sort for 64-bit keys on an AVX-512 / AVX2 host: the order of EQUAL distances in a block of more than 16 lines is that
    code's own -- on values whose last bit is numpy's SVML `arccos`.  The product calls both functions themselves
    (csrc/np_dispatch.h); the oracle makes the reference's calls literally.  Bit for bit, incl. `distance`."""
    p = pkg()
    blks, lines, im_w, im_h, mask = grid_page(seed)
    got = p.textblock.group_output(copy.deepcopy(blks), lines.copy(), im_w, im_h, mask)
    ref = R.group_output(copy.deepcopy(blks), lines.copy(), im_w, im_h, mask)
    same_blocks(got, ref)


def reference_group_output(name, blks, lines, im_w, im_h, mask):
    def compute():
        with np.errstate(all="ignore"):
            return reference_post().TB.group_output(copy.deepcopy(blks), lines.copy(), im_w, im_h, mask)
    return reference_results(name, compute)


@pytest.mark.parametrize("seed", range(0, 40, 2))
def test_native_group_output_equals_reference_code_on_tied_lines(seed):
    """... and against the reference's OWN group_output on the same grids (round 6, by hand: 300 of 300; with a stable sort and
    glibc's acos in the product it was 151 of 300)."""
    p = pkg()
    blks, lines, im_w, im_h, mask = grid_page(seed)
    got = p.textblock.group_output(copy.deepcopy(blks), lines.copy(), im_w, im_h, mask)
    theirs = reference_group_output(f"group_output_tied_{seed}", blks, lines, im_w, im_h, mask)
    same_blocks(got, theirs)


def test_native_group_output_empty_inputs():
    p = pkg()
    none = (np.zeros((0, 4), np.int32), np.zeros((0,), np.int32), np.zeros((0,)))
    assert p.textblock.group_output(none, [], 640, 480, np.zeros((480, 640), np.uint8)) == []
    lines = np.array([[[10, 10], [100, 10], [100, 30], [10, 30]]], np.int32)
    got = p.textblock.group_output(none, lines, 640, 480, None)
    ref = R.group_output(none, lines, 640, 480, None)
    same_blocks(got, ref)
    # a wide page takes the two-page branch of the reading order (textblock.py:280-281)
    blks, lines, im_w, im_h, mask = random_page(3, im_w=1800, im_h=900)
    same_blocks(p.textblock.group_output(copy.deepcopy(blks), lines.copy(), im_w, im_h, mask),
                R.group_output(copy.deepcopy(blks), lines.copy(), im_w, im_h, mask))


@pytest.mark.parametrize("seed", range(0, 60, 3))
def test_native_group_output_equals_reference_code(seed):
    """The reference's OWN group_output (shapely stand-in = the oracle's polygon predicate)."""
    p = pkg()
    blks, lines, im_w, im_h, mask = random_page(seed)
    got = p.textblock.group_output(copy.deepcopy(blks), lines.copy(), im_w, im_h, mask)
    theirs = reference_group_output(f"group_output_{seed}", blks, lines, im_w, im_h, mask)
    same_blocks(got, theirs)
    for a, b in zip(got, theirs):
        assert type(a.font_size) is type(b.font_size)


def test_block_list_is_the_lazy_form_of_the_same_blocks():
    """`BlockList` (what `detect_stream`'s workers hand over): len / counts / columns come from the native records without
    building anything; iteration, indexing, comparison give the `TextBlock` objects `blocks_from_records` builds."""
    p = pkg()
    TBm = p.textblock
    for seed in (3, 7, 11):
        blks, lines, im_w, im_h, mask = random_page(seed)
        recs, lout, dout = TBm.group_output_native(blks[0], blks[1], lines, im_w, im_h, mask)
        eager = TBm.blocks_from_records(list(recs), lout, dout)
        arr = np.frombuffer((p._lib.CtdBlk * max(len(recs), 1))(*recs), dtype=TBm.BLK_DTYPE, count=len(recs)).copy()
        lazy = TBm.BlockList(arr, lout, dout)
        assert lazy._built is None and len(lazy) == len(eager) and bool(lazy) == bool(eager)
        assert lazy.n_lines == sum(len(b.lines) for b in eager) and lazy._built is None
        assert lazy.line_quads.shape == (len(lout), 4, 2)
        same_blocks(lazy, eager)
        assert lazy._built is not None and lazy[0] is lazy.to_list()[0] and len(lazy[:2]) == min(2, len(eager))
    empty = TBm.BlockList(np.empty((0,), TBm.BLK_DTYPE), np.empty((0, 8), np.int32), np.empty((0, 3)))
    assert len(empty) == 0 and not empty and list(empty) == [] and empty == [] and empty.n_lines == 0
