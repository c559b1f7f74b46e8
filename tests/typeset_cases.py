"""TEST INFRASTRUCTURE of tests/test_gpu_typeset_walk.py and tests/test_typeset_cases.py: glyph scenes AT the boundaries of the
group and chunk walk (csrc/glyph_walk.h) that `glyphs_kernel` (csrc/kernels_glyphs.hip) and `tilted_kernel`
(csrc/kernels_tilted.hip) share, and seeded random scenes for both typeset kernels.  The sizes below are `glyphs_kernel`'s;
`tilted` sends a case through the other kernel.

The kernel walks a tile's entries in chunks of `NC` = 256 staged records, finds the end of a layer's run inside a chunk with
one ballot a wave of 64 and an LDS atomicMin, carries a run over several chunks, maxes later chunks into the patch, resolves
the visible patch rows (`CW` = 88 bytes each) in batches of `BATCH` = 11 * 256 bytes, and rewrites its slot tables per group.
The cases put a run end at, one below and one above every wave and chunk boundary, make a chunk contribute nothing, land the
patch bytes on one batch, one batch plus a row and two batches, and stack every radius on the same pixels.

Every case is a function returning (pages, bitmaps, layers, places) in the form `glyph_ref.typeset` takes: pages a list of
(H, W, 3) u8 arrays, bitmaps the atlas (a list of (h, w) u8 arrays), layers `glyph_ref.glayer` dicts, places tuples
(layer, glyph, x, y).  Everything is deterministic and numpy only; what each docstring promises is asserted in
tests/test_typeset_cases.py."""
import functools

import numpy as np

import glyph_ref as GR
import typeset_ref as TR

TW, TH, RMAX = 64, 32, 12                                   # the tile and the largest radius (include/ctd_hip.h)
NC, WAVE, CW, BATCH = 256, 64, TW + 2 * RMAX, 11 * 256      # glyph_walk.h: NC, the wave, typeset_tile.h: CW, kernels_glyphs.hip: PB * TS_THREADS

RUN_N = (63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 511, 512, 513)
RUN_R = (0, 12)
LAST_N = (256, 512)
BATCH_ROWS = ((0, 32), (1, 30), (1, 31), (12, 8), (12, 9), (12, 32))    # (r, rows): rows + 2 r = 32, 32, 33, 32, 33, 56
LADDER = (12, 1, 0, 7, 11, 2, 10, 3, 9, 4, 8, 5, 6)
FORCED = (31, 32, 33, 63, 64, 65, 127, 128, 129)            # page sides around the tile seams, forced into the sweep
N_SEEDS = 72                                                # the sweep: see DESIGN.md section 4.23 for how it was chosen


def _page(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def small_glyphs(seed=0):
    """Sixteen glyphs, every size of 3 x 3 .. 6 x 6 once, noise with no zero byte (`| 1`): every covered byte counts."""
    return [TR.noise(3 + i // 4, 3 + i % 4, 1000 * seed + i) | 1 for i in range(16)]


def _scatter(rng, n, layer, x1, y1, x2, y2):
    """n placements of `small_glyphs` ids with the top-left pixel in [x1, x2] x [y1, y2]."""
    return [(layer, int(rng.integers(0, 16)), int(rng.integers(x1, x2 + 1)), int(rng.integers(y1, y2 + 1))) for _ in range(n)]


def run_then_other(n, r):
    """One tile.  Layer 0 is a run of `n` placements at radius `r`, every one inside the page, so the tile has exactly n entries
    of it; layer 1 follows with three placements of another colour and radius 3 in the middle of the tile, on pixels that
    layer 0 wrote.  The first entry of layer 1 is entry n of the tile: lane n % 64 of wave (n % 256) / 64 of chunk n / 256.  A run
    end found too late draws layer 1's glyphs in layer 0's colours and leaves its row at 0; one found too early applies layer 0
    twice, the second outline over the first fill."""
    rng = np.random.default_rng(100 * n + r)
    layers = [GR.glayer(0, r, (200, 30, 10), (0, 60, 250)), GR.glayer(0, 3, (20, 250, 40), (255, 255, 0))]
    places = _scatter(rng, n, 0, 0, 0, TW - 6, TH - 6) + [(1, 15, 22, 9), (1, 10, 27, 13), (1, 5, 32, 11)]
    return [_page(TH, TW, n + r)], small_glyphs(), layers, places


def run_is_last(n, r):
    """`run_then_other` without layer 1, n = 256 or 512: the run ends the tile's entries exactly at a chunk's end, so the walk
    must stop without a continuation chunk."""
    pages, bitmaps, layers, places = run_then_other(n, r)
    return pages, bitmaps, layers[:1], places[:n]


def cross_chunk_max():
    """One tile, one layer of 300 placements at r = 3: two chunks.  Placement 0 (first chunk) and placement 280 (second chunk)
    are two different 6 x 6 glyphs at the same place (50, 20), where no other placement reaches: in some of their bytes the
    earlier value is the larger, in others the later, so the second chunk must take max(new, patch) and neither alone.  The other
    placements lie left of x = 48; some bytes there are covered by first-chunk glyphs only and lie inside the box of the second
    chunk, which must keep them."""
    rng = np.random.default_rng(7)
    bitmaps = small_glyphs() + [TR.noise(6, 6, 71) | 1, TR.noise(6, 6, 72) | 1]
    places = _scatter(rng, 300, 0, 0, 0, 42, TH - 6)
    places[0], places[280] = (0, 16, 50, 20), (0, 17, 50, 20)
    return [_page(TH, TW, 8)], bitmaps, [GR.glayer(0, 3, (250, 10, 120), (10, 240, 30))], places


def idle_chunk(first):
    """Two tiles side by side (32 x 128), one layer of 300 placements at r = 12, for a RAW table that lists every placement in
    every tile.  first=True: placements 0 .. 255 lie in tile 1 at x >= 77, more than r from tile 0, and 256 .. 299 in tile 0 at
    x <= 45, more than r from tile 1: tile 0's FIRST chunk stages nothing that contributes (and must still zero the patch and
    carry the run on), tile 1's last chunk likewise.  first=False: mirrored, tile 0's LAST chunk is the idle one."""
    rng = np.random.default_rng(11 + first)
    far, near = _scatter(rng, NC, 0, 77, 0, 2 * TW - 6, TH - 6), _scatter(rng, 300 - NC, 0, 0, 0, 45, TH - 6)
    if not first:
        far, near = _scatter(rng, NC, 0, 0, 0, 45, TH - 6), _scatter(rng, 300 - NC, 0, 77, 0, 2 * TW - 6, TH - 6)
    return [_page(TH, 2 * TW, 12)], small_glyphs(), [GR.glayer(0, 12, (5, 200, 250), (250, 40, 5))], far + near


def long_run_over_seams(r=12):
    """A 64 x 128 page, four tiles.  One layer of 300 glyphs strung along the seams x = 63/64 (150 of them, y = 15 .. 46) and
    y = 31/32 (150, x = 47 .. 78), so close to the corner that EVERY tile holds more than 256 of them: a multi-chunk group in
    each tile, across both seams, at r = 12.  The clip (49, 17, 84, 49) cuts through the glyphs at the ends of both strings."""
    rng = np.random.default_rng(13)
    places = []
    for k in range(150):
        places.append((0, int(rng.integers(0, 16)), 58 + k % 7, 15 + k % 32))
        places.append((0, int(rng.integers(0, 16)), 47 + k % 32, 26 + k % 7))
    return [_page(2 * TH, 2 * TW, 14)], small_glyphs(), [GR.glayer(0, r, (240, 240, 10), (10, 10, 120), clip=(49, 17, 84, 49))], places


def batch_rows(r, rows):
    """One tile, one layer at radius `r` whose clip is `rows` high and as wide as the tile, 200 glyphs all over the tile.  The
    kernel gathers (rows + 2 r) * 88 patch bytes in batches of 2816: the pairs of `BATCH_ROWS` make that exactly one batch
    (32 rows, three ways), one batch plus one row (33, two ways) and the whole patch of 56 rows, 4928 bytes."""
    rng = np.random.default_rng(10 * r + rows)
    y1 = (TH - rows) // 2
    layers = [GR.glayer(0, r, (10, 20, 230), (240, 230, 20), clip=(0, y1, TW, y1 + rows))]
    return [_page(TH, TW, 15)], small_glyphs(), layers, _scatter(rng, 200, 0, -3, -3, TW - 2, TH - 2)


def radius_ladder():
    """One tile, 13 layers on the same pixels with the radii 12, 1, 0, 7, 11, 2, 10, 3, 9, 4, 8, 5, 6 in that order, distinct
    colours, each layer 2 .. 4 overlapping glyphs: the slot tables and the planes (which also hold the staged records) are
    rewritten by every group, and a table left over from the group before gives another outline."""
    rng = np.random.default_rng(17)
    layers, places = [], []
    for li, r in enumerate(LADDER):
        layers.append(GR.glayer(0, r, (19 * li + 3, 250 - 17 * li, (97 * li) % 256), (255 - 19 * li, 11 * li + 5, (53 * li + 128) % 256)))
        places += _scatter(rng, 2 + li % 3, li, 28, 12, 29, 13)
    return [_page(TH, TW, 18)], small_glyphs(), layers, places


# ---- the sweep ---------------------------------------------------------------------------------------------------------------

_VALUES = np.array([0, 1, 127, 254, 255], np.uint8)


def _scene_glyph(rng, k):
    if k < 4:
        h, w = ((0, 0), (1, 1), (40, 40), (0, 7))[k]
    else:
        h, w = int(rng.integers(1, 41)), int(rng.integers(1, 41))
    if k % 2:
        return _VALUES[rng.integers(0, 5, (h, w))]
    return rng.integers(0, 256, (h, w), dtype=np.uint8)


def scene(seed):
    """A random scene.  1 .. 3 pages with H and W drawn from 1 .. 200; page 0 of an even seed is FORCED[seed % 9] wide and
    page 0 of an odd seed FORCED[seed // 2 % 9] high, so 18 consecutive seeds hold every forced side both ways.  1 .. 12 layers,
    r uniform in 0 .. 12, colours with 0 and 255 forced into some; a layer's clip is none, inside the page, cut through its first
    glyph, empty, or reaching beyond the page; 0 .. 40 placements a layer from an atlas of 12 glyphs of 0 x 0, 1 x 1, 40 x 40,
    0 x 7 and random sizes up to 40 x 40, coverage noise or drawn from {0, 1, 127, 254, 255}; positions from -50 to side + 50.
    Layer 0 has no clip and its first placement puts a byte that is not 0 on a page pixel: every scene writes."""
    rng = np.random.default_rng(5000 + seed)
    shapes = [(int(rng.integers(1, 201)), int(rng.integers(1, 201))) for _ in range(int(rng.integers(1, 4)))]
    force = FORCED[seed % 9] if seed % 2 == 0 else FORCED[seed // 2 % 9]
    shapes[0] = (shapes[0][0], force) if seed % 2 == 0 else (force, shapes[0][1])
    pages = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in shapes]
    bitmaps = [_scene_glyph(rng, k) for k in range(12)]
    layers, places = [], []
    for li in range(int(rng.integers(1, 13))):
        pg = 0 if li == 0 else int(rng.integers(0, len(shapes)))
        H, W = shapes[pg]
        run = [(li, int(rng.integers(0, 12)), int(rng.integers(-50, W + 51)), int(rng.integers(-50, H + 51)))
               for _ in range(int(rng.integers(0, 41)))]
        if li == 0:
            run.insert(0, (0, 4, int(rng.integers(0, W)), int(rng.integers(0, H))))
            bitmaps[4][0, 0] |= 1
        kind = 0 if li == 0 else int(rng.integers(0, 5))
        clip = None
        if kind == 1:
            cx, cy = sorted(rng.integers(0, W + 1, 2)), sorted(rng.integers(0, H + 1, 2))
            clip = (int(cx[0]), int(cy[0]), int(cx[1]), int(cy[1]))
        elif kind == 2 and run:
            _, g, x, y = run[0]
            h, w = bitmaps[g].shape
            clip = (x + w // 2, y + h // 2, x + w // 2 + int(rng.integers(1, 60)), y + h // 2 + int(rng.integers(1, 60)))
        elif kind == 3:
            cx = int(rng.integers(0, W + 1))
            clip = (cx, 0, cx, H)
        elif kind == 4:
            clip = (-int(rng.integers(1, 60)), -int(rng.integers(1, 60)), W + int(rng.integers(1, 60)), H + int(rng.integers(1, 60)))
        fill, stroke = (tuple(int(v) for v in rng.integers(0, 256, 3)) for _ in range(2))
        if li % 4 == 1:
            fill, stroke = (0, fill[1], 255), (255, 0, stroke[2])
        layers.append(GR.glayer(pg, int(rng.integers(0, 13)), fill, stroke, clip))
        places += run
    return pages, bitmaps, layers, places


# ---- the cases by name, and their references -------------------------------------------------------------------------------------

API_CASES = ([(f"run_then_other-n{n}-r{r}", run_then_other, (n, r)) for n in RUN_N for r in RUN_R] +
             [(f"run_is_last-n{n}-r{r}", run_is_last, (n, r)) for n in LAST_N for r in RUN_R] +
             [("cross_chunk_max", cross_chunk_max, ()), ("long_run_over_seams-r12", long_run_over_seams, (12,))] +
             [(f"batch_rows-r{r}-rows{rows}", batch_rows, (r, rows)) for r, rows in BATCH_ROWS] +
             [("radius_ladder", radius_ladder, ())])
RAW_CASES = [("idle_chunk-first", idle_chunk, (True,)), ("idle_chunk-last", idle_chunk, (False,))]
SEED_CASES = [(f"scene-seed{s}", scene, (s,)) for s in range(N_SEEDS)]
CASES = {name: (fn, args) for name, fn, args in API_CASES + RAW_CASES + SEED_CASES}


@functools.lru_cache(None)
def case(name):
    """(pages, bitmaps, layers, places) of the case `name`, built once.  Nobody writes into it."""
    fn, args = CASES[name]
    return fn(*args)


@functools.lru_cache(None)
def reference(name):
    """`glyph_ref.typeset` on the case `name`, computed once: (pages, rows, composed bitmap layers)."""
    pages, bitmaps, layers, places = case(name)
    return GR.typeset(pages, layers, places, bitmaps)


def tilted(name):
    """The case `name` as a call that `tilted_kernel` (csrc/kernels_tilted.hip) serves: (layers, angle, pivot), its layers at
    angle 0 -- (c, s) = (65536, 0), where the rule gives `ctd_typeset_glyphs`' bytes -- and one more layer on page 0, turned by
    5 degrees and without a placement.  That layer is EMPTY and draws nothing, but a call with any non-zero angle goes to
    `ctd_typeset_tilted` as a whole.  `reference(name)` is the answer for the case's own layers."""
    layers = case(name)[2]
    return layers + [GR.glayer(0, 3)], [0] * len(layers) + [5], [(9, 9)] * (len(layers) + 1)


def sizes_of(bitmaps, places):
    return [bitmaps[q[1]].shape for q in places]


def statuses(name):
    pages, bitmaps, layers, places = case(name)
    shapes = [pg.shape[:2] for pg in pages]
    return [GR.status_of(li, layers, places, sizes_of(bitmaps, places), shapes) for li in range(len(layers))]
