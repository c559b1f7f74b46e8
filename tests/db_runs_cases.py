"""TEST INFRASTRUCTURE of tests/test_db_runs_cases.py and tests/test_gpu_db_runs.py: maps for the segment skip of
`dbc_accum_kernel` (csrc/kernels_tail.hip).  The label pass of `launch_ccl_dual` leaves one flag per 64 consecutive linear
pixels of a page, "some label here is not -1"; `dbc_accum_kernel` skips a segment whose flag is clear unless background
component -1 is a hole.  What can go wrong: a segment skipped that had something to add (a flag wrongly clear, a flag of
another page or another segment, -1 taken for plain background where it is a hole), or a row / page whose segments do not line
up with the sweep's.  So the maps put

  * label -1 as the outer background (skip on), as a HOLE (a foreground frame around the page, nested rings, a bar along the
    top edge with a slot in it: skip off, and the hole's sum is nearly the whole page), and nowhere (all foreground);
  * components, holes and ring pixels at segment ends: W = 160, 131, 65 and 70 are no multiples of 64, so segments straddle
    rows; 257 x 131 and 33 x 65 pages end in a partial segment;
  * pages of different kinds in ONE call, so that a flag or a `par_b` row read from the neighbouring page shows;
  * pages with holes next to pages without any (`hole_rows` = 0: the kernel then leaves out the ring test and the `par_b`
    gathers as well), with and without ink.

No GPU is needed to build a map or its reference."""
import functools

import numpy as np

LO, HI = 0.05, 0.9


def _blocks(prob, rng, n, size):
    """`n` rectangles of text-like ink, every other one with a hole, every fourth with an island in the hole."""
    H, W = prob.shape
    for k in range(n):
        h, w = rng.randint(size // 2, size), rng.randint(size, 3 * size)
        y, x = rng.randint(1, max(2, H - h - 1)), rng.randint(1, max(2, W - w - 1))
        prob[y: y + h, x: x + w] = rng.uniform(0.5, 0.95)
        if k % 2 == 0 and h > 6 and w > 6:
            prob[y + 2: y + h - 2, x + 2: x + w - 2] = rng.uniform(0.05, 0.25)
            if k % 4 == 0 and h > 10 and w > 10:
                prob[y + 4: y + h - 4, x + 4: x + w - 4] = rng.uniform(0.5, 0.95)


def text_map(H, W, seed, n=6, size=12):
    prob = np.full((H, W), LO, np.float32)
    _blocks(prob, np.random.RandomState(seed), n, size)
    return prob


def solid_map(H, W, seed, n=8, size=12):
    """Text-like ink without a single hole (the usual text-line map): the page has no ring and no hole sum."""
    from scipy import ndimage
    prob = text_map(H, W, seed, n, size)
    ink = ndimage.binary_fill_holes(prob > 0.3)
    prob[ink & ~(prob > 0.3)] = 0.6
    return prob


def frame_map(H, W, seed, t=2):
    """A foreground frame `t` thick around a text-like page: background -1 is a hole and holds most of the page."""
    prob = text_map(H, W, seed)
    prob[:t], prob[-t:], prob[:, :t], prob[:, -t:] = HI, HI, HI, HI
    prob[t: t + 1, t:-t] = LO                                      # (the blocks never close the ring off)
    return prob


def rings_map(H, W):
    """Nested rings from the page frame inwards, two pixels each: holes inside holes, the outermost one is -1."""
    prob = np.full((H, W), LO, np.float32)
    for k in range(0, min(H, W) // 2 - 1, 4):
        prob[k: H - k, k: W - k] = HI
        prob[k + 2: H - k - 2, k + 2: W - k - 2] = LO
    return prob


def top_bar_map(H, W, seed):
    """A bar along the whole top edge with a slot in it: the slot is background -1 and a hole, the page below is -2."""
    prob = text_map(H, W, seed)
    prob[:7] = HI
    prob[2:5, 10: W - 10] = 0.2
    prob[7:9] = LO
    return prob


def late_background_map(H, W, seed):
    """The first rows are foreground to the last column but one: background -1 starts deep in the first segments."""
    prob = text_map(H, W, seed)
    prob[:2, : W - 1] = HI
    prob[2:4] = LO
    return prob


def noise_map(H, W, seed):
    from scipy import ndimage
    rng = np.random.RandomState(seed)
    pr = ndimage.uniform_filter(rng.rand(H, W), 2).astype(np.float32)
    span = float(pr.max() - pr.min())
    return ((pr - pr.min()) / span * 0.62 if span > 0 else np.full((H, W), HI)).astype(np.float32)


def big_map():
    """One 1024 x 1024 text-like page: 4 096 blocks of the accumulation's sweep, about 3 % ink."""
    prob = np.full((1024, 1024), LO, np.float32)
    _blocks(prob, np.random.RandomState(11), 60, 20)
    return prob


# maps whose background -1 is a hole (the skip must be off), and those where it is the outer background
HOLE_FIRST = ("frame", "rings", "top bar", "frame 257 x 131", "frame 33 x 65")


@functools.lru_cache(None)
def calls():
    """[(call name, tuning keys, [(map name, prob (H,W) f32)])]: the maps of one call share a shape."""
    H, W = 96, 160
    mixed = [("text", text_map(H, W, 1)), ("empty", np.full((H, W), LO, np.float32)), ("frame", frame_map(H, W, 2)),
             ("full", np.full((H, W), HI, np.float32)), ("rings", rings_map(H, W)), ("top bar", top_bar_map(H, W, 3))]
    odd = [("text 257 x 131", text_map(257, 131, 4, n=10)), ("frame 257 x 131", frame_map(257, 131, 5)),
           ("late background 257 x 131", late_background_map(257, 131, 6)), ("noise 257 x 131", noise_map(257, 131, 7)),
           ("solid 257 x 131", solid_map(257, 131, 10))]
    small = [("text 33 x 65", text_map(33, 65, 8, n=3, size=6)), ("frame 33 x 65", frame_map(33, 65, 9, t=1)),
             ("empty 33 x 65", np.full((33, 65), LO, np.float32))]
    out = [("96 x 160, six kinds of page in one call", {}, mixed),
           # 16 blocks for six pages: two per page, so every block walks 30 steps of the sweep in batches of four
           ("the same call under tail_max_blocks = 16", {"tail_max_blocks": 16}, mixed),
           ("257 x 131: rows straddle segments, the page ends in a partial one", {}, odd),
           ("33 x 65", {}, small)]
    for h, w in ((1, 70), (70, 1), (64, 64)):
        out.append((f"{h} x {w}", {}, [(f"noise {h} x {w}", noise_map(h, w, 20 + h)), (f"empty {h} x {w}", np.full((h, w), LO, np.float32)),
                                       (f"full {h} x {w}", np.full((h, w), HI, np.float32))]))
    return out


def segment_flags(t):
    """What the label pass writes for a page of `dbc_emul.dbc_tables`: per 64 linear pixels, "some label is not -1"."""
    other = (t["lab_b"].ravel() != 1)
    pad = (-other.size) % 64
    return np.r_[other, np.zeros(pad, bool)].reshape(-1, 64).any(axis=1)
