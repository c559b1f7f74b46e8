"""The seeded, GPU-free case generators of the parity sweeps: tests/test_gpu_sweeps.py runs a fixed range of each inside
`pytest -m gpu`, the scripts/gpu_*_stress.py run thousands by hand, tests/test_sweep_cases.py checks without a GPU (from the
oracle alone) that the ranges are not vacuous.  Every generator takes `(case, rng)` -- `rng` a `np.random.RandomState` that the
caller carries from case to case, so one seed fixes a whole sweep -- or a seed, and returns numpy inputs plus a short description
for failure messages.  Nothing here touches a GPU or the product's library."""
import numpy as np
from scipy import ndimage

# ------------------------------------------------------------------------------------------------------------------ NMS

NMS_CONF, NMS_IOU, NMS_MAX_DET = 0.4, 0.35, 300          # what the detector runs (inference.py:150)


def nms_case(case, rng, pages=None, rows=None):
    """A fake Detect tensor (B,rows,no) f32: row counts 50 .. 70 000, candidate fractions 0 .. 1 (scores above / below 0.4), box
    sizes from dense overlap to sparse, `no` in 6 / 7 / 8, every 5th case with an eighth of the rows duplicated (equal scores:
    the lower row wins), every 7th with scores on a 1/20 grid.  `pages` / `rows` force B and the row count (drawn otherwise)."""
    B = int(rng.randint(1, 4))
    r = int(rng.choice([50, 300, 1008, 4032, 16128, 64512, int(rng.randint(50, 70000))]))
    B, r = (B if pages is None else int(pages)), (r if rows is None else int(rows))
    frac = float(rng.choice([0.0, 0.01, 0.05, 0.3, 1.0, rng.uniform(0, 1)]))
    no = int(rng.choice([6, 7, 8]))
    size = int(rng.choice([256, 1024, 2048]))
    b = np.zeros((B, r, no), np.float32)
    b[..., 0:2] = rng.uniform(0, size, (B, r, 2))
    b[..., 2:4] = rng.uniform(2, rng.choice([20, 300, 900]), (B, r, 2))
    b[..., 4] = np.where(rng.uniform(size=(B, r)) < frac, rng.uniform(0.4, 1.0, (B, r)), rng.uniform(0, 0.4, (B, r)))
    b[..., 5:] = rng.uniform(0, 1, (B, r, no - 5))
    if case % 5 == 0 and r >= 64:                        # exact duplicates with equal scores: tie-break = lower row first
        k = r // 8
        b[:, k: 2 * k] = b[:, :k]
    if case % 7 == 0:                                    # scores on a coarse grid: many equal confidences
        b[..., 4] = np.round(b[..., 4] * 20) / 20
    return b, f"nms case {case}: pages {B} rows {r} frac {frac:.3f} no {no} size {size}"


def nms_thresholds(case, rng):
    """(conf_thres, iou_thres, max_det) of sweep case `case`: the detector's own, except every 4th case."""
    if case % 4 != 3:
        return NMS_CONF, NMS_IOU, NMS_MAX_DET
    return float(rng.choice([0.05, 0.25, 0.4, 0.7])), float(rng.choice([0.1, 0.35, 0.6, 0.9])), int(rng.choice([1, 50, 300]))


NMS_SWEEP_SEED = 1
NMS_SWEEP_B32 = {41: 1008, 83: 4032}                     # case -> rows of the two calls on 32 pages


def nms_sweep(n=100, seed=NMS_SWEEP_SEED):
    """The cases of `test_nms_sweep`: (case, blks, (conf, iou, max_det), description).  Tensors and thresholds come from two
    streams, so the tensors are those of `scripts/gpu_nms_stress.py` with the same seed up to the first 32-page case."""
    rng, trng = np.random.RandomState(seed), np.random.RandomState(seed + 1000)
    for case in range(n):
        b, what = nms_case(case, rng, *((32, NMS_SWEEP_B32[case]) if case in NMS_SWEEP_B32 else ()))
        thr = nms_thresholds(case, trng)
        yield case, b, thr, f"{what} conf {thr[0]} iou {thr[1]} max_det {thr[2]}"


# ------------------------------------------------------------------------------------------------------------- DB stage

DB_KINDS = ("smoothed noise", "rotated bars", "blobs with holes and islands", "gradient times noise")


def db_map(case, rng, shape=None):
    """A probability map (H,W) f32 that is NOT text-like, kind = case % 4 (`DB_KINDS`); `shape` forces (H, W)."""
    H, W = int(rng.randint(24, 300)), int(rng.randint(24, 400))
    if shape is not None:
        H, W = shape
    kind = case % 4
    if kind == 0:                                        # smoothed noise
        pr = ndimage.uniform_filter(rng.rand(H, W), int(rng.randint(1, 9)))
        pr = (pr - pr.min()) / max(pr.max() - pr.min(), 1e-9) * rng.uniform(0.4, 0.9)
    elif kind == 1:                                      # rotated bars
        pr = np.full((H, W), 0.05)
        yy, xx = np.mgrid[0:H, 0:W]
        for _ in range(rng.randint(1, 8)):
            ang = rng.uniform(0, np.pi)
            cx, cy, L, T = rng.uniform(0, W), rng.uniform(0, H), rng.uniform(5, 120), rng.uniform(1, 14)
            u = (xx - cx) * np.cos(ang) + (yy - cy) * np.sin(ang)
            v = -(xx - cx) * np.sin(ang) + (yy - cy) * np.cos(ang)
            pr[(np.abs(u) < L) & (np.abs(v) < T)] = rng.uniform(0.35, 0.99)
    elif kind == 2:                                      # blobs with holes and islands
        pr = np.full((H, W), 0.1)
        for _ in range(rng.randint(1, 6)):
            y, x, h, w = rng.randint(0, H), rng.randint(0, W), rng.randint(4, 80), rng.randint(4, 120)
            pr[y: y + h, x: x + w] = rng.uniform(0.5, 0.95)
            if h > 8 and w > 8:
                pr[y + 2: y + h - 2, x + 2: x + w - 2] = 0.1
                if h > 14 and w > 14:
                    pr[y + 5: y + h - 5, x + 5: x + w - 5] = rng.uniform(0.5, 0.95)
    else:                                                # gradient times noise
        pr = np.linspace(0, 1, W)[None, :] * np.linspace(0.2, 1, H)[:, None] * (0.6 + 0.4 * rng.rand(H, W))
    return pr.astype(np.float32), f"db case {case} kind {kind} ({DB_KINDS[kind]}) {H}x{W}"


DB_SWEEP_SEED = 1
DB_SWEEP_BATCH = 8
DB_SWEEP_BATCHED = 24        # the last 24 maps (the issue asks for 20; whole batches of 8) go three calls of 8 equal-size maps


def db_sweep(n=200, seed=DB_SWEEP_SEED):
    """The calls of `test_db_stage_sweep`: lists of (case, map, description), one map per call for the first n - 24 cases (the
    stream of `scripts/gpu_db_stress.py` with the same seed), then batches of 8 maps of one size drawn per batch."""
    rng = np.random.RandomState(seed)
    single = n - DB_SWEEP_BATCHED
    for case in range(single):
        yield [(case,) + db_map(case, rng)]
    for first in range(single, n, DB_SWEEP_BATCH):
        shape = (int(rng.randint(24, 300)), int(rng.randint(24, 400)))
        yield [(case,) + db_map(case, rng, shape) for case in range(first, first + DB_SWEEP_BATCH)]


# ------------------------------------------------------------------------------------------------------------- labelling

CCL_KINDS = ("noise", "diagonal chains", "tile-aligned blocks", "smooth blobs")
CCL_FORCED = [(1, 1), (1, 2), (2, 1), (1, 33), (33, 1), (1, 300), (300, 1), (31, 31), (32, 32), (33, 33), (31, 33), (33, 32)]


def ccl_image(case, rng, shape=None):
    """A boolean image, 1 .. 299 pixels a side, kind = case % 4 (`CCL_KINDS`): where the run-pruned border links are delicate
    (tile corners, thin diagonal chains, dense noise); `shape` forces (h, w)."""
    h, w = int(rng.randint(1, 300)), int(rng.randint(1, 300))
    if shape is not None:
        h, w = shape
    kind = case % 4
    if kind == 0:
        img = rng.uniform(size=(h, w)) < rng.uniform(0.02, 0.98)
    elif kind == 1:                                   # diagonal / anti-diagonal chains crossing tile corners
        yy, xx = np.mgrid[0:h, 0:w]
        img = ((yy + xx) % int(rng.randint(2, 7)) == 0) | ((yy - xx) % int(rng.randint(2, 9)) == 0)
        img &= rng.uniform(size=(h, w)) < 0.9
    elif kind == 2:                                   # blocks aligned to the 32-pixel tiles with random gaps
        img = np.ones((h, w), bool)
        img[::32] = rng.uniform(size=img[::32].shape) < 0.5
        img[:, ::32] = rng.uniform(size=img[:, ::32].shape) < 0.5
        img[31::32] = rng.uniform(size=img[31::32].shape) < 0.5
        img[:, 31::32] = rng.uniform(size=img[:, 31::32].shape) < 0.5
    else:                                             # smooth blobs
        img = ndimage.gaussian_filter(rng.uniform(size=(h, w)), rng.uniform(0.5, 3)) > 0.5
    return img, f"ccl case {case} kind {kind} ({CCL_KINDS[kind]}) {h}x{w}"


def ccl_sweep(n=100, seed=0):
    """The images of `test_ccl_sweep`: the shapes of `CCL_FORCED` in the first 12 cases, drawn shapes after."""
    rng = np.random.RandomState(seed)
    for case in range(n):
        yield (case,) + ccl_image(case, rng, CCL_FORCED[case] if case < len(CCL_FORCED) else None)


# ---------------------------------------------------------------------------------------------------------------- resize

# (source h, w), (destination h, w): 1 x 1 source, 1-pixel destinations, equal size, more than 16x up and down
RESIZE_FORCED = [((1, 1), (37, 53)), ((1, 1), (1, 1)), ((211, 97), (1, 1)), ((64, 300), (1, 450)), ((300, 64), (450, 1)),
                 ((123, 231), (123, 231)), ((17, 23), (17 * 17, 23 * 19)), ((40, 3), (41, 900)), ((680, 697), (40, 41)),
                 ((699, 1), (3, 5))]


def resize_case(case, rng, shapes=None):
    """(image u8 (sh,sw) or (sh,sw,3), (dh,dw), canvas (ch,cw) or None, description): source 1 .. 699 a side, destination
    1 .. 899, odd cases 3 channels, every 3rd case inside a larger zero canvas (the letterbox); `shapes` forces both shapes."""
    sh, sw = int(rng.randint(1, 700)), int(rng.randint(1, 700))
    dh, dw = int(rng.randint(1, 900)), int(rng.randint(1, 900))
    if shapes is not None:
        (sh, sw), (dh, dw) = shapes
    ch = 3 if case % 2 else 1
    img = rng.randint(0, 256, (sh, sw, 3) if ch == 3 else (sh, sw)).astype(np.uint8)
    canvas = (dh + int(rng.randint(0, 40)), dw + int(rng.randint(0, 40))) if case % 3 == 2 else None
    return img, (dh, dw), canvas, f"resize case {case}: {sh}x{sw}x{ch} -> {dh}x{dw} canvas {canvas}"


def resize_sweep(n=150, seed=1):
    rng = np.random.RandomState(seed)
    for case in range(n):
        yield (case,) + resize_case(case, rng, RESIZE_FORCED[case] if case < len(RESIZE_FORCED) else None)


def mixed_size_batches(n=6, seed=1):
    """The batches of `test_mixed_size_batch_equals_single_calls`: (case, pages, refine_mode, keep_undetected_mask), 2 .. 6
    text-like pages of 160 .. 699 pixels a side each."""
    from conftest import pkg
    rng = np.random.RandomState(seed)
    for case in range(n):
        k = int(rng.randint(2, 7))
        pages = [pkg().synth.text_like_page((int(rng.randint(160, 700)), int(rng.randint(160, 700))), 500 + 10 * case + i,
                                            n_blocks=int(rng.randint(2, 7))) for i in range(k)]
        yield case, pages, int(rng.randint(0, 2)), bool(rng.randint(0, 2))


# ------------------------------------------------------------------------------------------------------------ whole tail

def blks_tensor(blks, rows=4096):
    """(blines, cls, confs) -> a fake Detect tensor (1,rows,7) whose NMS gives those blocks back."""
    blines, cls, confs = blks
    t = np.zeros((1, rows, 7), np.float32)
    for i, (bb, c, s) in enumerate(zip(blines, cls, confs)):
        x1, y1, x2, y2 = bb
        t[0, i] = [(x1 + x2) / 2, (y1 + y2) / 2, x2 - x1, y2 - y1, 0.99, 0.0, 0.0]
        t[0, i, 5 + c] = s / 0.99
    return t


def tail_case(seed, size, rows=4096):
    """Text-like network outputs of one size x size page (tests/test_post_host.py `fake_outputs`) as the native tail and
    `R.detector_tail` take them: (page, blks (1,rows,7), mask_u8, prob, mask f32 (1,1,H,W), lines_map (1,2,H,W), description)."""
    from test_post_host import fake_outputs
    page, mask_u8, prob, blks = fake_outputs(seed, size)
    mask_f = (mask_u8.astype(np.float32) + 0.5) / 255            # postprocess_mask truncates back to mask_u8
    lines_map = np.stack([prob, np.zeros_like(prob)])[None]
    return page, blks_tensor(blks, rows), mask_u8, prob, mask_f[None, None], lines_map, f"tail seed {seed} at {size}"


def tail_batch32(call, seed0=7000, size=512):
    """The 32 pages of one native tail call of `test_tail_on_32_different_pages_per_call`: seeds seed0 + 32 * call + 0 .. 31,
    every Detect tensor padded to one row count."""
    from test_post_host import fake_outputs
    outs = [fake_outputs(seed0 + 32 * call + i, size) for i in range(32)]
    rows = max(max(len(o[3][0]) for o in outs) + 8, 64)
    cases = []
    for i, (page, mask_u8, prob, blks) in enumerate(outs):
        mask_f = (mask_u8.astype(np.float32) + 0.5) / 255
        cases.append((page, blks_tensor(blks, rows), mask_u8, prob, mask_f[None, None], np.stack([prob, np.zeros_like(prob)])[None],
                      f"call {call} page {i} (seed {seed0 + 32 * call + i}) at {size}"))
    return cases


LETTERBOX_SIZE = 512


def letterbox_tail_case(seed, size=LETTERBOX_SIZE):
    """A page of random size and aspect ratio (200 .. 1499 pixels a side) with network outputs consistent with its letterbox at
    `size` (tests/test_reference_pin.py `letterboxed_case`): (page, blks, mask f32 (1,1,H,W), lines_map, (dw, dh), description)."""
    import test_reference_pin as pin
    rng = np.random.RandomState(7000 + seed)
    im_hw = (int(rng.randint(200, 1500)), int(rng.randint(200, 1500)))
    page, bt, mask, lines_map, (dw, dh) = pin.letterboxed_case(seed, im_hw, size)
    return page, bt, mask, lines_map, (dw, dh), f"letterbox seed {seed} page {im_hw[0]}x{im_hw[1]} at {size}"


# ------------------------------------------------------------------------------------------ block lists up to tied lines

def equal_up_to_tied_lines(got, ref):
    """Same blocks, and every block's lines equal as a set and in order except among lines whose distances agree to 1e-6:
    `TextBlock.sort_lines` orders lines of one text row -- a mathematical tie -- by the last bit of `|sin(acos(c))| * len`,
    which numpy's SIMD libm and glibc compute differently now and then ("ties")."""
    if len(got) != len(ref):
        return False
    for a, b in zip(got, ref):
        if [int(v) for v in a.xyxy] != [int(v) for v in b.xyxy] or len(a.lines) != len(b.lines):
            return False
        key = lambda blk: sorted((round(float(d), 6), tuple(np.asarray(l).reshape(-1).tolist()))               # noqa: E731
                                 for d, l in zip(np.asarray(blk.distance).reshape(-1), blk.lines))
        if key(a) != key(b):
            return False
    return True


# ------------------------------------------------------------------------------------- histograms that tie (mask refinement)

TIED_KINDS = ("one value", "two or three values with equal counts", "equal peaks closer than color_var",
              "plateau of more than 16 equal counts", "empty", "only 0 and 255", "plateau over the whole range 0 .. 255")
_TIED_SCHEDULE = (3, 1, 2, 3, 0, 5, 6, 1, 2, 3, 4, 5)


def tied_pixels(case, rng):
    """uint8 pixels whose histogram ties where the colour pick (np.histogram(bins=255) + `get_topk_color`: an argsort of the
    counts) or Otsu's threshold decides.  The reference's histogram has 255 bins over [min, max]: as long as max - min < 255
    every value has a bin of its own, at a range of exactly 255 the values 254 and 255 share the last bin -- the kinds that
    reach 255 split that bin's count between the two values, so the tie holds in the 255 bins and not only in a 256-bin
    count.  Kinds (`TIED_KINDS`) follow a fixed schedule over `case`; the pixels are shuffled."""
    kind = _TIED_SCHEDULE[case % len(_TIED_SCHEDULE)]
    m = int(rng.randint(1, 60))
    if kind == 0:
        vals, cnts = [int(rng.randint(0, 256))], [m]
    elif kind == 1:
        k = int(rng.randint(2, 4))
        vals, cnts = sorted(rng.choice(255, k, replace=False).tolist()), [m] * k       # below 255: one bin per value
    elif kind == 2:
        a, d = int(rng.randint(0, 230)), int(rng.randint(1, 11))
        vals, cnts = [a, a + d], [m + 5, m + 5]
        if rng.rand() < 0.7:                                                           # a lower third peak, or two tied ones
            far = [v for v in (a - 30, a + d + 25) if 0 <= v < 255]
            vals, cnts = vals + far, cnts + [int(rng.randint(1, m + 5))] * len(far)
    elif kind == 3:
        w = int(rng.randint(17, 200))
        v0 = int(rng.randint(0, 255 - w))
        vals, cnts = list(range(v0, v0 + w)), [m] * w
        if rng.rand() < 0.5:                                                           # one bin above the plateau
            cnts[int(rng.randint(0, w))] += int(rng.randint(1, 4))
    elif kind == 4:
        vals, cnts = [], []
    elif kind == 5:
        vals, cnts = [0, 255], ([m, m] if case % 2 else [m, int(rng.randint(1, 60))])
    else:
        vals, cnts = list(range(256)), [2 * m] * 254 + [m, m]                          # 254 and 255 share the last bin
        if rng.rand() < 0.5:                                                           # a gap: bins of count 0 tie as well
            g = int(rng.randint(1, 200))
            for v in range(g, g + int(rng.randint(1, 40))):
                cnts[v] = 0
    px = np.repeat(np.asarray(vals, np.uint8), np.asarray(cnts, np.int64))
    rng.shuffle(px)
    return px, f"tied case {case} kind {kind} ({TIED_KINDS[kind]}): {len(px)} pixels, {len(vals)} values, count {m}"


def tied_sweep(n=200, seed=5):
    rng = np.random.RandomState(seed)
    for case in range(n):
        yield (case,) + tied_pixels(case, rng)
