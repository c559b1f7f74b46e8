"""TEST INFRASTRUCTURE of tests/test_gpu_tail_trace.py and tests/test_tail_trace_cases.py: the cases, references and compare
helpers for the tables the tail's kernels write and the host only draws decisions from (`Tail.set_trace`, include/ctd_hip.h
ABI v9):

  * mask refinement -- per window the four histograms of `tw_hist_kernel`, the rules `refine_rules` draws from them, the six
    xor sums of `tw_xor_kernel` and the candidates `refine_candidates` returns (csrc/kernels_tail.hip, csrc/host_refine.cpp).
    Reference: `host_replay.refine_window_expected` on the window's CROP, with numpy as it is.  The kernels read the PAGE, so
    every page here is adversarial outside its windows.
  * DB stage -- the tables of `dbc_prep / scan / init / accum_kernel` against `dbc_emul.dbc_tables`.

No GPU is needed to build a case or its reference."""
import functools

import numpy as np

import dbc_emul
from host_replay import refine_window_expected
from oracle import cv_ref as cv
from oracle import postproc_ref as R

U = 2.0 ** -53                      # unit roundoff of binary64


# ====================================================================================================== refine: windows

def padding(bw, bh):
    """`paddings` of R.expand_textwindow(expand_r=16) for arrays of block sizes (np.rint and round() both round half to even)."""
    bw, bh = np.asarray(bw, np.float64), np.asarray(bh, np.float64)
    return np.rint((np.maximum(bh, bw) * 0.25 + np.minimum(bh, bw) * 0.75) / 16).astype(np.int64)


def _axis_options(lo, size, limit, pad):
    """Blocks [b1, b2] of one axis whose expansion by `pad`, clamped to [0, limit - 1], is [lo, lo + size]: a clamped end is
    free (the block may reach beyond the page, as a detection's box may)."""
    hi = lo + size
    b1s = [lo + pad] if lo > 0 else list(range(pad, pad - 40, -1))
    b2s = [hi - pad] if hi < limit - 1 else list(range(hi - pad, hi - pad + 40))
    return [(b1, b2) for b1 in b1s for b2 in b2s if b2 >= b1]


def block_for_window(im_w, im_h, win):
    """A block box whose `R.expand_textwindow(.., expand_r=16)` is the window (x1, y1, w, h); a window that no padding
    produces in the open (31 x 1: a 31-wide block is padded by 1) has to touch a page edge, where the clamp cuts it."""
    x1, y1, w, h = win
    assert x1 >= 0 and y1 >= 0 and x1 + w <= im_w - 1 and y1 + h <= im_h - 1, win
    for pad in range(0, 48):
        xs, ys = _axis_options(x1, w, im_w, pad), _axis_options(y1, h, im_h, pad)
        if not xs or not ys:
            continue
        bw = np.array([b - a for a, b in xs])[:, None]
        bh = np.array([b - a for a, b in ys])[None, :]
        hit = np.argwhere(padding(bw, bh) == pad)
        if len(hit):
            (ax, bx), (ay, by) = xs[hit[0][0]], ys[hit[0][1]]
            box = [int(ax), int(ay), int(bx), int(by)]
            got = R.expand_textwindow((im_h, im_w), box, expand_r=16)
            assert got == [x1, y1, x1 + w, y1 + h], (win, box, got)
            return box
    raise AssertionError(f"no block gives window {win} on a {im_w} x {im_h} page")


def windows_of(shape, boxes):
    """(x1, y1, w, h) of the windows `refine_mask` cuts for `boxes`, in order (an empty crop is skipped, textmask.py:164)."""
    out = []
    for b in boxes:
        x1, y1, x2, y2 = R.expand_textwindow(shape, [int(v) for v in b], expand_r=16)
        if x2 > x1 and y2 > y1:
            out.append((x1, y1, x2 - x1, y2 - y1))
    return out


def open_height(w, at_least=8):
    """The smallest height >= `at_least` at which a window `w` wide exists away from the page edges (8 x 9 does not: an 8 x 9
    block is padded by 1, a 6 x 7 block by 0)."""
    for h in range(at_least, at_least + 16):
        for pad in range(0, 1 + min(w, h) // 2):
            if padding(w - 2 * pad, h - 2 * pad) == pad:
                return h
    raise AssertionError(f"no window {w} wide in the open")


WIDTHS = list(range(1, 18)) + [31, 32, 33, 63, 64, 65]
HEIGHTS = (1, 2, 3, 8)              # 8: `open_height(w, 8)`
IMAGE_KINDS = ("flat", "two-valued", "noisy", "grey")


def width_class_windows(im_w=203, im_h=232):
    """Every width of WIDTHS at every height of HEIGHTS, origins cycling through x1 mod 4.  Widths up to 17 in the open; the
    wide ones at heights 1 .. 3 stacked on the top / bottom edge (no block in the open pads to them)."""
    wins = []
    for r, h in enumerate(HEIGHTS):
        x = 2 + r
        for w in range(1, 18):
            wins.append((x, 6 + 14 * r, w, h if h < 8 else open_height(w, h)))
            x += w + 1 + (w + r) % 3              # gaps 1 .. 3: the origins take every residue of 4
    for h in (1, 2, 3):                           # top edge: y1 = 0; bottom edge: y2 = im_h - 1
        x = 1
        for w in (31, 32, 33, 63):
            wins.append((x, 0, w, h))
            x += w + 2
        x = 3
        for w in (64, 65):
            wins.append((x, im_h - 1 - h, w, h))
            x += w + 2
    x = 0                                         # touches the left edge
    for w in (31, 32, 33, 63):
        wins.append((x, 70, w, open_height(w, 9 + w % 3)))
        x += w + 2
    wins.append((2, 92, 64, open_height(64, 10)))
    wins.append((im_w - 1 - 65, 92, 65, 11))      # touches the right edge (x2 = im_w - 1: the reference's clamp)
    # the four corners, narrow and wide
    wins += [(0, 110, 5, 7), (im_w - 1 - 6, 110, 6, 9), (0, 0, 7, 4), (im_w - 1 - 9, 0, 9, 5), (0, im_h - 1 - 12, 3, 12),
             (im_w - 1 - 13, im_h - 1 - 8, 13, 8)]
    return wins


def page_for_windows(im_w, im_h, wins, kind, seed):
    """(image, mask) adversarial to the crop semantics: inside a window the mask is mostly high (or mostly low, alternating)
    with 127 / 128 mixed in, the ring just outside it is the opposite extreme, and the image outside every window is random
    colour whatever the kind inside.  An erosion that reads beyond the window, or counts it as 0, changes bins."""
    rng = np.random.RandomState(seed)
    if kind == "flat":
        img = np.broadcast_to(rng.randint(0, 256, 3), (im_h, im_w, 3)).astype(np.uint8).copy()
    elif kind == "two-valued":
        pick = rng.rand(im_h, im_w) < 0.4
        img = np.where(pick[..., None], rng.randint(0, 100, 3), rng.randint(150, 256, 3)).astype(np.uint8)
    elif kind == "noisy":
        img = rng.randint(0, 256, (im_h, im_w, 3)).astype(np.uint8)
    else:
        g = rng.randint(0, 256, (im_h, im_w)).astype(np.uint8)
        g = np.where(rng.rand(im_h, im_w) < 0.5, g, (g // 64) * 64).astype(np.uint8)
        img = np.repeat(g[..., None], 3, axis=2)
    covered = np.zeros((im_h, im_w), bool)
    for x1, y1, w, h in wins:
        covered[y1: y1 + h, x1: x1 + w] = True
    img[~covered] = rng.randint(0, 256, (int((~covered).sum()), 3))
    mask = (rng.rand(im_h, im_w) < 0.5).astype(np.uint8) * 255
    order = sorted(range(len(wins)), key=lambda i: -wins[i][2] * wins[i][3])
    for i in order:
        x1, y1, w, h = wins[i]
        high = i % 2 == 0
        levels = np.array([255, 128, 200, 128, 255, 127, 255, 128] if high else [0, 127, 60, 0, 128, 0, 255, 127], np.uint8)
        inside = levels[rng.randint(0, len(levels), (h, w))]
        ya, yb, xa, xb = max(y1 - 1, 0), min(y1 + h + 1, im_h), max(x1 - 1, 0), min(x1 + w + 1, im_w)
        ring = ~covered[ya:yb, xa:xb]
        mask[ya:yb, xa:xb][ring] = 0 if high else 255
        mask[y1: y1 + h, x1: x1 + w] = inside
    return np.ascontiguousarray(img), np.ascontiguousarray(mask)


def _case(name, pages, masks, boxes, keep=False, tune=None, mode=0):
    return dict(name=name, pages=pages, masks=masks, boxes=boxes, keep=keep, tune=dict(tune or {}), mode=mode)


def _big_page(seed, wins, im_w=251, im_h=256, kind="noisy"):
    img, mask = page_for_windows(im_w, im_h, wins, kind, seed)
    return img, mask, [block_for_window(im_w, im_h, w) for w in wins]


BIG2 = (20, 30, 96, 48)            # 4 608 pixels: two blocks of 4 096
BIG4 = (101, 120, 131, 97)         # 12 707 pixels, w mod 4 = 3: four blocks, 3 201 groups = four trips of 1 024 per block row
MIXED = [BIG2, BIG4, (7, 5, 1, 1), (13, 9, 3, 2), (60, 50, 96, 48), (101, 120, 131, 97), (130, 10, 40, 30), (150, 25, 33, 20)]


@functools.lru_cache(None)
def width_class_case():
    """The four image kinds as four pages of one call (widths 203, 201, 202, 200)."""
    pages, masks, boxes = [], [], []
    for k, kind in enumerate(IMAGE_KINDS):
        im_w, im_h = (203, 201, 202, 200)[k], 232
        wins = width_class_windows(im_w, im_h)
        img, mask = page_for_windows(im_w, im_h, wins, kind, 40 + k)
        pages.append(img), masks.append(mask), boxes.append([block_for_window(im_w, im_h, w) for w in wins])
    return _case("width classes x image kinds", pages, masks, boxes)


@functools.lru_cache(None)
def refine_cases():
    """Every refine call of tests/test_gpu_tail_trace.py but the width-class page (run three times there)."""
    out = []
    img, mask, bx = _big_page(50, [BIG2], kind="two-valued")
    out.append(_case("96 x 48 alone: two blocks", [img], [mask], [bx]))
    img, mask, bx = _big_page(51, [BIG4])
    out.append(_case("131 x 97 alone: four blocks, grid-stride trips", [img], [mask], [bx], mode=1))
    img, mask, bx = _big_page(52, MIXED)
    out.append(_case("big, tiny, overlapping and repeated windows in one call", [img], [mask], [bx]))
    # the per-window grid is min(blocks the largest window asks for = 4, tail_max_blocks / windows): 16 / 8 = 2
    out.append(_case("the same call under tail_max_blocks = 16: two blocks per window", [img], [mask], [bx],
                     tune={"tail_max_blocks": 16}))
    pages, masks, boxes = [], [], []
    for k, (im_w, im_h) in enumerate(((203, 90), (64, 131), (131, 77))):
        wins = [(0, 0, 9, 6), (im_w - 1 - 11, 0, 11, 5), (0, im_h - 1 - 7, 6, 7), (im_w - 1 - 15, im_h - 1 - 9, 15, 9),
                (5, 12, im_w - 12, open_height(im_w - 12, 30)), (17 + k, 20, 14, open_height(14, 22)), (3, 50, 5, 3)]
        img, mask = page_for_windows(im_w, im_h, wins, IMAGE_KINDS[k], 60 + k)
        pages.append(img), masks.append(mask), boxes.append([block_for_window(im_w, im_h, w) for w in wins])
    out.append(_case("three pages of different widths", pages, masks, boxes, mode=1))
    # refine_undetected_mask: blobs of the mask that no block covers become windows of a second pass
    rng = np.random.RandomState(70)
    im_w, im_h = 203, 160
    wins = [(10, 10, 60, open_height(60, 40)), (100, 20, 33, open_height(33, 30))]
    img, mask = page_for_windows(im_w, im_h, wins, "noisy", 71)
    img[:, : im_w // 2] = (img[:, : im_w // 2] // 64) * 64
    mask[60:, :] = 0
    for x, y, w, h in ((20, 70, 50, 20), (120, 80, 41, 35), (5, 120, 23, 30), (150, 125, 51, 33), (90, 70, 9, 8)):
        mask[y: y + h, x: x + w] = rng.randint(100, 256)
        mask[y + 2: y + h - 2: 3, x + 1: x + w - 1: 4] = 20
    out.append(_case("keep_undetected_mask: a second pass", [img], [mask], [[block_for_window(im_w, im_h, w) for w in wins]],
                     keep=True))
    return out


def undetected_blocks(mask_pred, mask_refined, boxes):
    """The blocks `R.refine_undetected_mask` adds (textmask.py:135-153), from the oracle's own pieces; edits `mask_pred` in
    place as the reference does."""
    mask_pred[np.where(mask_refined > 30)] = 0
    n, labels, stats = R.connected_components_with_stats(cv.threshold_binary(mask_pred, 30, 255), 4)
    valid = np.where(stats[:, -1] > 50)[0]
    out = []
    for li in valid[1:]:
        x, y, w, h, area = (int(v) for v in stats[li])
        bbox = [x, y, x + w, y + h]
        score = max([R.union_area(b, bbox) for b in boxes] + [-1])
        if score / w / h < 0.5:
            out.append(bbox)
    return out


def window_reference(page, x1, y1, w, h, pass_, img, mask):
    hist4, rules, sums, npix, want = refine_window_expected(np.ascontiguousarray(img[y1: y1 + h, x1: x1 + w]),
                                                            np.ascontiguousarray(mask[y1: y1 + h, x1: x1 + w]), libm_side=False)
    n = int(want["rc"][0])
    return dict(page=page, x1=x1, y1=y1, w=w, h=h, pass_=pass_, hist=hist4.astype(np.uint32), rules=rules.reshape(6, 3).astype(np.int32),
                sums=sums.astype(np.uint64), n_cand=n, cand_rule=want["cand_rule"][:n].astype(np.int32),
                cand_invert=want["cand_invert"][:n].astype(np.int32), cand_dist=want["cand_dist"][:n].astype(np.uint64))


def refine_reference(case):
    """(window records in the order the native tail sees them -- pass 0 of every page, then pass 1 of every page --,
    refined masks, masks after the call) of one case, from the oracle alone."""
    recs, refined, after, second = [], [], [], []
    for b, (img, mask, boxes) in enumerate(zip(case["pages"], case["masks"], case["boxes"])):
        for x1, y1, w, h in windows_of(img.shape, boxes):
            recs.append(window_reference(b, x1, y1, w, h, 0, img, mask))
        blks = [R.TextBlock(list(bx)) for bx in boxes]
        ref = R.refine_mask(img, mask, blks, case["mode"])
        m = mask.copy()
        if case["keep"]:
            extra = undetected_blocks(m, ref, boxes)                        # (m edited in place: pass 1 reads the edited mask)
            for x1, y1, w, h in windows_of(img.shape, extra):
                second.append(window_reference(b, x1, y1, w, h, 1, img, m))
            m2 = mask.copy()
            ref = R.refine_undetected_mask(img, m2, ref, blks, case["mode"])
            assert np.array_equal(m, m2)
        refined.append(ref), after.append(m)
    return recs + second, refined, after


_WIN_FIELDS = ("page", "x1", "y1", "w", "h", "pass_", "n_cand")


def compare_window(got, ref):
    """One window record of `Tail.trace_windows()` against `window_reference`: every field exact; the message names the first
    differing field and element."""
    for k in _WIN_FIELDS:
        assert int(got[k]) == int(ref[k]), f"{k}: {int(got[k])} vs {int(ref[k])}"
    n = int(ref["n_cand"])
    for k, g, r in (("hist", got["hist"], ref["hist"]), ("rules", got["rules"], ref["rules"]), ("sums", got["sums"], ref["sums"]),
                    ("cand_rule", got["cand_rule"][:n], ref["cand_rule"]), ("cand_invert", got["cand_invert"][:n], ref["cand_invert"]),
                    ("cand_dist", got["cand_dist"][:n], ref["cand_dist"])):
        g, r = np.asarray(g), np.asarray(r)
        assert g.shape == r.shape, f"{k}: shape {g.shape} vs {r.shape}"
        bad = np.argwhere(g != r)
        assert not len(bad), f"{k}{tuple(int(v) for v in bad[0])}: {g[tuple(bad[0])]} vs {r[tuple(bad[0])]} ({len(bad)} differ)"
    unused = np.asarray(ref["rules"])[:, 0] < 0
    assert not np.asarray(got["sums"])[unused].any(), "the sum of an unused rule is not 0"


def as_record(ref, path=0):
    """A reference window as a record of `Tail.trace_windows()` (the CPU test perturbs these)."""
    from conftest import pkg
    rec = np.zeros((), pkg().tail.TRACE_WIN_DTYPE)
    for k in _WIN_FIELDS + ("hist", "rules", "sums"):
        rec[k] = ref[k]
    n = int(ref["n_cand"])
    for k in ("cand_rule", "cand_invert", "cand_dist"):
        rec[k][:n] = ref[k]
    rec["path"] = path
    return rec


def compare_paths(recs, paths):
    """The `path` fields of a call's records against `Tail.refine_paths()`."""
    p = np.asarray(recs["path"])
    mine = {"lds": int((p == 0).sum()), "canvas": int((p >= 1).sum()), "overflow": int((p == 2).sum())}
    assert mine == dict(paths) and ((p >= 0) & (p <= 2)).all(), f"paths {mine} vs {dict(paths)}"


def before_merge(recs):
    """What of the records does not depend on the merge stage's path."""
    return [recs[k].tobytes() for k in recs.dtype.names if k != "path"]


# ============================================================================= refine: the launch-shape keys of the merge stage
# `tail_lds_threads`, `tail_lds_cls0 / cls1`, `tail_lds_runs_x10` (csrc/tuning.def): cases whose windows have word counts
# chosen relative to the block sizes, and a plain restatement of how the host sizes and groups the launches of
# `tw_lds_kernel` (csrc/tail.hip `refine_windows`, csrc/kernels_twlds.hip `tw_lds_rcap / tw_lds_bytes / launch_tw_lds`).

BLOCK_SIZES = (256, 512, 1024)      # what `tail_lds_threads` clamps to
LDS_KEYS = ("tail_lds", "tail_lds_rcap", "tail_lds_max_bytes", "tail_lds_runs_x10", "tail_lds_threads", "tail_lds_cls0", "tail_lds_cls1")


@functools.lru_cache(None)
def key_defaults():
    """What the library holds for the keys of the merge stage's launches (csrc/tuning.def), read from the library."""
    from conftest import pkg
    L = pkg()._lib
    return {k: L.tuning_get(k) for k in LDS_KEYS}


def clamped_threads(value):
    """What `launch_tw_lds` makes of `tail_lds_threads`."""
    return 1024 if value >= 1024 else (512 if value >= 512 else 256)


def words_of(w, h):
    return ((w + 31) >> 5) * h


def lds_rcap(words, runs_x10, rcap_key=0):
    """Runs a labelling may have in a launch whose largest window has `words` plane words: `runs_x10` / 10 per word, at
    least 1 024, at most 65 000 (a u16 prefix); `rcap_key` > 0 (`tail_lds_rcap`) replaces the rule, still clamped."""
    return min(65000, rcap_key if rcap_key > 0 else max(1024, words * runs_x10 // 10))


def lds_need(words, runs_x10, rcap_key=0):
    """Bytes of dynamic LDS of a block laid out for `words` plane words: three planes, a u16 prefix per word (rounded up to
    whole u32), parent + acc of `rlay` = max(rcap, ceil(words / 2)) entries (they double as the scratch plane), 20 words
    of partials."""
    rlay = max(lds_rcap(words, runs_x10, rcap_key), (words + 1) // 2)
    return (3 * words + (words + 1) // 2 + 2 * rlay + 20) * 4


def lds_launches(words_list, cls0, cls1, lds_max, runs_x10, rcap_key=0, lds=1):
    """(indices of the windows that take the canvases up front, launches) for windows of `words_list` plane words: a window
    goes to LDS if its need is at most `lds_max`; those, in ascending order of words (stable), are cut into up to three
    launches -- need <= cls0, then need <= cls1, then the rest --, each laid out for its LARGEST window.  A launch is
    (windows, max_words, rcap, bytes, [window indices])."""
    need = [lds_need(w, runs_x10, rcap_key) for w in words_list]
    canvas = [i for i, nd in enumerate(need) if not lds or nd > lds_max]
    order = sorted((i for i, nd in enumerate(need) if lds and nd <= lds_max), key=lambda i: words_list[i])
    launches, k0 = [], 0
    for c, limit in enumerate((cls0, cls1, None)):
        k1 = k0
        while k1 < len(order) and (limit is None or need[order[k1]] <= limit):
            k1 += 1
        if k1 > k0:
            mw = words_list[order[k1 - 1]]
            launches.append((k1 - k0, mw, lds_rcap(mw, runs_x10, rcap_key), lds_need(mw, runs_x10, rcap_key), order[k0:k1]))
        k0 = k1
    return canvas, launches


def case_words(case):
    """Plane words of a case's windows in the order the native tail sees them (pass 0 only: no case here keeps undetected)."""
    assert not case["keep"]
    return [words_of(w, h) for img, boxes in zip(case["pages"], case["boxes"]) for _, _, w, h in windows_of(img.shape, boxes)]


def stroke_page(im_w, im_h, seed, density):
    """Text-like content: dark horizontal and vertical strokes and a few squares with a light hole on a light ground, light
    on dark in the left half, mild noise; the mask is the ink grown by one pixel (holes covered) with 3 % of it knocked about.
    Few runs per word -- the noisy kinds of `page_for_windows` have about 8 and overflow every run table."""
    from scipy import ndimage
    rng = np.random.RandomState(seed)
    ink = np.zeros((im_h, im_w), bool)
    hole = np.zeros((im_h, im_w), bool)
    n = max(6, int(density * im_w * im_h / 450))
    for k in range(n):
        y, x = rng.randint(0, im_h), rng.randint(0, im_w)
        if k % 5 in (0, 1):
            ink[y: y + rng.randint(2, 4), x: x + rng.randint(3, 40)] = True              # horizontal strokes
        elif k % 5 in (2, 3):
            ink[y: y + rng.randint(3, 40), x: x + rng.randint(2, 4)] = True              # vertical strokes
        else:
            s = rng.randint(9, 14)
            ink[y: y + s, x: x + s] = True                                               # a square with a hole
            hole[y + 3: y + s - 3, x + 3: x + s - 3] = True
    hole &= ndimage.binary_erosion(ink, np.ones((7, 7), bool))                           # holes stay inside their squares
    page = np.full((im_h, im_w, 3), 215, np.uint8)
    page[ink & ~hole] = 35
    page = (page.astype(int) + rng.randint(-6, 7, page.shape)).clip(0, 255).astype(np.uint8)
    page[:, : im_w // 2] = 255 - page[:, : im_w // 2]
    mask = (ndimage.maximum_filter(ink.astype(np.uint8), size=3) * 210).astype(np.uint8)
    knock = rng.rand(im_h, im_w) < 0.03
    mask[knock] = rng.randint(0, 256, int(knock.sum()))
    return np.ascontiguousarray(page), np.ascontiguousarray(mask)


def _stroke_case(name, sheets, mode=0):
    """A case from [(im_w, im_h, seed, stroke density, windows or ready-made boxes)]: stroke content everywhere."""
    pages, masks, boxes = [], [], []
    for im_w, im_h, seed, density, wins in sheets:
        img, mask = stroke_page(im_w, im_h, seed, density)
        pages.append(img), masks.append(mask)
        boxes.append([w if len(w) == 5 else block_for_window(im_w, im_h, w) for w in wins])
    for b in boxes:
        for i, w in enumerate(b):
            b[i] = list(w[:4])
    return _case(name, pages, masks, boxes, mode=mode)


# word counts of `block_size_case`, in window order (checked against `windows_of` in tests/test_tail_trace_cases.py)
ONE_WORD_HEIGHTS = (255, 256, 257, 511, 512, 513, 1023, 1024, 1025)
THREE_WORD_HEIGHTS = (85, 86, 171, 341, 342)                  # 255, 258, 513, 1 023, 1 026 words: blockDim is no multiple of wp = 3
STRIP = (8193, 3)                                             # wp = 257 > 256: dy_t = 0 at 256 threads
LARGE = (256, 260)                                            # 2 080 words > 2 048: at `tail_lds_runs_x10` = 1, rlay = 1 040 > rcap = 1 024


def block_size_windows():
    """[page][window] of `block_size_case`: a tall page of one- and three-word columns, the strip's own page, a page with
    the large window next to a 1 x 1 and a 33 x 2 one.  (A tall window narrower than twice its padding -- about h / 32 --
    exists only where a page edge cuts it: the 5- and 9-wide ones stand on the left and right edge.)"""
    im_w, im_h = TALL_PAGE
    H = ONE_WORD_HEIGHTS
    tall = [(8, 0, 32, H[0]), (8, 258, 31, H[1]), (8, im_h - 1 - H[2], 17, H[2]), (43, 0, 32, H[3]), (43, im_h - 1 - H[4], 25, H[4]),
            (78, 0, 30, H[5]), (im_w - 1 - 9, 0, 9, H[6]), (113, 0, 32, H[7]), (0, 0, 5, H[8])]
    three = ((65, 85), (96, 86), (70, 171), (95, 341), (81, 342))
    y = 0
    for w, h in three[:3]:
        tall.append((148, y, w, h))
        y += h + 3
    tall.append((247, 0, *three[3]))
    tall.append((247, 345, *three[4]))
    small = [(20, 12, *LARGE), (7, 5, 1, 1), (100, SMALL_PAGE[1] - 1 - 2, 33, 2)]
    return [tall, [(0, 0, *STRIP)], small]


SMALL_DENSITY = 0.4       # the large window's labellings stay under 1 024 runs: it completes at `tail_lds_runs_x10` = 1
TALL_PAGE, STRIP_PAGE, SMALL_PAGE = (360, 1030), (STRIP[0] + 1, STRIP[1] + 1), (300, 300)


@functools.lru_cache(None)
def block_size_case():
    """One call whose windows have word counts on both sides of each block size of `tw_lds_kernel` (`tail_lds_threads`)."""
    tall, strip, small = block_size_windows()
    # the strip reaches the page's four edges: a block one row high, whose padding (128) overshoots them all
    strip_box = [10, 1, STRIP[0] - 10, 2, "box"]
    assert windows_of((STRIP_PAGE[1], STRIP_PAGE[0]), [strip_box[:4]]) == strip
    return _stroke_case("block sizes: word counts around 256 / 512 / 1 024", [(*TALL_PAGE, 80, 1.0, tall), (*STRIP_PAGE, 81, 1.0, [strip_box]),
                                                                               (*SMALL_PAGE, 82, SMALL_DENSITY, small)])


@functools.lru_cache(None)
def large_window_case():
    """`block_size_case`'s large window alone (2 080 words)."""
    return _stroke_case("the 256 x 260 window alone", [(*SMALL_PAGE, 82, SMALL_DENSITY, [(20, 12, *LARGE)])], mode=1)


# (w, h) of `class_case`, in window order: 1 .. 4 515 words (the largest count whose need is within 150 KB, `tail_lds_max_bytes`), two of 600
CLASS_SIZES = ((480, 301), (1, 1), (96, 200), (256, 260), (20, 40), (160, 120), (200, 171), (64, 50), (224, 186), (100, 100), (33, 2))
CLASS_PAGE = (520, 640)


def class_windows():
    at = ((3, 0), (7, 5), (10, 20), (2, 310), (400, 8), (150, 40), (262, 310), (340, 200), (270, 450), (330, 60), (100, 640 - 1 - 2))
    return [(x, y, w, h) for (x, y), (w, h) in zip(at, CLASS_SIZES)]


@functools.lru_cache(None)
def class_case():
    """About ten windows from 1 x 1 to the largest the default LDS limit admits, unsorted, two of equal word counts."""
    return _stroke_case("launch classes: 1 to 4 515 words", [(*CLASS_PAGE, 83, 1.0, class_windows())])


def need_by_default(words):
    k = key_defaults()
    return lds_need(words, k["tail_lds_runs_x10"], k["tail_lds_rcap"])


def class_settings():
    """[(what, {tuning key: value})] for `class_case`: the limits of the first two launch classes moved so that windows
    change launch, a limit exactly AT a window's need (it stays in the lower class) and one byte below (it moves up)."""
    k = key_defaults()
    n400, n600, n1197, n2080 = (need_by_default(w) for w in (400, 600, 1197, 2080))
    return [("the defaults", {}),
            ("one class", {"tail_lds_cls0": k["tail_lds_max_bytes"], "tail_lds_cls1": k["tail_lds_max_bytes"]}),
            ("cls0 = 0", {"tail_lds_cls0": 0}),
            ("cls1 < cls0", {"tail_lds_cls0": k["tail_lds_cls1"], "tail_lds_cls1": k["tail_lds_cls0"]}),
            ("cls0 at the need of the 1 197-word window, cls1 at that of the 2 080-word one", {"tail_lds_cls0": n1197, "tail_lds_cls1": n2080}),
            ("both one byte below", {"tail_lds_cls0": n1197 - 1, "tail_lds_cls1": n2080 - 1}),
            ("the two 600-word windows a launch of their own", {"tail_lds_cls0": n400, "tail_lds_cls1": n600}),
            ("the 1 x 1 window alone, then all but the largest", {"tail_lds_cls0": need_by_default(1), "tail_lds_cls1": n2080})]


def launches_of_setting(words_list, tune=()):
    """`lds_launches` under the library's defaults with `tune` = {key: value} on top."""
    k = {**key_defaults(), **dict(tune)}
    return lds_launches(words_list, k["tail_lds_cls0"], k["tail_lds_cls1"], k["tail_lds_max_bytes"], k["tail_lds_runs_x10"],
                        k["tail_lds_rcap"], k["tail_lds"])


def compare_launches(got, want):
    """`Tail.trace_lds_launches()` (plus the threads every launch must show) against (launches of `lds_launches`, threads)."""
    launches, threads = want
    mine = [(g["windows"], g["max_words"], g["rcap"], g["bytes"], g["threads"], g["refused"]) for g in got]
    assert mine == [(n, mw, rc, by, threads, 0) for n, mw, rc, by, _ in launches], f"launches {mine} vs {[l[:4] for l in launches]} at {threads} threads"


@functools.lru_cache(None)
def merge_stats(case_fn):
    """Per window of a case, from tests/twlds_emul.py on the oracle's own candidates: `words`; `runs` = (most runs of a
    candidate after the small-component rule, runs of the complement hole filling labels in mode 0, in mode 1);
    `accepted` = pixels the merge rounds set; `filled` = pixels hole filling added, both modes together."""
    import twlds_emul as E
    case = case_fn()
    out = []
    for img, mask, boxes in zip(case["pages"], case["masks"], case["boxes"]):
        for x1, y1, w, h in windows_of(img.shape, boxes):
            im = np.ascontiguousarray(img[y1: y1 + h, x1: x1 + w])
            msk = np.ascontiguousarray(mask[y1: y1 + h, x1: x1 + w])
            ml = R.get_topk_masklist(im, msk) + R.get_otsuthresh_masklist(im, msk)
            ml.sort(key=lambda c: c[1])
            win = E.Win(h, w)
            pred = E.pred_plane(win, msk)
            merged = [[0] * win.wp for _ in range(h)]
            runs = [max(E.accept_round(win, E.to_plane(c > 0), pred, merged) for c, _ in ml)]
            accepted = sum(E.popc(v) for row in merged for v in row)
            filled = 0
            for mode in (0, 1):
                m = E.dilate(win, merged) if mode == 0 else [row[:] for row in merged]
                before = sum(E.popc(v) for row in m for v in row)
                runs.append(E.fill_holes(win, pred, m))
                filled += sum(E.popc(v) for row in m for v in row) - before
            out.append(dict(words=words_of(w, h), runs=tuple(runs), accepted=accepted, filled=filled))
    return out


def expected_paths(case_fn, mode, tune=()):
    """`Tail.refine_paths()` of a case in one refine mode from the restatement and the emulation's run counts: a window
    overflows iff a candidate's labelling, or the complement's, has more runs than its LAUNCH's rcap."""
    st = merge_stats(case_fn)
    canvas, launches = launches_of_setting([s["words"] for s in st], tune)
    over = sum(max(st[i]["runs"][0], st[i]["runs"][1 + mode]) > rcap for _, _, rcap, _, idx in launches for i in idx)
    return {"lds": len(st) - len(canvas) - over, "canvas": len(canvas) + over, "overflow": over}


# ---- what the wrong kernels the issue measured would write (the CPU test: the cases tell them from the right one) -----------

def hist_with(img, msk, mode):
    """The grey histogram of a window under one of the errors of the issue's table: 'page0' = pixels outside the window count
    as 0 in the erosion, 'ge127' = eroded >= 127 selects, 'lastcol' = the window's last column is left out."""
    grey = cv.cvt_bgr2gray(np.ascontiguousarray(img))
    assert mode in ("right", "page0", "ge127", "lastcol")
    if mode == "page0":
        pad = np.zeros((msk.shape[0] + 2, msk.shape[1] + 2), np.uint8)
        pad[1:-1, 1:-1] = msk
        er = cv.erode(pad, cv.RECT3, 1)[1:-1, 1:-1]
    else:
        er = cv.erode(np.ascontiguousarray(msk), cv.RECT3, 1)
    sel = er >= 127 if mode == "ge127" else er > 127
    if mode == "lastcol":
        sel = sel.copy()
        sel[:, -1] = False
    return np.bincount(grey[sel], minlength=256).astype(np.uint32)


def hist_reading_the_page(img, mask, win):
    """The grey histogram if the erosion read the page's mask beyond the window instead of ignoring it."""
    x1, y1, w, h = win
    er = cv.erode(np.ascontiguousarray(mask), cv.RECT3, 1)[y1: y1 + h, x1: x1 + w]
    grey = cv.cvt_bgr2gray(np.ascontiguousarray(img[y1: y1 + h, x1: x1 + w]))
    return np.bincount(grey[er > 127], minlength=256).astype(np.uint32)


# ============================================================================================================ DB stage

COMP_CAP = 1 << 16                  # kCompCap / kRowCap of csrc/tail.hip
ROW_CAP = 1 << 18


def overflow_map():
    """More single-pixel components than the compact tables hold (67 259 > 65 536), plus one solid block: the construction of
    test_db_stage_on_device_tables_matches_oracle_and_falls_back_on_overflow, whose own 516-a-side map has 65 179 and fits."""
    big = np.full((524, 524), 0.05, np.float32)
    big[::2, ::2] = 0.9
    big[100:140, 200:330] = 0.95
    return big


@functools.lru_cache(None)
def db_calls():
    """[(call name, [(map name, prob (H,W) f32)])]: the maps of one call share a shape."""
    import test_db_compact as T
    edge = [(c, T.edge_map(c)[0]) for c in T.EDGE_CASES]
    calls = [("edge maps holes / thin / empty in one call", edge[:3]), ("edge maps full / cap / frame in one call", edge[3:])]
    for seed in (0, 1, 3):
        calls.append((f"speckle {seed}", [(f"speckle {seed}", T.speckle(seed))]))
    rng = np.random.RandomState(5)
    for h, w in ((1, 1), (1, 40), (40, 1), (31, 31), (32, 32), (33, 33)):
        from scipy import ndimage
        pr = ndimage.uniform_filter(rng.rand(h, w), 2).astype(np.float32)
        span = float(pr.max() - pr.min())
        pr = ((pr - pr.min()) / span * 0.62 if span > 0 else np.full((h, w), 0.9)).astype(np.float32)
        if h == 1 and w == 1:
            calls.append(("1 x 1, foreground and background in one call", [("1 x 1 set", np.full((1, 1), 0.9, np.float32)),
                                                                            ("1 x 1 clear", np.full((1, 1), 0.1, np.float32))]))
        else:
            calls.append((f"{h} x {w}", [(f"{h} x {w}", pr)]))
    calls.append(("over the table capacity", [("overflow", overflow_map())]))
    return calls


def db_counts(prob):
    """(n_f, n_b) of a map from the labelling alone (the overflow map: its tables are not emulated)."""
    bitmap = prob > 0.3
    nf = R.connected_components_with_stats(bitmap.astype(np.uint8), 8)[0] - 1
    nb = R.connected_components_with_stats((~bitmap).astype(np.uint8), 4)[0] - 1
    return nf, nb


def gamma(k):
    """Higham's gamma_k = k u / (1 - k u): k successive roundings change a product of (1 + d_i), |d_i| <= u, by at most this."""
    k = np.asarray(k, np.float64)
    return k * U / (1 - k * U)


def db_reference(prob):
    """`dbc_tables` of prob > 0.3 plus, per f64 sum, the bound on |device - emulation| DERIVED from how each side adds:

    Emulation (`np.bincount` with f64 weights, `+=` in a loop): n - 1 successive f64 additions of the n pixels p (f32 values, exact
    in f64): |emul - exact| <= gamma(n-1) S, S = sum |p|.

    ring_sum on the device (dbc_accum_kernel): one f64 atomic add per ring pixel into a zeroed f64, in any order: n - 1 roundings,
    the same bound, so |device - emul| <= 2 gamma(n-1) S  (first order: 2 (n-1) 2^-53 S).

    sum_f / sum_b on the device are NOT plain adds.  A wave holds 64 consecutive pixels of the page's linear index (blocks start
    at multiples of 256).  It takes the inclusive prefix sums ps_i of its 64 values in six shuffle-add steps (every ps_i is a
    tree of depth <= 6 over the values before it: |ps_i - exact| <= gamma(6) A_i, A_i = sum_{j <= i} |p_j| over ALL labels in the
    wave), then a run of equal labels [a, b] inside the wave contributes fl(ps_b - ps_{a-1}):
        |run - exact| <= gamma(6) (A_b + A_{a-1}) + u |ps_b - ps_{a-1}|  <=  gamma(7) (A_b + A_{a-1})      (|ps| <= (1 + gamma(6)) A),
    and the R runs of a component are added by f64 atomics in any order: R - 1 more roundings of partial sums bounded by
    sum |run| <= S + sum of the run errors.  Altogether
        |device - exact| <= (1 + gamma(R)) sum_runs gamma(7) (A_b + A_{a-1}) + gamma(R-1) S.
    The bound returned is that plus the emulation's gamma(n-1) S.  It is a few 1e-14 relative here, against a pixel's 0.05 .. 0.9."""
    bitmap = prob > 0.3
    t = dbc_emul.dbc_tables(prob, bitmap)
    H, W = bitmap.shape
    N = H * W
    key = np.where(t["lab_f"] > 0, t["lab_f"], -t["lab_b"]).astype(np.int64).ravel()
    a = np.abs(prob.astype(np.float64)).ravel()
    pad = (-N) % 64
    A = np.cumsum(np.r_[a, np.zeros(pad)].reshape(-1, 64), axis=1).ravel()[:N]
    idx = np.arange(N)
    head = (idx % 64 == 0) | (idx % W == 0)
    head[1:] |= key[1:] != key[:-1]
    hi = np.nonzero(head)[0]
    ti = np.r_[hi[1:] - 1, N - 1]
    a_prev = np.where(hi % 64 == 0, 0.0, A[np.maximum(hi - 1, 0)])
    spread = A[ti] + a_prev
    rk = key[hi]
    nf, nb = t["n_f"], t["n_b"]

    def bound(labels_of_runs, n_lab, labels_of_pixels):
        s1 = np.bincount(labels_of_runs, weights=spread, minlength=n_lab + 1)[1:]
        runs = np.bincount(labels_of_runs, minlength=n_lab + 1)[1:]
        n = np.bincount(labels_of_pixels, minlength=n_lab + 1)[1:]
        S = np.bincount(labels_of_pixels, weights=a, minlength=n_lab + 1)[1:]
        return (1 + gamma(runs)) * gamma(7) * s1 + gamma(np.maximum(runs - 1, 0)) * S + gamma(np.maximum(n - 1, 0)) * S

    t["bound_sum_f"] = bound(np.maximum(rk, 0), nf, np.maximum(key, 0))
    hole = t["par_b"] > 0 if nb else np.zeros(0, bool)
    t["bound_sum_b"] = bound(np.maximum(-rk, 0), nb, np.maximum(-key, 0)) * hole
    # ring pixels: S from the emulation's own ring membership is not kept; ring values are probabilities of foreground pixels of
    # the ringing component, so S = |ring_sum| up to its own error (all p >= 0 here; asserted)
    assert (prob >= 0).all()
    n = t["ring_cnt"].astype(np.float64)
    t["bound_ring_sum"] = 2 * gamma(np.maximum(n - 1, 0)) * t["ring_sum"] * (1 + gamma(np.maximum(n - 1, 0)))
    t["rows"] = int(t["st_f"][:, 3].sum()) + int(np.where(hole, t["st_b"][:, 3] + 2, 0).sum())
    return t


_INT_TABLES = ("st_f", "first_f", "par_f", "off_f", "st_b", "first_b", "par_b", "off_b", "ring_cnt")
_EMPTY_LO, _EMPTY_HI = 0x7fffffff, -1


def compare_db_tables(got, ref):
    """One page of `Tail.trace_db()` against `db_reference`: header, every integer table over its used range and the row
    tables exact (a row no pixel touched is empty on both sides, whatever it holds), the f64 sums within their derived bounds."""
    nf, nb, rows = int(ref["n_f"]), int(ref["n_b"]), int(ref["rows"])
    if nf > COMP_CAP or nb > COMP_CAP or rows > ROW_CAP:                 # by the EMULATION's counts only
        assert int(got["hdr"][3]) == 1, f"overflow flag {int(got['hdr'][3])} vs 1"
        return
    want = [nf, nb, rows, 0]
    assert [int(v) for v in got["hdr"]] == want, f"hdr: {[int(v) for v in got['hdr']]} vs {want}"
    for k in _INT_TABLES:
        g, r = np.asarray(got[k]), np.asarray(ref[k])
        assert g.shape == r.shape, f"{k}: shape {g.shape} vs {r.shape}"
        bad = np.argwhere(g != r)
        assert not len(bad), f"{k}{tuple(int(v) for v in bad[0])}: {g[tuple(bad[0])]} vs {r[tuple(bad[0])]} ({len(bad)} differ)"
    glo, ghi = np.asarray(got["row_lo"]).copy(), np.asarray(got["row_hi"]).copy()
    rlo, rhi = np.asarray(ref["row_lo"])[:rows].copy(), np.asarray(ref["row_hi"])[:rows].copy()
    assert len(glo) == len(ghi) == rows, f"row tables: {len(glo)}, {len(ghi)} entries vs {rows}"
    for lo, hi in ((glo, ghi), (rlo, rhi)):
        e = lo > hi
        lo[e], hi[e] = _EMPTY_LO, _EMPTY_HI
    for k, g, r in (("row_lo", glo, rlo), ("row_hi", ghi, rhi)):
        bad = np.nonzero(g != r)[0]
        assert not len(bad), f"{k}[{int(bad[0])}]: {g[bad[0]]} vs {r[bad[0]]} ({len(bad)} differ)"
    for k in ("sum_f", "sum_b", "ring_sum"):
        g, r, bnd = np.asarray(got[k]), np.asarray(ref[k]), np.asarray(ref["bound_" + k])
        assert g.shape == r.shape, f"{k}: shape {g.shape} vs {r.shape}"
        bad = np.nonzero(~(np.abs(g - r) <= bnd))[0]
        assert not len(bad), f"{k}[{int(bad[0])}]: {g[bad[0]]!r} vs {r[bad[0]]!r}, bound {bnd[bad[0]]:.3e} ({len(bad)} beyond)"
