"""The pull-push fill rule of include/ctd_hip.h (`ctd_fill_rest`) restated in numpy, three times:

  fill_loops   plain Python loops, pixel by pixel, straight from the rule's text;
  fill_vec     whole levels at a time;
  fill_emul    tile-wise, as csrc/kernels_fill.hip runs it: a pull of levels 1 .. 6 per aligned 64 x 64 tile, one block per page
               for the levels above 6 and the push down to level 6, a push per tile from levels 1 .. 6 loaded with a halo of
               one pixel at coordinates clamped to the level.

All three return (out, row): `out` (H,W,3) u8 and `row` = {status, n_hole, levels, top}.  Integers only, so every comparison
with them is exact.  `material()` is the pages the tests of the rule and of the kernels share, `large_material()` the pages at
the sizes the page launch is sized for (up to T = 13 and 378 tiles), and `fill_blocks` the rule on a page that is constant on
aligned 2^s x 2^s blocks, where it scales exactly: the reference of the 8192 x 8192 pages of `capacity_blocks()`."""
import numpy as np

OK, NO_HOLE, NO_KNOWN = range(3)
MAX_SIDE, TILE = 8192, 64
FIELDS = ("status", "n_hole", "levels", "top")


def level_shapes(H, W):
    """[(H_l, W_l)] for l = 0 .. T."""
    out = [(int(H), int(W))]
    while out[-1] != (1, 1):
        h, w = out[-1]
        out.append(((h + 1) // 2, (w + 1) // 2))
    return out


def row_dict(rec):
    """A `fill.ROW_DTYPE` record as the dict the restatements return."""
    return {"status": int(rec["status"]), "n_hole": int(rec["n_hole"]), "levels": int(rec["levels"]),
            "top": [int(v) for v in rec["top"]]}


def _row(n_hole, T, top_c, top_k):
    status = NO_HOLE if n_hole == 0 else OK if top_k else NO_KNOWN
    return {"status": status, "n_hole": int(n_hole), "levels": int(T), "top": [int(v) for v in top_c] if top_k else [0, 0, 0]}


# ---- 1. plain loops ------------------------------------------------------------------------------------------------------------

def fill_loops(P, R):
    H, W = R.shape
    shapes = level_shapes(H, W)
    T = len(shapes) - 1
    c = [[[[int(v) for v in P[y, x]] for x in range(W)] for y in range(H)]]
    k = [[[1 if R[y, x] == 0 else 0 for x in range(W)] for y in range(H)]]
    n_hole = sum(1 - v for r in k[0] for v in r)
    for l in range(T):                                               # pull
        (h, w), (h2, w2) = shapes[l], shapes[l + 1]
        cl, kl = [], []
        for y in range(h2):
            cr, kr = [], []
            for x in range(w2):
                n, S = 0, [0, 0, 0]
                for dy in (0, 1):
                    for dx in (0, 1):
                        yy, xx = 2 * y + dy, 2 * x + dx
                        if yy < h and xx < w and k[l][yy][xx]:
                            n += 1
                            for ch in range(3):
                                S[ch] += c[l][yy][xx][ch]
                kr.append(1 if n else 0)
                cr.append([(2 * s + n) // (2 * n) for s in S] if n else [0, 0, 0])
            cl.append(cr)
            kl.append(kr)
        c.append(cl)
        k.append(kl)
    row = _row(n_hole, T, c[T][0][0], k[T][0][0])
    out = P.copy()
    if row["status"] != OK:
        return out, row
    for l in range(T - 1, -1, -1):                                   # push
        (h, w), (h2, w2) = shapes[l], shapes[l + 1]
        for y in range(h):
            for x in range(w):
                if k[l][y][x]:
                    continue
                py, px = y >> 1, x >> 1
                ny = min(max(py + (1 if y & 1 else -1), 0), h2 - 1)
                nx = min(max(px + (1 if x & 1 else -1), 0), w2 - 1)
                u = c[l + 1]
                c[l][y][x] = [(9 * u[py][px][ch] + 3 * u[py][nx][ch] + 3 * u[ny][px][ch] + u[ny][nx][ch] + 8) >> 4 for ch in range(3)]
    for y in range(H):
        for x in range(W):
            if R[y, x] != 0:
                out[y, x] = c[0][y][x]
    return out, row


# ---- 2. whole levels -------------------------------------------------------------------------------------------------------------

def pull_level(c, k):
    """(c (h,w,3) i64, k (h,w) bool) of level l -> the same of level l + 1; c is 0 where k is not set."""
    h, w = k.shape
    h2, w2 = (h + 1) // 2, (w + 1) // 2
    cp = np.zeros((2 * h2, 2 * w2, 3), np.int64)
    kp = np.zeros((2 * h2, 2 * w2), np.int64)
    cp[:h, :w] = c * k[:, :, None]
    kp[:h, :w] = k
    n = kp.reshape(h2, 2, w2, 2).sum(axis=(1, 3))
    S = cp.reshape(h2, 2, w2, 2, 3).sum(axis=(1, 3))
    n3 = n[:, :, None]
    return np.where(n3 > 0, (2 * S + n3) // np.maximum(2 * n3, 1), 0), n > 0


def _neighbours(n, n2):
    """py, ny of the rule for coordinates 0 .. n - 1 of a level whose parent level has n2 rows (or columns)."""
    y = np.arange(n)
    py = y >> 1
    return py, np.clip(py + np.where(y & 1, 1, -1), 0, n2 - 1)


def push_level(c, k, up):
    """Level l as pulled (c, k) and the FINISHED level l + 1 -> the finished level l."""
    h, w = k.shape
    py, ny = _neighbours(h, up.shape[0])
    px, nx = _neighbours(w, up.shape[1])
    v = (9 * up[py][:, px] + 3 * up[py][:, nx] + 3 * up[ny][:, px] + up[ny][:, nx] + 8) >> 4
    return np.where(k[:, :, None], c, v)


def fill_vec(P, R):
    H, W = R.shape
    T = len(level_shapes(H, W)) - 1
    c, k = [P.astype(np.int64)], [R == 0]
    for l in range(T):
        cn, kn = pull_level(c[l], k[l])
        c.append(cn)
        k.append(kn)
        assert kn.shape == level_shapes(H, W)[l + 1]
    row = _row(int((R != 0).sum()), T, c[T][0, 0], bool(k[T][0, 0]))
    if row["status"] != OK:
        return P.copy(), row
    fin = c[T]
    for l in range(T - 1, -1, -1):
        fin = push_level(c[l], k[l], fin)
    return fin.astype(np.uint8), row


# ---- 3. as the three launches run it -------------------------------------------------------------------------------------------

def _dim(n, l):
    return (n + (1 << l) - 1) >> l


def fill_emul(P, R):
    H, W = R.shape
    T = len(level_shapes(H, W)) - 1
    ty_n, tx_n = _dim(H, 6), _dim(W, 6)
    # launch A: every tile pulls its 64 x 64 pixels up to ONE pixel; what lies beyond the page has k = 0
    lc = {l: np.zeros((_dim(H, l), _dim(W, l), 3), np.int64) for l in range(1, 7)}
    lk = {l: np.zeros((_dim(H, l), _dim(W, l)), bool) for l in range(1, 7)}
    counts = np.zeros((ty_n, tx_n), np.int64)
    for ty in range(ty_n):
        for tx in range(tx_n):
            y0, x0 = 64 * ty, 64 * tx
            th, tw = min(64, H - y0), min(64, W - x0)
            c = np.zeros((64, 64, 3), np.int64)
            k = np.zeros((64, 64), bool)
            c[:th, :tw] = P[y0:y0 + th, x0:x0 + tw]
            k[:th, :tw] = R[y0:y0 + th, x0:x0 + tw] == 0
            counts[ty, tx] = int((R[y0:y0 + th, x0:x0 + tw] != 0).sum())
            for l in range(1, 7):
                c, k = pull_level(c, k)
                n = 64 >> l
                hh, ww = min(n, _dim(H, l) - n * ty), min(n, _dim(W, l) - n * tx)
                assert not k[hh:].any() and not k[:, ww:].any()      # nothing beyond the level's edge
                lc[l][n * ty:n * ty + hh, n * tx:n * tx + ww] = c[:hh, :ww]
                lk[l][n * ty:n * ty + hh, n * tx:n * tx + ww] = k[:hh, :ww]
    # launch B: one block per page pulls the level-6 plane up to 1 x 1 and pushes it back down; below T = 6 the plane is
    # one pixel already
    n_hole = 0
    for v in counts.ravel():                                         # a sum in a fixed order
        n_hole += int(v)
    uc, uk = [lc[6]], [lk[6]]
    while uk[-1].shape != (1, 1):
        cn, kn = pull_level(uc[-1], uk[-1])
        uc.append(cn)
        uk.append(kn)
    assert 6 + len(uc) - 1 == max(T, 6)
    row = _row(n_hole, T, uc[-1][0, 0], bool(uk[-1][0, 0]))
    if row["status"] != OK:
        return P.copy(), row                                         # launch C copies
    fin = uc[-1]
    for i in range(len(uc) - 2, -1, -1):
        fin = push_level(uc[i], uk[i], fin)
    lc[6], lk[6] = fin, np.ones_like(lk[6])
    # launch C: a tile loads levels 6 .. 1 with a halo of one at coordinates clamped to the level and pushes down
    out = P.copy()
    for ty in range(ty_n):
        for tx in range(tx_n):
            if counts[ty, tx] == 0:
                continue
            slots_c, coords = {}, {}
            for l in range(6, 0, -1):
                n = 64 >> l
                ys = np.clip(n * ty - 1 + np.arange(n + 2), 0, _dim(H, l) - 1)
                xs = np.clip(n * tx - 1 + np.arange(n + 2), 0, _dim(W, l) - 1)
                sc, sk = lc[l][ys][:, xs], lk[l][ys][:, xs]
                if l < 6:
                    # a slot is the level pixel at its clamped coordinate; its parents lie in the level above's slots
                    oy2, ox2 = (n // 2) * ty - 1, (n // 2) * tx - 1
                    py = ys >> 1
                    ny = np.clip(py + np.where(ys & 1, 1, -1), 0, _dim(H, l + 1) - 1)
                    px = xs >> 1
                    nx = np.clip(px + np.where(xs & 1, 1, -1), 0, _dim(W, l + 1) - 1)
                    a, b, cc, d = py - oy2, ny - oy2, px - ox2, nx - ox2
                    for idx in (a, b, cc, d):
                        assert idx.min() >= 0 and idx.max() <= n // 2 + 1     # the halo of ONE pixel is enough
                    up = slots_c[l + 1]
                    # and those slots hold the pixels the rule names
                    assert np.array_equal(coords[l + 1][0][a], py) and np.array_equal(coords[l + 1][0][b], ny)
                    assert np.array_equal(coords[l + 1][1][cc], px) and np.array_equal(coords[l + 1][1][d], nx)
                    v = (9 * up[a][:, cc] + 3 * up[a][:, d] + 3 * up[b][:, cc] + up[b][:, d] + 8) >> 4
                    sc = np.where(sk[:, :, None], sc, v)
                slots_c[l], coords[l] = sc, (ys, xs)
            y0, x0 = 64 * ty, 64 * tx
            th, tw = min(64, H - y0), min(64, W - x0)
            y, x = y0 + np.arange(th), x0 + np.arange(tw)
            py, px = y >> 1, x >> 1
            ny = np.clip(py + np.where(y & 1, 1, -1), 0, _dim(H, 1) - 1)
            nx = np.clip(px + np.where(x & 1, 1, -1), 0, _dim(W, 1) - 1)
            oy1, ox1 = 32 * ty - 1, 32 * tx - 1
            a, b, cc, d = py - oy1, ny - oy1, px - ox1, nx - ox1
            up = slots_c[1]
            v = (9 * up[a][:, cc] + 3 * up[a][:, d] + 3 * up[b][:, cc] + up[b][:, d] + 8) >> 4
            hole = R[y0:y0 + th, x0:x0 + tw] != 0
            out[y0:y0 + th, x0:x0 + tw] = np.where(hole[:, :, None], v, P[y0:y0 + th, x0:x0 + tw])
    return out, row


# ---- 4. the material ---------------------------------------------------------------------------------------------------------

SIZES = ((1, 1), (1, 7), (9, 1), (63, 65), (64, 64), (65, 129), (97, 83), (130, 67), (200, 330))


def ramp_page(H, W):
    """Linear ramps of 0 .. 255: across, down, and along the diagonal."""
    x = (np.arange(W) * 255 // max(W - 1, 1))[None, :] + np.zeros((H, 1), np.int64)
    y = (np.arange(H) * 255 // max(H - 1, 1))[:, None] + np.zeros((1, W), np.int64)
    return np.stack([x, y, (x + y) // 2], axis=2).astype(np.uint8)


def parity_singles(H, W, qy, qx):
    """Single hole pixels of parity (qy, qx) next to every edge and corner, and in the middle."""
    R = np.zeros((H, W), np.uint8)
    ys = sorted({v for v in (0, 1, H - 2, H - 1, H // 2, H // 2 + 1) if 0 <= v < H and (v & 1) == qy})
    xs = sorted({v for v in (0, 1, W - 2, W - 1, W // 2, W // 2 + 1) if 0 <= v < W and (v & 1) == qx})
    for y in ys:
        for x in xs:
            R[y, x] = 255
    return R


def holes_of(H, W, rng):
    """[(name, R)] for one size, in the order they are passed: a page without a hole stands between pages with holes."""
    out = [("all", np.full((H, W), 255, np.uint8))]
    for dens in (0.02, 0.5, 0.98):
        out.append((f"random{dens}", ((rng.random((H, W)) < dens) * rng.integers(1, 256, (H, W))).astype(np.uint8)))
    out.insert(2, ("none", np.zeros((H, W), np.uint8)))
    yy, xx = np.mgrid[0:H, 0:W]
    out.append(("checker", (((yy + xx) & 1) * 255).astype(np.uint8)))
    for cy, cx in dict.fromkeys(((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1))):   # a 1 x n page has fewer corners
        R = np.full((H, W), 1, np.uint8)
        R[cy, cx] = 0
        out.append((f"one_known_{cy}_{cx}", R))
    for qy in (0, 1):
        for qx in (0, 1):
            R = parity_singles(H, W, qy, qx)
            if R.any():
                out.append((f"singles{qy}{qx}", R))
    if (H, W) == (200, 330):
        R = np.zeros((H, W), np.uint8)
        R[0:130, 60:260] = 255                                       # covers whole aligned tiles: level 6 has unknown pixels
        out.append(("big_top", R))
        R = np.zeros((H, W), np.uint8)
        R[H - 130:, W - 200:] = 255
        out.append(("big_corner", R))
        R = np.zeros((H, W), np.uint8)
        for x in (64, 128, 192, 256):                                # thin bars across the tile seams
            R[10:190, x - 2:x + 3] = 255
        for y in (64, 128):
            R[y - 1:y + 2, 5:325] = 200
        out.append(("bars", R))
    return out


_MATERIAL = {}


def material():
    """[(name, page, hole mask)]: every size with every hole pattern; pages of noise, the ramp page and a flat colour in turn,
    the ramp page under the big holes.  Made once."""
    if "m" not in _MATERIAL:
        rng = np.random.default_rng(419)
        out = []
        for H, W in SIZES:
            for i, (name, R) in enumerate(holes_of(H, W, rng)):
                kind = 1 if name.startswith("big") else i % 3
                page = (rng.integers(0, 256, (H, W, 3), dtype=np.uint8), ramp_page(H, W),
                        np.full((H, W, 3), (17, 250, 133), np.uint8))[kind]
                out.append((f"{H}x{W}-{name}-{('noise', 'ramp', 'flat')[kind]}", page, R))
        _MATERIAL["m"] = out
    return _MATERIAL["m"]


_REFERENCE = {}


def reference():
    """[(out, row)] of `fill_vec` on `material()`: computed once, shared, never changed."""
    if "r" not in _REFERENCE:
        res = [fill_vec(p, r) for _, p, r in material()]
        for o, _ in res:
            o.setflags(write=False)
        _REFERENCE["r"] = res
    return _REFERENCE["r"]


# ---- 5. pages at the sizes the page launch is sized for ------------------------------------------------------------------------

LARGE_SIZES = ((1, 8192), (8192, 1), (65, 8129), (1024, 1024), (1025, 1025), (1100, 1300))
# what each size gets (about 40 cases in all: `fill_vec` takes a quarter of a second a megapixel); the thin pages have two corners
_LARGE_PICK = {
    (1, 8192): ("all", "random0.5", "one_known_0_0", "one_known_0_8191", "islands"),
    (8192, 1): ("none", "random0.5", "one_known_0_0", "one_known_8191_0", "islands"),
    (65, 8129): ("random0.5", "one_known_0_0", "one_known_0_8128", "one_known_64_0", "one_known_64_8128", "islands", "big", "seams"),
    (1024, 1024): ("random0.5", "one_known_0_0", "one_known_1023_1023", "islands", "big", "seams"),
    (1025, 1025): ("all", "none", "random0.5", "one_known_0_0", "one_known_0_1024", "one_known_1024_0", "one_known_1024_1024",
                   "islands", "big", "seams"),
    (1100, 1300): ("none", "random0.5", "one_known_0_1299", "one_known_1099_0", "islands", "big", "seams"),
}


def known_plane(R, l):
    """k of level l after the pull, from the hole mask alone: a level pixel is known where any child is."""
    k = R == 0
    for _ in range(l):
        h, w = k.shape
        kp = np.zeros((2 * ((h + 1) // 2), 2 * ((w + 1) // 2)), bool)
        kp[:h, :w] = k
        k = kp.reshape(kp.shape[0] // 2, 2, kp.shape[1] // 2, 2).any(axis=(1, 3))
    return k


def _tile_span(n, t0, t1):
    """Pixels of the whole tiles t0 .. t1 - 1 of an axis of n pixels, or the whole axis where it has too few tiles."""
    return (t0 * TILE, t1 * TILE) if _dim(n, 6) >= t1 + 2 else (0, n)


def large_holes_of(H, W, rng):
    """{name: R} for one of LARGE_SIZES, every pattern the size allows."""
    out = {"all": np.full((H, W), 255, np.uint8), "none": np.zeros((H, W), np.uint8)}
    out["random0.5"] = ((rng.random((H, W)) < 0.5) * rng.integers(1, 256, (H, W))).astype(np.uint8)
    for cy, cx in dict.fromkeys(((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1))):
        R = np.full((H, W), 1, np.uint8)
        R[cy, cx] = 0
        out[f"one_known_{cy}_{cx}"] = R
    R = np.full((H, W), 7, np.uint8)                                 # all hole but a few dozen single known pixels
    R[rng.integers(0, H, 40), rng.integers(0, W, 40)] = 0
    out["islands"] = R
    R = np.zeros((H, W), np.uint8)                                   # whole aligned tiles: tile rows 2 .. 7, tile columns 4 .. 9,
    (ya, yb), (xa, xb) = _tile_span(H, 2, 8), _tile_span(W, 4, 10)   # which hold the aligned 4 x 4 tiles (4 .. 7, 4 .. 7)
    R[ya:yb, xa:xb] = 255
    R[max(H - 130, 0):, max(W - 200, 0):] = 255                      # and one flush with the bottom-right corner
    out["big"] = R
    R = np.zeros((H, W), np.uint8)                                   # thin bars astride every fourth tile seam
    for x in range(256, W, 256):
        R[min(10, H - 1):max(H - 10, 1), x - 2:x + 3] = 255
    for y in (range(256, H, 256) if H > 256 else range(64, H, 64)):
        R[y - 1:y + 2, 5:max(W - 5, 6)] = 200
    out["seams"] = R
    return out


def large_material():
    """[(name, page, hole mask)] at LARGE_SIZES; pages of noise, the ramp page and a flat colour in turn, the ramp page under
    the big holes.  Made once, read-only."""
    if "l" not in _MATERIAL:
        rng = np.random.default_rng(1419)
        out = []
        for H, W in LARGE_SIZES:
            holes = large_holes_of(H, W, rng)
            for i, name in enumerate(_LARGE_PICK[(H, W)]):
                kind = 1 if name == "big" else i % 3
                page = (rng.integers(0, 256, (H, W, 3), dtype=np.uint8), ramp_page(H, W),
                        np.full((H, W, 3), (17, 250, 133), np.uint8))[kind]
                page.setflags(write=False)
                holes[name].setflags(write=False)
                out.append((f"{H}x{W}-{name}-{('noise', 'ramp', 'flat')[kind]}", page, holes[name]))
        _MATERIAL["l"] = out
    return _MATERIAL["l"]


def large_reference():
    """[(out, row)] of `fill_vec` on `large_material()`: computed once, shared, never changed."""
    if "l" not in _REFERENCE:
        res = [fill_vec(p, r) for _, p, r in large_material()]
        for o, _ in res:
            o.setflags(write=False)
        _REFERENCE["l"] = res
    return _REFERENCE["l"]


# ---- 6. pages that are constant on aligned 2^s x 2^s blocks: the rule scales -----------------------------------------------------

def repeat_blocks(A, s):
    """Every pixel of A as a 2^s x 2^s block."""
    return np.repeat(np.repeat(A, 1 << s, axis=0), 1 << s, axis=1)


def _push_window(fin, c, k):
    """`push_level` on a WINDOW of the levels: `fin` the finished level l + 1 over some rows and columns, (c, k) level l as
    pulled over twice as many from twice the origin.  ny and nx are clamped to the window: at an edge of the level that is the
    rule's clamp, elsewhere it makes the window's outermost rows and columns wrong (see `fill_blocks`)."""
    n_r, n_c = fin.shape[:2]
    py, ny = _neighbours(2 * n_r, n_r)
    px, nx = _neighbours(2 * n_c, n_c)
    v = (9 * fin[py][:, px] + 3 * fin[py][:, nx] + 3 * fin[ny][:, px] + fin[ny][:, nx] + 8) >> 4
    return np.where(k[:, :, None], c, v)


def fill_blocks(Q, M, s, win=8):
    """(out, row) of `fill_vec(repeat_blocks(Q, s), repeat_blocks(M, s))` without a full-size plane.  Levels 1 .. s of the pull
    are the coarser repeats of Q (a mean of equal known values is that value) and level s is (Q, M == 0), so the row is
    `fill_vec(Q, M)`'s with 4^s times the holes and s more levels, and the finished level s is `fill_vec(Q, M)`'s output; the
    levels s - 1 .. 0 are plain pushes from it.  These run on windows of Q around the hole blocks (runs of `win` x `win`
    blocks that hold one) widened by ONE block: a level-l pixel needs its parent and the parent's neighbour, so of a window
    whose level-(l + 1) rows from r on are right the level-l rows from 2 r - 1 on are right, and 2 (2^j y0 - 1) - 1 stays
    below 2^(j + 1) y0: what the window's clamp spoils never reaches the rows and columns that are kept."""
    f = 1 << s
    H, W = M.shape
    o, r = fill_vec(Q, M)
    out = repeat_blocks(Q, s)
    row = dict(r, n_hole=r["n_hole"] * f * f, levels=r["levels"] + s)
    if row["status"] != OK or s == 0:
        return (out if s else o), row
    known = M == 0
    gh, gw = (H + win - 1) // win, (W + win - 1) // win
    pad = np.zeros((gh * win, gw * win), bool)
    pad[:H, :W] = ~known
    grid = pad.reshape(gh, win, gw, win).any(axis=(1, 3))
    for i in range(gh):
        edges = np.flatnonzero(np.diff(np.concatenate(([0], grid[i].astype(np.int8), [0]))))
        for j0, j1 in zip(edges[::2], edges[1::2]):                  # a run of windows with a hole block
            y0, y1, x0, x1 = win * i, min(win * (i + 1), H), win * int(j0), min(win * int(j1), W)
            a0, a1, b0, b1 = max(y0 - 1, 0), min(y1 + 1, H), max(x0 - 1, 0), min(x1 + 1, W)
            fin = o[a0:a1, b0:b1].astype(np.int32)
            for l in range(s - 1, -1, -1):
                fin = _push_window(fin, repeat_blocks(Q[a0:a1, b0:b1], s - l).astype(np.int32), repeat_blocks(known[a0:a1, b0:b1], s - l))
            out[f * y0:f * y1, f * x0:f * x1] = fin[f * (y0 - a0):f * (y1 - a0), f * (x0 - b0):f * (x1 - b0)]
    return out, row


def block_mask(n, rng):
    """The hole blocks of the capacity page, n x n (n = 1024 for the page of 8192 x 8192 at s = 3; a smaller n has the same
    parts in proportion): a large hole at an offset that is no multiple of 8 blocks, so that it covers whole tiles and cuts
    others; a square hole flush with each corner; a bar one block wide along the whole right and bottom edge; scattered single
    hole blocks."""
    M = np.zeros((n, n), np.uint8)
    y, x, h, w, c = 301 * n // 1024, 227 * n // 1024, 160 * n // 1024, 200 * n // 1024, 24 * n // 1024
    M[y:y + h, x:x + w] = 255
    for ys in (slice(0, c), slice(n - c, n)):
        for xs in (slice(0, c), slice(n - c, n)):
            M[ys, xs] = 9
    M[:, n - 1] = 1
    M[n - 1, :] = 128
    k = max(300 * n * n // (1024 * 1024), 4)
    M[rng.integers(0, n, k), rng.integers(0, n, k)] = 77
    return M


def capacity_blocks(deep=False):
    """(Q, M, s) of the capacity page, 8192 x 8192 = `repeat_blocks` of 1024 x 1024 noise and `block_mask(1024)` at s = 3: every
    64 x 64 tile holds 64 block colours.  Noise averages out, though: from level 10 on every pixel of that page is known and
    127 or 128, so a wrong layout of the top levels would go unseen.  `deep` is its companion: a ramp under weak noise, whose
    means differ from place to place, and aligned square holes of 4096, 2048 and 1024 pixels, so that levels 6 .. 12 all have
    unknown pixels and a quarter of the page hangs on the top level alone.  Made once, read-only."""
    key = "d" if deep else "c"
    if key not in _MATERIAL:
        rng = np.random.default_rng(8192 + deep)
        if deep:
            Q = (ramp_page(1024, 1024).astype(np.int64) * 7 // 8 + rng.integers(0, 32, (1024, 1024, 3))).astype(np.uint8)
            M = np.zeros((1024, 1024), np.uint8)
            M[512:, :512] = 255                                      # a pixel of level 12
            M[:256, 512:768] = 2                                     # of level 11
            M[384:512, 128:256] = 1                                  # of level 10
            M[rng.integers(0, 1024, 300), rng.integers(0, 1024, 300)] = 77
        else:
            Q, M = rng.integers(0, 256, (1024, 1024, 3), dtype=np.uint8), block_mask(1024, rng)
        Q.setflags(write=False)
        M.setflags(write=False)
        _MATERIAL[key] = (Q, M, 3)
    return _MATERIAL[key]
