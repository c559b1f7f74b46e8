"""The pull-push fill rule of include/ctd_hip.h (`ctd_fill_rest`) restated in numpy, three times:

  fill_loops   plain Python loops, pixel by pixel, straight from the rule's text;
  fill_vec     whole levels at a time;
  fill_emul    tile-wise, as csrc/kernels_fill.hip runs it: a pull of levels 1 .. 6 per aligned 64 x 64 tile, one block per page
               for the levels above 6 and the push down to level 6, a push per tile from levels 1 .. 6 loaded with a halo of
               one pixel at coordinates clamped to the level.

All three return (out, row): `out` (H,W,3) u8 and `row` = {status, n_hole, levels, top}.  Integers only, so every comparison
with them is exact.  `material()` is the pages the tests of the rule and of the kernels share."""
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
