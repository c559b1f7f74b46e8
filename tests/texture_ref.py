"""The texture fill rule of include/ctd_hip.h (`ctd_texture_fill`) restated in numpy, twice:

  texture_loops   plain Python loops, one target at a time, straight from the rule's text (small pages);
  texture_vec     vectorised over the targets.

Both return (out, row): `out` (H,W,3) u8 and `row` = {status, n_hole, n_target, n_source, n_unmatched}.  Integers only, so
every comparison with them is exact.  `material()` is the pages the tests of the kernels use, `reference()` the rule on them
(pull-push `init`, default parameters), made once; `quality_cases()` the six screentone pages of DESIGN.md section 4.30."""
import numpy as np

import fill_ref

OK, NO_HOLE, NO_SOURCE = range(3)
PATCH, PR, MAX_RADIUS = 7, 3, 127
FIELDS = ("status", "n_hole", "n_target", "n_source", "n_unmatched")
DEFAULTS = dict(radius=32, n_em=5, n_sweep=2, n_init=8, seed=0)
PROP_STEPS = (1, 2, 4, 8)
PROP_DIRS = ((0, -1), (0, 1), (-1, 0), (1, 0))                       # (dy, dx) per unit step: left, right, up, down
M32 = 0xFFFFFFFF


def hash32(x, y, s, k, seed):
    """The rule's hash, on Python ints or integer arrays (the result is an int / a uint64 array below 2^32)."""
    if isinstance(x, np.ndarray) or isinstance(y, np.ndarray):
        u = lambda v: np.asarray(v).astype(np.uint64)                # noqa: E731
        m = np.uint64(M32)
        h = (u(x) * np.uint64(0x9E3779B1) + u(y) * np.uint64(0x85EBCA77) + np.uint64((s * 0xC2B2AE3D + k * 0x27D4EB2F + seed) & M32)) & m
        h ^= h >> np.uint64(16)
        h = (h * np.uint64(0x7FEB352D)) & m
        h ^= h >> np.uint64(15)
        h = (h * np.uint64(0x846CA68B)) & m
        h ^= h >> np.uint64(16)
        return h
    h = (x * 0x9E3779B1 + y * 0x85EBCA77 + s * 0xC2B2AE3D + k * 0x27D4EB2F + seed) & M32
    h ^= h >> 16
    h = (h * 0x7FEB352D) & M32
    h ^= h >> 15
    h = (h * 0x846CA68B) & M32
    h ^= h >> 16
    return h


def draw(x, y, s, k, seed, rho):
    """Draw k of radius rho for the target (x, y) in sweep s: -rho .. rho."""
    h = hash32(x, y, s, k, seed)
    if isinstance(h, np.ndarray):
        return (h % np.uint64(2 * rho + 1)).astype(np.int64) - rho
    return h % (2 * rho + 1) - rho


def radii(R):
    """R, R >> 1, .., 1."""
    out = []
    while R >= 1:
        out.append(R)
        R >>= 1
    return out


def classes(hole):
    """(target, valid) planes of a bool hole plane: a target's 7 x 7 patch (clipped to the page) holds a hole pixel; a valid
    centre's patch lies inside the page and holds none."""
    H, W = hole.shape
    pad = np.zeros((H + 2 * PR, W + 2 * PR), bool)
    pad[PR:PR + H, PR:PR + W] = hole
    anyh = np.zeros((H, W), bool)
    for oy in range(PATCH):
        for ox in range(PATCH):
            anyh |= pad[oy:oy + H, ox:ox + W]
    inner = np.zeros((H, W), bool)
    if H >= PATCH and W >= PATCH:
        inner[PR:H - PR, PR:W - PR] = True
    return anyh, inner & ~anyh


def _check(P, M, init, radius, n_em, n_sweep, n_init):
    assert P.dtype == np.uint8 and P.ndim == 3 and P.shape[2] == 3 and M.shape == P.shape[:2] and init.shape == P.shape
    assert 1 <= radius <= MAX_RADIUS and 1 <= n_em <= 16 and 1 <= n_sweep <= 8 and 1 <= n_init <= 16


def _row(n_hole, n_target, n_source, n_unmatched):
    status = NO_HOLE if n_hole == 0 else NO_SOURCE if n_source == 0 else OK
    return {"status": status, "n_hole": int(n_hole), "n_target": int(n_target), "n_source": int(n_source),
            "n_unmatched": int(n_unmatched)}


def row_dict(rec):
    """A `texture.ROW_DTYPE` record as the dict the restatements return."""
    return {f: int(rec[f]) for f in FIELDS}


# ---- 1. plain loops ------------------------------------------------------------------------------------------------------------

def texture_loops(P, M, init, radius=32, n_em=5, n_sweep=2, n_init=8, seed=0):
    _check(P, M, init, radius, n_em, n_sweep, n_init)
    H, W = M.shape
    R = radius
    hole = [[bool(M[y, x] != 0) for x in range(W)] for y in range(H)]
    C = [[[int(v) for v in (init[y, x] if hole[y][x] else P[y, x])] for x in range(W)] for y in range(H)]
    offs = [(oy, ox) for oy in range(-PR, PR + 1) for ox in range(-PR, PR + 1)]
    valid = [[False] * W for _ in range(H)]
    target = [[False] * W for _ in range(H)]
    for y in range(H):
        for x in range(W):
            inside, anyh = True, False
            for oy, ox in offs:
                yy, xx = y + oy, x + ox
                if 0 <= yy < H and 0 <= xx < W:
                    anyh = anyh or hole[yy][xx]
                else:
                    inside = False
            target[y][x] = anyh
            valid[y][x] = inside and not anyh
    targets = [(y, x) for y in range(H) for x in range(W) if target[y][x]]
    field = {t: (0, 0, 0) for t in targets}                          # (dy, dx, ok)

    def cost(y, x, dy, dx):
        c = 0
        for oy, ox in offs:
            a = C[min(max(y + oy, 0), H - 1)][min(max(x + ox, 0), W - 1)]
            b = C[y + dy + oy][x + dx + ox]
            c += (a[0] - b[0]) ** 2 + (a[1] - b[1]) ** 2 + (a[2] - b[2]) ** 2
        return c

    def admissible(y, x, dy, dx):
        return abs(dy) <= R and abs(dx) <= R and 0 <= y + dy < H and 0 <= x + dx < W and valid[y + dy][x + dx]

    def sweep(s, initial):
        new = {}
        for (y, x) in targets:
            dy, dx, ok = field[(y, x)]
            best = (dy, dx, cost(y, x, dy, dx)) if ok else None

            def consider(cy, cx, best):
                if not admissible(y, x, cy, cx):
                    return best
                c = cost(y, x, cy, cx)
                return (cy, cx, c) if best is None or c < best[2] else best

            if initial:
                for j in range(n_init):
                    best = consider(draw(x, y, s, 2 * j, seed, R), draw(x, y, s, 2 * j + 1, seed, R), best)
            else:
                for d in PROP_STEPS:
                    for uy, ux in PROP_DIRS:
                        ny, nx = y + d * uy, x + d * ux
                        if 0 <= ny < H and 0 <= nx < W and target[ny][nx] and field[(ny, nx)][2]:
                            best = consider(field[(ny, nx)][0], field[(ny, nx)][1], best)
                for j, rho in enumerate(radii(R)):
                    cy, cx = (best[0], best[1]) if best else (0, 0)
                    best = consider(cy + draw(x, y, s, 2 * j, seed, rho), cx + draw(x, y, s, 2 * j + 1, seed, rho), best)
            new[(y, x)] = (best[0], best[1], 1) if best else (0, 0, 0)
        return new

    def vote():
        for y in range(H):
            for x in range(W):
                if not hole[y][x]:
                    continue
                n, S = 0, [0, 0, 0]
                for oy, ox in offs:
                    ty, tx = y - oy, x - ox
                    if 0 <= ty < H and 0 <= tx < W and target[ty][tx] and field[(ty, tx)][2]:
                        v = C[ty + field[(ty, tx)][0] + oy][tx + field[(ty, tx)][1] + ox]
                        n += 1
                        for ch in range(3):
                            S[ch] += v[ch]
                if n:
                    C[y][x] = [(2 * v + n) // (2 * n) for v in S]

    s = 0
    for em in range(n_em):
        for _ in range(n_sweep + (em == 0)):
            field = sweep(s, s == 0)
            s += 1
        vote()
    out = np.array(C, np.uint8).reshape(H, W, 3)
    n_hole = sum(v for r in hole for v in r)
    return out, _row(n_hole, len(targets), sum(v for r in valid for v in r), sum(1 for t in targets if not field[t][2]))


# ---- 2. vectorised over the targets --------------------------------------------------------------------------------------------

def texture_vec(P, M, init, radius=32, n_em=5, n_sweep=2, n_init=8, seed=0):
    _check(P, M, init, radius, n_em, n_sweep, n_init)
    H, W = M.shape
    R = radius
    hole = M != 0
    target, valid = classes(hole)
    C = np.where(hole[:, :, None], init, P).astype(np.int32)
    ty, tx = np.nonzero(target)
    T = len(ty)
    index = np.full((H, W), -1, np.int64)
    index[ty, tx] = np.arange(T)
    oys, oxs = [a.ravel() for a in np.mgrid[-PR:PR + 1, -PR:PR + 1]]
    # the targets' own patch coordinates, clamped to the page: (T, 49)
    cy = np.clip(ty[:, None] + oys[None, :], 0, H - 1)
    cx = np.clip(tx[:, None] + oxs[None, :], 0, W - 1)
    dy, dx, ok = np.zeros(T, np.int64), np.zeros(T, np.int64), np.zeros(T, bool)

    own_all = None                                                   # C on every target's own patch, (T, 49, 3): made per sweep

    def cost(sel, ddy, ddx):
        c = np.zeros(len(sel), np.int64)
        for a in range(0, len(sel), 4096):                           # chunks keep the (n, 49, 3) temporaries small
            q = sel[a:a + 4096]
            own = own_all[q]
            src = C[(ty[q] + ddy[a:a + 4096])[:, None] + oys[None, :], (tx[q] + ddx[a:a + 4096])[:, None] + oxs[None, :]]
            d = own - src
            c[a:a + 4096] = (d * d).sum(axis=(1, 2))
        return c

    def consider(best, cand_y, cand_x, live=None):
        """The candidates (cand_y, cand_x) of all targets (those of `live`) against best = [dy, dx, cost, ok]."""
        sy, sx = ty + cand_y, tx + cand_x
        adm = (np.abs(cand_y) <= R) & (np.abs(cand_x) <= R) & (sy >= 0) & (sy < H) & (sx >= 0) & (sx < W)
        if live is not None:
            adm &= live
        adm[adm] = valid[sy[adm], sx[adm]]
        sel = np.flatnonzero(adm)
        if not len(sel):
            return
        c = cost(sel, cand_y[sel], cand_x[sel])
        win = ~best[3][sel] | (c < best[2][sel])
        w = sel[win]
        best[0][w], best[1][w], best[2][w], best[3][w] = cand_y[w], cand_x[w], c[win], True

    def sweep(s, initial):
        nonlocal dy, dx, ok, own_all
        own_all = C[cy, cx]
        best = [dy.copy(), dx.copy(), np.zeros(T, np.int64), ok.copy()]
        had = np.flatnonzero(ok)
        best[2][had] = cost(had, dy[had], dx[had])
        if initial:
            for j in range(n_init):
                consider(best, draw(tx, ty, s, 2 * j, seed, R), draw(tx, ty, s, 2 * j + 1, seed, R))
        else:
            for d in PROP_STEPS:
                for uy, ux in PROP_DIRS:
                    ny, nx = ty + d * uy, tx + d * ux
                    inside = (ny >= 0) & (ny < H) & (nx >= 0) & (nx < W)
                    ni = np.where(inside, index[np.clip(ny, 0, H - 1), np.clip(nx, 0, W - 1)], -1)
                    live = (ni >= 0) & ok[np.maximum(ni, 0)]
                    consider(best, dy[np.maximum(ni, 0)], dx[np.maximum(ni, 0)], live)
            for j, rho in enumerate(radii(R)):
                by, bx = np.where(best[3], best[0], 0), np.where(best[3], best[1], 0)
                consider(best, by + draw(tx, ty, s, 2 * j, seed, rho), bx + draw(tx, ty, s, 2 * j + 1, seed, rho))
        ok = best[3]
        dy, dx = np.where(ok, best[0], 0), np.where(ok, best[1], 0)

    hy, hx = np.nonzero(hole)

    def vote():
        S = np.zeros((len(hy), 3), np.int64)
        n = np.zeros(len(hy), np.int64)
        for oy, ox in zip(oys, oxs):
            vy, vx = hy - oy, hx - ox
            inside = (vy >= 0) & (vy < H) & (vx >= 0) & (vx < W)
            ti = np.where(inside, index[np.clip(vy, 0, H - 1), np.clip(vx, 0, W - 1)], -1)
            live = (ti >= 0) & ok[np.maximum(ti, 0)]
            t = ti[live]
            S[live] += C[vy[live] + dy[t] + oy, vx[live] + dx[t] + ox]
            n[live] += 1
        got = n > 0
        C[hy[got], hx[got]] = (2 * S[got] + n[got, None]) // (2 * n[got, None])

    if T and valid.any():                                            # without a valid centre no candidate is admissible
        s = 0
        for em in range(n_em):
            for _ in range(n_sweep + (em == 0)):
                sweep(s, s == 0)
                s += 1
            vote()
    return C.astype(np.uint8), _row(hole.sum(), T, valid.sum(), T - int(ok.sum()))


# ---- 3. the material -----------------------------------------------------------------------------------------------------------

def tone_page(H, W, p):
    """Screentone dots of period p on a slow ramp (the `tone(p)` page of section 4.30 at any size)."""
    y, x = np.mgrid[0:H, 0:W]
    g = np.where((x % p < p // 2) & (y % p < p // 2), 40, 200 - (60 * x) // 128)
    return np.stack([g, g, g], axis=2).astype(np.uint8)


def diag_page(H, W):
    """Diagonal hatching of period 6 (the `diag` page of section 4.30 at any size)."""
    y, x = np.mgrid[0:H, 0:W]
    g = np.where((x + 2 * y) % 6 < 2, 30, 220)
    return np.stack([g, g, np.minimum(g + 20, 255)], axis=2).astype(np.uint8)


def rect_hole(H=96, W=128):
    R = np.zeros((H, W), np.uint8)
    R[30:54, 40:90] = 255
    return R


def strokes_hole(H=96, W=128):
    R = np.zeros((H, W), np.uint8)
    for i in range(6):
        R[20 + 9 * i:24 + 9 * i, 30:100] = 255
        R[20:70, 34 + 12 * i:38 + 12 * i] = 255
    return R


def quality_cases():
    """[(name, page, hole)]: the six cases of the quality condition, 96 x 128."""
    out = []
    for pname, page in (("tone4", tone_page(96, 128, 4)), ("tone6", tone_page(96, 128, 6)), ("diag", diag_page(96, 128))):
        for hname, hole in (("rect", rect_hole()), ("strokes", strokes_hole())):
            out.append((f"{pname}-{hname}", page, hole))
    return out


def hole_error(out, page, hole):
    """The mean of |out - page| over hole pixels and channels."""
    h = hole != 0
    return float(np.abs(out[h].astype(np.int64) - page[h].astype(np.int64)).mean())


def text_holes(H, W):
    """Text-like strokes scaled to the page: thin horizontal and vertical bars in its middle."""
    R = np.zeros((H, W), np.uint8)
    y0, y1, x0, x1 = H // 5, H - H // 4, W // 4, W - W // 5
    for y in range(y0, y1 - 3, 9):
        R[y:y + 3, x0:x1] = 200
    for x in range(x0 + 4, x1 - 3, 12):
        R[y0:y1, x:x + 3] = 255
    return R


def seam_bars(H, W):
    """Bars on the tile seams: rows and columns 63 - 64 of every seam the page has."""
    R = np.zeros((H, W), np.uint8)
    for y in range(64, H, 64):
        R[y - 1:y + 1, 4:W - 4] = 255
    for x in range(64, W, 64):
        R[4:H - 4, x - 1:x + 1] = 7
    return R


def _random(H, W, dens, rng):
    return ((rng.random((H, W)) < dens) * rng.integers(1, 256, (H, W))).astype(np.uint8)


def _corner(H, W, which):
    R = np.zeros((H, W), np.uint8)
    h, w = max(H // 3, 1), max(W // 3, 1)
    R[(slice(0, h), slice(H - h, H))[which >> 1], (slice(0, w), slice(W - w, W))[which & 1]] = 255
    return R


def _page(kind, H, W, rng):
    return {"noise": lambda: rng.integers(0, 256, (H, W, 3), dtype=np.uint8), "ramp": lambda: fill_ref.ramp_page(H, W),
            "flat": lambda: np.full((H, W, 3), (17, 250, 133), np.uint8), "tone": lambda: tone_page(H, W, 4),
            "diag": lambda: diag_page(H, W)}[kind]()


# (H, W, hole pattern, page kind), in the order they are passed: a page without a hole stands between pages with holes
_PLAN = (
    (1, 1, "all", "noise"), (6, 9, "random0.1", "noise"), (7, 8, "pixel_0_7", "ramp"), (7, 7, "none", "noise"),
    (33, 70, "corner3", "tone"), (33, 70, "text", "diag"), (33, 70, "random0.02", "noise"), (33, 70, "all", "flat"),
    (64, 64, "random0.02", "tone"), (64, 64, "none", "diag"), (64, 64, "corner0", "ramp"), (64, 64, "random0.5", "noise"),
    (65, 129, "seams", "tone"), (65, 129, "random0.1", "ramp"), (65, 129, "text", "noise"), (65, 129, "corner1", "flat"),
    (97, 83, "random0.02", "diag"), (97, 83, "corner2", "noise"), (97, 83, "seams", "ramp"),
    (130, 200, "seams", "diag"), (130, 200, "corner3", "ramp"), (130, 200, "random0.1", "noise"),
    (1, 1, "none", "flat"),
)

_MATERIAL, _REFERENCE = {}, {}


def material():
    """[(name, page, hole mask)] of `_PLAN`.  Made once, read-only."""
    if "m" not in _MATERIAL:
        rng = np.random.default_rng(430)
        out = []
        for H, W, pat, kind in _PLAN:
            if pat == "all":
                R = np.full((H, W), 255, np.uint8)
            elif pat == "none":
                R = np.zeros((H, W), np.uint8)
            elif pat.startswith("random"):
                R = _random(H, W, float(pat[6:]), rng)
            elif pat.startswith("corner"):
                R = _corner(H, W, int(pat[6:]))
            elif pat.startswith("pixel"):
                R = np.zeros((H, W), np.uint8)
                R[int(pat.split("_")[1]), int(pat.split("_")[2])] = 1
            else:
                R = {"text": text_holes, "seams": seam_bars}[pat](H, W)
            page = _page(kind, H, W, rng)
            page.setflags(write=False)
            R.setflags(write=False)
            out.append((f"{H}x{W}-{pat}-{kind}", page, R))
        _MATERIAL["m"] = out
    return _MATERIAL["m"]


def pull_push(page, hole):
    """The `init` the public call uses where none is given: the pull-push fill of the same page and mask."""
    return fill_ref.fill_vec(page, hole)[0]


def reference():
    """[(out, row)] of `texture_vec` on `material()` with the pull-push `init` and the default parameters: computed once,
    shared, never changed."""
    if "r" not in _REFERENCE:
        res = [texture_vec(p, r, pull_push(p, r)) for _, p, r in material()]
        for o, _ in res:
            o.setflags(write=False)
        _REFERENCE["r"] = res
    return _REFERENCE["r"]
