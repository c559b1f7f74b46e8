"""The raster rule of include/ctd_hip.h ("glyph outlines rasterised into the atlas") restated in numpy int64: transform, box,
flatten, coverage.  A loop over edges, vectorised over sample rows; `A_k(px)` is evaluated as the rule writes it, a clamp per
pixel, not through delta cells and a prefix sum as the kernel does it.  Plus hand-made shapes and a seeded generator of closed
random outlines with lines and curves mixed.  No GPU, no package import."""
import numpy as np

MAX_SIDE, MAX_SCALE = 1024, 1 << 22
OK, EMPTY, REFUSED = 0, 1, 2


def scale_of(size, upem):
    return int(round(float(size) * 65536 / upem))


def transform(segs, S):
    """(n, 3, 2) int64: the 26.6 points (X, Y) of every segment, y down."""
    sg = np.asarray(segs, np.int64).reshape(-1, 3, 2)
    return np.stack([(sg[..., 0] * S + 512) >> 10, (-sg[..., 1] * S + 512) >> 10], axis=-1)


def box(segs, S):
    """(bx, by, w, h) from ALL transformed points; no segments: zeros."""
    if len(segs) == 0:
        return 0, 0, 0, 0
    P = transform(segs, S)
    X, Y = P[..., 0], P[..., 1]
    bx, by = int(X.min()) >> 6, int(Y.min()) >> 6
    return bx, by, -((-int(X.max())) >> 6) - bx, -((-int(Y.max())) >> 6) - by


def level(P):
    """The flatten level of a curve with 26.6 points P (3, 2)."""
    dd = int(np.abs(P[0] - 2 * P[1] + P[2]).max())
    for lv in range(6):
        if (dd >> (2 * lv)) <= 16:
            return lv
    return 5


def flatten(segs, S):
    """The edges (X0, Y0, X1, Y1) in 26.6, in the segments' order and direction: an (m, 4) int64 array."""
    raw = np.asarray(segs, np.int64).reshape(-1, 3, 2)
    out = []
    for r, P in zip(raw, transform(segs, S)):
        if (r[1] == r[0]).all() or (r[1] == r[2]).all():
            out.append((P[0, 0], P[0, 1], P[2, 0], P[2, 1]))
            continue
        lv = level(P)
        N = 1 << lv
        k = np.arange(N + 1, dtype=np.int64)[:, None]
        Q = ((N - k) ** 2 * P[0] + 2 * k * (N - k) * P[1] + k * k * P[2] + ((N * N) >> 1)) >> (2 * lv)
        out += [(Q[i, 0], Q[i, 1], Q[i + 1, 0], Q[i + 1, 1]) for i in range(N)]
    return np.array(out, np.int64).reshape(-1, 4)


def coverage(edges, bx, by, w, h, rows_a_block=64):
    """The (h, w) uint8 coverage of flattened edges in the box: the rule's A_k and byte, a block of pixel rows at a time."""
    out = np.zeros((h, w), np.uint8)
    if w == 0 or h == 0:
        return out
    right = 256 * (np.arange(w, dtype=np.int64) + 1)
    for p0 in range(0, h, rows_a_block):
        p1 = min(h, p0 + rows_a_block)
        Ys = 64 * by + 4 * np.arange(16 * p0, 16 * p1, dtype=np.int64) + 2    # 64 (by + py) + 4 k + 2
        A = np.zeros((len(Ys), w), np.int64)
        for X0, Y0, X1, Y1 in edges.tolist():
            if Y0 == Y1:
                continue
            d = 1 if Y0 < Y1 else -1
            (lx, ly), (hx, hy) = ((X0, Y0), (X1, Y1)) if d > 0 else ((X1, Y1), (X0, Y0))
            at = np.flatnonzero((ly <= Ys) & (Ys < hy))
            if len(at) == 0:
                continue
            ys = Ys[at]
            Xc = (4 * (lx * (hy - ys) + hx * (ys - ly))) // (hy - ly) - 256 * bx
            assert Xc.min() >= 0 and Xc.max() <= 256 * w
            A[at] += d * np.clip(right[None, :] - Xc[:, None], 0, 256)
        s = np.minimum(np.abs(A), 256).reshape(p1 - p0, 16, w).sum(axis=1)
        out[p0:p1] = (255 * s + 2048) >> 12
    return out


def rasterise(segs, S):
    """(coverage (h, w) uint8, bx, by) of an outline at scale S."""
    segs = np.asarray(segs, np.int64).reshape(-1, 6)
    assert 0 < S <= MAX_SCALE and (len(segs) == 0 or np.abs(segs).max() <= 1 << 15)
    bx, by, w, h = box(segs, S)
    assert w <= MAX_SIDE and h <= MAX_SIDE
    return coverage(flatten(segs, S), bx, by, w, h), bx, by


# ---- shapes -----------------------------------------------------------------------------------------------------------------

def line(a, b):
    return (a[0], a[1], a[0], a[1], b[0], b[1])


def polygon(pts):
    """A closed contour of straight lines through pts, in their order."""
    pts = [tuple(int(v) for v in p) for p in pts]
    return np.array([line(a, b) for a, b in zip(pts, pts[1:] + pts[:1])], np.int32).reshape(-1, 6)


def rect(x1, y1, x2, y2, cw=False):
    """The rectangle x1 .. x2, y1 .. y2 (font units, y up), counter-clockwise, or clockwise."""
    pts = [(x1, y1), (x2, y1), (x2, y2), (x1, y2)]
    return polygon(pts[::-1] if cw else pts)


def blob(n=8, radius=400, centre=(500, 500), cw=False):
    """A closed contour of n curves around a centre: on-curve points on a circle, controls outside it (a round shape)."""
    a = np.arange(n) * 2 * np.pi / n * (-1 if cw else 1)
    on = np.stack([centre[0] + radius * np.cos(a), centre[1] + radius * np.sin(a)], 1).round().astype(np.int64)
    am = a + (np.pi / n) * (-1 if cw else 1)
    off = np.stack([centre[0] + radius / np.cos(np.pi / n) * np.cos(am), centre[1] + radius / np.cos(np.pi / n) * np.sin(am)],
                   1).round().astype(np.int64)
    return np.array([(*on[i], *off[i], *on[(i + 1) % n]) for i in range(n)], np.int32).reshape(-1, 6)


def random_outline(rng, upem=1000, contours=None, points=None):
    """A seeded outline of closed contours, lines and curves mixed: each contour runs once around a centre through points at
    random radii, either orientation; about half of its segments are curves with a control point off the chord."""
    segs = []
    for _ in range(int(rng.integers(1, 4)) if contours is None else contours):
        n = int(rng.integers(3, 10)) if points is None else points
        c = rng.integers(upem // 4, 3 * upem // 4, 2)
        ang = np.sort(rng.random(n) * 2 * np.pi)
        if rng.random() < 0.5:
            ang = ang[::-1]
        rad = rng.integers(upem // 16, upem // 3, n)
        pts = np.stack([c[0] + rad * np.cos(ang), c[1] + rad * np.sin(ang)], 1).round().astype(np.int64)
        for i in range(n):
            a, b = pts[i], pts[(i + 1) % n]
            if rng.random() < 0.5:
                segs.append((*a, *a, *b))
            else:
                ctl = (a + b) // 2 + rng.integers(-upem // 6, upem // 6 + 1, 2)
                segs.append((*a, *ctl, *b))
    return np.array(segs, np.int32).reshape(-1, 6)


def arch(c=100):
    """One closed contour: the curve (0, 0) (c, 2 c) (2 c, 0) and the chord back.  Its dd is about 4 c S / 1024."""
    return np.array([(0, 0, c, 2 * c, 2 * c, 0), line((2 * c, 0), (0, 0))], np.int32)


# the scale at which `arch()`'s curve flattens at level 0 .. 5 (dd about 15, 62, 250, 1000, 4000, 25600)
ARCH_SCALE_OF_LEVEL = (40, 160, 640, 2560, 10240, 65536)
