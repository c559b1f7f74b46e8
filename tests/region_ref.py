"""numpy restatement of the reference's `TextBlock.get_transformed_region` (utils/textblock.py:162-194) -- test
infrastructure, no GPU, nothing of the product in it.

PARITY UNPINNED: no cv2 can run here, so its two primitives are written from the published algorithm:
  * `cv2.findHomography(src, dst, RANSAC, 5.0)` on exactly four points skips RANSAC and the refinement and returns the
    unique homography through the four correspondences, normalised to h22 = 1 -- here `np.linalg.solve` of the 8x8 system;
  * `cv2.warpPerspective(img, M, (w, h))` with the defaults INTER_LINEAR / BORDER_CONSTANT 0, the classic fixed-point path
    of OpenCV 4.1.2 - 4.10 (imgproc/imgwarp.cpp): Minv (here `np.linalg.inv`), per output pixel in double
        W = Minv[6] x + Minv[7] y + Minv[8];  W = W ? 32 / W : 0
        X = rint(clamp((Minv[0] x + Minv[1] y + Minv[2]) W, INT_MIN, INT_MAX)),  Y likewise          (1/32 px)
    taps (X >> 5, Y >> 5) + {0,1}^2 with weights 32 (32 - ax)(32 - ay), 32 ax (32 - ay), 32 (32 - ax) ay, 32 ax ay of
    ax = X & 31, ay = Y & 31, taps outside the image read 0, dst = (sum + 16384) >> 15.  The dot products are taken as
    (M0 x + M1 y) + M2 on the full column index (OpenCV forms them per 32-column block; the two differ in the last bit of
    a double, which matters only where fX / fY is a rounding tie);
  * `cv2.rotate(region, ROTATE_90_COUNTERCLOCKWISE)`: out[i][j] = region[j][w - 1 - i].

TIE BAND: a pixel whose fX or fY lies within `BAND` = 1e-6 (1/32-px units) of a rounding boundary (k + 1/2) may round
either way under another float64 route to the same homography (8x8 solve + adjugate against normalised DLT + inverse
disagree by <= 3.1e-10 of such a unit over 600 quads with page coordinates up to 4500: the band is 3000 times that).
`warp_candidates` returns, besides the warp itself, the band and every candidate value of its pixels: the tied
coordinates rounded down and up.
"""
from __future__ import annotations

import numpy as np

BAND = 1e-6
RESIDUAL_MAX = 1e-4      # px: a solved homography must map the quad onto the crop's corners this well (well-posed: ~1e-9)
INT_MIN, INT_MAX = -2147483648.0, 2147483647.0


def line_quad(quad, language: str, vertical: bool, font_size, im_w: int, im_h: int) -> np.ndarray:
    """Step 1, the margin of English / unknown-horizontal lines (textblock.py:165-172): (4,2) float64."""
    src = np.array(quad, dtype=np.float64).reshape(4, 2)
    if language == "eng" or (language == "unknown" and not vertical):
        e = font_size / 3
        src[..., 0] += np.array([-e, e, e, -e])
        src[..., 1] += np.array([-e, -e, e, e])
        src[..., 0] = np.clip(src[..., 0], 0, im_w)
        src[..., 1] = np.clip(src[..., 1], 0, im_h)
    return src


def _norm(v) -> float:
    return float(np.sqrt(v[0] * v[0] + v[1] * v[1]))          # unfused sqrt(x*x + y*y)


def region_size(src: np.ndarray, vertical: bool, textheight):
    """Steps 2 and 3 (textblock.py:174-187): (w, h) of the warp.  Raises like the reference where it would (int(round(nan)),
    int(round(inf)))."""
    mid = (src[[1, 2, 3, 0]] + src) / 2
    vec_v = mid[2] - mid[0]
    vec_h = mid[1] - mid[3]
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.float64(_norm(vec_v)) / np.float64(_norm(vec_h))
        if not vertical:
            h = int(textheight)
            w = int(round(float(textheight / ratio)))
        else:
            w = int(textheight)
            h = int(round(float(textheight * ratio)))
    return w, h


def homography(src: np.ndarray, w: int, h: int) -> np.ndarray:
    """Step 4: the homography through src[i] -> [[0,0],[w-1,0],[w-1,h-1],[0,h-1]][i] with h22 = 1."""
    dst = np.array([[0, 0], [w - 1, 0], [w - 1, h - 1], [0, h - 1]]).astype(np.float32).astype(np.float64)
    A, b = [], []
    for (x, y), (u, v) in zip(src, dst):
        A.append([x, y, 1, 0, 0, 0, -u * x, -u * y])
        b.append(u)
        A.append([0, 0, 0, x, y, 1, -v * x, -v * y])
        b.append(v)
    hh = np.linalg.solve(np.array(A, np.float64), np.array(b, np.float64))
    return np.append(hh, 1.0).reshape(3, 3)


def transform(quad, language: str, vertical: bool, font_size, im_w: int, im_h: int, textheight):
    """Steps 1-4 + Minv: (w, h, M, Minv).  ValueError for a degenerate line (the reference raises from inside cv2 or from
    int(round(nan))): w < 1, h < 1, a non-finite ratio, a singular system."""
    src = line_quad(quad, language, vertical, font_size, im_w, im_h)
    try:
        w, h = region_size(src, vertical, textheight)
    except (ValueError, OverflowError) as e:
        raise ValueError(f"degenerate line: {e}")
    if w < 1 or h < 1:
        raise ValueError("degenerate line: empty region")
    try:
        M = homography(src, w, h)
        Minv = np.linalg.inv(M)
    except np.linalg.LinAlgError as e:
        raise ValueError(f"degenerate line: {e}")
    if not (np.isfinite(M).all() and np.isfinite(Minv).all()):
        raise ValueError("degenerate line: non-finite homography")
    # collinear points have no homography onto a rectangle, but LAPACK may still return a finite "solution" of the singular
    # system: what was solved must map the four points onto the corners
    with np.errstate(divide="ignore", invalid="ignore"):
        p = np.c_[src, np.ones(4)] @ M.T
        got = p[:, :2] / p[:, 2:]
    want = np.array([[0, 0], [w - 1, 0], [w - 1, h - 1], [0, h - 1]], np.float64)
    if not (np.abs(got - want) <= RESIDUAL_MAX).all():
        raise ValueError("degenerate line: singular system")
    return w, h, M, Minv


def source_coords(Minv: np.ndarray, w: int, h: int):
    """fX, fY (h,w) float64: where output pixel (x, y) reads the image, in 1/32-px units, before rounding."""
    m = np.asarray(Minv, np.float64).reshape(9)
    x = np.arange(w, dtype=np.float64)[None, :]
    y = np.arange(h, dtype=np.float64)[:, None]
    W = (m[6] * x + m[7] * y) + m[8]
    with np.errstate(divide="ignore", invalid="ignore"):
        W = np.where(W != 0, 32.0 / W, 0.0)
        fX = np.fmax(INT_MIN, np.fmin(INT_MAX, ((m[0] * x + m[1] * y) + m[2]) * W))
        fY = np.fmax(INT_MIN, np.fmin(INT_MAX, ((m[3] * x + m[4] * y) + m[5]) * W))
    return fX, fY


def _sample(img: np.ndarray, X: np.ndarray, Y: np.ndarray) -> np.ndarray:
    """The fixed-point bilinear taps at integer 1/32-px coordinates X, Y (int64 arrays of one shape)."""
    im = img if img.ndim == 3 else img[:, :, None]
    H, Wd = im.shape[:2]
    sx, sy, ax, ay = X >> 5, Y >> 5, X & 31, Y & 31
    acc = np.zeros(X.shape + (im.shape[2],), np.int64)
    for dy, dx, wt in ((0, 0, 32 * (32 - ax) * (32 - ay)), (0, 1, 32 * ax * (32 - ay)), (1, 0, 32 * (32 - ax) * ay),
                       (1, 1, 32 * ax * ay)):
        yy, xx = sy + dy, sx + dx
        inside = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < Wd)
        px = im[np.clip(yy, 0, H - 1), np.clip(xx, 0, Wd - 1)].astype(np.int64)
        acc += np.where(inside[..., None], px, 0) * wt[..., None]
    out = ((acc + 16384) >> 15).astype(np.uint8)
    return out if img.ndim == 3 else out[:, :, 0]


def _rot(a: np.ndarray, rotate: bool) -> np.ndarray:
    return np.rot90(a, 1) if rotate else a                # counter-clockwise: out[i][j] = a[j][w - 1 - i]


def warp_candidates(img: np.ndarray, Minv: np.ndarray, w: int, h: int, rotate: bool = False):
    """Steps 5 and 6 with the tie band: (region, band, candidates, (fX, fY)).  region: the warp (rotated if asked); band:
    bool mask of the region's pixels whose fX or fY is within BAND of a rounding boundary; candidates: the four warps with
    the tied coordinates rounded (down, down), (up, down), (down, up), (up, up) -- outside the band all equal `region`."""
    fX, fY = source_coords(Minv, w, h)
    tx = np.abs(fX - np.floor(fX) - 0.5) < BAND
    ty = np.abs(fY - np.floor(fY) - 0.5) < BAND
    X, Y = np.rint(fX).astype(np.int64), np.rint(fY).astype(np.int64)
    region = _sample(img, X, Y)
    cands = []
    for uy in (0, 1):
        for ux in (0, 1):
            Xc = np.where(tx, np.floor(fX).astype(np.int64) + ux, X)
            Yc = np.where(ty, np.floor(fY).astype(np.int64) + uy, Y)
            cands.append(_rot(_sample(img, Xc, Yc), rotate))
    return _rot(region, rotate), _rot(tx | ty, rotate), cands, (fX, fY)


def warp(img: np.ndarray, Minv: np.ndarray, w: int, h: int, rotate: bool = False) -> np.ndarray:
    """cv2.warpPerspective(img, inv(Minv), (w, h)) [+ cv2.rotate(.., ROTATE_90_COUNTERCLOCKWISE)]."""
    fX, fY = source_coords(Minv, w, h)
    return np.ascontiguousarray(_rot(_sample(img, np.rint(fX).astype(np.int64), np.rint(fY).astype(np.int64)), rotate))


def get_transformed_region(img: np.ndarray, quad, language: str, vertical: bool, font_size, textheight):
    """The whole method for one line: (region, band, candidates)."""
    im_h, im_w = img.shape[:2]
    w, h, _, Minv = transform(quad, language, vertical, font_size, im_w, im_h, textheight)
    region, band, cands, _ = warp_candidates(img, Minv, w, h, rotate=bool(vertical))
    return region, band, cands
