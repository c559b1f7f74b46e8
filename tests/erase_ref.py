"""numpy restatement of the erase rule (include/ctd_hip.h, "erase text on plain backgrounds"): per block, is the background next
to its glyphs one colour; per page, the cleaned page and the mask an inpainter still needs.  Written from the rule's statement:
dilation by shifted ORs, `np.bincount`, the two inequalities as written.  The product's kernels (csrc/kernels_erase.hip) are
compared with `erase_page` field by field and byte by byte (tests/test_gpu_erase.py); tests/test_erase_ref.py checks the
rule's own promises here, without a GPU."""
import numpy as np

PLAIN, TEXTURED, NO_RING, NO_MASK, EMPTY, TOO_LARGE = range(6)
MAX_PIXELS, MAX_COORD, MAX_GROW, MAX_RING = 1 << 24, 1 << 29, 8, 16
FIELDS = ("status", "n_fill", "n_ring", "cnt", "med")
DEFAULTS = dict(grow=2, ring=4, tol=12, min_ring=16)


def check_params(grow, ring, tol, min_ring):
    if not (0 <= grow <= MAX_GROW and 1 <= ring <= MAX_RING and 0 <= tol <= 255 and min_ring >= 1):
        raise ValueError("grow 0..8, ring 1..16, tol 0..255, min_ring >= 1")


def dilate(s, k):
    """D_k(S) on a boolean plane the size of the page: the pixels within Chebyshev distance <= k of a pixel of S; rows, then
    columns, each an OR of the plane shifted by -k .. k (what is shifted in from outside the page is empty)."""
    if k == 0:
        return s.copy()
    H, W = s.shape
    rows = s.copy()
    for d in range(1, k + 1):
        rows[:, d:] |= s[:, :W - d] if d < W else False
        rows[:, :max(W - d, 0)] |= s[:, d:]
    out = rows.copy()
    for d in range(1, k + 1):
        out[d:, :] |= rows[:H - d, :] if d < H else False
        out[:max(H - d, 0), :] |= rows[d:, :]
    return out


def _zero_row(status):
    return dict(status=status, n_fill=0, n_ring=0, cnt=[0, 0, 0], med=[0, 0, 0])


def box_status(xyxy, H, W, grow, ring):
    """(status or None, clipped box): what is decided from xyxy, H and W before any pixel is read."""
    x1, y1, x2, y2 = (int(v) for v in xyxy)
    if any(abs(v) > MAX_COORD for v in (x1, y1, x2, y2)):
        return TOO_LARGE, None
    x1, y1, x2, y2 = max(x1, 0), max(y1, 0), min(x2, W), min(y2, H)
    if x1 >= x2 or y1 >= y2:
        return EMPTY, None
    k = grow + ring
    if (x2 - x1 + 2 * k) * (y2 - y1 + 2 * k) > MAX_PIXELS:
        return TOO_LARGE, None
    return None, (x1, y1, x2, y2)


def block_row(page, text, near_text, xyxy, grow, ring, tol, min_ring):
    """(row, F_b or None).  text = M, near_text = D_g(M), both boolean planes of the page."""
    H, W = text.shape
    status, box = box_status(xyxy, H, W, grow, ring)
    if status is not None:
        return _zero_row(status), None
    x1, y1, x2, y2 = box
    # everything of this block lies within g + r of its box: work on that window of the page
    k = grow + ring
    wx1, wy1, wx2, wy2 = max(x1 - k, 0), max(y1 - k, 0), min(x2 + k, W), min(y2 + k, H)
    T = np.zeros((wy2 - wy1, wx2 - wx1), bool)
    T[y1 - wy1:y2 - wy1, x1 - wx1:x2 - wx1] = text[y1:y2, x1:x2]
    F = np.zeros((H, W), bool)
    if not T.any():
        return dict(_zero_row(NO_MASK)), F
    fill = dilate(T, grow)
    ringm = dilate(T, k) & ~near_text[wy1:wy2, wx1:wx2]
    F[wy1:wy2, wx1:wx2] = fill
    n_ring = int(ringm.sum())
    px = page[wy1:wy2, wx1:wx2][ringm]                      # (n_ring, 3)
    med, cnt = [], []
    for c in range(3):
        h = np.bincount(px[:, c], minlength=256).astype(np.int64)
        cum = np.cumsum(h)
        m = int(np.nonzero(2 * cum >= n_ring)[0][0])         # the smallest v with 2 * sum_{u <= v} h[u] >= n_ring
        med.append(m)
        cnt.append(int(h[max(m - tol, 0):m + tol + 1].sum()))
    if n_ring < min_ring:
        status = NO_RING
    else:
        status = PLAIN if 16 * min(cnt) >= 15 * n_ring else TEXTURED
    return dict(status=status, n_fill=int(fill.sum()), n_ring=n_ring, cnt=cnt, med=med), F


def erase_page(page, mask, boxes, grow=2, ring=4, tol=12, min_ring=16):
    """The rule on one page: (rows, out, rest).  page (H,W,3) u8, mask (H,W) u8, boxes: the blocks' xyxy in blk_list order."""
    check_params(grow, ring, tol, min_ring)
    page, mask = np.asarray(page), np.asarray(mask)
    H, W = mask.shape
    text = mask != 0
    near = dilate(text, grow)
    rows, fills = [], []
    for xyxy in boxes:
        row, F = block_row(page, text, near, xyxy, grow, ring, tol, min_ring)
        rows.append(row)
        fills.append(F)
    out = page.copy()
    painted = np.zeros((H, W), bool)
    keep = text.copy()
    for row, F in zip(rows, fills):                              # ascending index: the highest PLAIN block is the last to write
        if F is None:
            continue
        if row["status"] == PLAIN:
            out[F] = np.array(row["med"], np.uint8)
            painted |= F
        elif row["status"] in (TEXTURED, NO_RING):
            keep |= F
    rest = np.where(~painted & keep, 255, 0).astype(np.uint8)
    return rows, out, rest


def row_dict(row):
    """A record of the kernel's result table as the dict `block_row` returns."""
    return {k: (row[k].tolist() if np.ndim(row[k]) else int(row[k])) for k in FIELDS}


# ---- flat pages with known answers (tests/test_erase_ref.py; the GPU test runs the same through the kernels) -----------------

def flat_page(text_colour, balloon, shape=(60, 90), box=(20, 15, 70, 45), bar_h=3):
    """A page of one colour with bar "glyphs" of another inside `box`, 6 pixels from its edges; (page, mask): the mask is the
    glyphs exactly."""
    H, W = shape
    page = np.empty((H, W, 3), np.uint8)
    page[:] = np.array(balloon, np.uint8)
    mask = np.zeros((H, W), np.uint8)
    x1, y1, x2, y2 = box
    for y in range(y1 + 6, y2 - 6 - bar_h + 1, 2 * bar_h + 2):
        mask[y:y + bar_h, x1 + 6:x2 - 6] = 255
    page[mask != 0] = np.array(text_colour, np.uint8)
    return page, mask


FLAT = [((20, 30, 40), (250, 240, 230)), ((255, 255, 255), (0, 0, 0)), ((0, 0, 200), (0, 180, 0)), ((90, 90, 90), (102, 102, 102))]


def flat_cases():
    """(page, mask, boxes, balloon colour) of every flat case."""
    for text_colour, balloon in FLAT:
        page, mask = flat_page(text_colour, balloon)
        yield page, mask, [(20, 15, 70, 45)], list(balloon)
