"""TEST INFRASTRUCTURE of tests/test_ccl_runs_emul.py and tests/test_gpu_ccl_runs.py: the labelling on row runs
(`launch_ccl_dual` and its single-class front `launch_ccl`, csrc/kernels_post.hip) in numpy and plain
Python, kernel by kernel, and the pages both tests label.

    pack()         ccl2_pack          bits / starts words; the class flip of the 4-connected single-class labelling
    scan()         ccl2_run_scan      base words, the run count R
    word_unions()  ccl2_word_unions   one word against the row above: groups of set bits, halo bits for the foreground
    label_runs()   ccl2_band (a table in "LDS" per band, global when the band has more than RB_CAP runs),
                   ccl2_band_border, ccl2_flatten_count / ccl2_scan_chunks / ccl2_rank / ccl2_spread
    paint()        ccl2_label         the plane, statistics, first pixels, segment flags; keep = its single-class form
    label_single() launch_ccl         conn 8: the foreground class; conn 4: the background class of the flipped page

What can go wrong in the kernels and shows here first: a run id off by one at a word's first or last bit, a halo bit taken
from the wrong word or at the page's edge, the background joined diagonally, a union skipped because "the word to the left
made it" where that word did not, a band's local ids based on the wrong word, a band over the table's capacity, bits beyond
W starting runs.  No GPU is needed."""
import functools

import numpy as np

RB_ROWS = 32     # = RB_ROWS of kernels_post.hip
RB_CAP = 8192    # = RB_CAP of kernels_post.hip (test_ccl_runs_emul.py compares the two with the source)
M32 = 0xFFFFFFFF


def popc(v):
    return bin(v).count("1")


def ffs(v):
    """1-based index of the lowest set bit, 0 for 0 (the device's __ffs)."""
    return (v & -v).bit_length()


def pack(fg, flip=False):
    """(H, W) bool (pixel > thresh) -> bits, starts: lists of H * wp Python ints.  A bit is set where fg != flip."""
    fg = fg != flip
    H, W = fg.shape
    wp = (W + 31) // 32
    bits, starts = [], []
    for y in range(H):
        for wx in range(wp):
            v = 0
            for i in range(min(32, W - 32 * wx)):
                v |= int(fg[y, 32 * wx + i]) << i
            nbit = min(32, W - 32 * wx)
            vmask = M32 if nbit >= 32 else (1 << nbit) - 1
            pb = int(fg[y, 32 * wx - 1]) if wx > 0 else (~v & 1)          # x == 0 always starts a run
            bits.append(v)
            starts.append((v ^ (((v << 1) & M32) | pb)) & vmask)
    return bits, starts


def scan(starts):
    base, c = [], 0
    for s in starts:
        base.append(c)
        c += popc(s)
    return base, c


def low_mask(i):
    """(2u << i) - 1u in 32 bits: bits 0..i."""
    return (((2 << i) & M32) - 1) & M32


def word_unions(bits, starts, base, y, wx, wp, W, unite):
    w = y * wp + wx
    wa = w - wp
    hl, hr = wx > 0, wx + 1 < wp
    c, sc, a, sa, bc, ba = bits[w], starts[w], bits[wa], starts[wa], base[w], base[wa]
    al, sal, bal = (bits[wa - 1], starts[wa - 1], base[wa - 1]) if hl else (0, 0, 0)
    ar, sar, bar = (bits[wa + 1], starts[wa + 1], base[wa + 1]) if hr else (0, 0, 0)
    nbit = min(32, W - 32 * wx)
    vmask = M32 if nbit >= 32 else (1 << nbit) - 1
    for cls in (0, 1):
        m = (c if cls else ~c) & vmask
        ma = (a if cls else ~a) & vmask
        rest = m
        while rest:
            lo = ffs(rest) - 1
            frm = m >> lo
            nf = ~frm & M32
            ln = ffs(nf) - 1 if nf else 32 - lo
            g = ((M32 if ln >= 32 else (1 << ln) - 1) << lo) & M32
            rest &= ~g
            me = bc + popc(sc & low_mask(lo)) - 1
            cont = lo == 0 and not (sc & 1)
            reach = g
            if cls:
                reach |= ((g << 1) & M32) | (g >> 1)
            ov = ma & reach
            while ov:
                bpos = ffs(ov) - 1
                if not (cont and bpos == 0 and not (sa & 1)):
                    unite(me, ba + popc(sa & low_mask(bpos)) - 1)
                froma = ma >> bpos
                nfa = ~froma & M32
                lena = ffs(nfa) - 1 if nfa else 32 - bpos
                ov &= ~(((M32 if lena >= 32 else (1 << lena) - 1) << bpos) & M32)
            if cls:
                if lo == 0 and (al >> 31):
                    unite(me, bal + popc(sal) - 1)
                if lo + ln == 32 and (ar & 1):
                    unite(me, bar + (sar & 1) - 1)


def find(parent, x):
    while parent[x] != x:
        x = parent[x]
    return x


def union(parent, a, b):
    """uf_union / lds_union: the larger root goes under the smaller."""
    a, b = find(parent, a), find(parent, b)
    if a != b:
        parent[max(a, b)] = min(a, b)


def label_runs(fg, cap=RB_CAP, flip=False):
    """The run tables of one page: bits, starts, base, R, rcls, rparent (flat), rlabel, n_f, n_b, and `over` = the bands
    that did not fit a table of `cap` runs."""
    H, W = fg.shape
    wp = (W + 31) // 32
    bits, starts = pack(fg, flip)
    base, R = scan(starts)
    rparent, rcls, over = [None] * R, [None] * R, []
    nbands = (H + RB_ROWS - 1) // RB_ROWS
    for k in range(nbands):                                           # ccl2_band
        y0, y1 = k * RB_ROWS, min(H, (k + 1) * RB_ROWS)
        gbase = base[y0 * wp]
        n = (base[y1 * wp] if y1 < H else R) - gbase
        in_lds = n <= cap
        if in_lds:
            lp = list(range(n))
            unite = lambda p, q: union(lp, p - gbase, q - gbase)      # noqa: E731 (a local id outside [0, n) raises)
        else:
            over.append(k)
            for i in range(n):
                rparent[gbase + i] = gbase + i
            unite = lambda p, q: union(rparent, p, q)                 # noqa: E731
        for wi in range(y0 * wp, y1 * wp):
            y, wx = divmod(wi, wp)
            s, rid = starts[wi], base[wi]
            while s:
                pos = ffs(s) - 1
                s &= s - 1
                rcls[rid] = (bits[wi] >> pos) & 1
                rid += 1
            if y > y0:
                word_unions(bits, starts, base, y, wx, wp, W, unite)
        if in_lds:
            for i in range(n):
                rparent[gbase + i] = gbase + find(lp, i)
    assert None not in rparent and None not in rcls
    for k in range(1, nbands):                                        # ccl2_band_border
        for wx in range(wp):
            word_unions(bits, starts, base, RB_ROWS * k, wx, wp, W, lambda p, q: union(rparent, p, q))
    rparent = [find(rparent, r) for r in range(R)]                    # flatten; roots ranked per class in run order
    rlabel, n_f, n_b = [0] * R, 0, 0
    for r in range(R):
        if rparent[r] == r:
            if rcls[r]:
                n_f += 1
                rlabel[r] = 2 * n_f + 1                               # the low bit: a root
            else:
                n_b += 1
                rlabel[r] = -2 * n_b + 1
    for r in range(R):                                                # ccl2_spread
        if rparent[r] != r:
            rlabel[r] = rlabel[rparent[r]] & ~1
    return dict(H=H, W=W, wp=wp, bits=bits, starts=starts, base=base, R=R, rcls=rcls, rparent=rparent, rlabel=rlabel, n_f=n_f,
                n_b=n_b, over=over)


def paint(t, max_labels, keep=0, other=0):
    """The plane from base / starts / rlabel; statistics [x, y, w, h, area] and first pixels of labels 1..max_labels of
    either class (rows beyond the count stay -1 here; the device leaves them unwritten); the 64-pixel segment flags.
    keep = +1 / -1 (ccl2_label<KEEP>): that class alone -- its pixels get |id| and its tables are st[1] / first[1], a
    pixel of the other class gets `other` and takes no part in the tables; no segment flags."""
    H, W, wp = t["H"], t["W"], t["wp"]
    plane = np.zeros((H, W), np.int32)
    st = {1: np.full((max_labels, 5), -1, np.int64), -1: np.full((max_labels, 5), -1, np.int64)}
    first = {1: np.full(max_labels, -1, np.int64), -1: np.full(max_labels, -1, np.int64)}
    box = {}
    for y in range(H):
        for x in range(W):
            w, bit = y * wp + (x >> 5), x & 31
            run = t["base"][w] + popc(t["starts"][w] & low_mask(bit)) - 1
            lab, root = t["rlabel"][run] >> 1, t["rlabel"][run] & 1
            if keep:
                lab = abs(lab) if (lab > 0) == (keep > 0) else 0
                if not lab:
                    plane[y, x] = other
                    continue
            plane[y, x] = lab
            mag, sign = abs(lab), (1 if lab > 0 else -1)
            if mag > max_labels:
                continue
            if (t["starts"][w] >> bit) & 1 and root:
                first[sign][mag - 1] = y * W + x
            b = box.setdefault(lab, [W, H, -1, -1, 0])
            b[0], b[1], b[2], b[3], b[4] = min(b[0], x), min(b[1], y), max(b[2], x), max(b[3], y), b[4] + 1
    for lab, b in box.items():
        st[1 if lab > 0 else -1][abs(lab) - 1] = [b[0], b[1], b[2] - b[0] + 1, b[3] - b[1] + 1, b[4]]
    if keep:
        return plane, st, first, None
    live = plane.ravel() != -1
    seg = np.r_[live, np.zeros((-live.size) % 64, bool)].reshape(-1, 64).any(axis=1)
    return plane, st, first, seg


def label_single(fg, conn, max_labels, other=0, cap=RB_CAP):
    """launch_ccl on (pixel > thresh) = fg: (run tables, n, plane, stats, first).  conn 8 is the foreground half of the dual
    labelling; conn 4 is the background half of the dual labelling of the flipped page."""
    keep = 1 if conn == 8 else -1
    t = label_runs(fg, cap, flip=(conn == 4))
    plane, st, first, _ = paint(t, max_labels, keep, other)
    return t, (t["n_f"] if keep > 0 else t["n_b"]), plane, st[1], first[1]


# ---------------------------------------------------------------------------------------------------------------------------
# the pages
# ---------------------------------------------------------------------------------------------------------------------------
WIDTHS = (1, 31, 32, 33, 64, 65, 131)
HEIGHTS = (1, 2, 31, 32, 33, 65)          # a band boundary at every position: none, after the last row, inside


def noise(H, W, density, seed):
    return np.random.RandomState(seed).rand(H, W) < density


def _grid(H, W):
    return np.mgrid[0:H, 0:W]


def pages_for(H, W):
    """[(name, (H, W) bool foreground)] -- every kind of page that makes sense at this size."""
    y, x = _grid(H, W)
    out = [(f"noise {d}", noise(H, W, d, 1000 * H + W + int(100 * d))) for d in (0.1, 0.3, 0.5, 0.6, 0.85)]
    out += [("all foreground", np.ones((H, W), bool)), ("all background", np.zeros((H, W), bool)),
            ("checkerboard", (x + y) % 2 == 0), ("checkerboard, odd", (x + y) % 2 == 1),
            # diagonals through every word and band boundary, both ways: they join for the foreground only
            ("diagonals down", (x - y) % 4 == 0), ("diagonals up", (x + y) % 4 == 1),
            ("background diagonals", (x - y) % 4 != 0),
            # rows that are one run across all words
            ("rows", y % 2 == 0), ("rows, odd", y % 2 == 1), ("columns", x % 2 == 0),
            # single pixels at bits 0 and 31
            ("bits 0 and 31", ((x % 32 == 0) | (x % 32 == 31)) & (y % 2 == 0)),
            ("holes at bits 0 and 31", ~(((x % 32 == 0) | (x % 32 == 31)) & (y % 3 == 1)))]
    pairs = np.zeros((H, W), bool)          # diagonal pixel pairs across a word boundary and across a band boundary
    for (ya, xa), (yb, xb) in (((0, 31), (1, 32)), ((3, 32), (4, 31)), ((31, 5), (32, 6)), ((31, 9), (32, 8)),
                               ((31, 31), (32, 32)), ((31, 64), (32, 63)), ((6, 63), (7, 64)), ((63, 64), (64, 63))):
        if max(ya, yb) < H and max(xa, xb) < W:
            pairs[ya, xa] = pairs[yb, xb] = True
    out += [("diagonal pairs", pairs), ("diagonal pairs of background", ~pairs)]
    if H >= 33 and W >= 65:
        from db_runs_cases import frame_map, rings_map, top_bar_map
        out += [("frame", frame_map(H, W, 2, t=1) > 0.3), ("rings", rings_map(H, W) > 0.3), ("top bar", top_bar_map(H, W, 3) > 0.3)]
    elif H >= 9 and W >= 9:
        from db_runs_cases import rings_map
        out += [("rings", rings_map(H, W) > 0.3)]
    return out


@functools.lru_cache(None)
def small_calls():
    """[((H, W), [(name, page)])]: the pages of one call share a shape."""
    return [((H, W), pages_for(H, W)) for H in HEIGHTS for W in WIDTHS]


def over_capacity_page(W=1024, seed=5):
    """96 x W: a band of alternating pixels (32 * W runs > RB_CAP) between two sparse bands under the capacity."""
    fg = noise(96, W, 0.02, seed)
    fg[32:64] = (np.arange(W) % 2 == 0)[None, :]
    return fg


def reference(fg):
    """{+1: (n, labels, stats rows 1..n), -1: ...} from the oracle: 8-connected foreground, 4-connected background."""
    from oracle import postproc_ref as R
    out = {}
    for sign, img, conn in ((1, fg, 8), (-1, ~fg, 4)):
        n, lab, st = R.connected_components_with_stats(img.astype(np.uint8) * 255, conn)
        out[sign] = (n - 1, lab, st[1:])
    return out
