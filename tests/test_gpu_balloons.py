"""-m gpu: balloon regions -- `ctd_balloon_regions` (csrc/kernels_balloon.hip), `balloons.balloon_regions` and
`TextDetector.balloons` -- against the numpy restatement tests/balloon_ref.py, whose components come from a queue flood fill.
The rule is integers only and a connected component has one answer, so every comparison is EXACT: every field of every row
and every word of every bit plane.  One call carries all pages of the material."""
import ctypes as C

import numpy as np
import pytest
import torch

import balloon_ref as BR
import erase_ref as ER
import test_gpu_regions as TG
from conftest import pkg

pytestmark = pytest.mark.gpu

WHITE, INK = 255, 0


# ---- the material ------------------------------------------------------------------------------------------------------------

def _room(page, mask, x1, y1, x2, y2, text, colour=WHITE):
    """A room of `colour` with a bar of text (x1, y1, x2, y2 of the bar) on `page`; returns the bar."""
    page[y1:y2, x1:x2] = colour
    tx1, ty1, tx2, ty2 = text
    mask[ty1:ty2, tx1:tx2] = 255
    page[ty1:ty2, tx1:tx2] = INK
    return text


def spiral(n=45):
    """An n x n plane, True on a 1-pixel corridor that winds from (1, 1) clockwise to the middle between 1-pixel walls; and the
    corridor's last pixel (x, y)."""
    a = np.zeros((n, n), bool)
    x = y = 1
    a[y, x] = True
    d = 0
    steps = ((1, 0), (0, 1), (-1, 0), (0, -1))
    turned = 0
    while turned < 2:
        dx, dy = steps[d]
        nx, ny, fx, fy = x + dx, y + dy, x + 2 * dx, y + 2 * dy
        if 1 <= nx <= n - 2 and 1 <= ny <= n - 2 and not a[ny, nx] and not (0 <= fx < n and 0 <= fy < n and a[fy, fx]):
            x, y = nx, ny
            a[y, x] = True
            turned = 0
        else:
            d = (d + 1) % 4
            turned += 1
    return a, (x, y)


def comb(h=41, teeth=20):
    """An h x (2 teeth + 1) plane: 1-pixel corridors between 1-pixel walls that hang from the top and stand on the bottom in
    turn, so the way from column 1 to the last corridor goes down, up, down, ...; and the last corridor's far end (x, y)."""
    w = 2 * teeth + 1
    a = np.zeros((h, w), bool)
    a[1:h - 1, 1:w - 1:2] = True
    for k in range(teeth - 1):
        a[h - 2 if k % 2 == 0 else 1, 2 + 2 * k] = True
    last = teeth - 1
    return a, (1 + 2 * last, 1 if last % 2 == 1 else h - 2)


def maze_page(plane, entry_y=1):
    """`plane` (True = corridor) at the left of a black page, a white room with a bar of text at its right, joined along row
    `entry_y` through the plane's right wall; the block's box is the whole page.  (page, mask, boxes)."""
    sh, sw = plane.shape
    H, W = max(sh, 36), sw + 52
    page = np.zeros((H, W, 3), np.uint8)
    mask = np.zeros((H, W), np.uint8)
    page[:sh, :sw][plane] = WHITE
    page[entry_y, sw - 1:sw + 6] = WHITE
    _room(page, mask, sw + 6, 0, sw + 50, 35, (sw + 18, 14, sw + 38, 20))
    return page, mask, [(0, 0, W, H)]


def word_geometry_pages():
    """Flat 40 x 300 pages for reach = 0, reach_min = 8 (window = box grown by 8): windows 63, 64, 65 and 129 wide whose x origin
    is 0, 1, 62 and 63 (mod 64), all open (a 64-pixel run that fills one word; runs across one and two word boundaries); and
    the same with single wall pixels that end runs at bit 62, 63, 0 and 1 of a word."""
    out = []
    for walls in (False, True):
        page = np.full((40, 300, 3), (180, 200, 220), np.uint8)
        mask = np.zeros((40, 300), np.uint8)
        boxes = []
        for origin, width in ((64, 63), (1, 64), (62, 65), (63, 129), (128, 64), (0, 129), (127, 65), (190, 63)):
            x1, x2 = origin + 8, origin + width - 8
            boxes.append((x1, 16, x2, 22))
            mask[18:20, x1 + 2:x2 - 2] = 255
        page[mask != 0] = (10, 20, 30)
        if walls:
            for x in (62, 63, 64, 65, 126, 127, 128, 129, 191, 192, 255, 256):
                page[9 + (x % 5), x] = (0, 0, 0)
                page[30 - (x % 3), x] = (0, 0, 0)
            page[11, 70:260] = (0, 0, 0)                            # a wall above the text with one door
            page[11, 128] = (180, 200, 220)
        out.append((page, mask, boxes))
    return out


def noise_page(shape, dens, seed, colour=(240, 230, 250)):
    """Wall pixels at random (density 1 - dens) on a page of one colour, a clean room with a bar of text in the middle, the
    block's box the whole page: near the site percolation threshold the region is a ragged thing that a flood fill and the
    kernel's sweeps reach in very different orders."""
    rng = np.random.default_rng(seed)
    H, W = shape
    page = np.empty((H, W, 3), np.uint8)
    page[:] = np.array(colour, np.uint8)
    page[rng.random((H, W)) >= dens] = (30, 30, 30)
    mask = np.zeros((H, W), np.uint8)
    cx, cy = W // 2, H // 2
    _room(page, mask, cx - 20, cy - 10, cx + 20, cy + 10, (cx - 12, cy - 2, cx + 12, cy + 2), colour)
    return page, mask, [(0, 0, W, H), (cx - 12, cy - 2, cx + 12, cy + 2)]


def connectivity_page():
    """One 80 x 200 black page: (a) a room whose right wall is a checkerboard (diagonal contact only beyond its first column),
    (b) an "O" of own text whose counter is joined through F_b, with another block's text as a hole beside it, (c) one box over
    two closed rooms with text in both."""
    page = np.zeros((80, 200, 3), np.uint8)
    mask = np.zeros((80, 200), np.uint8)
    boxes = [_room(page, mask, 2, 2, 50, 30, (12, 12, 36, 18))]
    ys, xs = np.mgrid[2:30, 50:60]
    page[ys, xs] = np.where(((ys + xs) % 2 == 0)[..., None], WHITE, 0).astype(np.uint8)
    page[40:78, 2:70] = WHITE                                       # (b)
    mask[50:66, 14:30] = 255
    mask[55:61, 19:25] = 0                                          # the counter of the O: 6 x 6, not text
    mask[56:60, 44:60] = 255                                        # the neighbour
    page[mask != 0] = INK
    page[50:66, 14:30][mask[50:66, 14:30] == 0] = WHITE
    boxes += [(14, 50, 30, 66), (44, 56, 60, 60)]
    _room(page, mask, 80, 4, 130, 36, (92, 16, 118, 22))            # (c)
    _room(page, mask, 132, 4, 190, 36, (146, 16, 176, 22))
    boxes.append((80, 4, 190, 36))
    return page, mask, boxes


def colour_page(tol=12):
    """A room of (100, 150, 200) with, far from the text, pixels that differ in ONE channel by exactly tol (open) and by
    tol + 1 (a hole), up and down, for each channel."""
    page = np.zeros((60, 120, 3), np.uint8)
    mask = np.zeros((60, 120), np.uint8)
    base = (100, 150, 200)
    _room(page, mask, 4, 4, 116, 56, (48, 27, 72, 33), base)
    box = (4, 4, 116, 56)                                           # the block's box is the room: the window is the page
    holes = 0
    for c in range(3):
        for k, d in enumerate((tol, -tol, tol + 1, -tol - 1)):
            px = list(base)
            px[c] += d
            page[8 + 4 * c, 10 + 6 * k] = px
            page[50, 80 + 3 * (4 * c + k)] = px                     # and a second copy in a row of its own
            holes += 2 * (abs(d) > tol)
    return page, mask, [box], 112 * 52 - holes


def flags_page():
    """A 240 x 300 black page with eight small rooms, each with one 3-pixel arm: four in the middle whose arm runs out of the
    window (reach_min = 32) on one side each, four whose arm runs to the page's edge on one side each."""
    page = np.zeros((240, 300, 3), np.uint8)
    mask = np.zeros((240, 300), np.uint8)
    boxes, want = [], []
    arms = {"l": (-50, 0), "t": (0, -50), "r": (50, 0), "b": (0, 50)}
    bit = {"l": BR.CUT_LEFT, "t": BR.CUT_TOP, "r": BR.CUT_RIGHT, "b": BR.CUT_BOTTOM}
    spots = [(100, 80, "l", 0), (200, 80, "t", 0), (100, 160, "r", 0), (200, 160, "b", 0),
             (30, 120, "l", 4), (150, 20, "t", 4), (270, 120, "r", 4), (150, 220, "b", 4)]
    for cx, cy, side, shift in spots:
        boxes.append(_room(page, mask, cx - 18, cy - 10, cx + 18, cy + 10, (cx - 10, cy - 2, cx + 10, cy + 2)))
        dx, dy = arms[side]
        xa, xb = sorted((cx, cx + dx))
        ya, yb = sorted((cy, cy + dy))
        arm = page[max(ya - 1, 0):min(yb + 2, 240), max(xa - 1, 0):min(xb + 2, 300)]
        arm[(arm != INK).all(axis=2) | (mask[max(ya - 1, 0):min(yb + 2, 240), max(xa - 1, 0):min(xb + 2, 300)] == 0)] = WHITE
        page[mask != 0] = INK
        want.append(bit[side] << shift)
    return page, mask, boxes, want


def status_page():
    """Blocks the erase rule does not call plain: on noise (TEXTURED), in dense lettering (NO_RING), without text (NO_MASK),
    outside the page (EMPTY); and one plain block, last."""
    rng = np.random.default_rng(8)
    page = np.full((70, 160, 3), 200, np.uint8)
    page[:, :60] = rng.integers(60, 256, (70, 60, 3), dtype=np.uint8)
    mask = np.zeros((70, 160), np.uint8)
    mask[30:34, 10:50] = 255                                        # on the noise
    mask[4:66:4, 70:110] = 255                                      # a text row every 4 pixels
    mask[30:34, 125:150] = 255
    page[mask != 0] = 5
    return page, mask, [(10, 30, 50, 34), (80, 28, 100, 29), (112, 2, 122, 12), (-30, 5, -10, 14), (160, 0, 190, 9), (125, 30, 150, 34)]


def _material():
    """[(page, mask, boxes)]: the pages of ONE call, mixed sizes, a page without blocks in the middle."""
    out = word_geometry_pages()
    out.append(maze_page(spiral()[0]))
    out.append(maze_page(comb()[0]))
    out.append((np.zeros((33, 47, 3), np.uint8), np.zeros((33, 47), np.uint8), []))          # no blocks
    out.append(maze_page(comb()[0].T.copy(), entry_y=1))
    out += [noise_page((71, 203), 0.62, 1), noise_page((97, 131), 0.7, 2), noise_page((64, 129), 0.55, 3)]
    out.append(connectivity_page())
    out.append(colour_page()[:3])
    out.append(flags_page()[:3])
    out.append(status_page())
    page, mask, box = BR.chamber_page(bg=255, gap=(20, 30))
    out.append((page, mask, [box]))
    return out


_REF = {}


def reference(kw_key, material, kw):
    """`balloon_ref.balloon_page` of every page of the material, computed once per parameter set."""
    if kw_key not in _REF:
        _REF[kw_key] = [BR.balloon_page(page, mask, boxes, **kw) for page, mask, boxes in material]
    return _REF[kw_key]


def _compare(br, material, ref, what=""):
    """Every field of every row, every word; returns the reference rows."""
    host_rows, host_bits = br.to_host()
    assert host_rows.dtype.itemsize == 48 and host_bits.dtype == np.uint64
    want_rows, k, bad, covered = [], 0, [], 0
    for i, ((page, mask, boxes), (rows, words, wins, erows)) in enumerate(zip(material, ref)):
        for b, (row, w, win, erow) in enumerate(zip(rows, words, wins, erows)):
            assert br.index[k].tolist() == [i, b] and tuple(br.windows[k]) == win
            got = BR.row_dict(host_rows[k])
            if got != row:
                bad.append((i, b, boxes[b], {f: (got[f], row[f]) for f in BR.FIELDS if got[f] != row[f]}))
            assert (w is None) == bool(br.too_large[k])
            if w is not None:
                assert br.word0[k] == covered
                mine = host_bits[covered: covered + len(w)]
                covered += len(w)
                if not np.array_equal(mine, w):
                    diff = np.nonzero(mine != w)[0]
                    bad.append((i, b, "words", len(diff), [(int(d), hex(int(mine[d])), hex(int(w[d]))) for d in diff[:3]]))
                if len(w):
                    m = br.mask(k)
                    assert m.dtype == torch.bool and m.is_cuda and tuple(m.shape) == (win[3] - win[1], win[2] - win[0])
                    if not np.array_equal(m.cpu().numpy(), BR.unpack(w, win[3] - win[1], win[2] - win[0])):
                        bad.append((i, b, "mask()"))
            if row["status"] == BR.OK:
                assert int(br.erase_rows[k]["n_fill"]) == row["n_seed"] == got["n_seed"] == erow["n_fill"]
                assert br.center[k].tolist() == [row["sum_x"] // row["area"], row["sum_y"] // row["area"]]
            else:
                assert br.center[k].tolist() == [-1, -1]
            assert ER.row_dict(br.erase_rows[k]) == erow
            k += 1
        want_rows += rows
    assert k == len(br) == len(host_rows) and covered == len(host_bits)
    assert not bad, f"{what}: {len(bad)} differences, first: {bad[:4]}"
    return want_rows


def _device_inputs(material, dev):
    """Device tensors of the material; pages 2 and 6 are views with a row pitch beyond their width whose masks have another
    pitch (odd widths: 97, 203)."""
    pages = [torch.from_numpy(m[0]).to(dev) for m in material]
    masks = [torch.from_numpy(m[1]).to(dev) for m in material]
    for i, (lead, extra) in ((2, (17, 9)), (6, (5, 30))):
        H, W = material[i][0].shape[:2]
        wide = torch.zeros((H, W + lead + extra, 3), dtype=torch.uint8, device=dev)
        wide[:, lead:lead + W] = pages[i]
        pages[i] = wide[:, lead:lead + W]
        wm = torch.zeros((H, W + 2 * lead + 1), dtype=torch.uint8, device=dev)
        wm[:, lead:lead + W] = masks[i]
        masks[i] = wm[:, lead:lead + W]
        assert not pages[i].is_contiguous() and not masks[i].is_contiguous() and W % 2 == 1
    return pages, masks


class _Blk:
    def __init__(self, xyxy):
        self.xyxy = list(xyxy)


PARAMS = [dict(), dict(grow=0, tol=0, reach=0, reach_min=8), dict(grow=8, tol=40, reach=32, reach_min=9)]


# ---- 1. the kernel -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", range(len(PARAMS)), ids=["defaults", "g0reach0", "g8reach32"])
def test_kernel_equals_the_restatement_in_every_field_and_word(k):
    """One `balloon_regions` call over the whole material against `balloon_ref.balloon_page`, at three parameter sets; the same
    call twice gives identical bytes, and `erased=` from a prior `erase_text` gives the same as the self-made erase rows."""
    p = pkg()
    B, E = p.balloons, p.erase
    kw = PARAMS[k]
    dev = torch.device("cuda:0")
    material = _material()
    ref = reference(k, material, kw)
    pages, masks = _device_inputs(material, dev)
    lists = [[_Blk(b) for b in m[2]] for m in material]
    br = B.balloon_regions(pages, masks, lists, **kw)
    want = _compare(br, material, ref, str(kw))
    counts = [sum(w["status"] == s for w in want) for s in range(3)]
    print(f"\n{kw}: {len(want)} blocks on {len(material)} pages, status counts {counts}, {len(br.bits)} words")
    assert counts[BR.OK] >= 10 and counts[BR.NOT_PLAIN] >= 4
    again = B.balloon_regions(pages, masks, lists, **kw)
    assert again.rows.tobytes() == br.rows.tobytes() and torch.equal(again.bits.view(torch.int64), br.bits.view(torch.int64))
    er = E.erase_text(pages, masks, lists, grow=kw.get("grow", 2), tol=kw.get("tol", 12))
    other = B.balloon_regions(pages, masks, lists, erased=er, **kw)
    assert other.rows.tobytes() == br.rows.tobytes() and torch.equal(other.bits.view(torch.int64), br.bits.view(torch.int64))
    assert np.array_equal(other.erase_rows, er.rows) and np.array_equal(br.erase_rows, er.rows)


def test_what_the_material_is_there_for():
    """The cases of the material by name, at the default parameters (and the word geometry at reach 0): the spiral's and the
    combs' far ends are reached, diagonal contact does not join, an O's counter does, a neighbour's text is a hole, two rooms
    under one box come back as their union, a pixel at tol is open and one beyond is not, each cut and each page-edge flag
    alone, the four not-plain statuses."""
    p = pkg()
    B = p.balloons
    material = _material()
    ref = reference(0, material, PARAMS[0])
    lists = [[_Blk(b) for b in m[2]] for m in material]
    br = B.balloon_regions([m[0] for m in material], [m[1] for m in material], lists)
    _compare(br, material, ref)
    first = {int(pg): j for j, (pg, b) in reversed(list(enumerate(br.index.tolist())))}

    def plane(j):
        x1, y1, x2, y2 = br.windows[j].tolist()
        full = np.zeros(material[br.index[j][0]][1].shape, bool)
        full[y1:y2, x1:x2] = br.mask(j).cpu().numpy()
        return full

    # convergence: the far end of the spiral (page 2), of the comb (3) and of the comb on its side (5)
    (sp, end), (cb, cend) = spiral(), comb()
    assert sp[end[1], end[0]] and int(sp.sum()) == 967
    got = plane(first[2])
    assert got[end[1], end[0]] and np.array_equal(got[:45, :44], sp[:, :44])        # (column 44 holds the door)
    got = plane(first[3])
    assert got[cend[1], cend[0]] and np.array_equal(got[:41, :40], cb[:, :40])
    got = plane(first[5])
    assert got[cend[0], cend[1]] and np.array_equal(got[:41, :40], cb.T[:, :40])
    # connectivity (page 9)
    j = first[9]
    a = plane(j)
    assert a[2:30, 50].sum() == 14 and not a[2:30, 51:60].any() and br.area[j] == 48 * 28 + 14
    o = plane(j + 1)
    assert o[55:61, 19:25].all() and not o[56:60, 44:60].any() and o[57, 43] and br.area[j + 1] == 38 * 60 - 16 * 4
    assert br.flags[j + 1] == BR.CUT_RIGHT                          # its window ends at x = 62, inside the white area
    assert not plane(j + 2)[50:66, 14:30].any()
    two = plane(j + 3)
    assert br.area[j + 3] == 50 * 32 + 58 * 32 and two[4:36, 80:130].all() and two[4:36, 132:190].all() and not two[:, 130:132].any()
    assert br.bbox[j + 3].tolist() == [80, 4, 190, 36] and br.flags[j + 3] == 0
    # colour (page 10), flags (page 11), statuses (page 12), the leak (page 13)
    assert br.area[first[10]] == colour_page()[3] and br.status[first[10]] == BR.OK
    j = first[11]
    assert br.flags[j:j + 8].tolist() == flags_page()[3] and br.ok[j:j + 8].all()
    j = first[12]
    assert br.erase_rows["status"][j:j + 6].tolist() == [ER.TEXTURED, ER.NO_RING, ER.NO_MASK, ER.EMPTY, ER.EMPTY, ER.PLAIN]
    assert br.status[j:j + 6].tolist() == [BR.NOT_PLAIN] * 5 + [BR.OK]
    assert not br.rows[j:j + 5].view(np.uint8).reshape(5, -1)[:, 8:].any() and (br.rows["status"][j:j + 5] == 1).all()
    assert br.flags[first[13]] == 0xA5
    # word geometry at reach 0: the windows are the ones the material promises, and all of each is reached on the flat page
    kw = PARAMS[1]
    br0 = B.balloon_regions([m[0] for m in material[:2]], [m[1] for m in material[:2]], lists[:2], **kw)
    _compare(br0, material[:2], reference(1, material, kw)[:2])
    ws = br0.windows[:8]
    assert (ws[:, 2] - ws[:, 0]).tolist() == [63, 64, 65, 129, 64, 129, 65, 63] and (ws[:, 0] % 64).tolist() == [0, 1, 62, 63, 0, 0, 63, 62]
    assert br0.area[:8].tolist() == [int(w) * 22 - n for w, n in zip(ws[:, 2] - ws[:, 0], _others_text(material[0], ws))]


def _others_text(entry, ws):
    """Per window of the first word-geometry page: the text pixels of OTHER blocks inside it (holes on the flat page)."""
    page, mask, boxes = entry
    out = []
    for (x1, y1, x2, y2), b in zip(ws.tolist(), boxes):
        other = mask != 0
        other[b[1]:b[3], b[0]:b[2]] = False
        f = ER.dilate((mask != 0) & ~other, 0)
        out.append(int((other[y1:y2, x1:x2] & ~f[y1:y2, x1:x2]).sum()))
    return out


def test_the_largest_window_and_one_beyond_it():
    """512 x 1024 pixels, flat, all open: 8192 words, every one all ones, area 524288 -- the answer is written out, no flood
    fill is needed.  A flat 600 x 1100 page with a full-page box is TOO_LARGE and owns no word."""
    p = pkg()
    B = p.balloons
    dev = torch.device("cuda:0")
    big = torch.full((1024, 512, 3), 77, dtype=torch.uint8, device=dev)
    bm = torch.zeros((1024, 512), dtype=torch.uint8, device=dev)
    bm[500:510, 200:300] = 255
    over = torch.full((1100, 600, 3), 77, dtype=torch.uint8, device=dev)
    om = torch.zeros((1100, 600), dtype=torch.uint8, device=dev)
    om[500:510, 200:300] = 255
    br = B.balloon_regions([over, big], [om, bm], [[_Blk((0, 0, 600, 1100))], [_Blk((0, 0, 512, 1024))]])
    assert br.erase_rows["status"].tolist() == [ER.PLAIN, ER.PLAIN] and br.too_large.tolist() == [True, False]
    assert BR.row_dict(br.rows[0]) == BR._zero_row(BR.TOO_LARGE)
    assert BR.row_dict(br.rows[1]) == dict(status=BR.OK, area=524288, bbox=[0, 0, 512, 1024], flags=0xF0, n_seed=104 * 14,
                                           sum_x=1024 * (511 * 512 // 2), sum_y=512 * (1023 * 1024 // 2))
    rows, bits = br.to_host()
    assert len(bits) == 8192 and (bits == np.uint64(2 ** 64 - 1)).all() and br.center[1].tolist() == [255, 511]
    with pytest.raises(ValueError):
        br.mask(0)
    assert bool(br.mask(1).all())


# ---- 2. the entry point with the test's own buffers ------------------------------------------------------------------------------

def test_every_owned_word_is_written_once_and_nothing_else_is_touched():
    """`ctd_balloon_regions` through ctypes: the bit buffer is pre-filled with 0xA5 and laid out by the test with guard words in
    front, between the blocks and behind; the erase rows are the restatement's, uploaded.  Every owned word of an OK or
    NOT_PLAIN block equals the restatement's, every guard word and the bytes around the row table still hold 0xA5."""
    p = pkg()
    B, E, L = p.balloons, p.erase, p._lib
    dev = torch.device("cuda:0")
    material = [m for m in _material() if len(m[2])][:2] + [status_page(), connectivity_page()]
    ref = [BR.balloon_page(page, mask, boxes) for page, mask, boxes in material]
    pages, masks = [torch.from_numpy(m[0]).to(dev) for m in material], [torch.from_numpy(m[1]).to(dev) for m in material]
    n = sum(len(m[2]) for m in material)
    jobs = np.zeros((n,), B.JOB_DTYPE)
    erows = np.zeros((n,), E.ROW_DTYPE)
    pt = np.zeros((len(material),), E.PAGE_DTYPE)
    k, at, layout, max_words = 0, 3, [], 0
    for i, ((page, mask, boxes), (rows, words, wins, er)) in enumerate(zip(material, ref)):
        pt[i]["page_dev"], pt[i]["mask_dev"] = pages[i].data_ptr(), masks[i].data_ptr()
        pt[i]["H"], pt[i]["W"], pt[i]["pitch"], pt[i]["mask_pitch"] = page.shape[0], page.shape[1], pages[i].stride(0), masks[i].stride(0)
        for b, w, e in zip(boxes, words, er):
            jobs[k]["page"], jobs[k]["xyxy"], jobs[k]["erase_row"], jobs[k]["word0"] = i, b, n - 1 - k, at   # rows in another order
            for f in ER.FIELDS:
                erows[n - 1 - k][f] = e[f]
            layout.append((at, w))
            at += len(w) + 1 + k % 3                               # 1 .. 3 guard words behind every block
            max_words = max(max_words, len(w))
            k += 1
    total = at + 2
    tab = torch.from_numpy(np.concatenate([jobs.view(np.uint8), pt.view(np.uint8), erows.view(np.uint8)])).to(dev)
    bits = torch.full((total * 8,), 0xA5, dtype=torch.uint8, device=dev)
    rows_dev = torch.full((64 + n * 48 + 64,), 0xA5, dtype=torch.uint8, device=dev)
    prm = L.CtdBalloonParams(2, 12, 8, 32, max_words)
    o_pages, o_rows = n * 32, n * 32 + len(material) * 72
    L.check(L.lib().ctd_balloon_regions(tab.data_ptr(), n, tab.data_ptr() + o_pages, len(material), tab.data_ptr() + o_rows,
                                        C.byref(prm), rows_dev.data_ptr() + 64, bits.data_ptr(), None), "ctd_balloon_regions")
    torch.cuda.synchronize()
    got_bits = bits.cpu().numpy().view(np.uint64)
    got_rows = rows_dev.cpu().numpy()
    assert (got_rows[:64] == 0xA5).all() and (got_rows[-64:] == 0xA5).all()
    rows = got_rows[64:-64].view(B.ROW_DTYPE)
    want_rows = [r for rf in ref for r in rf[0]]
    assert [BR.row_dict(r) for r in rows] == want_rows
    guard = np.ones((total,), bool)
    for at, w in layout:
        assert np.array_equal(got_bits[at: at + len(w)], w), at
        guard[at: at + len(w)] = False
    assert guard.sum() >= n + 5 and (got_bits[guard] == np.uint64(0xA5A5A5A5A5A5A5A5)).all()
    # a block larger than the call's max_words is refused, not computed: nothing of the buffer is touched
    bits.fill_(0xA5)
    prm = L.CtdBalloonParams(2, 12, 8, 32, 16)
    L.check(L.lib().ctd_balloon_regions(tab.data_ptr(), n, tab.data_ptr() + o_pages, len(material), tab.data_ptr() + o_rows,
                                        C.byref(prm), rows_dev.data_ptr() + 64, bits.data_ptr(), None), "ctd_balloon_regions")
    torch.cuda.synchronize()
    rows = rows_dev.cpu().numpy()[64:-64].view(B.ROW_DTYPE)
    assert [int(r["status"]) for r in rows] == [BR.TOO_LARGE if w["status"] == BR.OK else BR.NOT_PLAIN for w in want_rows]
    small = np.ones((total,), bool)
    for at, w in layout:
        if len(w) <= 16:
            small[at: at + len(w)] = False
    assert (bits.cpu().numpy().view(np.uint64)[small] == np.uint64(0xA5A5A5A5A5A5A5A5)).all()


# ---- 3. through the detector ---------------------------------------------------------------------------------------------------

def test_detector_balloons_equals_the_restatement():
    """`det.balloons(pages, det.detect_batch(pages))` against the restatement on the same masks and boxes, for host and device
    pages, with and without `erased=`."""
    p, det = pkg(), TG.detector()
    pages = [p.synth.text_like_page((256, 256), 3, n_blocks=4), p.synth.text_like_page((200, 300), 4, n_blocks=2),
             p.synth.text_like_page((256, 256), 5, n_blocks=3)]
    results = det.detect_batch(pages)
    assert sum(len(r[2]) for r in results) >= 4
    material = [(pg, r[1], [[int(v) for v in b.xyxy] for b in r[2]]) for pg, r in zip(pages, results)]
    br = det.balloons(pages, results)
    want = _compare(br, material, [BR.balloon_page(*m) for m in material])
    print(f"\nstatuses {[w['status'] for w in want]}, areas {[w['area'] for w in want]}")
    assert len(want) == sum(len(r[2]) for r in results)
    er = det.erase_text(pages, results, grow=3)
    other = det.balloons([torch.from_numpy(x).cuda() for x in pages], results, erased=er, grow=3, reach=4)
    _compare(other, material, [BR.balloon_page(*m, grow=3, reach=4) for m in material])
    with pytest.raises(ValueError):
        det.balloons(pages, results, reach_min=7)


# ---- 4. bad arguments --------------------------------------------------------------------------------------------------------

def test_bad_arguments_are_refused_without_a_launch():
    p = pkg()
    B, E, L = p.balloons, p.erase, p._lib
    dev = torch.device("cuda:0")
    page = torch.full((40, 60, 3), 200, dtype=torch.uint8, device=dev)
    mask = torch.zeros((40, 60), dtype=torch.uint8, device=dev)
    mask[18:22, 20:40] = 255
    blk = _Blk((20, 18, 40, 22))
    for bad in (dict(grow=-1), dict(grow=9), dict(tol=-1), dict(tol=256), dict(reach=-1), dict(reach=33), dict(reach_min=7),
                dict(reach_min=1025)):
        with pytest.raises(ValueError):
            B.balloon_regions([page], [mask], [[blk]], **bad)
    for pg, mk in ((page[:, :, 0], mask), (page, mask[:, :59]), (page.int(), mask), (page, mask[:39])):
        with pytest.raises(ValueError):
            B.balloon_regions([pg], [mk], [[blk]])
    with pytest.raises(ValueError):
        B.balloon_regions([page, page], [mask], [[blk], []])
    er = E.erase_text([page, page], [mask, mask], [[blk], [blk]])
    with pytest.raises(ValueError):                                             # an `erased` of another length
        B.balloon_regions([page], [mask], [[blk]], erased=er)
    with pytest.raises(ValueError):                                             # ... and one made with another grow
        B.balloon_regions([page], [mask], [[blk]], erased=E.erase_text([page], [mask], [[blk]], grow=3))
    assert B.balloon_regions([page], [mask], [[blk]], erased=E.erase_text([page], [mask], [[blk]])).ok.tolist() == [True]
    none = B.balloon_regions([page], [mask], [[]])                              # a page without blocks: nothing launched
    assert len(none) == 0 and len(none.bits) == 0
    lib = L.lib()
    prm = L.CtdBalloonParams(2, 12, 8, 32, 8)
    assert lib.ctd_balloon_regions(8, 1, 8, 1, 8, C.byref(prm), 8, None, None) != L.OK          # words to write and no buffer
    assert lib.ctd_balloon_regions(8, 1, 8, 1, None, C.byref(prm), 8, 8, None) != L.OK
    assert lib.ctd_balloon_regions(8, 1, 8, 1, 8, C.byref(prm), None, 8, None) != L.OK
    torch.cuda.synchronize()
