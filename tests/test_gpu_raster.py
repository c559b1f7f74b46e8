"""-m gpu: glyph outlines rasterised into the atlas -- `ctd_rasterise_glyphs` (csrc/kernels_raster.hip), `glyphs.OutlineFont`,
`GlyphAtlas.rasterise`, `TextDetector.typeset_text` -- against the numpy restatement of the rule (tests/raster_ref.py).
Integers only, so every comparison is EXACT: every byte of every record, and every guard byte between the records.  The raw
entry point is driven through ctypes with records laid out at odd offsets with guard bytes between them; the launch-shape
constants of `_lib` (band height, chunk width, segments a staging pass, workgroups a job) put sizes on both sides of every
boundary the kernel has."""
import numpy as np
import pytest
import torch

import raster_ref as RR
import test_gpu_regions as TG
from conftest import pkg

pytestmark = pytest.mark.gpu

GUARD, GAP = 0xA5, 5
ONE = 65536


def quad(w, h):
    """Four slanted edges whose box at a pixel a unit is exactly w x h."""
    return RR.polygon([(0, 0), (w, min(1, h)), (max(w - 1, 0), h), (min(1, w), max(h - 1, 0))])


def ngon(n, rx=300, ry=200):
    """n straight segments around an ellipse."""
    a = np.arange(n) * 2 * np.pi / n
    return RR.polygon(np.stack([400 + rx * np.cos(a), 300 + ry * np.sin(a)], 1).round().astype(np.int64))


def _jobs(G, outlines, inst):
    """The job table the host would make for inst = [(glyph, S)], records GAP guard bytes apart from byte 3 on: (jobs,
    n_bytes, references)."""
    first = np.cumsum([0] + [len(o) for o in outlines])
    jobs, refs, at = np.zeros((len(inst),), G.RASTER_JOB_DTYPE), [], 3
    for i, (g, S) in enumerate(inst):
        cov, bx, by = RR.rasterise(outlines[g], S)
        h, w = cov.shape
        jobs[i] = (at, w, h, bx, by, first[g], len(outlines[g]), S, 0)
        refs.append(cov)
        at += w * h + GAP
    return jobs, at, refs


def _launch(p, outlines, jobs, n_bytes, n_segs=None, atlas_bytes=None):
    """`ctd_rasterise_glyphs` on a buffer of guard bytes: (buffer, status)."""
    L = p._lib
    segs = np.concatenate([np.asarray(o, np.int32).reshape(-1, 6) for o in outlines] + [np.zeros((1, 6), np.int32)])
    dev = torch.device("cuda")
    segs_dev = torch.from_numpy(segs).to(dev)
    jobs_dev = torch.from_numpy(jobs.view(np.uint8).copy()).to(dev)
    buf = torch.full((n_bytes,), GUARD, dtype=torch.uint8, device=dev)
    status = torch.full((len(jobs),), -7, dtype=torch.int32, device=dev)
    st = torch.cuda.current_stream()
    L.check(L.lib().ctd_rasterise_glyphs(segs_dev.data_ptr(), len(segs) - 1 if n_segs is None else n_segs, jobs_dev.data_ptr(),
                                         len(jobs), buf.data_ptr(), n_bytes if atlas_bytes is None else atlas_bytes,
                                         status.data_ptr(), st.cuda_stream), "ctd_rasterise_glyphs")
    st.synchronize()
    return buf.cpu().numpy(), status.cpu().numpy()


def _exact(p, outlines, inst):
    """Every byte of the buffer -- records and guards -- and every status against the restatement.  Returns the references."""
    jobs, n_bytes, refs = _jobs(p.glyphs, outlines, inst)
    got, status = _launch(p, outlines, jobs, n_bytes)
    want = np.full((n_bytes,), GUARD, np.uint8)
    for j, cov in zip(jobs, refs):
        want[int(j["off"]): int(j["off"]) + cov.size] = cov.ravel()
    want_status = [RR.EMPTY if (c.size == 0 or len(outlines[g]) == 0) else RR.OK for c, (g, _) in zip(refs, inst)]
    assert status.tolist() == want_status
    bad = np.flatnonzero(got != want)
    if len(bad):
        i = int(np.searchsorted(jobs["off"], bad[0], side="right")) - 1
        o = int(bad[0] - jobs["off"][i])
        w = max(int(jobs["w"][i]), 1)
        raise AssertionError(f"{len(bad)} bytes differ, the first in job {i} {inst[i]} ({jobs['w'][i]} x {jobs['h'][i]}) at row {o // w}, "
                             f"column {o % w}: {got[bad[0]]} for {want[bad[0]]}")
    return refs


# ---- 1. shapes -----------------------------------------------------------------------------------------------------------------

def test_hand_made_shapes_equal_the_restatement_in_every_byte():
    p = pkg()
    ring = np.concatenate([RR.rect(0, 0, 20, 20), RR.rect(5, 5, 15, 15, cw=True)])
    two = np.concatenate([RR.rect(0, 0, 12, 8), RR.rect(6, 4, 20, 14)])
    flat = np.array([RR.line((0, 0), (10, 0)), RR.line((10, 0), (0, 0))], np.int32)
    outlines = [RR.rect(2, 3, 12, 8), RR.rect(1, 1, 11, 7), RR.rect(1, 1, 11, 7, cw=True), RR.blob(), RR.blob(cw=True), ring, two,
                RR.rect(0, 0, 1, 1), RR.rect(1, 1, 3, 3), flat, np.zeros((0, 6), np.int32), RR.rect(-7, -4, -1, 9)]
    inst = [(0, ONE), (1, ONE // 4), (2, ONE // 4), (3, RR.scale_of(24, 1000)), (4, RR.scale_of(24, 1000)), (5, ONE), (6, ONE),
            (7, ONE), (8, ONE // 8), (9, ONE), (10, ONE), (11, ONE), (3, RR.scale_of(61, 1000))]
    refs = _exact(p, outlines, inst)
    assert (refs[0] == 255).all() and refs[1].tolist() == [[143, 191, 143], [143, 191, 143]]
    assert np.array_equal(refs[1], refs[2]) and np.array_equal(refs[3], refs[4])
    assert (refs[5][5:15, 5:15] == 0).all() and refs[7].tolist() == [[255]]
    assert refs[8].shape == (1, 1) and 0 < refs[8][0, 0] < 32                # a glyph smaller than a pixel: 1/16 of one
    assert refs[9].shape == (0, 10) and refs[10].shape == (0, 0)            # horizontal edges only; a space


def test_a_curve_at_each_flatten_level_and_one_glyph_at_six_scales():
    p = pkg()
    refs = _exact(p, [RR.arch()], [(0, S) for S in RR.ARCH_SCALE_OF_LEVEL])
    assert [r.shape for r in refs[3:]] == [(8, 8), (32, 32), (200, 200)]
    rng = np.random.default_rng(3)
    sg = RR.random_outline(rng, contours=3)
    _exact(p, [sg], [(0, RR.scale_of(s, 1000)) for s in (5, 11, 24, 47, 96, 333)])


def test_sides_and_segment_counts_on_both_sides_of_every_boundary():
    """Heights around the band height and around one round of a job's workgroups; widths around the chunk width, twice it,
    and the scan's quarters of it; segment counts around one and two staging passes."""
    p = pkg()
    L = p._lib
    bh, cw, sc, by = L.RASTER_BAND_H, L.RASTER_CHUNK_W, L.RASTER_SEG_CHUNK, L.RASTER_BANDS_Y
    assert (bh, cw, sc, by) == (4, 128, 32, 8)
    hs = sorted({v + d for v in (bh, 2 * bh, bh * by, 2 * bh * by) for d in (-1, 0, 1)})
    ws = sorted({v + d for v in (cw // 4, cw // 2, cw, 2 * cw) for d in (-1, 0, 1)})
    outlines = [quad(37, h) for h in hs] + [quad(w, 9) for w in ws] + [quad(cw + 1, bh * by + 1), quad(2 * cw, 2 * bh * by)]
    refs = _exact(p, outlines, [(g, ONE) for g in range(len(outlines))])
    assert [r.shape[0] for r in refs[:len(hs)]] == hs and [r.shape[1] for r in refs[len(hs):len(hs) + len(ws)]] == ws
    counts = sorted({v + d for v in (sc, 2 * sc) for d in (-1, 0, 1)}) + [3, 5 * sc + 7]
    outlines = [ngon(n) for n in counts]
    assert [len(o) for o in outlines] == counts
    _exact(p, outlines, [(g, RR.scale_of(s, 1000)) for g in range(len(outlines)) for s in (20, 260)])


def test_edges_left_of_a_chunk_feed_its_carry():
    p = pkg()
    cw = p._lib.RASTER_CHUNK_W
    wide = RR.rect(0, 0, 2 * cw + 44, 10)                  # the middle chunk holds no edge at all: it is all carry
    spike = np.concatenate([RR.rect(0, 0, 20, 10), [RR.line((20, 0), (2 * cw + 44, 0)), RR.line((2 * cw + 44, 0), (20, 0))]]).astype(np.int32)
    slant = RR.polygon([(0, 0), (3 * cw, 0), (3 * cw, 20), (cw // 2, 20)])           # the left edge crosses the first chunk only
    refs = _exact(p, [wide, spike, slant], [(0, ONE), (1, ONE), (2, ONE), (2, ONE // 2 + 77)])
    assert (refs[0] == 255).all() and refs[1].shape == (10, 2 * cw + 44)
    assert (refs[1][:, :20] == 255).all() and not refs[1][:, 20:].any()     # every edge left of the last two chunks; they cancel
    assert (refs[2][:, cw:] == 255).all() and refs[2][10, 0] == 0


def test_one_instance_of_the_largest_side():
    p = pkg()
    n = p._lib.RASTER_MAX_SIDE
    big = np.concatenate([quad(n, n), RR.blob(8, 400, (512, 512), cw=True)])
    refs = _exact(p, [big], [(0, ONE)])
    assert refs[0].shape == (n, n) and refs[0][512, 512] == 0 and refs[0][512, 60] == 255


def test_300_seeded_instances_of_mixed_sizes_in_one_launch():
    p = pkg()
    rng = np.random.default_rng(77)
    outlines = [RR.random_outline(rng) for _ in range(60)] + [np.zeros((0, 6), np.int32)]
    sizes = (6, 9, 12, 17, 24, 33, 48, 70, 140)
    inst = [(int(rng.integers(0, len(outlines))), RR.scale_of(sizes[int(rng.integers(0, len(sizes)))], 1000)) for _ in range(300)]
    refs = _exact(p, outlines, inst)
    assert sum(r.size for r in refs) > 200000 and max(r.shape[1] for r in refs) > p._lib.RASTER_CHUNK_W // 2


# ---- 2. what the kernel must refuse ------------------------------------------------------------------------------------------

def test_broken_jobs_among_good_ones_write_nothing():
    """Range, offset, side and scale: each broken job is REFUSED and writes nothing, the good ones around them are exact, and
    a wrong box (bx, by) with honest sides costs pixels and faults nothing: it stays inside its record."""
    p = pkg()
    G = p.glyphs
    rng = np.random.default_rng(5)
    outlines = [RR.random_outline(rng) for _ in range(6)]
    n_segs = sum(len(o) for o in outlines)
    inst = [(g % 6, RR.scale_of(30, 1000)) for g in range(16)]
    jobs, n_bytes, refs = _jobs(G, outlines, inst)
    breaks = {1: ("seg_first", -1), 2: ("seg_count", -1), 3: ("seg_first", n_segs), 4: ("seg_count", n_segs + 1), 5: ("off", -1),
              6: ("off", n_bytes - 10), 7: ("off", n_bytes + 1), 8: ("w", 1025), 9: ("h", -1), 10: ("h", 1025), 11: ("scale", 0),
              12: ("scale", (1 << 22) + 1), 13: ("scale", -5)}
    for i, (f, v) in breaks.items():
        jobs[f][i] = v
    got, status = _launch(p, outlines, jobs, n_bytes)
    want = np.full((n_bytes,), GUARD, np.uint8)
    honest = _jobs(G, outlines, inst)[0]
    for i, cov in enumerate(refs):
        if i not in breaks:
            want[int(honest["off"][i]): int(honest["off"][i]) + cov.size] = cov.ravel()
    assert status.tolist() == [RR.REFUSED if i in breaks else RR.OK for i in range(16)]
    assert np.array_equal(got, want)
    # the segment count and the atlas size are the call's: a shorter one refuses what it cuts off
    jobs = honest.copy()
    got, status = _launch(p, outlines, jobs, n_bytes, n_segs=n_segs - 1, atlas_bytes=int(jobs["off"][15]) + refs[15].size - 1)
    assert status.tolist() == [RR.REFUSED if i in (5, 11, 15) else RR.OK for i in range(16)]      # glyph 5 holds the last segment
    assert (got[int(jobs["off"][15]):] == GUARD).all() and (got[int(jobs["off"][5]): int(jobs["off"][6])] == GUARD).all()
    # a wrong box: pixels, not faults; the guards stand
    jobs = honest.copy()
    jobs["bx"][0] += 9
    jobs["by"][1] -= 300
    jobs["bx"][2] = -(1 << 31)
    jobs["by"][3] = (1 << 31) - 1
    got, status = _launch(p, outlines, jobs, n_bytes)
    assert (status == RR.OK).all()
    want[:] = GUARD
    for i, cov in enumerate(refs):
        want[int(honest["off"][i]): int(honest["off"][i]) + cov.size] = cov.ravel()
    rec = np.zeros((n_bytes,), bool)
    for i in range(4):
        rec[int(honest["off"][i]): int(honest["off"][i]) + refs[i].size] = True
    assert np.array_equal(got[~rec], want[~rec])


# ---- 3. the atlas --------------------------------------------------------------------------------------------------------------

def _font(G, n=20, seed=9):
    rng = np.random.default_rng(seed)
    outlines = [RR.random_outline(rng) for _ in range(n - 1)] + [np.zeros((0, 6), np.int32)]
    font = G.OutlineFont(1000, 800, 200)
    font.add(outlines[:7], [int(a) for a in rng.integers(300, 900, 7)])
    font.add(outlines[7:], [int(a) for a in rng.integers(300, 900, n - 8)] + [350])       # the device buffer is appended to
    return font, outlines


def _atlas_bytes(atlas):
    return atlas._cov[:atlas.nbytes].cpu().numpy()


def test_rasterise_appends_caches_and_grows_the_atlas():
    p = pkg()
    G = p.glyphs
    font, outlines = _font(G)
    atlas = G.GlyphAtlas()
    first = [np.full((3, 5), 200, np.uint8), np.zeros((0, 0), np.uint8)]
    assert atlas.add(first).tolist() == [0, 1]
    gids = [4, 19, 0, 4, 11]
    ids = atlas.rasterise(font, gids, 24)
    assert ids.dtype == np.int32 and ids.tolist() == [2, 3, 4, 2, 5] and len(atlas) == 6
    S = RR.scale_of(24, 1000)
    refs = [RR.rasterise(outlines[g], S) for g in (4, 19, 0, 11)]
    assert np.array_equal(_atlas_bytes(atlas), np.concatenate([first[0].ravel()] + [r[0].ravel() for r in refs]))
    m = font.metrics([4, 19, 0, 11], 24)
    assert np.array_equal(atlas.sizes[2:], [r[0].shape for r in refs]) and np.array_equal(atlas.sizes[2:], m.sizes)
    assert np.array_equal(atlas.advance[2:], m.advance) and np.array_equal(atlas.bearing[2:], m.bearing)
    rec = atlas._rec[:6 * 16].cpu().numpy().view(G.RECORD_DTYPE)
    assert rec["off"].tolist() == atlas.offsets.tolist() and np.array_equal(np.stack([rec["h"], rec["w"]], 1), atlas.sizes)
    # again: nothing is added; another size, and sizes per gid in one call: only the new instances
    n, nb = len(atlas), atlas.nbytes
    assert atlas.rasterise(font, gids, 24).tolist() == ids.tolist() and (len(atlas), atlas.nbytes) == (n, nb)
    more = atlas.rasterise(font, [4, 4, 0], [24, 40, 40])
    assert more.tolist() == [2, 6, 7] and len(atlas) == 8
    assert np.array_equal(_atlas_bytes(atlas)[nb:], np.concatenate([RR.rasterise(outlines[g], RR.scale_of(40, 1000))[0].ravel() for g in (4, 0)]))
    # grown past its capacity by a rasterise: the bytes before it are kept, the ids stand
    before, cap = _atlas_bytes(atlas).copy(), atlas._cov.numel()
    big = atlas.rasterise(font, np.arange(19), 90)
    assert atlas._cov.numel() > cap and big.tolist() == list(range(8, 27))
    now = _atlas_bytes(atlas)
    assert np.array_equal(now[:len(before)], before)
    assert np.array_equal(now[len(before):], np.concatenate([RR.rasterise(outlines[g], RR.scale_of(90, 1000))[0].ravel() for g in range(19)]))
    other = G.OutlineFont(1000, 800, 200)                   # another font is another instance
    other.add([outlines[4]], [500])
    assert atlas.rasterise(other, [0], 24).tolist() == [27]
    for bad in (dict(gids=[20], size=24), dict(gids=[0], size=0), dict(gids=[0, 1], size=[24, 24, 24]), dict(gids=[0], size=20000)):
        n = len(atlas)
        with pytest.raises(ValueError):
            atlas.rasterise(font, **bad)
        assert len(atlas) == n
    with pytest.raises(ValueError):
        atlas.rasterise(None, [0], 24)


def test_typeset_glyphs_on_rasterised_ids_equals_the_added_reference_bitmaps():
    p = pkg()
    G = p.glyphs
    font, outlines = _font(G)
    rng = np.random.default_rng(31)
    run = rng.integers(0, 20, 40)
    made = G.GlyphAtlas()
    ids = made.rasterise(font, run, 22)
    uniq = np.unique(run)
    m = font.metrics(uniq, 22)
    added = G.GlyphAtlas()
    base = added.add([RR.rasterise(outlines[g], font.scale(22))[0] for g in uniq], advance=m.advance, bearing=m.bearing)
    ids2 = base[np.searchsorted(uniq, run)]
    pages = [np.full((150, 260, 3), 230, np.uint8), np.full((90, 100, 3), 40, np.uint8)]
    out = []
    for atlas, use in ((made, ids), (added, ids2)):
        xy, fits = G.flow(use, atlas, (8, 6, 250, 140), line=m.line, gap=2)
        xy2, _ = G.flow(use[:9], atlas, (-10, 5, 120, 80), line=m.line, vertical=True)
        tp = G.typeset_glyphs(pages, atlas, [0, 1], [0] * 40 + [1] * 9, np.concatenate([use, use[:9]]), np.concatenate([xy, xy2]),
                              fill=(0, 0, 0), stroke=(255, 255, 255), radius=3)
        out.append((tp.to_host(), tp.rows.copy(), xy))
    assert np.array_equal(out[0][2], out[1][2]) and np.array_equal(out[0][2], G.flow_outlines(run, font, (8, 6, 250, 140), 22, gap=2)[0])
    assert all(np.array_equal(a, b) for a, b in zip(out[0][0], out[1][0])) and out[0][1].tobytes() == out[1][1].tobytes()
    assert (out[0][0][0] != pages[0]).sum() > 3000


def test_typeset_text_equals_the_chain_done_by_hand():
    """detect, fill_rest, layout_boxes on the detector's small synthetic pages, then `typeset_text`: the sizes are `fit`'s, the
    positions `flow_outlines`', and the pages are, byte for byte, `typeset_glyphs` on an atlas that was handed the
    restatement's bitmaps through `add`."""
    p, det = pkg(), TG.detector()
    G = p.glyphs
    pages = [p.synth.text_like_page((256, 256), 3, n_blocks=4), p.synth.text_like_page((200, 300), 4, n_blocks=2)]
    results = det.detect_batch(pages)
    fp = det.fill_rest(pages, results)
    lb = det.layout_boxes(pages, results)
    assert len(lb) >= 3 and lb.ok.sum() >= 1
    font, outlines = _font(G)
    rng = np.random.default_rng(14)
    runs = [rng.integers(0, 20, 4 + 2 * j) for j in range(len(lb))]
    if len(lb) > 3:
        runs[3] = None
    sizes = [6, 8, 10, 12, 14, 16, 20, 24]
    atlas = G.GlyphAtlas(device=det.net.device)
    tp = det.typeset_text(fp.pages, lb, font, atlas, runs, sizes, fill=(10, 20, 30), stroke=(255, 250, 245), gap=1)
    idx = [j for j in range(len(lb)) if lb.ok[j] and runs[j] is not None]
    assert tp.layer_of.tolist() == [idx.index(j) if j in idx else -1 for j in range(len(lb))]
    assert len(tp.size) == len(tp.fits) == len(idx) == len(tp)
    hand = G.GlyphAtlas(device=det.net.device)
    glyph, xy, layer = [], [], []
    for i, j in enumerate(idx):
        rect = lb.a_rect[j] if lb.a_area[j] > 0 else lb.rect[j]
        size, fits = G.fit(runs[j], font, rect, sizes, gap=1)
        assert size == tp.size[i] and fits == bool(tp.fits[i])
        scan = [s for s in sizes if G.flow_outlines(runs[j], font, rect, s, gap=1)[1]]
        assert (size, fits) == ((max(scan), True) if scan else (sizes[0], False))
        uniq = np.unique(runs[j])
        m = font.metrics(uniq, size)
        ids = hand.add([RR.rasterise(outlines[g], font.scale(size))[0] for g in uniq], advance=m.advance, bearing=m.bearing)
        glyph.append(ids[np.searchsorted(uniq, runs[j])])
        xy.append(G.flow_outlines(runs[j], font, rect, size, gap=1)[0])
        layer += [i] * len(runs[j])
    assert np.array_equal(np.concatenate(xy), tp.xy)
    want = G.typeset_glyphs(fp.pages, hand, lb.index[idx, 0], layer, np.concatenate(glyph), np.concatenate(xy), fill=(10, 20, 30),
                            stroke=(255, 250, 245), radius=3, device=det.net.device)
    got = tp.to_host()
    assert all(np.array_equal(a, b) for a, b in zip(got, want.to_host())) and tp.rows.tobytes() == want.rows.tobytes()
    assert tp.n_fill.sum() > 0 and any(not np.array_equal(a, b.cpu().numpy()) for a, b in zip(got, fp.pages))
    print(f"\n{len(lb)} blocks, {len(idx)} layers, sizes {tp.size.tolist()}, fits {tp.fits.tolist()}, n_fill {tp.n_fill.tolist()}")
    n = len(atlas)
    det.typeset_text(fp.pages, lb, font, atlas, runs, sizes, fill=(10, 20, 30), stroke=(255, 250, 245), gap=1)
    assert len(atlas) == n                                   # every instance was there already
