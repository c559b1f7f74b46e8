"""-m gpu: the group and chunk walk (csrc/glyph_walk.h) at its boundaries, through both kernels that use it -- `glyphs_kernel`
(csrc/kernels_glyphs.hip) and, at (c, s) = (65536, 0), `tilted_kernel` (csrc/kernels_tilted.hip) -- and seeded random scenes
through both typeset kernels.  The material is tests/typeset_cases.py (what each case is there for is asserted without a GPU in
tests/test_typeset_cases.py): run ends at, below and above every wave and chunk boundary, a run that ends the entries at a
chunk's end, a max across two chunks, a chunk that contributes nothing (raw tables), a multi-chunk group over both seams with a
clip at r = 12, patch rows that make one gather batch, one batch and a row, and two, and all 13 radii stacked on the same
pixels.  The oracles are those of tests/test_gpu_glyphs.py, whose helpers are imported: the restatement tests/glyph_ref.py for
every page byte, both row fields and the status, and the bitmap kernel on the composed bitmaps.  Everything is EXACT."""
import numpy as np
import pytest
import torch

import glyph_ref as GR
import test_gpu_glyphs as GT
import typeset_cases as TC
import typeset_ref as TR
from conftest import pkg

pytestmark = pytest.mark.gpu


def _bitmap_status(bl, pages):
    return [TR.status_of(ly, *pages[ly["page"]].shape[:2]) for ly in bl]


# ---- the API path ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", [name for name, _, _ in TC.API_CASES])
def test_walk_case_equals_both_oracles_in_every_byte(name):
    """One `typeset_glyphs` call on the case against the restatement (pages, rows, status) and the bitmap kernel (pages)."""
    p = pkg()
    pages, bitmaps, layers, places = TC.case(name)
    want, want_rows, bl = TC.reference(name)
    tp, w2, r2, _ = GT._both(p, pages, layers, places, bitmaps)
    assert not GT._same(w2, want) and np.array_equal(r2, want_rows)       # `_both` compared with the same restatement
    assert tp.status.tolist() == TC.statuses(name) == [TR.OK] * len(layers)
    assert want_rows[:, 0].min() > 0


@pytest.mark.parametrize("name", [name for name, _, _ in TC.API_CASES])
def test_walk_case_through_the_tilted_kernel_equals_the_restatement_in_every_byte(name):
    """The same case as one `typeset_glyphs` call that `tilted_kernel` serves at (c, s) = (65536, 0) (`TC.tilted`), where the
    rule gives `ctd_typeset_glyphs`' bytes: every page byte, both row fields of the case's own layers and the status against the
    same restatement.  That its tiles still hold the entry counts the case is there for: tests/test_typeset_cases.py."""
    p = pkg()
    pages, bitmaps, _, places = TC.case(name)
    want, want_rows, _ = TC.reference(name)
    layers, angle, pivot = TC.tilted(name)
    tp = p.glyphs.typeset_glyphs(pages, GT._atlas(p, bitmaps), angle=angle, pivot=pivot, **GT._args(pages, layers, places))
    got = tp.to_host()
    assert not GT._same(got, want), f"pages {GT._same(got, want)} differ from the restatement"
    rows = np.stack([tp.n_fill, tp.n_stroke], axis=1)
    assert np.array_equal(rows[:-1], want_rows) and not rows[-1].any() and want_rows[:, 0].min() > 0
    assert tp.status.tolist() == TC.statuses(name) + [p._lib.TYPESET_EMPTY] == [TR.OK] * (len(layers) - 1) + [TR.EMPTY]


# ---- the raw path: a chunk that contributes nothing ----------------------------------------------------------------------------------

def _idle_chunk(name, tilted):
    p = pkg()
    host, bitmaps, layers, places = TC.case(name)
    want, want_rows, _ = TC.reference(name)
    pages = [torch.from_numpy(pg).cuda() for pg in host]
    rows = GT._raw(p, pages, layers, places, bitmaps, tilted=tilted)
    got = [pg.cpu().numpy() for pg in pages]
    assert not GT._same(got, want), f"pages {GT._same(got, want)} differ from the restatement"
    assert np.array_equal(rows, want_rows) and rows[0, 1] > rows[0, 0] > 1000


@pytest.mark.parametrize("name", [name for name, _, _ in TC.RAW_CASES])
def test_a_chunk_that_contributes_nothing_to_its_tile(name):
    """`ctd_typeset_glyphs` through ctypes with EVERY placement listed in EVERY tile: in each tile one of the layer's two
    chunks stages nothing that contributes.  Pages and rows against the restatement; the guard bytes behind the rows are
    checked by `_raw`."""
    _idle_chunk(name, tilted=False)


@pytest.mark.parametrize("name", [name for name, _, _ in TC.RAW_CASES])
def test_a_chunk_that_contributes_nothing_to_its_tile_through_the_tilted_kernel(name):
    """The same through `ctd_typeset_tilted`: the same every-placement-in-every-tile tables, a `ctd_tilt_layer` table at
    (c, s) = (65536, 0), the same guard bytes behind the rows, the same restatement."""
    _idle_chunk(name, tilted=True)


# ---- every radius back to back, through the bitmap kernel too ----------------------------------------------------------------------

def test_radius_ladder_through_the_bitmap_kernel():
    """The composed bitmaps of `radius_ladder` through `typeset_pages` against `typeset_ref.typeset`: pages, rows, status."""
    p = pkg()
    pages, bitmaps, layers, places = TC.case("radius_ladder")
    _, _, bl = TC.reference("radius_ladder")
    assert [ly["r"] for ly in bl] == list(TC.LADDER)
    want, want_rows = TR.typeset(pages, bl)
    tp = GT._bitmap_api(p, pages, bl)
    got = tp.to_host()
    assert not GT._same(got, want), "the page differs from the restatement"
    assert np.array_equal(np.stack([tp.n_fill, tp.n_stroke], axis=1), want_rows) and tp.status.tolist() == _bitmap_status(bl, pages)
    assert not GT._same(got, TC.reference("radius_ladder")[0])


# ---- the sweep ---------------------------------------------------------------------------------------------------------------

def _rows_of(tp):
    return np.stack([tp.n_fill, tp.n_stroke], axis=1)


def test_random_scenes_through_both_kernels():
    """Every seed of `typeset_cases.SEED_CASES` through the glyph kernel and, as composed bitmaps, through the bitmap kernel,
    against the restatement: pages, rows, status.  Even seeds run on fresh device pages; odd seeds run `inplace=True` on views
    at an odd offset and an odd pitch inside a buffer of guard bytes, and the WHOLE buffer is compared, so a write between the
    rows of a page or beyond one fails."""
    p = pkg()
    for seed, (name, _, _) in enumerate(TC.SEED_CASES):
        pages, bitmaps, layers, places = TC.case(name)
        want, want_rows, bl = TC.reference(name)
        atlas = GT._atlas(p, bitmaps)
        kw = GT._args(pages, layers, places)
        if seed % 2 == 0:
            tp = p.glyphs.typeset_glyphs(pages, atlas, **kw)
            tb = GT._bitmap_api(p, pages, bl)
            for what, t in (("glyph", tp), ("bitmap", tb)):
                assert not GT._same(t.to_host(), want), f"{name}: {what} kernel, pages {GT._same(t.to_host(), want)} differ"
        else:
            for what in ("glyph", "bitmap"):
                host, expect, buf, views = GT._odd_views(pages, want)
                if what == "glyph":
                    t = tp = p.glyphs.typeset_glyphs(views, atlas, inplace=True, **kw)
                else:
                    t = tb = GT._bitmap_api(p, views, bl, inplace=True)
                assert all(a.data_ptr() == v.data_ptr() for a, v in zip(t.pages, views)), name
                bad = np.flatnonzero(buf.cpu().numpy() != expect)
                assert not len(bad), f"{name}: {what} kernel, {len(bad)} bytes of the buffer differ, first at {bad[:5]}"
        assert np.array_equal(_rows_of(tp), want_rows), f"{name}: glyph kernel rows"
        assert np.array_equal(_rows_of(tb), want_rows), f"{name}: bitmap kernel rows"
        assert tp.status.tolist() == TC.statuses(name), f"{name}: glyph status"
        assert tb.status.tolist() == _bitmap_status(bl, pages), f"{name}: bitmap status"
        atlas.close()
