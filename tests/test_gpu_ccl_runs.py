"""-m gpu: `launch_ccl_dual` on row runs (csrc/kernels_post.hip) through `backend.connected_components_dual` on
the pages of tests/ccl_runs_emul.py, several different pages per call: the signed label plane, both counts, the statistics and
the first pixels exactly as the oracle's `connected_components_with_stats` has them (8-connected foreground, 4-connected
background).  That the same formulation in numpy gives these is checked without a GPU in tests/test_ccl_runs_emul.py."""
import numpy as np
import pytest
import torch

import ccl_runs_emul as E
from conftest import pkg

pytestmark = pytest.mark.gpu


def run_call(pages, max_labels, thresh=0):
    """One call on `pages` = [(name, (H, W) bool)] of one shape; the mismatches against the oracle as a list of strings."""
    imgs = np.stack([fg for _, fg in pages]).astype(np.uint8) * 255
    labels, n, st, fi = pkg().backend.connected_components_dual(torch.from_numpy(imgs).cuda(), thresh, max_labels=max_labels)
    torch.cuda.synchronize()
    lab = labels.cpu().numpy()
    n, st, fi = [a.cpu().numpy() for a in n], [a.cpu().numpy() for a in st], [a.cpu().numpy() for a in fi]
    bad = []
    for b, (name, fg) in enumerate(pages):
        ref = E.reference(fg)
        for c, sign in enumerate((1, -1)):
            nref, lref, sref = ref[sign]
            what = f"{name} {fg.shape[0]} x {fg.shape[1]}, class {sign}"
            if int(n[c][b]) != nref:
                bad.append(f"{what}: {int(n[c][b])} components, the oracle has {nref}")
                continue
            if not np.array_equal(np.maximum(sign * lab[b], 0), lref):
                bad.append(f"{what}: {int((np.maximum(sign * lab[b], 0) != lref).sum())} labels differ")
            k = min(nref, max_labels)
            if not np.array_equal(st[c][b, :k], sref[:k]):
                bad.append(f"{what}: statistics differ in rows {np.nonzero((st[c][b, :k] != sref[:k]).any(axis=1))[0][:5]}")
            flat = lref.ravel()
            # the first pixel of label l in raster order: where the running maximum of the plane first reaches l
            want = np.searchsorted(np.maximum.accumulate(flat), np.arange(1, k + 1))
            if not np.array_equal(fi[c][b, :k], want):
                bad.append(f"{what}: first pixels differ at labels {np.nonzero(fi[c][b, :k] != want)[0][:5] + 1}")
    return bad


@pytest.mark.parametrize("H", E.HEIGHTS)
def test_every_kind_of_page_at_every_width(H):
    bad = []
    for (h, W), pages in E.small_calls():
        if h == H:
            bad += run_call(pages, max_labels=max(1, H * W))
    assert not bad, "\n".join(bad[:20])


def test_bands_over_the_table_next_to_sparse_pages():
    """64 x 1024 of alternating pixels (both bands have 32 768 runs and go through global memory) stacked with sparse pages
    and the mirrored pattern; then 96 x 1024 with only the middle band over the capacity."""
    alt = np.broadcast_to(np.arange(1024) % 2 == 0, (64, 1024)).copy()
    pages = [("sparse", E.noise(64, 1024, 0.02, 1)), ("alternating", alt), ("blobs", E.noise(64, 1024, 0.3, 2)),
             ("alternating, odd", ~alt), ("empty", np.zeros((64, 1024), bool))]
    bad = run_call(pages, max_labels=40000)
    bad += run_call([("band over the capacity", E.over_capacity_page()), ("sparse", E.noise(96, 1024, 0.05, 3)),
                     ("band over the capacity, other seed", E.over_capacity_page(seed=6))], max_labels=4096)
    assert not bad, "\n".join(bad[:20])


def test_max_labels_below_the_component_count():
    """Rows beyond max_labels are dropped: the plane and the counts are whole, the tables hold the first max_labels rows."""
    pages = [(name, fg) for name, fg in E.pages_for(65, 131) if name.startswith("noise") or name == "checkerboard"]
    for _, fg in pages:
        assert max(E.reference(fg)[s][0] for s in (1, -1)) > 7
    bad = run_call(pages, max_labels=7)
    assert not bad, "\n".join(bad[:20])


def test_a_threshold_other_than_zero_and_an_unaligned_width():
    """Pixels are compared with the threshold (the DB stage calls with 0 on 0 / 1 bitmaps, the selftest with 127)."""
    rng = np.random.RandomState(4)
    vals = rng.randint(0, 256, (3, 70, 130)).astype(np.uint8)
    labels, (n_f, n_b), _, _ = pkg().backend.connected_components_dual(torch.from_numpy(vals).cuda(), 127, max_labels=4096)
    lab = labels.cpu().numpy()
    for b in range(3):
        ref = E.reference(vals[b] > 127)
        assert int(n_f[b]) == ref[1][0] and int(n_b[b]) == ref[-1][0]
        np.testing.assert_array_equal(np.maximum(lab[b], 0), ref[1][1])
        np.testing.assert_array_equal(np.maximum(-lab[b], 0), ref[-1][1])


def test_one_page_of_blobs_at_1024():
    from scipy import ndimage
    fg = ndimage.uniform_filter(np.random.RandomState(8).rand(1024, 1024), 3) > 0.52
    bad = run_call([("blobs", fg)], max_labels=65536)
    assert not bad, "\n".join(bad)
