"""-m gpu: `launch_ccl_dual` on row runs (csrc/kernels_post.hip) through `backend.connected_components_dual` on
the pages of tests/ccl_runs_emul.py, several different pages per call: the signed label plane, both counts, the statistics and
the first pixels exactly as the oracle's `connected_components_with_stats` has them (8-connected foreground, 4-connected
background).  That the same formulation in numpy gives these is checked without a GPU in tests/test_ccl_runs_emul.py.

`launch_ccl` is one class of the same engine: the same pages through `backend.connected_components` for
connectivity 4 and 8, the workspace contract of `ctd_ccl` / `ctd_ccl_dual` (nothing written beyond
`ctd_ccl_workspace_bytes`, one byte less refused) and the tail's page-by-page labelling of `refine_undetected_mask` on pages
whose word tables are larger than their pixel count suggests."""
import numpy as np
import pytest
import torch

import ccl_runs_emul as E
import tail_trace_cases as T
from conftest import pkg
from oracle import postproc_ref as R
from test_gpu_sweeps import report
from test_gpu_tail_trace import check_call, reference, traced_refine

ERR_INVALID = -1         # CTD_ERR_INVALID of include/ctd_hip.h

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


# ---------------------------------------------------------------------------------------------------------------------------
# launch_ccl: one class of the same engine
# ---------------------------------------------------------------------------------------------------------------------------
_SINGLE_REF = {}


def single_reference(fg, conn):
    """The oracle's (n, labels, stats rows 1..n) of one page, computed once per page and connectivity and only read."""
    key = (fg.shape, fg.tobytes(), conn)
    if key not in _SINGLE_REF:
        n, lab, st = R.connected_components_with_stats(fg.astype(np.uint8) * 255, conn)
        _SINGLE_REF[key] = (n - 1, lab, st[1:])
    return _SINGLE_REF[key]


def compare_single(what, fg, conn, lab, n, st, max_labels):
    nref, lref, sref = single_reference(fg, conn)
    if int(n) != nref:
        return [f"{what}: {int(n)} components, the oracle has {nref}"]
    bad = []
    if not np.array_equal(lab, lref):
        bad.append(f"{what}: {int((lab != lref).sum())} labels differ")
    k = min(nref, max_labels)
    if not np.array_equal(st[:k], sref[:k]):
        bad.append(f"{what}: statistics differ in rows {np.nonzero((st[:k] != sref[:k]).any(axis=1))[0][:5]}")
    return bad


def run_single(pages, conn, max_labels, imgs=None, thresh=0):
    """One `connected_components` call on `pages` = [(name, (H, W) bool)] of one shape (`imgs`: the u8 pages whose
    `> thresh` they are); the mismatches against the oracle."""
    if imgs is None:
        imgs = np.stack([fg for _, fg in pages]).astype(np.uint8) * 255
    labels, n, st = pkg().backend.connected_components(torch.from_numpy(imgs).cuda(), thresh, conn, max_labels=max_labels)
    torch.cuda.synchronize()
    lab, n, st = labels.cpu().numpy(), n.cpu().numpy(), st.cpu().numpy()
    bad = []
    for b, (name, fg) in enumerate(pages):
        bad += compare_single(f"{name} {fg.shape[0]} x {fg.shape[1]}, conn {conn}", fg, conn, lab[b], n[b], st[b], max_labels)
    return bad


@pytest.mark.parametrize("conn", (4, 8))
@pytest.mark.parametrize("H", E.HEIGHTS)
def test_one_class_of_every_kind_of_page_at_every_width(H, conn):
    bad = []
    for (h, W), pages in E.small_calls():
        if h == H:
            bad += run_single(pages, conn, max_labels=max(1, H * W))
    assert not bad, "\n".join(bad[:20])


@pytest.mark.parametrize("conn", (4, 8))
def test_one_class_with_a_band_over_the_table(conn):
    """96 x 1024 with only the middle band over RB_CAP, next to a sparse page; then batches of 1 and of 5 of one shape."""
    bad = run_single([("band over the capacity", E.over_capacity_page()), ("sparse", E.noise(96, 1024, 0.05, 3))], conn, max_labels=4096)
    pages = [(f"noise {d}", E.noise(70, 130, d, 20 + i)) for i, d in enumerate((0.1, 0.3, 0.5, 0.6, 0.85))]
    bad += run_single(pages[:1], conn, max_labels=4096)
    bad += run_single(pages, conn, max_labels=4096)
    bad += run_single(pages, conn, max_labels=7)              # rows beyond max_labels dropped, plane and counts whole
    assert not bad, "\n".join(bad[:20])


@pytest.mark.parametrize("conn", (4, 8))
def test_one_class_at_threshold_30_and_a_width_that_is_no_multiple_of_4(conn):
    vals = np.random.RandomState(6).randint(0, 64, (3, 70, 131)).astype(np.uint8)
    bad = run_single([(f"values, page {b}", vals[b] > 30) for b in range(3)], conn, max_labels=4096, imgs=vals, thresh=30)
    assert not bad, "\n".join(bad[:20])


GUARD = 4096


def guarded_workspace(B, H, W):
    """(buffer, ws_bytes): `ctd_ccl_workspace_bytes` bytes followed by GUARD bytes of a pattern."""
    nbytes = pkg()._lib.lib().ctd_ccl_workspace_bytes(B, H, W)
    buf = torch.zeros(nbytes + GUARD, dtype=torch.uint8, device="cuda")
    buf[nbytes:] = 0xA5
    return buf, nbytes


def guard_intact(buf, nbytes):
    return bool((buf[nbytes:] == 0xA5).all())


@pytest.mark.parametrize("shape", ((4096, 1), (2048, 31), (1024, 33), (65, 131)))
def test_ctd_ccl_stays_inside_the_workspace_it_asks_for(shape):
    """`ctd_ccl` with exactly `ctd_ccl_workspace_bytes` inside a larger buffer: exact results, the bytes behind untouched; one
    byte less is refused."""
    lib = pkg()._lib.lib()
    H, W = shape
    B, cap = 2, 4096
    pages = [("noise 0.3", E.noise(H, W, 0.3, H + W)), ("noise 0.6", E.noise(H, W, 0.6, H + W + 1))]
    img = torch.from_numpy(np.stack([fg for _, fg in pages]).astype(np.uint8) * 255).cuda()
    labels = torch.empty((B, H, W), dtype=torch.int32, device="cuda")
    n = torch.empty((B,), dtype=torch.int32, device="cuda")
    st = torch.empty((B, cap, 5), dtype=torch.int32, device="cuda")
    buf, nbytes = guarded_workspace(B, H, W)
    stream = torch.cuda.current_stream().cuda_stream
    bad = []
    for conn in (4, 8):
        rc = lib.ctd_ccl(img.data_ptr(), B, H, W, 0, conn, labels.data_ptr(), n.data_ptr(), st.data_ptr(), cap, buf.data_ptr(),
                         nbytes, stream)
        assert rc == 0, lib.ctd_last_error()
        torch.cuda.synchronize()
        assert guard_intact(buf, nbytes), f"{H} x {W}, conn {conn}: bytes behind the workspace were written"
        for b, (name, fg) in enumerate(pages):
            bad += compare_single(f"{name} {H} x {W}, conn {conn}", fg, conn, labels[b].cpu().numpy(), n[b].cpu().numpy(),
                                  st[b].cpu().numpy(), cap)
        rc = lib.ctd_ccl(img.data_ptr(), B, H, W, 0, conn, labels.data_ptr(), n.data_ptr(), st.data_ptr(), cap, buf.data_ptr(),
                         nbytes - 1, stream)
        assert rc == ERR_INVALID, f"{H} x {W}, conn {conn}: a workspace one byte short returned {rc}"
    assert not bad, "\n".join(bad[:20])


def test_ctd_ccl_dual_stays_inside_the_workspace_it_asks_for():
    lib = pkg()._lib.lib()
    B, H, W, cap = 2, 1024, 33, 8192
    pages = [("noise 0.3", E.noise(H, W, 0.3, 11)), ("noise 0.6", E.noise(H, W, 0.6, 12))]
    img = torch.from_numpy(np.stack([fg for _, fg in pages]).astype(np.uint8) * 255).cuda()
    labels = torch.empty((B, H, W), dtype=torch.int32, device="cuda")
    n = [torch.empty((B,), dtype=torch.int32, device="cuda") for _ in range(2)]
    st = [torch.empty((B, cap, 5), dtype=torch.int32, device="cuda") for _ in range(2)]
    fi = [torch.empty((B, cap), dtype=torch.int32, device="cuda") for _ in range(2)]
    buf, nbytes = guarded_workspace(B, H, W)
    stream = torch.cuda.current_stream().cuda_stream

    def call(ws_bytes):
        return lib.ctd_ccl_dual(img.data_ptr(), B, H, W, 0, labels.data_ptr(), n[0].data_ptr(), n[1].data_ptr(), st[0].data_ptr(),
                                st[1].data_ptr(), fi[0].data_ptr(), fi[1].data_ptr(), cap, buf.data_ptr(), ws_bytes, stream)
    assert call(nbytes) == 0, lib.ctd_last_error()
    torch.cuda.synchronize()
    assert guard_intact(buf, nbytes), "bytes behind the workspace were written"
    lab = labels.cpu().numpy()
    bad = []
    for b, (name, fg) in enumerate(pages):
        for c, (sign, conn) in enumerate(((1, 8), (-1, 4))):
            bad += compare_single(f"{name}, class {sign}", fg if sign > 0 else ~fg, conn, np.maximum(sign * lab[b], 0),
                                  n[c][b].cpu().numpy(), st[c][b].cpu().numpy(), cap)
    assert not bad, "\n".join(bad[:20])
    assert call(nbytes - 1) == ERR_INVALID


def narrow_pages_case():
    """A `keep_undetected_mask` call on two pages of different sizes, 65 and 33 wide: `refine_undetected_mask` labels them page
    by page, and either page has more words per table (80 x 3, 100 x 2) than the larger pixel count / 32 gives (163)."""
    rng = np.random.RandomState(80)
    pages, masks, boxes = [], [], []
    for k, (im_w, im_h, win, blobs) in enumerate(((65, 80, (6, 5, 40, 12), ((5, 36, 30, 14), (40, 55, 21, 20))),
                                                   (33, 100, (3, 4, 20, 10), ((4, 40, 21, 15), (9, 70, 19, 22))))):
        win = win[:3] + (T.open_height(win[2], win[3]),)
        img, mask = T.page_for_windows(im_w, im_h, [win], "noisy", 81 + k)
        img[:, : im_w // 2] = (img[:, : im_w // 2] // 64) * 64
        mask[win[1] + win[3] + 4:, :] = 0
        for x, y, w, h in blobs:
            mask[y: y + h, x: x + w] = rng.randint(100, 256)
            mask[y + 2: y + h - 2: 3, x + 1: x + w - 1: 4] = 20
        pages.append(img), masks.append(mask), boxes.append([T.block_for_window(im_w, im_h, win)])
    return T._case("keep_undetected_mask: two narrow pages of different sizes", pages, masks, boxes, keep=True)


def test_tail_labels_narrow_pages_of_different_sizes_page_by_page():
    """The launcher checks the workspace it is handed against the page's own shape: sized by pixel count this call fails."""
    case = narrow_pages_case()
    shapes = [m.shape for m in case["masks"]]
    assert shapes[0] != shapes[1] and all(w % 32 for _, w in shapes)
    assert all(h * ((w + 31) // 32) > (max(a * b for a, b in shapes) + 31) // 32 for h, w in shapes)
    got = traced_refine(case)
    n, bad = check_call(case, got)
    assert sorted({(r["page"], r["pass_"]) for r in reference(case)[0]}) == [(0, 0), (0, 1), (1, 0), (1, 1)], "a second pass on both pages"
    report(case["name"], n, bad)
