"""-m gpu: the smooth pull-push fill of a hole mask -- `ctd_fill_rest` (csrc/kernels_fill.hip), `fill.fill_rest`,
`TextDetector.fill_rest` and the `fill=True` option of `model2annotations` -- against the numpy restatement tests/fill_ref.py.
The rule is integers only, so every comparison is EXACT: every field of every row, every byte of every filled page."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import fill_ref as R
import test_gpu_regions as TG
from conftest import pkg

pytestmark = pytest.mark.gpu


def _compare(fp, pages, holes, want, names=None):
    """Every row field, every byte of every page against (out, row) pairs of the restatement."""
    bad = []
    assert len(fp) == len(fp.rows) == len(want)
    for i, (out, row) in enumerate(want):
        name = names[i] if names else str(i)
        got = R.row_dict(fp.rows[i])
        if got != row or fp.rows[i]["pad_"].any():
            bad.append((name, {f: (got[f], row[f]) for f in R.FIELDS if got[f] != row[f]}))
        g = fp.pages[i].cpu().numpy()
        assert g.shape == out.shape and fp.pages[i].is_contiguous() and fp.pages[i].data_ptr() % 256 == 0
        if not np.array_equal(g, out):
            d = (g != out).any(axis=2)
            bad.append((name, "out", int(d.sum()), np.argwhere(d)[:4].tolist()))
    assert not bad, f"{len(bad)} differences, first: {bad[:4]}"


def test_kernels_equal_the_restatement_in_every_field_and_byte():
    """ONE `ctd_fill_rest` call over every page of the material -- 1 x 1 to 200 x 330, every hole pattern, a page without a
    hole between pages with holes -- against `fill_ref.fill_vec`: all fields of all rows, all bytes of all pages.  One page and
    one mask are strided views of larger tensors; host inputs give the same; the same call twice gives identical bytes; the
    outputs are views of one allocation."""
    F, L = pkg().fill, pkg()._lib
    dev = torch.device("cuda:0")
    material, want = R.material(), R.reference()
    names = [m[0] for m in material]
    pages = [torch.from_numpy(m[1]).to(dev) for m in material]
    holes = [torch.from_numpy(m[2]).to(dev) for m in material]
    i = names.index("97x83-random0.5-noise")
    wide = torch.full((97, 120, 3), 77, dtype=torch.uint8, device=dev)
    wide[:, 19:19 + 83] = pages[i]
    pages[i] = wide[:, 19:19 + 83]
    wm = torch.full((97, 150), 1, dtype=torch.uint8, device=dev)
    wm[:, 41:41 + 83] = holes[i]
    holes[i] = wm[:, 41:41 + 83]
    assert pages[i].stride(0) == 360 and holes[i].stride(0) == 150 and not pages[i].is_contiguous()
    fp = F.fill_rest(pages, holes)
    _compare(fp, pages, holes, want, names)
    counts = [int((fp.status == s).sum()) for s in (L.FILL_OK, L.FILL_NO_HOLE, L.FILL_NO_KNOWN)]
    print(f"\n{len(material)} pages, status counts {counts}")
    assert all(counts)
    assert fp.n_hole.tolist() == [w[1]["n_hole"] for w in want] and fp.top.tolist() == [w[1]["top"][::-1] for w in want]
    assert torch.equal(wide[:, :19], torch.full_like(wide[:, :19], 77)) and bool((wm[:, :41] == 1).all())   # inputs untouched
    base = fp.pages[0].untyped_storage().data_ptr()
    assert all(p.untyped_storage().data_ptr() == base for p in fp.pages)
    again = F.fill_rest(pages, holes)
    assert again.rows.tobytes() == fp.rows.tobytes() and all(torch.equal(a, b) for a, b in zip(again.pages, fp.pages))
    host = F.fill_rest([m[1] for m in material], [m[2] for m in material], stream=torch.cuda.Stream(dev))
    assert host.rows.tobytes() == fp.rows.tobytes() and all(torch.equal(a, b) for a, b in zip(host.pages, fp.pages))
    mixed = F.fill_rest([m[1] for m in material[:5]], holes[:5])
    assert all(np.array_equal(a, b.cpu().numpy()) for a, b in zip(mixed.to_host(), fp.pages[:5]))


def test_one_page_alone_and_no_pages():
    """A call of one page whose tiles are all filled, and the empty call."""
    F, L = pkg().fill, pkg()._lib
    names = [m[0] for m in R.material()]
    for name in ("200x330-big_top-ramp", "1x1-all-noise", "65x129-checker-flat"):
        i = names.index(name)
        _, page, hole = R.material()[i]
        _compare(F.fill_rest([page], [hole]), [page], [hole], [R.reference()[i]], [name])
    assert len(F.fill_rest([], [])) == 0
    prm = L.CtdFillParams(0)
    assert L.lib().ctd_fill_rest(None, 0, C.byref(prm), None, None, None) == L.OK        # nothing to do, nothing launched
    assert L.lib().ctd_fill_rest(None, 0, None, None, None, None) == L.OK


def test_bad_arguments_are_refused_without_a_launch():
    """The entry point itself: an error rc and a message, nothing launched -- the buffers the tables name do not exist, and a
    side of 8193 is declared in the table only."""
    F, L = pkg().fill, pkg()._lib
    lib = L.lib()
    dev = torch.device("cuda:0")

    def call(n_tiles=1, n_pages=1, null=None, **cols):
        pt = np.zeros((1,), F.PAGE_DTYPE)
        pt["page_dev"], pt["hole_dev"], pt["out_dev"] = 256, 512, 768
        pt["H"], pt["W"], pt["pitch"], pt["hole_pitch"], pt["out_pitch"], pt["tile0"], pt["lvl0"] = 20, 30, 90, 30, 90, 0, 1
        for k, v in cols.items():
            pt[k] = v
        tab = torch.from_numpy(pt.view(np.uint8)).to(dev)
        prm = L.CtdFillParams(n_tiles)
        args = {"pages": tab.data_ptr(), "params": C.byref(prm), "scratch": 1024, "rows": 2048}
        if null:
            args[null] = None
        rc = lib.ctd_fill_rest(args["pages"], n_pages, args["params"], args["scratch"], args["rows"], None)
        return rc, lib.ctd_last_error()

    for kw in (dict(H=0), dict(W=0), dict(H=-3), dict(H=8193, n_tiles=129), dict(W=8193, n_tiles=129), dict(pitch=89), dict(hole_pitch=29),
               dict(out_pitch=89), dict(tile0=1), dict(n_tiles=2), dict(n_tiles=0), dict(n_tiles=-1), dict(lvl0=-1), dict(page_dev=0),
               dict(hole_dev=0), dict(out_dev=0), dict(n_pages=-1), dict(null="pages"), dict(null="params"), dict(null="scratch"),
               dict(null="rows")):
        rc, msg = call(**kw)
        assert rc < 0 and msg, kw
    assert b"sides" in call(H=8193, n_tiles=129)[1] and b"pitch" in call(pitch=89)[1]
    torch.cuda.synchronize()
    page = torch.zeros((20, 30, 3), dtype=torch.uint8, device=dev)
    with pytest.raises(ValueError):
        F.fill_rest([page], [torch.zeros((20, 31), dtype=torch.uint8, device=dev)])
    with pytest.raises(ValueError):
        F.fill_rest([page.int()], [torch.zeros((20, 30), dtype=torch.uint8, device=dev)])


def test_detector_fill_rest_fills_what_erase_leaves():
    """`det.fill_rest(pages, results)` equals the restatement applied to `det.erase_text(pages, results)`'s own outputs, equals
    the same call given `erased=`, and is the erased page wherever the rest mask is 0."""
    p, det = pkg(), TG.detector()
    pages = [p.synth.text_like_page((256, 256), 3, n_blocks=4), p.synth.text_like_page((200, 300), 4, n_blocks=2)]
    results = det.detect_batch(pages)
    er = det.erase_text(pages, results)
    clean, rest = er.to_host()
    assert any(r.any() for r in rest)
    want = [R.fill_vec(c, r) for c, r in zip(clean, rest)]
    fp = det.fill_rest(pages, results)
    _compare(fp, clean, rest, want)
    other = det.fill_rest(pages, results, erased=er)
    assert other.rows.tobytes() == fp.rows.tobytes() and all(torch.equal(a, b) for a, b in zip(other.pages, fp.pages))
    for out, c, r in zip(fp.to_host(), clean, rest):
        assert np.array_equal(out[r == 0], c[r == 0])
    grown = det.fill_rest([torch.from_numpy(x).cuda() for x in pages], results, grow=3)
    er3 = det.erase_text(pages, results, grow=3)
    _compare(grown, *er3.to_host(), [R.fill_vec(c, r) for c, r in zip(*er3.to_host())])
    with pytest.raises(ValueError):
        det.fill_rest(pages, results, ring=0)


def test_model2annotations_writes_the_filled_pages_on_request(tmp_path):
    """`model2annotations(fill=True)` writes `filled-<name>.png` that decodes to `.pages` of `fill_rest` on the same detection;
    every other file is the bytes a run with `erase=True` writes."""
    p, det = pkg(), TG.detector()
    A = p.annotations
    src = tmp_path / "pages"
    src.mkdir()
    pages = {"a.png": p.synth.text_like_page((256, 256), 3, n_blocks=4), "b.png": p.synth.text_like_page((256, 256), 5, n_blocks=3)}
    for name, img in pages.items():
        (src / name).write_bytes(A.png_bytes(img))
    sets = {}
    for key, kw in (("erase", dict(erase=True)), ("fill", dict(fill=True))):
        out = tmp_path / key
        assert A.model2annotations(None, str(src), str(out), save_json=True, batch_size=2, detector=det, **kw) == 2
        sets[key] = sorted(os.listdir(out))
    assert sets["fill"] == sorted(sets["erase"] + ["filled-a.png", "filled-b.png"])
    assert not any(f.startswith("filled-") for f in sets["erase"])
    for f in sets["erase"]:
        assert (tmp_path / "erase" / f).read_bytes() == (tmp_path / "fill" / f).read_bytes(), f
    imgs = list(pages.values())
    results = det.detect_batch(imgs, refine_mode=p.textmask.REFINEMASK_ANNOTATION, keep_undetected_mask=True)
    fp = det.fill_rest(imgs, results)
    for name, filled in zip(pages, fp.to_host()):
        assert np.array_equal(A.imread(str(tmp_path / "fill" / f"filled-{name}")), filled)
