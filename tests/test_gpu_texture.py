"""-m gpu: the texture fill of a hole mask -- `ctd_texture_fill` (csrc/kernels_texture.hip), `texture.texture_fill`,
`TextDetector.texture_fill` and the `texture=True` option of `model2annotations` -- against the numpy restatement
tests/texture_ref.py.  The rule is integers only, so every comparison is EXACT: every field of every row, every byte of every
page."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import texture_ref as R
import test_gpu_regions as TG
from conftest import pkg

pytestmark = pytest.mark.gpu


def _compare(tp, want, names=None):
    """Every row field, every byte of every page against (out, row) pairs of the restatement."""
    bad = []
    assert len(tp) == len(tp.rows) == len(want)
    for i, (out, row) in enumerate(want):
        name = names[i] if names else str(i)
        got = R.row_dict(tp.rows[i])
        if got != row or tp.rows[i]["pad_"].any():
            bad.append((name, {f: (got[f], row[f]) for f in R.FIELDS if got[f] != row[f]}))
        g = tp.pages[i].cpu().numpy()
        assert g.shape == out.shape and tp.pages[i].is_contiguous() and tp.pages[i].data_ptr() % 256 == 0
        if not np.array_equal(g, out):
            d = (g != out).any(axis=2)
            bad.append((name, "out", int(d.sum()), np.argwhere(d)[:4].tolist()))
    assert not bad, f"{len(bad)} differences, first: {bad[:4]}"


def _same(a, b):
    return a.rows.tobytes() == b.rows.tobytes() and all(torch.equal(x, y) for x, y in zip(a.pages, b.pages))


def test_kernels_equal_the_restatement_in_every_field_and_byte():
    """ONE `ctd_texture_fill` call over every page of the material -- 1 x 1 to 130 x 200, pages without a centre, with one
    centre, without a hole between pages with holes, holes on the tile seams and at the page's corners -- against
    `texture_ref.texture_vec` started from the pull-push fill: all fields of all rows, all bytes of all pages.  One page and
    one mask are strided views of larger tensors, whose surroundings stay.  The same call twice gives identical bytes; host
    inputs and an explicit stream give the same; the outputs are views of one allocation; the same page at batch positions
    0 and 5 gives the same bytes."""
    X, L = pkg().texture, pkg()._lib
    dev = torch.device("cuda:0")
    material, want = R.material(), R.reference()
    names = [m[0] for m in material]
    assert {m[1].shape[:2] for m in material} == {(1, 1), (6, 9), (7, 8), (7, 7), (33, 70), (64, 64), (65, 129), (97, 83), (130, 200)}
    pages = [torch.from_numpy(m[1].copy()).to(dev) for m in material]
    holes = [torch.from_numpy(m[2].copy()).to(dev) for m in material]
    i = names.index("97x83-random0.02-diag")
    wide = torch.full((97, 120, 3), 77, dtype=torch.uint8, device=dev)
    wide[:, 19:19 + 83] = pages[i]
    pages[i] = wide[:, 19:19 + 83]
    wm = torch.full((97, 150), 1, dtype=torch.uint8, device=dev)
    wm[:, 41:41 + 83] = holes[i]
    holes[i] = wm[:, 41:41 + 83]
    assert pages[i].stride(0) == 360 and holes[i].stride(0) == 150 and not pages[i].is_contiguous()
    tp = X.texture_fill(pages, holes)
    _compare(tp, want, names)
    counts = [int((tp.status == s).sum()) for s in (L.TEXTURE_OK, L.TEXTURE_NO_HOLE, L.TEXTURE_NO_SOURCE)]
    print(f"\n{len(material)} pages, status counts {counts}, unmatched {tp.n_unmatched.tolist()}")
    assert all(counts)
    assert any(s == L.TEXTURE_OK and u > 0 for s, u in zip(tp.status, tp.n_unmatched))
    assert any(s == L.TEXTURE_OK and u == 0 and t > 1000 for s, u, t in zip(tp.status, tp.n_unmatched, tp.n_target))
    assert tp.status[names.index("64x64-none-diag")] == L.TEXTURE_NO_HOLE                # between pages with holes
    for f in ("n_hole", "n_target", "n_source", "n_unmatched"):
        assert getattr(tp, f).tolist() == [w[1][f] for w in want]
    assert tp.n_source[names.index("7x8-pixel_0_7-ramp")] == 1 and tp.n_source[names.index("6x9-random0.1-noise")] == 0
    assert torch.equal(wide[:, :19], torch.full_like(wide[:, :19], 77)) and torch.equal(wide[:, 102:], torch.full_like(wide[:, 102:], 77))
    assert bool((wm[:, :41] == 1).all()) and bool((wm[:, 124:] == 1).all())                # inputs untouched
    assert all(np.array_equal(p.cpu().numpy(), m[1]) for p, m in zip(pages, material))
    base = tp.pages[0].untyped_storage().data_ptr()
    assert all(p.untyped_storage().data_ptr() == base for p in tp.pages)
    assert _same(X.texture_fill(pages, holes), tp)
    host = X.texture_fill([m[1] for m in material], [m[2] for m in material], stream=torch.cuda.Stream(dev))
    assert _same(host, tp)
    # the same page at positions 0 and 5 of a batch
    j = names.index("65x129-seams-tone")
    order = [j, 4, 5, 6, 9, j]
    twice = X.texture_fill([pages[k] for k in order], [holes[k] for k in order])
    _compare(twice, [want[k] for k in order], [names[k] for k in order])
    assert torch.equal(twice.pages[0], twice.pages[5]) and twice.rows[0].tobytes() == twice.rows[5].tobytes()
    assert len(X.texture_fill([], [])) == 0
    assert L.lib().ctd_texture_fill(None, 0, None, None, None, None) == L.OK             # nothing to do, nothing launched


CORNERS = (("R1", "33x70-text-diag", dict(radius=1)), ("R127", "33x70-text-diag", dict(radius=127)),
           ("one-sweep", "33x70-corner3-tone", dict(iterations=1, sweeps=1)), ("n_init1", "33x70-random0.02-noise", dict(n_init=1)),
           ("seed", "33x70-corner3-tone", dict(seed=0xDEADBEEF)), ("most", "33x70-corner3-tone", dict(iterations=16, sweeps=8, n_init=16, radius=3)))


@pytest.mark.parametrize("corner", CORNERS, ids=[c[0] for c in CORNERS])
def test_parameter_corners(corner):
    """The ends of every parameter's range on one small page each, against the restatement."""
    X = pkg().texture
    _, name, kw = corner
    _, page, hole = next(m for m in R.material() if m[0] == name)
    ref_kw = {{"iterations": "n_em", "sweeps": "n_sweep"}.get(k, k): v for k, v in kw.items()}
    want = R.texture_vec(page, hole, R.pull_push(page, hole), **ref_kw)
    _compare(X.texture_fill([page], [hole], **kw), [want], [name])
    if "seed" in kw:
        assert not np.array_equal(want[0], R.reference()[[m[0] for m in R.material()].index(name)][0])


def test_an_explicit_init_that_is_not_the_pull_push_fill():
    X = pkg().texture
    rng = np.random.default_rng(11)
    cases = [m for m in R.material() if m[0] in ("33x70-text-diag", "65x129-text-noise", "33x70-all-flat")]
    inits = [rng.integers(0, 256, m[1].shape, dtype=np.uint8) for m in cases]
    want = [R.texture_vec(m[1], m[2], i, n_em=2) for m, i in zip(cases, inits)]
    assert not np.array_equal(inits[0], R.pull_push(cases[0][1], cases[0][2]))
    tp = X.texture_fill([m[1] for m in cases], [m[2] for m in cases], init=inits, iterations=2)
    _compare(tp, want, [m[0] for m in cases])
    k = [m[0] for m in cases].index("33x70-all-flat")
    assert np.array_equal(tp.to_host()[k], inits[k])                                     # no source: `init` on the holes, all holes
    dev_init = [torch.from_numpy(i).cuda() for i in inits]
    assert _same(X.texture_fill([m[1] for m in cases], [m[2] for m in cases], init=dev_init, iterations=2), tp)


OUT_SENTINEL, SCRATCH_SENTINEL, ROWS_SENTINEL, GUARD = 0xA5, 0x5E, 0xC3, 4096


def _strided(flat, off, H, n, pitch):
    return np.lib.stride_tricks.as_strided(flat[off:], (H, n), (pitch, 1))


def test_the_raw_entry_point_between_guards():
    """One page of 200 x 330 through ctypes on a hand-made table, with out_pitch - 3 W, pitch - 3 W, init_pitch - 3 W and
    hole_pitch - W not 0 and `out_dev` on an odd address: the output arena (a sentinel wherever no row lies), the scratch
    buffer and the rows between guards are compared whole afterwards, and the inputs are unchanged."""
    X, L = pkg().texture, pkg()._lib
    dev = torch.device("cuda:0")
    H, W = 200, 330
    rng = np.random.default_rng(20)
    page = R.tone_page(H, W, 6)
    hole = np.maximum(R.seam_bars(H, W), R.text_holes(H, W))
    hole[H - 30:, W - 40:] = 9                                                           # flush with a corner
    init = R.pull_push(page, hole)
    prm_kw = dict(radius=20, n_em=2, n_sweep=2, n_init=4, seed=7)
    want, row = R.texture_vec(page, hole, init, **prm_kw)
    assert row["status"] == R.OK and row["n_target"] > 5000
    pitches = {"page": 3 * W + 2, "hole": W + 5, "init": 3 * W + 7, "out": 3 * W + 3}
    offs = {"page": 256, "hole": 257, "init": 258, "out": 259}
    host, devs = {}, {}
    for key, rows in (("page", page.reshape(H, 3 * W)), ("hole", hole), ("init", init.reshape(H, 3 * W))):
        a = rng.integers(0, 256, (offs[key] + H * pitches[key] + 256,), dtype=np.uint8)
        _strided(a, offs[key], H, rows.shape[1], pitches[key])[...] = rows
        host[key], devs[key] = a, torch.from_numpy(a).to(dev)
    exp = np.full((offs["out"] + H * pitches["out"] + 256,), OUT_SENTINEL, np.uint8)
    _strided(exp, offs["out"], H, 3 * W, pitches["out"])[...] = want.reshape(H, 3 * W)
    out_d = torch.full((len(exp),), OUT_SENTINEL, dtype=torch.uint8, device=dev)

    tile0, n_tiles, fld0, cls0, scratch_bytes = X.texture_tables([(H, W)])
    assert n_tiles == 24 and scratch_bytes == 16 * 24 + 9 * H * W
    pt = np.zeros((1,), X.PAGE_DTYPE)
    for key in ("page", "hole", "init"):
        pt[key + "_dev"] = devs[key].data_ptr() + offs[key]
    pt["out_dev"] = out_d.data_ptr() + offs["out"]
    pt["H"], pt["W"], pt["pitch"], pt["hole_pitch"], pt["init_pitch"], pt["out_pitch"] = H, W, pitches["page"], pitches["hole"], pitches["init"], pitches["out"]
    pt["tile0"], pt["fld0"], pt["cls0"] = tile0, fld0, cls0
    tab = torch.from_numpy(pt.view(np.uint8)).to(dev)
    scratch = torch.full((GUARD + scratch_bytes + GUARD,), SCRATCH_SENTINEL, dtype=torch.uint8, device=dev)
    rb = X.ROW_DTYPE.itemsize
    rows_d = torch.full((GUARD + rb + GUARD,), ROWS_SENTINEL, dtype=torch.uint8, device=dev)
    prm = L.CtdTextureParams(n_tiles, prm_kw["radius"], prm_kw["n_em"], prm_kw["n_sweep"], prm_kw["n_init"], prm_kw["seed"], scratch_bytes)
    rc = L.lib().ctd_texture_fill(tab.data_ptr(), 1, C.byref(prm), scratch.data_ptr() + GUARD, rows_d.data_ptr() + GUARD, None)
    assert rc == L.OK, L.lib().ctd_last_error()
    torch.cuda.synchronize()

    rows_h = rows_d.cpu().numpy()
    assert (rows_h[:GUARD] == ROWS_SENTINEL).all() and (rows_h[GUARD + rb:] == ROWS_SENTINEL).all(), "rows guards"
    assert bool((scratch[:GUARD] == SCRATCH_SENTINEL).all()) and bool((scratch[GUARD + scratch_bytes:] == SCRATCH_SENTINEL).all()), "scratch guards"
    for key in ("page", "hole", "init"):
        assert np.array_equal(devs[key].cpu().numpy(), host[key]), f"the {key} arena changed"
    rec = rows_h[GUARD:GUARD + rb].view(X.ROW_DTYPE)[0]
    assert R.row_dict(rec) == row and not rec["pad_"].any()
    got = out_d.cpu().numpy()
    if not np.array_equal(got, exp):
        diff = got != exp
        inside = _strided(diff, offs["out"], H, 3 * W, pitches["out"]).reshape(H, W, 3).any(axis=2)
        raise AssertionError(f"{int(diff.sum())} arena bytes differ, {int(inside.sum())} pixels inside, first {np.argwhere(inside)[:4].tolist()}, "
                             f"first byte {int(np.flatnonzero(diff)[0])}")


def test_bad_arguments_are_refused_without_a_launch():
    """The entry point itself: an error rc and a message, nothing launched -- the buffers the tables name do not exist, and a
    side of 8193 is declared in the table only.  Then the `ValueError`s of the Python layer."""
    X, L = pkg().texture, pkg()._lib
    lib = L.lib()
    dev = torch.device("cuda:0")
    MB = 1 << 20

    def call(n_pages=1, null=None, scratch=16 * MB, prm_kw=None, **cols):
        pt = np.zeros((1,), X.PAGE_DTYPE)
        pt["page_dev"], pt["hole_dev"], pt["init_dev"], pt["out_dev"] = 1 * MB, 2 * MB, 3 * MB, 4 * MB
        pt["H"], pt["W"], pt["pitch"], pt["hole_pitch"], pt["init_pitch"], pt["out_pitch"] = 20, 30, 90, 30, 90, 90
        pt["tile0"], pt["fld0"], pt["cls0"] = 0, 16, 16 + 8 * 600
        for k, v in cols.items():
            pt[k] = v
        tab = torch.from_numpy(pt.view(np.uint8)).to(dev)
        p = dict(n_tiles=1, radius=32, n_em=5, n_sweep=2, n_init=8, seed=0, scratch_bytes=16 + 9 * 600)
        p.update(prm_kw or {})
        prm = L.CtdTextureParams(*p.values())
        args = {"pages": tab.data_ptr(), "params": C.byref(prm), "scratch": scratch, "rows": 32 * MB}
        if null:
            args[null] = None
        rc = lib.ctd_texture_fill(args["pages"], n_pages, args["params"], args["scratch"], args["rows"], None)
        return rc, lib.ctd_last_error()

    big = dict(n_tiles=129, scratch_bytes=1 << 40)
    for kw in (dict(H=0), dict(W=0), dict(H=-3), dict(H=8193, prm_kw=big), dict(W=8193, prm_kw=big), dict(pitch=89), dict(hole_pitch=29),
               dict(init_pitch=89), dict(out_pitch=89), dict(tile0=1), dict(fld0=20), dict(fld0=0), dict(cls0=16 + 8 * 600 + 1), dict(cls0=-1),
               dict(page_dev=0), dict(hole_dev=0), dict(init_dev=0), dict(out_dev=0), dict(n_pages=-1), dict(null="pages"),
               dict(null="params"), dict(null="scratch"), dict(null="rows"), dict(scratch=16 * MB + 8),
               dict(out_dev=1 * MB + 90), dict(out_dev=2 * MB - 5), dict(out_dev=3 * MB + 20 * 90 - 1), dict(out_dev=3 * MB - 19 * 90 - 89)) + tuple(
                   dict(prm_kw=p) for p in (dict(n_tiles=2), dict(n_tiles=0), dict(n_tiles=-1), dict(scratch_bytes=16 + 9 * 600 - 1),
                                            dict(radius=0), dict(radius=128), dict(n_em=0), dict(n_em=17), dict(n_sweep=0), dict(n_sweep=9),
                                            dict(n_init=0), dict(n_init=17))):
        rc, msg = call(**kw)
        assert rc < 0 and msg, kw
    assert b"sides" in call(H=8193, prm_kw=big)[1] and b"pitch" in call(pitch=89)[1] and b"radius" in call(prm_kw=dict(radius=128))[1]
    assert b"overlaps" in call(out_dev=1 * MB + 90)[1]
    torch.cuda.synchronize()
    page = torch.zeros((20, 30, 3), dtype=torch.uint8, device=dev)
    hole = torch.zeros((20, 30), dtype=torch.uint8, device=dev)
    for bad in (lambda: X.texture_fill([page], [torch.zeros((20, 31), dtype=torch.uint8, device=dev)]),
                lambda: X.texture_fill([page.int()], [hole]),
                lambda: X.texture_fill([page], [hole], init=[page[:19]]),
                lambda: X.texture_fill([page], [hole], init=[page, page]),
                lambda: X.texture_fill([page], [hole, hole]),
                lambda: X.texture_fill([page], [hole], radius=0), lambda: X.texture_fill([page], [hole], radius=128),
                lambda: X.texture_fill([page], [hole], iterations=0), lambda: X.texture_fill([page], [hole], sweeps=9),
                lambda: X.texture_fill([page], [hole], n_init=17), lambda: X.texture_fill([page], [hole], seed=-1),
                lambda: X.texture_fill([page], [hole], seed=2 ** 32)):
        with pytest.raises(ValueError):
            bad()


def test_detector_texture_fill_starts_from_its_own_erase_and_fill():
    """`det.texture_fill(pages, results)` equals `texture.texture_fill` on the detector's own erase and fill outputs and the
    same call given `erased=` and `filled=`; a short run of it equals the restatement on those outputs."""
    p, det = pkg(), TG.detector()
    pages = [p.synth.text_like_page((256, 256), 3, n_blocks=4), p.synth.text_like_page((200, 300), 4, n_blocks=2)]
    results = det.detect_batch(pages)
    er = det.erase_text(pages, results)
    fp = det.fill_rest(pages, results, erased=er)
    clean, rest = er.to_host()
    assert any(r.any() for r in rest)
    tp = det.texture_fill(pages, results)
    assert _same(tp, p.texture.texture_fill(er.pages, er.rest, init=fp.pages))
    assert _same(tp, det.texture_fill(pages, results, erased=er, filled=fp))
    assert _same(tp, p.texture.texture_fill(er.pages, er.rest))                          # the default init is that fill
    for out, c, r in zip(tp.to_host(), clean, rest):
        assert np.array_equal(out[r == 0], c[r == 0])
    short = det.texture_fill(pages, results, erased=er, filled=fp, iterations=1, radius=8)
    _compare(short, [R.texture_vec(c, r, f, n_em=1, radius=8) for c, r, f in zip(clean, rest, fp.to_host())])


def test_model2annotations_writes_the_textured_pages_on_request(tmp_path):
    """`model2annotations(texture=True)` writes `textured-<name>.png` that decodes to `.pages` of `texture_fill` on the same
    detection; every other file is the bytes a run with `fill=True` writes, and the default writes what it wrote before."""
    p, det = pkg(), TG.detector()
    A = p.annotations
    src = tmp_path / "pages"
    src.mkdir()
    pages = {"a.png": p.synth.text_like_page((256, 256), 3, n_blocks=4), "b.png": p.synth.text_like_page((256, 256), 5, n_blocks=3)}
    for name, img in pages.items():
        (src / name).write_bytes(A.png_bytes(img))
    sets = {}
    for key, kw in (("plain", {}), ("fill", dict(fill=True)), ("texture", dict(texture=True))):
        out = tmp_path / key
        assert A.model2annotations(None, str(src), str(out), save_json=True, batch_size=2, detector=det, **kw) == 2
        sets[key] = sorted(os.listdir(out))
    assert sets["texture"] == sorted(sets["fill"] + ["textured-a.png", "textured-b.png"])
    assert not any(f.startswith(("textured-", "filled-", "clean-", "rest-")) for f in sets["plain"])
    assert sets["fill"] == sorted(sets["plain"] + [f"{k}-{n}.png" for k in ("clean", "rest", "filled") for n in "ab"])
    for f in sets["fill"]:
        assert (tmp_path / "fill" / f).read_bytes() == (tmp_path / "texture" / f).read_bytes(), f
    imgs = list(pages.values())
    results = det.detect_batch(imgs, refine_mode=p.textmask.REFINEMASK_ANNOTATION, keep_undetected_mask=True)
    tp = det.texture_fill(imgs, results)
    for name, tex in zip(pages, tp.to_host()):
        assert np.array_equal(A.imread(str(tmp_path / "texture" / f"textured-{name}")), tex)
