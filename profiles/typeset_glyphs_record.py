"""The record of DESIGN.md section 4.22: typeset from a glyph atlas against the bitmap path on the same content.

    python profiles/typeset_glyphs_record.py [out.json]

Rebuilds the bench batch of section 4.21 in this process (32 `synth.text_like_page` pages of 1024 x 1024 through the bench's
blob checkpoint, fp16 `detect_batch`, `fill_rest`, `layout_boxes`), makes an atlas of 64 glyph-like 24 x 24 bitmaps
(`typeset_ref.glyph`) and flows a run of random glyphs into every box: the `ok` layout boxes (sparse) and every detected
block's own box (dense).  At r = 0, 3, 12, median of 30 calls after 5 warm-ups with min and max:
  (a) HIP events around the one `ctd_typeset_glyphs` call, tables uploaded once;
  (b) the whole `glyphs.typeset_glyphs` call on the host clock;
  (c) what there was before on the same content: the numpy composition of the block bitmaps (a host loop over glyphs: its cost
      depends on the font engine's glue, this is the cheapest form of it), the whole `typeset.typeset_pages` call on them,
      and HIP events around its one `ctd_typeset` call;
  (d) the bytes each path uploads per call.
The pages of the two paths are compared byte for byte.  Needs a GPU; prints one JSON document."""
import ctypes as C
import importlib
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import typeset_ref as TR  # noqa: E402

pkg = importlib.import_module("comic-text-detector_amd")
L, T, G = pkg._lib, pkg.typeset, pkg.glyphs
CALLS, WARM = 30, 5


def stats(v, unit):
    v = np.sort(np.asarray(v, np.float64))
    return {"median_" + unit: round(float(np.median(v)), 2), "min": round(float(v[0]), 2), "max": round(float(v[-1]), 2)}


def events(fn, st):
    """`fn()` enqueues on stream `st`: microseconds between two events around it, CALLS times after WARM."""
    out = []
    for i in range(WARM + CALLS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(st)
        fn()
        b.record(st)
        b.synchronize()
        if i >= WARM:
            out.append(a.elapsed_time(b) * 1e3)
    return stats(out, "us")


def host(fn):
    out = []
    for i in range(WARM + CALLS):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if i >= WARM:
            out.append((time.perf_counter() - t) * 1e6)
    return stats(out, "us")


def blob(parts, dev):
    b, at = pkg.pagecall.pack(parts)
    tab = torch.from_numpy(b).to(dev)
    return tab, [tab.data_ptr() + int(a) for a in at], len(b)


def page_table(pages):
    pt = np.zeros((len(pages),), T.PAGE_DTYPE)
    pt["page_dev"] = [o.data_ptr() for o in pages]
    pt["H"], pt["W"], pt["pitch"] = [o.shape[0] for o in pages], [o.shape[1] for o in pages], [o.stride(0) for o in pages]
    return pt


def compose(bitmaps, ids, xy):
    """One block's bitmap from its glyphs, pasted one at a time with numpy: (cov, x0, y0)."""
    sizes = np.array([bitmaps[g].shape for g in ids], np.int64).reshape(-1, 2)
    x0, y0 = int(xy[:, 0].min()), int(xy[:, 1].min())
    cov = np.zeros((int((xy[:, 1] + sizes[:, 0]).max()) - y0, int((xy[:, 0] + sizes[:, 1]).max()) - x0), np.uint8)
    for g, (x, y) in zip(ids, xy):
        b = bitmaps[g]
        v = cov[y - y0:y - y0 + b.shape[0], x - x0:x - x0 + b.shape[1]]
        np.maximum(v, b, out=v)
    return cov, x0, y0


def case(name, pages, page_of, rects, atlas, bitmaps, rng, dev):
    shapes = [tuple(int(v) for v in p.shape[:2]) for p in pages]
    nl = len(rects)
    runs, xys = [], []
    for rc in rects:
        n = int(max(1, ((rc[2] - rc[0]) // 24) * ((rc[3] - rc[1]) // 24)))
        run = rng.integers(0, len(bitmaps), n)
        xy, _ = G.flow(run, atlas, rc)
        runs.append(run), xys.append(xy)
    count = [len(r) for r in runs]
    layer_of, glyph, xy = np.repeat(np.arange(nl), count), np.concatenate(runs), np.concatenate(xys)
    out = {"layers": nl, "placements": int(len(glyph)), "radius": {}}
    st = torch.cuda.current_stream(dev)
    for r in (0, 3, 12):
        rec = {}
        # ---- the glyph path
        tiles, entries, status = G.glyph_tables(shapes, page_of, layer_of, atlas.sizes[glyph], xy, r)
        work = T._copies(pages, dev)
        lt = np.zeros((nl,), G.LAYER_DTYPE)
        lt["page"], lt["clip"], lt["radius"] = page_of, [(0, 0, shapes[p][1], shapes[p][0]) for p in page_of], r
        lt["stroke"] = 255
        qt = np.zeros((len(glyph),), G.PLACE_DTYPE)
        qt["layer"], qt["glyph"], qt["x"], qt["y"] = layer_of, glyph, xy[:, 0], xy[:, 1]
        tab, ptr, n_up = blob([x.view(np.uint8) for x in (page_table(work), lt, qt, tiles, entries)], dev)
        rows = torch.empty((nl * 8,), dtype=torch.uint8, device=dev)
        prm = L.CtdGlyphParams(nl, len(pages), len(tiles) - 1, len(entries), len(glyph), len(atlas), atlas.nbytes)
        lib = L.lib()

        def launch_glyphs():
            L.check(lib.ctd_typeset_glyphs(ptr[0], ptr[1], ptr[2], atlas._rec.data_ptr(), ptr[3], ptr[4], atlas._cov.data_ptr(),
                                           C.byref(prm), rows.data_ptr(), st.cuda_stream), "ctd_typeset_glyphs")
        rec["tiles"], rec["entries"] = len(tiles) - 1, len(entries)
        rec["a_glyph_launch"] = events(launch_glyphs, st)
        rec["b_typeset_glyphs_call"] = host(lambda: G.typeset_glyphs(pages, atlas, page_of, layer_of, glyph, xy, radius=r))
        rec["d_glyph_upload_bytes"] = n_up
        # ---- the bitmap path on the same content
        t = []
        for i in range(3):
            t0 = time.perf_counter()
            comp = [compose(bitmaps, runs[j], xys[j]) for j in range(nl)]
            t.append((time.perf_counter() - t0) * 1e6)
        rec["c_numpy_composition"] = stats(t, "us")
        maps, bxy = [c[0] for c in comp], np.array([(c[1], c[2]) for c in comp], np.int64).reshape(nl, 2)
        rec["c_typeset_pages_call"] = host(lambda: T.typeset_pages(pages, page_of, maps, bxy, radius=r))
        sizes = np.array([m.shape for m in maps], np.int64).reshape(nl, 2)
        btiles, bentries, _ = T.typeset_tables(shapes, page_of, sizes, bxy, r)
        work2 = T._copies(pages, dev)
        bl = np.zeros((nl,), T.LAYER_DTYPE)
        area = sizes[:, 0] * sizes[:, 1]
        bl["cov0"], bl["page"], bl["x0"], bl["y0"], bl["h"], bl["w"] = np.cumsum(area) - area, page_of, bxy[:, 0], bxy[:, 1], sizes[:, 0], sizes[:, 1]
        bl["cov_pitch"], bl["clip"], bl["radius"] = sizes[:, 1], [(0, 0, shapes[p][1], shapes[p][0]) for p in page_of], r
        bl["stroke"] = 255
        cov = np.concatenate([m.ravel() for m in maps])
        tab2, ptr2, n_up2 = blob([x.view(np.uint8) for x in (page_table(work2), bl, btiles, bentries)] + [cov], dev)
        rows2 = torch.empty((nl * 8,), dtype=torch.uint8, device=dev)
        prm2 = L.CtdTypesetParams(nl, len(pages), len(btiles) - 1, len(bentries), len(cov), 0)

        def launch_bitmaps():
            L.check(lib.ctd_typeset(ptr2[0], ptr2[1], ptr2[2], ptr2[3], ptr2[4], C.byref(prm2), rows2.data_ptr(), st.cuda_stream), "ctd_typeset")
        rec["c_bitmap_tiles"], rec["c_bitmap_entries"] = len(btiles) - 1, len(bentries)
        rec["c_bitmap_launch"] = events(launch_bitmaps, st)
        rec["d_bitmap_upload_bytes"] = n_up2
        # ---- the same pages, byte for byte, and the same rows
        a = G.typeset_glyphs(pages, atlas, page_of, layer_of, glyph, xy, radius=r)
        b = T.typeset_pages(pages, page_of, maps, bxy, radius=r)
        rec["pages_identical"] = all(torch.equal(x, y) for x, y in zip(a.pages, b.pages))
        rec["rows_identical"] = a.rows.tobytes() == b.rows.tobytes()
        out["radius"][str(r)] = rec
        print(name, r, json.dumps(rec), flush=True)
    return out


def main():
    assert torch.cuda.is_available(), "the record needs a GPU"
    dev = torch.device("cuda", 0)
    ckpt = pkg.synth.make_blob_checkpoint(0, sparse_det=True, line_density="fixture")
    det = pkg.detector.TextDetector(ckpt, input_size=1024, device="cuda:0", precision="fp16")
    pages = [pkg.synth.text_like_page((1024, 1024), i) for i in range(32)]
    results = det.detect_batch(pages)
    fp = det.fill_rest(pages, results)
    lb = det.layout_boxes(pages, results)
    bitmaps = [TR.glyph(24, 24, 100 + i) for i in range(64)]
    atlas = G.GlyphAtlas(device=dev)
    atlas.add(bitmaps)
    rng = np.random.default_rng(0)
    ok = np.flatnonzero(lb.ok)
    sparse = np.where((lb.a_area[ok] > 0)[:, None], lb.a_rect[ok], lb.rect[ok]).astype(np.int64)
    dense = np.array([results[pg][2][b].xyxy for pg, b in lb.index], np.int64).reshape(-1, 4)
    doc = {"blocks": len(lb), "ok_boxes": int(len(ok)), "atlas_bytes": atlas.nbytes, "calls": CALLS, "warm_up": WARM,
           "device": torch.cuda.get_device_name(0)}
    doc["sparse"] = case("sparse", fp.pages, lb.index[ok, 0].astype(np.int64), sparse, atlas, bitmaps, rng, dev)
    doc["dense"] = case("dense", fp.pages, lb.index[:, 0].astype(np.int64), dense, atlas, bitmaps, rng, dev)
    text = json.dumps(doc, indent=1)
    print(text)
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        open(sys.argv[1], "w").write(text)
    det.close()


if __name__ == "__main__":
    main()
