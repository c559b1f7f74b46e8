"""The record of DESIGN.md section 4.25: glyph outlines rasterised into the atlas in one launch.

    python profiles/raster_record.py [out.json]

Seeded outlines (`raster_ref.random_outline`: 1 .. 3 closed contours, lines and curves mixed, 1000 units an em), every one a
distinct glyph of one `OutlineFont`; 64 and 2 000 instances at 24 and 48 px an em.  Median of 30 after 5 warm-ups with min
and max:
  (a) HIP events around the one `ctd_rasterise_glyphs` launch, the job table uploaded once, into a buffer of the atlas's size;
  (b) the whole `GlyphAtlas.rasterise` call on the host clock, into a fresh atlas each time (host boxes and metrics, growing
      the buffer, the job upload, the launch, the status download);
  (c) where PIL and a TrueType file are on the box (matplotlib's DejaVu Sans), the path this replaces for the same count:
      `font.getmask` per glyph plus one `atlas.add` of the bitmaps (DejaVu's own outlines, not the seeded ones: the count
      and the pixel size are what is equal).
Needs a GPU; prints one JSON document."""
import glob
import importlib
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import raster_ref as RR  # noqa: E402

pkg = importlib.import_module("comic-text-detector_amd")
L, G = pkg._lib, pkg.glyphs
CALLS, WARM = 30, 5


def stats(v, unit):
    v = np.sort(np.asarray(v, np.float64))
    return {"median_" + unit: round(float(np.median(v)), 2), "min": round(float(v[0]), 2), "max": round(float(v[-1]), 2)}


def events(fn, st):
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


def host(make, fn):
    """`fn(make())` on the host clock, `make()` outside it."""
    out = []
    for i in range(WARM + CALLS):
        x = make()
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn(x)
        torch.cuda.synchronize()
        if i >= WARM:
            out.append((time.perf_counter() - t) * 1e6)
    return stats(out, "us")


def ttf():
    try:
        import matplotlib
        from PIL import ImageFont  # noqa: F401
    except ImportError:
        return None
    found = glob.glob(os.path.join(os.path.dirname(matplotlib.__file__), "mpl-data", "fonts", "ttf", "DejaVuSans.ttf"))
    return found[0] if found else None


def main():
    assert torch.cuda.is_available(), "the record needs a GPU"
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    outlines = [RR.random_outline(rng) for _ in range(2000)]
    font = G.OutlineFont(1000, 800, 200, device=dev)
    font.add(outlines, rng.integers(300, 900, len(outlines)))
    segs_dev = font._sync()
    st = torch.cuda.current_stream(dev)
    lib = L.lib()
    path = ttf()
    doc = {"device": torch.cuda.get_device_name(0), "calls": CALLS, "warm_up": WARM, "segments": font.n_segs, "ttf": bool(path),
           "cases": []}
    for n in (64, 2000):
        for size in (24, 48):
            gids = np.arange(n)
            m = font.metrics(gids, size)
            area = m.box[:, 2] * m.box[:, 3]
            jobs = np.zeros((n,), G.RASTER_JOB_DTYPE)
            jobs["off"], jobs["w"], jobs["h"], jobs["bx"], jobs["by"] = np.cumsum(area) - area, m.box[:, 2], m.box[:, 3], m.box[:, 0], m.box[:, 1]
            jobs["seg_first"], jobs["seg_count"], jobs["scale"] = font.seg_first[gids], font.seg_count[gids], m.scale
            jobs_dev = torch.from_numpy(jobs.view(np.uint8).copy()).to(dev)
            total = int(area.sum())
            buf = torch.empty((total,), dtype=torch.uint8, device=dev)
            status = torch.empty((n,), dtype=torch.int32, device=dev)

            def launch():
                L.check(lib.ctd_rasterise_glyphs(segs_dev.data_ptr(), font.n_segs, jobs_dev.data_ptr(), n, buf.data_ptr(), total,
                                                 status.data_ptr(), st.cuda_stream), "ctd_rasterise_glyphs")
            rec = {"instances": n, "size_px": size, "segments": int(font.seg_count[gids].sum()), "atlas_bytes": total,
                   "mean_box": [round(float(m.box[:, 2].mean()), 1), round(float(m.box[:, 3].mean()), 1)],
                   "job_upload_bytes": int(jobs.nbytes)}
            rec["a_launch"] = events(launch, st)
            assert int((status.cpu() != L.RASTER_OK).sum()) == 0
            rec["b_rasterise_call"] = host(lambda: G.GlyphAtlas(device=dev), lambda a: a.rasterise(font, gids, size))
            if path:
                from PIL import ImageFont
                f = ImageFont.truetype(path, size)
                chars = [chr(0x21 + i) for i in range(n)]

                def pil(atlas):
                    maps = []
                    for c in chars:
                        mk = f.getmask(c)
                        maps.append(np.frombuffer(bytes(mk), np.uint8).reshape(mk.size[1], mk.size[0]) if mk.size[0] * mk.size[1]
                                    else np.zeros((0, 0), np.uint8))
                    atlas.add(maps)
                    return maps
                rec["c_getmask_plus_add"] = host(lambda: G.GlyphAtlas(device=dev), pil)
                rec["c_pil_atlas_bytes"] = int(sum(b.size for b in pil(G.GlyphAtlas(device=dev))))
            doc["cases"].append(rec)
            print(json.dumps(rec), flush=True)
    text = json.dumps(doc, indent=1)
    print(text)
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        open(sys.argv[1], "w").write(text)


if __name__ == "__main__":
    main()
