"""The record of DESIGN.md section 4.30: the texture fill call against the pull-push fill it starts from.

    python profiles/texture_record.py [out.json]

Rebuilds the bench batch of section 4.19 in this process (32 `synth.text_like_page` pages of 1024 x 1024 through the bench's
blob checkpoint, fp16 `detect_batch`, `erase_text`) and measures two batches: (sparse) `er.pages` / `er.rest` as they are, and
(dense) the same pages with a 300 x 400 hole and 2 % speckle on every page.  The tables are built and uploaded once; `init` is
`fill_rest`'s output for the batch.  Median of 30 after 5 warm-ups with min and max, HIP events around
  (a) the one `ctd_texture_fill` call (default parameters: 1 + 11 + 5 + 1 launches, the table fetch in front included);
  (b) the yardstick: the one `ctd_fill_rest` call on the same batch.
From the rows it prints the counts of holes, targets, sources and unmatched targets, and from them and the parameters the
candidates a call tries at most (inadmissible ones cost no patch compare, so this is an upper bound) and two floors known
without a run: targets x candidates x 147 squared differences at 2 lane-operations each against the vector rate (256 CUs x 4
SIMDs x 32 lanes x 2.4 GHz), and the bytes of the planes and pages every launch must move against 6.3 TB/s.  The time per
launch class comes from a kernel trace of this script in a run of its own (kernel names `texture_*_kernel`):

    rocprofv3 --kernel-trace --output-format csv -d <dir> -o texture -- python profiles/texture_record.py
    python profiles/texture_record.py --trace <dir> [out.json]

where the second command (no GPU) reads the trace's CSV and prints, per batch and launch class, the median, min and max over
the 30 timed calls (profiles/texture_record_trace.json).  The measuring run needs a GPU; it prints one JSON document."""
import csv
import glob
import ctypes as C
import importlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

pkg = importlib.import_module("comic-text-detector_amd")
L, F, X = pkg._lib, pkg.fill, pkg.texture
CALLS, WARM = 30, 5
PRM = dict(radius=32, n_em=5, n_sweep=2, n_init=8, seed=0)
LANE_OPS_PER_S = 256 * 4 * 32 * 2.4e9
HBM_BYTES_PER_S = 6.3e12


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


def case(name, pages, holes, dev, st):
    lib = L.lib()
    n = len(pages)
    shapes = [tuple(p.shape[:2]) for p in pages]
    init = F.fill_rest(pages, holes).pages
    out = pkg.pagecall.views([(h, w, 3) for h, w in shapes], dev)[1]
    # ---- the texture call's tables
    tile0, n_tiles, fld0, cls0, scratch_bytes = X.texture_tables(shapes)
    pt = np.zeros((n,), X.PAGE_DTYPE)
    pt["page_dev"], pt["hole_dev"] = [p.data_ptr() for p in pages], [h.data_ptr() for h in holes]
    pt["init_dev"], pt["out_dev"] = [p.data_ptr() for p in init], [o.data_ptr() for o in out]
    pt["H"], pt["W"] = [s[0] for s in shapes], [s[1] for s in shapes]
    pt["pitch"], pt["hole_pitch"] = [p.stride(0) for p in pages], [h.stride(0) for h in holes]
    pt["init_pitch"], pt["out_pitch"] = [p.stride(0) for p in init], [o.stride(0) for o in out]
    pt["tile0"], pt["fld0"], pt["cls0"] = tile0, fld0, cls0
    tab = torch.from_numpy(pt.view(np.uint8).copy()).to(dev)
    scratch = torch.empty((scratch_bytes,), dtype=torch.uint8, device=dev)
    rows_dev = torch.empty((n * X.ROW_DTYPE.itemsize,), dtype=torch.uint8, device=dev)
    prm = L.CtdTextureParams(n_tiles, PRM["radius"], PRM["n_em"], PRM["n_sweep"], PRM["n_init"], PRM["seed"], scratch_bytes)

    def texture():
        L.check(lib.ctd_texture_fill(tab.data_ptr(), n, C.byref(prm), scratch.data_ptr(), rows_dev.data_ptr(), st.cuda_stream), "ctd_texture_fill")
    # ---- the yardstick's tables
    ftile0, fn_tiles, lvl0, scratch_dwords, _ = F.fill_tables(shapes)
    ft = np.zeros((n,), F.PAGE_DTYPE)
    ft["page_dev"], ft["hole_dev"], ft["out_dev"] = pt["page_dev"], pt["hole_dev"], pt["out_dev"]
    ft["H"], ft["W"], ft["pitch"], ft["hole_pitch"], ft["out_pitch"] = pt["H"], pt["W"], pt["pitch"], pt["hole_pitch"], pt["out_pitch"]
    ft["tile0"], ft["lvl0"] = ftile0, lvl0
    ftab = torch.from_numpy(ft.view(np.uint8).copy()).to(dev)
    fscratch = torch.empty((scratch_dwords,), dtype=torch.int32, device=dev)
    frows = torch.empty((n * F.ROW_DTYPE.itemsize,), dtype=torch.uint8, device=dev)
    fprm = L.CtdFillParams(fn_tiles)

    def fill():
        L.check(lib.ctd_fill_rest(ftab.data_ptr(), n, C.byref(fprm), fscratch.data_ptr(), frows.data_ptr(), st.cuda_stream), "ctd_fill_rest")

    rec = {"batch": name, "pages": n, "pixels": int(sum(h * w for h, w in shapes)), "tiles": n_tiles, "scratch_bytes": scratch_bytes}
    rec["b_fill_rest_call"] = events(fill, st)
    rec["a_texture_fill_call"] = events(texture, st)
    rows = rows_dev.cpu().numpy().view(X.ROW_DTYPE)
    for f in ("n_hole", "n_target", "n_source", "n_unmatched"):
        rec[f] = int(rows[f].sum())
    rec["hole_share"] = round(rec["n_hole"] / rec["pixels"], 5)
    rec["status_counts"] = [int((rows["status"] == s).sum()) for s in range(3)]
    # what the parameters allow a target: the old entry, then n_init draws or 16 neighbours and one draw pair a radius
    n_rho = int(PRM["radius"]).bit_length()
    sweeps = PRM["n_em"] * PRM["n_sweep"] + 1
    per_target = PRM["n_init"] + (sweeps - 1) * (1 + 16 + n_rho)
    rec["launches"] = 1 + sweeps + PRM["n_em"] + 1
    rec["candidates_per_target_at_most"] = per_target
    rec["squared_differences_at_most"] = rec["n_target"] * per_target * 147
    rec["floor_valu_us"] = round(rec["squared_differences_at_most"] * 2 / LANE_OPS_PER_S * 1e6, 2)
    # bytes without any patch traffic: prepare reads page + mask + init where a hole and writes out + class (+ 4 a target);
    # every sweep reads and writes a field dword a target and the class byte of the tiles it works on (not counted);
    # every vote reads up to 49 field dwords and source pixels a hole pixel from cache and writes 3 bytes a hole pixel
    px = rec["pixels"]
    rec["plane_bytes"] = int(px * (3 + 1 + 3 + 1) + rec["n_target"] * 4 + sweeps * rec["n_target"] * 8 + PRM["n_em"] * rec["n_hole"] * 3)
    rec["floor_hbm_us"] = round(rec["plane_bytes"] / HBM_BYTES_PER_S * 1e6, 2)
    floor = max(rec["floor_valu_us"], rec["floor_hbm_us"])
    rec["call_over_floor"] = round(rec["a_texture_fill_call"]["median_us"] / floor, 1)
    rec["call_over_fill_rest"] = round(rec["a_texture_fill_call"]["median_us"] / rec["b_fill_rest_call"]["median_us"], 1)
    print(json.dumps(rec), flush=True)
    return rec


def trace_classes(trace_dir):
    """Per batch and launch class, the kernel times of the timed calls of one traced run of `main()`: a call is 18 launches,
    a batch WARM + CALLS calls, the yardstick's calls lie between them under other names."""
    path = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)[0]
    rows = [r for r in csv.DictReader(open(path)) if "texture_" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    per_call = 1 + PRM["n_em"] * PRM["n_sweep"] + 1 + PRM["n_em"] + 1
    calls = [rows[i:i + per_call] for i in range(0, len(rows), per_call)]
    assert len(calls) == 2 * (WARM + CALLS), len(calls)
    us = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3      # noqa: E731
    out = {}
    for b, name in enumerate(("sparse", "dense")):
        cls = {}
        for c in calls[b * (WARM + CALLS) + WARM:(b + 1) * (WARM + CALLS)]:
            for j, r in enumerate(c):
                k = r["Kernel_Name"].split("texture_")[1].split("_kernel")[0]
                cls.setdefault("initial_sweep" if (k, j) == ("sweep", 1) else k, []).append(us(r))
            cls.setdefault("all_launches", []).append(sum(us(r) for r in c))
        out[name] = {k: dict(stats(v, "us"), n=len(v)) for k, v in cls.items()}
    return out


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--trace":
        text = json.dumps(trace_classes(sys.argv[2]), indent=1)
        print(text)
        if len(sys.argv) > 3:
            open(sys.argv[3], "w").write(text)
        return
    assert torch.cuda.is_available(), "the record needs a GPU"
    dev = torch.device("cuda", 0)
    ckpt = pkg.synth.make_blob_checkpoint(0, sparse_det=True, line_density="fixture")
    det = pkg.detector.TextDetector(ckpt, input_size=1024, device="cuda:0", precision="fp16")
    pages = [pkg.synth.text_like_page((1024, 1024), i) for i in range(32)]
    results = det.detect_batch(pages)
    er = det.erase_text(pages, results)
    st = torch.cuda.current_stream(dev)
    doc = {"device": torch.cuda.get_device_name(0), "calls": CALLS, "warm_up": WARM, "parameters": PRM, "cases": []}
    doc["cases"].append(case("sparse", er.pages, er.rest, dev, st))
    g = torch.Generator(device=dev).manual_seed(419)
    dense = []
    for r in er.rest:
        m = (torch.rand(r.shape, generator=g, device=dev) < 0.02).to(torch.uint8) * 255
        m[300:600, 200:600] = 255
        dense.append(torch.maximum(m, r))
    doc["cases"].append(case("dense", er.pages, dense, dev, st))
    text = json.dumps(doc, indent=1)
    print(text)
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        open(sys.argv[1], "w").write(text)
    det.close()


if __name__ == "__main__":
    main()
