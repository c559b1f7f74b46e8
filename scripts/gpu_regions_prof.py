#!/usr/bin/env python3
"""OCR line crops (`regions.line_regions`) and OCR input batches (`regions.line_batches`) at the benchmark's shape,
in separate processes so that a kernel trace of the measured one holds nothing but its own launches:

    python scripts/gpu_regions_prof.py detect blocks.pkl          # 32 text-like 1024x1024 pages through the benchmark's detector
    rocprofv3 --kernel-trace --stats -d out -o regions -- \\
        python scripts/gpu_regions_prof.py warp blocks.pkl         # line_regions on 32 / 8 / 1 of those pages, CALLS times each
    rocprofv3 --kernel-trace --stats -d out2 -o batches -- \\
        python scripts/gpu_regions_prof.py batches blocks.pkl calls.json
    python scripts/gpu_regions_prof.py report out2 calls.json      # the trace's kernel statistics split by route

`warp` prints per page count: lines, crop bytes, wall time per call and GPU time per call (events around the call); the trace's
kernel statistics then show `region_warp_kernel` exactly once per call whatever the line count, and nothing else.

`batches` builds the same float16 NCHW bucket tensors (max_batch 16, width multiple 8, (v - 127.5) / 127.5) by two routes on
32 / 8 / 1 pages: route (a), what the package offered before `line_batches` -- `line_regions`, `padded(W_k)[lines]` per bucket,
torch normalise + permute (and (a1): ONE `padded()` sliced per bucket) -- and route (b) `line_batches`.  Per route and page
count it records calls, bytes of the result, `torch.cuda.max_memory_allocated` over a call (above what was allocated before
it), wall and event time per call, and checks that the routes' tensors are equal.  `region_batch_kernel` is launched by route
(b) only and `region_warp_kernel` once at the head of every (a) / (a1) call, so `report` splits the kernel trace into the
calls in dispatch order: launches and kernel time per call, per route and page count."""
import csv
import glob
import importlib
import json
import os
import pickle
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("comic-text-detector_amd")

B, S, CALLS, TH = 32, 1024, 20, 48


def pages():
    return [pkg.synth.text_like_page((S, S), 131 + i) for i in range(B)]


def detect(path):
    det = pkg.detector.TextDetector(pkg.synth.make_blob_checkpoint(0, sparse_det=True, line_density="fixture"), input_size=S,
                                    device="cuda:0", half=True)
    res = det.detect_batch(pages())
    out = [[dict(xyxy=b.xyxy, lines=np.asarray(b.lines).tolist(), language=b.language, vertical=bool(b.vertical),
                 font_size=b.font_size) for b in r[2]] for r in res]
    with open(path, "wb") as f:
        pickle.dump(out, f)
    n = sum(len(b["lines"]) for pg in out for b in pg)
    print(f"detected {sum(len(pg) for pg in out)} blocks, {n} lines on {B} pages ({n / B:.1f} lines per page) -> {path}")


def warp(path):
    with open(path, "rb") as f:
        recs = pickle.load(f)
    lists = [[pkg.textblock.TextBlock(**b) for b in pg] for pg in recs]
    dev = torch.device("cuda:0")
    dev_pages = list(torch.from_numpy(np.stack(pages())).to(dev))
    torch.cuda.synchronize()
    for nb in (B, 8, 1):
        pg, bl = dev_pages[:nb], lists[:nb]
        regs = pkg.regions.line_regions(pg, bl, TH)                       # warm-up (library load, allocator)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        gpu_ms, t0 = 0.0, time.perf_counter()
        for _ in range(CALLS):
            e0.record()
            regs = pkg.regions.line_regions(pg, bl, TH)
            e1.record()
            e1.synchronize()
            gpu_ms += e0.elapsed_time(e1)
        wall = (time.perf_counter() - t0) / CALLS * 1e3
        print(f"{nb:2d} pages: {len(regs)} lines ({int((~regs.valid).sum())} invalid), {regs.packed.numel()} crop bytes, widths "
              f"{int(regs.widths.min())}..{int(regs.widths.max())}; {CALLS + 1} calls; wall {wall:.3f} ms per call, events "
              f"{gpu_ms / CALLS:.3f} ms per call (host work + upload + the launch)")


def _buckets_a(pg, bl, one_padded):
    """Route (a): the bucket tensors from the packed crops with torch ops."""
    regs = pkg.regions.line_regions(pg, bl, TH)
    plan = pkg.regions.batch_plan(regs.widths, regs.valid, 16, 8)
    full = regs.padded(int(plan.batch_width.max())) if one_padded and len(plan.batch_width) else None
    out = []
    for k, wk in enumerate(plan.batch_width.tolist()):
        lines = torch.from_numpy(plan.order[plan.bounds[k]: plan.bounds[k + 1]]).to(regs.packed.device)
        x = full[lines][:, :, :wk] if one_padded else regs.padded(wk)[lines]
        out.append(((x.permute(0, 3, 1, 2).float() - 127.5) / 127.5).half().contiguous())
    return out


def _buckets_b(pg, bl, one_padded=None):
    lb = pkg.regions.line_batches(pg, bl, TH)
    return [x for x, _ in lb]


def batches(path, out_json):
    with open(path, "rb") as f:
        recs = pickle.load(f)
    lists = [[pkg.textblock.TextBlock(**b) for b in pg] for pg in recs]
    dev = torch.device("cuda:0")
    dev_pages = list(torch.from_numpy(np.stack(pages())).to(dev))
    torch.cuda.synchronize()
    record = []
    for nb in (B, 8, 1):
        pg, bl = dev_pages[:nb], lists[:nb]
        results = {}
        for route, fn, one, calls in (("b", _buckets_b, None, CALLS), ("a", _buckets_a, False, 3), ("a1", _buckets_a, True, 3)):
            xs = fn(pg, bl, one)                                 # warm-up (library load, allocator), counted as a call
            torch.cuda.synchronize()
            results[route] = xs
            peak = 0
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            gpu_ms, t0 = 0.0, time.perf_counter()
            for _ in range(calls):
                del xs
                torch.cuda.synchronize()
                base = torch.cuda.memory_allocated(dev) - sum(x.numel() * x.element_size() for x in results[route])
                torch.cuda.reset_peak_memory_stats(dev)
                e0.record()
                xs = fn(pg, bl, one)
                e1.record()
                e1.synchronize()
                gpu_ms += e0.elapsed_time(e1)
                peak = max(peak, torch.cuda.max_memory_allocated(dev) - base)
                results[route] = xs
            wall = (time.perf_counter() - t0) / calls * 1e3
            nbytes = sum(x.numel() * x.element_size() for x in xs)
            rec = dict(pages=nb, route=route, calls=calls + 1, buckets=len(xs), lines=sum(len(x) for x in xs), result_bytes=nbytes,
                       peak_bytes_over_call=int(peak), wall_ms_per_call=round(wall, 3), event_ms_per_call=round(gpu_ms / calls, 3))
            record.append(rec)
            print(rec)
        for route in ("a", "a1"):
            # compared on the host: a torch comparison would put kernels of its own into the trace
            same = len(results[route]) == len(results["b"]) and all(
                np.array_equal(x.cpu().numpy().view(np.int16), y.cpu().numpy().view(np.int16)) for x, y in zip(results[route], results["b"]))
            print(f"{nb:2d} pages: route ({route}) tensors equal route (b): {same}")
            record.append(dict(pages=nb, route=route, equal_to_b=bool(same)))
        del results, xs
    with open(out_json, "w") as f:
        json.dump(record, f, indent=1)


def report(trace_dir, calls_json):
    """Splits the kernel trace of a `batches` run into its calls: in dispatch order every route (b) call is ONE
    `region_batch_kernel`, every route (a) / (a1) call starts with ONE `region_warp_kernel` and owns the kernels up to the next
    `region_*` kernel; the order of the calls is the order `batches` made them in (calls.json)."""
    with open(calls_json) as f:
        record = [r for r in json.load(f) if "calls" in r]
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    if len(files) != 1:
        raise SystemExit(f"expected one *kernel_trace.csv under {trace_dir}, found {files}")
    with open(files[0]) as f:
        rows = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))
    calls = []                                                   # [first kernel's name, launches, ns, {name: count}]
    for r in rows:
        name = r["Kernel_Name"]
        if "region_batch_kernel" in name or "region_warp_kernel" in name or not calls:
            calls.append([name, 0, 0, {}])
        c = calls[-1]
        c[1] += 1
        c[2] += int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
        short = name.split("(")[0][-70:]
        c[3][short] = c[3].get(short, 0) + 1
    want = sum(r["calls"] for r in record)
    print(f"{len(rows)} kernel dispatches in {len(calls)} calls ({want} made)")
    if len(calls) != want:
        raise SystemExit("the trace does not split into the calls that were made")
    k = 0
    for r in record:
        mine, k = calls[k: k + r["calls"]], k + r["calls"]
        head = "region_batch_kernel" if r["route"] == "b" else "region_warp_kernel"
        if not all(head in c[0] for c in mine):
            raise SystemExit(f"route ({r['route']}) at {r['pages']} pages: a call does not start with {head}")
        launches = sorted(c[1] for c in mine)
        ns = sorted(c[2] for c in mine)
        names = {}
        for c in mine:
            for nm, cnt in c[3].items():
                names[nm] = names.get(nm, 0) + cnt
        print(f"{r['pages']:2d} pages, route ({r['route']}): {r['calls']} calls, {r['lines']} lines in {r['buckets']} buckets, "
              f"{r['result_bytes']} result bytes; kernel launches per call {launches[0]}..{launches[-1]} (median "
              f"{launches[len(launches) // 2]}); kernel time per call median {ns[len(ns) // 2] / 1e3:.1f} us (min {ns[0] / 1e3:.1f}, max "
              f"{ns[-1] / 1e3:.1f}); peak device memory over a call {r['peak_bytes_over_call'] / 1e6:.1f} MB; wall "
              f"{r['wall_ms_per_call']} ms, events {r['event_ms_per_call']} ms per call; {len(names)} different kernels")
        for nm, cnt in sorted(names.items(), key=lambda kv: -kv[1])[:(2 if r["route"] == "b" else 6)]:
            print(f"      {cnt / r['calls']:8.1f} per call  {nm}")


if __name__ == "__main__":
    {"detect": detect, "warp": warp, "batches": batches, "report": report}[sys.argv[1]](*sys.argv[2:])
