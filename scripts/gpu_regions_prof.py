#!/usr/bin/env python3
"""OCR line crops (`regions.line_regions`) at the benchmark's shape, in two processes so that a kernel trace of the
second holds nothing but the crops' own launches:

    python scripts/gpu_regions_prof.py detect blocks.pkl          # 32 text-like 1024x1024 pages through the benchmark's detector
    rocprofv3 --kernel-trace --stats -d out -o regions -- \\
        python scripts/gpu_regions_prof.py warp blocks.pkl         # line_regions on 32 / 8 / 1 of those pages, CALLS times each

`warp` prints per page count: lines, crop bytes, wall time per call and GPU time per call (events around the call); the trace's
kernel statistics then show `region_warp_kernel` exactly once per call whatever the line count, and nothing else."""
import importlib
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


if __name__ == "__main__":
    {"detect": detect, "warp": warp}[sys.argv[1]](sys.argv[2])
