"""GPU: per-op times of the C3 chains at the benchmark shape with the bottleneck (+ cv3) kernel of the 64 / 128-channel C3
blocks (csrc/kernels_c3b.hip, fuse bit 8) and the other round-5 multi-layer kernels on and off.

    python scripts/gpu_c3b_check.py [time]

The comparison with the launches they replace (`check`) is in the suite now:
tests/test_gpu_edge.py::test_c3b_tilings_equal_the_layer_per_launch_program_bit_for_bit (every tiling, both K walks, leaky
and relu heads) and ::test_fused_blocks_equal_the_per_layer_program_for_silu_and_relu_heads.
"""
import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
pkg = importlib.import_module("comic-text-detector_amd")
L = pkg._lib


def tune(key, value):
    L.check(L.lib().ctd_tuning_set(key.encode(), int(value)), "ctd_tuning_set " + key)


def check():
    print("the check is part of the suite: pytest -m gpu tests/test_gpu_edge.py -k 'c3b_tilings or fused_blocks' compares the\n"
          "network outputs of every tiling of c3b_kernel (c3b_cfg64 x c3b_cfg128), both K walks of the absorbed 3x3 and the head\n"
          "activations with the per-layer program, bit for bit, and asserts by op_kernels() which tiling ran")
    return 0


def time_chains():
    ck = pkg.synth.make_checkpoint(0)
    be = pkg.backend.HipTextDetBackend(ck, device="cuda", precision="fp16")
    x = torch.randint(0, 256, (32, 1024, 1024, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(1)).cuda()
    variants = [("unfused", 7, 0, 0), ("c3b 0/0", 15, 0, 0), ("c3b 0/1", 15, 0, 1), ("+post1x1", 31, 0, 1), ("+segtaps", 63, 0, 1)]
    rows = {}
    for name, fuse, c64, c128 in variants:
        tune("fuse", fuse)
        tune("c3b_cfg64", c64)
        tune("c3b_cfg128", c128)
        for _ in range(3):
            be.forward_u8(x)
        torch.cuda.synchronize()
        acc = None
        for _ in range(5):
            p = be.profile(x)
            acc = p["ms"] if acc is None else acc + p["ms"]
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(5):
            be.forward_u8(x)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(40):
            be.forward_u8(x)
        e1.record()
        torch.cuda.synchronize()
        rows[name] = (acc / 5, p["names"], e0.elapsed_time(e1) / 40)
    tune("fuse", 63)
    tune("c3b_cfg64", 0)
    tune("c3b_cfg128", 1)
    names = rows["unfused"][1]
    print(f"{'op (ms per 32 pages)':44s} " + " ".join(f"{n:>9s}" for n, *_ in variants))
    tot = np.zeros(len(variants))
    chain = np.zeros(len(variants))
    for i, n in enumerate(names):
        v = np.array([rows[k][0][i] for k, *_ in variants])
        tot += v
        if ".m." in n or n.endswith("cv3.conv") or n.endswith(".cv3"):
            chain += v
        if ((".m." in n and "cv1" in n) or n.endswith("conv.1") or "upconv5.conv.0.cv1+cv2" in n or n == "db.conv.0" or n == "seg.upconv6") and v.max() > 0.05:
            print(f"{n:44s} " + " ".join(f"{q:9.4f}" for q in v))
    print(f"{'bottleneck + cv3 ops':44s} " + " ".join(f"{q:9.4f}" for q in chain))
    print(f"{'all ops (sum of per-op events)':44s} " + " ".join(f"{q:9.4f}" for q in tot))
    print(f"{'forward, 40 back to back':44s} " + " ".join(f"{rows[k][2]:9.4f}" for k, *_ in variants))


if __name__ == "__main__":
    what = sys.argv[1:] or ["time"]
    rc = 0
    if "check" in what:
        rc = check()
    if "time" in what:
        time_chains()
    sys.exit(1 if rc else 0)
