"""Randomised checks without a test file of their own (round 6): (1) `backend.resize_linear_u8` (ctd_resize_linear_u8) against the
oracle's restatement of cv2.resize(INTER_LINEAR) on random source / destination shapes, 1 and 3 channels, with and without a
canvas; (2) `TextDetector.detect_batch` on pages of DIFFERENT sizes in one batch against the same pages one at a time (letterbox
per page, one forward, per-page inverse mapping) -- masks, refined masks and blocks identical.  Cases: tests/sweep_cases.py
`resize_case`, `mixed_size_batches`.  RB_STRESS_N, RB_STRESS_SEED."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import pkg, checkpoint          # noqa: E402
from oracle import cv_ref as cv             # noqa: E402
from test_post_host import blocks_equal     # noqa: E402
from sweep_cases import mixed_size_batches, resize_case   # noqa: E402

p = pkg()
n_cases = int(os.environ.get("RB_STRESS_N", "150"))
rng = np.random.RandomState(int(os.environ.get("RB_STRESS_SEED", "1")))
bad = 0
for case in range(n_cases):
    img, dst_hw, canvas, what = resize_case(case, rng)
    got = p.backend.resize_linear_u8(torch.from_numpy(img).cuda(), dst_hw, canvas).cpu().numpy()
    ref = np.zeros(got.shape, np.uint8)
    ref[: dst_hw[0], : dst_hw[1]] = cv.resize_linear_u8(img, (dst_hw[1], dst_hw[0]))
    if not np.array_equal(got, ref):
        bad += 1
        print(f"{what}: {int((got != ref).sum())} differing values", flush=True)
print(f"resize stress: {n_cases} cases, {bad} mismatches")
size = 256
det = p.detector.TextDetector(checkpoint(), input_size=size, device="cuda", precision="fp32s")
bad2 = 0
for case, pages, mode, keep in mixed_size_batches(max(4, n_cases // 10), int(os.environ.get("RB_STRESS_SEED", "1"))):
    batch = det.detect_batch(pages, mode, keep)
    for i, (pg, (m, r, bl)) in enumerate(zip(pages, batch)):
        m1, r1, bl1 = det(pg, mode, keep)
        try:
            np.testing.assert_array_equal(m, m1)
            np.testing.assert_array_equal(r, r1)
            blocks_equal(bl, bl1)
        except AssertionError as e:
            bad2 += 1
            print(f"batch case {case} page {i} {pg.shape}: {str(e)[:120]}", flush=True)
print(f"mixed-size batch against single calls: {max(4, n_cases // 10)} batches, {bad2} mismatching pages")
sys.exit(1 if bad or bad2 else 0)
