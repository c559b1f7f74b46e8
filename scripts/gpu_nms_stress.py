"""Randomised stress of the GPU NMS (`backend.nms`: ctd launch_nms) against the oracle's restatement of
`non_max_suppression` (reference utils/yolov5_utils.py:124-218): row counts 50 .. 70 000, candidate fractions 0 .. 1, box sizes
from dense overlap to sparse, duplicated boxes with equal scores (tests/sweep_cases.py `nms_case`).  NMS_STRESS_N cases (default 200), NMS_STRESS_SEED."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import pkg          # noqa: E402
from oracle import postproc_ref as R   # noqa: E402
from sweep_cases import nms_case       # noqa: E402

p = pkg()
n_cases = int(os.environ.get("NMS_STRESS_N", "200"))
rng = np.random.RandomState(int(os.environ.get("NMS_STRESS_SEED", "1")))
bad = 0
for case in range(n_cases):
    b, what = nms_case(case, rng)
    B = len(b)
    dets, counts = p.backend.nms(torch.from_numpy(b).cuda(), 0.4, 0.35)
    torch.cuda.synchronize()
    ref = R.non_max_suppression(b, 0.4, 0.35)
    for i in range(B):
        n = int(counts[i])
        if n != len(ref[i]) or not np.array_equal(dets[i, :n].cpu().numpy(), ref[i]):
            bad += 1
            print(f"{what} page {i}: {n} vs {len(ref[i])} detections", flush=True)
            break
print(f"nms stress: {n_cases} cases, {bad} mismatches")
sys.exit(1 if bad else 0)
