"""Randomised stress of the DB text-line stage (`postproc.SegRepresenter`: two GPU labelling passes + contour tables, hull /
min-area rectangle / Clipper unclip on the host) against the oracle's `boxes_from_bitmap` (contour walk + polygon fill;
reference utils/db_utils.py:123-211) on maps that are NOT text-like: smoothed noise at several scales (speckle, holes, islands
in holes), thresholded gradients, rotated bars, maps touching every border (tests/sweep_cases.py `db_map`).  DB_STRESS_N cases (default 120), DB_STRESS_SEED."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import pkg          # noqa: E402
from oracle import postproc_ref as R   # noqa: E402
from sweep_cases import db_map         # noqa: E402

p = pkg()
rep = p.postproc.SegRepresenter()
n_cases = int(os.environ.get("DB_STRESS_N", "120"))
rng = np.random.RandomState(int(os.environ.get("DB_STRESS_SEED", "1")))
bad = 0
for case in range(n_cases):
    pr, what = db_map(case, rng)
    H, W = pr.shape
    t = torch.from_numpy(pr)[None].cuda()
    boxes, scores = rep(t, (t > 0.3).to(torch.uint8))
    rb, rs = R.boxes_from_bitmap(pr, pr > 0.3, W, H)
    if len(boxes[0]) != len(rb) or not np.array_equal(boxes[0], rb) or not np.allclose(scores[0], rs, rtol=0, atol=1e-6):
        bad += 1
        nd = int((np.asarray(boxes[0]).reshape(len(rb), -1) != np.asarray(rb).reshape(len(rb), -1)).any(1).sum()) if len(boxes[0]) == len(rb) else -1
        print(f"{what}: {len(boxes[0])} vs {len(rb)} boxes, {nd} differ", flush=True)
print(f"db stress: {n_cases} cases, {bad} mismatches")
sys.exit(1 if bad else 0)
