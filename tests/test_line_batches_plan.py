"""`regions.batch_plan` (the width buckets of `line_batches`) and `regions.value_tables` (its normalisation) -- host code, no
GPU.  Every property is checked from its statement, not from the function's own output."""
import numpy as np
import pytest
import torch

from conftest import pkg


def _cases():
    rng = np.random.default_rng(5)
    every = np.arange(1, 701)
    cases = {
        "1..700 shuffled": (rng.permutation(every), np.ones(700, bool)),
        "1..700 descending": (every[::-1].copy(), np.ones(700, bool)),
        "many ties": (rng.integers(40, 46, 333), np.ones(333, bool)),
        "one width": (np.full(37, 48), np.ones(37, bool)),
        "invalid first, middle, last": (np.array([0, 0, 17, 300, 17, 0, 0, 9, 64, 65, 63, 1, 0]),
                                        np.array([0, 0, 1, 1, 1, 0, 0, 1, 1, 1, 1, 1, 0], bool)),
        "valid flag with width 0, width with invalid flag": (np.array([0, 12, 5, 0, 12]), np.array([1, 0, 1, 1, 1], bool)),
        "seeded with holes": (rng.integers(0, 701, 500), rng.random(500) > 0.2),
        "one line": (np.array([123]), np.array([True])),
        "all invalid": (np.zeros(9, np.int64), np.zeros(9, bool)),
        "empty": (np.zeros(0, np.int64), np.zeros(0, bool)),
    }
    return cases


PARAMS = [dict(), dict(max_batch=4, width_multiple=1), dict(max_batch=1, width_multiple=32), dict(max_batch=7, width_multiple=8,
          max_width=64), dict(max_batch=None), dict(max_batch=None, width_multiple=16, max_width=48), dict(max_batch=1000,
          width_multiple=3, max_width=699)]


@pytest.mark.parametrize("kw", PARAMS, ids=[str(sorted(k.items())) for k in PARAMS])
def test_batch_plan_properties(kw):
    R = pkg().regions
    for name, (widths, valid) in _cases().items():
        plan = R.batch_plan(widths, valid, **kw)
        order, bounds, bw, cut = plan.order, plan.bounds, plan.batch_width, plan.cut
        max_batch = kw.get("max_batch", 16)
        mult = kw.get("width_multiple", 8)
        max_width = kw.get("max_width")
        want = [i for i in range(len(widths)) if valid[i] and widths[i] >= 1]
        # every valid line exactly once
        assert order.dtype == np.int64 and sorted(order.tolist()) == want, name
        w = np.asarray(widths)[order]
        # widths non-decreasing, equal widths in line order
        assert (np.diff(w) >= 0).all(), name
        assert all(order[j] < order[j + 1] for j in range(len(order) - 1) if w[j] == w[j + 1]), name
        # cut
        assert np.array_equal(cut, w if max_width is None else np.minimum(w, max_width)), name
        K = len(bw)
        assert bounds.shape == (K + 1,) and bounds[0] == 0 and bounds[-1] == len(order), name
        if not want:
            assert K == 0 and len(order) == 0 and len(cut) == 0, name
            continue
        sizes = np.diff(bounds)
        if max_batch is None:
            assert K == 1, name
        else:
            assert (sizes >= 1).all() and (sizes <= max_batch).all() and (sizes[:-1] == max_batch).all(), name
            assert K == -(-len(order) // max_batch), name
        for k in range(K):
            c = cut[bounds[k]: bounds[k + 1]]
            top = int(c.max())
            assert bw[k] == -(-top // mult) * mult and bw[k] % mult == 0 and (bw[k] >= c).all() and bw[k] - top < mult, (name, k)
            if max_width is not None:
                assert bw[k] <= max_width


def test_batch_plan_fixed_example():
    R = pkg().regions
    #                    0  1  2  3   4   5  6   7
    plan = R.batch_plan([5, 0, 3, 3, 700, 9, 5, 64], [1, 1, 1, 1, 1, 0, 1, 1], max_batch=2, width_multiple=8, max_width=64)
    assert plan.order.tolist() == [2, 3, 0, 6, 7, 4]
    assert plan.bounds.tolist() == [0, 2, 4, 6]
    assert plan.batch_width.tolist() == [8, 8, 64]
    assert plan.cut.tolist() == [3, 3, 5, 5, 64, 64]
    one = R.batch_plan([5, 0, 3, 3, 700, 9, 5, 64], [1, 1, 1, 1, 1, 0, 1, 1], max_batch=None, width_multiple=1)
    assert one.bounds.tolist() == [0, 6] and one.batch_width.tolist() == [700] and one.cut.tolist() == [3, 3, 5, 5, 64, 700]


def test_batch_plan_rejects_a_max_width_off_the_multiple():
    R = pkg().regions
    with pytest.raises(ValueError):
        R.batch_plan([10, 20], [True, True], width_multiple=8, max_width=60)
    with pytest.raises(ValueError):
        R.batch_plan([10, 20], [True, True], width_multiple=8, max_width=4)
    R.batch_plan([10, 20], [True, True], width_multiple=1, max_width=61)
    with pytest.raises(ValueError):
        R.batch_plan([10, 20], [True], width_multiple=8)
    with pytest.raises(ValueError):
        R.batch_plan([10, 20], [True, True], max_batch=0)


@pytest.mark.parametrize("dtype,npdt", [(torch.float16, np.float16), (torch.float32, np.float32)])
def test_value_tables_are_the_numpy_expression(dtype, npdt):
    R = pkg().regions
    v = np.arange(256, dtype=np.float32)
    bits = {np.float16: np.uint16, np.float32: np.uint32}[npdt]
    for ch, mean, std in [(3, 127.5, 127.5), (1, 127.5, 127.5), (3, 0.0, 255.0), (1, [114.0], [57.5]),
                          (3, [123.675, 116.28, 103.53], [58.395, 57.12, 57.375]), (3, 127.5, [1.0, 2.0, 3.0]),
                          (3, [0.1, 0.2, 0.3], 0.7)]:
        t = R.value_tables(dtype, ch, mean, std)
        assert t.shape == (ch, 256) and t.dtype == npdt
        m = np.broadcast_to(np.asarray(mean, np.float32).reshape(-1), (ch,))
        s = np.broadcast_to(np.asarray(std, np.float32).reshape(-1), (ch,))
        for c in range(ch):
            want = ((v - m[c]) / s[c]).astype(npdt)
            assert np.array_equal(t[c].view(bits), want.view(bits)), (ch, mean, std, c)
    assert np.array_equal(R.value_tables(npdt, 3)[0].view(bits), ((v - np.float32(127.5)) / np.float32(127.5)).astype(npdt).view(bits))
    with pytest.raises(ValueError):
        R.value_tables(dtype, 3, [1.0, 2.0], 1.0)                # neither a scalar nor one per channel
    with pytest.raises(ValueError):
        R.value_tables(torch.float64, 3)


def test_uint8_tables_are_the_identity_and_take_no_normalisation():
    R = pkg().regions
    t = R.value_tables(torch.uint8, 3)
    assert t.dtype == np.uint8 and np.array_equal(t, np.tile(np.arange(256, dtype=np.uint8), (3, 1)))
    with pytest.raises(ValueError):
        R.value_tables(torch.uint8, 3, mean=0.0)
    with pytest.raises(ValueError):
        R.value_tables(torch.uint8, 3, std=[1.0, 1.0, 1.0])


def test_batch_job_mirror_has_the_c_layout():
    """`BATCH_JOB_DTYPE` / `_lib.CtdRegionBatchJob` against the header, compiled: size and every field's offset."""
    import ctypes as C
    import os
    import subprocess
    import tempfile
    from conftest import ROOT
    p = pkg()
    L, R = p._lib, p.regions
    prog = r'''
    #include <stdio.h>
    #include <stddef.h>
    #include "ctd_hip.h"
    int main(void){ printf("%zu %zu %zu %zu %zu %zu %zu %d\n", sizeof(ctd_region_job), sizeof(ctd_region_batch_job),
        offsetof(ctd_region_batch_job, warp), offsetof(ctd_region_batch_job, slot), offsetof(ctd_region_batch_job, rows),
        offsetof(ctd_region_batch_job, Wk), offsetof(ctd_region_batch_job, cut), CTD_ABI_VERSION); return 0; }
    '''
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c")
        open(c, "w").write(prog)
        exe = os.path.join(d, "t")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        vals = [int(v) for v in subprocess.check_output([exe]).split()]
    J = L.CtdRegionBatchJob
    assert vals == [120, C.sizeof(J), J.warp.offset, J.slot.offset, J.rows.offset, J.Wk.offset, J.cut.offset, L.ABI_VERSION]
    f = R.BATCH_JOB_DTYPE.fields
    assert vals[1:7] == [R.BATCH_JOB_DTYPE.itemsize] + [f[k][1] for k in ("warp", "slot", "rows", "Wk", "cut")]
    assert vals[7] == 10
