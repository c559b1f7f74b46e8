"""CPU tests of `bench.py --dump-outputs`: the arrays written for one end-to-end batch (blocks, lines, a seeded sample of
the masks) and for the network-only step, their dtypes and the 64 MB limit."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, pkg

sys.path.insert(0, ROOT)


def fake_batch(n_pages=6, h=64, w=48, seed=0):
    TB = pkg().textblock
    rng = np.random.RandomState(seed)
    res = []
    for p in range(n_pages):
        mask = rng.randint(0, 256, (h, w)).astype(np.uint8)
        refined = rng.randint(0, 2, (h, w)).astype(np.uint8) * 255
        blks = []
        for b in range(p % 3):
            lines = [[[1 + b, 2], [30, 2], [30, 9 + p], [1 + b, 9 + p]], [[1, 12], [30, 12], [30, 20], [1, 20]]]
            blks.append(TB.TextBlock([1 + b, 2, 30, 20], lines, language=("ja", "eng", "unknown")[b], vertical=bool(b),
                                     font_size=8.5 + b, distance=[0.0, 10.0], angle=b, vec=[1.0, 0.0], norm=28.0,
                                     merged=b == 1, weight=0.5))
        res.append((mask, refined, blks))
    return res


def test_e2e_outputs_are_float_arrays_of_the_whole_batch(tmp_path):
    import bench
    res = fake_batch()
    arr = bench.e2e_output_arrays(res)
    shapes = bench.write_outputs(str(tmp_path), arr)
    assert set(shapes) == {"mask_pages", "mask_stride", "mask", "mask_refined", "blocks", "lines", "blocks_per_page"}
    for name in shapes:
        a = np.load(os.path.join(tmp_path, name + ".npy"))
        assert a.dtype in (np.float32, np.float64) and list(a.shape) == shapes[name]
    pick = arr["mask_pages"].astype(int)
    assert len(pick) == bench.DUMP_MASK_PAGES and np.all(np.diff(pick) > 0)
    np.testing.assert_array_equal(arr["mask"], np.stack([res[i][0] for i in pick]).astype(np.float32))
    np.testing.assert_array_equal(arr["mask_refined"], np.stack([res[i][1] for i in pick]).astype(np.float32))
    assert arr["blocks"].shape == (sum(p % 3 for p in range(6)), len(bench.BLOCK_COLUMNS))
    assert arr["lines"].shape == (2 * arr["blocks"].shape[0], len(bench.LINE_COLUMNS))
    np.testing.assert_array_equal(arr["blocks_per_page"], [p % 3 for p in range(6)])
    row = arr["blocks"][arr["blocks"][:, 0] == 5][1]                  # page 5, block 1
    assert list(row) == [5, 1, 2, 2, 30, 20, 1, 0, 9.5, 1, 1, 0, 28, 0.5, 1, 2]
    line = arr["lines"][(arr["lines"][:, 0] == 5) & (arr["lines"][:, 1] == 1)][0]
    assert list(line) == [5, 1, 0, 2, 2, 30, 2, 30, 14, 2, 14, 0.0]
    again = bench.e2e_output_arrays(fake_batch())                     # same results -> same arrays (the sample is seeded)
    for k in arr:
        np.testing.assert_array_equal(arr[k], again[k])


def test_e2e_outputs_stay_within_the_limit_on_large_pages():
    import bench
    res = fake_batch(n_pages=5, h=3000, w=2900)
    arr = bench.e2e_output_arrays(res)
    total = sum(a.nbytes for a in arr.values())
    assert total <= bench.DUMP_LIMIT_BYTES
    s = int(arr["mask_stride"][0])
    assert s > 1 and arr["mask"].shape[1:] == res[0][0][::s, ::s].shape


def test_net_outputs_and_the_checks_of_the_writer(tmp_path):
    import bench
    dets, counts = torch.rand(4, 100, 6, dtype=torch.float16), torch.tensor([3, 0, 100, 7], dtype=torch.int32)
    arr = bench.net_output_arrays(dets, counts)
    assert arr["dets"].dtype == np.float32 and arr["counts"].dtype == np.float64
    bench.write_outputs(str(tmp_path), arr)
    with pytest.raises(TypeError):
        bench.write_outputs(str(tmp_path), {"x": np.zeros(3, np.uint8)})
    with pytest.raises(ValueError):
        bench.write_outputs(str(tmp_path), {"x": np.zeros(bench.DUMP_LIMIT_BYTES // 8 + 1, np.float64)})
