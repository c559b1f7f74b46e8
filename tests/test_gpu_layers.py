"""-m gpu: every op of every engine against a float64 recomputation of that op from the engine's own stored inputs, with
the error bound derived from the engine's arithmetic (tests/layer_ref.py) -- a per-layer check where the rest of the
suite compares only the end of the forward with a reference, or one HIP kernel with another.

Engines run with `no_reuse` = 1 (every activation stays readable) and `fuse` = 0 (one launch per op: the multi-layer
kernels are tied to the per-layer program bit for bit by tests/test_gpu_edge.py); in-place C3 slices are read through
identity-copy snapshots (layer_ref.snapshot_program).  The coverage test asserts that every kernel the timed B = 32
dispatch launches is among the kernels checked here, or is a multi-layer kernel listed with the test that ties it to
the per-layer program.

The timed dispatch.  `timed_u8_32x1024x1024` is bench.py's shape with its checkpoint and first batch
(test_gpu_dispatch.workload) at the DEFAULT thresholds, fuse = 0, no_reuse = 1, all three engines, one engine alive at a
time: the grids, page counts and tensor sizes (up to 1.3 GB of the 2 GiB byte-offset budget on the fp16 engine; no split on
the other two) of the published number, which the small configs reach only through forced tuning keys.  Pages
TIMED_PAGES = (0, 1, 15, 16, 18, 20, 30, 31): both ends with their neighbours, an adjacent middle pair and two seeded
random ones; every op is checked on each of them, the maps above 128 x 128 on the windows of layer_ref.EDGES (77 per
page of a 1024 map).  The coverage test then asserts PER OP that the default run (fuse = 63, B = 32) launches, for every op,
the kernel that was checked for that op here, or a multi-layer kernel of FUSED (bit for bit at B = 32 in
tests/test_gpu_edge.py).

Measured on the MI355X, B = 32, no_reuse = 1:

  engine   workspace_bytes()   wall time of the config   ops checked   worst ratio (op, kernel, page)
  fp16     12 447 645 696      68 s (set-up + fwd 0.5 s)    102           0.999  seg.down_conv1.down, avgpool2_kernel, page 0
  fp32     25 366 102 016      37 s (set-up + fwd 0.8 s)    103           0.992  input, input_kernel, page 0
  fp32s    25 366 102 016      82 s (set-up + fwd 1.0 s)    102           0.496  model.24.decode0, detect_decode_kernel, page 30

  The checker keeps at most 0.94 GB of engine tensors (the requested pages only, a tensor is dropped after its last
  reader); peak RSS of the pytest process running this file 7.1 GB (read_tensor hands out all 32 pages of a tensor as f32,
  up to 2.1 GB, before the pages are cut out).  It looks at 14 % of the elements the ops wrote (58 % at B = 2).

  worst |engine - f64| / bound per (engine, kernel)      B <= 3    B = 32
  fp16   avgpool2_kernel                                 1.000     0.999
  fp16   conv_halo3_kernel                               0.454     0.389
  fp16   conv_halo_kernel                                0.992     0.743
  fp16   conv_igemm_kernel                               0.959     0.694
  fp16   db_up_mfma_kernel                               0.166     0.0733
  fp16   detect_decode_kernel                            0.499     0.495
  fp16   seg_final_mfma_kernel                           0.388     0.116
  fp16   stem_mfma_kernel                                0.206     0.167
  fp32   avgpool2_kernel                                 0.633     0.600
  fp32   conv_f32_mfma_kernel                            0.486     0.232
  fp32   db_up_kernel                                    0.166     0.0634
  fp32   detect_decode_kernel                            0.496     0.495
  fp32   input_kernel                                    0.992     0.992
  fp32   seg_final_f32_kernel                            0.0823    0.0532
  fp32s  avgpool2_kernel                                 0.308     0.292
  fp32s  conv_split_halo_kernel                          0.0399    0.0590
  fp32s  conv_split_kernel                               0.968     0.201
  fp32s  db_up_kernel                                    0.140     0.0394
  fp32s  detect_decode_kernel                            0.498     0.496
  fp32s  seg_final_f32_kernel                            0.0728    0.0481
  fp32s  stem_split_kernel                               0.150     0.0441
  (maxpool_kernel: exact on every engine.  B <= 3 includes the wide-range checkpoint and the forced dispatches; the B = 32
  column is the benchmark's checkpoint.  The fp16 avgpool value is 0.9996: the bound is tight for a mean of fp16 values.)

Time.  The config adds 186 s, nearly all of it float64 convolution on the host (mostly the maps up to 128 x 128, checked in
full); with the wider window set on the small configs the file takes 288 s where it took 99 s, and the per-file wall time
of the whole -m gpu suite went from 340 s to 530 s in the same visit (+56 %, above the third aimed at).  The page set is
the smallest the plan allows, so no page was cut -- and no seam class or op ever is.  For the same reason the wide-range
checkpoint (wide_ckpt.py) is NOT run at B = 32: it stays at forced_3x320x448.
"""
import resource
import time

import numpy as np
import pytest
import torch

from conftest import checkpoint, pkg
from layer_ref import ENGINES, LayerCheck, snapshot_program
from oracle import gen_golden
from oracle.net_ref import OracleNet
from wide_ckpt import make_wide_checkpoint

pytestmark = pytest.mark.gpu

# name -> (shape, uint8 input, force the halo / halo3 kernels onto every map)
CONFIGS = {
    "u8_2x1024x1024": ((2, 1024, 1024), True, False),
    "1x640x1024": ((1, 640, 1024), False, False),
    "forced_3x320x448": ((3, 320, 448), False, True),
    "forced_1x64x64": ((1, 64, 64), False, True),
    # bench.py's shape, checkpoint and first batch (test_gpu_dispatch.workload) at the DEFAULT thresholds
    "timed_u8_32x1024x1024": ((32, 1024, 1024), True, False),
}
TIMED = "timed_u8_32x1024x1024"
# the pages checked at B = 32: both ends with their neighbours, an adjacent middle pair, two seeded random ones
TIMED_PAGES = tuple(sorted({0, 1, 15, 16, 30, 31} | {int(b) for b in np.random.RandomState(32).choice(
    [b for b in range(32) if b not in (0, 1, 15, 16, 30, 31)], 2, replace=False)}))
# multi-layer kernels of the timed dispatch, each tied to the per-layer program by an existing test
FUSED = {
    "c3_fused_kernel": "test_gpu_edge.py::test_fused_blocks_equal_the_layer_per_launch_program_bit_for_bit (fuse bit 2)",
    "c3b_kernel": "test_gpu_edge.py::test_fused_blocks_equal_the_layer_per_launch_program_bit_for_bit (fuse bit 8)",
    "conv_halo3_kernel+1x1": "test_gpu_edge.py::test_fused_blocks_equal_the_layer_per_launch_program_bit_for_bit (bit 16)",
    "conv_halo3_kernel+taps": "test_gpu_edge.py::test_fused_blocks_equal_the_layer_per_launch_program_bit_for_bit (bit 32)",
    "seg_final_gather_kernel": "test_gpu_edge.py::test_fused_blocks_equal_the_layer_per_launch_program_bit_for_bit (bit 32)",
    "stem_conv2_kernel": "test_gpu_edge.py::test_fused_blocks_equal_the_layer_per_launch_program_bit_for_bit (fuse bit 1)",
    "sppf_pool3_kernel": "test_gpu_edge.py::test_fused_blocks_equal_the_layer_per_launch_program_bit_for_bit (fuse bit 4)",
    "(fused)": "the op's work is done by the launch of the op next to it (one of the kernels above, or stem_split_kernel "
               "reading the page for the input op)",
}
_DEFAULTS = ((b"no_reuse", 0), (b"fuse", 63), (b"halo_min_patches", 1024), (b"halo3_min_blocks", 1024))
_S = {}
TABLE = {}          # (engine, kernel) -> worst ratio at B <= 3
TABLE32 = {}        # (engine, kernel) -> worst ratio at B = 32
STATS = {}          # engine -> measurements of the B = 32 run


def _tune(key, value):
    L = pkg()._lib
    L.check(L.lib().ctd_tuning_set(key, value), "ctd_tuning_set")


def _engine(ck, prec, prog, act):
    """A backend that runs `prog` (the lowering of `ck`, possibly with snapshot copies) instead of lowering `ck` again."""
    B = pkg().backend
    lower = B.graph.lower
    B.graph.lower = lambda *a, **k: prog
    try:
        return B.HipTextDetBackend(ck, device="cuda", precision=prec, act=act)
    finally:
        B.graph.lower = lower


def _input(shape, u8, seed):
    B, H, W = shape
    if u8:
        x = torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(seed))
        return x, x.permute(0, 3, 1, 2).double().numpy() / 255.0
    x = gen_golden.make_input(seed, shape)
    return x, x.double().numpy()


def run_checks(engine, config, ck_key="synth0", act="leaky"):
    key = (engine, config, ck_key, act)
    if key in _S:
        return _S[key]
    p = pkg()
    L = p._lib
    shape, u8, forced = CONFIGS[config]
    timed = config == TIMED
    t0 = time.time()
    if timed:
        from test_gpu_dispatch import workload
        assert ck_key == "synth0" and act == "leaky"
        ck, pages = workload()
        x = torch.from_numpy(np.stack(pages))
        assert tuple(x.shape) == shape + (3,) and x.dtype == torch.uint8
        page = x.permute(0, 3, 1, 2).numpy()                 # uint8 here; / 255 in f64 on the pages that are kept
    else:
        ck = checkpoint(0) if ck_key == "synth0" else _wide(act)
        x, page = _input(shape, u8, 11)
    prec = {"fp32": L.PREC_F32, "fp32s": L.PREC_F32S, "fp16": L.PREC_F16}[engine]
    prog = p.graph.lower(ck, prec, act=act)
    snap, index, snaps = snapshot_program(prog)
    xd = x.cuda()
    fwd = (lambda be: be.forward_u8(xd)) if u8 else (lambda be: be(xd))        # noqa: E731
    try:
        _tune(b"fuse", 0)
        if forced:
            _tune(b"halo_min_patches", 1)
            _tune(b"halo3_min_blocks", 1)
        _tune(b"no_reuse", 0)
        plain = _engine(ck, engine, prog, act)
        fwd(plain)
        torch.cuda.synchronize()
        plain_kernels = plain.op_kernels()
        del plain
        _tune(b"no_reuse", 1)
        be = _engine(ck, engine, snap, act)
        _tune(b"no_reuse", 0)
        blks, mask, lines = fwd(be)
        torch.cuda.synchronize()
        outs = dict(blks=blks.cpu().numpy(), mask=mask.cpu().numpy(), lines=lines.cpu().numpy(),
                    mask_u8=be.mask_u8.cpu().numpy(), bitmap=be.bitmap.cpu().numpy())
        snap_kernels = be.op_kernels()
        workspace = be.workspace_bytes()
    finally:
        for k, v in _DEFAULTS:
            _tune(k, v)
    del xd, blks, mask, lines
    kernels = [snap_kernels[index[i]][1] for i in range(len(prog.ops))]
    # the premise: neither no_reuse nor the snapshot copies change what the program's own ops launch
    assert kernels == [k for _, k in plain_kernels], [(a, b) for a, b in zip(kernels, plain_kernels) if a != b[1]]
    if timed:
        chk = LayerCheck(prog, snaps, engine, be.read_tensor, outs, _PagesOver255(page), u8=True, kernels=kernels, seed=len(_S),
                         pages=TIMED_PAGES)
    else:
        chk = LayerCheck(prog, snaps, engine, be.read_tensor, outs, page, u8=u8, kernels=kernels, seed=len(_S))
    t1 = time.time()
    res = chk.check_all()
    if timed:
        STATS[engine] = dict(workspace_bytes=workspace, forward_s=t1 - t0, check_s=time.time() - t1,
                             checker_peak_tensor_bytes=chk.peak_cached_bytes,
                             process_peak_rss_bytes=resource.getrusage(resource.RUSAGE_SELF).ru_maxrss * 1024)
    del chk, be
    table = TABLE32 if timed else TABLE
    for i, r in res.items():
        r["kernel"] = kernels[i]
        if r["n"]:
            t = (engine, kernels[i])
            table[t] = max(table.get(t, 0.0), r["ratio"])
    _S[key] = res
    return res


class _PagesOver255:
    """(B,3,H,W) uint8 pages that turn into u8 / 255 in float64 only where the checker indexes them (32 pages of 1024 x 1024 in
    f64 are 0.8 GB; the checker keeps eight)."""

    def __init__(self, u8):
        self.u8 = u8

    def __len__(self):
        return len(self.u8)

    def __getitem__(self, idx):
        return np.asarray(self.u8[idx], np.float64) / 255.0


def _wide(act):
    if ("wide", act) not in _S:
        _S[("wide", act)] = make_wide_checkpoint(0, act)
    return _S[("wide", act)]


def _assert_all_within(res, what):
    bad = {f"{i}:{r['name']} ({r['kernel']})": r["ratio"] for i, r in res.items() if not r["ratio"] <= 1.0}
    assert not bad, (what, bad)


@pytest.mark.parametrize("config", sorted(CONFIGS))
@pytest.mark.parametrize("engine", ENGINES)
def test_every_op_within_its_float64_bound(engine, config):
    res = run_checks(engine, config)
    _assert_all_within(res, (engine, config))
    worst = max(res.items(), key=lambda kv: kv[1]["ratio"])
    n, total = sum(r["n"] for r in res.values()), sum(r["total"] for r in res.values() if r["n"])
    print(f"\n{engine} {config}: {sum(r['n'] > 0 for r in res.values())} ops checked, worst ratio "
          f"{worst[1]['ratio']:.3g} at op {worst[0]} {worst[1]['name']} ({worst[1]['kernel']}) page {worst[1]['page']} "
          f"window {worst[1]['win']}; looked at {n / total:.2%} of the elements those ops wrote")
    if config == TIMED:
        assert sorted({r["page"] for r in res.values() if r["page"] is not None} - set(TIMED_PAGES)) == []
        print(f"{engine} {config}: pages {TIMED_PAGES}, {STATS.get(engine)}")


@pytest.mark.parametrize("act", ["leaky", "silu"])
@pytest.mark.parametrize("engine", ENGINES)
def test_wide_range_checkpoint_every_op_within_its_bound(engine, act):
    _assert_all_within(run_checks(engine, "forced_3x320x448", "wide", act), (engine, "wide", act))


@pytest.mark.parametrize("act", ["leaky", "silu"])
@pytest.mark.parametrize("engine", ["fp32", "fp32s"])
def test_wide_range_checkpoint_end_to_end_fp32_bars(engine, act):
    """The fp32-level engines on trained-like BN statistics, default dispatch: the bars of tests/test_gpu_net.py."""
    ck = _wide(act)
    x = gen_golden.make_input(12, (3, 320, 448))
    ob, om, ol = OracleNet(ck, act=act)(x)
    be = pkg().backend.HipTextDetBackend(ck, device="cuda", precision=engine, act=act)
    blks, mask, lines = be(x.cuda())
    torch.cuda.synchronize()
    np.testing.assert_allclose(mask.cpu().numpy(), om.numpy(), rtol=0, atol=2e-5)
    np.testing.assert_allclose(lines.cpu().numpy(), ol.numpy(), rtol=0, atol=2e-5)
    np.testing.assert_allclose(blks.cpu().numpy(), ob.numpy(), rtol=1e-4, atol=2e-3)


def test_every_kernel_of_the_timed_dispatch_is_checked():
    """B = 32 pages of 1024 x 1024 at the default tunings (bench.py's shape): each kernel it launches was checked above
    per op, or is a multi-layer kernel in FUSED."""
    p = pkg()
    checked = {}
    for engine in ENGINES:
        for config in CONFIGS:
            for r in run_checks(engine, config).values():
                if r["n"]:
                    checked.setdefault(engine, set()).add(r["kernel"])
    pages = torch.randint(0, 256, (32, 1024, 1024, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(2)).cuda()
    for engine in ENGINES:
        be = p.backend.HipTextDetBackend(checkpoint(0), device="cuda", precision=engine)
        be.forward_u8(pages)
        torch.cuda.synchronize()
        names = {k for _, k in be.op_kernels()}
        del be
        missing = names - checked[engine] - set(FUSED)
        assert not missing, (engine, missing)
    # per op, not per name: every op of the timed run (default thresholds, fuse = 63, the benchmark's checkpoint and batch) is
    # done by a multi-layer kernel (FUSED: tied to the per-layer program bit for bit at B = 32 by tests/test_gpu_edge.py,
    # test_timed_dispatch_fused_equals_unfused_on_all_32_pages for each engine), or
    # launches the SAME kernel that this op launched in the fuse = 0, B = 32 run whose every op was checked above
    from test_gpu_dispatch import workload
    ck, wpages = workload()
    pages = torch.from_numpy(np.stack(wpages)).cuda()
    for engine in ENGINES:
        res = run_checks(engine, TIMED)
        _assert_all_within(res, (engine, TIMED))
        be = p.backend.HipTextDetBackend(ck, device="cuda", precision=engine)
        be.forward_u8(pages)
        torch.cuda.synchronize()
        timed = be.op_kernels()
        del be
        assert len(timed) == len(res)
        uncovered = [(i, name, kern, res[i]["kernel"]) for i, (name, kern) in enumerate(timed)
                     if not (kern in FUSED or (kern == res[i]["kernel"] and res[i]["n"] > 0))]
        assert not uncovered, (engine, uncovered)
        multi = sum(kern in FUSED for _, kern in timed)
        print(f"\n{engine}: all {len(timed)} ops of the timed B = 32 run are covered: {len(timed) - multi} launch the kernel that "
              f"was checked per op at B = 32, {multi} are done by a multi-layer kernel (bit for bit at B = 32)")
    print("\nworst |engine - f64| / bound per (engine, kernel):        B <= 3     B = 32")
    for engine, kern in sorted(set(TABLE) | set(TABLE32)):
        small, big = TABLE.get((engine, kern)), TABLE32.get((engine, kern))
        print(f"  {engine:6s} {kern:28s} {'-' if small is None else format(small, '.3g'):>10s} "
              f"{'-' if big is None else format(big, '.3g'):>10s}")
    for engine, st in sorted(STATS.items()):
        print(f"  {engine} B = 32 no_reuse: {st}")
