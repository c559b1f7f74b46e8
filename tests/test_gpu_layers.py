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

  worst |engine - f64| / bound per (engine, kernel)      B <= 3    B = 32    keys
  fp16   avgpool2_kernel                                1     0.999     0.999
  fp16   conv_direct_kernel                             -         -       0.4
  fp16   conv_halo3_kernel                          0.454     0.389     0.361
  fp16   conv_halo_kernel                           0.992     0.743     0.712
  fp16   conv_igemm_kernel                          0.959     0.694     0.751
  fp16   convt_direct_kernel                            -         -     0.447
  fp16   db_up_kernel                                   -         -  0.000701
  fp16   db_up_mfma_kernel                          0.166    0.0733     0.131
  fp16   detect_decode_kernel                       0.499     0.495     0.463
  fp16   seg_final_kernel                               -         -     0.246
  fp16   seg_final_mfma_kernel                      0.388     0.116     0.247
  fp16   stem_mfma_kernel                           0.217     0.167     0.207
  fp32   avgpool2_kernel                            0.633       0.6     0.576
  fp32   conv_direct_kernel                             -         -     0.178
  fp32   conv_f32_mfma_kernel                       0.486     0.232         -
  fp32   convt_direct_kernel                            -         -     0.198
  fp32   db_up_kernel                               0.166    0.0634     0.101
  fp32   detect_decode_kernel                       0.496     0.495     0.458
  fp32   input_kernel                               0.992     0.992         0
  fp32   seg_final_f32_kernel                      0.0823    0.0532    0.0665
  fp32s  avgpool2_kernel                            0.308     0.292     0.291
  fp32s  conv_split_halo_kernel                    0.0399     0.059         -
  fp32s  conv_split_kernel                          0.968     0.201    0.0864
  fp32s  db_up_kernel                                0.14    0.0394    0.0796
  fp32s  detect_decode_kernel                       0.498     0.496     0.438
  fp32s  input_kernel                                   -         -         0
  fp32s  seg_final_f32_kernel                      0.0728    0.0481    0.0513
  fp32s  stem_split_kernel                          0.166    0.0441    0.0343
  (maxpool_kernel: exact on every engine.  B <= 3 includes the wide-range checkpoint (leaky, silu, relu) and the forced
  dispatches; the B = 32 column is the benchmark's checkpoint; "keys" is the worst over the KEYED configurations and the
  hand-built direct program, described below.  The fp16 avgpool value is 0.9996: the bound is tight for a mean of fp16
  values.  db_up_kernel on fp16 input keeps the hidden ConvTranspose's output in f32 where the bound allows its fp16
  storage: hence 0.0007.  input_kernel copies a float page exactly.)

Kernels a tuning key selects.  The configs above run the kernels each op gets at the default keys (and two forced thresholds).
KEYED runs the same check -- fuse = 0, no_reuse = 1, snapshot program, ratio <= 1 -- under the keys of ctd_tuning_set that
put another kernel or instantiation behind an op, each with assertions on op_kernels() that the kernel in question ran on
ops with checked elements:

  fp32   f32_mfma = 0 at (1, 64, 64) and (3, 128, 64)         conv_direct_kernel<float, true> on every CONV, convt_direct_kernel<float,
                                                              true> on every CONVT, no *mfma* kernel.  (A sequential fmaf chain in f32
                                                              is the arithmetic of the bound's fp32 row.)
  fp16   db_up_mfma = seg_final_mfma = 0, u8 (3, 128, 64)     db_up_kernel on fp16 input, seg_final_kernel
  fp16   halo_min_patches = 1, halo_pair = 0 / 1              conv_halo_kernel's unpaired path on the 64-output ConvTransposes; the
                                                              network outputs of the two runs are compared as well
  fp16   halo = 0; halo3 = 0 / 1 with the thresholds at 1     conv_igemm_kernel on every 3x3 and ConvTranspose; conv_halo_kernel on the
                                                              ConvTransposes that conv_halo3_kernel takes under halo3 = 1
  fp32s  split_planes = split_halo = split_stem = 0           fp32 tensors everywhere: input_kernel + conv_split_kernel
  fp32s  split_planes = 0                                     conv_split_kernel on fp32 tensors behind stem_split_kernel.
                                                              conv_split_halo_kernel takes split-plane sources only
                                                              (conv_split_halo_supported: x_sp), so it does not run under this key.

The `half` direct kernels are reached by no lowering of the network (the fp16 engine takes them for channel counts that
are no multiple of 32 or pitches that are no multiple of 8) and are the yardstick of the native selftest:
layer_ref.direct_program is a seven-conv program built by hand for them (cin 24 / 40 / 48, cout 20 / 24, channel offsets 3
and 23, two sources with an upsample, 3x3 / s2, a residual into a channel offset, ConvTranspose 4x4 / s2 / p1 and 2x2 / s2 /
p0, silu / leaky / relu / none), run on the fp16 and the fp32 engine, every op on a *_direct_kernel.

The wide-range checkpoint runs with act = "relu" too (the reference's Conv knows 'leaky' and 'relu'), at forced_3x128x64.

The ledger.  DISPATCH_KEYS lists, per key and value, the kernels that prove the value took effect and where they were
checked (float64 here, or bit for bit against the per-layer program in tests/test_gpu_edge.py: the tilings of c3b_kernel,
the multi-layer kernels under silu / relu heads); NOT_DISPATCH_KEYS the keys that select no kernel, with the reason.
tests/test_layer_ref.py reads the keys out of the sources: a key in neither table fails on the CPU.

Measured: every op of every KEYED configuration and of the direct program within its bound (column "keys" above; per op
of the direct program 0.09 ... 0.45 on the fp16 engine, 0.03 ... 0.20 on the fp32 engine); the network outputs under
halo_pair = 0 equal those under halo_pair = 1 bit for bit (max |difference| 0 on all five).  Nothing had to be added to
the bound and no kernel had to be changed.  The additions take 15.6 s of this file's 294 s (sum of the per-test times; the
slowest new case 3.2 s), and 1.0 s of the 15.3 s of tests/test_gpu_edge.py (26 new cases that share cached runs).

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
from layer_ref import ENGINES, LayerCheck, direct_program, snapshot_program
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
# the small shape of the wide-range `relu` checkpoint (leaky and silu cover forced_3x320x448)
SMALL = {"forced_3x128x64": ((3, 128, 64), False, True)}
# Configurations under tuning keys: name -> (engine, shape, uint8 input, keys).  The keys are set before the engines are
# created (`f32_mfma` is read at creation) and put back by `_lib.tuning`.  (3, 128, 64) is the non-square B > 1 shape of the
# suite, (1, 64, 64) takes the maps down to 1 x 1; the kernels these keys select have no tile larger than the maps here.
KEYED = {
    "f32_direct_1x64x64": ("fp32", (1, 64, 64), False, {"f32_mfma": 0}),
    "f32_direct_3x128x64": ("fp32", (3, 128, 64), False, {"f32_mfma": 0}),
    "valu_tails_u8_3x128x64": ("fp16", (3, 128, 64), True, {"db_up_mfma": 0, "seg_final_mfma": 0}),
    "halo_unpaired_3x128x64": ("fp16", (3, 128, 64), False, {"halo_min_patches": 1, "halo_pair": 0}),
    "halo_paired_3x128x64": ("fp16", (3, 128, 64), False, {"halo_min_patches": 1, "halo_pair": 1}),
    "halo_off_3x128x64": ("fp16", (3, 128, 64), False, {"halo_min_patches": 1, "halo": 0}),
    "halo3_off_3x128x64": ("fp16", (3, 128, 64), False, {"halo_min_patches": 1, "halo3_min_blocks": 1, "halo3": 0}),
    "halo3_on_3x128x64": ("fp16", (3, 128, 64), False, {"halo_min_patches": 1, "halo3_min_blocks": 1, "halo3": 1}),
    "fp32_tensors_3x128x64": ("fp32s", (3, 128, 64), False, {"split_planes": 0, "split_halo": 0, "split_stem": 0}),
    "planes_off_3x128x64": ("fp32s", (3, 128, 64), False, {"split_planes": 0}),
}
TIMED = "timed_u8_32x1024x1024"
# the pages checked at B = 32: both ends with their neighbours, an adjacent middle pair, two seeded random ones
TIMED_PAGES = tuple(sorted({0, 1, 15, 16, 30, 31} | {int(b) for b in np.random.RandomState(32).choice(
    [b for b in range(32) if b not in (0, 1, 15, 16, 30, 31)], 2, replace=False)}))
# multi-layer kernels of the timed dispatch, each tied to the per-layer program by an existing test
FUSED = {
    "c3_fused_kernel": "test_gpu_edge.py::test_fused_blocks_equal_the_layer_per_launch_program_bit_for_bit (fuse bit 2)",
    "c3b_kernel": "test_gpu_edge.py::test_fused_blocks_equal_the_layer_per_launch_program_bit_for_bit (fuse bit 8)",
    "c3b_kernel<64,16,2>": "test_gpu_edge.py::test_c3b_tilings_equal_the_layer_per_launch_program_bit_for_bit (c3b_cfg64 = 1)",
    "c3b_kernel<64,8,2>": "test_gpu_edge.py::test_c3b_tilings_equal_the_layer_per_launch_program_bit_for_bit (c3b_cfg64 = 2)",
    "c3b_kernel<128,8,1>": "test_gpu_edge.py::test_c3b_tilings_equal_the_layer_per_launch_program_bit_for_bit (c3b_cfg128 = 0)",
    "conv_halo3_kernel+1x1": "test_gpu_edge.py::test_fused_blocks_equal_the_layer_per_launch_program_bit_for_bit (bit 16)",
    "conv_halo3_kernel+taps": "test_gpu_edge.py::test_fused_blocks_equal_the_layer_per_launch_program_bit_for_bit (bit 32)",
    "seg_final_gather_kernel": "test_gpu_edge.py::test_fused_blocks_equal_the_layer_per_launch_program_bit_for_bit (bit 32)",
    "stem_conv2_kernel": "test_gpu_edge.py::test_fused_blocks_equal_the_layer_per_launch_program_bit_for_bit (fuse bit 1)",
    "sppf_pool3_kernel": "test_gpu_edge.py::test_fused_blocks_equal_the_layer_per_launch_program_bit_for_bit (fuse bit 4)",
    "(fused)": "the op's work is done by the launch of the op next to it (one of the kernels above, or stem_split_kernel "
               "reading the page for the input op)",
}
_S = {}
OUTS = {}           # keyed config -> the network outputs of its run
TABLE = {}          # (engine, kernel) -> worst ratio at B <= 3
TABLEK = {}         # (engine, kernel) -> worst ratio under the tuning keys of KEYED and on the hand-built direct program
TABLE32 = {}        # (engine, kernel) -> worst ratio at B = 32
STATS = {}          # engine -> measurements of the B = 32 run


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
    keys = {}
    if config in KEYED:
        assert (ck_key, act) == ("synth0", "leaky")
        eng, shape, u8, keys = KEYED[config]
        assert eng == engine
        forced = False
    else:
        shape, u8, forced = CONFIGS[config] if config in CONFIGS else SMALL[config]
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
    force = {"halo_min_patches": 1, "halo3_min_blocks": 1} if forced else {}
    with L.tuning({"fuse": 0, **force, **keys, "no_reuse": 0}):
        plain = _engine(ck, engine, prog, act)
        fwd(plain)
        torch.cuda.synchronize()
        plain_kernels = plain.op_kernels()
        del plain
        with L.tuning(no_reuse=1):
            be = _engine(ck, engine, snap, act)
        blks, mask, lines = fwd(be)
        torch.cuda.synchronize()
        outs = dict(blks=blks.cpu().numpy(), mask=mask.cpu().numpy(), lines=lines.cpu().numpy(),
                    mask_u8=be.mask_u8.cpu().numpy(), bitmap=be.bitmap.cpu().numpy())
        snap_kernels = be.op_kernels()
        workspace = be.workspace_bytes()
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
    if keys:
        OUTS[config] = outs
    table = TABLE32 if timed else (TABLEK if keys else TABLE)
    for i, r in res.items():
        r["kernel"] = kernels[i]
        r["kind"], r["cout"], r["k"] = prog.ops[i]["kind"], prog.ops[i]["cout"], prog.ops[i]["k"]
        if r["n"]:
            t = (engine, kernels[i])
            table[t] = max(table.get(t, 0.0), r["ratio"])
    _S[key] = res
    return res


def _print_table():
    print("\nworst |engine - f64| / bound per (engine, kernel):        B <= 3     B = 32       keys")
    fmt = lambda v: "-" if v is None else format(v, ".3g")          # noqa: E731
    for engine, kern in sorted(set(TABLE) | set(TABLE32) | set(TABLEK)):
        print(f"  {engine:6s} {kern:28s} {fmt(TABLE.get((engine, kern))):>10s} {fmt(TABLE32.get((engine, kern))):>10s} "
              f"{fmt(TABLEK.get((engine, kern))):>10s}")


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


def _wide_config(act):
    """`relu` differs from the other two in the heads' activation epilogues only: the small shape is enough for it."""
    return "forced_3x128x64" if act == "relu" else "forced_3x320x448"


@pytest.mark.parametrize("act", ["leaky", "silu", "relu"])
@pytest.mark.parametrize("engine", ENGINES)
def test_wide_range_checkpoint_every_op_within_its_bound(engine, act):
    res = run_checks(engine, _wide_config(act), "wide", act)
    _assert_all_within(res, (engine, "wide", act))
    L = pkg()._lib
    heads = [r for r in res.values() if r["name"].startswith(("seg.", "db.")) and r["kind"] in (L.OP_CONV, L.OP_CONVT)]
    assert heads and all(r["n"] > 0 for r in heads)


@pytest.mark.parametrize("act", ["leaky", "silu", "relu"])
@pytest.mark.parametrize("engine", ["fp32", "fp32s"])
def test_wide_range_checkpoint_end_to_end_fp32_bars(engine, act):
    """The fp32-level engines on trained-like BN statistics, default dispatch: the bars of tests/test_gpu_net.py."""
    ck = _wide(act)
    x = gen_golden.make_input(12, {**CONFIGS, **SMALL}[_wide_config(act)][0])
    ob, om, ol = OracleNet(ck, act=act)(x)
    be = pkg().backend.HipTextDetBackend(ck, device="cuda", precision=engine, act=act)
    blks, mask, lines = be(x.cuda())
    torch.cuda.synchronize()
    np.testing.assert_allclose(mask.cpu().numpy(), om.numpy(), rtol=0, atol=2e-5)
    np.testing.assert_allclose(lines.cpu().numpy(), ol.numpy(), rtol=0, atol=2e-5)
    np.testing.assert_allclose(blks.cpu().numpy(), ob.numpy(), rtol=1e-4, atol=2e-3)


def _keyed(config):
    res = run_checks(KEYED[config][0], config)
    _assert_all_within(res, config)
    worst = max(res.items(), key=lambda kv: kv[1]["ratio"])
    print(f"\n{config} {KEYED[config][3]}: {sum(r['n'] > 0 for r in res.values())} ops checked, worst ratio "
          f"{worst[1]['ratio']:.3g} at op {worst[0]} {worst[1]['name']} ({worst[1]['kernel']})")
    return res


def _seen(res, kernel):
    """The ops of a run that launched `kernel` and had elements checked."""
    return [r for r in res.values() if r["kernel"] == kernel and r["n"] > 0]


@pytest.mark.parametrize("config", ["f32_direct_1x64x64", "f32_direct_3x128x64"])
def test_fp32_engine_on_the_direct_kernels_every_op_within_its_bound(config):
    """`f32_mfma` = 0, the exact-order mode of the fp32 engine and its fallback for whatever the MFMA kernel refuses:
    conv_direct_kernel<float, true> and convt_direct_kernel<float, true> on every conv of the network.  A sequential fmaf
    chain in f32 is the arithmetic of the fp32 row of the bound."""
    L = pkg()._lib
    res = _keyed(config)
    convs = [r for r in res.values() if r["kind"] == L.OP_CONV]
    convts = [r for r in res.values() if r["kind"] == L.OP_CONVT]
    assert len(convs) > 50 and len(convts) >= 7
    assert all(r["kernel"] == "conv_direct_kernel" and r["n"] > 0 for r in convs), [r for r in convs if r["kernel"] != "conv_direct_kernel"]
    assert all(r["kernel"] == "convt_direct_kernel" and r["n"] > 0 for r in convts)
    assert not [r["kernel"] for r in res.values() if "mfma" in r["kernel"]]


def test_fp16_engine_on_the_valu_tail_kernels_every_op_within_its_bound():
    """`db_up_mfma` = 0 and `seg_final_mfma` = 0: db_up_kernel on fp16 input and seg_final_kernel, the fallbacks for odd
    pitches, which the native selftest compares with their MFMA siblings only."""
    res = _keyed("valu_tails_u8_3x128x64")
    assert _seen(res, "db_up_kernel") and _seen(res, "seg_final_kernel")
    assert not [r["kernel"] for r in res.values() if r["kernel"] in ("db_up_mfma_kernel", "seg_final_mfma_kernel")]


def test_fp16_engine_unpaired_convtranspose_every_op_within_its_bound():
    """`halo_pair` = 0 (with the halo kernel forced onto these maps): the 64-output ConvTranspose layers go through the
    one-phase-per-block path of conv_halo_kernel.  Per op against float64, and the network outputs against the paired run of
    the same shape: at fuse = 0 the two differ in nothing but which block computes a phase."""
    L = pkg()._lib
    res = _keyed("halo_unpaired_3x128x64")
    paired = _keyed("halo_paired_3x128x64")
    for r in (res, paired):
        ct64 = [q for q in r.values() if q["kind"] == L.OP_CONVT and q["cout"] == 64]
        assert ct64 and all(q["kernel"] == "conv_halo_kernel" and q["n"] > 0 for q in ct64), ct64
    a, b = OUTS["halo_unpaired_3x128x64"], OUTS["halo_paired_3x128x64"]
    diff = {k: float(np.abs(a[k].astype(np.float64) - b[k].astype(np.float64)).max()) for k in a}
    print(f"\nhalo_pair 0 against 1, max |difference| per output: {diff}")
    if not all(np.array_equal(a[k], b[k]) for k in a):
        # same arithmetic, other K order: the bar of test_gpu_edge.test_halo_kernel_forced_onto_small_maps_matches_oracle
        assert diff["mask"] < 5e-3 and diff["lines"] < 5e-3 and float(np.abs(a["blks"][..., 4:] - b["blks"][..., 4:]).max()) < 5e-3, diff


def test_fp16_engine_with_the_halo_kernels_switched_off_every_op_within_its_bound():
    """`halo` = 0 and `halo3` = 0, each with the thresholds lifted so that the key alone decides: without `halo` no op runs
    conv_halo_kernel (the 3x3s and ConvTransposes are conv_igemm_kernel's), without `halo3` the ConvTranspose layers that
    conv_halo3_kernel takes under `halo3` = 1 stay with conv_halo_kernel."""
    L = pkg()._lib
    res = _keyed("halo_off_3x128x64")
    assert not _seen(res, "conv_halo_kernel") and not _seen(res, "conv_halo3_kernel")
    assert [r for r in _seen(res, "conv_igemm_kernel") if r["kind"] == L.OP_CONV and r["k"] == 3]
    assert [r for r in _seen(res, "conv_igemm_kernel") if r["kind"] == L.OP_CONVT]
    on, off = _keyed("halo3_on_3x128x64"), _keyed("halo3_off_3x128x64")
    took = [i for i, r in on.items() if r["kernel"] == "conv_halo3_kernel" and r["n"] > 0]
    assert took and all(off[i]["kernel"] == "conv_halo_kernel" and off[i]["n"] > 0 for i in took), [(on[i], off[i]) for i in took]
    assert not _seen(off, "conv_halo3_kernel")


def test_fp32s_engine_on_fp32_tensors_every_op_within_its_bound():
    """`split_planes` = `split_halo` = `split_stem` = 0: the split engine with fp32 tensors everywhere, operands split in the
    K loop of conv_split_kernel, the page read by input_kernel."""
    res = _keyed("fp32_tensors_3x128x64")
    assert not [r["kernel"] for r in res.values() if r["kernel"] in ("conv_split_halo_kernel", "stem_split_kernel")]
    assert _seen(res, "input_kernel") and len(_seen(res, "conv_split_kernel")) > 50


def test_fp32s_engine_without_split_planes_every_op_within_its_bound():
    """`split_planes` = 0 alone.  conv_split_halo_kernel reads split-plane sources only (conv_split_halo_supported: x_sp),
    so with fp32 tensors every conv is conv_split_kernel's, the first layer stays with stem_split_kernel: that pair, on fp32
    tensors, is what this key selects."""
    res = _keyed("planes_off_3x128x64")
    assert not _seen(res, "conv_split_halo_kernel")
    assert _seen(res, "stem_split_kernel") and len(_seen(res, "conv_split_kernel")) > 50


@pytest.mark.parametrize("engine", ["fp16", "fp32"])
def test_direct_kernels_on_a_hand_built_program_every_op_within_its_bound(engine):
    """The `half` direct kernels (the fp16 engine's universal fallback and the native selftest's yardstick, which no lowering
    of the network reaches) and the float ones on layer_ref.direct_program: channel counts no vector path can take, two
    sources with an upsample, stride 2, a residual into a channel offset, both ConvTranspose geometries, four activations."""
    res = run_direct(engine)
    assert len(res) == 7 and all(r["kernel"] == ("convt_direct_kernel" if r["kind"] == pkg()._lib.OP_CONVT else "conv_direct_kernel")
                                 and r["n"] > 0 for r in res.values()), res
    _assert_all_within(res, ("direct program", engine))
    print(f"\ndirect program, {engine}: " + ", ".join(f"{r['name']} {r['ratio']:.3g}" for r in res.values()))


def run_direct(engine):
    if ("direct", engine) in _S:
        return _S[("direct", engine)]
    p = pkg()
    L = p._lib
    prog, ops = direct_program(L.PREC_F16 if engine == "fp16" else L.PREC_F32)
    x, page = _input((2, 192, 320), False, 13)
    with L.tuning(fuse=0):
        with L.tuning(no_reuse=1):
            be = _engine({}, engine, prog, "leaky")
        be(x.cuda())
        torch.cuda.synchronize()
        kernels = [k for _, k in be.op_kernels()]
    res = LayerCheck(prog, {}, engine, be.read_tensor, {}, page, kernels=kernels, seed=5).check_all(ops)
    del be
    for i, r in res.items():
        r["kernel"], r["kind"], r["cout"] = kernels[i], prog.ops[i]["kind"], prog.ops[i]["cout"]
        TABLEK[(engine, kernels[i])] = max(TABLEK.get((engine, kernels[i]), 0.0), r["ratio"])
    _S[("direct", engine)] = res
    return res


# ---------------------------------------------------------------------------------------------------------------------
# the ledger of tuning keys
# ---------------------------------------------------------------------------------------------------------------------
# Every key of ctd_tuning_set (the rows of csrc/tuning.def) is in one of the two tables: tests/test_layer_ref.py reads the
# rows and fails on a key that is in neither.  DISPATCH_KEYS: (key, value, what the value selects, where it is proven).  The proof is
#   ("f64", engine, config, kernels)   run_checks(engine, config): each kernel launched by an op with n > 0 checked elements
#   ("direct", engine, kernels)        the same on the hand-built program
#   ("bits", act, shape, u8, masks, cfg, label, kernels)
#                                      test_gpu_edge.fused_runs: the run `label` equals the per-layer program bit for bit and
#                                      launched each kernel
_T = (3, 128, 64)
_ALL_FUSED = ("c3_fused_kernel", "c3b_kernel", "conv_halo3_kernel+taps", "seg_final_gather_kernel", "stem_conv2_kernel",
              "sppf_pool3_kernel")
DISPATCH_KEYS = (
    ("fuse", 0, "one launch per op: the program every float64 check runs", ("f64", "fp16", "forced_1x64x64", ("conv_igemm_kernel",))),
    ("fuse", 63, "the multi-layer kernels (each bit alone: test_gpu_edge.py)", ("bits", "relu", _T, True, (8, 16, 32, 63), (0, 1), "63 + halo3", _ALL_FUSED)),
    ("fuse", 63, "bit 16 needs maps that are multiples of 128", ("bits", "relu", (2, 128, 128), True, (8, 16, 32, 63), (0, 1), "63 + halo3", ("conv_halo3_kernel+1x1",))),
    ("f32_mfma", 0, "fp32 engine: the float direct kernels", ("f64", "fp32", "f32_direct_3x128x64", ("conv_direct_kernel", "convt_direct_kernel"))),
    ("f32_mfma", 1, "fp32 engine: conv_f32_mfma_kernel", ("f64", "fp32", "forced_1x64x64", ("conv_f32_mfma_kernel",))),
    ("f32_mfma", 1, "what the MFMA kernels refuse: direct kernels, float and half", ("direct", "fp32", ("conv_direct_kernel", "convt_direct_kernel"))),
    ("f32_mfma", 1, "", ("direct", "fp16", ("conv_direct_kernel", "convt_direct_kernel"))),
    ("db_up_mfma", 0, "fp16 engine: db_up_kernel on fp16 input", ("f64", "fp16", "valu_tails_u8_3x128x64", ("db_up_kernel",))),
    ("db_up_mfma", 1, "db_up_mfma_kernel", ("f64", "fp16", "forced_1x64x64", ("db_up_mfma_kernel",))),
    ("seg_final_mfma", 0, "fp16 engine: seg_final_kernel", ("f64", "fp16", "valu_tails_u8_3x128x64", ("seg_final_kernel",))),
    ("seg_final_mfma", 1, "seg_final_mfma_kernel", ("f64", "fp16", "forced_1x64x64", ("seg_final_mfma_kernel",))),
    ("halo", 0, "every 3x3 and ConvTranspose on conv_igemm_kernel, whatever the threshold", ("f64", "fp16", "halo_off_3x128x64", ("conv_igemm_kernel",))),
    ("halo", 1, "conv_halo_kernel", ("f64", "fp16", "halo_paired_3x128x64", ("conv_halo_kernel",))),
    ("halo_pair", 0, "64-channel ConvTranspose: one phase per block of conv_halo_kernel", ("f64", "fp16", "halo_unpaired_3x128x64", ("conv_halo_kernel",))),
    ("halo_pair", 1, "both px phases per block", ("f64", "fp16", "halo_paired_3x128x64", ("conv_halo_kernel",))),
    ("halo3", 0, "the ConvTranspose layers stay with conv_halo_kernel (bit for bit against halo3 = 1: test_gpu_edge.py)", ("f64", "fp16", "halo3_off_3x128x64", ("conv_halo_kernel",))),
    ("halo3", 1, "conv_halo3_kernel", ("f64", "fp16", "halo3_on_3x128x64", ("conv_halo3_kernel",))),
    ("split_planes", 0, "fp32s engine: fp32 tensors, conv_split_kernel splits in its K loop", ("f64", "fp32s", "planes_off_3x128x64", ("conv_split_kernel", "stem_split_kernel"))),
    ("split_planes", 1, "split-plane tensors", ("f64", "fp32s", "forced_1x64x64", ("conv_split_kernel",))),
    ("split_halo", 0, "no conv_split_halo_kernel", ("f64", "fp32s", "fp32_tensors_3x128x64", ("conv_split_kernel",))),
    ("split_halo", 1, "conv_split_halo_kernel (above split_halo_min_patches)", ("f64", "fp32s", "u8_2x1024x1024", ("conv_split_halo_kernel",))),
    ("split_stem", 0, "fp32s engine: input_kernel + conv_split_kernel for the first layer", ("f64", "fp32s", "fp32_tensors_3x128x64", ("input_kernel",))),
    ("split_stem", 1, "stem_split_kernel", ("f64", "fp32s", "forced_1x64x64", ("stem_split_kernel",))),
) + tuple(
    (key, cfg[i], f"c3b_kernel tiling: {names[w]}", ("bits", "relu", _T, True, (8, 63), cfg, "8 + halo", (names[w],)))
    for cfg, names in (((0, 0), {64: "c3b_kernel", 128: "c3b_kernel<128,8,1>"}), ((1, 1), {64: "c3b_kernel<64,16,2>", 128: "c3b_kernel"}),
                       ((2, 1), {64: "c3b_kernel<64,8,2>", 128: "c3b_kernel"}))
    for i, key, w in ((0, "c3b_cfg64", 64), (1, "c3b_cfg128", 128)))
NOT_DISPATCH_KEYS = {
    "halo_min_patches": "threshold; forced to 1 by the forced_* configs here and in test_gpu_edge.py",
    "halo3_min_blocks": "threshold; forced to 1 by the forced_* configs here and in test_gpu_edge.py",
    "c3_min_patches": "threshold; forced to 1 in test_gpu_edge.py",
    "c3b_min_patches": "threshold; forced to 1 in test_gpu_edge.py",
    "c3b_max_ch": "width threshold of c3b_kernel; forced to 64 in test_gpu_edge.py",
    "split_halo_min_patches": "threshold; the default is crossed by u8_2x1024x1024, forced to 1 in the native selftest",
    "fwd_prio": "wave priority of the network's kernels: same kernels, same arithmetic",
    "no_reuse": "arena layout only: every activation stays readable (what the float64 checks run under)",
    "tail_max_blocks": "tail: grid cap",
    "tail_chain": "tests/test_gpu_e2e.py::test_detect_stream_equals_detect_batch_under_every_tail_chain (0, 1, 2; with and without tail_lds)",
    "tail_lds": "tail: LDS variant of the window kernels (tests/test_gpu_sweeps.py)", "tail_lds_rcap": "tail: LDS run capacity",
    "tail_lds_max_bytes": "tail: LDS threshold",
    "tail_lds_runs_x10": "tests/test_gpu_tail_trace.py::test_run_capacity (1, 25, 160, 1000: logged rcap, routing, overflows)",
    "tail_lds_threads": "tests/test_gpu_tail_trace.py::test_block_size_case_at_every_block_size (256, 512, 1024; the clamp in "
                        "::test_block_size_key_is_clamped_to_256_512_1024)",
    "tail_lds_cls0": "tests/test_gpu_tail_trace.py::test_launch_classes (the launch log under every setting of class_settings)",
    "tail_lds_cls1": "tests/test_gpu_tail_trace.py::test_launch_classes (the launch log under every setting of class_settings)",
    "tail_dma_min": "tail: copy-engine threshold",
    "tail_skip_page_download": "tail: measurement knob, not in the shipped library", "tail_ablate": "tail: measurement knob, not in the shipped library",
    "tail_priority": "tests/test_gpu_e2e.py::test_tail_created_under_every_stream_priority_refines_exactly (0, 1, 2)",
    # untested on purpose: CU-masked streams are an experiment of `bench.py --cu-split`; this suite creates none (the GPUs it runs
    # on are shared)
    "tail_cus": "tail: CU mask experiment, not exercised (no CU-masked streams in the suite)",
    "tail_cu_first": "tail: CU mask experiment, not exercised (no CU-masked streams in the suite)",
}


def test_every_dispatch_key_value_ran_the_kernel_it_selects_and_was_checked():
    """The ledger: for each row of DISPATCH_KEYS the kernels that prove the value took effect were launched by ops whose
    elements were checked against float64 within the bound, or by a run that equals the per-layer program bit for bit."""
    import test_gpu_edge as E
    for key, value, _, proof in DISPATCH_KEYS:
        if proof[0] == "f64":
            _, engine, config, kernels = proof
            res = run_checks(engine, config)
            # the row's value is what that configuration ran under: the key as set there, the library's default otherwise
            held = KEYED[config][3] if config in KEYED else {"fuse": 0}
            assert held.get(key, pkg()._lib.tuning_get(key)) == value, (key, value, config)
        elif proof[0] == "direct":
            _, engine, kernels = proof
            res = run_direct(engine)
        else:
            _, act, shape, u8, masks, cfg, label, kernels = proof
            diff, kern = E.fused_runs(act, shape, u8, masks, cfg, halo_walks=masks == (8, 63))[label]
            assert not diff, (key, value, diff)
            assert set(kernels) <= {k for _, _, k in kern}, (key, value, set(kernels) - {k for _, _, k in kern})
            continue
        _assert_all_within(res, (key, value))
        missing = [k for k in kernels if not _seen(res, k)]
        assert not missing, (key, value, missing)
    assert not {k for k, *_ in DISPATCH_KEYS} & set(NOT_DISPATCH_KEYS)
    _print_table()


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
    _print_table()
    for engine, st in sorted(STATS.items()):
        print(f"  {engine} B = 32 no_reuse: {st}")
