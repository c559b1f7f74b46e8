"""-m gpu: every op of every engine against a float64 recomputation of that op from the engine's own stored inputs, with
the error bound derived from the engine's arithmetic (tests/layer_ref.py) -- a per-layer check where the rest of the
suite compares only the end of the forward with a reference, or one HIP kernel with another.

Engines run with `no_reuse` = 1 (every activation stays readable) and `fuse` = 0 (one launch per op: the multi-layer
kernels are tied to the per-layer program bit for bit by tests/test_gpu_edge.py); in-place C3 slices are read through
identity-copy snapshots (layer_ref.snapshot_program).  The coverage test asserts that every kernel the timed B = 32
dispatch launches is among the kernels checked here, or is a multi-layer kernel listed with the test that ties it to
the per-layer program.
"""
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
}
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
TABLE = {}          # (engine, kernel) -> worst ratio


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
    ck = checkpoint(0) if ck_key == "synth0" else _wide(act)
    shape, u8, forced = CONFIGS[config]
    prec = {"fp32": L.PREC_F32, "fp32s": L.PREC_F32S, "fp16": L.PREC_F16}[engine]
    prog = p.graph.lower(ck, prec, act=act)
    snap, index, snaps = snapshot_program(prog)
    x, page = _input(shape, u8, 11)
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
    finally:
        for k, v in _DEFAULTS:
            _tune(k, v)
    kernels = [snap_kernels[index[i]][1] for i in range(len(prog.ops))]
    # the premise: neither no_reuse nor the snapshot copies change what the program's own ops launch
    assert kernels == [k for _, k in plain_kernels], [(a, b) for a, b in zip(kernels, plain_kernels) if a != b[1]]
    chk = LayerCheck(prog, snaps, engine, be.read_tensor, outs, page, u8=u8, kernels=kernels, seed=len(_S))
    res = chk.check_all()
    del chk, be
    for i, r in res.items():
        r["kernel"] = kernels[i]
        if r["n"]:
            t = (engine, kernels[i])
            TABLE[t] = max(TABLE.get(t, 0.0), r["ratio"])
    _S[key] = res
    return res


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
    print(f"\n{engine} {config}: {sum(r['n'] > 0 for r in res.values())} ops checked, worst ratio "
          f"{worst[1]['ratio']:.3g} at {worst[1]['name']} ({worst[1]['kernel']})")


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
    print("\nworst |engine - f64| / bound per (engine, kernel):")
    for (engine, kern), v in sorted(TABLE.items()):
        print(f"  {engine:6s} {kern:28s} {v:.3g}")
