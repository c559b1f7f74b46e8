"""-m gpu: edge cases of the hot path -- empty / saturated maps, smallest and largest page
sizes, non-square inputs, batch remainders (reference behaviour: empty results are legal,
inference.py:166-167; H, W multiples of 64)."""
import numpy as np
import pytest
import torch

from conftest import checkpoint, pkg
from oracle import gen_golden
from oracle import postproc_ref as R
from oracle.net_ref import OracleNet
from test_post_host import blocks_equal

pytestmark = pytest.mark.gpu


def _det(size):
    from test_gpu_e2e import detector
    return detector(size)


def test_no_detections_gives_empty_results():
    size = 256
    det = _det(size)
    page = np.full((size, size, 3), 255, np.uint8)
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device="cuda")       # noqa: E731
    m, refined, blks = det.tail_batch([page], z(1, 1008, 7), z(1, size, size, dt=torch.uint8), z(1, size, size),
                                      z(1, size, size, dt=torch.uint8), keep_undetected_mask=True)[0]
    assert blks == [] and refined.sum() == 0 and m.sum() == 0
    ref = R.detector_tail(page, np.zeros((1, 1008, 7), np.float32), np.zeros((1, 1, size, size), np.float32),
                          np.zeros((1, 2, size, size), np.float32), input_size=(size, size), keep_undetected_mask=True)
    assert ref[2] == [] and ref[1].sum() == 0


def test_saturated_maps_single_component():
    """Everything is text: one component touching all borders, no holes; one block covering the page."""
    size = 256
    det = _det(size)
    page = np.random.RandomState(0).randint(0, 256, (size, size, 3)).astype(np.uint8)
    blks = np.zeros((1, 1008, 7), np.float32)
    blks[0, 0] = [size / 2, size / 2, size - 20, size - 20, 0.95, 0.1, 0.9]
    mask_u8 = np.full((size, size), 230, np.uint8)
    prob = np.full((size, size), 0.9, np.float32)
    got = det.tail_batch([page], torch.from_numpy(blks).cuda(), torch.from_numpy(mask_u8)[None].cuda(),
                         torch.from_numpy(prob)[None].cuda(), torch.ones(1, size, size, dtype=torch.uint8, device="cuda"),
                         keep_undetected_mask=True)[0]
    ref = R.detector_tail(page, blks, ((mask_u8.astype(np.float32) + 0.5) / 255)[None, None],
                          np.stack([prob, np.zeros_like(prob)])[None], input_size=(size, size), keep_undetected_mask=True)
    np.testing.assert_array_equal(got[0], ref[0])
    blocks_equal(got[2], ref[2])
    np.testing.assert_array_equal(got[1], ref[1])


@pytest.mark.parametrize("shape", [(1, 64, 64), (1, 640, 1024), (3, 128, 64), (1, 1536, 1536)])
def test_network_sizes_against_oracle(shape):
    """Smallest legal input, non-square, odd batch, and the largest bucket of BASELINE config 5."""
    ck = checkpoint(0)
    x = gen_golden.make_input(31, shape)
    ob, om, ol = OracleNet(ck)(x)
    p = pkg()
    for prec, tol in (("fp32", 3e-5), ("fp32s", 3e-5), ("fp16", 3e-2)):   # all three engines, the fp32-level ones at the same bar
        be = p.backend.HipTextDetBackend(ck, device="cuda", precision=prec)
        blks, mask, lines = be(x.cuda())
        torch.cuda.synchronize()
        assert blks.shape == ob.shape
        assert float((mask.cpu() - om).abs().max()) < tol
        assert float((lines.cpu() - ol).abs().max()) < tol
        assert float((blks.cpu()[..., 4:] - ob[..., 4:]).abs().max()) < tol
        del be


@pytest.mark.parametrize("shape", [(1, 64, 64), (3, 128, 64), (2, 320, 448)])
def test_halo_kernel_forced_onto_small_maps_matches_oracle(shape):
    """The halo-tile conv kernel normally takes only maps with >= 1024 patches; forced onto tiny
    ones (`ctd_tuning_set("halo_min_patches", 1)`) every 16x16 patch is partial: 2x2 ... 14x10 pixel maps, patches
    hanging over the right / bottom edge, ConvTranspose phases on 2x2 inputs."""
    ck = checkpoint(0)
    x = gen_golden.make_input(33, shape)
    ob, om, ol = OracleNet(ck)(x)
    p = pkg()
    be = p.backend.HipTextDetBackend(ck, device="cuda", precision="fp16")
    ref = [t.clone() for t in be(x.cuda())]
    with p._lib.tuning(halo_min_patches=1):
        got = [t.clone() for t in be(x.cuda())]
        torch.cuda.synchronize()
    assert not all(torch.equal(g, r) for g, r in zip(got, ref)), "the forced dispatch did not change any kernel"
    # the fp16 golden tolerances of tests/test_gpu_net.py (2e-2 max, 2e-3 mean), not a looser bar for the forced dispatch
    for g, o in ((got[1].cpu(), om), (got[2].cpu(), ol)):
        d = (g - o).abs()
        assert float(d.max()) < 2e-2 and float(d.mean()) < 2e-3, (float(d.max()), float(d.mean()))
    assert float((got[0].cpu()[..., 4:] - ob[..., 4:]).abs().max()) < 2e-2
    # same arithmetic up to the summation order of the K walk
    assert float((got[1] - ref[1]).abs().max()) < 5e-3 and float((got[2] - ref[2]).abs().max()) < 5e-3


def test_replanning_between_sizes_keeps_results():
    """A mixed-size stream re-plans the arena; going back to an earlier size reproduces its result."""
    be = pkg().backend.HipTextDetBackend(checkpoint(0), device="cuda", precision="fp16")
    xa = gen_golden.make_input(41, (2, 256, 256)).cuda()
    xb = gen_golden.make_input(42, (1, 512, 384)).cuda()
    a1 = [t.clone() for t in be(xa)]
    b1 = [t.clone() for t in be(xb)]
    a2 = be(xa)
    torch.cuda.synchronize()
    for u, v in zip(a1, a2):
        assert torch.equal(u, v)
    assert b1[1].shape == (1, 1, 512, 384)


def test_large_batch_is_split_transparently():
    """B above the 2 GiB-per-tensor limit of the MFMA kernel's 32-bit offsets runs as sub-batches."""
    be = pkg().backend.HipTextDetBackend(checkpoint(0), device="cuda", precision="fp16")
    H = W = 256
    max_b = (2 ** 31 - 1) // (H * W * 40)
    B = max_b + 3
    pages = torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(1)).cuda()
    blks, mask, lines = be.forward_u8(pages)
    assert mask.shape[0] == B and be.mask_u8.shape[0] == B
    one = be.forward_u8(pages[B - 1: B].contiguous())
    torch.cuda.synchronize()
    assert torch.equal(one[1][0], mask[B - 1])


@pytest.mark.parametrize("shape,u8", [((1, 64, 64), False), ((3, 128, 64), True), ((2, 320, 448), False),
                                      ((2, 1024, 1024), True), ((1, 1536, 1536), True), ((32, 1024, 1024), True)])
def test_fused_blocks_equal_the_layer_per_launch_program_bit_for_bit(shape, u8):
    """The multi-layer kernels of the fp16 engine (stem + layer 1, the 32-channel C3 block, SPPF's three pools, bit 8:
    bottleneck + cv3 of the 64 / 128-channel C3 blocks of backbone, neck and heads -- kernels_c3b.hip; bit 16: a 128-channel
    ConvTranspose and the 1x1 conv that is its only consumer, bit 32: the last 64-channel ConvTranspose and the tap
    products of the 64 -> 1 one behind it -- kernels_halo3.hip;
    `ctd_tuning_set("fuse", mask)`) do the arithmetic of the launches they replace in the same order: every output
    of the network must be IDENTICAL with and without them -- interior and border patches, float and uint8 input,
    maps smaller than one patch (the C3 kernels are forced onto them with c3_min_patches = c3b_min_patches = 1), and
    for bit 8 both K walks of the 3x3 it absorbs (the halo kernel's, forced onto every map by halo_min_patches = 1,
    and the implicit GEMM's).  32 x 1024 x 1024 is the shape bench.py times: the grids, page counts and tensor sizes of the
    published number.  (This test is what found that the compiler rounded SiLU outputs once or twice depending
    on the kernel: ctd_common.h ctd_act_fast.)"""
    be = pkg().backend.HipTextDetBackend(checkpoint(0), device="cuda", precision="fp16")
    if u8:
        x = torch.randint(0, 256, (shape[0], shape[1], shape[2], 3), dtype=torch.uint8,
                          generator=torch.Generator().manual_seed(5)).cuda()
        run = lambda: [t.clone() for t in be.forward_u8(x)] + [be.mask_u8.clone(), be.bitmap.clone()]   # noqa: E731
    else:
        x = gen_golden.make_input(77, shape).cuda()
        run = lambda: [t.clone() for t in be(x)] + [be.mask_u8.clone(), be.bitmap.clone()]              # noqa: E731
    tuning = pkg()._lib.tuning          # each block puts back what it found: `fuse` is 0 again after every mask
    outs = {}
    with tuning(fuse=0):
        ref = run()
        with tuning(c3_min_patches=1, c3b_min_patches=1):
            for mask in (1, 2, 4, 6, 7, 8, 15, 16, 31, 32, 63):
                with tuning(fuse=mask):
                    outs[mask] = run()
            with tuning(halo_min_patches=1):            # the 3x3s (and ConvT phases) on the halo kernel everywhere
                ref_h = run()
                with tuning(fuse=8):
                    outs["8 + halo"] = run()
                    with tuning(c3b_max_ch=64):
                        outs["8 + halo, 64 only"] = run()
                # bit 16 (a 128-channel ConvTranspose + its single 1x1 consumer in one launch of the big-tile kernel) needs
                # that kernel: lift its grid threshold so that also the small shapes go through it (maps that are multiples
                # of 16)
                with tuning(halo3_min_blocks=1):
                    ref_3 = run()
                    for mask in (16, 31, 32, 63):
                        with tuning(fuse=mask):
                            outs[f"{mask} + halo3"] = run()
                    torch.cuda.synchronize()
    for mask, got in outs.items():
        base = ref if not isinstance(mask, str) else (ref_3 if "halo3" in mask else ref_h)
        for i, (g, r) in enumerate(zip(got, base)):
            assert torch.equal(g, r), f"fuse mask {mask}: output {i} differs from the unfused program " \
                                      f"(max |d| {float((g.float() - r.float()).abs().max()):.3g})"


NAMES = ("blks", "mask", "lines", "mask_u8", "bitmap")
# (c3b_cfg64, c3b_cfg128) -> the names launch_c3b reports for the 64-wide and the 128-wide blocks: "c3b_kernel" for the
# default tiling of each width, the tiling spelled out for the others
C3B_TILINGS = {
    (0, 1): {64: "c3b_kernel", 128: "c3b_kernel"},
    (0, 0): {64: "c3b_kernel", 128: "c3b_kernel<128,8,1>"},
    (1, 1): {64: "c3b_kernel<64,16,2>", 128: "c3b_kernel"},
    (2, 1): {64: "c3b_kernel<64,8,2>", 128: "c3b_kernel"},
    (1, 0): {64: "c3b_kernel<64,16,2>", 128: "c3b_kernel<128,8,1>"},
    (2, 0): {64: "c3b_kernel<64,8,2>", 128: "c3b_kernel<128,8,1>"},
}
_BE = {}
_RUNS = {}


def _act_backend(act):
    """One fp16 engine per head activation, on a checkpoint made for it (the heads' activations see both signs)."""
    if act not in _BE:
        p = pkg()
        ck = checkpoint(0) if act == "leaky" else p.synth.make_checkpoint(0, act=act)
        _BE[act] = p.backend.HipTextDetBackend(ck, device="cuda", precision="fp16", act=act)
    return _BE[act]


def _runner(be, shape, u8):
    if u8:
        x = torch.randint(0, 256, (shape[0], shape[1], shape[2], 3), dtype=torch.uint8,
                          generator=torch.Generator().manual_seed(5)).cuda()
        fwd = lambda: be.forward_u8(x)              # noqa: E731
    else:
        x = gen_golden.make_input(77, shape).cuda()
        fwd = lambda: be(x)                         # noqa: E731

    def run():
        return [t.clone() for t in fwd()] + [be.mask_u8.clone(), be.bitmap.clone()]
    return run


def _differences(got, ref):
    return [f"{n}: {int((g != r).sum())} elements differ, max |d| {float((g.float() - r.float()).abs().max()):.3g}"
            for n, g, r in zip(NAMES, got, ref) if not torch.equal(g, r)]


def fused_runs(act, shape, u8, masks, cfg=(0, 1), halo_walks=False):
    """Cached.  The fp16 engine with head activation `act` at `shape`, c3_min_patches = c3b_min_patches = 1 and the c3b
    tilings `cfg`: every fuse mask of `masks` against fuse = 0 -- at the default thresholds (with `halo_walks`: also with
    halo_min_patches = 1, the other K walk of the 3x3 that c3b_kernel absorbs), and with halo3_min_blocks = 1 on top.
    -> {label: (differences from the per-layer program, [(op name, cout, kernel)] of the run)}"""
    key = (act, shape, u8, tuple(masks), cfg, halo_walks)
    if key in _RUNS:
        return _RUNS[key]
    be = _act_backend(act)
    run = _runner(be, shape, u8)
    out = {}

    tuning = pkg()._lib.tuning

    def compare(label):
        with tuning(fuse=0):
            ref = run()
        for mask in masks:
            with tuning(fuse=mask):
                got = run()
                torch.cuda.synchronize()
                kern = [(n, be.program.ops[i]["cout"], k) for i, (n, k) in enumerate(be.op_kernels())]
            out[f"{mask}{label}"] = (_differences(got, ref), kern)
    with tuning(c3_min_patches=1, c3b_min_patches=1, c3b_cfg64=cfg[0], c3b_cfg128=cfg[1]):
        compare("")
        with tuning({"halo_min_patches": 1} if halo_walks else {}):
            if halo_walks:
                compare(" + halo")
            with tuning(halo3_min_blocks=1):
                compare(" + halo3")
    _RUNS[key] = out
    return out


def _c3b_names(kern):
    """{block width: the names the c3b launches of that width reported}"""
    by = {}
    for _, cout, k in kern:
        if k.startswith("c3b_kernel"):
            by.setdefault(cout, set()).add(k)
    return by


C3B_SHAPES = [pytest.param((3, 128, 64), True, id="u8_3x128x64"), pytest.param((2, 320, 448), False, id="2x320x448")]


@pytest.mark.parametrize("act", ["leaky", "relu"])
@pytest.mark.parametrize("shape,u8", C3B_SHAPES)
@pytest.mark.parametrize("cfg", [(0, 0), (1, 1), (2, 1), (1, 0), (2, 0)], ids=lambda c: f"cfg64_{c[0]}-cfg128_{c[1]}")
def test_c3b_tilings_equal_the_layer_per_launch_program_bit_for_bit(cfg, shape, u8, act):
    """The tilings of c3b_kernel that `c3b_cfg64` / `c3b_cfg128` select besides the default pair (0, 1): <64,16,2>, <64,8,2> and
    <128,8,1>, with and without cv3, for the head activations leaky and relu.  (3, 128, 64) makes every patch partial (a
    16 x 8 map at stride 8); (2, 320, 448) has 40 x 56 and 20 x 28 maps: two full 16-row patches plus a half, full plus half
    16-column patches -- interior, ragged right edge and ragged bottom edge at once for BH = 16.  fuse = 8 against fuse = 0 for
    both K walks of the absorbed 3x3, and fuse = 63 against fuse = 0 with halo3_min_blocks = 1; by op_kernels() the blocks of
    each width ran the tiling that was asked for."""
    runs = fused_runs(act, shape, u8, (8, 63), cfg, halo_walks=True)
    for label in ("8", "8 + halo", "63 + halo3"):
        diff, kern = runs[label]
        assert not diff, (cfg, act, label, diff)
        assert _c3b_names(kern) == {w: {n} for w, n in C3B_TILINGS[cfg].items()}, (label, _c3b_names(kern))


@pytest.mark.parametrize("act", ["silu", "relu"])
@pytest.mark.parametrize("shape,u8", C3B_SHAPES + [pytest.param((2, 128, 128), True, id="u8_2x128x128")])
def test_fused_blocks_equal_the_per_layer_program_for_silu_and_relu_heads(shape, u8, act):
    """test_fused_blocks_equal_the_layer_per_launch_program_bit_for_bit for the other two head activations, each on a
    checkpoint made for it: c3b_kernel in seg.* / db.*, conv_halo3_kernel+1x1 (epilogue2 with CTD_ACT_SILU / CTD_ACT_RELU as
    post_act) and conv_halo3_kernel+taps.  The big-tile kernel takes maps that are multiples of 16 only, and the 128-channel
    ConvTranspose of the +1x1 form reads the maps at stride 8: it can run only where H and W are multiples of 128, which
    neither (3, 128, 64) nor (2, 320, 448) is -- (2, 128, 128) is the smallest shape that has it."""
    runs = fused_runs(act, shape, u8, (8, 16, 32, 63))
    for label, (diff, _) in runs.items():
        assert not diff, (act, label, diff)
    names = {k for _, _, k in runs["63 + halo3"][1]}
    want = {"c3b_kernel", "conv_halo3_kernel+taps"} | ({"conv_halo3_kernel+1x1"} if shape[1] % 128 == 0 and shape[2] % 128 == 0 else set())
    assert want <= names, (want - names, sorted(names))
    # ... and c3b_kernel ran inside both heads (their inner layers carry no head prefix: by position in the program)
    kern = runs["63 + halo3"][1]
    seg0 = next(i for i, (n, _, _) in enumerate(kern) if n == "seg.down_conv1.down")
    seg1 = next(i for i, (n, _, _) in enumerate(kern) if n == "seg.upconv6")
    c3b = [i for i, (_, _, k) in enumerate(kern) if k == "c3b_kernel"]
    assert any(seg0 < i < seg1 for i in c3b) and any(i > seg1 for i in c3b), [kern[i] for i in c3b]


@pytest.mark.parametrize("prec", ["fp16", "fp32s", "fp32"])
def test_timed_dispatch_fused_equals_unfused_on_all_32_pages(prec):
    """bench.py's batch (its checkpoint, its first 32 pages of 1024 x 1024, uint8) at the DEFAULT thresholds -- no tuning key
    but `fuse` is touched: the program with every multi-layer kernel (fuse = 63, what is timed) against the one launch per
    layer program (fuse = 0, what tests/test_gpu_layers.py checks op by op at this shape).  Every output equal on every page.
    The fp16 engine is the one that is timed and has all seven multi-layer kernels; on the fp32 / fp32s engines the only
    fusion is SPPF's three max pools (exact in any precision)."""
    from test_gpu_dispatch import workload
    ck, pages = workload()
    x = torch.from_numpy(np.stack(pages)).cuda()
    assert tuple(x.shape) == (32, 1024, 1024, 3)
    be = pkg().backend.HipTextDetBackend(ck, device="cuda", precision=prec)
    names = ("blks", "mask", "lines", "mask_u8", "bitmap")
    run = lambda: [t.clone() for t in be.forward_u8(x)] + [be.mask_u8.clone(), be.bitmap.clone()]       # noqa: E731
    got = run()
    kernels = be.op_kernels()
    with pkg()._lib.tuning(fuse=0):
        ref = run()
        plain = be.op_kernels()
        torch.cuda.synchronize()
    fused = {k for _, k in kernels} - {k for _, k in plain}
    want = {"c3_fused_kernel", "c3b_kernel", "conv_halo3_kernel+1x1", "conv_halo3_kernel+taps", "seg_final_gather_kernel",
            "stem_conv2_kernel", "sppf_pool3_kernel"} if prec == "fp16" else {"sppf_pool3_kernel"}
    assert want <= fused, fused
    for name, g, r in zip(names, got, ref):
        assert g.shape == r.shape and g.shape[0] == 32
        if not torch.equal(g, r):
            page = int((g != r).reshape(32, -1).any(1).nonzero()[0])
            at = [int(v) for v in (g[page] != r[page]).nonzero()[0]]
            raise AssertionError(f"{name}: first difference on page {page} at {at}: fused {g[page][tuple(at)].item()!r}, "
                                 f"per layer {r[page][tuple(at)].item()!r}; {int((g != r).sum())} elements differ on pages "
                                 f"{(g != r).reshape(32, -1).any(1).nonzero().flatten().tolist()}")


@pytest.mark.parametrize("shape", [(2, 512, 512), (1, 1024, 768), (3, 256, 512), (32, 1024, 1024)])
def test_big_tile_convt_kernels_reproduce_the_256x128_kernel_bit_for_bit(shape):
    """The ConvTranspose layers on kernels_halo3.hip (256 x 128 tiles, four waves, two blocks per CU) walk K and issue
    their MFMAs per accumulator in the order of kernels_halo.hip:
    with the grid threshold lifted (`halo3_min_blocks` = 1: also maps whose ConvT inputs are 16x16 ... 64x48, i.e. every
    tile at an image border) every output of the network equals the output without it, bit for bit."""
    ck = checkpoint(0)
    x = gen_golden.make_input(51, shape).cuda()
    be = pkg().backend.HipTextDetBackend(ck, device="cuda", precision="fp16")
    # both sides run the ConvT layers on their own (fuse bits 16 and 32 off): a tuning key re-plans the engine, and with
    # halo3 on the plan would fold their consumers into them
    tuning = pkg()._lib.tuning
    with tuning(fuse=15, halo_min_patches=1):
        with tuning(halo3=0):                           # the reference side: the 256 x 128 halo kernel on every ConvT layer
            ref = [t.clone() for t in be(x)]
            ref_side = (be.mask_u8.clone(), be.bitmap.clone())
        with tuning(halo3=1, halo3_min_blocks=1):
            got = [t.clone() for t in be(x)]
            got_side = (be.mask_u8.clone(), be.bitmap.clone())
            torch.cuda.synchronize()
    for g, r in zip(got + list(got_side), ref + list(ref_side)):
        assert torch.equal(g, r)
