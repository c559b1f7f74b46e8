"""CPU tests of the float64 per-op checker (tests/layer_ref.py): the program interpreter (oracle/program_interp.py) stands
in for an engine.  Correct arithmetic -- the fp32 interpreter, an fp16 emulation, an fp32s (hi + lo operand)
emulation -- must pass its engine's bound on every op; each plausible kernel bug below must be caught at the op it hits."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import checkpoint, pkg
from layer_ref import LayerCheck, snapshot_program
from oracle.program_interp import run_program

SHAPE = (2, 128, 128)


def _L():
    return pkg()._lib


def _prog(engine, ck=None):
    L = _L()
    return pkg().graph.lower(ck if ck is not None else checkpoint(0), L.PREC_F16 if engine == "fp16" else L.PREC_F32)


def _x(shape=SHAPE, seed=3):
    B, H, W = shape
    return torch.rand(B, 3, H, W, generator=torch.Generator().manual_seed(seed))


def _f16(t):
    return t.half().float()


def _split(t):
    hi = t.half().float()
    return hi + (t - hi).half().float()


def fp16_emulation(prog):
    """fp16-rounded blob, every stored activation rounded to fp16 (f32 tensors -- the Detect convs -- excepted)."""
    blob = prog.blob().astype(np.float16).astype(np.float32)

    def hook(i, o, stage, y, ctx):
        if stage == "out" and prog.tensors[o["dst"]][2] != 1:
            return _f16(y)
        return y
    return blob, hook


def fp32s_blob(prog):
    """The split engine's weights: per output channel scaled by a power of two to put the largest weight in [512, 1024),
    split into fp16 hi + lo, scaled back (exact)."""
    L = _L()
    blob = prog.blob().copy()
    for o in prog.ops:
        if o["kind"] not in (L.OP_CONV, L.OP_CONVT, L.OP_STEM) or o["w_off"] < 0:
            continue
        cin = 3 if o["kind"] == L.OP_STEM else o["src0_c"] + (o["src1_c"] if o["src1"] >= 0 else 0)
        n = o["cout"] * cin * o["k"] ** 2
        w = blob[o["w_off"]: o["w_off"] + n].reshape((cin, o["cout"], -1) if o["kind"] == L.OP_CONVT else (o["cout"], cin, -1))
        wn = np.moveaxis(w, 1, 0) if o["kind"] == L.OP_CONVT else w
        m = np.abs(wn).reshape(o["cout"], -1).max(1)
        e = np.where(m > 0, 9 - np.floor(np.log2(np.where(m > 0, m, 1))), 0).astype(np.float32)
        sc = np.ldexp(np.float32(1), e.astype(int)).astype(np.float32).reshape(-1, 1, 1)
        ws = (wn * sc).astype(np.float32)
        hi = ws.astype(np.float16).astype(np.float32)
        lo = (ws - hi).astype(np.float16).astype(np.float32)
        wn[...] = (hi + lo) / sc
    return blob


def fp32s_emulation(prog, drop_lo_at=None):
    """Split weights; every stored activation as hi + lo (the image stays f32: the first layer splits it in its K loop)."""
    L = _L()

    def hook(i, o, stage, y, ctx):
        if stage == "out" and o["kind"] != L.OP_INPUT:
            return _f16(y) if i == drop_lo_at else _split(y)
        return y
    return fp32s_blob(prog), hook


def run_and_check(engine, prog=None, x=None, blob=None, hook=None, ops=None, checker_engine=None):
    prog = prog if prog is not None else _prog(engine)
    x = x if x is not None else _x()
    snap, index, snaps = snapshot_program(prog)
    shook = None
    if hook is not None:
        inv = {v: k for k, v in index.items()}

        def shook(i, o, stage, y, ctx):                 # the hook sees ORIGINAL op indices; the copies stay exact
            return hook(inv[i], o, stage, y, ctx) if i in inv else y
    if blob is not None:
        blob = np.concatenate([blob, snap.blob()[blob.size:]])
    out = run_program(snap, x, blob=blob, hook=shook, return_tensors=True)
    T = out["tensors"]
    outs = {k: out[k].numpy() for k in ("blks", "mask", "lines", "mask_u8", "bitmap")}
    chk = LayerCheck(prog, snaps, checker_engine or engine, lambda t: T[t].permute(0, 2, 3, 1).numpy(), outs, x.numpy())
    return chk.check_all(ops)


def _op(prog, name, nth=0):
    return [i for i, o in enumerate(prog.ops) if o["name"] == name][nth]


@pytest.mark.parametrize("engine", ["fp32", "fp16", "fp32s"])
def test_correct_arithmetic_passes_its_bound(engine):
    L = _L()
    prog = _prog(engine)
    blob = hook = None
    if engine == "fp16":
        blob, hook = fp16_emulation(prog)
    elif engine == "fp32s":
        blob, hook = fp32s_emulation(prog)
    res = run_and_check(engine, prog, blob=blob, hook=hook)
    kinds = {prog.ops[i]["kind"] for i, r in res.items() if r["n"] > 0}
    want = {L.OP_CONV, L.OP_CONVT, L.OP_MAXPOOL, L.OP_AVGPOOL2, L.OP_DETECT, L.OP_SEG_FINAL, L.OP_DB_UP}
    want |= {L.OP_STEM} if engine == "fp16" else {L.OP_INPUT}
    assert want <= kinds, want - kinds
    bad = {prog.ops[i]["name"]: r["ratio"] for i, r in res.items() if not r["ratio"] <= 1}
    assert not bad, bad
    print(f"\n{engine}: worst ratio {max(r['ratio'] for r in res.values()):.3g}")


def test_sampled_windows_pass_on_a_large_map():
    """320 x 256: the stem output and its neighbours are larger than 128 x 128 -> 16 x 16 windows with zero-padded crops
    (borders, seams, random) and the ConvTranspose / DB / seg-final window arithmetic."""
    res = run_and_check("fp32", x=_x((2, 320, 256), 4))
    assert all(r["ratio"] <= 1 for r in res.values()), {i: r for i, r in res.items() if not r["ratio"] <= 1}


def test_export_ops_are_checked_exactly():
    """EXPORT (the mask / lines of programs without the fused seg-final and DB tails): replace the fused tails of a
    program by plain ConvTranspose + EXPORT ops built from the same weights."""
    L = _L()
    G = pkg().graph
    prog = _prog("fp32")
    i = next(j for j, o in enumerate(prog.ops) if o["kind"] == L.OP_SEG_FINAL)
    o = prog.ops[i]
    w = prog.blob()[o["w_off"]: o["w_off"] + o["src0_c"] * 16].reshape(o["src0_c"], 1, 4, 4)
    tail = prog.ops[i + 1:]
    prog.ops = prog.ops[:i]
    m = prog.convt(G.View(o["src0"], 0, o["src0_c"], prog.tensors[o["src0"]][1]), w, None, 4, 2, 1, "sigmoid", name="m")
    prog.op(L.OP_EXPORT, src0=m.tid, src0_coff=0, src0_c=1, aux=[L.OUT_MASK, 0] + [0] * 6, name="seg.export")
    prog.ops += tail
    res = run_and_check("fp32", prog)
    e = _op(prog, "seg.export")
    assert res[e]["n"] > 0 and res[e]["ratio"] == 0.0
    assert all(r["ratio"] <= 1 for r in res.values())


# ---------------------------------------------------------------------------------------------------------------------
# mutations: each must be rejected at the op it hits
# ---------------------------------------------------------------------------------------------------------------------

def _recompute(o, ctx, a=None, w=None, b="same"):
    a = ctx["a"] if a is None else a
    w = ctx["w"] if w is None else w
    b = ctx["b"] if isinstance(b, str) else b
    return F.conv2d(a, w, b, o["stride"], o["pad"])


def _mut_tap(o, y, ctx):
    w = ctx["w"].clone()
    w[5, :, 1, 2] = 0                       # output channel 5 loses its right-middle tap
    return _recompute(o, ctx, w=w)


def _mut_halo(o, y, ctx):
    a = ctx["a"].clone()
    a[..., 16] = 0                          # the last column of a 16-wide patch reads zero for its right neighbour
    y = y.clone()
    y[..., 15] = _recompute(o, ctx, a=a)[..., 15]
    return y


def _mut_bias(o, y, ctx):
    y = y.clone()
    y[:, :, -1, :] -= ctx["b"].view(1, -1, 1)     # bottom border row without bias
    return y


def _mut_concat(o, y, ctx):
    a = ctx["a"].clone()
    c0 = o["src0_c"]
    a[:, c0:] = torch.roll(a[:, c0:], 8, 1)       # source 1's channel slice read 8 channels off
    return _recompute(o, ctx, a=a)


MUTATIONS = {
    "tap_dropped": ("model.4.m.0.cv2.conv", "pre", _mut_tap),
    "halo_off_by_one": ("model.2.m.0.cv2.conv", "pre", _mut_halo),
    "bias_missing_on_border_row": ("model.3.conv", "pre", _mut_bias),
    "concat_slice_shifted": ("model.13.cv1+cv2", "pre", _mut_concat),
    "residual_twice": ("model.4.m.1.cv2.conv", "out", lambda o, y, ctx: y + ctx["res"]),
    "residual_left_out": ("model.6.m.1.cv2.conv", "out", lambda o, y, ctx: y - ctx["res"]),
    "page1_written_to_page0": ("model.5.conv", "out", lambda o, y, ctx: torch.cat([y[1:2], y[1:]], 0)),
    "fp16_rounding_under_the_fp32_bound": ("model.8.cv3.conv", "out", lambda o, y, ctx: _f16(y)),
}


@pytest.mark.parametrize("case", sorted(MUTATIONS))
def test_mutation_is_rejected(case):
    name, stage, fn = MUTATIONS[case]
    prog = _prog("fp32")
    i = _op(prog, name)
    if case == "concat_slice_shifted":
        assert prog.ops[i]["src1"] >= 0
    if case.startswith("residual"):
        assert prog.ops[i]["res"] >= 0
    if case == "halo_off_by_one":
        assert prog.ops[i]["k"] == 3 and SHAPE[2] >> 2 > 16

    def hook(j, o, st, y, ctx):
        return fn(o, y, ctx) if (j == i and st == stage) else y
    res = run_and_check("fp32", prog, hook=hook, ops=[i])
    assert res[i]["ratio"] > 1, (case, res[i])


def test_mutation_fp32s_lo_halves_dropped_is_rejected():
    prog = _prog("fp32s")
    i = _op(prog, "model.6.cv3.conv")
    blob, hook = fp32s_emulation(prog, drop_lo_at=i)
    res = run_and_check("fp32s", prog, blob=blob, hook=hook, ops=[i])
    assert res[i]["ratio"] > 1, res[i]


def test_unmutated_ops_of_the_mutation_programs_pass():
    """The same ops unmutated pass their bound: the mutation tests above fail for the mutation and nothing else."""
    prog = _prog("fp32")
    ops = [_op(prog, n) for n, _, _ in MUTATIONS.values()] + [_op(prog, "model.6.cv3.conv")]
    res = run_and_check("fp32", prog, ops=ops)
    assert all(r["ratio"] <= 1 for r in res.values()), res
    prog = _prog("fp32s")
    blob, hook = fp32s_emulation(prog)
    res = run_and_check("fp32s", prog, blob=blob, hook=hook, ops=[_op(prog, "model.6.cv3.conv")])
    assert all(r["ratio"] <= 1 for r in res.values()), res


def test_snapshot_program_computes_the_same_outputs():
    """The identity copies change nothing the program computes."""
    prog = _prog("fp32")
    snap, index, snaps = snapshot_program(prog)
    assert len(snaps) >= 10 and len(snap.ops) == len(prog.ops) + len(snaps)
    x = _x((1, 64, 64))
    a, b = run_program(prog, x), run_program(snap, x)
    for k in ("blks", "mask", "lines", "mask_u8", "bitmap"):
        assert torch.equal(a[k], b[k]), k


# ---------------------------------------------------------------------------------------------------------------------
# the wide-dynamic-range checkpoint family (tests/wide_ckpt.py)
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("act", ["leaky", "silu"])
def test_wide_checkpoint_family_spans_the_range_it_claims(act):
    from wide_ckpt import make_wide_checkpoint
    L = _L()
    ck = make_wide_checkpoint(0, act)
    prog = pkg().graph.lower(ck, L.PREC_F32, act=act)
    out = run_program(prog, _x((1, 128, 128), 5), return_tensors=True)
    spans, peak = [], 0.0
    for tid, t in out["tensors"].items():
        peak = max(peak, float(t.abs().max()))
        rms = t.double().pow(2).mean(dim=(0, 2, 3)).sqrt()
        rms = rms[rms > 0]
        if rms.numel() > 1:
            spans.append(float(torch.log2(rms.max() / rms.min())))
    print(f"\nwide {act}: per-channel activation RMS spans 2^{np.median(spans):.1f} (median over {len(spans)} tensors), "
          f"min 2^{min(spans):.1f}; max |activation| {peak:.3g}")
    assert sum(s >= 12 for s in spans) >= 10, spans          # inside many layers, per-channel RMS spans >= 2^12
    assert peak < 2 ** 14                                    # no fp16 overflow: not the subject here
    for m in (out["mask"], out["lines"]):                    # the heads' maps still spread over (0, 1)
        assert float(((m > 0.02) & (m < 0.98)).float().mean()) > 0.5
        assert float(m.std()) > 0.01


def test_wide_checkpoint_fp32s_emulation_passes_its_bound():
    """The fp32s bound (activations unscaled, 2^-25 absolute floor) holds for split arithmetic on the wide family."""
    from wide_ckpt import make_wide_checkpoint
    L = _L()
    prog = pkg().graph.lower(make_wide_checkpoint(0, "leaky"), L.PREC_F32)
    blob, hook = fp32s_emulation(prog)
    res = run_and_check("fp32s", prog, x=_x((1, 128, 128), 6), blob=blob, hook=hook)
    assert all(r["ratio"] <= 1 for r in res.values()), {prog.ops[i]["name"]: r for i, r in res.items() if not r["ratio"] <= 1}
