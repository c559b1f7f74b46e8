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


@pytest.mark.parametrize("engine", ["fp32", "fp16"])
def test_hand_built_direct_program_passes_and_a_swapped_tap_index_is_rejected(engine):
    """layer_ref.direct_program (the program tests/test_gpu_layers.py runs on the direct kernels): the checker takes a
    program without the network's output ops, correct arithmetic passes on every op, and a ConvTranspose that reads its
    weights with ky and kx swapped is rejected at both ConvTranspose ops and nowhere else."""
    from layer_ref import direct_program
    L = _L()
    prog, ops = direct_program(L.PREC_F16 if engine == "fp16" else L.PREC_F32)
    x = _x((2, 192, 320), 8)
    blob = hook = None
    if engine == "fp16":
        blob, hook = fp16_emulation(prog)
    kinds = [prog.ops[i]["kind"] for i in ops]
    assert kinds.count(L.OP_CONV) == 5 and kinds.count(L.OP_CONVT) == 2
    assert {prog.ops[i]["act"] for i in ops} == {L.ACT[a] for a in ("silu", "leaky", "relu", "none")}

    def run(hk):
        out = run_program(prog, x, blob=blob, hook=hk, return_tensors=True)
        T = out["tensors"]
        chk = LayerCheck(prog, {}, engine, lambda t: T[t].permute(0, 2, 3, 1).numpy(), {}, x.numpy())
        return chk.check_all(ops)
    res = run(hook)
    assert all(r["n"] > 0 and r["ratio"] <= 1 for r in res.values()), res
    print(f"\n{engine}: worst ratio {max(r['ratio'] for r in res.values()):.3g}")

    def swapped(i, o, stage, y, ctx):
        if stage == "pre" and o["kind"] == L.OP_CONVT:
            y = F.conv_transpose2d(ctx["a"], ctx["w"].transpose(2, 3), ctx["b"], o["stride"], o["pad"])
        return y if hook is None else hook(i, o, stage, y, ctx)
    bad = run(swapped)
    assert {i for i, r in bad.items() if r["ratio"] > 1} == {i for i in ops if prog.ops[i]["kind"] == L.OP_CONVT}, bad


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


def tuning_keys_in_the_sources():
    """The keys ctd_tuning_set accepts: the rows of csrc/tuning.def (the measurement-only ones included)."""
    import os
    import re
    src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "comic-text-detector_amd", "csrc")
    with open(os.path.join(src, "tuning.def")) as fh:
        return re.findall(r'^TUNE\("([a-z0-9_]+)",', fh.read(), re.M)


def test_every_tuning_key_is_in_the_ledger(monkeypatch):
    """A key of ctd_tuning_set is either a dispatch key with the kernels that prove each value (checked on the GPU by
    tests/test_gpu_layers.py) or is listed as knowingly not one, with the reason: a new key needs a decision."""
    import os
    import re
    import test_gpu_layers as G
    keys = tuning_keys_in_the_sources()
    assert len(keys) == len(set(keys)) and len(keys) > 30 and {"fuse", "halo_pair", "halo3", "c3b_cfg64"} <= set(keys)
    dispatch = {k for k, *_ in G.DISPATCH_KEYS}

    def unlisted():
        return sorted(set(keys) - dispatch - set(G.NOT_DISPATCH_KEYS))
    assert not unlisted()
    assert not dispatch & set(G.NOT_DISPATCH_KEYS)
    assert not (dispatch | set(G.NOT_DISPATCH_KEYS)) - set(keys), "the ledger names a key the library does not parse"
    assert all(reason for reason in G.NOT_DISPATCH_KEYS.values())
    # a reason that names the test exercising the key's values names one that exists
    tests = os.path.dirname(os.path.abspath(__file__))
    named = [m for reason in G.NOT_DISPATCH_KEYS.values() for m in re.findall(r"tests/(test_\w+\.py)::(test_\w+)", reason)]
    assert len(named) >= 6
    for mod, fn in named:
        with open(os.path.join(tests, mod)) as fh:
            assert re.search(rf"^def {fn}\(", fh.read(), re.M), (mod, fn)
    # every key a keyed configuration sets is one the library knows (`_lib.tuning` reads it, sets it and puts it back:
    # tests/test_gpu_tuning.py)
    assert {k for c in G.KEYED.values() for k in c[3]} <= set(keys)
    # the check bites: a key in neither table is reported
    monkeypatch.delitem(G.NOT_DISPATCH_KEYS, "fwd_prio")
    assert unlisted() == ["fwd_prio"]


# ---------------------------------------------------------------------------------------------------------------------
# the wide-dynamic-range checkpoint family (tests/wide_ckpt.py)
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("act", ["leaky", "silu", "relu"])
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


# ---------------------------------------------------------------------------------------------------------------------
# sampling that follows the kernels' geometry, and the pages
# ---------------------------------------------------------------------------------------------------------------------

TIMED_PAGES = (0, 1, 15, 16, 30, 31, 7, 22)


def _windows_as_before(Ho, Wo, B, seed, salt):
    """The window set of the sampling before EDGES, restated (not imported): pages 0 and B - 1."""
    ys = lambda v: min(max(v, 0), Ho - 16)      # noqa: E731
    xs = lambda v: min(max(v, 0), Wo - 16)      # noqa: E731
    pos = [(0, 0), (0, Wo), (Ho, 0), (Ho, Wo), (0, Wo // 2 - 8), (Ho, Wo // 2 - 8), (Ho // 2 - 8, 0), (Ho // 2 - 8, Wo)]
    for m in (16, 32, 64, 128, 256):
        if m < Ho or m < Wo:
            pos += [(m - 8, m - 8), (m - 8, Wo // 2 + 3), (Ho // 2 + 5, m - 8)]
    r = np.random.RandomState(seed * 7919 + salt)
    pos += [(int(r.randint(0, Ho - 16 + 1)), int(r.randint(0, Wo - 16 + 1))) for _ in range(4)]
    pos = sorted({(ys(y), xs(x)) for y, x in pos})
    return [(b, y, x, 16, 16) for b in sorted({0, B - 1}) for y, x in pos]


def _planner(B, pages=None, seed=0):
    return LayerCheck(_prog("fp32"), {}, "fp32", None, {}, np.zeros((B, 3, 64, 64)), pages=pages, seed=seed)


def _straddled(wins, b, axis):
    """Positions p of the axis (0: rows, 1: columns) with p - 1 and p both inside one window of page position b."""
    out = set()
    for w in wins:
        if w[0] == b:
            out |= set(range(w[1 + axis] + 1, w[1 + axis] + w[3 + axis]))
    return out


@pytest.mark.parametrize("shape", [(256, 256), (512, 512), (1024, 1024), (1536, 1536), (640, 1024), (320, 448)])
def test_window_plan_visits_every_seam_class_on_every_requested_page(shape):
    import layer_ref as LR
    Ho, Wo = shape
    chk = _planner(32, TIMED_PAGES, seed=3)
    wins = chk.windows(Ho, Wo, len(TIMED_PAGES), salt=5)
    assert {w[0] for w in wins} == set(range(len(TIMED_PAGES))) and chk.real == sorted(TIMED_PAGES)
    assert all(0 <= y and y + h <= Ho and 0 <= x and x + w <= Wo for _, y, x, h, w in wins)
    per_page = [{w[1:] for w in wins if w[0] == b} for b in range(len(TIMED_PAGES))]
    assert all(s == per_page[0] for s in per_page)                       # the same windows on every requested page
    have = per_page[0]
    classes = 0
    for eh, ew, kernel in LR.EDGES:
        ys, xs = LR.seam_positions(eh, Ho), LR.seam_positions(ew, Wo)
        for e, n, got in ((eh, Ho, ys), (ew, Wo, xs)):
            if e < n:                                                    # first, last, and an interior one where there is one
                last = (n - 1) // e * e
                assert got[0] == e and got[-1] == last and all(p % e == 0 and 0 < p < n for p in got), (kernel, n, got)
                assert last - e < 2 * e or any(e < p < last for p in got), (kernel, n, got)
        for y in ys:                                                     # crossed: a corner of four patches of THIS kernel
            for x in xs:
                assert any(y0 < y < y0 + h and x0 < x < x0 + w for y0, x0, h, w in have), (kernel, shape, y, x)
                classes += 1
    assert classes >= 9 * 4
    if shape == (1024, 1024):
        for axis in (0, 1):
            assert {512, 768, 1008} <= _straddled(wins, 0, axis)
    # a row wrap of the linear-block kernels in a late row: the right end of rows and the left start of the same rows
    late = [y for y, x, _, _ in have if x == 0 and (y, Wo - 16, 16, 16) in have and Ho // 2 < y < Ho - 16]
    assert late, shape
    inside = lambda q: any(y <= q // Wo < y + h and x <= q % Wo < x + w for y, x, h, w in have)      # noqa: E731
    for lb in LR.LINEAR_BLOCKS:              # a block edge past the middle of the map: its first pixel and the one before it
        assert any(inside(q) and inside(q - 1) for q in range((Ho // 2 * Wo) // lb * lb + lb, Ho * Wo, lb)), (shape, lb)
    # what the earlier sampling looked at is all still there: on the pages it used, with and without `pages`
    old = _windows_as_before(Ho, Wo, len(TIMED_PAGES), 3, 5)
    assert set(old) <= set(wins) and set(old) == set(chk.windows(Ho, Wo, len(TIMED_PAGES), salt=5, legacy=True))
    plain = _planner(32, None, seed=3)
    assert set(_windows_as_before(Ho, Wo, 32, 3, 5)) <= set(plain.windows(Ho, Wo, 32, salt=5))
    assert {w[0] for w in plain.windows(Ho, Wo, 32, salt=5)} == {0, 31}
    print(f"\n{shape}: {len(have)} windows per page ({len(old) // 2} before), "
          f"{len(have) * 256 / (Ho * Wo):.2%} of a page's positions at the most")


def test_small_maps_are_checked_in_full_on_the_requested_pages():
    chk = _planner(32, TIMED_PAGES)
    assert chk.windows(128, 128, 8) == [(b, 0, 0, 128, 128) for b in range(8)] and chk.B == 8 and chk.B_all == 32
    assert _planner(4).windows(64, 128, 4) == [(b, 0, 0, 64, 128) for b in range(4)]


BIG = (3, 512, 512)
_BIG = {}


def _big():
    """The fp32 program on three 512 x 512 pages (the first conv's map is 256 x 256: sampled), run once."""
    if not _BIG:
        L = _L()
        prog = _prog("fp32")
        snap, index, snaps = snapshot_program(prog)
        x = _x(BIG, 8)
        out = run_program(snap, x, return_tensors=True)
        i = next(j for j, o in enumerate(prog.ops) if o["kind"] == L.OP_CONV and prog.tensors[o["dst"]][1] == 1)
        assert i not in snaps and prog.ops[i]["dst_coff"] == 0
        _BIG.update(prog=prog, snaps=snaps, x=x, T=out["tensors"], i=i,
                    outs={k: out[k].numpy() for k in ("blks", "mask", "lines", "mask_u8", "bitmap")})
    return _BIG


def _check_big(T, **kw):
    g = _big()
    chk = LayerCheck(g["prog"], g["snaps"], "fp32", lambda t: T[t].permute(0, 2, 3, 1).numpy(), g["outs"], g["x"].numpy(), **kw)
    return chk, chk.check_all([g["i"]])[g["i"]]


def _with_error(page, y0, x0, factor=4.0):
    """The engine's tensors with `factor` times the bound added to the 16 x 16 patch at (y0, x0) of one page of the op."""
    g = _big()
    i = g["i"]
    chk = LayerCheck(g["prog"], g["snaps"], "fp32", lambda t: g["T"][t].permute(0, 2, 3, 1).numpy(), g["outs"], g["x"].numpy())
    (_, ref, D), = chk.conv_bounds(i, [(page, y0, x0, 16, 16)])
    assert float(D.min()) > 0
    T = dict(g["T"])
    t = T[g["prog"].ops[i]["dst"]].clone()
    t[page, :, y0: y0 + 16, x0: x0 + 16] = torch.from_numpy(ref + factor * D).float()
    T[g["prog"].ops[i]["dst"]] = t
    return T


def test_unmutated_large_map_passes_with_the_new_windows_on_every_page():
    chk, r = _check_big(_big()["T"], pages=(0, 1, 2))
    assert r["ratio"] <= 1 and r["total"] == 3 * 256 * 256 * _big()["prog"].ops[_big()["i"]]["cout"] and 0 < r["n"] < r["total"]
    _, r2 = _check_big(_big()["T"])
    assert r2["ratio"] <= r["ratio"] and r2["n"] < r["n"]                     # pages 0 and 2 only


def test_mutation_in_one_interior_patch_is_missed_by_the_earlier_windows_and_rejected_now():
    import layer_ref as LR
    g = _big()
    Ho = Wo = BIG[1] // 2
    old = LayerCheck(g["prog"], g["snaps"], "fp32", None, g["outs"], g["x"].numpy(), legacy_windows=True)
    before = old.windows(Ho, Wo, BIG[0], salt=g["i"])
    assert set(before) == set(_windows_as_before(Ho, Wo, BIG[0], 0, g["i"]))
    s = LR.seam_positions(16, Ho)
    # a 16 x 16 patch up and left of a corner of four patches (last seam x interior seam first) that no earlier window touches
    cand = [(y - 16, x - 16) for y in reversed(s) for x in s[1:]]
    free = [(y, x) for y, x in cand if not any(y0 < y + 16 and y < y0 + 16 and x0 < x + 16 and x < x0 + 16
                                                for _, y0, x0, _, _ in before)]
    assert free, cand
    y0, x0 = free[0]
    assert 16 <= y0 and y0 + 32 <= Ho and 16 <= x0 and x0 + 32 <= Wo        # interior
    T = _with_error(0, y0, x0)
    _, missed = _check_big(T, legacy_windows=True)
    _, caught = _check_big(T)
    print(f"\npatch ({y0}, {x0}) of page 0 off by 4 bounds: earlier windows {missed['ratio']:.3g}, now {caught['ratio']:.3g} "
          f"at page {caught['page']} window {caught['win']}")
    assert missed["ratio"] <= 1, missed
    assert caught["ratio"] > 1 and caught["page"] == 0, caught
    assert caught["ratio"] > 2.9                                              # 4 bounds, less the engine's own error (< 1)


def test_mutation_on_a_middle_page_is_missed_by_the_earlier_pages_and_rejected_now():
    T = _with_error(1, 0, 0)                                                  # the corner window: every plan has it
    _, missed = _check_big(T, legacy_windows=True)
    _, missed_too = _check_big(T)                                             # without `pages`: 0 and B - 1, as before
    _, caught = _check_big(T, pages=(0, 1, 2))
    assert missed["ratio"] <= 1 and missed_too["ratio"] <= 1, (missed, missed_too)
    assert caught["ratio"] > 2.9 and caught["page"] == 1 and caught["win"] == (0, 0), caught
    _, named = _check_big(T, pages=(1,))                                      # results name the page of the batch
    assert named["ratio"] > 2.9 and named["page"] == 1


def test_only_the_requested_pages_are_kept_and_tensors_are_dropped_after_their_last_reader():
    L = _L()
    prog = _prog("fp32")
    snap, index, snaps = snapshot_program(prog)
    x = _x((4, 64, 64), 9)
    out = run_program(snap, x, return_tensors=True)
    T = out["tensors"]
    outs = {k: out[k].numpy() for k in ("blks", "mask", "lines", "mask_u8", "bitmap")}
    reads = []

    def get(t):
        reads.append(t)
        return T[t].permute(0, 2, 3, 1).numpy()
    full = LayerCheck(prog, snaps, "fp32", get, outs, x.numpy()).check_all()
    assert len(reads) == len(set(reads))                                      # eviction never made the checker read twice
    chk = LayerCheck(prog, snaps, "fp32", get, outs, x.numpy(), pages=(1, 2))
    part = chk.check_all()
    assert not chk._cache and chk.peak_cached_bytes > 0
    everything = sum(T[t].numel() * 4 for t in set(reads)) // 2               # two of four pages of every tensor read
    assert chk.peak_cached_bytes < everything / 2, (chk.peak_cached_bytes, everything)
    only = LayerCheck(prog, snaps, "fp32", lambda t: T[t][1:3].permute(0, 2, 3, 1).numpy(), {k: v[1:3] for k, v in outs.items()},
                      x[1:3].numpy()).check_all()
    for i in full:
        assert part[i]["ratio"] == only[i]["ratio"] <= full[i]["ratio"] <= 1 and part[i]["n"] == only[i]["n"], (i, part[i], only[i])
        assert part[i]["page"] in (None, 1, 2) and part[i]["total"] == full[i]["total"]
