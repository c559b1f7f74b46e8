"""Pins the oracle network (oracle/net_ref.py):
  * against the committed golden vectors, which were produced by the REFERENCE's
    own torch modules (oracle/gen_golden.py) -- runs everywhere;
  * bit-for-bit against the reference modules themselves: live where the reference
    tree is present, else against their stored results (tests/refcode.py)."""
import numpy as np
import pytest
import torch

from conftest import checkpoint, ckpt_checksum, load_golden
from oracle import gen_golden
from oracle.net_ref import OracleNet
from refcode import reference_results

SMALL = sorted(gen_golden.SMALL_CASES)


@pytest.mark.parametrize("name", SMALL)
def test_oracle_matches_reference_golden(name):
    g = load_golden(name)
    ck = checkpoint(int(g["wseed"]))
    # the seeded generators must reproduce the exact weights/inputs the fixture was made from
    assert ckpt_checksum(ck) == pytest.approx(float(g["ckpt_sum"]), rel=0, abs=1e-9)
    x = gen_golden.make_input(int(g["iseed"]), tuple(int(v) for v in g["shape"]))
    assert float(x.double().sum()) == pytest.approx(float(g["input_sum"]), rel=0, abs=1e-9)
    blks, mask, lines = OracleNet(ck)(x)
    # same torch build + same op sequence => identical bits; allow 2 ulp-ish slack for
    # a different CPU's oneDNN kernel selection on the GPU box's host
    np.testing.assert_allclose(mask.numpy(), g["mask"], rtol=0, atol=2e-6)
    np.testing.assert_allclose(lines.numpy(), g["lines"], rtol=0, atol=2e-6)
    np.testing.assert_allclose(blks.numpy(), g["blks"], rtol=2e-5, atol=2e-4)


def test_oracle_bit_exact_vs_reference_modules():
    ck = checkpoint(0)
    x = torch.rand(2, 3, 128, 192, generator=torch.Generator().manual_seed(7))

    def compute():
        from oracle.ref_import import ReferenceNet
        return ReferenceNet(ck)(x)
    rb, rm, rl = (torch.from_numpy(t) for t in reference_results("net_bit_exact", compute))
    ob, om, ol = OracleNet(ck)(x)
    assert torch.equal(rb, ob) and torch.equal(rm, om) and torch.equal(rl, ol)


def test_synthetic_checkpoint_is_in_reference_format():
    """strict load_state_dict into the reference's Model / UnetHead / DBHead succeeds: the checkpoint's names and shapes
    are those of the reference modules' state dicts."""
    ck = checkpoint(3)

    def compute():
        from oracle.ref_import import ReferenceNet
        ref = ReferenceNet(ck)
        n = sum(p.numel() for m in (ref.blk_det, ref.text_seg, ref.text_det) for p in m.parameters())
        # the heads' state dicts; the detector's BNs are folded after its strict load, so for it the names and shapes
        # that load accepted
        shapes = {k: {name: tuple(v.shape) for name, v in getattr(ref, k).state_dict().items()} for k in ("text_seg", "text_det")}
        return dict(n=n, blk_det={name: tuple(v.shape) for name, v in ck["blk_det"]["weights"].items()}, **shapes)
    t = reference_results("checkpoint_format", compute)
    assert 23.0e6 < t["n"] < 23.8e6     # SURVEY: 23.4 M params
    for k, sd in (("blk_det", ck["blk_det"]["weights"]), ("text_seg", ck["text_seg"]), ("text_det", ck["text_det"])):
        assert {name: tuple(v.shape) for name, v in sd.items()} == t[k], k


def test_oracle_step_function_equals_reference_dbhead_step_eval():
    """`DBHead.forward(step_eval=True)` (reference basemodel.py:121-122,159-160) vs the restated step function
    applied to the oracle's two DB planes."""
    ck = checkpoint(0)
    x = torch.rand(1, 3, 128, 128, generator=torch.Generator().manual_seed(11))

    def compute():
        from oracle.ref_import import ReferenceNet
        ref = ReferenceNet(ck)
        with torch.no_grad():
            blks, feats = ref.blk_det(x, detect=True)
            mask, feats2 = ref.text_seg(*feats, forward_mode=ref._mode)
            return ref.text_det(*feats2, step_eval=True), ref.text_det.k
    theirs, k = reference_results("dbhead_step_eval", compute)
    theirs = torch.from_numpy(theirs)
    _, _, lines = OracleNet(ck)(x)
    ours = OracleNet.step_function(lines, k=k)
    assert theirs.shape == ours.shape == (1, 1, 128, 128)
    assert torch.equal(theirs, ours)
