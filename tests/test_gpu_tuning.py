"""-m gpu: `_lib.tuning` on the real library -- an engine re-plans when a key is set AND when it is put back, and
`ctd_tuning_get` answers for every row of csrc/tuning.def."""
import pytest
import torch

from conftest import checkpoint, pkg
from oracle import gen_golden
from test_layer_ref import tuning_keys_in_the_sources

pytestmark = pytest.mark.gpu


def test_tuning_context_replans_on_the_way_in_and_on_the_way_out():
    """One fp16 engine at (3, 128, 64), the shape at which tests/test_gpu_layers.py proves conv_halo_kernel under
    halo_min_patches = 1 and never at the library's thresholds: forwards before, inside and after
    `tuning(halo_min_patches=1, halo3_min_blocks=1)`.  Then `ctd_tuning_get` of every key, and the clamp of one."""
    p = pkg()
    L = p._lib
    be = p.backend.HipTextDetBackend(checkpoint(0), device="cuda", precision="fp16")
    x = gen_golden.make_input(11, (3, 128, 64)).cuda()

    def forward():
        out = [t.clone() for t in be(x)]
        torch.cuda.synchronize()
        return out, be.op_kernels()
    before, k_before = forward()
    with L.tuning(halo_min_patches=1, halo3_min_blocks=1):
        _, k_inside = forward()
    after, k_after = forward()
    assert "conv_halo_kernel" in {k for _, k in k_inside}
    assert k_before == k_after and "conv_halo_kernel" not in {k for _, k in k_before}
    assert len(before) == len(after) == 3 and all(torch.equal(a, b) for a, b in zip(before, after))

    # every row of the table answers (the two measurement knobs exist under `make MEASURE=1` only); a clamped key reads back
    # clamped and goes back to what it held
    keys = tuning_keys_in_the_sources()
    shipped = [k for k in keys if k not in ("tail_skip_page_download", "tail_ablate")]
    assert len(shipped) == len(keys) - 2
    v = L.C.c_int64()
    for k in shipped:
        assert L.lib().ctd_tuning_get(k.encode(), L.C.byref(v)) == L.OK, k
    assert L.lib().ctd_tuning_get(b"tail_", L.C.byref(v)) != L.OK and L.lib().ctd_tuning_get(b"fuse", None) != L.OK
    held = L.tuning_get("tail_max_blocks")
    with L.tuning(tail_max_blocks=0):
        assert L.tuning_get("tail_max_blocks") == 1
    assert L.tuning_get("tail_max_blocks") == held
