"""-m gpu: parity AT THE DISPATCH THAT IS TIMED.  `bench.py` times B = 32 pages of 1024 x 1024 with the default grid
thresholds; at that shape the engine launches kernels that a B = 1 forward never selects (`conv_halo3_kernel`: at least
1024 blocks; `c3_fused_kernel`, `c3b_kernel`: at least 1024 patches).  Every other oracle comparison of the suite runs small
shapes, where those kernels are either off or forced on by a tuning key and checked against OTHER HIP kernels.  Here the
benchmark's own batch (its checkpoint, its first 32 pages) goes through the fp16, the fp32s and the fp32 engine (the detector's
default precision) ONCE, as benchmarked,
and all 32 pages' outputs are compared with the oracle network (the reference's torch modules on the CPU, fp32) --
reference seam `inference.py:129,146`:

  * the kernels that ran are asserted by name (`ctd_engine_op_kernel`);
  * fp32s, fp32: the fp32 tolerances of tests/test_gpu_net.py (maps 2e-5 abs, Detect rows 1e-4 rel, u8 mask at most one level
    on < 0.1 % of the pixels) on every page;
  * fp16: the golden tolerances (2e-2 max / 2e-3 mean) on every page and the threshold-band assertions of
    tests/test_gpu_accept.py on pages 0, 10, 21 and 31;
  * end to end through `detect_batch` (one forward + one native tail for the 32 pages): those four pages' lines / blocks /
    masks against oracle forward + oracle tail.
"""
import numpy as np
import pytest
import torch

from conftest import pkg
from oracle import accept
from oracle import postproc_ref as R
from oracle.net_ref import OracleNet

pytestmark = pytest.mark.gpu

B, SIZE = 32, 1024
E2E_PAGES = (0, 10, 21, 31)
EPS_FP16 = 4e-3                 # tests/test_gpu_accept.py
_S = {}


def workload():
    """bench.py's default workload on rank 0: its checkpoint and the 32 pages of its first batch."""
    if "ck" not in _S:
        p = pkg()
        _S["ck"] = p.synth.make_blob_checkpoint(0, sparse_det=True, line_density="fixture")
        _S["pages"] = [p.synth.text_like_page((SIZE, SIZE), i) for i in range(B)]
    return _S["ck"], _S["pages"]


def oracle():
    """Oracle network outputs of the 32 pages (bs = 1 like the reference's `__call__`), ~15 s of host time, once."""
    if "oracle" not in _S:
        ck, pages = workload()
        torch.set_num_threads(16)
        net = OracleNet(ck)
        outs = []
        for pg in pages:
            x = torch.from_numpy(np.ascontiguousarray(pg.transpose(2, 0, 1)[None])).float() / 255
            ob, om, ol = net(x)
            outs.append((ob.numpy(), om.numpy(), ol.numpy()))
        _S["oracle"] = outs
    return _S["oracle"]


def oracle_tail(b):
    key = ("tail", b)
    if key not in _S:
        _, pages = workload()
        ob, om, ol = oracle()[b]
        ref = R.detector_tail(pages[b], ob, om, ol, input_size=(SIZE, SIZE), refine_mode=0, keep_undetected_mask=False)
        dets = np.asarray(R.non_max_suppression(ob, 0.4, 0.35)[0])
        sbb = accept.score_band_boxes(ol, (SIZE, SIZE), EPS_FP16)
        cand = np.asarray(R.seg_rep((SIZE, SIZE), ol)[0][0])
        _S[key] = (ref, dets, sbb, cand)
    return _S[key]


def run_batch(prec):
    """One B = 32 forward at the DEFAULT thresholds + one native tail for the batch; everything fetched to the host."""
    key = ("run", prec)
    if key not in _S:
        ck, pages = workload()
        p = pkg()
        det = p.detector.TextDetector(ck, input_size=SIZE, device="cuda", precision=prec)
        x = torch.from_numpy(np.stack(pages)).cuda()
        blks, mask, lines = det.net.forward_u8(x)
        torch.cuda.synchronize()
        kernels = det.net.op_kernels()
        res = dict(det=det, x=x, blks=blks, mask=mask.cpu().numpy(), lines=lines.cpu().numpy(), blks_h=blks.cpu().numpy(),
                   lines_dev=lines, mask_u8=det.net.mask_u8.clone(), bitmap=det.net.bitmap.clone(), kernels=kernels)
        res["e2e"] = det.detect_batch([x[i] for i in range(B)], refine_mode=0, keep_undetected_mask=False)
        assert det.net.op_kernels() == kernels          # the tail's forward ran the same dispatch
        _S[key] = res
    return _S[key]


@pytest.mark.parametrize("prec", ["fp16", "fp32s", "fp32"])
def test_the_timed_dispatch_ran(prec):
    k = run_batch(prec)["kernels"]
    names = {kern for _, kern in k}
    if prec == "fp16":
        convt = [kern for n, kern in k if n.endswith("conv.1")]
        # the ConvTranspose 4x4/s2 layers from 64^2 maps up; two of them with their 1x1 consumer folded in
        assert len(convt) == 7 and sum(c.startswith("conv_halo3_kernel") for c in convt) >= 5, convt
        assert convt.count("conv_halo3_kernel+1x1") == 2 and convt.count("conv_halo3_kernel+taps") == 1, convt
        assert dict(k)["seg.upconv6"] == "seg_final_gather_kernel"
        assert dict(k)["model.2.cv1+cv2"] == "c3_fused_kernel"
        c3b = [n for n, kern in k if kern == "c3b_kernel"]
        # model.4 (x2), model.6 (x3), model.13 / 17 / 20, seg.upconv4 / 5.conv.0, db.upconv4.conv.0
        assert len(c3b) == 11 and "upconv5.conv.0.m.0.cv1.conv" in c3b, c3b
        assert {"stem_conv2_kernel", "conv_halo_kernel", "conv_igemm_kernel", "sppf_pool3_kernel", "db_up_mfma_kernel"} <= names, names
    elif prec == "fp32s":
        assert {"conv_split_halo_kernel", "conv_split_kernel", "stem_split_kernel"} <= names, names
    else:
        # f32 operands all the way: the page through input_kernel, every conv layer on the f32 MFMA kernel, the two heads'
        # tails on their f32 kernels -- and nothing of the fp16 or the split engine
        assert {"input_kernel", "conv_f32_mfma_kernel", "seg_final_f32_kernel", "db_up_kernel"} <= names, names
        assert not [n for n in names if any(w in n for w in ("split", "igemm", "halo", "c3", "stem"))], names
        conv = [kern for _, kern in k if kern.startswith("conv")]
        assert set(conv) <= {"conv_f32_mfma_kernel", "conv_direct_kernel", "convt_direct_kernel"}, set(conv)
        assert conv.count("conv_f32_mfma_kernel") * 2 > len(conv) >= 60, conv


def test_fp32s_batch_of_32_matches_oracle_on_every_page():
    _fp32_bars_on_every_page("fp32s")


def test_fp32_batch_of_32_matches_oracle_on_every_page():
    """The detector's DEFAULT precision at the timed shape: exactly the bars of the fp32s test above."""
    _fp32_bars_on_every_page("fp32")


def _fp32_bars_on_every_page(prec):
    r = run_batch(prec)
    mask_u8, bitmap = r["mask_u8"].cpu().numpy(), r["bitmap"].cpu().numpy()
    for b, (ob, om, ol) in enumerate(oracle()):
        np.testing.assert_allclose(r["mask"][b: b + 1], om, rtol=0, atol=2e-5, err_msg=f"page {b}")
        np.testing.assert_allclose(r["lines"][b: b + 1], ol, rtol=0, atol=2e-5, err_msg=f"page {b}")
        np.testing.assert_allclose(r["blks_h"][b: b + 1], ob, rtol=1e-4, atol=2e-3, err_msg=f"page {b}")
        ref_u8 = (om[0, 0] * 255).astype(np.uint8)
        diff = np.abs(ref_u8.astype(int) - mask_u8[b].astype(int))
        assert diff.max() <= 1 and (diff > 0).mean() < 1e-3, (b, diff.max(), (diff > 0).mean())
        assert ((ol[0, 0] > 0.3) != bitmap[b].astype(bool)).mean() < 1e-3, b


def test_fp16_batch_of_32_stays_inside_the_band_on_every_page():
    r = run_batch("fp16")
    mask_u8, bitmap = r["mask_u8"].cpu().numpy(), r["bitmap"].cpu().numpy()
    worst = 0.0
    for b, (ob, om, ol) in enumerate(oracle()):
        for got, ref in ((r["mask"][b: b + 1], om), (r["lines"][b: b + 1], ol)):
            d = np.abs(got - ref)
            assert d.max() < 2e-2 and d.mean() < 2e-3, (b, d.max(), d.mean())
            worst = max(worst, float(d.max()))
        # Detect scores: this checkpoint's detection head is calibrated to fire sparsely (steep logits), so a score moves
        # by up to sigmoid'(z) * |dz| = 0.25 * 0.13 where the golden network's (tests/test_gpu_net.py: 2e-2) moves 0.02;
        # bound: 5e-2 max, 2e-3 mean
        ds = np.abs(r["blks_h"][b: b + 1][..., 4:] - ob[..., 4:])
        assert ds.max() < 5e-2 and ds.mean() < 2e-3, (b, ds.max(), ds.mean())
        if b in E2E_PAGES:
            rep = accept.band_report(ol[0, 0], om[0, 0], bitmap[b], mask_u8[b], EPS_FP16, prob=r["lines"][b, 0], mask=r["mask"][b, 0])
            rep.pop("_flips")
            print(f"\nfp16 B=32 page {b}: {rep}")
            assert rep["prob_max_abs_delta"] < EPS_FP16 and rep["mask_max_abs_delta"] < EPS_FP16
            assert rep["bitmap_flips_out_of_band"] == 0 and rep["mask127_flips_out_of_band"] == 0
            assert rep["bitmap_in_band_frac"] < 0.01 and rep["mask127_in_band_frac"] < 0.01
    print(f"\nfp16 B=32: worst |map - oracle| over 32 pages {worst:.3g}")


@pytest.mark.parametrize("prec", ["fp32s", "fp16", "fp32"])
def test_detect_batch_of_32_matches_oracle_end_to_end(prec):
    p = pkg()
    r = run_batch(prec)
    _, pages = workload()
    for b in E2E_PAGES:
        ref, ref_dets, sbb, ref_cand = oracle_tail(b)
        got = r["e2e"][b]
        rep = accept.compare(got, ref)
        print(f"\nB=32 dispatch, engine {prec}, page {b}: {rep}")
        assert rep["lines"]["ref"] >= 5
        if prec in ("fp32s", "fp32"):
            assert rep["mask_u8_max_level_diff"] <= 1 and rep["mask_u8_equal_frac"] > 0.999
            assert rep["lines"]["identical"] == rep["lines"]["ref"] == rep["lines"]["ours"]
            assert rep["blocks"]["identical"] == rep["blocks"]["ref"] == rep["blocks"]["ours"]
            assert rep["refined_mask_equal_frac"] > 0.9999
            continue
        assert rep["mask_u8_max_level_diff"] <= 2 and rep["mask_iou_at_127"] > 0.995
        ob, om, ol = oracle()[b]
        band = accept.band_report(ol[0, 0], om[0, 0], r["bitmap"][b].cpu().numpy(), r["mask_u8"][b].cpu().numpy(), EPS_FP16,
                                  prob=r["lines"][b, 0], mask=r["mask"][b, 0])
        flips = band.pop("_flips")
        blks = r["blks"][b: b + 1]
        dets, counts = p.backend.nms(blks, 0.4, 0.35)
        extras = r["det"].tail_batch([pages[b]], blks, r["mask_u8"][b: b + 1], r["lines_dev"][b: b + 1, 0].contiguous(),
                                     r["bitmap"][b: b + 1], want_extras=True)[0][3]
        geo = accept.explain_geometry(got, ref, flips, dets=dets[0, : int(counts[0])].cpu().numpy(), ref_dets=ref_dets,
                                      score_band_boxes=sbb, candidates=(extras["db_boxes"], ref_cand, 1000))
        nl, nb = rep["lines"], rep["blocks"]
        assert geo["lines_unexplained"] == 0 and geo["blocks_unexplained"] == 0, geo
        assert nl["identical"] >= nl["ref"] - geo["lines_differing"] and nb["identical"] >= nb["ref"] - geo["blocks_differing"]
        assert nl["identical"] >= 0.5 * nl["ref"]


def test_detect_batch_of_32_in_the_reference_cli_configuration_matches_oracle():
    """The reference's command line runs `TextDetector.__call__(img, refine_mode=REFINEMASK_ANNOTATION,
    keep_undetected_mask=True)` (inference.py:35, `model2annotations`): no dilation in merge_mask_list, and
    refine_undetected_mask edits the predicted mask in place and gives the left-over components their own refine pass.
    The exact engine at the timed dispatch in THAT configuration, pages 0 / 10 / 21 / 31 against oracle forward + oracle tail:
    lines and blocks identical, the edited mask and the refined mask equal."""
    ck, pages = workload()
    r = run_batch("fp32s")
    got_all = r["det"].detect_batch([r["x"][i] for i in range(B)], refine_mode=1, keep_undetected_mask=True)
    paths = pkg().tail.thread_tail(torch.device("cuda", 0)).refine_paths()
    assert paths["lds"] > 0, paths                       # the window-local merge kernel served the second refine pass
    for b in E2E_PAGES:
        ob, om, ol = oracle()[b]
        ref = R.detector_tail(pages[b], ob, om, ol, input_size=(SIZE, SIZE), refine_mode=1, keep_undetected_mask=True)
        rep = accept.compare(got_all[b], ref)
        print(f"\nB=32 dispatch, fp32s, reference CLI configuration, page {b}: {rep}")
        assert rep["lines"]["identical"] == rep["lines"]["ref"] == rep["lines"]["ours"]
        assert rep["blocks"]["identical"] == rep["blocks"]["ref"] == rep["blocks"]["ours"]
        assert rep["mask_u8_max_level_diff"] <= 1 and rep["mask_u8_equal_frac"] > 0.999
        assert rep["refined_mask_equal_frac"] > 0.9999
