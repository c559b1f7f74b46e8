"""TEST INFRASTRUCTURE.  A wide-dynamic-range checkpoint family: `synth.make_checkpoint(seed, act)` (the reference's
weight-file format) with the BatchNorm statistics rewritten per channel the way trained networks have them --

  * running_var log-uniform over 1e-4 ... 1e1;
  * |gamma| log-uniform over 0.1 ... 3 with random signs, and a few channels with gamma = 0;
  * non-zero running_mean (and beta), a fraction of the channel's output scale;

and each conv's weight rows rescaled so that the channel's output RMS is a target t_n drawn log-uniform over
2^-8 ... 2^4 (the folded weights then span decades, near-dead channels get tiny running_var with large folded weights,
and the inputs of the next layer are uniformly small on many channels).  The layers without BatchNorm that end the
network (Detect convs, the heads' last ConvTranspose) are scaled back by the mean input RMS, so the maps still spread
over (0, 1).  tests/test_layer_ref.py checks that the family does what it claims."""
from __future__ import annotations

import importlib
import math

import numpy as np
import torch

LOG2_T = (-8.0, 4.0)                                     # per-channel target output RMS, log2
# quadratic mean of t for log2 t ~ U(-8, 4): the RMS a layer's input has over its channels
Q = math.sqrt((2.0 ** (2 * LOG2_T[1]) - 2.0 ** (2 * LOG2_T[0])) / (2 * math.log(2) * (LOG2_T[1] - LOG2_T[0])))
BASE = 0.2                                               # synth's tuned hidden-activation std


def make_wide_checkpoint(seed: int = 0, act: str = "leaky") -> dict:
    p = importlib.import_module("comic-text-detector_amd")
    arch = p.arch
    ck = p.synth.make_checkpoint(seed, act=act)
    r = np.random.RandomState(1000 + seed)
    layers, _ = arch.parse_yolo_cfg(ck["blk_det"]["cfg"])
    groups = ((ck["blk_det"]["weights"], list(arch.iter_convs(layers))),
              (ck["text_seg"], list(arch.iter_convs(arch.unet_spec(act)))),
              (ck["text_det"], list(arch.iter_convs(arch.db_spec(64, act)))))
    for sd, convs in groups:
        for cs in convs:
            w = sd[cs.prefix + ".weight"].double()
            first = cs.prefix == "model.0.conv"            # reads the image, not a wide hidden tensor
            if cs.bn_prefix is None:
                sd[cs.prefix + ".weight"] = (w * (BASE / Q)).float()
                continue
            bp = cs.bn_prefix
            c = cs.c2
            g0 = sd[bp + ".weight"].double().numpy()
            v0 = sd[bp + ".running_var"].double().numpy()
            eps = cs.bn_eps
            var = 10.0 ** r.uniform(-4, 1, c)
            gamma = np.sign(r.uniform(-1, 1, c)) * 10.0 ** r.uniform(-1, math.log10(3), c)
            if c >= 16:
                gamma[r.choice(c, 2, replace=False)] = 0.0
            t = 2.0 ** r.uniform(*LOG2_T, c)
            fold0 = g0 / np.sqrt(v0 + eps)
            fold = gamma / np.sqrt(var + eps)
            # folded weight row = old folded row x t / (BASE * input RMS ratio): output RMS ~ t
            want = fold0 * t / (BASE if first else Q)
            scale = np.where(gamma != 0, want / np.where(fold != 0, fold, 1.0), 1.0)
            shape = (1, -1, 1, 1) if cs.transposed else (-1, 1, 1, 1)
            sd[cs.prefix + ".weight"] = (w * torch.from_numpy(scale).view(shape)).float()
            # mean / beta: an offset of about half the output scale, either sign
            sd[bp + ".running_mean"] = torch.from_numpy(
                0.5 * r.standard_normal(c) * t * np.sqrt(var + eps) / np.maximum(np.abs(gamma), 1e-3)).float()
            sd[bp + ".bias"] = torch.from_numpy(sd[bp + ".bias"].double().numpy() * t / BASE).float()
            sd[bp + ".weight"] = torch.from_numpy(gamma).float()
            sd[bp + ".running_var"] = torch.from_numpy(var).float()
    return ck
