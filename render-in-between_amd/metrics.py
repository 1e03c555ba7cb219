"""Ground-truth quality metrics of rendered frames: the reference's Evaluator.compute_metrics
(PGNR/models/evaluator.py:149-163) with piq's defaults, psnr(data_range=1, reduction='mean') and ssim(data_range=1).

Restated from piq, unpinned (piq is not a dependency; the same status resize.py has for OpenCV):

    x = clamp(pred*0.5+0.5, 0, 1) * mask, y = the same of target       (frames NCHW in [-1,1], C = 3; mask [B,H,W] or None)
    PSNR = -10 log10(mean over C,H,W of (x-y)^2 + 1e-8)                 (full resolution; identical frames: exactly 80)
    SSIM:  f = max(1, round(min(H,W)/256)) (Python's round); f > 1: avg_pool2d(kernel f, stride f, floor) of x and y;
           11x11 gaussian window, sigma 1.5, normalised; depthwise convolution with valid padding -> mu_x, mu_y, E[x^2],
           E[y^2], E[xy]; s_xx = E[x^2]-mu_x^2, s_yy likewise, s_xy = E[xy]-mu_x mu_y;
           map = (2 mu_x mu_y + C1)/(mu_x^2 + mu_y^2 + C1) * (2 s_xy + C2)/(s_xx + s_yy + C2), C1 = 0.01^2, C2 = 0.03^2;
           per-frame SSIM = mean of the map over the channels and the valid positions.  A pooled side below 11 is a
           ValueError, as in piq.

psnr_ssim() runs the HIP kernels (rib_quality, Generator.quality) when it is given a native model and device tensors; the
torch statement below (fp64) serves CPU tensors and models that only speak the reference's call protocol.
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

WINDOW = 11
SIGMA = 1.5
C1 = 0.01 ** 2
C2 = 0.03 ** 2
EPS = 1e-8
PROTOCOL = {"source": "PGNR/models/evaluator.py:149-163 compute_metrics, piq defaults (restated from piq, unpinned)",
            "value_range": "frames in [-1,1] -> clamp(x*0.5+0.5, 0, 1) * mask", "psnr_data_range": 1.0, "psnr_eps": EPS,
            "ssim_data_range": 1.0, "ssim_window": WINDOW, "ssim_sigma": SIGMA, "ssim_k1": 0.01, "ssim_k2": 0.03,
            "ssim_downsample": "f = max(1, round(min(H,W)/256)), avg_pool2d(f)", "ssim_padding": "valid"}
# the `mask` field of a report measured under pose_mask=True (rasterise.human_mask; PGNR/datasets/HSM_auto_dataset.py:254-334)
POSE_MASK = "pose: _generate_human_mask restated from OpenCV's drawing, unpinned"


def downsample_factor(H, W):
    """piq's SSIM pre-pooling factor: max(1, round(min(H, W) / 256)), Python's round (half to even)."""
    return max(1, round(min(int(H), int(W)) / 256))


def _taps(dtype=torch.float64):
    c = torch.arange(WINDOW, dtype=torch.float64) - (WINDOW - 1) / 2
    g = torch.exp(-(c ** 2) / (2 * SIGMA ** 2))
    return (g / g.sum()).to(dtype)


def _check(pred, target, mask):
    if pred.dim() != 4 or pred.shape != target.shape:
        raise ValueError("pred and target must be [B,C,H,W] tensors of one shape, got %s and %s"
                         % (tuple(pred.shape), tuple(target.shape)))
    B, _, H, W = pred.shape
    if mask is not None and tuple(mask.shape) != (B, H, W):
        raise ValueError("mask must be [B,H,W] = %s, got %s" % ((B, H, W), tuple(mask.shape)))
    f = downsample_factor(H, W)
    if H // f < WINDOW or W // f < WINDOW:
        raise ValueError("SSIM: the frame is %dx%d after %dx downsampling, smaller than the %dx%d window"
                         % (H // f, W // f, f, WINDOW, WINDOW))


def psnr_ssim_torch(pred, target, mask=None):
    """The statement above in fp64 torch ops: (psnr[B], ssim[B]) as float32 tensors on pred's device."""
    _check(pred, target, mask)
    x = torch.clamp(pred.to(torch.float64) * 0.5 + 0.5, 0, 1)
    y = torch.clamp(target.to(torch.float64) * 0.5 + 0.5, 0, 1)
    if mask is not None:
        m = mask.to(x).unsqueeze(1)
        x, y = x * m, y * m
    B, Cc, H, W = x.shape
    psnr = -10 * torch.log10(((x - y) ** 2).mean(dim=(1, 2, 3)) + EPS)
    f = downsample_factor(H, W)
    if f > 1:
        x, y = F.avg_pool2d(x, kernel_size=f), F.avg_pool2d(y, kernel_size=f)
    g = _taps().to(x.device)
    gh, gv = g.view(1, 1, 1, WINDOW).repeat(5 * Cc, 1, 1, 1), g.view(1, 1, WINDOW, 1).repeat(5 * Cc, 1, 1, 1)
    stack = torch.cat([x, y, x * x, y * y, x * y], dim=1)                      # separable: the 2-D window is g g^T
    mom = F.conv2d(F.conv2d(stack, gh, groups=5 * Cc), gv, groups=5 * Cc)
    mx, my, exx, eyy, exy = mom.split(Cc, dim=1)
    sxx, syy, sxy = exx - mx * mx, eyy - my * my, exy - mx * my
    cs = (2 * sxy + C2) / (sxx + syy + C2)
    smap = (2 * mx * my + C1) / (mx * mx + my * my + C1) * cs
    return psnr.to(torch.float32), smap.mean(dim=(1, 2, 3)).to(torch.float32)


def psnr_ssim(pred, target, mask=None, model=None):
    """Per-frame (psnr[B], ssim[B]) of [B,3,H,W] frames in [-1,1] against ground truth, mask [B,H,W] optional.
    With a native model (Generator) and tensors on its device: the HIP kernels on the model's stream; else the torch
    statement (CPU tensors, reference-protocol models)."""
    if model is not None and hasattr(model, "quality") and pred.is_cuda:
        return model.quality(pred, target, mask)
    return psnr_ssim_torch(pred, target, mask)


def mean_record(records):
    """The reference's four keys averaged over per-frame records (evaluator.py:131-134: sums / cnt)."""
    keys = ("DAIN_PSNR", "DAIN_SSIM", "OURS_PSNR", "OURS_SSIM")
    n = len(records)
    if n == 0:
        return {k: math.nan for k in keys}
    return {k: math.fsum(r[k] for r in records) / n for k in keys}
