"""Ground-truth PSNR / SSIM on the MI355X: rib_quality (csrc/quality.hip.h, Generator.quality) against an independent fp64
restatement of the reference's compute_metrics with piq's defaults (PGNR/models/evaluator.py:149-163), and the folder
driver's measurements end to end on the native path."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import render_in_between_amd as rib
from render_in_between_amd import evaluator as ev, synth

pytestmark = pytest.mark.gpu

_G = {}


def restated(pred, target, mask=None):
    """piq psnr / ssim (data_range=1) per frame, fp64, 2-D 11x11 gaussian window (sigma 1.5), valid padding."""
    x = torch.clamp(pred.double() * 0.5 + 0.5, 0, 1)
    y = torch.clamp(target.double() * 0.5 + 0.5, 0, 1)
    if mask is not None:
        m = mask.double().unsqueeze(1).expand_as(x)
        x, y = x * m, y * m
    psnr = -10 * torch.log10(((x - y) ** 2).mean(dim=(1, 2, 3)) + 1e-8)
    f = max(1, round(min(x.shape[-2:]) / 256))
    if f > 1:
        x, y = F.avg_pool2d(x, f), F.avg_pool2d(y, f)
    c = (torch.arange(11, dtype=torch.float64) - 5) ** 2
    g = torch.exp(-(c.view(1, -1) + c.view(-1, 1)) / 4.5)
    g = (g / g.sum()).expand(3, 1, 11, 11)
    conv = lambda t: F.conv2d(t, g, groups=3)                                  # noqa: E731
    mx, my = conv(x), conv(y)
    sxx, syy, sxy = conv(x * x) - mx * mx, conv(y * y) - my * my, conv(x * y) - mx * my
    smap = (2 * mx * my + 1e-4) / (mx * mx + my * my + 1e-4) * (2 * sxy + 9e-4) / (sxx + syy + 9e-4)
    return psnr, smap.mean(dim=(1, 2, 3))


def handle(dtype="f32"):
    if dtype not in _G:
        cfg = rib.hsm_gen_config()
        spec = rib.GenSpec.from_cfg(cfg)
        G = rib.Generator(cfg, compute_dtype=dtype).eval()
        G.load_state_dict(synth.make_state_dict(spec, 0))
        _G[dtype] = G
    return _G[dtype]


def pair(B, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.linspace(0, 5, H), torch.linspace(0, 7, W), indexing="ij")
    a = torch.sin(xx + 0.6 * yy + torch.rand(B, 3, 1, 1, generator=g) * 6) * 0.9 + 0.05 * torch.randn(B, 3, H, W, generator=g)
    b = a + 0.15 * torch.randn(B, 3, H, W, generator=g)
    b[:, :, : H // 3] = torch.rand(B, 3, H // 3, W, generator=g) * 2.4 - 1.2     # a band of unrelated, out-of-range values
    return a.contiguous(), b.contiguous()


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("B,H,W", [(1, 64, 64), (3, 96, 160), (8, 320, 480), (4, 512, 512), (2, 1030, 1030)])
def test_quality_matches_the_restatement(B, H, W, masked):
    G = handle()
    a, b = pair(B, H, W, H + W + B)
    mask = (torch.rand(B, H, W, generator=torch.Generator().manual_seed(5)) > 0.25).float() if masked else None
    p, s = G.quality(a.cuda(), b.cuda(), mask.cuda() if masked else None)
    torch.cuda.synchronize()
    assert p.shape == s.shape == (B,) and p.is_cuda and p.dtype == torch.float32
    rp, rs = restated(a, b, mask)
    assert (p.cpu().double() - rp).abs().max() <= 1e-3, (p, rp)
    assert (s.cpu().double() - rs).abs().max() <= 1e-5, (s, rs)
    # identical inputs: exactly 80 dB and 1
    p, s = G.quality(a.cuda(), a.cuda(), mask.cuda() if masked else None)
    assert torch.all(p.cpu() == 80.0) and torch.all(s.cpu() == 1.0), (p, s)


@pytest.mark.parametrize("H,W", [(96, 160), (1030, 1030)])
def test_every_pixel_is_counted_once(H, W):
    """One differing pixel in each corner (outside the valid SSIM map) and, at 1030 (f = 4, 1030 = 4*257 + 2), in a row the
    floor pooling drops: the squared error is exactly 0.25 per differing value, so PSNR is known to the last bit of fp64."""
    G = handle()
    a = torch.zeros(1, 3, H, W)
    b = a.clone()
    pts = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)] + ([(H - 2, W // 2)] if H % 4 else [])
    for y, x in pts:
        b[0, :, y, x] = 1.0                                                    # 0.5 -> 1.0 after denormalising
    p, _ = G.quality(a.cuda(), b.cuda())
    want = -10 * np.log10(len(pts) * 3 * 0.25 / (3 * H * W) + 1e-8)
    rp, _ = restated(a, b)
    assert abs(float(rp) - want) < 1e-9
    assert abs(float(p.cpu()) - want) <= 1e-4, (float(p), want)               # one pixel more or less: ~1 dB


def test_results_are_deterministic_and_batch_independent():
    G = handle()
    a, b = pair(4, 512, 512, 9)
    mask = (torch.rand(4, 512, 512, generator=torch.Generator().manual_seed(2)) > 0.5).float().cuda()
    a, b = a.cuda(), b.cuda()
    p1, s1 = [t.clone() for t in G.quality(a, b, mask)]
    p2, s2 = G.quality(a, b, mask)
    assert torch.equal(p1, p2) and torch.equal(s1, s2)
    for k in range(4):
        pk, sk = G.quality(a[k:k + 1], b[k:k + 1], mask[k:k + 1])
        assert torch.equal(pk, p1[k:k + 1]) and torch.equal(sk, s1[k:k + 1]), k
    with pytest.raises(ValueError):
        G.quality(torch.zeros(1, 3, 8, 8, device="cuda"), torch.zeros(1, 3, 8, 8, device="cuda"))


@pytest.mark.parametrize("dtype,masked", [("f32", False), ("bf16", False), ("f32", True)])
def test_folder_metrics_end_to_end(tmp_path, dtype, masked):
    from PIL import Image
    from tests.test_driver import _write_example
    root = str(tmp_path)
    H = W = 128
    n = _write_example(root, n_key=3, rate=4, H=H, W=W)                   # 9 frames: two 3-frame segments -> one chain of batch 2
    rng = np.random.default_rng(4)
    os.makedirs(os.path.join(root, "gt", "clipA"))
    for i in range(n):
        Image.fromarray(rng.integers(0, 255, (H, W, 3), dtype=np.uint8)).save(os.path.join(root, "gt", "clipA", "g%03d.png" % i))
    mask_dir = os.path.join(root, "masks") if masked else None
    if masked:
        os.makedirs(os.path.join(mask_dir, "clipA"))
        for i in range(n):
            Image.fromarray(rng.integers(0, 255, (H, W), dtype=np.uint8)).save(os.path.join(mask_dir, "clipA", "m%03d.png" % i))
    G = handle(dtype)
    cfg = rib.AttrDict(gen=rib.hsm_gen_config(), model_height=H, model_width=W, gauss_sigma=5, skeleton_thres=0.001, foot_thres=0.001)
    dirs = [os.path.join(root, d) for d in ("inputs", "DAIN", "Predict_motion")]
    gt_dir = os.path.join(root, "gt")
    fuses = []
    chain = G.chain

    def recording_chain(*a, **k):
        out = chain(*a, **k)
        fuses.append(out[2].clone())
        return out

    G.chain = recording_chain
    try:
        E = ev.Evaluator(cfg, batch=2, chunk=0, lanes=1)
        out = os.path.join(root, "m")
        written = E.evaluate_from_folder(G, *dirs, out, gt_dir=gt_dir, metrics=True, mask_dir=mask_dir)
    finally:
        del G.chain
    assert len(written) == n and len(fuses) == 1 and fuses[0].shape == (3, 2, 3, H, W)
    with open(os.path.join(out, "metrics.json")) as f:
        rep = json.load(f)
    pf = rep["clips"]["clipA"]["per_frame"]
    assert [r["i"] for r in pf] == [1, 2, 3, 5, 6, 7]
    fz = fuses[0].cpu()
    for r in pf:
        i = r["i"]
        gt = E.load_image(os.path.join(gt_dir, "clipA", "g%03d.png" % i))[0].unsqueeze(0)
        dain = E.load_image(os.path.join(root, "DAIN", "clipA", "f%03d.png" % i))[0].unsqueeze(0)
        mk = None
        if masked:
            mk = torch.from_numpy((np.asarray(Image.open(os.path.join(mask_dir, "clipA", "m%03d.png" % i))) > 127).astype(np.float32)).unsqueeze(0)
        dp, ds = restated(dain, gt, mk)
        op, os_ = restated(fz[(i % 4) - 1, i // 4].unsqueeze(0), gt, mk)     # chain sample b = segment b, step t = frame offset
        assert abs(r["DAIN_PSNR"] - float(dp)) <= 1e-3 and abs(r["DAIN_SSIM"] - float(ds)) <= 1e-5, (r, float(dp), float(ds))
        assert abs(r["OURS_PSNR"] - float(op)) <= 1e-3 and abs(r["OURS_SSIM"] - float(os_)) <= 1e-5, (r, float(op), float(os_))
    # metrics=False: the same PNG bytes
    out2 = os.path.join(root, "plain")
    written2 = ev.Evaluator(cfg, batch=2, chunk=0, lanes=1).evaluate_from_folder(G, *dirs, out2, gt_dir=gt_dir)
    assert [os.path.relpath(w, out2) for w in written2] == [os.path.relpath(w, out) for w in written]
    for x, y in zip(written, written2):
        assert open(x, "rb").read() == open(y, "rb").read(), y
    assert not os.path.exists(os.path.join(out2, "metrics.json"))
