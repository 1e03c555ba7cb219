"""The pose-derived human mask on the MI355X: rib_human_mask (csrc/human_mask.hip.h, Generator.human_mask) bit for bit
against the host statement rasterise.human_mask (tests/test_human_mask_cpu.py holds that one to an exact restatement), and the
folder driver's measurements under pose_mask=True end to end on the native path."""
import json
import os

import numpy as np
import pytest
import torch

import render_in_between_amd as rib
from render_in_between_amd import evaluator as ev, rasterise
from tests.test_gpu_quality import handle, restated as metric_restated
from tests.test_human_mask_cpu import CASES, frame_mask, golden_peaks, stick, write_person_poses

pytestmark = pytest.mark.gpu


def host(peaks, H, W):
    return torch.from_numpy(np.stack([rasterise.human_mask(p, H, W) for p in peaks]).astype(np.float32))


@pytest.mark.parametrize("name,peaks,H,W", CASES, ids=[c[0] for c in CASES])
def test_device_mask_equals_the_host_statement(name, peaks, H, W):
    G = handle()
    m = G.human_mask(peaks, H, W)
    assert m.shape == (1, H, W) and m.dtype == torch.float32 and m.is_cuda
    assert torch.equal(m.cpu(), host([peaks], H, W)), name


def scaled_poses(H, W):
    """The committed poses a-e stretched to H x W, the stick figure at three places (one partly outside: joints off) and an
    18-joint-like pose (the last joint off): 16 different poses of 19 joints."""
    out = []
    for n in "abcde":
        pk, h0, w0 = golden_peaks(n)
        q = pk.astype(np.int64)
        q = np.where(q[:, :1] >= 0, np.stack([q[:, 0] * W // w0, q[:, 1] * H // h0], 1), -1)
        out.append(q.astype(np.int32))
    s = min(H / 120.0, W / 96.0)
    for k, (fx, fy, f) in enumerate([(0.0, 0.0, 1.0), (0.5, 0.2, 0.5), (0.7, 0.6, 0.4), (0.05, 0.5, 0.45), (0.3, 0.3, 0.7), (0.62, 0.02, 0.37),
                                      (0.2, 0.55, 0.44), (0.45, 0.45, 0.55), (0.0, 0.3, 0.69), (0.8, 0.1, 0.2), (0.1, 0.1, 0.3)]):
        p = stick(19, ox=fx * W, oy=fy * H, s=s * f)
        off = (p[:, 0] >= W) | (p[:, 1] >= H)
        p[off] = -1
        if k % 4 == 3:
            p[18] = -1
        out.append(p)
    assert len(out) == 16
    return out


@pytest.mark.parametrize("H,W", [(320, 480), (512, 512), (1024, 1024), (67, 93), (130, 250)])
def test_batches_sizes_and_tails(H, W):
    """T = 1, 5 and 16 with a different pose per frame; W % 4 != 0 (scalar stores) and sizes that are no multiple of the 64 x 16
    tile; every frame of a batch equals its own T = 1 call (a frame's bytes do not depend on T)."""
    G = handle()
    poses = scaled_poses(H, W)
    want = host(poses, H, W)
    assert 0.02 < float(want.mean()) < 0.9
    for T in (1, 5, 16):
        m = G.human_mask(np.stack(poses[:T]), H, W)
        assert m.shape == (T, H, W)
        assert torch.equal(m.cpu(), want[:T]), (T, H, W)
    m16 = G.human_mask(np.stack(poses), H, W).cpu()
    for t in (0, 3, 4, 15):
        assert torch.equal(G.human_mask(poses[t], H, W).cpu()[0], m16[t]), t


def test_repeatable_written_everywhere_and_eighteen_joints():
    G = handle()
    H, W = 256, 320
    poses = np.stack(scaled_poses(H, W))
    a = G.human_mask(poses, H, W).clone()
    b = G.human_mask(poses, H, W)
    assert torch.equal(a, b)
    # every element is written: a destination full of NaN comes back as 0 / 1 only, and `out` is what is returned
    dst = torch.full((16, H, W), float("nan"), device="cuda")
    assert G.human_mask(poses, H, W, out=dst) is dst
    assert torch.equal(dst, a) and set(dst.unique().tolist()) == {0.0, 1.0}
    # 18 joints: the foot / hand-tip limbs are not drawn
    p18 = poses[5][:18]
    assert torch.equal(G.human_mask(p18, H, W).cpu(), host([p18], H, W))
    assert not torch.equal(G.human_mask(p18, H, W).cpu(), host([poses[5]], H, W))
    # a view at an address that is not 16-byte aligned takes the scalar stores
    buf = torch.zeros(16 * H * W + 1, device="cuda")
    odd = buf[1:].view(16, H, W)
    G.human_mask(poses, H, W, out=odd)
    assert torch.equal(odd, a)
    # the mask is what Generator.quality takes
    x = torch.rand(16, 3, H, W, device="cuda") * 2 - 1
    y = torch.rand(16, 3, H, W, device="cuda") * 2 - 1
    p, s = G.quality(x, y, a)
    rp, rs = metric_restated(x.cpu(), y.cpu(), a.cpu())
    assert (p.cpu().double() - rp).abs().max() <= 1e-3 and (s.cpu().double() - rs).abs().max() <= 1e-5


def test_bad_arguments_raise():
    G = handle()
    p = stick()
    with pytest.raises(ValueError):
        G.human_mask(p[:17], 128, 100)                           # 17 joints
    with pytest.raises(ValueError):
        G.human_mask(p.astype(np.float32), 128, 100)             # not the integer peak table
    with pytest.raises(ValueError):
        G.human_mask(p, 0, 100)
    with pytest.raises(ValueError):
        G.human_mask(p, 128, 16385)
    with pytest.raises(ValueError):
        G.human_mask(p, 100, 60)                                 # joints outside the frame
    with pytest.raises(ValueError):
        G.human_mask(p, 128, 100, out=torch.empty(1, 128, 100))  # destination on the host
    # the C ABI checks on its own
    from render_in_between_amd import _native
    dst = torch.empty(1, 128, 100, device="cuda")
    pk = np.ascontiguousarray(p, np.int32)
    L = _native.lib()
    for args in ((0, 128, 100, pk.ctypes.data, 19, dst.data_ptr()), (1, 128, 100, pk.ctypes.data, 17, dst.data_ptr()),
                 (1, 128, 16385, pk.ctypes.data, 19, dst.data_ptr()), (1, 128, 100, None, 19, dst.data_ptr()),
                 (1, 128, 100, pk.ctypes.data, 19, None), (1, 100, 60, pk.ctypes.data, 19, dst.data_ptr())):
        assert L.rib_human_mask(G._h, *args, None) == -1          # RIB_ERR_INVALID
        assert b"rib_human_mask" in L.rib_last_error(G._h)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_folder_metrics_under_the_pose_mask_end_to_end(tmp_path, dtype):
    from tests.test_driver import _write_example
    from PIL import Image
    root = str(tmp_path)
    H = W = 128
    n = _write_example(root, n_key=3, rate=4, H=H, W=W)                   # 9 frames: two 3-frame segments -> one chain of batch 2
    poses = write_person_poses(root, n, H, W)
    rng = np.random.default_rng(4)
    os.makedirs(os.path.join(root, "gt", "clipA"))
    for i in range(n):
        Image.fromarray(rng.integers(0, 255, (H, W, 3), dtype=np.uint8)).save(os.path.join(root, "gt", "clipA", "g%03d.png" % i))
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
        written = E.evaluate_from_folder(G, *dirs, out, gt_dir=gt_dir, metrics=True, pose_mask=True)
    finally:
        del G.chain
    assert len(written) == n and len(fuses) == 1 and fuses[0].shape == (3, 2, 3, H, W)
    with open(os.path.join(out, "metrics.json")) as f:
        rep = json.load(f)
    assert rep["protocol"]["mask"] == "pose: _generate_human_mask restated from OpenCV's drawing, unpinned"
    pf = rep["clips"]["clipA"]["per_frame"]
    assert [r["i"] for r in pf] == [1, 2, 3, 5, 6, 7]
    fz = fuses[0].cpu()
    for r in pf:
        i = r["i"]
        gt = E.load_image(os.path.join(gt_dir, "clipA", "g%03d.png" % i))[0].unsqueeze(0)
        dain = E.load_image(os.path.join(root, "DAIN", "clipA", "f%03d.png" % i))[0].unsqueeze(0)
        m = frame_mask(E, poses[i], H, W)
        assert m.mean() > 0.05, (i, m.mean())                              # a person is in the frame
        mk = torch.from_numpy(m).float().unsqueeze(0)
        dp, ds = metric_restated(dain, gt, mk)
        op, os_ = metric_restated(fz[(i % 4) - 1, i // 4].unsqueeze(0), gt, mk)     # chain sample b = segment b, step t = frame offset
        print("frame %d coverage %.3f DAIN %.6f/%.6f %.8f/%.8f OURS %.6f/%.6f %.8f/%.8f"
              % (i, m.mean(), r["DAIN_PSNR"], float(dp), r["DAIN_SSIM"], float(ds), r["OURS_PSNR"], float(op), r["OURS_SSIM"], float(os_)))
        assert abs(r["DAIN_PSNR"] - float(dp)) <= 1e-3 and abs(r["DAIN_SSIM"] - float(ds)) <= 1e-5, (r, float(dp), float(ds))
        assert abs(r["OURS_PSNR"] - float(op)) <= 1e-3 and abs(r["OURS_SSIM"] - float(os_)) <= 1e-5, (r, float(op), float(os_))
    # without metrics: the same PNG bytes
    out2 = os.path.join(root, "plain")
    written2 = ev.Evaluator(cfg, batch=2, chunk=0, lanes=1).evaluate_from_folder(G, *dirs, out2, gt_dir=gt_dir)
    assert [os.path.relpath(w, out2) for w in written2] == [os.path.relpath(w, out) for w in written]
    for x, y in zip(written, written2):
        assert open(x, "rb").read() == open(y, "rb").read(), y
    assert not os.path.exists(os.path.join(out2, "metrics.json"))
