"""Inputs shared by tests/test_composite_cpu.py and tests/test_gpu_composite.py (no test lives here): the frames the source-size
composite is exercised with, made once per size pair, and the folder recipe of the driver tests (tests/test_driver.py's, with the
key frames and the DAIN frames at sizes of their own)."""
import json
import os

import numpy as np

from render_in_between_amd import resize

_IN = {}


def mask_steps():
    """Every k / 255 as float32 with its two float32 neighbours, and -0.0, 1.0, values below 0 and above 1."""
    steps = (np.arange(256) / 255.0).astype(np.float32)
    return np.concatenate([np.array([-0.0, 1.0, -0.1, -3.0, 1.0000001, 1.1, 7.0], np.float32), steps,
                           np.nextafter(steps, np.float32(-2)), np.nextafter(steps, np.float32(2))])


def inputs(H, W, H0, W0, n=2):
    """(pred float32 [n,3,H,W], mask float32 [n,1,H,W], bg uint8 [n,H0,W0,3]) of one size pair, made once.
    pred: frame 0 band-limited noise scaled to +-1.5 (both clamps act), frame 1 the quantiser's steps (k / 255 - 0.5) / 0.5 with
    their float neighbours, shuffled; mask: frame 0 uniform in [-0.1, 1.1] with a block of exact 0 and a block of exact 1, frame
    1 the k / 255 steps with their neighbours, shuffled; bg: frame 0 noise, frame 1 a 1-px checkerboard."""
    key = (H, W, H0, W0, n)
    if key in _IN:
        return _IN[key]
    rng = np.random.default_rng(H * 1000003 + W * 1009 + H0 * 31 + W0)
    pred = np.empty((n, 3, H, W), np.float32)
    mask = np.empty((n, 1, H, W), np.float32)
    bg = np.empty((n, H0, W0, 3), np.uint8)
    psteps = ((np.arange(256) / 255.0 - 0.5) / 0.5).astype(np.float32)
    pvals = np.concatenate([np.array([-1.0, 1.0, -0.0], np.float32), psteps, np.nextafter(psteps, np.float32(-2)), np.nextafter(psteps, np.float32(2))])
    yy, xx = np.mgrid[0:H0, 0:W0]
    for i in range(n):
        if i % 2 == 0:
            coarse = rng.normal(0, 1, (3, H // 4 + 2, W // 4 + 2))
            a = np.kron(coarse, np.ones((4, 4)))[:, 1:H + 1, 2:W + 2] + rng.normal(0, 0.1, (3, H, W))
            pred[i] = a / np.abs(a).max() * 1.5
            m = rng.uniform(-0.1, 1.1, (H, W))
            m[:max(1, H // 3), :max(1, W // 2)] = 0.0
            m[H - max(1, H // 3):, W - max(1, W // 2):] = 1.0
            mask[i, 0] = m
            bg[i] = rng.integers(0, 256, (H0, W0, 3), dtype=np.uint8)
        else:
            pred[i] = rng.permutation(np.resize(pvals, 3 * H * W)).reshape(3, H, W)
            mask[i, 0] = rng.permutation(np.resize(mask_steps(), H * W)).reshape(H, W)
            bg[i] = (((yy + xx) & 1) * 255).astype(np.uint8)[:, :, None]
    _IN[key] = (pred, mask, bg)
    return _IN[key]


def footprint_clear(zero, H0, W0):
    """zero: bool [H, W], True where the model-size mask is 0 -> bool [H0, W0]: True where all 16 taps of the output pixel's
    cubic footprint (resize._cubic_taps' clamped indices) lie in the zero region."""
    H, W = zero.shape
    ix, _ = resize._cubic_taps(W0, W)
    iy, _ = resize._cubic_taps(H0, H)
    ok = np.ones((H0, W0), bool)
    for j in range(4):
        for i in range(4):
            ok &= zero[iy[:, j][:, None], ix[:, i][None, :]]
    return ok


def write_example(root, n_key=2, rate=2, key_hw=(40, 48), dain_hw=(40, 48), clip="clipA", seed=0, odd=None):
    """tests/test_driver.py's folder recipe: inputs/ (key frames), DAIN/ (one frame per output frame), Predict_motion/ (one json
    per output frame; the keypoints in the key frames' pixels).  odd = (frame index, (h, w)): that DAIN frame has another size."""
    from PIL import Image
    rng = np.random.default_rng(seed)
    n = (n_key - 1) * rate + 1
    for d in ("inputs", "DAIN", "Predict_motion"):
        os.makedirs(os.path.join(root, d, clip))
    for k in range(n_key):
        Image.fromarray(rng.integers(0, 255, key_hw + (3,), dtype=np.uint8)).save(os.path.join(root, "inputs", clip, "%04d.png" % k))
    for i in range(n):
        hw = odd[1] if (odd is not None and odd[0] == i) else dain_hw
        Image.fromarray(rng.integers(0, 255, hw + (3,), dtype=np.uint8)).save(os.path.join(root, "DAIN", clip, "f%03d.png" % i))
        body = []
        for j in range(25):
            body += [float(rng.uniform(4, key_hw[1] - 4)), float(rng.uniform(4, key_hw[0] - 4)), 0.9]
        hand = [10.0, 10.0, 0.9] * 21
        with open(os.path.join(root, "Predict_motion", clip, "f%03d_keypoints.json" % i), "w") as f:
            json.dump({"people": [{"pose_keypoints_2d": body, "hand_left_keypoints_2d": hand, "hand_right_keypoints_2d": hand}]}, f)
    return n
