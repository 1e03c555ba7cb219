"""The pose-derived human mask of the ground-truth metrics (no GPU): rasterise.human_mask - _generate_human_mask
(PGNR/datasets/HSM_auto_dataset.py:254-334) restated from OpenCV's drawing, unpinned - against an independent per-pixel
restatement in exact rational arithmetic written here, a float64 sandwich derived from the definition (everything within h of
a shape is set, nothing at h + 1 or beyond), and the folder driver / CLI surface of pose_mask on the reference-protocol path."""
import json
import math
import os

import numpy as np
import pytest
import torch

import render_in_between_amd as rib
from render_in_between_amd import _native, evaluator as ev, rasterise, synth
from oracle import generator_ref
from tests.test_driver import _write_example, oracle_labels
from tests.test_quality_cpu import _Model, _cfg, _inference_module, _write_gt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")

# the drawing of HSM_auto_dataset.py:263-275,291-292,300-325, written out once more: (a, b, thickness)
LIMBS_18 = [(0, 1, 30), (1, 2, 30), (2, 3, 30), (3, 4, 30), (1, 5, 30), (5, 6, 30), (6, 7, 30), (8, 9, 30), (9, 10, 30), (10, 11, 30),
            (8, 12, 30), (12, 13, 30), (13, 14, 30), (1, 8, 40), (2, 9, 40), (5, 12, 40)]
LIMBS_19 = LIMBS_18 + [(4, 18, 30), (7, 17, 30), (11, 16, 30), (14, 15, 30)]


def shapes_of(peaks):
    """[(A, B, r)] capsules of a pose: a joint disc is a capsule with A == B."""
    pk = [(int(x), int(y)) for x, y in peaks]
    out = [(p, p, 30 if i == 0 else 15) for i, p in enumerate(pk) if p[0] >= 0]
    for a, b, t in (LIMBS_19 if len(pk) == 19 else LIMBS_18):
        if pk[a][0] >= 0 and pk[b][0] >= 0:
            out.append((pk[a], pk[b], t // 2))
    return out


def restated(peaks, H, W):
    """Per pixel, python ints only: the squared distance from the pixel to the capsule's segment as an exact fraction num / den,
    set iff it is <= (r + 1/2)^2, i.e. 4 num <= (2r + 1)^2 den."""
    shapes = shapes_of(peaks)
    out = np.zeros((H, W), bool)
    for py in range(H):
        for px in range(W):
            for (ax, ay), (bx, by), r in shapes:
                if abs(px - (ax + bx) // 2) > abs(ax - bx) + r + 2 or abs(py - (ay + by) // 2) > abs(ay - by) + r + 2:
                    continue                                     # farther than r + 1 from the box of the segment: cannot be set
                dx, dy, vx, vy = bx - ax, by - ay, px - ax, py - ay
                L2, s = dx * dx + dy * dy, vx * dx + vy * dy
                if s <= 0:
                    num, den = vx * vx + vy * vy, 1              # before A (or A == B): distance to A
                elif s >= L2:
                    num, den = (px - bx) ** 2 + (py - by) ** 2, 1
                else:
                    num, den = (vx * vx + vy * vy) * L2 - s * s, L2   # |v|^2 - (v.d)^2 / |d|^2
                if 4 * num <= (2 * r + 1) ** 2 * den:
                    out[py, px] = True
                    break
    return out


def golden_peaks(name):
    g = np.load(os.path.join(GOLD, "raster_%s.npz" % name))
    H, W = g["skeleton"].shape[:2]
    return rasterise.peak_table(g["landmarks"], g["conf"], H, W), H, W


def stick(n=19, ox=0, oy=0, s=1.0):
    """A standing figure in a 96 x 120 box at (ox, oy), scaled by s: [n, 2] int peaks, every joint on."""
    base = [(48, 12), (48, 30), (34, 32), (26, 50), (22, 68), (62, 32), (70, 50), (74, 68), (48, 66), (40, 68), (38, 90), (36, 112),
            (56, 68), (58, 90), (60, 112), (66, 116), (30, 116), (78, 74), (18, 74)]
    return np.array([(int(ox + x * s), int(oy + y * s)) for x, y in base[:n]], np.int32)


def synthetic_cases():
    """(name, peaks, H, W): what the issue lists beyond the committed poses."""
    cases = []
    p = stick(); p[3] = (-1, -1); p[8] = (-1, -1)
    cases.append(("joint_off", p, 128, 100))                     # limbs (2,3)(3,4)(1,8)(8,9)(8,12) vanish
    p = stick(); p[2] = p[1]; p[10] = p[9]
    cases.append(("same_pixel", p, 128, 100))                    # A == B: discs only
    p = stick(); p[0] = (47, 0); p[1] = (47, 20); p[5] = (95, 32); p[6] = (95, 60); p[11] = (36, 119); p[16] = (0, 119)
    cases.append(("clipped", p, 120, 96))                        # joints on row 0, column W-1, row H-1, column 0
    p = np.full((19, 2), -1, np.int32)
    p[1], p[2], p[5], p[8] = (40, 40), (80, 40), (40, 90), (75, 75)   # horizontal (1,2), vertical (1,5), 45 degrees (1,8)
    cases.append(("axis_and_diagonal", p, 120, 110))
    p = np.full((19, 2), -1, np.int32)
    p[8], p[9], p[12] = (60, 50), (25, 15), (95, 15)             # the other diagonal, and a limb running right to left
    cases.append(("anti_diagonal", p, 90, 120))
    cases.append(("eighteen", stick(18), 128, 100))              # no foot / hand-tip limbs; joints 15-17 still get their discs
    cases.append(("nobody", np.full((19, 2), -1, np.int32), 40, 67))
    cases.append(("odd_size", stick(s=0.55), 67, 93))            # W % 4 != 0, not a multiple of any tile; every joint inside
    return cases


def all_cases():
    out = []
    for n in "abcde":
        pk, H, W = golden_peaks(n)
        out.append(("golden_" + n, pk, H, W))
    return out + synthetic_cases()


CASES = all_cases()


@pytest.mark.parametrize("name,peaks,H,W", CASES, ids=[c[0] for c in CASES])
def test_human_mask_equals_the_exact_restatement(name, peaks, H, W):
    got = rasterise.human_mask(peaks, H, W)
    assert got.shape == (H, W) and got.dtype == bool
    want = restated(peaks, H, W)
    assert np.array_equal(got, want), (name, int((got != want).sum()))


def capsule_distance(A, B, H, W):
    """float64 distance of every pixel centre to the segment A-B (a point when A == B)."""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    ax, ay, bx, by = (float(v) for v in (*A, *B))
    dx, dy = bx - ax, by - ay
    L2 = dx * dx + dy * dy
    t = np.clip(((xx - ax) * dx + (yy - ay) * dy) / L2, 0.0, 1.0) if L2 > 0 else np.zeros_like(xx)
    return np.hypot(xx - (ax + t * dx), yy - (ay + t * dy))


@pytest.mark.parametrize("name,peaks,H,W", CASES, ids=[c[0] for c in CASES])
def test_mask_lies_between_radius_h_and_h_plus_one(name, peaks, H, W):
    """Derived, not measured: the rule is 'within h + 1/2', so every pixel within h of a shape is set and no pixel at h + 1 or
    beyond of every shape is (the half pixel either side is the band OpenCV's boundary pixels live in: 'unpinned')."""
    got = rasterise.human_mask(peaks, H, W)
    outside = np.ones((H, W), bool)
    for A, B, r in shapes_of(peaks):
        d = capsule_distance(A, B, H, W)
        assert got[d <= r].all(), (name, A, B, r)
        outside &= d >= r + 1
    assert not got[outside].any(), name


def test_coverage_of_the_committed_poses():
    """The comparisons above cannot pass on empty masks: poses a-d hold a person (coverage 0.26, 0.26, 0.27, 0.77), e nobody."""
    for n in "abcd":
        pk, H, W = golden_peaks(n)
        cov = rasterise.human_mask(pk, H, W).mean()
        assert 0.05 <= cov <= 0.80, (n, cov)
    pk, H, W = golden_peaks("e")
    assert not rasterise.human_mask(pk, H, W).any()
    for name, pk, H, W in synthetic_cases():
        cov = rasterise.human_mask(pk, H, W).mean()
        assert (cov == 0) if name == "nobody" else (0.05 <= cov <= 0.95), (name, cov)


def test_limb_table_and_argument_checks():
    assert [tuple(l) for l in rasterise.mask_limbs(19)] == LIMBS_19 and [tuple(l) for l in rasterise.mask_limbs(18)] == LIMBS_18
    with pytest.raises(ValueError):
        rasterise.human_mask(np.zeros((17, 2), np.int32), 32, 32)
    with pytest.raises(ValueError):
        rasterise.human_mask(np.zeros((19, 3), np.int32), 32, 32)
    with pytest.raises(ValueError):
        rasterise.human_mask(stick(), 0, 32)
    with pytest.raises(ValueError):
        rasterise.human_mask(stick(), 32, 16385)
    # the off limbs of 'joint_off' really vanish: a pixel beside limb (3,4) is far from every shape left once joint 3 is off
    p = stick(); p[3] = (-1, -1)
    assert rasterise.human_mask(stick(), 128, 100)[52, 10] and not rasterise.human_mask(p, 128, 100)[52, 10]


def write_person_poses(root, n, H, W, clip="clipA", seed=5):
    """Replaces _write_example's poses (joints anywhere in the frame: their discs cover nearly all of a small frame) by a figure
    that fills about a third of it and moves from frame to frame.  -> the json paths."""
    rng = np.random.default_rng(seed)
    s = 0.45 * min(H / 120.0, W / 96.0)
    paths = []
    for i in range(n):
        pk = stick(19, ox=rng.uniform(2, W - 96 * s - 2), oy=rng.uniform(2, H - 120 * s - 2), s=s).astype(np.float64) + 0.25
        body = np.zeros((25, 3))
        for j, k in enumerate(list(range(15)) + [19, 22]):
            body[k] = (pk[j][0], pk[j][1], 0.9)
        hand = lambda c: [v for _ in range(21) for v in (float(c[0]), float(c[1]), 0.9)]      # noqa: E731
        doc = {"people": [{"pose_keypoints_2d": [float(v) for v in body.reshape(-1)],
                           "hand_left_keypoints_2d": hand(pk[17]), "hand_right_keypoints_2d": hand(pk[18])}]}
        paths.append(os.path.join(root, "Predict_motion", clip, "f%03d_keypoints.json" % i))
        assert os.path.exists(paths[-1])
        with open(paths[-1], "w") as f:
            json.dump(doc, f)
    return paths


def frame_mask(E, json_path, H, W):
    """rasterise.human_mask of one frame's pose, as the driver sees the pose (scaled with the W x H ground-truth frame)."""
    lm, conf = E.load_pose(json_path, (W, H))
    return rasterise.human_mask(rasterise.peak_table(lm, conf, H, W, E.skeleton_thres), H, W)


def test_folder_metrics_under_the_pose_mask(tmp_path):
    root = str(tmp_path)
    H, W = 64, 96
    n = _write_example(root, n_key=2, rate=4, H=H, W=W)        # frames 0..4: one segment 1..3
    _write_gt(root, n, H=H, W=W)
    poses = write_person_poses(root, n, H, W)
    cfg = _cfg(H, W)
    spec = rib.GenSpec.from_cfg(cfg.gen)
    R = generator_ref.RefGenerator(spec, synth.make_state_dict(spec, 2))
    dirs = [os.path.join(root, d) for d in ("inputs", "DAIN", "Predict_motion")]
    E = ev.Evaluator(cfg, label_fn=oracle_labels)
    M = _Model(R)
    out = os.path.join(root, "m")
    written = E.evaluate_from_folder(M, *dirs, out, gt_dir=os.path.join(root, "gt"), metrics=True, pose_mask=True)
    assert len(written) == n
    with open(os.path.join(out, "metrics.json")) as f:
        rep = json.load(f)
    assert rep["protocol"]["mask"] == "pose: _generate_human_mask restated from OpenCV's drawing, unpinned"
    pf = rep["clips"]["clipA"]["per_frame"]
    assert [r["i"] for r in pf] == [1, 2, 3] and sorted(pf[0]) == ["DAIN_PSNR", "DAIN_SSIM", "OURS_PSNR", "OURS_SSIM", "file", "i"]
    plain = ev.Evaluator(cfg, label_fn=oracle_labels)
    plain.evaluate_from_folder(_Model(R), *dirs, os.path.join(root, "u"), gt_dir=os.path.join(root, "gt"), metrics=True)
    assert plain.metrics_report["protocol"]["mask"] is None
    for t, r in enumerate(pf):
        i = r["i"]
        m = frame_mask(E, poses[i], H, W)
        assert 0.05 < m.mean() < 0.95, m.mean()                  # a person, not the whole frame: the mask changes the values
        mk = torch.from_numpy(m).float().unsqueeze(0)
        gt = E.load_image(os.path.join(root, "gt", "clipA", "g%03d.png" % i))[0].unsqueeze(0)
        dain = E.load_image(os.path.join(root, "DAIN", "clipA", "f%03d.png" % i))[0].unsqueeze(0)
        dp, ds = E.compute_metrics(dain, gt, mk)
        op, os_ = E.compute_metrics(M.fused[t], gt, mk)
        assert abs(r["DAIN_PSNR"] - float(dp)) <= 1e-4 and abs(r["DAIN_SSIM"] - float(ds)) <= 1e-6, (r, float(dp), float(ds))
        assert abs(r["OURS_PSNR"] - float(op)) <= 1e-4 and abs(r["OURS_SSIM"] - float(os_)) <= 1e-6, (r, float(op), float(os_))
        assert abs(r["DAIN_PSNR"] - plain.metrics[t]["DAIN_PSNR"]) > 0.1          # ... and not what the unmasked run reports
    # the files do not depend on the measurement
    for a, b in zip(written, sorted(os.listdir(os.path.join(root, "u", "clipA")))):
        assert open(a, "rb").read() == open(os.path.join(root, "u", "clipA", b), "rb").read()


def test_pose_mask_arguments_are_checked(tmp_path):
    root = str(tmp_path)
    n = _write_example(root, n_key=2, rate=2)
    _write_gt(root, n, masks=True)
    cfg = _cfg()
    spec = rib.GenSpec.from_cfg(cfg.gen)
    M = _Model(generator_ref.RefGenerator(spec, synth.make_state_dict(spec, 2)))
    dirs = [os.path.join(root, d) for d in ("inputs", "DAIN", "Predict_motion")]
    E = ev.Evaluator(cfg, label_fn=oracle_labels)
    with pytest.raises(ValueError, match="pose_mask is a setting of metrics=True"):
        E.evaluate_from_folder(M, *dirs, os.path.join(root, "a"), gt_dir=os.path.join(root, "gt"), pose_mask=True)
    with pytest.raises(ValueError, match="pose_mask and mask_dir"):
        E.evaluate_from_folder(M, *dirs, os.path.join(root, "b"), gt_dir=os.path.join(root, "gt"), metrics=True,
                               mask_dir=os.path.join(root, "masks"), pose_mask=True)
    assert not os.path.exists(os.path.join(root, "a")) and not os.path.exists(os.path.join(root, "b"))


def test_cli_pose_mask_flag():
    mod = _inference_module()
    o = mod.parse_args(["--input-dir", "x", "--gt-dir", "g", "--metrics", "--pose-mask"])
    assert o.metrics and o.pose_mask and o.mask_dir is None
    assert not mod.parse_args(["--input-dir", "x", "--gt-dir", "g", "--metrics"]).pose_mask
    with pytest.raises(SystemExit):
        mod.parse_args(["--input-dir", "x", "--gt-dir", "g", "--pose-mask"])
    with pytest.raises(SystemExit):
        mod.parse_args(["--input-dir", "x", "--gt-dir", "g", "--metrics", "--pose-mask", "--mask-dir", "m"])


def test_abi_declares_binds_and_exports_the_entry():
    hdr = open(os.path.join(ROOT, "include", "rib.h")).read()
    assert "int rib_human_mask(rib_handle* h, int T, int H, int W, const int32_t* peaks, int n_joints," in hdr
    assert "HSM_auto_dataset.py:254-334" in hdr and "unpinned" in hdr[hdr.index("pose mask"):hdr.index("int rib_human_mask(")]
    assert len(_native.SIGNATURES["rib_human_mask"][1]) == 8
    from tests.test_native_host import _build_module
    assert any(os.path.basename(d) == "human_mask.hip.h" for d in _build_module().DEPS)
    if os.path.exists(_native.LIB_PATH):
        import subprocess
        out = subprocess.run(["nm", "-D", "--defined-only", _native.LIB_PATH], capture_output=True, text=True, check=True).stdout
        assert any(l.split()[-1] == "rib_human_mask" for l in out.splitlines())
    assert math.isfinite(rasterise.MASK_MAX_SIDE) and rasterise.MASK_MAX_SIDE == 16384
