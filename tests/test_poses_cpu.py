"""Poses interpolated in the folder driver's process (evaluate_from_folder(poses="keyframes")), the host side.

motion.pose_io.openpose_arrays is the definition of the keypoints a clip's frames are drawn from when no json file is written
between the two stages; here it is held, exactly (np.array_equal on fp64), to the real round trip of the two commands:
Evaluator._post_process -> motion2openpose into a folder -> rasterise.read_json_keypoint of every file.  Then the driver's
plumbing: a frame's row of the clip's array in place of its json path gives the same files, and every refusal."""
import json
import os
import shutil

import numpy as np
import pytest
import torch

import render_in_between_amd as rib
from render_in_between_amd import evaluator as ev, io_worker, rasterise
from render_in_between_amd.motion import pose_io

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "motion_json")
_E = []


def stage1():
    """pose_io.Evaluator with the shipped pose statistics (no model: the network's output is supplied by the cases)."""
    if not _E:
        _E.append(pose_io.Evaluator({}))
    return _E[0]


def round_trip(motion, conf, scale, offset, folder):
    """What the two commands do: motion fp32 [38][L] as the network's output -> json files -> the driver's reader."""
    E = stage1()
    world = E._post_process(torch.from_numpy(motion).unsqueeze(0))
    pose_io.motion2openpose(world, conf, folder, scale=scale, offset=offset)
    names = sorted(os.listdir(folder))
    assert names == ["%06d_keypoints.json" % i for i in range(motion.shape[1])]
    return np.stack([rasterise.read_json_keypoint(os.path.join(folder, x)) for x in names])


def definition(motion, conf, scale, offset):
    ds = stage1().dataset
    return pose_io.openpose_arrays(motion, conf, scale, offset, ds.mean_pose, ds.std_pose)


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype == np.float64 and np.array_equal(a, b) and np.array_equal(np.signbit(a), np.signbit(b))


def noisy_clip(json_dir, rate, seed):
    """The clip stage 1 makes of a key-frame folder, the network's output replaced by the linear clip plus seeded fp32 noise."""
    (scale, offset, conf), _, interp, _, _ = stage1().dataset.get_openpose_data(json_dir, rate)
    rng = np.random.default_rng(seed)
    motion = (interp.numpy() + rng.normal(0, 0.05, tuple(interp.shape)).astype(np.float32)).astype(np.float32)
    return motion, conf, scale, offset


def random_clip(L, seed):
    """Random doubles with full mantissas everywhere: fp32 motion times fp64 statistics, a scale and an offset that are no
    powers of two, random confidences."""
    rng = np.random.default_rng(seed)
    return rng.standard_normal((38, L)).astype(np.float32), rng.uniform(0.2, 1.0, (19, 1, L)), float(rng.uniform(300, 900)), float(rng.uniform(10, 300))


@pytest.mark.parametrize("rate", [2, 4])
@pytest.mark.parametrize("clip,n_key", [("a", 5), ("b", 9)])
def test_definition_equals_the_json_round_trip_of_the_golden_folders(tmp_path, clip, n_key, rate):
    motion, conf, scale, offset = noisy_clip(os.path.join(GOLDEN, clip), rate, n_key * 10 + rate)
    L = (n_key - 1) * rate + 1
    assert motion.shape == (38, L) and conf.shape == (19, 1, L) and motion.dtype == np.float32
    got = definition(motion, conf, scale, offset)
    assert got.shape == (L, 19, 3) and np.abs(got).max() > 0
    assert same(got, round_trip(motion, conf, scale, offset, str(tmp_path / "json")))
    # and of the linear clip itself, what Linear_motion holds
    lin = stage1().dataset.get_openpose_data(os.path.join(GOLDEN, clip), rate)[2].numpy()
    assert same(definition(lin, conf, scale, offset), round_trip(lin, conf, scale, offset, str(tmp_path / "lin")))


def test_full_mantissas_show_the_order_of_the_21_term_sum(tmp_path):
    motion, conf, scale, offset = random_clip(9, 5)
    got = definition(motion, conf, scale, offset)
    assert same(got, round_trip(motion, conf, scale, offset, str(tmp_path / "json")))
    # the hands are means of 21 copies: a running sum / 21, which is not always the double that was copied
    ds = stage1().dataset
    world = pose_io.post_process(motion, ds.mean_pose, ds.std_pose) * scale + offset          # [19][2][L]
    plain = world[17:].transpose(2, 0, 1)                                                      # [L][2][2]
    assert np.allclose(got[:, 17:, :2], plain, rtol=1e-14, atol=0) and (got[:, 17:, :2] != plain).any()
    assert np.array_equal(got[:, :17, :2], world[:17].transpose(2, 0, 1))                      # the body joints are the doubles themselves
    x = plain[..., 0].ravel()
    s = x.copy()
    for _ in range(20):
        s = s + x
    assert np.array_equal(got[:, 17:, 0].ravel(), s / 21)                                      # in row order, one addition per copy


def test_the_readers_rules_both_ways(tmp_path):
    """Frame 1: the left hand's confidence is 0 (a zero row), the right hand's is not; frame 2: 3 body joints above 0.1 (no
    person: all zeros), frame 3: 4 of them; frame 4: confidences of exactly 0.1 do not count (3 above + 12 at 0.1: no person);
    frame 5: every confidence 0 - the reader finds no person; frame 6: a toe and a hand above 0.1 do not count as body joints."""
    motion, conf, scale, offset = random_clip(8, 6)
    conf[17, 0, 1] = 0.0
    conf[:15, 0, 2] = 0.05; conf[:3, 0, 2] = 0.5
    conf[:15, 0, 3] = 0.05; conf[:4, 0, 3] = 0.5
    conf[:15, 0, 4] = 0.1; conf[:3, 0, 4] = 0.5
    conf[:, 0, 5] = 0.0
    conf[:15, 0, 6] = 0.05; conf[:3, 0, 6] = 0.5
    got = definition(motion, conf, scale, offset)
    assert same(got, round_trip(motion, conf, scale, offset, str(tmp_path / "json")))
    assert not got[1, 17].any() and got[1, 18].all() and got[1, :17].all()
    assert not got[2].any() and got[3, :, :2].all() and not got[4].any() and not got[5].any() and not got[6].any()
    assert got[0].all() and got[7].all()


def test_a_key_frame_without_a_person(tmp_path):
    """The first key frame's json has no person: stage 1 gives that frame zero confidences, the frames next to it halves."""
    src = str(tmp_path / "keys")
    shutil.copytree(os.path.join(GOLDEN, "a"), src)
    with open(os.path.join(src, "000000_keypoints.json"), "w") as f:
        json.dump({"version": 1.3, "people": []}, f)
    motion, conf, scale, offset = noisy_clip(src, 2, 3)
    assert not conf[:, 0, 0].any() and conf[:, 0, 1].any()
    got = definition(motion, conf, scale, offset)
    assert same(got, round_trip(motion, conf, scale, offset, str(tmp_path / "json")))
    assert not got[0].any() and got[2].any()


def test_bad_arrays_are_refused():
    motion, conf, scale, offset = random_clip(3, 1)
    for m, c in ((motion.astype(np.float64), conf), (motion[:36], conf), (motion, conf[:, 0]), (motion, conf[:, :, :2])):
        with pytest.raises(ValueError, match="openpose_arrays"):
            definition(m, c, scale, offset)


# ---- the driver ----------------------------------------------------------------------------------------------------------------
def test_scaled_pose_takes_the_array_the_reader_returns(tmp_path):
    path = os.path.join(GOLDEN, "a", "000002_keypoints.json")
    pose = rasterise.read_json_keypoint(path)
    assert io_worker.scaled_pose(path, (640, 360), 48, 32) == io_worker.scaled_pose(pose, (640, 360), 48, 32) == io_worker.scale_pose(pose, (640, 360), 48, 32)


class FolderMotion:
    """Stands in for motion.model.ModelInference: the clip's arrays are read from the folders stage 1's command would have
    written, so that the driver's two ways to a frame's pose can be compared without a GPU."""

    def __init__(self, root):
        self.root, self.calls = root, []

    def interpolate_clip(self, json_dir, sample_rate, save_dir=None):
        sub = os.path.basename(json_dir)
        self.calls.append((sub, sample_rate, save_dir))
        rows = np.stack([rasterise.read_json_keypoint(os.path.join(self.root, "Predict_motion", sub, x))
                         for x in sorted(os.listdir(os.path.join(self.root, "Predict_motion", sub)))])
        return rows, rows[::-1].copy()


class Model:
    """The reference's call protocol: the frame is a function of its label maps and background."""

    def eval(self):
        return self

    def __call__(self, label, label_prev, dain, prev):
        return (0.5 * dain + 0.25 * label[:, :3] + 0.25 * prev).clamp(-1, 1), label[:, 3:4].clamp(0, 1)


def _example(root, n_key=3, rate=2):
    from tests.test_driver import _write_example
    n = _write_example(root, n_key=n_key, rate=rate)
    os.makedirs(os.path.join(root, "keys", "clipA"))
    for k in range(n_key):
        shutil.copy(os.path.join(root, "Predict_motion", "clipA", "f%03d_keypoints.json" % (k * rate)), os.path.join(root, "keys", "clipA", "%04d_keypoints.json" % k))
    return n


def _cfg():
    return rib.AttrDict(gen=rib.hsm_gen_config(), model_height=32, model_width=48, gauss_sigma=5, skeleton_thres=0.001, foot_thres=0.001)


def test_rows_in_place_of_json_paths_give_the_same_files(tmp_path):
    from tests.test_driver import oracle_labels
    root = str(tmp_path)
    n = _example(root)
    inputs, dain, poses, keys = (os.path.join(root, d) for d in ("inputs", "DAIN", "Predict_motion", "keys"))
    E = ev.Evaluator(_cfg(), label_fn=oracle_labels)
    a = E.evaluate_from_folder(Model(), inputs, dain, poses, os.path.join(root, "a"))
    fm = FolderMotion(root)
    b = E.evaluate_from_folder(Model(), inputs, dain, None, os.path.join(root, "b"), poses="keyframes", key_pose_dir=keys, upsample_rate=2, motion=fm)
    assert fm.calls == [("clipA", 2, None)]
    assert [os.path.relpath(x, os.path.join(root, "a")) for x in a] == [os.path.relpath(x, os.path.join(root, "b")) for x in b] and len(b) == n == 5
    for x, y in zip(a, b):
        assert open(x, "rb").read() == open(y, "rb").read(), x
    # keyframes-linear takes the second array (here: the clip reversed, so the generated frames differ)
    c = E.evaluate_from_folder(Model(), inputs, dain, None, os.path.join(root, "c"), poses="keyframes-linear", key_pose_dir=keys, upsample_rate=2, motion=fm)
    assert any(open(x, "rb").read() != open(y, "rb").read() for x, y in zip(a, c))
    # save_poses hands stage 1 the two folders beside save_dir
    out = os.path.join(root, "run", "Generated_frames")
    E.evaluate_from_folder(Model(), inputs, dain, None, out, poses="keyframes", key_pose_dir=keys, upsample_rate=2, motion=fm, save_poses=True)
    assert fm.calls[-1] == ("clipA", 2, {"pred_dir": os.path.join(root, "run", "Predict_motion", "clipA"),
                                        "linear_dir": os.path.join(root, "run", "Linear_motion", "clipA")})


def test_the_drivers_refusals(tmp_path):
    root = str(tmp_path)
    _example(root)
    inputs, dain, poses, keys = (os.path.join(root, d) for d in ("inputs", "DAIN", "Predict_motion", "keys"))
    E = ev.Evaluator(_cfg())
    fm = FolderMotion(root)

    def call(**kw):
        return E.evaluate_from_folder(Model(), inputs, dain, poses, os.path.join(root, "out"), **kw)

    for kw in (dict(key_pose_dir=keys), dict(upsample_rate=4), dict(save_poses=True), dict(motion=fm)):
        with pytest.raises(ValueError, match="settings of poses="):
            call(**kw)
    with pytest.raises(ValueError, match="poses must be"):
        call(poses="json")
    with pytest.raises(ValueError, match="needs key_pose_dir"):
        call(poses="keyframes", motion=fm)
    with pytest.raises(ValueError, match="needs key_pose_dir"):
        call(poses="keyframes-linear", motion=fm)
    with pytest.raises(ValueError, match="needs motion="):
        call(poses="keyframes", key_pose_dir=keys)
    for rate in (3, 0, 6, 2.0):
        with pytest.raises(ValueError, match="power of two"):
            call(poses="keyframes", key_pose_dir=keys, motion=fm, upsample_rate=rate)
    # a clip whose key-pose files and key frames differ in number: named, with both counts, before stage 1 runs
    os.remove(os.path.join(keys, "clipA", "0002_keypoints.json"))
    with pytest.raises(ValueError, match="clip clipA has 2 key-pose files and 3 key frames"):
        call(poses="keyframes", key_pose_dir=keys, motion=fm, upsample_rate=2)
    assert fm.calls == [] and not os.path.exists(os.path.join(root, "Predict_motion_written"))


def test_the_command_lines_refusals_and_what_it_passes_on(monkeypatch):
    from render_in_between_amd import inference
    o = inference.parse_args(["--input-dir", "x"])
    assert o.poses == "folder" and o.pose_dir is None and o.upsample_rate is None and o.motion_config is None and not o.save_poses
    o = inference.parse_args(["--input-dir", "x", "--poses", "keyframes", "--pose-dir", "p", "--upsample-rate", "4", "--motion-config", "m.yaml", "--save-poses"])
    assert (o.poses, o.pose_dir, o.upsample_rate, o.motion_config, o.save_poses) == ("keyframes", "p", 4, "m.yaml", True)
    assert inference.parse_args(["--input-dir", "x", "--poses", "keyframes-linear", "--pose-dir", "p"]).upsample_rate is None
    for bad in (["--pose-dir", "p"], ["--upsample-rate", "4"], ["--save-poses"], ["--motion-config", "m.yaml"], ["--poses", "keyframes"],
                ["--poses", "keyframes-linear"], ["--poses", "linear", "--pose-dir", "p"], ["--poses", "keyframes", "--pose-dir", "p", "--upsample-rate", "6"],
                ["--poses", "keyframes", "--pose-dir", "p", "--upsample-rate", "0"]):
        with pytest.raises(SystemExit):
            inference.parse_args(["--input-dir", "x"] + bad)
    # main: the default call passes none of the new arguments; a keyframes call loads stage 1 and lists no Predict_motion folder
    seen = []
    monkeypatch.setattr(inference, "load_generator", lambda *a, **k: object())
    monkeypatch.setattr(inference, "load_motion", lambda path, device=None: ("motion", path))
    monkeypatch.setattr(inference.rib, "get_config", lambda path: inference.rib.AttrDict(model_height=32, model_width=48, gauss_sigma=5,
                                                                                         skeleton_thres=0.001, foot_thres=0.001))
    monkeypatch.setattr(inference.Evaluator, "evaluate_from_folder", lambda self, model, *dirs, **kw: seen.append((dirs, kw)) or [])
    inference.main(inference.parse_args(["--input-dir", "x"]))
    dirs, kw = seen[-1]
    assert dirs[2] == os.path.join("x", "Predict_motion") and not {"poses", "key_pose_dir", "upsample_rate", "motion", "save_poses"} & set(kw)
    inference.main(inference.parse_args(["--input-dir", "x", "--poses", "keyframes", "--pose-dir", "p", "--background", "mci"]))
    dirs, kw = seen[-1]
    assert dirs[1] is None and dirs[2] is None
    assert (kw["poses"], kw["key_pose_dir"], kw["upsample_rate"], kw["save_poses"]) == ("keyframes", "p", 8, False)
    assert kw["motion"] == ("motion", os.path.join(os.path.dirname(inference.__file__), "configs", "motion.yaml"))
