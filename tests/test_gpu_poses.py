"""Poses interpolated in the folder driver's process, on the MI355X: the bridge kernel (ribm_openpose, csrc/motion.hip) bit for
bit against its definition motion.pose_io.openpose_arrays, and the one command (`inference.py --poses keyframes`) against the
two commands it replaces (motion/inference.py, then inference.py on the folder that wrote), file for file and byte for byte.
Every comparison is exact."""
import ctypes as C
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

import render_in_between_amd as rib
from render_in_between_amd import evaluator as ev
from render_in_between_amd.motion import MotionSpec, model, pose_io, synth as msynth, _native
from tests.test_poses_cpu import GOLDEN, FolderMotion, definition, noisy_clip, random_clip, stage1

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_T = []


def transformer():
    """A motion transformer with the shipped pose statistics and no weights: the bridge needs none."""
    if not _T:
        ds = stage1().dataset
        _T.append(model.MotionTransformer(MotionSpec(), device="cuda:0").eval().set_pose_stats(ds.mean_pose, ds.std_pose))
    return _T[0]


def rules(conf):
    """Both branches of each of the reader's rules, frame by frame (i % 6): 1: the left hand's confidence 0, the right hand's
    above; 2: 3 valid body joints (no person); 3: 4 of them; 4: 3 above 0.1 and 12 at exactly 0.1 (no person); 5: all 0."""
    for i in range(conf.shape[2]):
        k = i % 6
        if k == 1:
            conf[17, 0, i] = 0.0
        elif k in (2, 3):
            conf[:15, 0, i] = 0.05; conf[:k + 1, 0, i] = 0.5
        elif k == 4:
            conf[:15, 0, i] = 0.1; conf[:3, 0, i] = 0.5
        elif k == 5:
            conf[:, 0, i] = 0.0
    return conf


def clips(N, L):
    """N clips of L frames: (motion fp32 [38][L], conf fp64 [19][1][L]) each, and the one (scale, offset) of the launch."""
    if (N, L) == (1, 9):            # golden folder a at rate 2, the network's output = the linear clip + noise
        m, c, scale, offset = noisy_clip(os.path.join(GOLDEN, "a"), 2, 52)
        return [(m, c)], scale, offset
    if (N, L) == (2, 17):           # golden folder b at rate 2 beside full-mantissa doubles under the rules
        m, c, scale, offset = noisy_clip(os.path.join(GOLDEN, "b"), 2, 92)
        m2, c2, _, _ = random_clip(17, 7)
        return [(m, c), (m2, rules(c2))], scale, offset
    m, c, scale, offset = random_clip(L, 8)       # (1, 5): a scale and an offset that are no powers of two
    return [(m, rules(c))], scale, offset


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def run_bridge(T, cl, scale, offset, out=None):
    joints = torch.from_numpy(np.stack([m.T for m, _ in cl], axis=1).copy()).cuda()                    # [L][N][38]
    conf = torch.from_numpy(np.stack([c[:, 0, :] for _, c in cl]).copy()).cuda()                       # [N][19][L]
    return T.openpose(joints, conf, scale, offset, out=out)


@pytest.mark.parametrize("N,L", [(1, 9), (2, 17), (1, 5)])
def test_bridge_kernel_is_bit_equal_to_its_definition(N, L):
    T = transformer()
    cl, scale, offset = clips(N, L)
    want = np.stack([definition(m, c, scale, offset) for m, c in cl])
    assert want.shape == (N, L, 19, 3)
    # the destination inside a larger buffer, at an offset that is no multiple of a frame, with guard doubles around it
    n = N * L * 19 * 3
    buf = torch.full((37 + n + 41,), 77.0, dtype=torch.float64, device="cuda")
    got = run_bridge(T, cl, scale, offset, out=buf[37:37 + n].view(N, L, 19, 3))
    host = buf.cpu().numpy()
    assert (host[:37] == 77.0).all() and (host[37 + n:] == 77.0).all()
    assert np.array_equal(bits(got.cpu().numpy()), bits(want)), np.argwhere(bits(got.cpu().numpy()) != bits(want))[:5]
    if L != 9:                      # the cases do reach both branches
        zero = ~want.reshape(N, L, -1).any(axis=2)
        assert zero.any() and not zero.all() and (want[~zero][:, 17] == 0).all(axis=1).any() and (want[..., 17:, :2] != 0).any()
    # a frame's values depend on neither N nor L: a clip alone, and its first frames alone, give the same bits
    m, c = cl[-1]
    alone = run_bridge(T, [(m, c)], scale, offset).cpu().numpy()
    assert np.array_equal(bits(alone[0]), bits(want[-1]))
    head = run_bridge(T, [(m[:, :3].copy(), c[:, :, :3].copy())], scale, offset).cpu().numpy()
    assert np.array_equal(bits(head[0]), bits(want[-1][:3]))


def test_bad_arguments_launch_nothing():
    T = transformer()
    L_ = _native.lib()
    cl, scale, offset = clips(1, 5)
    joints = torch.from_numpy(np.stack([m.T for m, _ in cl], axis=1).copy()).cuda()
    conf = torch.from_numpy(np.stack([c[:, 0, :] for _, c in cl]).copy()).cuda()
    out = torch.full((1, 5, 19, 3), 77.0, dtype=torch.float64, device="cuda")
    ok = [1, 5, joints.data_ptr(), conf.data_ptr(), scale, offset, out.data_ptr()]
    for i, bad in ((0, 0), (0, -1), (1, 0), (1, -3), (2, None), (3, None), (6, None), (0, 1 << 20)):
        args = list(ok)
        args[i] = bad
        if (i, bad) == (0, 1 << 20):
            args[1] = 1 << 10           # N * L beyond the supported 2^24 frames
        assert L_.ribm_openpose(T._h, *args, None) == -1, (i, bad)              # RIBM_ERR_INVALID
        assert b"ribm_openpose" in L_.ribm_last_error(T._h)
    assert L_.ribm_set_pose_stats(T._h, None, None) == -1 and b"ribm_set_pose_stats" in L_.ribm_last_error(T._h)
    # statistics never set: RIBM_ERR_STATE
    fresh = model.MotionTransformer(MotionSpec(), device="cuda:0")
    assert L_.ribm_openpose(fresh._h, *ok, None) == -3 and b"ribm_set_pose_stats" in L_.ribm_last_error(fresh._h)
    with pytest.raises(_native.RibmError):
        fresh.openpose(joints, conf, scale, offset, out=out)
    # a model whose clips are not the 38 OpenPose channels
    other = model.MotionTransformer(MotionSpec(input_joints=36), device="cuda:0")
    stats = np.ones((19, 2))
    assert L_.ribm_set_pose_stats(other._h, C.c_void_p(stats.ctypes.data), C.c_void_p(stats.ctypes.data)) == -1
    assert L_.ribm_openpose(other._h, *ok, None) == -1 and b"38" in L_.ribm_last_error(other._h)
    # the Python entry refuses what it would have to convert
    for j, c in ((joints.double(), conf), (joints, conf.float()), (joints.cpu(), conf), (joints[:, :, :36].contiguous(), conf),
                 (joints, conf[:, :18].contiguous()), (joints.transpose(0, 1), conf)):
        with pytest.raises(RuntimeError, match="openpose"):
            T.openpose(j, c, scale, offset)
    with pytest.raises(RuntimeError, match="statistics"):
        T.set_pose_stats(np.ones((18, 2)), np.ones((19, 2)))
    torch.cuda.synchronize()
    assert (out == 77.0).all()


def test_interpolate_clip_is_the_stand_alone_commands_folders(tmp_path):
    """ModelInference.interpolate_clip in this process against Evaluator.interpolate_openpose's folders read back: the arrays
    are the files', and save_dir writes the same bytes."""
    from render_in_between_amd import rasterise
    spec = MotionSpec()
    T = model.MotionTransformer(spec, device="cuda:0").eval()
    T.load_state_dict(msynth.make_state_dict(spec, 4))
    ds = pose_io.OpenPoseClips({})
    M = model.ModelInference(model.PositionEmbeddingSine1D(spec.pos_hidden_dim // 2, normalize=True), T, dataset=ds)
    E = pose_io.Evaluator({})
    E.set_model(model.ModelInference(model.PositionEmbeddingSine1D(spec.pos_hidden_dim // 2, normalize=True), T))
    src = os.path.join(GOLDEN, "a")
    two = {"pred_dir": str(tmp_path / "two" / "P"), "linear_dir": str(tmp_path / "two" / "L")}
    one = {"pred_dir": str(tmp_path / "one" / "P"), "linear_dir": str(tmp_path / "one" / "L")}
    E.interpolate_openpose(src, 4, two)
    pred, lin = M.interpolate_clip(src, 4, save_dir=one)
    assert pred.shape == lin.shape == (17, 19, 3) and pred.dtype == np.float64
    for arr, key in ((pred, "pred_dir"), (lin, "linear_dir")):
        names = sorted(os.listdir(two[key]))
        assert names == sorted(os.listdir(one[key])) and len(names) == 17
        want = np.stack([rasterise.read_json_keypoint(os.path.join(two[key], x)) for x in names])
        assert np.array_equal(bits(arr), bits(want)), key
        for x in names:
            assert open(os.path.join(two[key], x), "rb").read() == open(os.path.join(one[key], x), "rb").read(), (key, x)
    assert not np.array_equal(pred, lin)
    with pytest.raises(RuntimeError, match="dataset"):
        E.model.interpolate_clip(src, 4)


# ---- the folder driver ---------------------------------------------------------------------------------------------------------
H64 = W64 = 64


def cfg64():
    return rib.AttrDict(gen=rib.hsm_gen_config(), model_height=H64, model_width=W64, gauss_sigma=5, skeleton_thres=0.001, foot_thres=0.001)


def tree(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)


def test_default_path_and_rows_through_the_native_pipeline(tmp_path):
    """Without the new arguments the native driver writes the tree it wrote before they existed (the listing and names of
    tests/test_gpu_video.py's plain run); with a frame's row of the clip's array in place of its json path - through threads
    and through worker processes, DAIN names kept - the same bytes."""
    from tests.test_driver import _write_example
    from tests.test_gpu_quality import handle
    root = str(tmp_path)
    n = _write_example(root, n_key=3, rate=4, H=H64, W=W64)
    os.makedirs(os.path.join(root, "keys", "clipA"))
    for k in range(3):
        shutil.copy(os.path.join(root, "Predict_motion", "clipA", "f%03d_keypoints.json" % (4 * k)), os.path.join(root, "keys", "clipA", "%d.json" % k))
    G = handle()
    dirs = [os.path.join(root, d) for d in ("inputs", "DAIN", "Predict_motion")]

    def run(name, io_mode="thread", **kw):
        out = os.path.join(root, name)
        return out, ev.Evaluator(cfg64(), batch=2, chunk=2, lanes=1, io_mode=io_mode).evaluate_from_folder(G, *dirs, out, **kw)

    plain, plain_w = run("plain")
    assert tree(plain) == [os.path.join("clipA", "f%03d.png" % i) for i in range(n)] and n == 9
    assert [os.path.relpath(w, plain) for w in plain_w] == tree(plain)
    named, named_w = run("named", poses="folder")
    assert tree(named) == tree(plain)
    for io_mode in ("thread", "process"):
        fm = FolderMotion(root)
        dirs[2] = None
        try:
            out, w = run("rows_" + io_mode, io_mode, poses="keyframes", key_pose_dir=os.path.join(root, "keys"), upsample_rate=4, motion=fm)
        finally:
            dirs[2] = os.path.join(root, "Predict_motion")
        assert fm.calls == [("clipA", 4, None)] and tree(out) == tree(plain)
        for x in tree(plain):
            assert open(os.path.join(out, x), "rb").read() == open(os.path.join(plain, x), "rb").read() == open(os.path.join(named, x), "rb").read(), (io_mode, x)


def _key_json(rng, W, H):
    body = []
    for _ in range(25):
        body += [float(rng.uniform(8, W - 8)), float(rng.uniform(8, H - 8)), float(rng.uniform(0.5, 1.0))]
    hand = lambda: [v for _ in range(21) for v in (float(rng.uniform(8, W - 8)), float(rng.uniform(8, H - 8)), 0.8)]      # noqa: E731
    return {"version": 1.3, "people": [{"person_id": [-1], "pose_keypoints_2d": body, "hand_left_keypoints_2d": hand(), "hand_right_keypoints_2d": hand()}]}


def child(args, limit=240):
    """One command as a fresh child process under its own time limit."""
    r = subprocess.run([sys.executable] + args, capture_output=True, text=True, timeout=limit)
    assert r.returncode == 0, (args, r.stdout[-2000:], r.stderr[-4000:])
    return r


@pytest.fixture(scope="module")
def commands(tmp_path_factory):
    """Two clips (3 and 2 key frames) at 64x64, rate 4, seed-defined generator and motion weights, --background mci: the two
    commands as today into `two*`, the one command into `one*`."""
    import yaml
    from PIL import Image
    from render_in_between_amd import synth
    from tests.test_gpu_mci import scene
    root = str(tmp_path_factory.mktemp("poses"))
    rng = np.random.default_rng(11)
    big = scene(H64 + 40, W64 + 40, 9)
    for clip, n_key in (("clipA", 3), ("clipB", 2)):
        os.makedirs(os.path.join(root, "inputs", clip)); os.makedirs(os.path.join(root, "keys", clip))
        for k in range(n_key):
            Image.fromarray(big[20 + 3 * k:20 + 3 * k + H64, 30 - 5 * k:30 - 5 * k + W64].copy()).save(os.path.join(root, "inputs", clip, "%04d.png" % k))
            with open(os.path.join(root, "keys", clip, "%04d_keypoints.json" % k), "w") as f:
                json.dump(_key_json(rng, W64, H64), f)
    pkg = os.path.join(ROOT, "render-in-between_amd")
    gck, mck = os.path.join(root, "netG.pth"), os.path.join(root, "motion.pth")
    torch.save(synth.make_state_dict(rib.GenSpec.from_cfg(rib.hsm_gen_config()), 3), gck)
    torch.save(msynth.make_state_dict(MotionSpec(), 5), mck)
    g = yaml.load(open(os.path.join(pkg, "configs", "HSM.yaml")), Loader=yaml.FullLoader)
    g["model_pretrain_G"] = gck; g["model_height"] = H64; g["model_width"] = W64
    m = yaml.load(open(os.path.join(pkg, "configs", "motion.yaml")), Loader=yaml.FullLoader)
    m["model_pretrain"] = mck; m["openpose_scale"] = 32; m["openpose_offset"] = 32          # network units -> the 64 x 64 frame
    gcfg, mcfg = os.path.join(root, "g.yaml"), os.path.join(root, "m.yaml")
    yaml.dump(g, open(gcfg, "w")); yaml.dump(m, open(mcfg, "w"))
    stage1_cli, driver = os.path.join(pkg, "motion", "inference.py"), os.path.join(pkg, "inference.py")
    keys = os.path.join(root, "keys")
    # today: stage 1 writes <root>/Predict_motion and <root>/Linear_motion, then the driver reads <root>/Predict_motion
    child([stage1_cli, "--config", mcfg, "--pose-dir", keys, "--save-dir", root, "--upsample-rate", "4"])
    lin_root = os.path.join(root, "lin")             # the same input folder with Linear_motion as its pose folder
    os.makedirs(lin_root)
    os.symlink(os.path.join(root, "inputs"), os.path.join(lin_root, "inputs"))
    os.symlink(os.path.join(root, "Linear_motion"), os.path.join(lin_root, "Predict_motion"))
    base = [driver, "--config", gcfg, "--background", "mci"]
    one = ["--input-dir", root, "--pose-dir", keys, "--upsample-rate", "4", "--motion-config", mcfg]
    child(base + ["--input-dir", root, "--save-dir", os.path.join(root, "two")])
    child(base + one + ["--poses", "keyframes", "--save-dir", os.path.join(root, "one"), "--save-poses"])
    child(base + ["--input-dir", root, "--save-dir", os.path.join(root, "two_video"), "--video", "--frames", "none"])
    child(base + one + ["--poses", "keyframes", "--save-dir", os.path.join(root, "one_video"), "--video", "--frames", "none"])
    child(base + ["--input-dir", lin_root, "--save-dir", os.path.join(root, "two_lin")])
    child(base + one + ["--poses", "keyframes-linear", "--save-dir", os.path.join(root, "one_lin")])
    return root


def same_tree(a, b):
    assert tree(a) == tree(b) and tree(a), (tree(a), tree(b))
    for x in tree(a):
        assert open(os.path.join(a, x), "rb").read() == open(os.path.join(b, x), "rb").read(), x
    return tree(a)


def test_one_command_writes_the_two_commands_frames(commands):
    files = same_tree(os.path.join(commands, "two", "Generated_frames"), os.path.join(commands, "one", "Generated_frames"))
    assert files == [os.path.join("clipA", "%06d.png" % i) for i in range(9)] + [os.path.join("clipB", "%06d.png" % i) for i in range(5)]


def test_one_command_writes_the_two_commands_video(commands):
    files = same_tree(os.path.join(commands, "two_video", "Generated_frames"), os.path.join(commands, "one_video", "Generated_frames"))
    assert files == ["clipA_video.avi", "clipB_video.avi"]


def test_keyframes_linear_is_the_run_on_linear_motion(commands):
    files = same_tree(os.path.join(commands, "two_lin", "Generated_frames"), os.path.join(commands, "one_lin", "Generated_frames"))
    pred = os.path.join(commands, "one", "Generated_frames")
    # the frames do depend on which poses they were drawn from
    assert any(open(os.path.join(pred, x), "rb").read() != open(os.path.join(commands, "one_lin", "Generated_frames", x), "rb").read() for x in files)


def test_save_poses_writes_the_stand_alone_commands_json(commands):
    for folder in ("Predict_motion", "Linear_motion"):
        files = same_tree(os.path.join(commands, folder), os.path.join(commands, "one", folder))
        assert files == [os.path.join("clipA", "%06d_keypoints.json" % i) for i in range(9)] + [os.path.join("clipB", "%06d_keypoints.json" % i) for i in range(5)]
    # and only --save-poses writes them
    assert sorted(os.listdir(os.path.join(commands, "one_video"))) == ["Generated_frames"]
    assert sorted(os.listdir(os.path.join(commands, "one_lin"))) == ["Generated_frames"]
