"""The folder driver's frame resize on the MI355X: rib_resize_cubic (csrc/resize.hip.h, Generator.resize_u8) against the host
function it replaces (resize.resize_cubic_u8) and the scalar oracle (oracle/resize_ref), bit for bit, and the folder driver
with resize_on="gpu" against resize_on="host" end to end (byte-identical files).  Every comparison is exact."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import render_in_between_amd as rib
from render_in_between_amd import evaluator as ev, resize, synth
from oracle import resize_ref

pytestmark = pytest.mark.gpu

_G = {}

# (H0, W0) -> (H, W); the scalar oracle is run on the small ones only
SMALL = [((45, 80), (32, 48)), ((32, 48), (45, 80)), ((37, 53), (64, 96)), ((120, 67), (32, 32)), ((16, 16), (64, 48)),
         ((5, 7), (32, 48)), ((1, 9), (16, 16)), ((90, 160), (32, 48))]
LARGE = [((1080, 1920), (512, 512)), ((720, 1280), (320, 480))]


def handle():
    if "g" not in _G:
        cfg = rib.hsm_gen_config()
        G = rib.Generator(cfg).eval()
        G.load_state_dict(synth.make_state_dict(rib.GenSpec.from_cfg(cfg), 0))
        _G["g"] = G
    return _G["g"]


def frames(kind, n, h0, w0, seed):
    rng = np.random.default_rng(seed)
    if kind == "uniform":
        return rng.integers(0, 256, (n, h0, w0, 3), dtype=np.uint8)
    return (rng.integers(0, 2, (n, h0, w0, 3), dtype=np.uint8) * 255).astype(np.uint8)       # only 0 / 255: overshoot, saturation


def torch_normalise(u8_nhwc):
    """The upload's ToTensor + Normalize(0.5, 0.5), by torch on the tensor's own device."""
    return ((u8_nhwc.permute(0, 3, 1, 2).float() / 255.0 - 0.5) / 0.5).contiguous()


@pytest.mark.parametrize("kind", ["uniform", "binary"])
@pytest.mark.parametrize("src,dst", SMALL + LARGE)
def test_resize_equals_the_host_function(src, dst, kind):
    (h0, w0), (h, w) = src, dst
    G = handle()
    a = frames(kind, 2, h0, w0, h0 * 7 + w0 + h)
    got = G.resize_u8(torch.from_numpy(a).cuda(), w, h)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (2, h, w, 3)
    got = got.cpu().numpy()
    for k in range(2):
        assert np.array_equal(got[k], resize.resize_cubic_u8(a[k], w, h)), (src, dst, kind, k)
        if (src, dst) in SMALL:
            assert np.array_equal(got[k], resize_ref.resize_cubic_u8(a[k], w, h)), (src, dst, kind, k)


def test_frames_do_not_depend_on_the_batch_or_the_run():
    G = handle()
    a = torch.from_numpy(frames("uniform", 5, 90, 160, 3)).cuda()
    five = G.resize_u8(a, 48, 32)
    again = G.resize_u8(a, 48, 32)
    assert torch.equal(five, again)
    for k in range(5):
        one = G.resize_u8(a[k:k + 1], 48, 32)
        assert torch.equal(one, five[k:k + 1]), k
        assert torch.equal(G.resize_u8(a[k], 48, 32), five[k])            # [H0,W0,3] in, [H,W,3] out
    fn = G.resize_u8(a, 48, 32, normalised=True)
    assert torch.equal(fn, G.resize_u8(a, 48, 32, normalised=True))
    assert torch.equal(G.resize_u8(a[2:3], 48, 32, normalised=True), fn[2:3])


@pytest.mark.parametrize("value", [0, 1, 127, 254, 255])
def test_constant_frames_stay_constant(value):
    G = handle()
    a = torch.full((2, 37, 53, 3), value, dtype=torch.uint8, device="cuda")
    for (w, h) in ((96, 64), (20, 11), (53, 37)):
        out = G.resize_u8(a, w, h)
        assert tuple(out.shape) == (2, h, w, 3) and bool((out == value).all()), (value, w, h)


def test_same_size_input_is_returned_unchanged():
    G = handle()
    a = torch.from_numpy(frames("uniform", 3, 32, 48, 9)).cuda()
    out = G.resize_u8(a, 48, 32)
    assert torch.equal(out, a) and out.data_ptr() != a.data_ptr()          # a copy, as the host function returns
    assert torch.equal(G.resize_u8(a, 48, 32, normalised=True), torch_normalise(a))


def test_normalised_output_is_torchs_expression_bit_for_bit():
    G = handle()
    # every uint8 value, through the same-size path
    ramp = torch.arange(256, dtype=torch.uint8, device="cuda").repeat_interleave(3).reshape(1, 16, 16, 3).contiguous()
    got = G.resize_u8(ramp, 16, 16, normalised=True)
    want = torch_normalise(ramp)
    assert got.dtype == torch.float32 and tuple(got.shape) == (1, 3, 16, 16)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32)), \
        [int(v) for v in ramp.permute(0, 3, 1, 2)[got.view(torch.int32) != want.view(torch.int32)].unique()]
    for (h0, w0), (h, w) in SMALL + LARGE[:1]:
        for kind in ("uniform", "binary"):
            a = torch.from_numpy(frames(kind, 2, h0, w0, h0 + w0)).cuda()
            u8 = G.resize_u8(a, w, h)
            fn = G.resize_u8(a, w, h, normalised=True)
            assert tuple(fn.shape) == (2, 3, h, w)
            assert torch.equal(fn.view(torch.int32), torch_normalise(u8).view(torch.int32)), ((h0, w0), (h, w), kind)
    out = torch.empty((2, 3, h, w), dtype=torch.float32, device="cuda")
    assert G.resize_u8(a, w, h, normalised=True, out=out) is out and torch.equal(out, fn)


def test_invalid_arguments_are_refused():
    from render_in_between_amd import _native
    G = handle()
    a = torch.zeros((1, 8, 8, 3), dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError):
        G.resize_u8(torch.zeros((1, 8, 8, 3), dtype=torch.uint8), 4, 4)           # a CPU tensor
    with pytest.raises(ValueError):
        G.resize_u8(a.float(), 4, 4)
    with pytest.raises(ValueError):
        G.resize_u8(torch.zeros((1, 8, 8, 4), dtype=torch.uint8, device="cuda"), 4, 4)   # not 3 channels
    with pytest.raises(ValueError):
        G.resize_u8(a, 0, 4)
    with pytest.raises(ValueError):
        G.resize_u8(a, 4, 4, out=torch.empty((1, 4, 4, 3), dtype=torch.float32, device="cuda"))
    # the C ABI itself: nothing is launched for any of these
    L = _native.lib()
    tab = torch.zeros(64, dtype=torch.int32, device="cuda")
    out = torch.zeros((1, 4, 4, 3), dtype=torch.uint8, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)      # noqa: E731
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(N=1, H0=8, W0=8, H=4, W=4, src=a, t=tab, o8=out, o32=None):
        return L.rib_resize_cubic(G._h, N, H0, W0, H, W, p(src), p(t), p(t), p(t), p(t), p(o8), p(o32), st)
    assert call() == 0
    assert call(o8=None, o32=None) == -1                    # RIB_ERR_INVALID: both outputs NULL
    assert call(src=None) == -1 and call(t=None) == -1
    for bad in (dict(N=0), dict(H0=0), dict(W0=-1), dict(H=0), dict(W=0)):
        assert call(**bad) == -1, bad
    assert b"rib_resize_cubic" in L.rib_last_error(G._h)
    torch.cuda.synchronize()


# ---- the folder driver, end to end --------------------------------------------------------------------------------------------
def _example(root, H, W, dain_sizes, gt_size=None, n_key=3, rate=4, clip="clipA", seed=0):
    """tests/test_driver._write_example's tree with the DAIN frames (and optional GT frames) at sizes of their own:
    dain_sizes[i % len] = (h, w) of DAIN frame i."""
    from PIL import Image
    from tests.test_driver import _write_example
    n = _write_example(root, n_key=n_key, rate=rate, H=H, W=W, clip=clip, seed=seed)
    rng = np.random.default_rng(seed + 11)
    for i in range(n):
        h, w = dain_sizes[i % len(dain_sizes)]
        Image.fromarray(rng.integers(0, 255, (h, w, 3), dtype=np.uint8)).save(os.path.join(root, "DAIN", clip, "f%03d.png" % i))
    if gt_size is not None:
        os.makedirs(os.path.join(root, "gt", clip))
        for i in range(n):
            Image.fromarray(rng.integers(0, 255, (gt_size[0], gt_size[1], 3), dtype=np.uint8)).save(os.path.join(root, "gt", clip, "g%03d.png" % i))
    return n


def _run_both(root, H, W, metrics=False, io_mode="process", capsys=None):
    G = handle()
    cfg = rib.AttrDict(gen=rib.hsm_gen_config(), model_height=H, model_width=W, gauss_sigma=5, skeleton_thres=0.001, foot_thres=0.001)
    dirs = [os.path.join(root, d) for d in ("inputs", "DAIN", "Predict_motion")]
    gt_dir = os.path.join(root, "gt") if os.path.isdir(os.path.join(root, "gt")) else None
    outs, said = {}, {}
    for where in ("host", "gpu"):
        E = ev.Evaluator(cfg, batch=2, chunk=2, lanes=2, resize_on=where, io_mode=io_mode)
        outs[where] = os.path.join(root, "out_" + where)
        written = E.evaluate_from_folder(G, *dirs, outs[where], gt_dir=gt_dir, metrics=metrics)
        assert len(written) > 0
        said[where] = capsys.readouterr().out if capsys is not None else ""
    for sub in sorted(os.listdir(outs["host"])):
        if sub == "metrics.json":
            continue
        names = sorted(os.listdir(os.path.join(outs["host"], sub)))
        assert names == sorted(os.listdir(os.path.join(outs["gpu"], sub))) and names
        for nm in names:
            assert open(os.path.join(outs["host"], sub, nm), "rb").read() == open(os.path.join(outs["gpu"], sub, nm), "rb").read(), (sub, nm)
    if metrics:
        with open(os.path.join(outs["host"], "metrics.json")) as f, open(os.path.join(outs["gpu"], "metrics.json")) as g:
            assert json.load(f) == json.load(g)
    return said


@pytest.mark.parametrize("io_mode", ["process", "thread"])
@pytest.mark.parametrize("factor", [2.0, 1.5, 1.0])
def test_folder_driver_writes_the_same_files(tmp_path, factor, io_mode, capsys):
    H, W = 64, 96
    _example(str(tmp_path), H, W, [(int(H * factor), int(W * factor))])
    said = _run_both(str(tmp_path), H, W, io_mode=io_mode, capsys=capsys)
    assert "falls back" not in said["gpu"]


@pytest.mark.parametrize("masked", [False])
def test_folder_driver_metrics_are_identical(tmp_path, masked, capsys):
    H, W = 64, 96
    _example(str(tmp_path), H, W, [(128, 192)], gt_size=(160, 200))
    said = _run_both(str(tmp_path), H, W, metrics=True, capsys=capsys)
    assert "falls back" not in said["gpu"]


def test_mixed_dain_sizes_fall_back_and_say_so(tmp_path, capsys):
    H, W = 64, 96
    _example(str(tmp_path), H, W, [(128, 192), (96, 144)])
    said = _run_both(str(tmp_path), H, W, capsys=capsys)
    assert "clipA" in said["gpu"] and "falls back to the host resize" in said["gpu"] and "DAIN" in said["gpu"]
    assert "falls back" not in said["host"]
