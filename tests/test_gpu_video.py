"""The frames' video on the MI355X: the float front end of the JPEG encoder (rib_jpeg_float: Generator.jpeg_f32 / jpeg_f32_into,
k_jpeg_segments<float> in csrc/jpeg.hip.h) byte for byte against panel.jpeg_encode_host(panel.quantise_host(x)) and against the
two-launch composition jpeg(quantise(x)), and the folder driver's video=True / frames="none" end to end on the native path.
Every comparison is exact."""
import os

import numpy as np
import pytest
import torch

import render_in_between_amd as rib
from render_in_between_amd import evaluator as ev, panel, video
from tests.test_gpu_quality import handle
from tests.test_jpeg_cpu import content
from tests.test_panels_cpu import parse_riff

pytestmark = pytest.mark.gpu

# one MCU; edge MCUs on both axes; across the 256-pixel chunk boundary with a partial chunk; W % 4 != 0 (scalar loads); the
# driver's smallest
SIZES = [(16, 16), (24, 40), (32, 272), (17, 35), (64, 64)]
KINDS = ("noise", "steps", "checker")
_X, _WANT = {}, {}


def frames_of(kind, H, W):
    """float32 [2, 3, H, W], made once.  noise: band-limited noise scaled to +-1.5, so both clamps act; steps: -1, +1, -0.0 and
    the quantiser's steps (k / 255 - 0.5) / 0.5 of all 256 k, and their float neighbours; checker: the 8 px black / white
    squares tests/test_jpeg_cpu.py reaches the long codes with."""
    key = (kind, H, W)
    if key in _X:
        return _X[key]
    rng = np.random.default_rng(H * 1000 + W)
    if kind == "noise":
        coarse = rng.normal(0, 1, (2, 3, H // 4 + 2, W // 4 + 2))
        a = np.kron(coarse, np.ones((4, 4)))[:, :, 1:H + 1, 2:W + 2] + rng.normal(0, 0.1, (2, 3, H, W))
        a = (a / np.abs(a).max() * 1.5).astype(np.float32)
        assert a.min() < -1 and a.max() > 1 and np.abs(a).max() == 1.5         # both clamps act
    elif kind == "steps":
        steps = ((np.arange(256) / 255.0 - 0.5) / 0.5).astype(np.float32)
        vals = np.concatenate([np.array([-1.0, 1.0, -0.0], np.float32), steps, np.nextafter(steps, np.float32(-2)), np.nextafter(steps, np.float32(2))])
        a = np.resize(vals, (3, H, W, 2)).transpose(3, 0, 1, 2).copy()          # consecutive values along a pixel's column, not its row
        a[1] = rng.permutation(np.resize(vals, 3 * H * W)).reshape(3, H, W)
        assert np.signbit(a).any() and (a == 0).any()
    else:
        u8 = np.stack([content("checker", H, W), 255 - content("checker", H, W)])
        a = ((u8.astype(np.float32) / 255.0 - 0.5) / 0.5).transpose(0, 3, 1, 2).copy()
        assert np.array_equal(panel.quantise_host(a), u8)
    _X[key] = a
    return a


def want(kind, H, W, q):
    """The definition's files of frames_of(kind, H, W), computed once."""
    key = (kind, H, W, q)
    if key not in _WANT:
        _WANT[key] = [video.frame_host(x, q) for x in frames_of(kind, H, W)]
    return _WANT[key]


@pytest.mark.parametrize("q", [50, 90, 100])
@pytest.mark.parametrize("H,W", SIZES)
def test_float_frames_give_the_definitions_files(H, W, q):
    G = handle()
    for kind in KINDS:
        x = torch.from_numpy(frames_of(kind, H, W)).cuda()
        got = G.jpeg_f32(x, q)
        assert got == want(kind, H, W, q), (kind, H, W, q)
        assert got == G.jpeg(G.quantise(x), q), (kind, H, W, q)
        assert np.array_equal(G.quantise(x).cpu().numpy(), panel.quantise_host(frames_of(kind, H, W)))


@pytest.mark.parametrize("H,W", [(24, 40), (64, 64), (32, 272)])
def test_a_source_that_is_not_16_byte_aligned(H, W):
    """The tensor starts 4, 8 and 12 bytes into an allocation: the rows are not 16-byte aligned and the loads are scalar."""
    G = handle()
    a = frames_of("noise", H, W)
    for off in (1, 2, 3):
        flat = torch.zeros(a.size + off, dtype=torch.float32, device="cuda")
        x = flat[off:].view(a.shape)
        x.copy_(torch.from_numpy(a))
        assert x.data_ptr() % 16 == 4 * off and x.is_contiguous()
        assert G.jpeg_f32(x, 90) == want("noise", H, W, 90), (H, W, off)


def test_a_frame_alone_and_as_frame_two_of_three():
    G = handle()
    H, W = 24, 40
    a = np.concatenate([frames_of("checker", H, W)[:1], frames_of("noise", H, W)[:1], frames_of("steps", H, W)[:1]])
    x = torch.from_numpy(a).cuda()
    three = G.jpeg_f32(x, 90)
    assert G.jpeg_f32(x[1:2].contiguous(), 90)[0] == three[1] == want("noise", H, W, 90)[0]


def test_destination_inside_a_larger_buffer():
    G = handle()
    H, W = 24, 40
    x = torch.from_numpy(frames_of("noise", H, W)).cuda()
    files = want("noise", H, W, 90)
    cap = G.jpeg_max_bytes(H, W) + 5                              # an odd stride: every frame starts at another alignment
    for off in (256, 4, 1, 7):
        buf = torch.full((off + 2 * cap + 64,), 77, dtype=torch.uint8, device="cuda")
        lengths = torch.full((4,), -7, dtype=torch.int32, device="cuda")
        assert G.jpeg_f32_into(x, buf[off:off + 2 * cap], lengths[1:3], 90, cap) == cap
        host, n = buf.cpu().numpy(), lengths.cpu().tolist()
        assert n == [-7] + [len(f) for f in files] + [-7]
        for t in range(2):
            assert host[off + t * cap:off + t * cap + n[t + 1]].tobytes() == files[t], (off, t)
            assert (host[off + t * cap + n[t + 1]:off + (t + 1) * cap] == 77).all()          # nor behind a file inside its stride
        assert (host[:off] == 77).all() and (host[off + 2 * cap:] == 77).all()              # nothing outside the strides


def test_a_cap_too_small_is_an_ordinary_refusal_and_bad_arguments_launch_nothing():
    G = handle()
    H, W = 24, 40
    noise = frames_of("noise", H, W)[0]
    flat = np.full((3, H, W), 0.5, np.float32)
    big, small = len(video.frame_host(noise, 100)), len(video.frame_host(flat, 100))
    cap = big - 1
    assert small < cap
    x = torch.from_numpy(np.stack([flat, noise, flat])).cuda()
    buf = torch.full((16 + 3 * cap + 16,), 77, dtype=torch.uint8, device="cuda")
    lengths = torch.full((3,), -7, dtype=torch.int32, device="cuda")
    G.jpeg_f32_into(x, buf[16:16 + 3 * cap], lengths, 100, cap)
    host = buf.cpu().numpy()
    assert lengths.cpu().tolist() == [small, 0, small]             # the noise frame is refused, its neighbours are not
    assert (host[16 + cap:16 + 2 * cap] == 77).all()               # a refused frame writes nothing
    assert host[16:16 + small].tobytes() == video.frame_host(flat, 100) == host[16 + 2 * cap:16 + 2 * cap + small].tobytes()
    assert (host[:16] == 77).all() and (host[16 + 3 * cap:] == 77).all()
    # the arguments the entry itself refuses: nothing is launched, nothing is written
    before = buf.clone()
    lengths.fill_(-7)
    for kw in (dict(quality=0), dict(quality=101), dict(quality=90.5), dict(cap=100), dict(cap=cap + 100)):
        with pytest.raises(ValueError):
            G.jpeg_f32_into(x, buf[16:16 + 3 * cap], lengths, **dict(dict(quality=90, cap=cap), **kw))
    for bad in (G.quantise(x), x.double(), x[:, :2].contiguous(), x[0], x.transpose(2, 3)):
        with pytest.raises(ValueError):
            G.jpeg_f32(bad, 90)
    from render_in_between_amd import _native
    L = _native.lib()
    ws = torch.empty(int(L.rib_jpeg_workspace_bytes(G._h, 3, H, W)), dtype=torch.uint8, device="cuda")
    ok = [3, H, W, x.data_ptr(), 90, buf.data_ptr(), cap, lengths.data_ptr(), ws.data_ptr()]
    for i, bad in ((0, 0), (0, 65536), (1, 0), (2, 65536), (3, None), (3, x.data_ptr() + 2), (4, 0), (4, 101), (5, None), (6, 630), (6, 2 ** 31),
                   (7, None), (7, lengths.data_ptr() + 2), (8, None), (8, ws.data_ptr() + 8)):
        args = list(ok)
        args[i] = bad
        assert L.rib_jpeg_float(G._h, *args, None) == -1, (i, bad)     # RIB_ERR_INVALID
        assert b"rib_jpeg_float" in L.rib_last_error(G._h)
    torch.cuda.synchronize()
    assert torch.equal(buf, before) and lengths.cpu().tolist() == [-7, -7, -7]


# ---- the folder driver ---------------------------------------------------------------------------------------------------------
H64 = W64 = 64


def cfg64():
    return rib.AttrDict(gen=rib.hsm_gen_config(), model_height=H64, model_width=W64, gauss_sigma=5, skeleton_thres=0.001, foot_thres=0.001)


def video_frames(avi):
    raw = open(avi, "rb").read()
    return [raw[o:o + size] for o, size in parse_riff(raw)["movi/00dc"]]


def test_native_folder_driver_video_and_frames_none(tmp_path):
    """64x64, 3 key frames at rate 4, batch 2, chunk 2 (first and later chunks, a loose last key frame): the PNG tree is the tree
    of a call without video, every video frame is the definition's file of the bytes its PNG holds, and frames="none" writes
    that video and nothing else - with threads and with worker processes."""
    from PIL import Image
    from tests.test_driver import _write_example
    root = str(tmp_path)
    n = _write_example(root, n_key=3, rate=4, H=H64, W=W64)
    G = handle()
    dirs = [os.path.join(root, d) for d in ("inputs", "DAIN", "Predict_motion")]

    def run(name, io_mode="thread", **kw):
        out = os.path.join(root, name)
        return out, ev.Evaluator(cfg64(), batch=2, chunk=2, lanes=1, io_mode=io_mode).evaluate_from_folder(G, *dirs, out, **kw)

    plain, plain_w = run("plain")
    out, written = run("video", video=True, video_quality=80, video_fps=24)
    assert [os.path.relpath(w, out) for w in written] == [os.path.relpath(w, plain) for w in plain_w] and len(written) == n == 9
    for x, y in zip(written, plain_w):
        assert open(x, "rb").read() == open(y, "rb").read(), x
    assert sorted(os.listdir(out)) == ["clipA", "clipA_video.avi"]
    avi = open(os.path.join(out, "clipA_video.avi"), "rb").read()
    frames = video_frames(os.path.join(out, "clipA_video.avi"))
    assert len(frames) == n
    for i in range(n):
        assert frames[i] == panel.jpeg_encode_host(np.asarray(Image.open(written[i])), 80), i
    for io_mode, keep in (("thread", False), ("process", True)):
        none, none_w = run("none_" + io_mode, io_mode, video=True, video_quality=80, video_fps=24, frames="none", video_frames=keep)
        assert open(os.path.join(none, "clipA_video.avi"), "rb").read() == avi, io_mode
        assert sorted(os.listdir(none)) == (["clipA_video", "clipA_video.avi"] if keep else ["clipA_video.avi"])
        assert none_w == [video.frame_name(none, "clipA", i) for i in range(n)]
        if keep:
            assert [open(w, "rb").read() for w in none_w] == frames
    both, both_w = run("process_png", "process", video=True, video_quality=80, video_fps=24)
    assert open(os.path.join(both, "clipA_video.avi"), "rb").read() == avi
    for x, y in zip(both_w, plain_w):
        assert open(x, "rb").read() == open(y, "rb").read(), x


def test_native_video_equals_the_reference_protocol_paths(tmp_path):
    """The .avi of the native path is the .avi of the reference-protocol path through the same Generator.  Under
    background="mci": there the two paths feed the generator the same floats (tests/test_gpu_mci.py), so nothing separates
    their frames; with --panels --panel-encode gpu beside it both videos are written and the frames' one is unchanged."""
    from tests.test_gpu_mci import Protocol, _moving_example
    root = str(tmp_path)
    n = _moving_example(root)
    G = handle()
    inputs, poses = os.path.join(root, "inputs"), os.path.join(root, "Predict_motion")
    kw = dict(background="mci", video=True, video_quality=85)
    nat = os.path.join(root, "native")
    ev.Evaluator(cfg64(), batch=2, chunk=2, lanes=1).evaluate_from_folder(G, inputs, None, poses, nat, frames="none", **kw)
    before = G.plan_batch
    G.set_plan_batch(2)                         # the reference-protocol path follows the plans the native group follows
    try:
        ref = os.path.join(root, "ref")
        ev.Evaluator(cfg64()).evaluate_from_folder(Protocol(G), inputs, None, poses, ref, **kw)
    finally:
        G.set_plan_batch(before)
    avi = open(os.path.join(nat, "clipA_video.avi"), "rb").read()
    assert len(video_frames(os.path.join(nat, "clipA_video.avi"))) == n == 9
    assert avi == open(os.path.join(ref, "clipA_video.avi"), "rb").read()
    assert sorted(os.listdir(nat)) == ["clipA_video.avi"]
    pan = os.path.join(root, "panels")
    ev.Evaluator(cfg64(), batch=2, chunk=2, lanes=1).evaluate_from_folder(G, inputs, None, poses, pan, panels=True, panel_encode="gpu", **kw)
    assert sorted(os.listdir(pan)) == ["clipA", "clipA.avi", "clipA_video.avi"]
    assert open(os.path.join(pan, "clipA_video.avi"), "rb").read() == avi
    assert len(video_frames(os.path.join(pan, "clipA.avi"))) == n
    for x in sorted(os.listdir(os.path.join(pan, "clipA"))):
        assert open(os.path.join(pan, "clipA", x), "rb").read() == open(os.path.join(ref, "clipA", x), "rb").read(), x
