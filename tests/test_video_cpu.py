"""The frames' video on the host (no GPU): evaluate_from_folder(video=True) and frames="none" behind the reference call protocol
(CPU model) - <clip>_video.avi through the RIFF parser of tests/test_panels_cpu.py, every frame against
panel.jpeg_encode_host of the bytes its PNG holds - the argument rules, the command-line flags, the fidelity of the composition
against PIL's encoder, and the binding of the float front end of the GPU encoder."""
import io
import os
import struct

import numpy as np
import pytest

from render_in_between_amd import evaluator as ev, panel, video
from tests.test_driver import _write_example, oracle_labels
from tests.test_jpeg_cpu import PSNR_MARGIN_DB, decode, pil_encode, psnr
from tests.test_panels_cpu import Recorder, parse_riff, small_cfg

H, W = 32, 48
# the C symbol of the float front end (Generator.jpeg_f32 / jpeg_f32_into): tests/test_native_host.py reads the names of
# include/rib.h with a pattern of lower-case letters and underscores, so an entry point's name carries no digit
SYMBOL = "rib_jpeg_float"


def tree(root):
    """{relative path: bytes} of every file under root."""
    out = {}
    for d, _, files in os.walk(root):
        for f in files:
            p = os.path.join(d, f)
            out[os.path.relpath(p, root)] = open(p, "rb").read()
    return out


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """One synthetic folder (3 key frames, rate 2: 5 frames) driven five ways, once for the module."""
    root = str(tmp_path_factory.mktemp("video"))
    n = _write_example(root, n_key=3, rate=2, H=H, W=W)
    cfg = small_cfg(H, W)
    dirs = [os.path.join(root, d) for d in ("inputs", "DAIN", "Predict_motion")]

    def run(name, **kw):
        out = os.path.join(root, name)
        written = ev.Evaluator(cfg, label_fn=oracle_labels).evaluate_from_folder(Recorder(cfg), *dirs, out, **kw)
        return out, written
    res = {"n": n, "root": root, "dirs": dirs, "cfg": cfg, "run": run}
    res["plain"] = run("plain")
    res["explicit"] = run("explicit", video=False, video_fps=30, video_quality=90, video_frames=False, frames="png")
    res["video"] = run("video", video=True, video_fps=12, video_quality=75)
    res["kept"] = run("kept", video=True, video_fps=12, video_quality=75, video_frames=True)
    res["none"] = run("none", video=True, video_fps=12, video_quality=75, frames="none")
    return res


def frames_of(avi):
    raw = open(avi, "rb").read()
    ck = parse_riff(raw)
    return raw, ck, [raw[o:o + size] for o, size in ck["movi/00dc"]]


def test_argument_errors(tmp_path):
    root = str(tmp_path)
    _write_example(root, n_key=2, rate=2)
    cfg = small_cfg()
    dirs = [os.path.join(root, d) for d in ("inputs", "DAIN", "Predict_motion")]
    E = ev.Evaluator(cfg, label_fn=oracle_labels)
    out = os.path.join(root, "o")
    with pytest.raises(ValueError, match="video"):
        E.evaluate_from_folder(Recorder(cfg), *dirs, out, frames="none")
    for kw in (dict(video_frames=True), dict(video_quality=80), dict(video_fps=25)):
        with pytest.raises(ValueError, match="video=True"):
            E.evaluate_from_folder(Recorder(cfg), *dirs, out, **kw)
    for q in (0, 101, 90.5, True):
        with pytest.raises(ValueError, match="video_quality"):
            E.evaluate_from_folder(Recorder(cfg), *dirs, out, video=True, video_quality=q)
    with pytest.raises(ValueError, match="video_fps"):
        E.evaluate_from_folder(Recorder(cfg), *dirs, out, video=True, video_fps=0)
    with pytest.raises(ValueError, match="frames"):
        E.evaluate_from_folder(Recorder(cfg), *dirs, out, video=True, frames="jpg")
    with pytest.raises(NotImplementedError, match="video=True"):
        E.evaluate_from_folder(Recorder(cfg), *dirs, out, gen_vid=True)
    assert not os.path.exists(out)


def test_command_line_flags_reach_the_driver(monkeypatch):
    from render_in_between_amd import inference
    o = inference.parse_args(["--input-dir", "x"])
    assert (o.video, o.video_fps, o.video_quality, o.video_frames, o.frames) == (False, None, None, False, "png")
    o = inference.parse_args(["--input-dir", "x", "--video", "--video-fps", "24", "--video-quality", "70", "--video-frames", "--frames", "none"])
    assert (o.video, o.video_fps, o.video_quality, o.video_frames, o.frames) == (True, 24.0, 70, True, "none")
    for bad in (["--frames", "none"], ["--video-fps", "24"], ["--video-quality", "70"], ["--video-frames"], ["--video", "--frames", "jpg"],
                ["--video", "--video-quality", "0"], ["--video", "--video-quality", "101"], ["--video", "--video-fps", "0"]):
        with pytest.raises(SystemExit):
            inference.parse_args(["--input-dir", "x"] + bad)
    # main() hands them to evaluate_from_folder
    seen = {}

    class Stop(Exception):
        pass

    def fake(self, model, *a, **kw):
        seen.update(kw)
        raise Stop
    monkeypatch.setattr(inference, "load_generator", lambda *a, **k: object())
    monkeypatch.setattr(inference.rib, "get_config", lambda path: inference.rib.AttrDict(model_height=H, model_width=W, gauss_sigma=5,
                                                                                         skeleton_thres=0.001, foot_thres=0.001))
    monkeypatch.setattr(inference.Evaluator, "evaluate_from_folder", fake)
    with pytest.raises(Stop):
        inference.main(o)
    assert {k: seen[k] for k in ("video", "video_fps", "video_quality", "video_frames", "frames")} == \
        dict(video=True, video_fps=24.0, video_quality=70, video_frames=True, frames="none")
    seen.clear()
    with pytest.raises(Stop):
        inference.main(inference.parse_args(["--input-dir", "x"]))
    assert {k: seen[k] for k in ("video", "video_fps", "video_quality", "video_frames", "frames")} == \
        dict(video=False, video_fps=30, video_quality=90, video_frames=False, frames="png")


def test_a_call_without_video_writes_what_it_wrote_before(runs):
    """All new arguments left out, and all of them at their defaults: the same tree, byte for byte - and under video=True the
    PNG folder is that tree's."""
    plain, explicit = tree(runs["plain"][0]), tree(runs["explicit"][0])
    assert sorted(plain) == sorted(os.path.join("clipA", "f%03d.png" % i) for i in range(runs["n"]))
    assert plain == explicit
    assert [os.path.relpath(w, runs["plain"][0]) for w in runs["plain"][1]] == [os.path.relpath(w, runs["explicit"][0]) for w in runs["explicit"][1]]
    with_video = tree(runs["video"][0])
    assert {k: v for k, v in with_video.items() if k.startswith("clipA" + os.sep)} == plain
    assert sorted(set(with_video) - set(plain)) == ["clipA_video.avi"]


def test_the_video_parses_and_every_frame_is_the_definition_of_its_png(runs):
    from PIL import Image
    out, written = runs["video"]
    n = runs["n"]
    raw, ck, frames = frames_of(os.path.join(out, "clipA_video.avi"))
    assert len(frames) == n == 5 and len(written) == n
    o, size = ck["hdrl/avih"][0]
    avih = struct.unpack("<14I", raw[o:o + size])
    assert avih[0] == int(round(1e6 / 12)) and avih[4] == n and (avih[8], avih[9]) == (W, H)
    o, size = ck["hdrl/strl/strh"][0]
    scale, rate, start, length = struct.unpack("<4I", raw[o + 20:o + 36])
    assert rate / scale == 12 and start == 0 and length == n
    for i in range(n):
        u8 = np.asarray(Image.open(written[i]))
        assert u8.shape == (H, W, 3) and u8.dtype == np.uint8
        assert frames[i] == panel.jpeg_encode_host(u8, 75), i
        im = decode(frames[i])                                   # PIL decodes every frame
        assert im.format == "JPEG" and im.size == (W, H) and im.mode == "RGB"
    assert not os.path.exists(os.path.join(out, "clipA_video"))   # the .jpg files are gone with their folder
    assert not os.path.exists(os.path.join(out, "clipA.avi"))     # the sheets' name stays the sheets'


def test_video_frames_keeps_the_jpg_files(runs):
    out, _ = runs["kept"]
    _, _, frames = frames_of(os.path.join(out, "clipA_video.avi"))
    assert open(os.path.join(out, "clipA_video.avi"), "rb").read() == open(os.path.join(runs["video"][0], "clipA_video.avi"), "rb").read()
    assert sorted(os.listdir(os.path.join(out, "clipA_video"))) == ["%04d.jpg" % i for i in range(runs["n"])]
    for i in range(runs["n"]):
        assert open(video.frame_name(out, "clipA", i), "rb").read() == frames[i]


def test_frames_none_writes_the_same_video_and_no_png(runs):
    out, written = runs["none"]
    assert tree(out) == {"clipA_video.avi": open(os.path.join(runs["video"][0], "clipA_video.avi"), "rb").read()}
    assert not os.path.exists(os.path.join(out, "clipA"))
    assert written == [video.frame_name(out, "clipA", i) for i in range(runs["n"])]      # what the rank wrote (muxed since)


def test_video_beside_panels_and_metrics(runs, tmp_path):
    """Both videos in one call, frames="none" with panels and metrics still working; two ranks dealt by hand and assembled by
    the caller give the single writer's file."""
    from PIL import Image
    root, dirs, n = runs["root"], runs["dirs"], runs["n"]
    gt_dir = str(tmp_path / "gt")
    os.makedirs(os.path.join(gt_dir, "clipA"))
    rng = np.random.default_rng(5)
    for i in range(n):
        Image.fromarray(rng.integers(0, 255, (H, W, 3), dtype=np.uint8)).save(os.path.join(gt_dir, "clipA", "g%03d.png" % i))
    cfg = runs["cfg"]
    ref = os.path.join(str(tmp_path), "ref")
    ev.Evaluator(cfg, label_fn=oracle_labels).evaluate_from_folder(Recorder(cfg), *dirs, ref, gt_dir=gt_dir, metrics=True, panels=True)
    both = os.path.join(str(tmp_path), "both")
    E = ev.Evaluator(cfg, label_fn=oracle_labels)
    E.evaluate_from_folder(Recorder(cfg), *dirs, both, gt_dir=gt_dir, metrics=True, panels=True, video=True, frames="none")
    got, want = tree(both), tree(ref)
    assert sorted(got) == ["clipA.avi", "clipA_video.avi", "metrics.json"]
    assert got["clipA.avi"] == want["clipA.avi"] and got["metrics.json"] == want["metrics.json"]
    _, _, frames = frames_of(os.path.join(both, "clipA_video.avi"))
    for i in range(n):                                            # gt_dir's frames are the key frames here
        u8 = np.asarray(Image.open(os.path.join(ref, "clipA", "f%03d.png" % i)))
        assert frames[i] == panel.jpeg_encode_host(u8, 90), i
    two = os.path.join(str(tmp_path), "two")
    for rank in (1, 0):
        ev.Evaluator(cfg, label_fn=oracle_labels).evaluate_from_folder(Recorder(cfg), *dirs, two, gt_dir=gt_dir, video=True, frames="none",
                                                                       rank=rank, world=2)
        assert not os.path.exists(os.path.join(two, "clipA_video.avi"))      # ranks without a process group do not mux
    assert sorted(os.listdir(os.path.join(two, "clipA_video"))) == ["%04d.jpg" % i for i in range(n)]
    video.assemble(two, "clipA")
    assert tree(two) == {"clipA_video.avi": got["clipA_video.avi"]}


def test_a_video_beyond_the_riff_limit_is_refused_with_every_file_in_place(runs, monkeypatch, tmp_path):
    out = os.path.join(str(tmp_path), "big")
    monkeypatch.setattr(panel, "AVI_MAX_BYTES", 1000)
    with pytest.raises(ValueError, match="OpenDML"):
        runs["run"](os.path.relpath(out, runs["root"]), video=True)
    assert not os.path.exists(os.path.join(out, "clipA_video.avi"))
    assert sorted(os.listdir(os.path.join(out, "clipA_video"))) == ["%04d.jpg" % i for i in range(runs["n"])]
    assert len(os.listdir(os.path.join(out, "clipA"))) == runs["n"]


def test_fidelity_of_the_composition_against_pil():
    """A float frame through quantise_host and the definition, decoded by PIL, is within test_jpeg_cpu.py's margin of PIL's own
    encode of the same bytes at the same quality."""
    y, x = np.mgrid[0:H, 0:W]
    rng = np.random.default_rng(3)
    smooth = np.stack([np.sin(x / 7.0 + c) * np.cos(y / 5.0 - c) for c in range(3)]).astype(np.float32) * 1.1      # clips at both ends
    smooth += rng.normal(0, 0.02, smooth.shape).astype(np.float32)
    u8 = panel.quantise_host(smooth)
    assert u8.min() == 0 and u8.max() == 255
    for q in (50, 90):
        ours = video.frame_host(smooth, q)
        assert ours == panel.jpeg_encode_host(u8, q)
        d_db = psnr(decode(pil_encode(u8, q)), u8) - psnr(decode(ours), u8)
        print("q%d: deficit against PIL %+.4f dB" % (q, d_db))
        assert d_db <= PSNR_MARGIN_DB, (q, d_db)


def test_bindings_and_exports_cover_the_float_front_end():
    import subprocess
    from render_in_between_amd import _native
    assert {SYMBOL, "rib_jpeg", "rib_jpeg_max_bytes", "rib_jpeg_workspace_bytes"} <= set(_native.SIGNATURES)
    assert _native.SIGNATURES[SYMBOL] == _native.SIGNATURES["rib_jpeg"]
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert SYMBOL + "(" in open(os.path.join(here, "include", "rib.h")).read()
    if not os.path.exists(_native.LIB_PATH):
        _native.lib()
    out = subprocess.run(["nm", "-D", "--defined-only", _native.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert SYMBOL in [l.split()[-1] for l in out.splitlines() if l.split()[1] in "Tt"]
    import render_in_between_amd as rib
    assert hasattr(rib.Generator, "jpeg_f32") and hasattr(rib.Generator, "jpeg_f32_into")
