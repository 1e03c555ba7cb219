"""The source-size composite on the host (no GPU): composite.composite_host against a per-pixel scalar restatement over the
project's independent scalar resize (oracle/resize_ref), its properties (mask 0 keeps the background, mask 1 is the enlarged
prediction, equal sizes take no resize, a sharp background survives wherever the mask's footprint is zero), the mask quantiser
at every step, the folder driver's output_size="source" on the reference-protocol path, and the argument rules.  Every
comparison is exact."""
import os
from fractions import Fraction

import numpy as np
import pytest
import torch

import render_in_between_amd as rib
from render_in_between_amd import composite, evaluator as ev, panel, resize, synth
from oracle import generator_ref, resize_ref
from tests.composite_common import footprint_clear, inputs, mask_steps, write_example
from tests.test_driver import MID_CFG, oracle_labels
from tests.test_panels_cpu import parse_riff

PAIRS = [((64, 64), (136, 240)), ((64, 64), (48, 100)), ((32, 32), (31, 33)), ((32, 32), (130, 257)), ((64, 64), (64, 64))]


def scalar_composite(pred, mask, bg):
    """The definition pixel by pixel, in Python numbers: the two quantisers in double, oracle/resize_ref's scalar resize, the blend."""
    n, _, H, W = pred.shape
    _, H0, W0, _ = bg.shape
    out = np.zeros_like(bg)
    for f in range(n):
        P = np.zeros((H, W, 3), np.uint8)
        M = np.zeros((H, W), np.uint8)
        for y in range(H):
            for x in range(W):
                for c in range(3):
                    P[y, x, c] = int(min(max(float(pred[f, c, y, x]) * 0.5 + 0.5, 0.0), 1.0) * 255.0)
                M[y, x] = int(min(max(float(mask[f, 0, y, x]), 0.0), 1.0) * 255.0)
        Pu, Mu = resize_ref.resize_cubic_u8(P, W0, H0), resize_ref.resize_cubic_u8(M, W0, H0)
        for y in range(H0):
            for x in range(W0):
                m = int(Mu[y, x])
                for c in range(3):
                    out[f, y, x, c] = (int(Pu[y, x, c]) * m + int(bg[f, y, x, c]) * (255 - m) + 127) // 255
    return out


@pytest.mark.parametrize("hw,hw0", [((16, 16), (23, 37)), ((16, 24), (9, 40))])
def test_composite_host_equals_the_scalar_restatement(hw, hw0):
    pred, mask, bg = inputs(*hw, *hw0)
    got = composite.composite_host(pred, mask, bg)
    assert got.dtype == np.uint8 and got.shape == bg.shape
    assert np.array_equal(got, scalar_composite(pred, mask, bg))


@pytest.mark.parametrize("hw,hw0", PAIRS)
def test_mask_zero_keeps_the_background_and_mask_one_is_the_enlarged_prediction(hw, hw0):
    pred, mask, bg = inputs(*hw, *hw0)
    (H0, W0) = hw0
    assert np.array_equal(composite.composite_host(pred, np.zeros_like(mask), bg), bg)
    want = np.stack([resize.resize_cubic_u8(p, W0, H0) for p in panel.quantise_host(pred)])
    assert np.array_equal(composite.composite_host(pred, np.ones_like(mask), bg), want)


def test_equal_sizes_take_no_resize():
    pred, mask, bg = inputs(64, 64, 64, 64)
    P = panel.quantise_host(pred).astype(np.int32)
    M = composite.quantise_mask_host(mask).astype(np.int32)[..., None]
    want = ((P * M + bg.astype(np.int32) * (255 - M) + 127) // 255).astype(np.uint8)
    assert np.array_equal(composite.composite_host(pred, mask, bg), want)
    assert M.max() == 255 and (M == 0).any() and ((M > 0) & (M < 255)).any()


@pytest.mark.parametrize("hw,hw0", PAIRS)
def test_a_sharp_background_survives_where_the_masks_footprint_is_zero(hw, hw0):
    """1-px checkerboard background, a mask that is zero outside a disc: out == bg on every pixel whose 4x4 tap footprint lies
    wholly in the zero region - and those are more than half of the frame."""
    (H, W), (H0, W0) = hw, hw0
    pred = inputs(*hw, *hw0)[0][:1]
    yy, xx = np.mgrid[0:H, 0:W]
    disc = (yy - H / 2) ** 2 + (xx - W / 2) ** 2 <= (min(H, W) / 5) ** 2
    mask = np.where(disc, np.float32(0.9), np.float32(0.0)).astype(np.float32)[None, None]
    y0, x0 = np.mgrid[0:H0, 0:W0]
    bg = np.repeat((((y0 + x0) & 1) * 255).astype(np.uint8)[:, :, None], 3, axis=2)[None]
    out = composite.composite_host(pred, mask, bg)
    clear = footprint_clear(~disc, H0, W0)
    assert clear.mean() > 0.5
    assert np.array_equal(out[0][clear], bg[0][clear])
    assert not np.array_equal(out[0], bg[0])                       # the disc is drawn


def test_mask_quantiser_at_every_step():
    vals = mask_steps()
    got = composite.quantise_mask_host(vals.reshape(1, 1, -1))
    assert got.dtype == np.uint8 and got.shape == (1, vals.size)
    want = [int(min(max(Fraction(float(v)), Fraction(0)), Fraction(1)) * 255) for v in vals]      # exact rationals, truncated
    assert got[0].tolist() == want
    steps = (np.arange(256) / 255.0).astype(np.float32)
    assert set(composite.quantise_mask_host(steps.reshape(1, 1, -1))[0].tolist()) >= {0, 1, 127, 254, 255}
    for v, q in ((-0.0, 0), (1.0, 255), (-0.1, 0), (-3.0, 0), (1.1, 255), (7.0, 255), (np.nextafter(np.float32(1), np.float32(0)), 254)):
        assert int(composite.quantise_mask_host(np.full((1, 1, 1), v, np.float32))[0, 0]) == q, v


# ---- the folder driver behind the reference's protocol -------------------------------------------------------------------------
def cfg32():
    return rib.AttrDict(gen=rib.hsm_gen_config(**MID_CFG), model_height=32, model_width=32, gauss_sigma=5, skeleton_thres=0.001,
                        foot_thres=0.001)


class Recorder:
    """The CPU oracle behind the reference's object protocol; keeps every call's (img, mask)."""

    def __init__(self):
        spec = rib.GenSpec.from_cfg(cfg32().gen)
        self.R = generator_ref.RefGenerator(spec, synth.make_state_dict(spec, 2))
        self.calls = []

    def eval(self):
        return self

    def __call__(self, label, label_prev, dain, prev):
        img, mask = self.R(label, label_prev, dain, prev)
        self.calls.append((img.detach().clone(), mask.detach().clone()))
        return img, mask


def dirs_of(root):
    return [os.path.join(root, d) for d in ("inputs", "DAIN", "Predict_motion")]


def png(path):
    from PIL import Image
    return np.asarray(Image.open(path).convert("RGB"))


def test_reference_protocol_driver_writes_the_composite_at_the_source_size(tmp_path):
    """32x32 model, 48x40 DAIN frames, 3 key frames at rate 2; the key frames are 44x36 files, so they are resized to 48x40."""
    root = str(tmp_path)
    n = write_example(root, n_key=3, rate=2, key_hw=(36, 44), dain_hw=(40, 48))
    inputs_dir, dain_dir, _ = dirs_of(root)
    M = Recorder()
    out = os.path.join(root, "out")
    written = ev.Evaluator(cfg32(), label_fn=oracle_labels).evaluate_from_folder(M, *dirs_of(root), out, output_size="source", video=True,
                                                                                 video_quality=80)
    assert [os.path.relpath(w, out) for w in written] == [os.path.join("clipA", "f%03d.png" % i) for i in range(n)] and n == 5
    assert len(M.calls) == 2
    calls = iter(M.calls)
    for i in range(n):
        got = png(written[i])
        assert got.shape == (40, 48, 3)
        if i % 2 == 0:                         # a key frame: the file's own pixels, resized because its size differs
            key = png(os.path.join(inputs_dir, "clipA", "%04d.png" % (i // 2)))
            assert key.shape == (36, 44, 3)
            assert np.array_equal(got, resize.resize_cubic_u8(key, 48, 40)), i
        else:
            img, mask = next(calls)
            bg = png(os.path.join(dain_dir, "clipA", "f%03d.png" % i))
            assert np.array_equal(got, composite.composite_host(img.numpy(), mask.numpy(), bg[None])[0]), i
    raw = open(os.path.join(out, "clipA_video.avi"), "rb").read()
    frames = [raw[o:o + size] for o, size in parse_riff(raw)["movi/00dc"]]
    assert len(frames) == n
    for i in range(n):
        assert frames[i] == panel.jpeg_encode_host(png(written[i]), 80), i


def test_a_key_frame_at_the_clips_size_is_its_files_pixels(tmp_path):
    root = str(tmp_path)
    write_example(root, n_key=2, rate=2, key_hw=(40, 48), dain_hw=(40, 48))
    out = os.path.join(root, "out")
    written = ev.Evaluator(cfg32(), label_fn=oracle_labels).evaluate_from_folder(Recorder(), *dirs_of(root), out, output_size="source")
    for k, i in ((0, 0), (1, 2)):
        assert np.array_equal(png(written[i]), png(os.path.join(root, "inputs", "clipA", "%04d.png" % k)))


def test_the_default_output_size_changes_no_file(tmp_path):
    root = str(tmp_path)
    write_example(root, n_key=3, rate=2)
    runs = {}
    for name, kw in (("never", {}), ("model", dict(output_size="model"))):
        out = os.path.join(root, name)
        w = ev.Evaluator(cfg32(), label_fn=oracle_labels).evaluate_from_folder(Recorder(), *dirs_of(root), out, video=True, video_frames=True, **kw)
        runs[name] = {os.path.relpath(os.path.join(d, f), out): open(os.path.join(d, f), "rb").read() for d, _, fs in os.walk(out) for f in fs}
        assert png(w[1]).shape == (32, 32, 3)
    assert runs["never"] == runs["model"] and len(runs["never"]) == 5 + 5 + 1


# ---- argument handling -----------------------------------------------------------------------------------------------------------
class NativeStub:
    """Looks like a native generator to the driver (chain, quantise); none of it is ever called."""
    device = torch.device("cpu")
    chain = quantise = resize_u8 = None

    def eval(self):
        return self


def test_refusals_of_evaluate_from_folder(tmp_path):
    root = str(tmp_path)
    write_example(root, n_key=2, rate=2, odd=(1, (40, 52)))
    out = os.path.join(root, "out")
    E = ev.Evaluator(cfg32(), label_fn=oracle_labels)
    with pytest.raises(ValueError, match="output_size must be one of"):
        E.evaluate_from_folder(Recorder(), *dirs_of(root), out, output_size="full")
    with pytest.raises(ValueError, match="output_size='source' with background='mci' is not supported"):
        E.evaluate_from_folder(Recorder(), dirs_of(root)[0], None, dirs_of(root)[2], out, output_size="source", background="mci")
    with pytest.raises(ValueError, match="output_size='source' needs resize_on='gpu' on the native path"):
        E.evaluate_from_folder(NativeStub(), *dirs_of(root), out, output_size="source")
    with pytest.raises(ValueError, match=r"clip clipA: the DAIN frames have mixed sizes \(48x40, 52x40\)"):
        E.evaluate_from_folder(Recorder(), *dirs_of(root), out, output_size="source")
    assert not os.path.exists(out) or not [f for _, _, fs in os.walk(out) for f in fs]       # nothing of the clip was written


def test_plan_counts_the_larger_download_block():
    """plan_gpu_resize with the source-size frame of the download block in the budget: the same sizes fit without it and send
    the DAIN list back to the host with it - which output_size="source" turns into an error."""
    sizes = [(192, 108)] * 8
    slot = 192 * 108 * 3
    free = ev.shm_windows_bytes(8 * slot) + 1
    src, why = ev.plan_gpu_resize(sizes, None, (32, 32), 8, shm_free=free)
    assert src["DAIN"] == (192, 108) and not why
    src, why = ev.plan_gpu_resize(sizes, None, (32, 32), 8, shm_free=free, out_slot_bytes=slot - 32 * 32 * 3)
    assert src["DAIN"] is None and why and why[0][0] == "DAIN"


def test_staging_spec_has_the_source_size_key_section_only_on_request():
    base = ev.staging_spec(2, 3, (8, 12), (20, 10), None)
    assert [s[0] for s in base] == ["dain", "gt", "mask", "key", "mci_keys"]
    spec = ev.staging_spec(2, 3, (8, 12), (20, 10), None, src_keys=(20, 10))
    assert spec[:5] == base and spec[5] == ("key_src", torch.uint8, (3, 10, 20, 3), True)
    table, total = ev.block_layout(ev.spec_bytes(spec))
    assert list(table) == ["dain", "key_src"] and table["key_src"][1] == 3 * 10 * 20 * 3 and total == table["key_src"][0] + table["key_src"][1]


def test_command_line(capsys):
    from render_in_between_amd import inference
    assert inference.parse_args(["--input-dir", "x"]).output_size == "model"
    o = inference.parse_args(["--input-dir", "x", "--resize-on", "gpu", "--output-size", "source", "--video", "--frames", "none"])
    assert o.output_size == "source"
    for bad, text in ((["--output-size", "source"], "--output-size source needs --resize-on gpu"),
                      (["--output-size", "source", "--background", "mci"], "--output-size source with --background mci is not supported"),
                      (["--output-size", "full", "--resize-on", "gpu"], "invalid choice")):
        with pytest.raises(SystemExit):
            inference.parse_args(["--input-dir", "x"] + bad)
        assert text in capsys.readouterr().err
