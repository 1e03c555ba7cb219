"""The folder driver's output_size="keyframes" (background="mci" at the size of the key frame files) on the host, behind a
recording model that speaks the reference's protocol: every file against background.mci_frames_scaled_host and
composite.composite_host, the refusals, the staging spec and the command line.  Every comparison is exact."""
import os

import numpy as np
import pytest
import torch

from render_in_between_amd import background as bg, composite, evaluator as ev, panel, resize
from tests.composite_common import write_example
from tests.test_composite_cpu import NativeStub, Recorder, cfg32, dirs_of, png
from tests.test_driver import oracle_labels
from tests.test_panels_cpu import parse_riff


def moving_keys(root, n_key, hw, clip="clipA", step=(4, -2), sizes=None):
    """Overwrites write_example's key frames with crops of one blocky scene that moves by `step` px per key frame (so the
    field is not zero); sizes: {key index: (h, w)} for keys of another size."""
    from PIL import Image
    h, w = hw
    rng = np.random.default_rng(5)
    pad = 4 * n_key + 8
    cells = rng.integers(30, 226, ((h + 2 * pad) // 6 + 1, (w + 2 * pad) // 6 + 1, 3)).astype(np.uint8)
    big = np.repeat(np.repeat(cells, 6, 0), 6, 1)
    for k in range(n_key):
        kh, kw = (sizes or {}).get(k, hw)
        oy, ox = pad + k * step[1], pad + k * step[0]
        Image.fromarray(np.ascontiguousarray(big[oy:oy + kh, ox:ox + kw])).save(os.path.join(root, "inputs", clip, "%04d.png" % k))


def run(model, root, out, **kw):
    inputs_dir, _, pose_dir = dirs_of(root)
    return ev.Evaluator(cfg32(), label_fn=oracle_labels).evaluate_from_folder(model, inputs_dir, None, pose_dir, out, background="mci", **kw)


@pytest.mark.parametrize("kw", [dict(), dict(mci_border="valid", mci_precision="half")])
def test_reference_protocol_driver_writes_the_composite_at_the_key_frames_size(tmp_path, kw):
    """32x32 model, 40x48 key frames, 3 key frames at rate 2: PNG i is composite_host of the model's (img, mask) over
    mci_frames_scaled_host's frame, key frames are their files, the .avi frames are jpeg_encode_host of the PNG arrays."""
    root = str(tmp_path)
    n = write_example(root, n_key=3, rate=2, key_hw=(40, 48))
    moving_keys(root, 3, (40, 48))
    M = Recorder()
    out = os.path.join(root, "out")
    written = run(M, root, out, output_size="keyframes", video=True, video_quality=80, **kw)
    assert [os.path.relpath(w, out) for w in written] == [os.path.join("clipA", "f%03d.png" % i) for i in range(n)] and n == 5
    assert len(M.calls) == 2
    keys = [png(os.path.join(root, "inputs", "clipA", "%04d.png" % k)) for k in range(3)]
    small = [resize.resize_cubic_u8(k_, 32, 32) for k_ in keys]
    border, precision = kw.get("mci_border", "clamp"), kw.get("mci_precision", "full")
    moved = False
    for i in range(n):
        got = png(written[i])
        assert got.shape == (40, 48, 3)
        if i % 2 == 0:
            assert np.array_equal(got, keys[i // 2]), i
        else:
            k = i // 2
            field = bg.mci_field_host(small[k], small[k + 1], border=border)
            if precision == "half":
                field = bg.mci_refine_host(small[k], small[k + 1], field, border=border)
            moved |= bool(field.any())
            back = bg.mci_frames_scaled_host(keys[k], keys[k + 1], field, (32, 32), 2, [1], border=border, precision=precision)
            img, mask = M.calls[k]
            assert np.array_equal(got, composite.composite_host(img.numpy(), mask.numpy(), back)[0]), i
    assert moved
    raw = open(os.path.join(out, "clipA_video.avi"), "rb").read()
    frames = [raw[o:o + size] for o, size in parse_riff(raw)["movi/00dc"]]
    assert len(frames) == n
    for i in range(n):
        assert frames[i] == panel.jpeg_encode_host(png(written[i]), 80), i


def test_the_chain_reads_what_it_reads_at_the_model_size(tmp_path):
    """The model is called with the same tensors under output_size="keyframes" and "model": the (img, mask) pairs are equal."""
    root = str(tmp_path)
    write_example(root, n_key=3, rate=2, key_hw=(40, 48))
    moving_keys(root, 3, (40, 48))
    calls = {}
    for size in ("model", "keyframes"):
        M = Recorder()
        w = run(M, root, os.path.join(root, size), output_size=size)
        calls[size] = M.calls
        assert png(w[1]).shape == ((32, 32, 3) if size == "model" else (40, 48, 3))
    assert len(calls["model"]) == len(calls["keyframes"]) == 2
    for (i0, m0), (i1, m1) in zip(calls["model"], calls["keyframes"]):
        assert torch.equal(i0, i1) and torch.equal(m0, m1)


def test_a_clip_with_mixed_key_sizes_is_refused_by_name_with_nothing_written(tmp_path):
    root = str(tmp_path)
    write_example(root, n_key=3, rate=2, key_hw=(40, 48))
    moving_keys(root, 3, (40, 48), sizes={2: (40, 52)})
    out = os.path.join(root, "out")
    with pytest.raises(ValueError, match=r"output_size='keyframes': clip clipA: the key frames have mixed sizes \(48x40, 52x40\)"):
        run(Recorder(), root, out, output_size="keyframes", video=True)
    assert not os.path.exists(out) or not [f for _, _, fs in os.walk(out) for f in fs]


def test_key_frames_beyond_the_ratio_are_refused_by_name(tmp_path):
    root = str(tmp_path)
    write_example(root, n_key=2, rate=2, key_hw=(40, 16 * 32 + 1))
    out = os.path.join(root, "out")
    with pytest.raises(ValueError, match=r"output_size='keyframes': clip clipA: .*within 1/16"):
        run(Recorder(), root, out, output_size="keyframes")
    assert not os.path.exists(out) or not [f for _, _, fs in os.walk(out) for f in fs]


def test_refusals_of_the_settings(tmp_path):
    root = str(tmp_path)
    write_example(root, n_key=2, rate=2)
    out = os.path.join(root, "out")
    E = ev.Evaluator(cfg32(), label_fn=oracle_labels)
    with pytest.raises(ValueError, match="output_size='keyframes' is a setting of background='mci'.*output_size='source'"):
        E.evaluate_from_folder(Recorder(), *dirs_of(root), out, output_size="keyframes")
    with pytest.raises(ValueError, match="output_size='source' with background='mci' is not supported.*use output_size='keyframes'"):
        E.evaluate_from_folder(Recorder(), dirs_of(root)[0], None, dirs_of(root)[2], out, output_size="source", background="mci")

    class Stub(NativeStub):                    # a native generator with the model-size interpolation only
        mci_frames = mci_refine = None
    with pytest.raises(RuntimeError, match="output_size='keyframes': this model has no GPU kernel"):
        run(Stub(), root, out, output_size="keyframes")
    assert not os.path.exists(out) or not [f for _, _, fs in os.walk(out) for f in fs]


def test_staging_spec_has_the_full_size_key_section_only_on_request():
    base = ev.staging_spec(2, 3, (8, 12), None, None, mci=True, mci_keys=True)
    assert [s[0] for s in base] == ["dain", "gt", "mask", "key", "mci_keys"]
    table0, total0 = ev.block_layout(ev.spec_bytes(base))
    spec = ev.staging_spec(2, 3, (8, 12), None, None, mci=True, mci_keys=True, mci_keys_src=(20, 10))
    assert spec[:5] == base and spec[5] == ("mci_keys_src", torch.uint8, (2, 3, 10, 20, 3), True)
    table, total = ev.block_layout(ev.spec_bytes(spec))
    assert list(table) == ["mci_keys", "mci_keys_src"] and table["mci_keys"] == table0["mci_keys"]
    assert table["mci_keys_src"][1] == 2 * 3 * 10 * 20 * 3 and total == table["mci_keys_src"][0] + table["mci_keys_src"][1] > total0
    both = ev.staging_spec(2, 3, (8, 12), None, None, mci=True, mci_keys=True, src_keys=(20, 10), mci_keys_src=(20, 10))
    assert [s[0] for s in both] == ["dain", "gt", "mask", "key", "mci_keys", "key_src", "mci_keys_src"]


def test_command_line(capsys):
    from render_in_between_amd import inference
    o = inference.parse_args(["--input-dir", "x", "--background", "mci", "--output-size", "keyframes", "--video", "--frames", "none",
                              "--poses", "keyframes", "--pose-dir", "p"])
    assert o.output_size == "keyframes" and o.background == "mci"
    for bad, text in ((["--output-size", "keyframes"], "--output-size keyframes is a setting of --background mci"),
                      (["--output-size", "keyframes", "--background", "dain", "--resize-on", "gpu"], "use --output-size source"),
                      (["--output-size", "keyframes", "--background", "mci", "--resize-on", "gpu"], "--background mci with --resize-on gpu is not supported"),
                      (["--output-size", "source", "--background", "mci"], "use --output-size keyframes")):
        with pytest.raises(SystemExit):
            inference.parse_args(["--input-dir", "x"] + bad)
        assert text in capsys.readouterr().err
    assert "at the key frames' size" in " ".join(inference.build_parser().format_help().split())


def test_summary_line_names_the_size():
    from render_in_between_amd import inference

    class E:
        timings = {"wall": 1.0, "frames": 2}
        io_threads, io_mode, png_compress_level, batch, reproducible = 1, "thread", None, 2, True
        background, mci_range, mci_border, mci_precision, output_size = "mci", 32, "clamp", "full", "keyframes"
    assert inference.summary_line(E()).endswith("| files at the key frames' size")
    E.output_size = "model"
    assert "key frames' size" not in inference.summary_line(E())
