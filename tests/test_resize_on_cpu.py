"""Host side of Evaluator(resize_on="gpu") (no GPU): constructor and CLI validation, the fallback decision as a pure function of
sizes and budgets, the file worker's "do not resize" decode into a shared block, the header's declaration of the entry, the
arithmetic the kernel is given (tap tables + integer sums == the host function), and that the default changes nothing."""
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

import render_in_between_amd as rib
from render_in_between_amd import evaluator as ev, io_worker, resize
from tests.test_driver import MID_CFG, _write_example

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cfg(H=32, W=48):
    return rib.AttrDict(gen=rib.hsm_gen_config(**MID_CFG), model_height=H, model_width=W)


def _inference_module(name="rib_inference_resize"):
    p = os.path.join(ROOT, "render-in-between_amd", "inference.py")
    spec = importlib.util.spec_from_file_location(name, p)
    mod = importlib.util.module_from_spec(spec); spec.loader.exec_module(mod)
    return mod


def test_constructor_validates_resize_on():
    assert ev.Evaluator(_cfg()).resize_on == "host"                         # the default is today's path
    assert ev.Evaluator(_cfg(), resize_on="gpu").resize_on == "gpu"
    for bad in ("cuda", "device", "", None, True):
        with pytest.raises(ValueError):
            ev.Evaluator(_cfg(), resize_on=bad)
    with pytest.raises(ValueError, match="cv2"):
        ev.Evaluator(_cfg(), resize="pil", resize_on="gpu")                 # PIL's filter is not on the GPU
    assert ev.Evaluator(_cfg(), resize="pil").resize_on == "host"


def test_a_model_without_the_kernel_is_refused(tmp_path):
    root = str(tmp_path)
    _write_example(root)
    dirs = [os.path.join(root, d) for d in ("inputs", "DAIN", "Predict_motion")]

    class Reference:                         # only speaks the reference's call protocol
        def eval(self):
            return self

        def __call__(self, label, label_prev, dain, prev):
            raise AssertionError("must not be called")

    class NativeWithoutResize(Reference):
        chain = quantise = lambda *a, **k: None

    for model in (Reference(), NativeWithoutResize()):
        with pytest.raises(RuntimeError, match="resize"):
            ev.Evaluator(_cfg(), resize_on="gpu", io_mode="thread").evaluate_from_folder(model, *dirs, os.path.join(root, "o"))


def test_cli_flag_and_summary_line():
    mod = _inference_module()
    base = ["--input-dir", "x"]
    assert mod.parse_args(base).resize_on == "host"
    assert mod.parse_args(base + ["--resize-on", "gpu"]).resize_on == "gpu"
    with pytest.raises(SystemExit):
        mod.parse_args(base + ["--resize-on", "cuda"])
    for where in ("host", "gpu"):
        E = ev.Evaluator(_cfg(), resize_on=where)
        E.timings = {"frames": 0}
        assert "resize on %s" % where in mod.summary_line(E)


def test_fallback_decision_is_a_function_of_sizes_and_budgets():
    plan = ev.plan_gpu_resize
    model = (48, 32)
    # uniform lists go to the GPU, each at its own size; equal to the model size too (the call is then the normalisation)
    assert plan([(96, 64)] * 5, None, model, 8) == ({"DAIN": (96, 64), "GT": None}, [])
    assert plan([(96, 64)] * 5, [(200, 160)] * 5, model, 8) == ({"DAIN": (96, 64), "GT": (200, 160)}, [])
    assert plan([(48, 32)] * 2, None, model, 8)[0]["DAIN"] == (48, 32)
    # mixed sizes inside a list: that list alone falls back, with a reason
    src, why = plan([(96, 64), (72, 48), (96, 64)], [(200, 160)] * 3, model, 8)
    assert src == {"DAIN": None, "GT": (200, 160)} and [n for n, _ in why] == ["DAIN"] and "mixed" in why[0][1]
    src, why = plan([(96, 64)] * 3, [(200, 160), (200, 161)], model, 8)
    assert src == {"DAIN": (96, 64), "GT": None} and [n for n, _ in why] == ["GT"]
    # budgets: the windows of the real per-slot bytes at the source size must fit
    windows = ev.DECODE_AHEAD + ev.MAX_UNITS_IN_FLIGHT + 4
    assert ev.shm_windows_bytes(1000) == windows * 1000
    slots, hd = 16, (1920, 1080)
    need_dain = windows * slots * 1920 * 1080 * 3
    assert plan([hd] * 4, None, (512, 512), slots, shm_free=need_dain)[0]["DAIN"] == hd
    src, why = plan([hd] * 4, None, (512, 512), slots, shm_free=need_dain - 1)
    assert src["DAIN"] is None and why[0][0] == "DAIN" and "shared memory" in why[0][1]
    # with metrics the GT list gives way first; the DAIN list stays when it fits beside a model-size GT section (and a mask)
    both = windows * slots * (2 * 1920 * 1080 * 3)
    dain_only = windows * slots * (1920 * 1080 * 3 + 512 * 512 * 3 + 512 * 512)
    assert plan([hd] * 4, [hd] * 4, (512, 512), slots, shm_free=both)[0] == {"DAIN": hd, "GT": hd}
    src, why = plan([hd] * 4, [hd] * 4, (512, 512), slots, mask=True, shm_free=dain_only)
    assert src == {"DAIN": hd, "GT": None} and [n for n, _ in why] == ["GT"]
    src, why = plan([hd] * 4, [hd] * 4, (512, 512), slots, mask=True, shm_free=dain_only - 1)
    assert src == {"DAIN": None, "GT": None} and [n for n, _ in why] == ["GT", "DAIN"]
    # no shared staging (thread mode): no budget applies
    assert plan([hd] * 4, [hd] * 4, (512, 512), slots, shm_free=None)[0] == {"DAIN": hd, "GT": hd}


def test_worker_decodes_the_source_size_frame_into_the_block(tmp_path):
    from PIL import Image
    root = str(tmp_path)
    _write_example(root, n_key=2, rate=2)                                    # key frames / json at 32 x 48
    rng = np.random.default_rng(5)
    big = rng.integers(0, 255, (70, 90, 3), dtype=np.uint8)
    gtb = rng.integers(0, 255, (50, 60, 3), dtype=np.uint8)
    dain = os.path.join(root, "big.png"); Image.fromarray(big).save(dain)
    gtp = os.path.join(root, "gt.png"); Image.fromarray(gtb).save(gtp)
    pose = os.path.join(root, "Predict_motion", "clipA", "f001_keypoints.json")
    args = (dain, gtp, pose, True, True, 48, 32, "cv2", 0.001, 0.001)
    want = io_worker.load_frame(*args)
    blk = ev._shm_get(1 << 16)
    try:
        blk.t.zero_()
        off, goff = 1000, 1000 + big.size + 77
        pool = ev._process_pool(2)
        got = pool.submit(io_worker.load_frame_shm, blk.name, off, *args, goff, None, -1, (90, 70), (60, 50)).result()
        flat = blk.t.numpy()
        assert np.array_equal(flat[off:off + big.size].reshape(70, 90, 3), big)             # not resized, at the given offset
        assert np.array_equal(flat[goff:goff + gtb.size].reshape(50, 60, 3), gtb)
        assert not flat[:off].any() and not flat[off + big.size:goff].any() and not flat[goff + gtb.size:].any()
        # the key frame and the tables are what the resizing load returns: they do not depend on the mode
        assert got[0] is None and np.array_equal(io_worker.normalised_chw(got[1]), want[1])
        assert all(np.array_equal(a, b) for a, b in zip(got[2], want[2]))
        # without the two sizes the same call resizes, as before
        io_worker.load_frame_shm(blk.name, off, *args)
        assert np.array_equal(flat[off:off + 32 * 48 * 3].reshape(32, 48, 3), want[0])
        # a file that is not the size the slot was planned for is an error, not an overrun
        with pytest.raises(ValueError, match="planned"):
            io_worker.decode_raw_into(blk.shm.buf, 0, dain, (91, 70))
    finally:
        flat = None
        ev._shm_put(blk)


def test_header_declares_the_entry_and_the_build_hashes_the_kernel():
    from render_in_between_amd import _native
    hdr = open(os.path.join(ROOT, "include", "rib.h")).read()
    m = re.search(r"int rib_resize_cubic\(rib_handle\* h, int N, int H0, int W0, int H, int W,([^;]*);", hdr)
    assert m and "out_u8_nhwc" in m.group(1) and "out_f32_nchw" in m.group(1) and "hip_stream" in m.group(1)
    assert "evaluator.py:18-26,219-221" in hdr
    assert "rib_resize_cubic" in _native.SIGNATURES and len(_native.SIGNATURES["rib_resize_cubic"][1]) == 14
    spec = importlib.util.spec_from_file_location("rib_build_resize", os.path.join(ROOT, "render-in-between_amd", "csrc", "build.py"))
    mod = importlib.util.module_from_spec(spec); spec.loader.exec_module(mod)
    assert any(os.path.basename(d) == "resize.hip.h" for d in mod.DEPS)
    src = open(os.path.join(ROOT, "render-in-between_amd", "csrc", "resize.hip.h")).read()
    assert "k_resize_cubic_u8" in src and "asm" not in src


@pytest.mark.parametrize("src,dst", [((45, 80), (32, 48)), ((32, 48), (45, 80)), ((120, 67), (32, 32)), ((5, 7), (32, 48)), ((1, 9), (16, 16))])
def test_the_kernels_arithmetic_is_the_host_function(src, dst):
    """What the kernel is given and asked to do - the tables of resize._cubic_taps, v = sum_j cy[j] * sum_i cx[i] * src[iy[j]][ix[i]]
    in int32, (v + 2^21) >> 22 saturated - stated densely in numpy, equals resize_cubic_u8 (whose sparse products add coinciding
    clamped taps up first), for random and for 0 / 255 frames."""
    (h0, w0), (h, w) = src, dst
    rng = np.random.default_rng(h0 + w0)
    (ix, cx), (iy, cy) = resize._cubic_taps(w, w0), resize._cubic_taps(h, h0)
    for a in (rng.integers(0, 256, (h0, w0, 3), dtype=np.uint8), (rng.integers(0, 2, (h0, w0, 3)) * 255).astype(np.uint8)):
        g = a.astype(np.int32)[iy][:, :, ix]                                 # [h, 4, w, 4, 3]
        v = (g * cy.astype(np.int32)[:, :, None, None, None] * cx.astype(np.int32)[None, None, :, :, None]).sum(axis=(1, 3), dtype=np.int32)
        out = np.clip((v + (1 << 21)) >> 22, 0, 255).astype(np.uint8)
        assert np.array_equal(out, resize.resize_cubic_u8(a, w, h))


def test_default_construction_writes_the_same_files(tmp_path):
    """resize_on defaults to "host" and that path is today's: the tiny example renders to the same bytes with the argument left
    out and with it spelled, through the reference-protocol loop with a small deterministic stand-in model."""
    root = str(tmp_path)
    n = _write_example(root, n_key=3, rate=2, H=40, W=60)                   # files larger than the 32 x 48 model: they are resized

    class Model:
        def eval(self):
            return self

        def __call__(self, label, label_prev, dain, prev):
            img = torch.tanh(label[:, :3] * 0.5 + prev * 0.25 + dain * 0.5)
            return img, torch.sigmoid(label[:, 3:4] + dain[:, :1])

    from tests.test_driver import oracle_labels as label_fn
    dirs = [os.path.join(root, d) for d in ("inputs", "DAIN", "Predict_motion")]
    outs = []
    for kw in ({}, {"resize_on": "host"}):
        E = ev.Evaluator(_cfg(), label_fn=label_fn, **kw)
        out = os.path.join(root, "o%d" % len(outs))
        written = E.evaluate_from_folder(Model(), *dirs, out)
        assert len(written) == n
        outs.append([open(w, "rb").read() for w in written])
    assert outs[0] == outs[1]
