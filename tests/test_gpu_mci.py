"""The motion-compensated background on the MI355X: rib_mci_field / rib_mci_frames (csrc/mci.hip.h, Generator.mci_field /
mci_frames) against the integer definition in background.py, bit for bit, and the folder driver's background="mci"."""
import os

import numpy as np
import pytest
import torch

import render_in_between_amd as rib
from render_in_between_amd import background as bg, evaluator as ev, panel, synth

pytestmark = pytest.mark.gpu

_G = {}


def handle():
    if "g" not in _G:
        cfg = rib.hsm_gen_config()
        G = rib.Generator(cfg, device="cuda:0").eval()
        G.load_state_dict(synth.make_state_dict(rib.GenSpec.from_cfg(cfg), 0))
        _G["g"] = G
    return _G["g"]


def scene(h, w, seed):
    """A smooth random texture (bilinearly enlarged noise plus fine noise): uint8 [h, w, 3]."""
    g = torch.Generator().manual_seed(seed)
    coarse = torch.nn.functional.interpolate(torch.rand(1, 3, h // 12 + 3, w // 12 + 3, generator=g), size=(h + 24, w + 24), mode="bicubic", align_corners=False)
    fine = torch.rand(1, 3, h + 24, w + 24, generator=g)
    img = (coarse * 200 + fine * 55).clamp(0, 255)[0].permute(1, 2, 0)
    return img.to(torch.uint8).numpy()


def pair(h, w, seed):
    """Two key frames: crops of one scene displaced by a seed-dependent motion, plus a patch that moves differently."""
    big = scene(h, w, seed)
    dx, dy = [(6, -4), (-10, 2), (3, 9), (0, 0)][seed % 4]
    a = big[12:12 + h, 12:12 + w].copy()
    b = big[12 - dy:12 - dy + h, 12 - dx:12 - dx + w].copy()
    ph, pw = max(2, h // 4), max(2, w // 4)
    patch = scene(ph, pw, seed + 100)[:ph, :pw]
    a[h // 3:h // 3 + ph, w // 4:w // 4 + pw] = patch
    b[h // 3 + 3:h // 3 + 3 + ph, w // 4 - 5:w // 4 - 5 + pw] = patch[:min(ph, h - h // 3 - 3)]
    return a, b


_REF = {}


def reference(h, w, seed, s):
    key = (h, w, seed, s)
    if key not in _REF:
        a, b = pair(h, w, seed)
        f = bg.mci_field_host(a, b)
        _REF[key] = (a, b, f, bg.mci_frames_host(a, b, f, s, range(1, s)))
    return _REF[key]


@pytest.mark.parametrize("h,w", [(40, 56), (67, 93), (130, 250), (320, 480)])
def test_field_and_frames_equal_the_host_definition(h, w):
    G = handle()
    a, b, f, frames = reference(h, w, 1, 4)
    ta, tb = torch.from_numpy(a).to(G.device), torch.from_numpy(b).to(G.device)
    field = G.mci_field(ta, tb)
    assert field.shape == bg.field_shape(h, w) + (2,) and field.dtype == torch.int16
    assert torch.equal(field.cpu(), torch.from_numpy(f))
    assert f.any()                                                      # (a moving scene: the zero field would prove little)
    u8 = G.mci_frames(ta, tb, field, 4, normalised=False)
    assert torch.equal(u8.cpu(), torch.from_numpy(frames))


def test_batch_rate_and_sub_range():
    G = handle()
    h, w = 67, 93
    for s in (2, 4, 8):
        refs = [reference(h, w, seed, s) for seed in (1, 2, 3)]
        for B in (1, 3):
            ta = torch.from_numpy(np.stack([r[0] for r in refs[:B]])).to(G.device)
            tb = torch.from_numpy(np.stack([r[1] for r in refs[:B]])).to(G.device)
            field = G.mci_field(ta, tb)
            assert torch.equal(field.cpu(), torch.from_numpy(np.stack([r[2] for r in refs[:B]])))
            u8 = G.mci_frames(ta, tb, field, s, normalised=False)       # [s-1, B, h, w, 3]
            assert torch.equal(u8.cpu(), torch.from_numpy(np.stack([r[3] for r in refs[:B]], 1)))
            if s == 8:                                                  # a sub-range: frames 3..5
                sub = G.mci_frames(ta, tb, field, s, k_first=3, count=3, normalised=False)
                assert torch.equal(sub, u8[2:5])
            if B == 3:                                                  # every frame of the batch equals its own B = 1, T = 1 call
                for b_ in range(B):
                    f1 = G.mci_field(ta[b_], tb[b_])
                    assert torch.equal(f1, field[b_])
                    for k in range(1, s):
                        one = G.mci_frames(ta[b_], tb[b_], f1, s, k_first=k, count=1, normalised=False)
                        assert torch.equal(one[0], u8[k - 1, b_])


@pytest.mark.parametrize("h,w", [(67, 93), (40, 56)])
def test_outputs_float_uint8_and_null(h, w):
    G = handle()
    a, b, f, frames = reference(h, w, 2, 4)
    ta, tb, tf = (torch.from_numpy(x).to(G.device) for x in (a, b, f))
    f32, u8 = G.mci_frames(ta, tb, tf, 4, normalised="both")
    assert f32.shape == (3, 3, h, w) and u8.shape == (3, h, w, 3)
    assert torch.equal(u8.cpu(), torch.from_numpy(frames))
    # the driver's own normalisation of the uint8 output (evaluator._FolderPipeline.upload)
    dn = u8.permute(0, 3, 1, 2).to(torch.float32)
    dn = ((dn / 255.0 - 0.5) / 0.5).contiguous()
    assert torch.equal(f32, dn)
    # ... and its statement on the host, which the reference-protocol path feeds its model
    assert torch.equal(f32.cpu(), torch.from_numpy(bg.normalised_upload(frames)))
    # a NULL output is honoured: each alone equals its half of the pair, into caller-owned, pre-filled destinations
    only_f = torch.full((3, 3, h, w), 7.0, device=G.device)
    only_u = torch.full((3, h, w, 3), 9, dtype=torch.uint8, device=G.device)
    G.mci_frames(ta, tb, tf, 4, normalised=True, out=only_f)
    G.mci_frames(ta, tb, tf, 4, normalised=False, out=only_u)
    assert torch.equal(only_f, f32) and torch.equal(only_u, u8)
    L = G._lib
    assert L.rib_mci_frames(G._h, 1, 1, h, w, ta.data_ptr(), tb.data_ptr(), tf.data_ptr(), 4, 1, 0, None, None, None) != 0
    assert b"both outputs are null" in L.rib_last_error(G._h)
    assert L.rib_mci_frames(G._h, 1, 1, h, w, ta.data_ptr(), tb.data_ptr(), tf.data_ptr(), 3, 1, 0, only_f.data_ptr(), None, None) != 0
    assert b"power of two" in L.rib_last_error(G._h)
    with pytest.raises(ValueError, match="outside the segment"):
        G.mci_frames(ta, tb, tf, 4, k_first=3, count=3)


def _moving_example(root, n_key=3, rate=4, H=64, W=64):
    """tests/test_driver.py's folder with key frames that show a moving scene, and no DAIN folder."""
    import shutil
    from PIL import Image
    from tests.test_driver import _write_example
    n = _write_example(root, n_key=n_key, rate=rate, H=H, W=W)
    shutil.rmtree(os.path.join(root, "DAIN"))
    big = scene(H + 40, W + 40, 9)
    for k in range(n_key):
        Image.fromarray(big[20 + 3 * k:20 + 3 * k + H, 20 - 5 * k + 10:20 - 5 * k + 10 + W].copy()).save(os.path.join(root, "inputs", "clipA", "%04d.png" % k))
    return n


class Protocol:
    """The same Generator behind the reference's call protocol (no chain, no quantise: the driver takes run_reference)."""

    def __init__(self, G):
        self.G, self.device, self.rasterise = G, G.device, G.rasterise

    def eval(self):
        return self

    def __call__(self, label, label_prev, dain, prev):
        return self.G(label, label_prev, dain, prev)


@pytest.mark.parametrize("panels", [False, True])
def test_native_folder_driver(tmp_path, panels):
    """background="mci" on the native path (64x64, s = 4, 3 key frames, batch 2) against the native path reading a DAIN folder
    that holds the host definition's frames as PNGs: the generator must see the bytes it would see had the frames come from
    PNGs, so the files - and with panels the whole sheets - are the same bytes."""
    from PIL import Image
    root = str(tmp_path)
    H = W = 64
    n = _moving_example(root)
    G = handle()
    cfg = rib.AttrDict(gen=rib.hsm_gen_config(), model_height=H, model_width=W, gauss_sigma=5, skeleton_thres=0.001, foot_thres=0.001)
    inputs, poses = os.path.join(root, "inputs"), os.path.join(root, "Predict_motion")
    kw = dict(panels=True, panel_frames=True) if panels else {}
    E = ev.Evaluator(cfg, batch=2, chunk=2, lanes=1)
    out = os.path.join(root, "mci")
    written = E.evaluate_from_folder(G, inputs, None, poses, out, background="mci", **kw)
    assert [os.path.basename(x) for x in written] == ["f%03d.png" % i for i in range(n)] and n == 9
    # the host definition's frames as a DAIN folder
    keys = [E._decode_resized_u8(os.path.join(inputs, "clipA", "%04d.png" % k))[0] for k in range(3)]
    host = {}
    for k in range(3):
        host[4 * k] = keys[k]
    for k in range(2):
        fr = bg.mci_frames_host(keys[k], keys[k + 1], bg.mci_field_host(keys[k], keys[k + 1]), 4, [1, 2, 3])
        assert bg.mci_field_host(keys[k], keys[k + 1]).any()
        for j in range(3):
            host[4 * k + 1 + j] = fr[j]
    os.makedirs(os.path.join(root, "DAIN", "clipA"))
    for i in range(n):
        Image.fromarray(host[i]).save(os.path.join(root, "DAIN", "clipA", "f%03d.png" % i))
    via_png = ev.Evaluator(cfg, batch=2, chunk=2, lanes=1).evaluate_from_folder(G, inputs, os.path.join(root, "DAIN"), poses, os.path.join(root, "dain"), **kw)
    for x, y in zip(written, via_png):
        assert open(x, "rb").read() == open(y, "rb").read(), x
    if panels:                                  # the DAIN pane shows the MCI frame
        for i in range(n):
            sheet = np.asarray(Image.open(os.path.join(out, "clipA_panels", "%04d.png" % i)).convert("RGB"))
            # (a pane shows tensor2images of the normalised frame, as for a DAIN file: tests/test_gpu_panel.py)
            assert np.array_equal(panel.pane(sheet, "DAIN", H, W), panel.quantise_host(bg.normalised(host[i]))), i
            other = np.asarray(Image.open(os.path.join(root, "dain", "clipA_panels", "%04d.png" % i)).convert("RGB"))
            assert np.array_equal(sheet, other), i


@pytest.mark.parametrize("panels", [False, True])
def test_native_folder_driver_against_the_reference_protocol(tmp_path, panels):
    """background="mci" on the native path (64x64, s = 4, 3 key frames, batch 2) writes the PNG bytes of the reference-protocol
    path fed by the host definition through the same Generator: that path feeds the model the floats the native chain reads
    (background.normalised_upload: the device's normalisation stated on the host), so nothing separates the two.  With panels
    the DAIN pane of both paths' sheets is the MCI frame."""
    from PIL import Image
    root = str(tmp_path)
    H = W = 64
    n = _moving_example(root)
    G = handle()
    cfg = rib.AttrDict(gen=rib.hsm_gen_config(), model_height=H, model_width=W, gauss_sigma=5, skeleton_thres=0.001, foot_thres=0.001)
    inputs, poses = os.path.join(root, "inputs"), os.path.join(root, "Predict_motion")
    kw = dict(panels=True, panel_frames=True) if panels else {}
    written = ev.Evaluator(cfg, batch=2, chunk=2, lanes=1).evaluate_from_folder(G, inputs, None, poses, os.path.join(root, "mci"), background="mci", **kw)
    before = G.plan_batch
    G.set_plan_batch(2)                         # the reference-protocol path follows the plans the native group follows
    try:
        ref = ev.Evaluator(cfg).evaluate_from_folder(Protocol(G), inputs, None, poses, os.path.join(root, "ref"), background="mci", **kw)
    finally:
        G.set_plan_batch(before)
    diffs = [(np.asarray(Image.open(x)).astype(int) - np.asarray(Image.open(y)).astype(int)) for x, y in zip(written, ref)]
    print("native vs reference-protocol: max |diff| %d, differing values %d of %d"
          % (max(np.abs(d).max() for d in diffs), sum(int((d != 0).sum()) for d in diffs), sum(d.size for d in diffs)))
    assert len(written) == len(ref) == n
    for x, y in zip(written, ref):
        assert open(x, "rb").read() == open(y, "rb").read(), x
    if panels:
        for i in range(n):
            mine, theirs = (np.asarray(Image.open(os.path.join(root, d, "clipA_panels", "%04d.png" % i)).convert("RGB")) for d in ("mci", "ref"))
            assert np.array_equal(panel.pane(mine, "DAIN", H, W), panel.pane(theirs, "DAIN", H, W)), i
