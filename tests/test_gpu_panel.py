"""The diagnostic sheet on the MI355X: rib_panel (csrc/panel.hip.h, Generator.panel) bit for bit against the host definition
panel.compose_host (tests/test_panels_cpu.py holds that one to the reference's bytes), and the folder driver's panels=True end to
end on the native path.  Every comparison is exact."""
import os

import numpy as np
import pytest
import torch

import render_in_between_amd as rib
from render_in_between_amd import evaluator as ev, panel
from tests.test_gpu_quality import handle
from tests.test_panels_cpu import SIZES, make_inputs, parse_riff

pytestmark = pytest.mark.gpu


def dev(a):
    return {k: torch.from_numpy(v).cuda() for k, v in a.items()}


@pytest.mark.parametrize("T", [1, 5])
@pytest.mark.parametrize("H,W", SIZES)
def test_device_sheet_equals_the_host_definition(H, W, T):
    G = handle()
    a = make_inputs(T, H, W, seed=H + T)
    assert not any(np.isnan(v).any() for v in a.values())
    d = dev(a)
    titles = panel.title_bitmap(W)
    SH, SW = panel.layout(H, W)["sheet"]
    for tt in (None, titles):
        got = G.panel(d["pred"], d["mask"], d["fuse"], d["dain"], d["gt"], d["label"], titles=tt)
        assert got.shape == (T, SH, SW, 3) and got.dtype == torch.uint8 and got.is_cuda
        want = panel.compose_host(a["pred"], a["mask"], a["fuse"], a["dain"], a["gt"], a["label"], tt)
        assert np.array_equal(got.cpu().numpy(), want), (H, W, T, tt is not None)
        key = G.panel(None, None, None, d["dain"], d["gt"], d["label"], titles=tt)
        assert np.array_equal(key.cpu().numpy(), panel.compose_host(None, None, None, a["dain"], a["gt"], a["label"], tt)), (H, W, T, "key")
    # the Fuse pane is what the quantiser writes
    assert torch.equal(panel.pane(got, "Fuse", H, W), G.quantise(d["fuse"]))
    # a sheet's bytes do not depend on T
    one = G.panel(*(d[k][T - 1:] for k in ("pred", "mask", "fuse", "dain", "gt", "label")), titles=titles)
    assert torch.equal(one[0], got[T - 1])


def test_out_into_a_larger_buffer_odd_sizes_and_alignment():
    G = handle()
    H, W, T = 96, 160, 3
    a = make_inputs(T, H, W, seed=3)
    d = dev(a)
    titles = panel.title_bitmap(W)
    want = torch.from_numpy(panel.compose_host(a["pred"], a["mask"], a["fuse"], a["dain"], a["gt"], a["label"], titles))
    SH, SW = panel.layout(H, W)["sheet"]
    n = T * SH * SW * 3
    for off in (256, 4, 1, 7):            # a slice of a larger buffer: aligned, dword-aligned and byte-aligned starts
        buf = torch.full((off + n + 64,), 77, dtype=torch.uint8, device="cuda")
        dst = buf[off:off + n].view(T, SH, SW, 3)
        assert G.panel(d["pred"], d["mask"], d["fuse"], d["dain"], d["gt"], d["label"], titles=titles, out=dst) is dst
        assert torch.equal(dst.cpu(), want), off
        assert (buf[:off] == 77).all() and (buf[off + n:] == 77).all()                    # nothing outside the destination is touched
    # widths that are no multiple of 4 (scalar loads, byte writes) and tiny frames; label_nc = 3
    for (h, w) in ((5, 7), (33, 61), (64, 66)):
        b = make_inputs(2, h, w, seed=h, label_nc=3)
        e = dev(b)
        tt = panel.title_bitmap(w)
        got = G.panel(e["pred"], e["mask"], e["fuse"], e["dain"], e["gt"], e["label"], titles=tt)
        assert np.array_equal(got.cpu().numpy(), panel.compose_host(b["pred"], b["mask"], b["fuse"], b["dain"], b["gt"], b["label"], tt)), (h, w)
    # float sources off their 16-byte alignment
    flat = torch.zeros(T * 3 * H * W + 1, device="cuda")
    odd = flat[1:].view(T, 3, H, W)
    odd.copy_(d["fuse"])
    got = G.panel(d["pred"], d["mask"], odd, d["dain"], d["gt"], d["label"], titles=titles)
    assert torch.equal(got.cpu(), want)


def test_bad_arguments_raise():
    G = handle()
    H, W = 32, 48
    d = dev(make_inputs(2, H, W))
    with pytest.raises(ValueError):
        G.panel(d["pred"], None, d["fuse"], d["dain"], d["gt"], d["label"])              # only some of pred / mask / fuse
    with pytest.raises(ValueError):
        G.panel(d["pred"], d["mask"], d["fuse"], d["dain"], d["gt"][:1], d["label"])     # frame counts differ
    with pytest.raises(ValueError):
        G.panel(d["pred"], d["mask"], d["fuse"], d["dain"], d["gt"], d["label"][:, :2])  # no skeleton channels
    with pytest.raises(ValueError):
        G.panel(d["pred"], d["mask"], d["fuse"], d["dain"], d["gt"], d["label"], titles=np.zeros((2, 24, 10), np.uint8))
    with pytest.raises(ValueError):
        G.panel(d["pred"], d["mask"], d["fuse"], d["dain"], d["gt"], d["label"], out=torch.empty(2, 10, 10, 3, dtype=torch.uint8, device="cuda"))
    # the C ABI checks on its own: nothing is launched for any of these
    from render_in_between_amd import _native
    L = _native.lib()
    SH, SW = panel.layout(H, W)["sheet"]
    out = torch.empty(2, SH, SW, 3, dtype=torch.uint8, device="cuda")
    p = {k: v.data_ptr() for k, v in d.items()}
    ok = (2, H, W, 22, p["pred"], p["mask"], p["fuse"], p["dain"], p["gt"], p["label"], None, out.data_ptr())
    for i, bad in ((0, 0), (1, 0), (2, 4097), (3, 2), (4, None), (7, None), (9, None), (11, None)):
        args = list(ok)
        args[i] = bad
        assert L.rib_panel(G._h, *args, None) == -1, i                                    # RIB_ERR_INVALID
        assert b"rib_panel" in L.rib_last_error(G._h)


@pytest.mark.parametrize("io_mode", ["process", "thread"])
def test_native_folder_driver_with_panels(tmp_path, io_mode):
    from tests.test_driver import _write_example
    from PIL import Image
    root = str(tmp_path)
    H = W = 128
    n = _write_example(root, n_key=3, rate=4, H=H, W=W)                   # 9 frames: two 3-frame segments -> a chain of batch 2
    rng = np.random.default_rng(4)
    os.makedirs(os.path.join(root, "gt", "clipA"))
    for i in range(n):
        Image.fromarray(rng.integers(0, 255, (H, W, 3), dtype=np.uint8)).save(os.path.join(root, "gt", "clipA", "g%03d.png" % i))
    G = handle()
    cfg = rib.AttrDict(gen=rib.hsm_gen_config(), model_height=H, model_width=W, gauss_sigma=5, skeleton_thres=0.001, foot_thres=0.001)
    dirs = [os.path.join(root, d) for d in ("inputs", "DAIN", "Predict_motion")]
    gt_dir = os.path.join(root, "gt")
    entries = ("chain", "quantise", "quality", "panel", "rasterise", "resize_u8", "human_mask", "blend")
    calls, shown = [], []

    def counted(name):
        fn = getattr(G, name)

        def wrapper(*a, **k):
            calls.append((name, a[0] is None if name == "panel" else None))
            out = fn(*a, **k)
            if name == "chain":
                shown.append([x.clone() if x is not None else None for x in out])
            return out
        return wrapper

    def run(out, **kw):
        del calls[:], shown[:]
        for name in entries:
            setattr(G, name, counted(name))
        try:
            E = ev.Evaluator(cfg, batch=2, chunk=2, lanes=1, io_mode=io_mode)
            return E, E.evaluate_from_folder(G, *dirs, out, **kw), list(calls), list(shown)
        finally:
            for name in entries:
                delattr(G, name)

    for gt in (gt_dir, None):
        tag = "gt" if gt else "nogt"
        _, plain_w, plain_calls, _ = run(os.path.join(root, "plain_" + tag), gt_dir=gt)
        out = os.path.join(root, "with_" + tag)
        E, written, with_calls, chains = run(out, gt_dir=gt, panels=True, panel_frames=True)
        # the frames: byte-identical with and without panels
        assert [os.path.relpath(w, out) for w in written] == [os.path.relpath(w, os.path.join(root, "plain_" + tag)) for w in plain_w] and len(written) == n
        for x, y in zip(written, plain_w):
            assert open(x, "rb").read() == open(y, "rb").read(), x
        # launches: two units (time chunks [0,2) and [2,3) of the one group); each gains one panel launch for its chain frames,
        # the first one more in key-frame mode for the two key frames it starts from; the clip's last key frame is a unit of
        # its own (its label maps and one key-mode launch, after the units).  Nothing else is added.
        assert [c for c in with_calls if c[0] != "panel"] == plain_calls + [("rasterise", None)]
        assert [c[0] for c in with_calls][-2:] == ["rasterise", "panel"]
        assert [c for c in with_calls if c[0] == "panel"] == [("panel", False), ("panel", True), ("panel", False), ("panel", True)]
        assert [c[0] for c in with_calls][:4] == ["rasterise", "chain", "quantise", "panel"]
        # the video and the lossless sheets
        ck = parse_riff(open(os.path.join(out, "clipA.avi"), "rb").read())
        assert len(ck["movi/00dc"]) == n
        assert sorted(os.listdir(os.path.join(out, "clipA_panels"))) == ["%04d.png" % i for i in range(n)]
        SH, SW = panel.layout(H, W)["sheet"]
        sheets = [np.asarray(Image.open(os.path.join(out, "clipA_panels", "%04d.png" % i)).convert("RGB")) for i in range(n)]
        titles = panel.title_bitmap(W)
        for i in range(n):
            assert sheets[i].shape == (SH, SW, 3)
            assert np.array_equal(panel.pane(sheets[i], "Fuse", H, W), np.asarray(Image.open(written[i]))), i
            src = os.path.join(gt_dir, "clipA", "g%03d.png" % i) if gt else os.path.join(root, "inputs", "clipA", "%04d.png" % (i // 4))
            assert np.array_equal(panel.pane(sheets[i], "Ground Truth", H, W), panel.quantise_host(E.load_image(src)[0].numpy())), i
            dain = panel.quantise_host(E.load_image(os.path.join(root, "DAIN", "clipA", "f%03d.png" % i))[0].numpy())
            assert np.array_equal(panel.pane(sheets[i], "DAIN", H, W), dain), i
            if i % 4 == 0:
                assert np.array_equal(panel.pane(sheets[i], "Predict", H, W), panel.pane(sheets[i], "Fuse", H, W)) and (panel.pane(sheets[i], "Mask", H, W) == 0).all()
            assert (sheets[i][panel.layout(H, W)["titles"][0][0]:][:24][titles[0] != 0] == np.array([0, 0, 255], np.uint8)).all()
        # Predict and Mask panes of the generated frames: the chain's own outputs (unit 0: steps 0-1, unit 1: step 2; sample b = segment b)
        assert len(chains) == 2 and chains[0][0].shape == (2, 2, 3, H, W) and chains[1][1].shape == (1, 2, 1, H, W)
        for i in (1, 2, 3, 5, 6, 7):
            t, b = (i % 4) - 1, i // 4
            imgs, masks, _ = chains[0] if t < 2 else chains[1]
            t = t if t < 2 else 0
            assert np.array_equal(panel.pane(sheets[i], "Predict", H, W), panel.quantise_host(imgs[t, b].cpu().numpy())), i
            assert np.array_equal(panel.pane(sheets[i], "Mask", H, W), panel.mask_host(masks[t, b].cpu().numpy())), i
            assert sheets[i].std() > 10
    # with metrics in the same call: the values ride beside the sheets, the frames stay the same
    out = os.path.join(root, "both")
    E, written, both_calls, _ = run(out, gt_dir=gt_dir, panels=True, metrics=True)
    assert len(E.metrics) == 6 and os.path.exists(os.path.join(out, "metrics.json")) and os.path.exists(os.path.join(out, "clipA.avi"))
    assert not os.path.exists(os.path.join(out, "clipA_panels"))
    E2, written2, _, _ = run(os.path.join(root, "metrics_only"), gt_dir=gt_dir, metrics=True)
    assert E.metrics == E2.metrics
    for x, y in zip(written, written2):
        assert open(x, "rb").read() == open(y, "rb").read(), x
