"""Ground-truth PSNR / SSIM (no GPU): the torch statement of the metric (metrics.py, Evaluator.compute_metrics) against an
independent fp64 restatement of piq's defaults written here with the 2-D window, and the folder driver's metrics output
(metrics.json) with a CPU model behind the reference's call protocol, in one process and under a world-2 process group."""
import importlib.util
import json
import math
import os
import socket

import numpy as np
import pytest
import torch
import torch.nn.functional as F
import torch.multiprocessing as mp

import render_in_between_amd as rib
from render_in_between_amd import evaluator as ev, synth
from oracle import generator_ref
from tests.test_driver import MID_CFG, _write_example, oracle_labels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def restated(pred, target, mask=None):
    """piq psnr(data_range=1, reduction='none') / ssim(data_range=1) per frame of the reference's compute_metrics inputs
    (PGNR/models/evaluator.py:149-163), fp64, 2-D 11x11 gaussian window."""
    x = torch.clamp(pred.double() * 0.5 + 0.5, 0, 1)
    y = torch.clamp(target.double() * 0.5 + 0.5, 0, 1)
    if mask is not None:
        m = mask.double().unsqueeze(1).repeat(1, 3, 1, 1)
        x, y = x * m, y * m
    psnr = -10 * torch.log10(((x - y) ** 2).mean(dim=(1, 2, 3)) + 1e-8)
    f = max(1, round(min(x.shape[-2:]) / 256))
    if f > 1:
        x, y = F.avg_pool2d(x, kernel_size=f), F.avg_pool2d(y, kernel_size=f)
    if x.shape[-1] < 11 or x.shape[-2] < 11:
        raise ValueError("smaller than the window")
    c = torch.arange(11, dtype=torch.float64) - 5
    g = c ** 2
    g = (-(g.unsqueeze(0) + g.unsqueeze(1)) / (2 * 1.5 ** 2)).exp()
    g = (g / g.sum()).view(1, 1, 11, 11).repeat(3, 1, 1, 1)
    conv = lambda t: F.conv2d(t, g, groups=3)                                  # noqa: E731
    mx, my = conv(x), conv(y)
    sxx, syy, sxy = conv(x * x) - mx ** 2, conv(y * y) - my ** 2, conv(x * y) - mx * my
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    cs = (2 * sxy + c2) / (sxx + syy + c2)
    smap = (2 * mx * my + c1) / (mx ** 2 + my ** 2 + c1) * cs
    return psnr, smap.mean(dim=(1, 2, 3))


def frames(kind, B, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    if kind == "random":
        return torch.rand(B, 3, H, W, generator=g) * 2 - 1
    if kind == "smooth":
        yy, xx = torch.meshgrid(torch.linspace(0, 3, H), torch.linspace(0, 4, W), indexing="ij")
        ph = torch.rand(B, 3, 1, 1, generator=g) * 6
        return torch.sin(xx + yy * 0.7 + ph) * 0.8 + 0.05 * torch.randn(B, 3, H, W, generator=g)
    if kind == "wide":                                                        # out of range: clamped
        return torch.randn(B, 3, H, W, generator=g) * 2
    raise ValueError(kind)


def test_downsample_factor_table():
    from render_in_between_amd.metrics import downsample_factor
    table = {(64, 64): 1, (320, 480): 1, (384, 384): 2, (512, 512): 2, (640, 640): 2, (896, 896): 4, (1024, 1024): 4}
    for (h, w), f in table.items():
        assert downsample_factor(h, w) == f, (h, w)


@pytest.mark.parametrize("shape", [(64, 64), (96, 160), (320, 480), (512, 512)])
@pytest.mark.parametrize("kind", ["random", "smooth", "wide", "masked"])
def test_compute_metrics_matches_the_restatement(shape, kind):
    H, W = shape
    B = 2
    E = ev.Evaluator(rib.AttrDict(gen=rib.hsm_gen_config(), model_height=H, model_width=W))
    base = "smooth" if kind == "masked" else kind
    a = frames(base, B, H, W, 1)
    b = (a + 0.1 * torch.randn(B, 3, H, W, generator=torch.Generator().manual_seed(2))) if base == "smooth" else frames(base, B, H, W, 2)
    mask = (torch.rand(B, H, W, generator=torch.Generator().manual_seed(3)) > 0.3).float() if kind == "masked" else None
    from render_in_between_amd import metrics
    p, s = metrics.psnr_ssim(a, b, mask)
    rp, rs = restated(a, b, mask)
    assert p.shape == s.shape == (B,)
    assert (p.double() - rp).abs().max() <= 1e-4 and (s.double() - rs).abs().max() <= 1e-6, (p, rp, s, rs)
    mp_, ms_ = E.compute_metrics(a, b, mask)
    assert mp_.dim() == ms_.dim() == 0
    assert abs(float(mp_) - float(rp.mean())) <= 1e-4 and abs(float(ms_) - float(rs.mean())) <= 1e-6


def test_identical_frames_and_small_frames():
    E = ev.Evaluator(rib.AttrDict(gen=rib.hsm_gen_config(), model_height=64, model_width=64))
    a = frames("random", 3, 64, 64, 4)
    p, s = E.compute_metrics(a, a.clone())
    assert float(p) == 80.0 and float(s) == 1.0
    with pytest.raises(ValueError):
        E.compute_metrics(frames("random", 1, 8, 8, 0), frames("random", 1, 8, 8, 1))
    p, s = E.compute_metrics(frames("random", 1, 16, 16, 0), frames("random", 1, 16, 16, 1))
    assert math.isfinite(float(p)) and math.isfinite(float(s))


def _cfg(H=32, W=48):
    return rib.AttrDict(gen=rib.hsm_gen_config(**MID_CFG), model_height=H, model_width=W, gauss_sigma=5,
                        skeleton_thres=0.001, foot_thres=0.001)


def _write_gt(root, n, H=32, W=48, clip="clipA", seed=11, masks=False):
    from PIL import Image
    rng = np.random.default_rng(seed)
    os.makedirs(os.path.join(root, "gt", clip), exist_ok=True)
    for i in range(n):
        Image.fromarray(rng.integers(0, 255, (H, W, 3), dtype=np.uint8)).save(os.path.join(root, "gt", clip, "g%03d.png" % i))
    if masks:
        os.makedirs(os.path.join(root, "masks", clip), exist_ok=True)
        for i in range(n):
            Image.fromarray(rng.integers(0, 255, (H, W), dtype=np.uint8)).save(os.path.join(root, "masks", clip, "m%03d.png" % i))


class _Model:
    """The reference's call protocol over the CPU oracle; keeps every fused frame the driver will form."""

    def __init__(self, R):
        self.R, self.fused = R, []

    def eval(self):
        return self

    def __call__(self, label, label_prev, dain, prev):
        img, mask = self.R(label, label_prev, dain, prev)
        self.fused.append(img * mask.repeat(1, 3, 1, 1) + dain * (1 - mask.repeat(1, 3, 1, 1)))
        return img, mask


@pytest.mark.parametrize("masks", [False, True])
def test_folder_metrics_match_the_restatement(tmp_path, masks):
    from PIL import Image
    root = str(tmp_path)
    n = _write_example(root, n_key=2, rate=4)                  # frames 0..4: key frames 0 and 4, one segment 1..3
    _write_gt(root, n, masks=masks)
    cfg = _cfg()
    spec = rib.GenSpec.from_cfg(cfg.gen)
    R = generator_ref.RefGenerator(spec, synth.make_state_dict(spec, 2))
    dirs = [os.path.join(root, d) for d in ("inputs", "DAIN", "Predict_motion")]
    E = ev.Evaluator(cfg, label_fn=oracle_labels)
    M = _Model(R)
    out = os.path.join(root, "m")
    written = E.evaluate_from_folder(M, *dirs, out, gt_dir=os.path.join(root, "gt"), metrics=True,
                                     mask_dir=os.path.join(root, "masks") if masks else None)
    assert len(written) == n
    with open(os.path.join(out, "metrics.json")) as f:
        rep = json.load(f)
    pf = rep["clips"]["clipA"]["per_frame"]
    assert [r["i"] for r in pf] == [1, 2, 3] and [r["file"] for r in pf] == ["f001.png", "f002.png", "f003.png"]
    assert rep["clips"]["clipA"]["frames"] == 3 and rep["overall"]["frames"] == 3 and len(M.fused) == 3
    assert len(E.metrics) == 3 and E.metrics[0]["clip"] == "clipA"
    for k in ("DAIN_PSNR", "DAIN_SSIM", "OURS_PSNR", "OURS_SSIM"):
        assert abs(rep["clips"]["clipA"][k] - np.mean([r[k] for r in pf])) < 1e-9
        assert abs(rep["overall"][k] - rep["clips"]["clipA"][k]) < 1e-12
    assert "unpinned" in rep["protocol"]["source"]
    for t, r in enumerate(pf):
        i = r["i"]
        gt = E.load_image(os.path.join(root, "gt", "clipA", "g%03d.png" % i))[0].unsqueeze(0)
        dain = E.load_image(os.path.join(root, "DAIN", "clipA", "f%03d.png" % i))[0].unsqueeze(0)
        mk = None
        if masks:
            mk = torch.from_numpy((np.asarray(Image.open(os.path.join(root, "masks", "clipA", "m%03d.png" % i))) > 127).astype(np.float32)).unsqueeze(0)
        dp, ds = restated(dain, gt, mk)
        op, os_ = restated(M.fused[t], gt, mk)
        assert abs(r["DAIN_PSNR"] - float(dp)) <= 1e-4 and abs(r["DAIN_SSIM"] - float(ds)) <= 1e-6
        assert abs(r["OURS_PSNR"] - float(op)) <= 1e-4 and abs(r["OURS_SSIM"] - float(os_)) <= 1e-6
    # metrics=False: the same files, byte for byte, and no report
    out2 = os.path.join(root, "plain")
    E2 = ev.Evaluator(cfg, label_fn=oracle_labels)
    written2 = E2.evaluate_from_folder(_Model(R), *dirs, out2, gt_dir=os.path.join(root, "gt"))
    assert [os.path.relpath(w, out2) for w in written2] == [os.path.relpath(w, out) for w in written]
    for a, b in zip(written, written2):
        assert open(a, "rb").read() == open(b, "rb").read()
    assert not os.path.exists(os.path.join(out2, "metrics.json")) and E2.metrics is None


def test_folder_metrics_arguments_are_checked(tmp_path):
    root = str(tmp_path)
    n = _write_example(root, n_key=2, rate=2)
    _write_gt(root, n)
    cfg = _cfg()
    spec = rib.GenSpec.from_cfg(cfg.gen)
    M = _Model(generator_ref.RefGenerator(spec, synth.make_state_dict(spec, 2)))
    dirs = [os.path.join(root, d) for d in ("inputs", "DAIN", "Predict_motion")]
    E = ev.Evaluator(cfg, label_fn=oracle_labels)
    with pytest.raises(ValueError, match="gt_dir"):
        E.evaluate_from_folder(M, *dirs, os.path.join(root, "a"), metrics=True)
    with pytest.raises(ValueError, match="mask_dir"):
        E.evaluate_from_folder(M, *dirs, os.path.join(root, "b"), gt_dir=os.path.join(root, "gt"), mask_dir=os.path.join(root, "gt"))
    # a mask at another size than the model's is an error (masks are not resized)
    from PIL import Image
    os.makedirs(os.path.join(root, "masks", "clipA"))
    for i in range(n):
        Image.fromarray(np.zeros((16, 24), np.uint8)).save(os.path.join(root, "masks", "clipA", "m%03d.png" % i))
    with pytest.raises(ValueError, match="resized"):
        E.evaluate_from_folder(M, *dirs, os.path.join(root, "c"), gt_dir=os.path.join(root, "gt"), metrics=True,
                               mask_dir=os.path.join(root, "masks"))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _metrics_worker(rank, world, port, root, q):
    import torch.distributed as dist
    from render_in_between_amd import distributed as ribdist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    ribdist.init_process_group("gloo")
    torch.set_num_threads(2)
    cfg = _cfg()
    spec = rib.GenSpec.from_cfg(cfg.gen)
    M = _Model(generator_ref.RefGenerator(spec, synth.make_state_dict(spec, 2)))
    E = ev.Evaluator(cfg, label_fn=oracle_labels)
    dirs = [os.path.join(root, d) for d in ("inputs", "DAIN", "Predict_motion")]
    E.evaluate_from_folder(M, *dirs, os.path.join(root, "sharded"), gt_dir=os.path.join(root, "gt"), metrics=True)
    q.put((rank, len(E.metrics)))
    dist.barrier()
    dist.destroy_process_group()


def test_folder_metrics_of_two_ranks_equal_one_rank(tmp_path):
    root = str(tmp_path)
    n = _write_example(root, n_key=4, rate=2)                  # 7 frames: 3 one-frame segments, dealt to 2 ranks
    _write_gt(root, n)
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_metrics_worker, args=(r, world, port, root, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=300) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert res == [(0, 3), (1, 3)]                               # every rank holds the merged records
    cfg = _cfg()
    spec = rib.GenSpec.from_cfg(cfg.gen)
    M = _Model(generator_ref.RefGenerator(spec, synth.make_state_dict(spec, 2)))
    dirs = [os.path.join(root, d) for d in ("inputs", "DAIN", "Predict_motion")]
    ev.Evaluator(cfg, label_fn=oracle_labels).evaluate_from_folder(M, *dirs, os.path.join(root, "single"), gt_dir=os.path.join(root, "gt"),
                                                                   metrics=True, rank=0, world=1)
    with open(os.path.join(root, "sharded", "metrics.json")) as f:
        two = json.load(f)
    with open(os.path.join(root, "single", "metrics.json")) as f:
        one = json.load(f)
    assert [r["i"] for r in two["clips"]["clipA"]["per_frame"]] == [1, 3, 5]
    assert two["clips"]["clipA"]["per_frame"] == one["clips"]["clipA"]["per_frame"]       # bit-equal values
    assert not os.path.exists(os.path.join(root, "sharded", "metrics_rank1.json"))


def _inference_module():
    p = os.path.join(ROOT, "render-in-between_amd", "inference.py")
    spec = importlib.util.spec_from_file_location("rib_inference_quality", p)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_cli_metrics_flags():
    mod = _inference_module()
    with pytest.raises(SystemExit):
        mod.parse_args(["--input-dir", "x", "--metrics"])
    with pytest.raises(SystemExit):
        mod.parse_args(["--input-dir", "x", "--gt-dir", "g", "--mask-dir", "m"])
    o = mod.parse_args(["--input-dir", "x", "--gt-dir", "g", "--metrics", "--mask-dir", "m"])
    assert o.metrics and o.gt_dir == "g" and o.mask_dir == "m"
    o = mod.parse_args(["--input-dir", "x"])
    assert not o.metrics and o.gt_dir is None
    E = ev.Evaluator(rib.AttrDict(gen=rib.hsm_gen_config(), model_height=320, model_width=480))
    E.timings = {"frames": 10, "wall": 1.0, "metrics": 0.25}
    E.metrics_report = {"overall": {"frames": 8, "DAIN_PSNR": 20.5, "DAIN_SSIM": 0.5, "OURS_PSNR": 21.25, "OURS_SSIM": 0.625}}
    line = mod.summary_line(E)
    for part in ("metrics over 8 frames", "DAIN PSNR 20.5000", "OURS PSNR 21.2500 SSIM 0.625000", "metric time 0.25 s"):
        assert part in line, (part, line)
