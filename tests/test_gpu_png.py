"""The lossless PNG encoder on the MI355X (rib_png: Generator.png / png_into, csrc/png.hip.h) byte for byte against the definition
(png.encode_host) on the fixtures of tests/png_common.py, its refusals, and the folder driver's png_on="gpu" end to end on the
native path: the same names and pixels as the default run, the bytes the definition states.  Every comparison is exact."""
import os

import numpy as np
import pytest
import torch

from render_in_between_amd import evaluator as ev, png
from tests import png_common as C
from tests.test_gpu_quality import handle

pytestmark = pytest.mark.gpu

CASES = dict(C.cases())
_WANT = {}


def want(name):
    """The definition's files of a case's three frames, computed once."""
    if name not in _WANT:
        _WANT[name] = [png.encode_host(f) for f in CASES[name]]
    return _WANT[name]


@pytest.mark.parametrize("name", list(CASES))
def test_the_files_are_the_definitions(name):
    G = handle()
    x = torch.from_numpy(CASES[name]).cuda()
    got = G.png(x)
    for t in range(3):
        assert got[t] == want(name)[t], (name, t, len(got[t]), len(want(name)[t]))
    assert len(set(got)) == 3                                       # three frames that differ
    # a frame's bytes do not depend on T
    assert G.png(x[1:2].contiguous())[0] == got[1]
    assert G.png(x[1:3].contiguous()) == got[1:3]


def test_max_bytes_is_the_definitions():
    G = handle()
    for H, W in ((1, 1), (9, 5), (17, 64), (8, 4096), (1080, 1920), (65535, 1)):
        assert G.png_max_bytes(H, W) == png.max_bytes(H, W)
    for bad in ((0, 1), (1, 0), (65536, 1), (1, 4097)):
        with pytest.raises(ValueError):
            G.png_max_bytes(*bad)


def test_a_stride_too_small_is_an_ordinary_refusal():
    """A dst_stride one byte below the middle frame's size: that frame gets length 0 and its stride stays as it was; its
    neighbours, which are smaller, are written; nothing is written outside the strides or behind a file."""
    G = handle()
    noise = np.random.default_rng(7).integers(0, 256, (40, 64, 3), dtype=np.uint8)
    frames = np.stack([CASES["40x64-gradient"][0], noise, CASES["40x64-gradient"][1]])
    files = [png.encode_host(f) for f in frames]
    cap = len(files[1]) - 1
    assert len(files[0]) < cap and len(files[2]) < cap
    x = torch.from_numpy(frames).cuda()
    buf = torch.full((16 + 3 * cap + 16,), 77, dtype=torch.uint8, device="cuda")
    lengths = torch.full((3,), -7, dtype=torch.int32, device="cuda")
    assert G.png_into(x, buf[16:16 + 3 * cap], lengths, cap) == cap
    host = buf.cpu().numpy()
    assert lengths.cpu().tolist() == [len(files[0]), 0, len(files[2])]
    assert (host[16 + cap:16 + 2 * cap] == 77).all()               # a refused frame writes nothing
    for t in (0, 2):
        o = 16 + t * cap
        assert host[o:o + len(files[t])].tobytes() == files[t]
        assert (host[o + len(files[t]):o + cap] == 77).all()
    assert (host[:16] == 77).all() and (host[16 + 3 * cap:] == 77).all()
    # an exact fit is no refusal
    cap = len(files[1])
    buf.fill_(77)
    G.png_into(x, buf[16:16 + 3 * cap], lengths, cap)
    assert lengths.cpu().tolist() == [len(f) for f in files]
    assert buf.cpu().numpy()[16 + cap:16 + 2 * cap].tobytes() == files[1]


def test_bad_arguments_and_tables_launch_nothing():
    G = handle()
    H, W = 9, 5
    x = torch.from_numpy(CASES["9x5"]).cuda()
    cap = G.png_max_bytes(H, W)
    buf = torch.full((3 * cap,), 77, dtype=torch.uint8, device="cuda")
    lengths = torch.full((3,), -7, dtype=torch.int32, device="cuda")
    for bad in (x.float(), x[..., :2].contiguous(), x[0], x.transpose(1, 2), x.cpu()):
        with pytest.raises(ValueError):
            G.png(bad)
    for kw in (dict(cap=0), dict(cap=cap + 1), dict(cap=2 ** 31)):
        with pytest.raises(ValueError):
            G.png_into(x, buf, lengths, **kw)
    with pytest.raises(ValueError):
        G.png_into(x, buf, lengths[:2], cap)
    tables = png.TABLES.copy()
    tables[2, 7] -= 1                                               # over-subscribed
    with pytest.raises(RuntimeError, match="complete"):
        G.png_into(x, buf, lengths, cap, tables)
    tables = png.TABLES.copy()
    tables[0] = png.TABLES[3]                                       # complete, but table 0 is no longer flat
    with pytest.raises(RuntimeError, match="flat"):
        G.png_into(x, buf, lengths, cap, tables)
    with pytest.raises(ValueError):
        G.png_into(x, buf, lengths, cap, png.TABLES[:, :285])
    from render_in_between_amd import _native
    L = _native.lib()
    assert L.rib_png_max_bytes(0, 1) == 0 and L.rib_png_max_bytes(1, 4097) == 0 and L.rib_png_workspace_bytes(G._h, 0, H, W) == 0
    ws = torch.empty(int(L.rib_png_workspace_bytes(G._h, 3, H, W)), dtype=torch.uint8, device="cuda")
    tab = np.ascontiguousarray(png.TABLES)
    K = tab.shape[0]
    ok = [3, H, W, x.data_ptr(), tab.ctypes.data, K, buf.data_ptr(), cap, lengths.data_ptr(), ws.data_ptr()]
    for i, bad in ((0, 0), (0, 65536), (1, 0), (1, 65536), (2, 0), (2, 4097), (3, None), (4, None), (5, 0), (5, 17), (6, None), (7, 0),
                   (7, 2 ** 31), (8, None), (8, lengths.data_ptr() + 2), (9, None), (9, ws.data_ptr() + 8)):
        args = list(ok)
        args[i] = bad
        assert L.rib_png(G._h, *args, None) == -1, (i, bad)           # RIB_ERR_INVALID
        assert b"rib_png" in L.rib_last_error(G._h), (i, bad)
    torch.cuda.synchronize()
    assert (buf == 77).all() and lengths.cpu().tolist() == [-7, -7, -7]
    # other tables are other files, and the first tables come back unchanged
    one = G.png(x)
    flat_only = G.png(x, png.TABLES[:1])
    assert flat_only == [png.encode_host(f, tables=png.TABLES[:1]) for f in CASES["9x5"]]
    assert G.png(x) == one == want("9x5")


# ---- the folder driver ---------------------------------------------------------------------------------------------------------
def tree(out):
    return {os.path.relpath(os.path.join(d, f), out): open(os.path.join(d, f), "rb").read() for d, _, fs in os.walk(out) for f in fs}


def check_pngs(gpu_tree, host_tree):
    """Every PNG of the default run is there under the same name, holds the same pixels, and is the definition's file of them."""
    import io
    from PIL import Image
    pngs = [n for n in host_tree if n.endswith(".png")]
    assert pngs and sorted(gpu_tree) == sorted(host_tree)
    for n in pngs:
        pixels = np.asarray(Image.open(io.BytesIO(host_tree[n])).convert("RGB"))
        assert gpu_tree[n] == png.encode_host(pixels), n
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(gpu_tree[n]))), pixels), n
    return pngs


def test_native_folder_driver_png_on_gpu(tmp_path):
    """64x64, two clips of 3 key frames at rate 4, batch 2, chunk 2 (first and later chunks, a loose last key frame): with
    png_on="gpu" the tree has the default run's names, every PNG holds the default run's pixels and is png.encode_host of them;
    with threads and with worker processes; combined with video=True the .avi is the default run's."""
    from tests.test_driver import _write_example
    from tests.test_gpu_video import cfg64
    root = str(tmp_path)
    n = _write_example(root, n_key=3, rate=4, H=64, W=64, clip="clipA", seed=0)
    _write_example(root, n_key=3, rate=4, H=64, W=64, clip="clipB", seed=5)
    G = handle()
    dirs = [os.path.join(root, d) for d in ("inputs", "DAIN", "Predict_motion")]

    def run(name, io_mode="thread", **kw):
        out = os.path.join(root, name)
        return out, ev.Evaluator(cfg64(), batch=2, chunk=2, lanes=1, io_mode=io_mode).evaluate_from_folder(G, *dirs, out, **kw)

    host, host_w = run("host")
    gpu, gpu_w = run("gpu", png_on="gpu")
    assert [os.path.relpath(w, gpu) for w in gpu_w] == [os.path.relpath(w, host) for w in host_w] and len(gpu_w) == 2 * n == 18
    assert len(check_pngs(tree(gpu), tree(host))) == 2 * n
    proc, proc_w = run("gpu_process", "process", png_on="gpu")
    assert tree(proc) == tree(gpu) and [os.path.relpath(w, proc) for w in proc_w] == [os.path.relpath(w, gpu) for w in gpu_w]
    explicit, _ = run("explicit", png_on="host")
    assert tree(explicit) == tree(host)
    # combined with the video: the frames' .avi is the default run's, the PNGs are the GPU's
    vhost, _ = run("video_host", video=True, video_quality=80)
    vgpu, vgpu_w = run("video_gpu", video=True, video_quality=80, png_on="gpu")
    a, b = tree(vgpu), tree(vhost)
    assert sorted(a) == sorted(b) and "clipA_video.avi" in a and "clipB_video.avi" in a
    for c in ("clipA", "clipB"):
        assert a[c + "_video.avi"] == b[c + "_video.avi"]
    assert {k: v for k, v in a.items() if k.endswith(".png")} == {k: v for k, v in tree(gpu).items() if k.endswith(".png")}
    assert [os.path.relpath(w, vgpu) for w in vgpu_w] == [os.path.relpath(w, gpu) for w in gpu_w]


def test_native_folder_driver_png_on_gpu_at_the_source_size(tmp_path):
    """64x64 model, 96x80 DAIN frames and key frames, resize_on="gpu", output_size="source": the PNGs are rib_png of
    rib_composite's bytes and of the key files' own pixels - the default run's pixels under the default run's names."""
    from PIL import Image
    from tests.composite_common import write_example
    from tests.test_gpu_video import cfg64
    root = str(tmp_path)
    n = write_example(root, n_key=3, rate=4, key_hw=(80, 96), dain_hw=(80, 96), clip="clipA", seed=1)
    G = handle()
    dirs = [os.path.join(root, d) for d in ("inputs", "DAIN", "Predict_motion")]

    def run(name, **kw):
        out = os.path.join(root, name)
        E = ev.Evaluator(cfg64(), batch=2, chunk=2, lanes=1, resize_on="gpu")
        return out, E.evaluate_from_folder(G, *dirs, out, output_size="source", **kw)

    host, host_w = run("host")
    gpu, gpu_w = run("gpu", png_on="gpu")
    assert [os.path.relpath(w, gpu) for w in gpu_w] == [os.path.relpath(w, host) for w in host_w] and len(gpu_w) == n == 9
    assert len(check_pngs(tree(gpu), tree(host))) == n
    assert np.asarray(Image.open(gpu_w[1])).shape == (80, 96, 3)
