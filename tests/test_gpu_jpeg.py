"""The JPEG encoder on the MI355X: rib_jpeg (csrc/jpeg.hip.h, Generator.jpeg / jpeg_into) byte for byte against the host
definition panel.jpeg_encode_host (tests/test_jpeg_cpu.py holds that one to PIL's decoder and tables), and the folder driver's
panel_encode="gpu" end to end on the native path.  Every comparison is exact."""
import os

import numpy as np
import pytest
import torch

import render_in_between_amd as rib
from render_in_between_amd import evaluator as ev, panel
from tests.test_gpu_quality import handle
from tests.test_jpeg_cpu import CONTENTS, SIZES, content
from tests.test_panels_cpu import parse_riff

pytestmark = pytest.mark.gpu

_WANT = {}


def want(kind, SH, SW, q):
    """The definition's file, computed once per case."""
    key = (kind, SH, SW, q)
    if key not in _WANT:
        _WANT[key] = panel.jpeg_encode_host(content(kind, SH, SW), q)
    return _WANT[key]


@pytest.mark.parametrize("q", [50, 90, 100])
@pytest.mark.parametrize("SH,SW", SIZES)
def test_device_files_equal_the_host_definition(SH, SW, q):
    G = handle()
    for kind in CONTENTS:                                         # T = 1
        got = G.jpeg(torch.from_numpy(content(kind, SH, SW)[None]).cuda(), q)
        assert len(got) == 1 and got[0] == want(kind, SH, SW, q), (kind, SH, SW, q)
    for k in range(2):                                            # T = 3: every content, at two positions
        kinds = [CONTENTS[(k + j) % 4] for j in range(3)] if k == 0 else [CONTENTS[3], CONTENTS[2], CONTENTS[0]]
        got = G.jpeg(torch.from_numpy(np.stack([content(c, SH, SW) for c in kinds])).cuda(), q)
        assert got == [want(c, SH, SW, q) for c in kinds], (kinds, SH, SW, q)


def test_a_wide_image_crosses_the_chunk_boundary():
    """More than one 16-MCU chunk per segment, the last one partial, an odd width and height: the carried bits and predictors."""
    G = handle()
    for kind, (SH, SW), q in (("noise", (19, 531), 100), ("gradient", (33, 257), 50), ("checker", (16, 272), 90)):
        a = content(kind, SH, SW)
        assert G.jpeg(torch.from_numpy(a[None]).cuda(), q) == [panel.jpeg_encode_host(a, q)], (kind, SH, SW)


def test_a_frame_alone_and_as_frame_two_of_three():
    G = handle()
    SH, SW = SIZES[-1]
    a = torch.from_numpy(np.stack([content(c, SH, SW) for c in ("noise", "sheet", "gradient")])).cuda()
    three = G.jpeg(a, 90)
    assert G.jpeg(a[1:2].contiguous(), 90)[0] == three[1] == want("sheet", SH, SW, 90)


def test_destination_inside_a_larger_buffer():
    G = handle()
    SH, SW = 40, 24
    kinds = ("sheet", "noise", "gradient")
    a = torch.from_numpy(np.stack([content(c, SH, SW) for c in kinds])).cuda()
    files = [want(c, SH, SW, 90) for c in kinds]
    cap = G.jpeg_max_bytes(SH, SW) + 5                            # an odd stride: every frame starts at another alignment
    assert cap - 5 == panel.jpeg_max_bytes(SH, SW)
    for off in (256, 4, 1, 7):
        buf = torch.full((off + 3 * cap + 64,), 77, dtype=torch.uint8, device="cuda")
        lengths = torch.full((5,), -7, dtype=torch.int32, device="cuda")
        assert G.jpeg_into(a, buf[off:off + 3 * cap], lengths[1:4], 90, cap) == cap
        host, n = buf.cpu().numpy(), lengths.cpu().tolist()
        assert n == [-7] + [len(f) for f in files] + [-7]
        for t in range(3):
            assert host[off + t * cap:off + t * cap + n[t + 1]].tobytes() == files[t], (off, t)
        assert (host[:off] == 77).all() and (host[off + 3 * cap:] == 77).all()              # nothing outside the strides


def test_a_cap_too_small_is_an_ordinary_refusal():
    G = handle()
    SH, SW = 40, 24
    noise, flat = content("noise", SH, SW), np.full((SH, SW, 3), 200, np.uint8)
    big = len(panel.jpeg_encode_host(noise, 100))
    small = len(panel.jpeg_encode_host(flat, 100))
    cap = big - 1
    assert small < cap
    a = torch.from_numpy(np.stack([flat, noise, flat])).cuda()
    buf = torch.full((16 + 3 * cap + 16,), 77, dtype=torch.uint8, device="cuda")
    lengths = torch.full((3,), -7, dtype=torch.int32, device="cuda")
    G.jpeg_into(a, buf[16:16 + 3 * cap], lengths, 100, cap)
    host = buf.cpu().numpy()
    assert lengths.cpu().tolist() == [small, 0, small]             # the noise frame is refused, its neighbours are not
    assert (host[16 + cap:16 + 2 * cap] == 77).all()               # a refused frame writes nothing
    assert host[16:16 + small].tobytes() == panel.jpeg_encode_host(flat, 100) == host[16 + 2 * cap:16 + 2 * cap + small].tobytes()
    assert (host[:16] == 77).all() and (host[16 + 3 * cap:] == 77).all()
    lengths.fill_(-7)
    G.jpeg_into(a, buf[16:16 + 3 * (cap + 1)], lengths, 100, cap + 1)                       # one byte more: it fits
    assert lengths.cpu().tolist() == [small, big, small]
    # the arguments the entry itself refuses: nothing is launched
    for kw in (dict(quality=0), dict(quality=101), dict(cap=100), dict(cap=cap + 100)):
        with pytest.raises(ValueError):
            G.jpeg_into(a, buf[16:16 + 3 * cap], lengths, **dict(dict(quality=90, cap=cap), **kw))
    with pytest.raises(ValueError):
        G.jpeg(a.float(), 90)
    from render_in_between_amd import _native
    L = _native.lib()
    ws = torch.empty(int(L.rib_jpeg_workspace_bytes(G._h, 3, SH, SW)), dtype=torch.uint8, device="cuda")
    ok = [3, SH, SW, a.data_ptr(), 90, buf.data_ptr(), cap, lengths.data_ptr(), ws.data_ptr()]
    for i, bad in ((0, 0), (1, 0), (2, 65536), (3, None), (4, 0), (4, 101), (5, None), (6, 630), (7, None), (8, None)):
        args = list(ok)
        args[i] = bad
        assert L.rib_jpeg(G._h, *args, None) == -1, i              # RIB_ERR_INVALID
        assert b"rib_jpeg" in L.rib_last_error(G._h)
    assert L.rib_jpeg_workspace_bytes(G._h, 0, SH, SW) == 0 and L.rib_jpeg_max_bytes(0, 5) == 0


def test_native_folder_driver_with_panel_encode_gpu(tmp_path):
    from tests.test_driver import _write_example
    from PIL import Image
    root = str(tmp_path)
    H = W = 128
    n = _write_example(root, n_key=3, rate=4, H=H, W=W)            # the clip of tests/test_gpu_panel.py, at its size
    G = handle()
    cfg = rib.AttrDict(gen=rib.hsm_gen_config(), model_height=H, model_width=W, gauss_sigma=5, skeleton_thres=0.001, foot_thres=0.001)
    dirs = [os.path.join(root, d) for d in ("inputs", "DAIN", "Predict_motion")]

    def run(name, io_mode="thread", **kw):
        out = os.path.join(root, name)
        E = ev.Evaluator(cfg, batch=2, chunk=2, lanes=1, io_mode=io_mode)
        return out, E.evaluate_from_folder(G, *dirs, out, panels=True, **kw)

    host_dir, host_w = run("host", panel_frames=True)
    host_again, _ = run("host_again", panel_frames=True, panel_encode="host")
    assert open(os.path.join(host_dir, "clipA.avi"), "rb").read() == open(os.path.join(host_again, "clipA.avi"), "rb").read()
    sheets = [np.asarray(Image.open(os.path.join(host_dir, "clipA_panels", "%04d.png" % i)).convert("RGB")) for i in range(n)]
    for i in range(n):                                             # host mode: PIL's files of the sheets, as before
        import io
        b = io.BytesIO()
        Image.fromarray(sheets[i]).save(b, format="JPEG", quality=90)
        ck = parse_riff(open(os.path.join(host_dir, "clipA.avi"), "rb").read())
        o, size = ck["movi/00dc"][i]
        assert open(os.path.join(host_dir, "clipA.avi"), "rb").read()[o:o + size] == b.getvalue(), i
    for io_mode, frames in (("thread", True), ("process", True), ("thread", False)):
        out, written = run("gpu_%s_%d" % (io_mode, frames), io_mode, panel_frames=frames, panel_encode="gpu", panel_quality=80)
        assert [os.path.relpath(w, out) for w in written] == [os.path.relpath(w, host_dir) for w in host_w] and len(written) == n
        for x, y in zip(written, host_w):
            assert open(x, "rb").read() == open(y, "rb").read(), x
        raw = open(os.path.join(out, "clipA.avi"), "rb").read()
        ck = parse_riff(raw)
        assert len(ck["movi/00dc"]) == n
        for i, (o, size) in enumerate(ck["movi/00dc"]):            # the sheets compose_host defines (the PNGs of the host run hold them)
            assert raw[o:o + size] == panel.jpeg_encode_host(sheets[i], 80), (io_mode, frames, i)
        if frames:
            assert sorted(os.listdir(os.path.join(out, "clipA_panels"))) == ["%04d.png" % i for i in range(n)]
            for i in range(n):
                assert np.array_equal(np.asarray(Image.open(os.path.join(out, "clipA_panels", "%04d.png" % i)).convert("RGB")), sheets[i])
        else:
            assert not os.path.exists(os.path.join(out, "clipA_panels"))
    with pytest.raises(ValueError, match="panels"):
        ev.Evaluator(cfg, batch=2, chunk=2, lanes=1).evaluate_from_folder(G, *dirs, os.path.join(root, "x"), panel_encode="gpu")
