"""The JPEG definition of the sheet video under panel_encode="gpu" (panel.jpeg_encode_host; numpy only, no GPU): PIL decodes
every file and finds its own tables in it, the marker structure is what the docstring states, distortion and size stay within a
stated margin of PIL's own encoder at the same tables, and the rare branches of the coder are reached by the inputs.  The HIP
kernels are held to these bytes in tests/test_gpu_jpeg.py."""
import io
import os
import struct

import numpy as np
import pytest

from render_in_between_amd import panel
from tests.test_panels_cpu import make_inputs, parse_riff

SIZES = [(1, 1), (8, 8), (16, 16), (17, 33), (40, 24), panel.layout(32, 32)["sheet"]]
CONTENTS = ("sheet", "gradient", "noise", "checker")
# fidelity against PIL's encoder at the same tables (test_fidelity_against_pil): twice the largest deficit observed over
# contents "sheet" and "gradient", all SIZES, quality 50 and 90 (DESIGN 4f lists the observations); the caps are 0.5 dB and 10 %
PSNR_MARGIN_DB = 0.096
SIZE_MARGIN = 0.10

_SHEET = None


def content(kind, SH, SW):
    """uint8 [SH, SW, 3].  sheet: the top-left SH x SW of a composed six-pane sheet of 32 x 32 panes (gutter, title bar and text, the Predict pane), all of it at the last size; gradient: a
    smooth two-axis gradient crossed by 1-pixel coloured lines; noise: uniform noise; checker: black / white squares of 8 px."""
    global _SHEET
    if kind == "sheet":
        if _SHEET is None:
            a = make_inputs(1, 32, 32, seed=7)
            _SHEET = panel.compose_host(a["pred"], a["mask"], a["fuse"], a["dain"], a["gt"], a["label"], panel.title_bitmap(32))[0]
        assert _SHEET.shape[:2] == SIZES[-1]
        return np.ascontiguousarray(_SHEET[:SH, :SW])
    y, x = np.mgrid[0:SH, 0:SW]
    if kind == "gradient":
        a = np.stack([(x * 255) // max(SW - 1, 1), (y * 255) // max(SH - 1, 1), ((x + y) * 255) // max(SH + SW - 2, 1)], -1).astype(np.uint8)
        a[5::11, :] = (255, 0, 0)
        a[:, 3::13] = (0, 255, 64)
        return a
    if kind == "noise":
        return np.random.default_rng(SH * 1000 + SW).integers(0, 256, (SH, SW, 3), dtype=np.uint8)
    if kind == "checker":
        return np.repeat((((y // 8 + x // 8) % 2) * 255).astype(np.uint8)[..., None], 3, -1)
    raise KeyError(kind)


def quality_of(kind):
    return 100 if kind in ("noise", "checker") else 90


def cases():
    return [(kind, SH, SW) for kind in CONTENTS for (SH, SW) in SIZES]


def walk(data):
    """Our own marker walk: -> (segments [(marker, payload)] up to and including SOS, the entropy-coded bytes, the tail)."""
    assert data[:2] == b"\xff\xd8"
    segs, i = [], 2
    while True:
        assert data[i] == 0xFF, i
        m = data[i + 1]
        n = struct.unpack(">H", data[i + 2:i + 4])[0]
        segs.append((m, data[i + 4:i + 2 + n]))
        i += 2 + n
        if m == 0xDA:
            break
    assert data[-2:] == b"\xff\xd9"
    return segs, data[i:-2]


def decode(data):
    from PIL import Image
    im = Image.open(io.BytesIO(data))
    im.load()
    return im


def pil_encode(a, q):
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(a).save(b, format="JPEG", quality=q, subsampling=2)
    return b.getvalue()


def psnr(a, b):
    mse = np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2)
    return 10 * np.log10(255.0 ** 2 / max(mse, 1e-12))


def test_the_inputs_reach_the_rare_branches():
    tot = {"stuffed": 0, "zrl": 0, "no_eob": 0, "max_dc_category": 0, "segments": 0}
    most_segments = 0
    for kind, SH, SW in cases():
        for q in {quality_of(kind), 50}:
            data, st = panel.jpeg_encode_host(content(kind, SH, SW), q, stats=True)
            assert st["segments"] == (SH + 15) // 16
            for k in ("stuffed", "zrl", "no_eob"):
                tot[k] += st[k]
            tot["max_dc_category"] = max(tot["max_dc_category"], st["max_dc_category"])
            most_segments = max(most_segments, st["segments"])
            assert data.count(b"\xff\x00") >= st["stuffed"] - 1
    print(tot, most_segments)
    assert tot["stuffed"] >= 1 and tot["zrl"] >= 1 and tot["no_eob"] >= 1 and tot["max_dc_category"] >= 10 and most_segments >= 9


@pytest.mark.parametrize("q", [1, 50, 90, 100])
def test_pil_decodes_every_file_and_finds_its_own_tables(q):
    for kind, SH, SW in cases():
        a = content(kind, SH, SW)
        im = decode(panel.jpeg_encode_host(a, q))
        assert im.format == "JPEG" and im.size == (SW, SH) and im.mode == "RGB"
        from PIL import JpegImagePlugin
        assert JpegImagePlugin.get_sampling(im) == 2
        theirs = decode(pil_encode(a, q))
        assert {k: list(v) for k, v in im.quantization.items()} == {k: list(v) for k, v in theirs.quantization.items()}, (kind, SH, SW)
        assert np.asarray(im).shape == (SH, SW, 3)


def test_the_huffman_tables_are_the_ones_pil_writes():
    ours = [p for m, p in walk(panel.jpeg_encode_host(content("noise", 16, 16), 90))[0] if m == 0xC4]
    theirs = [p for m, p in walk(pil_encode(content("noise", 16, 16), 90))[0] if m == 0xC4]
    assert len(ours) == 4 and ours == theirs


def test_structure_determinism_and_batch_independence():
    for kind, SH, SW in cases():
        a = content(kind, SH, SW)
        q = quality_of(kind)
        data = panel.jpeg_encode_host(a, q)
        segs, ecs = walk(data)
        assert [m for m, _ in segs] == [0xE0, 0xDB, 0xDB, 0xC0, 0xC4, 0xC4, 0xC4, 0xC4, 0xDD, 0xDA]
        assert data[:panel.JPEG_HEADER_BYTES] == panel.jpeg_header(SH, SW, q) and len(data) <= panel.jpeg_max_bytes(SH, SW)
        by = dict((m, p) for m, p in segs if m not in (0xDB, 0xC4))
        assert by[0xE0] == b"JFIF\0\x01\x01\x00\x00\x01\x00\x01\x00\x00"
        assert by[0xC0] == struct.pack(">BHHB", 8, SH, SW, 3) + bytes((1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1))
        assert [p[0] for m, p in segs if m == 0xDB] == [0, 1] and [p[0] for m, p in segs if m == 0xC4] == [0x00, 0x10, 0x01, 0x11]
        cols, rows = (SW + 15) // 16, (SH + 15) // 16
        assert struct.unpack(">H", by[0xDD])[0] == cols
        assert by[0xDA] == bytes((3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0))
        # entropy-coded data: 0xFF is followed by 0x00 or by the next RSTn, nothing else
        rst = []
        i = 0
        while i < len(ecs):
            if ecs[i] == 0xFF:
                assert i + 1 < len(ecs) and (ecs[i + 1] == 0 or 0xD0 <= ecs[i + 1] <= 0xD7), (kind, SH, SW, i)
                if ecs[i + 1]:
                    rst.append(ecs[i + 1] - 0xD0)
                i += 1
            i += 1
        assert rst == [k % 8 for k in range(rows - 1)]
        for part in ecs.replace(b"\xff\x00", b"").split(b"\xff"):
            assert len(part) >= 1                                       # no empty segment
        assert all(len(s) <= panel.jpeg_segment_bound(SW) for s in _split_segments(ecs))
        assert panel.jpeg_encode_host(a.copy(), q) == data
        other = content("noise", SH, SW)
        batch = panel.jpeg_encode_host(np.stack([other, other[::-1], a]), q)
        assert isinstance(batch, list) and len(batch) == 3 and batch[2] == data


def _split_segments(ecs):
    out, cur, i = [], bytearray(), 0
    while i < len(ecs):
        if ecs[i] == 0xFF and ecs[i + 1] != 0:
            out.append(bytes(cur))
            cur = bytearray()
            i += 2
            continue
        cur.append(ecs[i])
        i += 1
    out.append(bytes(cur))
    return out


def test_fidelity_against_pil():
    """Same tables, so distortion and size must be close to PIL's encoder (libjpeg's float-free DCT, no restart markers)."""
    worst_db, worst_size = -1e9, -1e9
    for kind in ("sheet", "gradient"):
        for SH, SW in SIZES:
            a = content(kind, SH, SW)
            for q in (50, 90):
                ours, theirs = panel.jpeg_encode_host(a, q), pil_encode(a, q)
                d_db = psnr(decode(theirs), a) - psnr(decode(ours), a)
                d_size = len(ours) / len(theirs) - 1.0
                print("%-8s %3dx%-3d q%-3d PSNR ours %.3f PIL %.3f (deficit %+.3f dB)  bytes ours %d PIL %d (%+.2f %%)"
                      % (kind, SH, SW, q, psnr(decode(ours), a), psnr(decode(theirs), a), d_db, len(ours), len(theirs), 100 * d_size))
                worst_db, worst_size = max(worst_db, d_db), max(worst_size, d_size)
                assert d_db <= PSNR_MARGIN_DB, (kind, SH, SW, q, d_db)
                assert d_size <= SIZE_MARGIN, (kind, SH, SW, q, d_size)
    print("largest deficits: %.4f dB, %.2f %%" % (worst_db, 100 * worst_size))
    assert PSNR_MARGIN_DB <= 0.5 and SIZE_MARGIN <= 0.10


def test_bad_arguments_are_refused():
    a = content("gradient", 16, 16)
    for q in (0, 101, 90.5, True):
        with pytest.raises(ValueError):
            panel.jpeg_encode_host(a, q)
    with pytest.raises(ValueError):
        panel.jpeg_encode_host(a.astype(np.float32), 90)
    with pytest.raises(ValueError):
        panel.jpeg_encode_host(a[..., :2], 90)
    with pytest.raises(ValueError):
        panel.jpeg_encode_host(a[0], 90)
    with pytest.raises(ValueError):
        panel.jpeg_encode_host(np.zeros((0, 4, 3), np.uint8), 90)


def test_avi_round_trip_of_our_files(tmp_path):
    SH, SW = SIZES[-1]
    files = [panel.jpeg_encode_host(content(k, SH, SW), 90) for k in ("sheet", "gradient", "noise")]
    paths = [panel.save_jpeg(d, str(tmp_path / ("%04d.jpg" % i))) for i, d in enumerate(files)]
    out = panel.write_mjpeg_avi(paths, str(tmp_path / "clip.avi"), 30)
    raw = open(out, "rb").read()
    ck = parse_riff(raw)
    assert len(ck["movi/00dc"]) == 3
    for (off, size), d in zip(ck["movi/00dc"], files):
        assert raw[off:off + size] == d
    o, n = ck["hdrl/avih"][0]
    avih = struct.unpack("<14I", raw[o:o + n])
    assert avih[4] == 3 and (avih[8], avih[9]) == (SW, SH)


def test_the_bounds_are_what_the_header_states():
    for SH, SW in SIZES + [(1096, 1568)]:
        cols, rows = (SW + 15) // 16, (SH + 15) // 16
        assert panel.jpeg_segment_bound(SW) == 2 * 216 * 6 * cols
        assert panel.jpeg_max_bytes(SH, SW) == panel.JPEG_HEADER_BYTES + rows * panel.jpeg_segment_bound(SW) + 2 * (rows - 1) + 2
    # the worst block the tables can code: DC category 11 and 63 coefficients of category 10 at the longest code
    H = panel._jpeg_tables()
    worst = max(int(H["dc"][c][1].max()) + 11 + 63 * (int(H["ac"][c][1].max()) + 10) for c in range(2))
    assert worst <= 64 * 27 == 216 * 8


def test_reference_protocol_driver_writes_the_defined_files(tmp_path):
    """A model behind the reference's call protocol with panel_encode="gpu": jpeg_encode_host on the host, the files the native
    path writes; host mode and the frames are untouched."""
    from PIL import Image
    from render_in_between_amd import evaluator as ev
    from tests.test_driver import _write_example, oracle_labels
    from tests.test_panels_cpu import Recorder, small_cfg
    root = str(tmp_path)
    H, W = 32, 48
    n = _write_example(root, n_key=2, rate=2, H=H, W=W)
    cfg = small_cfg(H, W)
    dirs = [os.path.join(root, d) for d in ("inputs", "DAIN", "Predict_motion")]
    runs = {}
    for name, kw in (("host", {}), ("gpu", dict(panel_encode="gpu", panel_quality=75))):
        out = os.path.join(root, name)
        runs[name] = (out, ev.Evaluator(cfg, label_fn=oracle_labels).evaluate_from_folder(Recorder(cfg), *dirs, out, panels=True, panel_frames=True, **kw))
    for x, y in zip(runs["host"][1], runs["gpu"][1]):
        assert open(x, "rb").read() == open(y, "rb").read()
    for name, q in (("host", None), ("gpu", 75)):
        out = runs[name][0]
        raw = open(os.path.join(out, "clipA.avi"), "rb").read()
        ck = parse_riff(raw)
        assert len(ck["movi/00dc"]) == n
        for i, (o, size) in enumerate(ck["movi/00dc"]):
            sheet = np.asarray(Image.open(os.path.join(out, "clipA_panels", "%04d.png" % i)).convert("RGB"))
            assert raw[o:o + size] == (panel.jpeg_encode_host(sheet, q) if q else pil_encode(sheet, 90)), (name, i)
    with pytest.raises(ValueError, match="panels"):
        ev.Evaluator(cfg, label_fn=oracle_labels).evaluate_from_folder(Recorder(cfg), *dirs, os.path.join(root, "o"), panel_encode="gpu")
    with pytest.raises(ValueError, match="panel_encode"):
        ev.Evaluator(cfg, label_fn=oracle_labels).evaluate_from_folder(Recorder(cfg), *dirs, os.path.join(root, "o"), panels=True, panel_encode="cpu")
    assert not os.path.exists(os.path.join(root, "o"))


def test_command_line_flag():
    from render_in_between_amd import inference
    assert inference.parse_args(["--input-dir", "x", "--panels"]).panel_encode is None
    assert inference.parse_args(["--input-dir", "x", "--panels", "--panel-encode", "gpu", "--panel-quality", "70"]).panel_encode == "gpu"
    for bad in (["--panel-encode", "gpu"], ["--panels", "--panel-encode", "cpu"]):
        with pytest.raises(SystemExit):
            inference.parse_args(["--input-dir", "x"] + bad)


def test_build_stamp_and_bindings_cover_the_jpeg_kernels():
    import importlib.util
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("rib_build_for_jpeg", os.path.join(here, "render-in-between_amd", "csrc", "build.py"))
    b = importlib.util.module_from_spec(spec); spec.loader.exec_module(b)
    assert any(os.path.basename(d) == "jpeg.hip.h" for d in b.DEPS) and not any(os.path.basename(d) == "jpeg.hip.h" for d in b.SHARD_DEPS)
    from render_in_between_amd import _native
    assert {"rib_jpeg", "rib_jpeg_max_bytes", "rib_jpeg_workspace_bytes"} <= set(_native.SIGNATURES)
