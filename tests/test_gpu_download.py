"""The folder driver's download buffer on the MI355X with several output options at once (evaluator.block_layout):
every option alone is pinned by its own test (test_gpu_quality / _panel / _jpeg / _video); here they share one unit's buffer -
metrics with video, and all five sections together - and every output must be the bytes the option writes alone."""
import os

import numpy as np
import pytest

from render_in_between_amd import evaluator as ev, panel
from tests.test_gpu_quality import handle
from tests.test_gpu_video import H64, W64, cfg64, video_frames

pytestmark = pytest.mark.gpu


def tree(out, sub):
    d = os.path.join(out, sub)
    return {f: open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d))}


@pytest.mark.parametrize("io_mode", ["thread", "process"])
def test_combined_options_write_what_each_writes_alone(tmp_path, io_mode):
    """64x64, 3 key frames at rate 4, batch 2, chunk 2 (a first chunk with its key frames, a later chunk, a loose last key
    frame).  (a) plain, (b) metrics, (c) sheets encoded on the GPU and (d) video each run alone; then (e) all of them in one
    call - sections frames | qual | sheet_len | video_len -, (f) metrics + video under frames="none" - qual | video_len - and
    (g) = (e) with panel_frames, the one setting under which all five sections travel.  PNG frames, metrics and both videos
    are equal to the single-option runs', byte for byte and value for value; a lossless sheet of (g), encoded by the
    definition, is its frame of the sheets' video.  After every call every shared block is back on a free list."""
    from PIL import Image
    from tests.test_driver import _write_example
    root = str(tmp_path)
    n = _write_example(root, n_key=3, rate=4, H=H64, W=W64)
    rng = np.random.default_rng(4)
    os.makedirs(os.path.join(root, "gt", "clipA"))
    for i in range(n):
        Image.fromarray(rng.integers(0, 255, (H64, W64, 3), dtype=np.uint8)).save(os.path.join(root, "gt", "clipA", "g%03d.png" % i))
    G = handle()
    dirs = [os.path.join(root, d) for d in ("inputs", "DAIN", "Predict_motion")]

    def run(name, **kw):
        out = os.path.join(root, name)
        E = ev.Evaluator(cfg64(), batch=2, chunk=2, lanes=1, io_mode=io_mode)
        written = E.evaluate_from_folder(G, *dirs, out, gt_dir=os.path.join(root, "gt"), **kw)
        ev._shm_trim()
        assert all(len(v) <= ev._SHM_KEEP for v in ev._SHM_FREE.values()), name
        assert sum(len(v) for v in ev._SHM_FREE.values()) == len(ev._SHM_ALL), name      # every block is back on a free list
        return out, written, E.metrics

    a, a_w, _ = run("a")
    b, _, b_m = run("b", metrics=True)
    c, _, _ = run("c", panels=True, panel_encode="gpu")
    d, _, _ = run("d", video=True)
    pngs, sheets_avi, frames_avi = tree(a, "clipA"), open(os.path.join(c, "clipA.avi"), "rb").read(), open(os.path.join(d, "clipA_video.avi"), "rb").read()
    assert len(a_w) == len(pngs) == n == 9 and len(b_m) == 6 and tree(b, "clipA") == pngs
    assert len(video_frames(os.path.join(c, "clipA.avi"))) == len(video_frames(os.path.join(d, "clipA_video.avi"))) == n

    e, e_w, e_m = run("e", metrics=True, panels=True, panel_encode="gpu", video=True)
    assert [os.path.relpath(w, e) for w in e_w] == [os.path.relpath(w, a) for w in a_w]
    assert sorted(os.listdir(e)) == ["clipA", "clipA.avi", "clipA_video.avi", "metrics.json"]
    assert tree(e, "clipA") == pngs
    assert e_m == b_m
    assert open(os.path.join(e, "clipA.avi"), "rb").read() == sheets_avi
    assert open(os.path.join(e, "clipA_video.avi"), "rb").read() == frames_avi

    f, f_w, f_m = run("f", metrics=True, video=True, frames="none")
    assert sorted(os.listdir(f)) == ["clipA_video.avi", "metrics.json"] and len(f_w) == n
    assert f_m == b_m
    assert open(os.path.join(f, "clipA_video.avi"), "rb").read() == frames_avi

    g, _, g_m = run("g", metrics=True, panels=True, panel_encode="gpu", panel_frames=True, video=True)
    assert sorted(os.listdir(g)) == ["clipA", "clipA.avi", "clipA_panels", "clipA_video.avi", "metrics.json"]
    assert tree(g, "clipA") == pngs and g_m == b_m
    assert open(os.path.join(g, "clipA.avi"), "rb").read() == sheets_avi
    assert open(os.path.join(g, "clipA_video.avi"), "rb").read() == frames_avi
    lossless = sorted(os.listdir(os.path.join(g, "clipA_panels")))
    assert lossless == ["%04d.png" % i for i in range(n)]
    for i, jpg in enumerate(video_frames(os.path.join(g, "clipA.avi"))):
        sheet = np.asarray(Image.open(os.path.join(g, "clipA_panels", lossless[i])))
        assert jpg == panel.jpeg_encode_host(sheet, 90), i
