"""The folder driver's staging block on the MI355X (evaluator.staging_spec / block_layout): the sections a unit
stages - dain | gt | mask | key | mci_keys, each under its option - change nothing of what the unit writes, whichever of them
share the block, with threads and with worker processes; and the loose key frames' one download (loose_keys) writes the
sheets' and the frames' videos as each option writes them alone."""
import os

import numpy as np
import pytest

from render_in_between_amd import evaluator as ev
from tests.test_gpu_download import tree
from tests.test_gpu_quality import handle
from tests.test_gpu_video import H64, W64, cfg64

pytestmark = pytest.mark.gpu
MODES = ("thread", "process")
_RUNS = {}


def example(root):
    """3 key frames at rate 4 (9 frames).  DAIN files at 90x70 and ground-truth files at 60x50, so that resize_on="gpu" stages
    both at their source sizes; masks at the model size.  The key frames in `inputs` are the ground-truth folder's files of the
    same frames: a call with a gt_dir and one without read the same key frames and scale the poses by the same size."""
    from PIL import Image
    from tests.test_driver import _write_example
    n = _write_example(root, n_key=3, rate=4, H=H64, W=W64)
    rng = np.random.default_rng(7)
    for d in ("gt", "masks"):
        os.makedirs(os.path.join(root, d, "clipA"))
    for i in range(n):
        Image.fromarray(rng.integers(0, 255, (70, 90, 3), dtype=np.uint8)).save(os.path.join(root, "DAIN", "clipA", "f%03d.png" % i))
        gt = Image.fromarray(rng.integers(0, 255, (50, 60, 3), dtype=np.uint8))
        gt.save(os.path.join(root, "gt", "clipA", "g%03d.png" % i))
        if i % 4 == 0:
            gt.save(os.path.join(root, "inputs", "clipA", "%04d.png" % (i // 4)))
        Image.fromarray((rng.integers(0, 2, (H64, W64), dtype=np.uint8) * 255)).save(os.path.join(root, "masks", "clipA", "m%03d.png" % i))
    return n


def runs(io_mode, tmp_path_factory):
    """Every run of this module in one io_mode, made once: name -> {written, pngs, metrics, avi, video_avi, tables}.  After
    every call every shared block is back on a free list and no clip holds a staging record."""
    if io_mode in _RUNS:
        return _RUNS[io_mode]
    root = str(tmp_path_factory.mktemp("staging_" + io_mode))
    n = example(root)
    G = handle()
    inputs, dain, poses, gt, masks = (os.path.join(root, d) for d in ("inputs", "DAIN", "Predict_motion", "gt", "masks"))
    plan_clip, layout = ev._FolderPipeline.plan_clip, ev.block_layout

    def run(name, mci=False, **kw):
        out, clips, tables = os.path.join(root, name), [], set()

        def planned(self, *a):
            clips.append(plan_clip(self, *a))
            return clips[-1]

        def laid_out(sections):
            tables.add(tuple(layout(sections)[0]))
            return layout(sections)
        ev._FolderPipeline.plan_clip, ev.block_layout = planned, laid_out
        try:
            E = ev.Evaluator(cfg64(), batch=2, chunk=2, lanes=1, io_mode=io_mode, resize_on="host" if mci else "gpu")
            written = E.evaluate_from_folder(G, inputs, None if mci else dain, poses, out, **dict({"background": "mci"} if mci else {}, **kw))
        finally:
            ev._FolderPipeline.plan_clip, ev.block_layout = plan_clip, layout
        ev._shm_trim()
        assert all(len(v) <= ev._SHM_KEEP for v in ev._SHM_FREE.values()), name
        assert sum(len(v) for v in ev._SHM_FREE.values()) == len(ev._SHM_ALL), name      # every block is back on a free list
        assert len(clips) == 1 and clips[0].staged == {}, name

        def read(f):
            return open(os.path.join(out, f), "rb").read() if os.path.exists(os.path.join(out, f)) else None
        return {"written": [os.path.relpath(w, out) for w in written], "metrics": E.metrics if kw.get("metrics") else None,
                "pngs": tree(out, "clipA") if os.path.isdir(os.path.join(out, "clipA")) else None,
                "avi": read("clipA.avi"), "video_avi": read("clipA_video.avi"), "tables": tables}

    measured = dict(gt_dir=gt, metrics=True, mask_dir=masks)
    r = {"n": n,
         "a": run("a", gt_dir=gt),
         "b": run("b", **measured),
         "c": run("c", panels=True, **measured),
         "d": run("d", mci=True, panels=True, **measured),
         "e": run("e", mci=True, panels=True),
         "f": run("f", gt_dir=gt, panels=True, panel_encode="gpu", video=True, frames="none"),
         "f_sheets": run("f_sheets", gt_dir=gt, panels=True, panel_encode="gpu"),
         "f_video": run("f_video", gt_dir=gt, video=True, frames="none")}
    _RUNS[io_mode] = r
    return r


@pytest.mark.parametrize("io_mode", MODES)
def test_sections_sharing_a_block_change_no_output(tmp_path_factory, io_mode):
    """64x64, batch 2, chunk 2, one lane: a first chunk with its key frames, a later chunk, a loose last key frame.  (a) plain
    under resize_on="gpu", (b) + metrics with masks, (c) + panels: dain | gt | mask | key; (d) background="mci" with metrics,
    masks and panels: gt | mask | mci_keys and no dain section; (e) = (d) without metrics and without a gt_dir, whose later
    chunk stages nothing.  The PNG trees of (b) and (c) are (a)'s and (c)'s metrics are (b)'s; (d) and (e) write equal trees."""
    r = runs(io_mode, tmp_path_factory)
    a, b, c, d, e = (r[k] for k in "abcde")
    assert len(a["written"]) == len(a["pngs"]) == r["n"] == 9
    assert ("dain",) in a["tables"] and ("dain", "gt", "mask") in b["tables"]
    assert {("dain", "gt", "mask", "key"), ("dain", "gt", "mask")} <= c["tables"]
    assert {("gt", "mask", "mci_keys"), ("gt", "mask")} <= d["tables"] and {("mci_keys",), ()} <= e["tables"]
    assert not any("dain" in t for t in d["tables"] | e["tables"])
    assert b["pngs"] == a["pngs"] and c["pngs"] == a["pngs"]
    assert b["written"] == a["written"] == c["written"]
    assert len(b["metrics"]) == 6 and c["metrics"] == b["metrics"]
    assert len(d["pngs"]) == 9 and d["pngs"] == e["pngs"] and d["written"] == e["written"]
    assert len(d["metrics"]) == 6 and d["avi"] is not None and e["avi"] is not None


@pytest.mark.parametrize("io_mode", MODES)
def test_loose_key_frames_ride_in_one_download(tmp_path_factory, io_mode):
    """(f) panels encoded on the GPU + video under frames="none": the loose last key frame's sheet and its video file come home
    in one buffer (sheet_len | video_len).  Both .avi files are the files of each option alone, and the written list names one
    .jpg per frame, the loose key frame's included."""
    r = runs(io_mode, tmp_path_factory)
    f = r["f"]
    assert f["avi"] is not None and f["avi"] == r["f_sheets"]["avi"]
    assert f["video_avi"] is not None and f["video_avi"] == r["f_video"]["video_avi"]
    assert ("sheet_len", "video_len") in f["tables"] and ("sheet_len",) in r["f_sheets"]["tables"] and ("video_len",) in r["f_video"]["tables"]
    assert f["written"] == r["f_video"]["written"] == [os.path.join("clipA_video", "%04d.jpg" % i) for i in range(r["n"])]
    assert f["pngs"] is None and r["f_video"]["pngs"] is None and len(r["f_sheets"]["pngs"]) == r["n"]


def test_threads_and_worker_processes_write_the_same(tmp_path_factory):
    """Every run above, decoded into page-locked tensors by threads and into shared blocks by worker processes: the same
    names, files, videos and metric values - and the same tables, so the two modes lay a unit out alike."""
    t, p = (runs(m, tmp_path_factory) for m in MODES)
    assert list(t) == list(p)
    for name in t:
        assert t[name] == p[name], name
