"""A unit's staging block on the host (no GPU): evaluator.staging_spec names the sections the decode tasks fill and upload()
sends to the GPU, evaluator.block_layout places them, evaluator.section_views and _FolderPipeline.slot_offset are the only two
readers of that table - and the file workers decode into exactly the bytes the table names, in-process and in a
worker process."""
import itertools
import os
from types import SimpleNamespace

import numpy as np
import torch

from render_in_between_amd import evaluator as ev, io_worker
from tests.test_driver import _write_example

TC, BC, H, W = 2, 3, 8, 12
SRC_DAIN, SRC_GT = (20, 14), (10, 6)         # (w0, h0) of resize_on="gpu"


def unit(table, first=True):
    """What slot_offset reads of a clip: unit 0's table, and the unit itself (group, members, c0, c1)."""
    return SimpleNamespace(staged={0: {"table": table}}, units=[(0, list(range(BC)), 0 if first else TC, (TC if first else 2 * TC))])


def slots_of(name):
    return [(t, b) for t in range(1 if name == "key" else TC) for b in range(BC)]


def test_staging_spec_and_block_layout_over_every_valid_combination():
    """mci or not x ground truth x masks (only with ground truth) x first chunk or not x panels or not x DAIN / ground truth at
    the source or the model size, at Tc = 2, B = 3, 8x12: the table lists exactly the sections the rules name, in buffer order,
    on multiples of 256, without overlap and with gaps of padding only; every slot's bytes lie inside its section, apart from
    every other slot's, where the section's view has them; an absent section is -1 / None.  A later chunk under mci with
    nothing else to stage has no bytes at all (open_units then allocates its max(1, total) = 1)."""
    seen = set()
    for mci, want_gt, masks, first, panels, src_dain, src_gt in itertools.product(
            (False, True), (False, True), (False, True), (False, True), (False, True), (None, SRC_DAIN), (None, SRC_GT)):
        if masks and not want_gt:
            continue
        case = (mci, want_gt, masks, first, panels, src_dain, src_gt)
        spec = ev.staging_spec(TC, BC, (H, W), src_dain, src_gt, want_gt=want_gt, masks=masks, keys=panels and first, mci=mci,
                               mci_keys=first)
        assert [s[0] for s in spec] == ["dain", "gt", "mask", "key", "mci_keys"] and all(s[1] == torch.uint8 for s in spec)
        (wd, hd), (wg, hg) = src_dain or (W, H), src_gt or (W, H)
        shapes = {"dain": (TC, BC, hd, wd, 3), "gt": (TC, BC, hg, wg, 3), "mask": (TC, BC, H, W), "key": (BC, H, W, 3),
                  "mci_keys": (2, BC, H, W, 3)}
        assert {s[0]: tuple(s[2]) for s in spec} == shapes, case
        want = [name for name, on in (("dain", not mci), ("gt", want_gt), ("mask", masks), ("key", panels and first and not mci),
                                      ("mci_keys", mci and first)) if on]
        table, total = ev.block_layout(ev.spec_bytes(spec))
        assert list(table) == want, case
        seen.add(tuple(want))
        end = 0
        for name, (off, nbytes) in table.items():
            assert off % 256 == 0 and end <= off < end + 256 and nbytes == int(np.prod(shapes[name])), (case, name)
            end = off + nbytes
        assert total == end, case
        flat = torch.zeros(max(1, total), dtype=torch.uint8)
        views = ev.section_views(flat, spec, table)
        assert list(views) == list(shapes), case
        clip, taken = unit(table, first), []
        for name in shapes:
            if name not in table:
                assert views[name] is None and ev._FolderPipeline.slot_offset(clip, 0, name, 1, 0) == -1, (case, name)
                continue
            off, nbytes = table[name]
            assert tuple(views[name].shape) == shapes[name] and views[name].dtype == torch.uint8, (case, name)
            assert views[name].storage_offset() == off and views[name].is_contiguous(), (case, name)
            if name == "mci_keys":               # filled by upload() through its view, not by slot
                continue
            size = int(np.prod(shapes[name][-3:] if name != "mask" else shapes[name][-2:]))
            for t, b in slots_of(name):
                at = ev._FolderPipeline.slot_offset(clip, 0, name, b, t)
                assert off <= at and at + size <= off + nbytes, (case, name, t, b)
                v = views[name][b] if name == "key" else views[name][t, b]
                assert v.storage_offset() == at and v.numel() == size, (case, name, t, b)       # the view's slot is the helper's
                taken.append((at, at + size))
        taken.sort()
        assert all(a[1] <= b[0] for a, b in zip(taken, taken[1:])), case
        if mci and not first and not want_gt:
            assert table == {} and total == 0 and all(v is None for v in views.values()), case
    assert ("dain", "gt", "mask", "key") in seen and ("gt", "mask", "mci_keys") in seen and () in seen and ("dain",) in seen


def test_file_workers_decode_into_the_offsets_of_the_table(tmp_path):
    """The most crowded block without mci - dain and gt at their source sizes, mask, key - in a shared block: two slots,
    one decoded by io_worker.load_frame_shm in this process and one in a worker process, at the offsets slot_offset reads from
    the table and with the keywords decode_in_worker passes.  The views of section_views then hold those files' pixels in
    those slots, and every other byte of the block is still zero."""
    from PIL import Image
    root = str(tmp_path)
    _write_example(root, n_key=2, rate=2, H=H, W=W)                  # for a pose file
    pose = os.path.join(root, "Predict_motion", "clipA", "f001_keypoints.json")
    rng = np.random.default_rng(11)
    files = {}
    for name, shape in (("dain", (SRC_DAIN[1], SRC_DAIN[0], 3)), ("gt", (SRC_GT[1], SRC_GT[0], 3)), ("key", (H, W, 3)), ("mask", (H, W))):
        files[name] = os.path.join(root, name + ".png")
        Image.fromarray(rng.integers(0, 255, shape, dtype=np.uint8)).save(files[name])
    want = {}
    for name, size in (("dain", SRC_DAIN), ("gt", SRC_GT), ("key", (W, H))):
        want[name] = np.zeros((size[1], size[0], 3), np.uint8)
        io_worker.decode_raw_into(want[name], 0, files[name], size)
    want["mask"] = io_worker.load_mask_u8(files["mask"], W, H)
    assert all(w.any() for w in want.values())

    spec = ev.staging_spec(TC, BC, (H, W), SRC_DAIN, SRC_GT, want_gt=True, masks=True, keys=True)
    table, total = ev.block_layout(ev.spec_bytes(spec))
    assert list(table) == ["dain", "gt", "mask", "key"]
    clip = unit(table)
    blk = ev._shm_get(total)
    try:
        blk.t.zero_()
        views = ev.section_views(blk.t, spec, table)
        common = (True, True, W, H, "cv2", 0.001, 0.001)
        pool = ev._process_pool(2)
        calls = {(0, 1): lambda *a, **kw: io_worker.load_frame_shm(*a, **kw),
                 (1, 2): lambda *a, **kw: pool.submit(io_worker.load_frame_shm, *a, **kw).result(timeout=120)}
        for (t, b), call in calls.items():
            off, gt_off, mask_off = (ev._FolderPipeline.slot_offset(clip, 0, name, b, t) for name in ("dain", "gt", "mask"))
            got = call(blk.name, off, files["dain"], files["gt"], pose, *common, gt_offset=gt_off, mask_path=files["mask"],
                       mask_offset=mask_off, dain_raw=SRC_DAIN, gt_raw=SRC_GT)
            assert got[0] is None and got[1].shape == (H, W, 3)
            # the key frame a first chunk starts from: its DAIN frame to the key section, at the model size
            call(blk.name, ev._FolderPipeline.slot_offset(clip, 0, "key", b), files["key"], files["key"], pose, *common,
                 gt_offset=-1, mask_path=None, mask_offset=-1, dain_raw=None, gt_raw=None)
        for t, b in calls:
            for name in ("dain", "gt", "mask"):
                assert np.array_equal(views[name][t, b].numpy(), want[name]), (name, t, b)
                views[name][t, b].zero_()
            assert np.array_equal(views["key"][b].numpy(), want["key"]), b
            views["key"][b].zero_()
        assert not blk.t.any()                   # nothing was written outside the two slots of each section
    finally:
        views = None
        ev._shm_put(blk)
