"""rib_mci_field (csrc/mci.hip.h; Generator.mci_field(..., levels)) with four and five pyramid levels - the driver's
mci_range = 64 and 128 - against background.mci_field_host(..., levels), bit for bit: fields saturated at +-39 and +-79 (beyond
what the old 6-bit key fields held), ties on the new top levels, frames smaller than a top-level block and pyramid levels of
1 x 1, batches, rib_mci_frames on such a field, and the native folder driver.  tests/test_mci_range_cpu.py builds the inputs and
shows with the definition alone that they reach the widened fields."""
import os

import numpy as np
import pytest
import torch

import render_in_between_amd as rib
from render_in_between_amd import background as bg, evaluator as ev
from tests.mci_gpu_common import check_defaults, check_field, dev, ref
from tests.test_background_cpu import random_pair, tie_pair
from tests.test_gpu_mci import Protocol, handle
from tests.test_mci_range_cpu import ODD_SIZES, WIDE_MOTIONS, WIDE_SIZES, WIDE_TIE_KINDS, WIDE_TIE_SIZES, wide_pair, write_moving_clips

pytestmark = pytest.mark.gpu

LEVELS = (4, 5)
RIB_ERR_INVALID = -1                                                    # include/rib.h


def wide_ref(levels, h, w, i):
    return ref(("wide", levels, h, w, i), lambda: wide_pair(levels, h, w, i), levels)


@pytest.mark.parametrize("levels", LEVELS)
@pytest.mark.parametrize("h,w", WIDE_SIZES)
def test_fields_saturated_at_the_widest_displacement(h, w, levels):
    G = handle()
    refs = [wide_ref(levels, h, w, i) for i in range(len(WIDE_MOTIONS[levels]))]
    if (h, w) == WIDE_SIZES[0]:
        allf = np.stack([r[2] for r in refs])
        assert allf.max() == bg.max_disp(levels) and allf.min() == -bg.max_disp(levels)
    batch = check_field(G, refs, levels)
    for i, r in enumerate(refs):
        assert torch.equal(check_field(G, [r], levels)[0], batch[i])


@pytest.mark.parametrize("levels", LEVELS)
@pytest.mark.parametrize("h,w", WIDE_TIE_SIZES)
def test_ties_on_the_new_top_levels(h, w, levels):
    G = handle()
    refs = [ref(("tie", kind, h, w), lambda: tie_pair(kind, h, w), levels) for kind in WIDE_TIE_KINDS]
    assert any(r[2].any() for r in refs)
    check_field(G, refs, levels)


@pytest.mark.parametrize("levels", LEVELS)
@pytest.mark.parametrize("h,w", ODD_SIZES)
def test_sizes_down_to_one_pixel(h, w, levels):
    G = handle()
    check_field(G, [ref(("odd", h, w), lambda: random_pair(h, w, 1), levels)], levels)


@pytest.mark.parametrize("levels", LEVELS)
def test_a_batch_of_three_different_pairs(levels):
    """B = 3: the three single calls' fields - no pair reads another's planes or fields (the 2B images of the new levels)."""
    G = handle()
    h, w = WIDE_SIZES[1]
    refs = [wide_ref(levels, h, w, 1), ref(("tie", "diagonal16", h, w), lambda: tie_pair("diagonal16", h, w), levels),
            ref(("rand", h, w), lambda: random_pair(h, w, 2), levels)]
    assert not np.array_equal(refs[0][2], refs[1][2]) and not np.array_equal(refs[1][2], refs[2][2])
    batch = check_field(G, refs, levels)
    for i, r in enumerate(refs):
        ta, tb = dev(G, r[0], r[1])
        assert torch.equal(G.mci_field(ta, tb, levels), batch[i])


def test_three_levels_and_the_clamp_border_are_the_defaults():
    """On saturated, tied, tiny and odd inputs (mci_gpu_common.check_defaults)."""
    G = handle()
    inputs = [wide_ref(5, *WIDE_SIZES[0], 1)[:2], wide_ref(4, *WIDE_SIZES[1], 0)[:2], tie_pair("checker8", 67, 93), random_pair(33, 15, 1),
              random_pair(1, 1, 1), random_pair(130, 250, 1)]
    for a, b in inputs:
        check_defaults(G, a, b)


def test_frames_from_a_field_of_plus_minus_79():
    """rib_mci_frames on a five-level field: every frame at s = 8, and k = 1, 512, 1023 at s = 1024 (2 k D near 4.2e7), both
    outputs, against mci_frames_host."""
    G = handle()
    h, w = WIDE_SIZES[0]
    a, b, f = wide_ref(5, h, w, 1)
    assert f.max() == 79 and f.min() == -79
    ta, tb, tf = dev(G, a, b, f)
    for s, ks in ((8, list(range(0, 9))), (1024, [1, 512, 1023])):
        want = bg.mci_frames_host(a, b, f, s, ks)
        got_f, got_u = [], []
        for k in ([ks[0]] if s == 8 else ks):                               # s = 8: all nine frames in one launch
            f32, u8 = G.mci_frames(ta, tb, tf, s, k_first=k, count=len(ks) if s == 8 else 1, normalised="both")
            got_f.append(f32)
            got_u.append(u8)
        u8, f32 = torch.cat(got_u).cpu(), torch.cat(got_f).cpu()
        assert torch.equal(u8, torch.from_numpy(want)), s
        assert torch.equal(f32, torch.from_numpy(bg.normalised_upload(want))), s


def test_native_folder_driver_with_range_64(tmp_path):
    """background="mci", mci_range=64 at 64 x 64, two clips of three key frames 48 px (40 x 24 px) apart, batch 2: the native
    path's PNGs and .avi are the reference-protocol path's through the same Generator, byte for byte, and are not range 32's."""
    root = str(tmp_path)
    keys = write_moving_clips(root, n_key=3)
    G = handle()
    cfg = rib.AttrDict(gen=rib.hsm_gen_config(), model_height=64, model_width=64, gauss_sigma=5, skeleton_thres=0.001, foot_thres=0.001)
    inputs, poses = os.path.join(root, "inputs"), os.path.join(root, "Predict_motion")
    kw = dict(background="mci", video=True)
    nat = ev.Evaluator(cfg, batch=2, chunk=2, lanes=1).evaluate_from_folder(G, inputs, None, poses, os.path.join(root, "nat"), mci_range=64, **kw)
    n32 = ev.Evaluator(cfg, batch=2, chunk=2, lanes=1).evaluate_from_folder(G, inputs, None, poses, os.path.join(root, "n32"), **kw)
    before = G.plan_batch
    G.set_plan_batch(2)                         # the reference-protocol path follows the plans the native group follows
    try:
        refw = ev.Evaluator(cfg).evaluate_from_folder(Protocol(G), inputs, None, poses, os.path.join(root, "ref"), mci_range=64, **kw)
    finally:
        G.set_plan_batch(before)
    assert len(nat) == len(refw) == len(n32) == 10
    for x, y in zip(nat, refw):
        assert os.path.basename(x) == os.path.basename(y) and open(x, "rb").read() == open(y, "rb").read(), x
    for clip in keys:
        avi = open(os.path.join(root, "nat", clip + "_video.avi"), "rb").read()
        assert avi == open(os.path.join(root, "ref", clip + "_video.avi"), "rb").read()
        assert avi != open(os.path.join(root, "n32", clip + "_video.avi"), "rb").read()
    # key frames pass through; a frame in between differs from range 32's wherever the definition's background does
    want = []
    for frames in keys.values():
        for a, b in zip(frames, frames[1:]):
            mid = [bg.mci_frames_host(a, b, bg.mci_field_host(a, b, levels), 2, [1]) for levels in (3, 4)]
            want += [False, not np.array_equal(*mid)]
        want.append(False)
    assert sum(want) >= 2 and [open(x, "rb").read() != open(y, "rb").read() for x, y in zip(nat, n32)] == want


def test_bad_levels_through_the_c_abi():
    G = handle()
    L = G._lib
    h, w = 40, 56
    a, b = random_pair(h, w, 1)
    ta, tb = dev(G, a, b)
    Hb, Wb = bg.field_shape(h, w)
    ws = torch.empty(L.rib_mci_workspace_bytes(G._h, 1, h, w, 5), dtype=torch.uint8, device=G.device)
    for bad in (2, 6, 0, -1):
        assert L.rib_mci_workspace_bytes(G._h, 1, h, w, bad) == 0
        field = torch.full((Hb, Wb, 2), 77, dtype=torch.int16, device=G.device)
        rc = L.rib_mci_field(G._h, 1, h, w, ta.data_ptr(), tb.data_ptr(), field.data_ptr(), bad, 0, ws.data_ptr(), None)
        assert rc == RIB_ERR_INVALID
        assert b"levels=%d" % bad in L.rib_last_error(G._h)
        torch.cuda.synchronize()
        assert (field == 77).all()                                          # nothing was launched
    with pytest.raises(ValueError, match="levels"):
        G.mci_field(ta, tb, levels=6)
