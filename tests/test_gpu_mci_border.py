"""rib_mci_field / rib_mci_frames with border = 1 (csrc/mci.hip.h: k_mci_search<R, true>, k_mci_frames<true>;
Generator.mci_field / mci_frames(..., border="valid")) - the one-sided border mode of the interpolated backgrounds - against
background.py's border="valid", bit for bit; border = 0 as the default of both; and the folder driver
with mci_border="valid".  The inputs and what they must reach are built and held in tests/test_mci_border_cpu.py."""
import functools
import os

import numpy as np
import pytest
import torch

import render_in_between_amd as rib
from render_in_between_amd import background as bg, evaluator as ev
from tests.mci_gpu_common import check_defaults, check_field, dev, ref
from tests.test_background_cpu import moving_pair, random_pair, tie_pair
from tests.test_gpu_mci import Protocol, handle
from tests.test_mci_border_cpu import BORDER_TIE_KINDS, GPU_PARTIAL_SIZES, GPU_TRANSLATIONS, INHERIT, ODD_SIZES, gpu_translation_pairs
from tests.test_mci_range_cpu import wide_pair, write_moving_clips

pytestmark = pytest.mark.gpu

LEVELS = (3, 4, 5)
RIB_ERR_INVALID = -1                                                    # include/rib.h
_translation_pairs = functools.lru_cache(None)(gpu_translation_pairs)


def translation_refs(levels):
    return [ref(("shift", levels, i), lambda: _translation_pairs(levels)[i], levels, "valid") for i in range(len(GPU_TRANSLATIONS[levels][2]))]


def check_frames(G, r, s, k_first, count, normalised="both"):
    """Frames k_first .. k_first + count - 1 of one pair in one launch against mci_frames_host(border="valid")."""
    a, b, f = r
    ta, tb, tf = dev(G, a, b, f)
    want = bg.mci_frames_host(a, b, f, s, range(k_first, k_first + count), border="valid")
    got = G.mci_frames(ta, tb, tf, s, k_first=k_first, count=count, normalised=normalised, border="valid")
    f32, u8 = got if normalised == "both" else (got, None) if normalised else (None, got)
    if u8 is not None:
        assert torch.equal(u8.cpu(), torch.from_numpy(want)), (a.shape, s, k_first)
    if f32 is not None:
        assert torch.equal(f32.cpu(), torch.from_numpy(bg.normalised_upload(want))), (a.shape, s, k_first)
    return want


# ---- the field -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("levels", LEVELS)
def test_translation_fields_in_a_batch_and_alone(levels):
    """Every block of the field is d - border blocks and inherited blocks included (64 x 96, 128 x 128, 128 x 256: interior and
    border blocks on every level); B = 3 and each pair alone; then every frame of s = 8 of each, k = 0 and 8 included."""
    G = handle()
    refs = translation_refs(levels)
    for (dx, dy), r in zip(GPU_TRANSLATIONS[levels][2], refs):
        assert (r[2] == (dx, dy)).all()
    batch = check_field(G, refs, levels, "valid")
    for i, r in enumerate(refs):
        assert torch.equal(check_field(G, [r], levels, "valid")[0], batch[i])
        frames = check_frames(G, r, 8, 0, 9)
        assert np.array_equal(frames[0], r[0]) and np.array_equal(frames[8], r[1])
        assert not np.array_equal(frames[3], bg.mci_frames_host(r[0], r[1], r[2], 8, [3])[0])        # (the mode decides pixels here)


@pytest.mark.parametrize("levels", LEVELS)
@pytest.mark.parametrize("h,w", GPU_PARTIAL_SIZES)
def test_partial_blocks_and_tiles(h, w, levels):
    """67 x 93, 130 x 250: N < 64 on every level, a last run of fewer than MCI_RUN blocks; a pan and unrelated content."""
    G = handle()
    refs = [ref(("pan", h, w), lambda: moving_pair(h, w, 30, -20, 50), levels, "valid"), ref(("rand", h, w), lambda: random_pair(h, w, 2), levels, "valid")]
    assert refs[0][2].any() and not np.array_equal(refs[0][2], bg.mci_field_host(refs[0][0], refs[0][1], levels))
    check_field(G, refs, levels, "valid")
    check_frames(G, refs[0], 8, 0, 9)


def test_inherited_blocks():
    """A 38 px pan in a 56 px frame: half of the level-0 blocks keep their start (tests/test_mci_border_cpu.py counts them)."""
    G = handle()
    r = ref(("inherit",), lambda: moving_pair(*INHERIT), 3, "valid")
    check_field(G, [r], 3, "valid")
    check_frames(G, r, 8, 1, 7)


@pytest.mark.parametrize("levels", LEVELS)
def test_ties_under_the_normalised_cost(levels):
    G = handle()
    refs = [ref(("tie", kind), lambda: tie_pair(kind, 64, 64), levels, "valid") for kind in BORDER_TIE_KINDS]
    assert any(r[2].any() for r in refs)
    check_field(G, refs, levels, "valid")
    check_frames(G, refs[3], 4, 1, 3)


@pytest.mark.parametrize("levels", LEVELS)
@pytest.mark.parametrize("h,w", ODD_SIZES)
def test_sizes_down_to_one_pixel(h, w, levels):
    """1 x 1 .. 40 x 1: planes with room for d = 0 alone, blocks of one pixel row or column."""
    G = handle()
    r = ref(("odd", h, w), lambda: random_pair(h, w, 1), levels, "valid")
    check_field(G, [r], levels, "valid")
    check_frames(G, r, 4, 0, 5)


@pytest.mark.parametrize("levels", LEVELS)
def test_a_saturated_wide_pair(levels):
    """About twice the range between the key frames: long vectors, and inheritance where they leave the frame."""
    G = handle()
    if levels == 3:
        r = ref(("long", 3), lambda: moving_pair(96, 160, -38, 36, 21), 3, "valid")
    else:
        r = ref(("long", levels), lambda: wide_pair(levels, 96, 160, 2 if levels == 5 else 0), levels, "valid")
    assert np.abs(r[2]).max() > {3: 16, 4: 32, 5: 64}[levels]
    check_field(G, [r], levels, "valid")
    check_frames(G, r, 8, 0, 9)


# ---- the frames ------------------------------------------------------------------------------------------------------------------
def test_sample_rates_one_and_1024():
    G = handle()
    r = translation_refs(4)[1]                                          # d = (-32, 8)
    frames = check_frames(G, r, 1, 0, 2)
    assert np.array_equal(frames[0], r[0]) and np.array_equal(frames[1], r[1])
    for k in (0, 1, 512, 1023, 1024):
        check_frames(G, r, bg.MAX_SAMPLE_RATE, k, 1)
    r = ref(("long", 5), lambda: wide_pair(5, 96, 160, 2), 5, "valid")          # the widest field at the largest rate
    for k in (1, 1023):
        check_frames(G, r, bg.MAX_SAMPLE_RATE, k, 1)


@pytest.mark.parametrize("h,w", [(16, 1030), (67, 93)])
def test_outputs_strips_and_unaligned_destinations(h, w):
    """W = 1030: a thread takes a second strip of four pixels, W % 4 = 2; W = 93: W % 4 = 1.  Float only, uint8 only and both;
    then the uint8 output 1 and 7 bytes off a 16-byte line of a larger allocation, around which nothing may change."""
    G = handle()
    r = ref(("strip", h, w), lambda: moving_pair(h, w, 36, -4, 30 + h), 3, "valid")
    a, b, f = r
    assert f.any()
    want = check_frames(G, r, 4, 1, 3, normalised="both")
    assert not np.array_equal(want, bg.mci_frames_host(a, b, f, 4, [1, 2, 3]))
    check_frames(G, r, 4, 1, 3, normalised=True)
    check_frames(G, r, 4, 1, 3, normalised=False)
    ta, tb, tf = dev(G, a, b, f)
    n = 3 * h * w * 3
    for off in (1, 7):
        buf = torch.full((off + n + 64,), 77, dtype=torch.uint8, device=G.device)
        out = buf[off:off + n].view(3, h, w, 3)
        assert out.data_ptr() % 16 == off
        G.mci_frames(ta, tb, tf, 4, normalised=False, out=out, border="valid")
        host = buf.cpu()
        assert torch.equal(host[off:off + n].view(3, h, w, 3), torch.from_numpy(want)), off
        assert (host[:off] == 77).all() and (host[off + n:] == 77).all(), off


# ---- mode equivalence and errors ---------------------------------------------------------------------------------------------------
def test_the_clamp_border_is_the_default_at_every_level():
    """On saturated, tied, tiny and wide inputs at their levels (mci_gpu_common.check_defaults)."""
    G = handle()
    inputs = [(5, wide_pair(5, 96, 160, 1)), (4, wide_pair(4, 67, 93, 0)), (3, tie_pair("checker8", 67, 93)), (3, random_pair(33, 15, 1)),
              (4, random_pair(1, 1, 1)), (3, moving_pair(16, 1030, 36, -4, 46))]
    for levels, (a, b) in inputs:
        check_defaults(G, a, b, levels)


def test_a_bad_border_through_the_c_abi():
    G = handle()
    L = G._lib
    h, w = 40, 56
    a, b = random_pair(h, w, 1)
    ta, tb = dev(G, a, b)
    Hb, Wb = bg.field_shape(h, w)
    ws = torch.empty(L.rib_mci_workspace_bytes(G._h, 1, h, w, 3), dtype=torch.uint8, device=G.device)
    zero = torch.zeros((Hb, Wb, 2), dtype=torch.int16, device=G.device)
    for bad in (2, -1, 255):
        field = torch.full((Hb, Wb, 2), 77, dtype=torch.int16, device=G.device)
        rc = L.rib_mci_field(G._h, 1, h, w, ta.data_ptr(), tb.data_ptr(), field.data_ptr(), 3, bad, ws.data_ptr(), None)
        assert rc == RIB_ERR_INVALID and b"border=%d" % bad in L.rib_last_error(G._h)
        out = torch.full((1, 1, h, w, 3), 9, dtype=torch.uint8, device=G.device)
        rc = L.rib_mci_frames(G._h, 1, 1, h, w, ta.data_ptr(), tb.data_ptr(), zero.data_ptr(), 4, 1, bad, None, out.data_ptr(), None)
        assert rc == RIB_ERR_INVALID and b"border=%d" % bad in L.rib_last_error(G._h)
        torch.cuda.synchronize()
        assert (field == 77).all() and (out == 9).all()                     # nothing was launched
    for bad in ("edge", 1, None):
        with pytest.raises(ValueError, match="border must be"):
            G.mci_field(ta, tb, border=bad)
        with pytest.raises(ValueError, match="border must be"):
            G.mci_frames(ta, tb, zero, 4, border=bad)


# ---- the driver ------------------------------------------------------------------------------------------------------------------
def test_native_folder_driver_with_the_valid_border(tmp_path):
    """background="mci", mci_range=64, mci_border="valid" at 64 x 64, two clips of three key frames 48 px (40 x 24 px) apart,
    batch 2: the native path's PNGs and .avi are the reference-protocol path's through the same Generator, byte for byte; two
    ranks write one rank's files; the default's files are an explicit "clamp"'s, and not "valid"'s."""
    root = str(tmp_path)
    keys = write_moving_clips(root, n_key=3)
    G = handle()
    cfg = rib.AttrDict(gen=rib.hsm_gen_config(), model_height=64, model_width=64, gauss_sigma=5, skeleton_thres=0.001, foot_thres=0.001)
    inputs, poses = os.path.join(root, "inputs"), os.path.join(root, "Predict_motion")
    kw = dict(background="mci", mci_range=64, video=True)
    run = lambda name, model=G, **more: (ev.Evaluator(cfg, batch=2, chunk=2, lanes=1) if model is G else ev.Evaluator(cfg)).evaluate_from_folder(
        model, inputs, None, poses, os.path.join(root, name), **dict(kw, **more))
    nat = run("nat", mci_border="valid")
    plain, clamp = run("plain"), run("clamp", mci_border="clamp")
    two = []
    for r in (1, 0):
        two += run("two", mci_border="valid", video=False, rank=r, world=2)
    before = G.plan_batch
    G.set_plan_batch(2)                         # the reference-protocol path follows the plans the native group follows
    try:
        refw = run("ref", model=Protocol(G), mci_border="valid")
    finally:
        G.set_plan_batch(before)
    assert len(nat) == len(refw) == len(plain) == len(clamp) == len(two) == 10
    read = lambda files: {os.path.relpath(x, root).split(os.sep, 1)[1]: open(x, "rb").read() for x in files}
    assert read(nat) == read(refw) == read(two)
    assert read(plain) == read(clamp)
    for clip in keys:
        avi = {d: open(os.path.join(root, d, clip + "_video.avi"), "rb").read() for d in ("nat", "ref", "plain", "clamp")}
        assert avi["nat"] == avi["ref"] and avi["plain"] == avi["clamp"] and avi["nat"] != avi["plain"]
    # key frames pass through; a frame in between differs from clamp's wherever the definition's background does
    want = []
    for frames in keys.values():
        for a, b in zip(frames, frames[1:]):
            mid = [bg.mci_frames_host(a, b, bg.mci_field_host(a, b, 4, border=m), 2, [1], border=m) for m in bg.BORDERS]
            want += [False, not np.array_equal(*mid)]
        want.append(False)
    assert sum(want) >= 2 and [open(x, "rb").read() != open(y, "rb").read() for x, y in zip(nat, clamp)] == want
