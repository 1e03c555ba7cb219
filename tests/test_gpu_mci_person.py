"""rib_masked_field / rib_masked_frames (csrc/mci.hip.h: k_mci_mask_pyramid, k_mci_search<R, VALID, true>, k_mci_fill,
k_mci_frames<VALID, HALF, true>; Generator.mci_field_masked / mci_frames_masked) - the interpolated backgrounds with the person
kept out - against background.mci_field_masked_host / mci_frames_masked_host, bit for bit; and the folder driver with
mci_person="exclude".  The shapes are the smallest at which the kernels can go wrong: one pixel, one block, partial blocks and
odd pyramid planes, more than one run and tile, a fourth level, a row wider than one workgroup's pass."""
import os

import numpy as np
import pytest
import torch

import render_in_between_amd as rib
from render_in_between_amd import background as bg, evaluator as ev
from tests.mci_gpu_common import dev
from tests.test_background_cpu import moving_pair, random_pair
from tests.test_gpu_mci import Protocol, handle
from tests.test_mci_range_cpu import write_moving_clips

pytestmark = pytest.mark.gpu

RIB_ERR_INVALID = -1                                                    # include/rib.h
MASKS = ("disc", "edges", "noise25", "noise75", "noise50", "cells", "zero", "one")
# (h, w, levels): L = 3, 4, 5 where the planes still have something to match
SHAPES = [(1, 1, 3), (8, 8, 3), (8, 8, 5), (67, 93, 3), (67, 93, 4), (67, 93, 5), (160, 192, 3), (160, 192, 5), (128, 160, 4), (16, 2056, 3),
          (16, 2056, 5)]
_PAIRS, _MASKS, _FIELDS = {}, {}, {}


def pair(h, w):
    if (h, w) not in _PAIRS:
        _PAIRS[h, w] = random_pair(h, w, 3) if min(h, w) <= 8 else moving_pair(h, w, min(12, w // 8), -min(6, h // 8), 60 + h)
    return _PAIRS[h, w]


def masks(kind, h, w):
    """(ma, mb) uint8 [h, w], nonzero = excluded, values other than 1 among them."""
    if (kind, h, w) not in _MASKS:
        Y, X = np.mgrid[0:h, 0:w]
        rng = np.random.default_rng([MASKS.index(kind), h, w])
        if kind == "disc":                                              # a disc per key frame, moved between them
            r = max(min(h, w) // 4, 1)
            m = [((Y - h // 2 - dy) ** 2 + (X - w // 2 - dx) ** 2 <= r * r) for dx, dy in ((-w // 8, 1), (w // 8, -1))]
        elif kind == "edges":                                           # touches the top and the left edge / the bottom and the right
            m = [(Y < h // 3) | (X < w // 4), (Y >= h - h // 3) | (X >= w - w // 4)]
        elif kind.startswith("noise"):                                  # many candidates on either side of 4 n >= N: at 1/2 a pixel is
            m = [rng.random((h, w)) < int(kind[5:]) / 100.0 for _ in range(2)]      # clear in both masks with probability 1/4
        elif kind == "cells":                                           # 16 x 16 cells at 0.4: partly covered blocks on the coarse levels too
            m = [np.repeat(np.repeat(rng.random(((h + 15) // 16, (w + 15) // 16)) < 0.4, 16, 0), 16, 1)[:h, :w] for _ in range(2)]
        else:
            m = [np.full((h, w), kind == "one")] * 2
        _MASKS[kind, h, w] = tuple((x * rng.integers(1, 256, (h, w))).astype(np.uint8) for x in m)
    return _MASKS[kind, h, w]


def field_ref(kind, h, w, levels, border):
    key = (kind, h, w, levels, border)
    if key not in _FIELDS:
        _FIELDS[key] = bg.mci_field_masked_host(*pair(h, w), *masks(kind, h, w), levels, border)
    return _FIELDS[key]


@pytest.mark.parametrize("border", bg.BORDERS)
@pytest.mark.parametrize("h,w,levels", SHAPES)
def test_field_and_frames_against_the_definition(h, w, levels, border):
    """Every mask kind as one segment of one call (B = 8, eight different mask pairs): the field, then frames k = 0..4 of s = 4 in
    one launch, both outputs, both precisions (the half-pel field made as 2 * field) - all the definition's bytes."""
    G = handle()
    a, b = pair(h, w)
    B = len(MASKS)
    ma, mb = (np.stack([masks(k, h, w)[i] for k in MASKS]) for i in (0, 1))
    want = np.stack([field_ref(k, h, w, levels, border) for k in MASKS])
    ta, tb, tma, tmb = dev(G, np.stack([a] * B), np.stack([b] * B), ma, mb)
    field = G.mci_field_masked(ta, tb, tma, tmb, levels, border=border)
    assert field.dtype == torch.int16 and torch.equal(field.cpu(), torch.from_numpy(want))
    assert not want[MASKS.index("one")].any()
    s, ks = 4, range(5)
    for precision, unit in (("full", 1), ("half", 2)):
        f = (unit * want).astype(np.int16)
        tf, = dev(G, f)
        f32, u8 = G.mci_frames_masked(ta, tb, tma, tmb, tf, s, k_first=0, count=5, normalised="both", border=border, precision=precision)
        for i, kind in enumerate(MASKS):
            ref = bg.mci_frames_masked_host(a, b, ma[i], mb[i], f[i], s, ks, border, precision)
            assert np.array_equal(ref[0], a) and np.array_equal(ref[4], b)
            assert torch.equal(u8[:, i].cpu(), torch.from_numpy(ref)), (kind, precision)
            assert torch.equal(f32[:, i].cpu(), torch.from_numpy(bg.normalised_upload(ref))), (kind, precision)
            if kind == "zero":
                assert np.array_equal(ref, bg.mci_frames_host(a, b, f[i], s, ks, border, precision))


def test_a_segment_does_not_depend_on_the_batch_nor_a_frame_on_the_launch():
    """67 x 93, L = 4, border "valid": B = 3 with three different mask pairs - each segment's field and frames are its B = 1
    call's; T = 3 in one launch is three launches of one frame; one output at a time is the pair's."""
    G = handle()
    h, w, levels, border = 67, 93, 4, "valid"
    a, b = pair(h, w)
    kinds = ("disc", "noise25", "edges")
    ta, tb = dev(G, np.stack([a] * 3), np.stack([b] * 3))
    tma, tmb = dev(G, *(np.stack([masks(k, h, w)[i] for k in kinds]) for i in (0, 1)))
    field = G.mci_field_masked(ta, tb, tma, tmb, levels, border=border)
    f32, u8 = G.mci_frames_masked(ta, tb, tma, tmb, field, 8, k_first=2, count=3, normalised="both", border=border)
    for i in range(3):
        one = G.mci_field_masked(ta[i], tb[i], tma[i], tmb[i], levels, border=border)
        assert torch.equal(one, field[i])
        for t in range(3):
            g32, g8 = G.mci_frames_masked(ta[i], tb[i], tma[i], tmb[i], one, 8, k_first=2 + t, count=1, normalised="both", border=border)
            assert torch.equal(g32[0], f32[t, i]) and torch.equal(g8[0], u8[t, i])
    assert torch.equal(G.mci_frames_masked(ta, tb, tma, tmb, field, 8, k_first=2, count=3, normalised=True, border=border), f32)
    out = torch.full((3, 3, h, w, 3), 9, dtype=torch.uint8, device=G.device)
    assert G.mci_frames_masked(ta, tb, tma, tmb, field, 8, k_first=2, count=3, normalised=False, border=border, out=out) is out
    assert torch.equal(out, u8)


def test_refusals_launch_nothing():
    G = handle()
    L = G._lib
    h, w = 40, 56
    a, b = random_pair(h, w, 1)
    ma, mb = masks("disc", h, w)
    ta, tb, tma, tmb = dev(G, a, b, ma, mb)
    Hb, Wb = bg.field_shape(h, w)
    sizes = [L.rib_masked_workspace_bytes(G._h, 1, h, w, n) for n in (3, 4, 5)]
    assert all(s > L.rib_mci_workspace_bytes(G._h, 1, h, w, n) for s, n in zip(sizes, (3, 4, 5))) and sizes[0] < sizes[1] < sizes[2]
    assert L.rib_masked_workspace_bytes(G._h, 1, h, w, 2) == 0 and L.rib_masked_workspace_bytes(G._h, 0, h, w, 3) == 0
    ws = torch.empty(sizes[0], dtype=torch.uint8, device=G.device)
    zero = torch.zeros((Hb, Wb, 2), dtype=torch.int16, device=G.device)
    field = torch.full((Hb, Wb, 2), 77, dtype=torch.int16, device=G.device)
    out = torch.full((1, 1, h, w, 3), 9, dtype=torch.uint8, device=G.device)
    p = lambda t: t.data_ptr()
    good_field = dict(ma=p(tma), mb=p(tmb), levels=3, border=0)
    for bad, text in ((dict(ma=None), b"null pointer"), (dict(mb=None), b"null pointer"), (dict(levels=6), b"levels=6"), (dict(border=2), b"border=2")):
        kw = dict(good_field, **bad)
        rc = L.rib_masked_field(G._h, 1, h, w, p(ta), p(tb), kw["ma"], kw["mb"], p(field), kw["levels"], kw["border"], p(ws), None)
        assert rc == RIB_ERR_INVALID and text in L.rib_last_error(G._h) and b"rib_masked_field" in L.rib_last_error(G._h)
    good_frames = dict(ma=p(tma), mb=p(tmb), s=4, k=1, border=0, precision=0, out=p(out))
    for bad, text in ((dict(ma=None), b"null pointer"), (dict(mb=None), b"null pointer"), (dict(border=-1), b"border=-1"), (dict(precision=2), b"precision=2"),
                      (dict(s=3), b"sample_rate=3"), (dict(k=5), b"outside the segment"), (dict(out=None), b"both outputs are null")):
        kw = dict(good_frames, **bad)
        rc = L.rib_masked_frames(G._h, 1, 1, h, w, p(ta), p(tb), kw["ma"], kw["mb"], p(zero), kw["s"], kw["k"], kw["border"], kw["precision"], None,
                                 kw["out"], None)
        assert rc == RIB_ERR_INVALID and text in L.rib_last_error(G._h) and b"rib_masked_frames" in L.rib_last_error(G._h)
    torch.cuda.synchronize()
    assert (field == 77).all() and (out == 9).all()                         # nothing was launched
    with pytest.raises(ValueError, match="masks of"):
        G.mci_field_masked(ta, tb, tma[:-1], tmb)
    with pytest.raises(ValueError, match="uint8 tensor"):
        G.mci_frames_masked(ta, tb, tma.float(), tmb, zero, 4)


# ---- the driver ------------------------------------------------------------------------------------------------------------------
def test_native_folder_driver_with_the_person_excluded(tmp_path):
    """background="mci", mci_person="exclude" at 64 x 64, two clips of three key frames, batch 2: the native path's PNGs and .avi
    are the reference-protocol path's through the same Generator, byte for byte, and not the default's; the two combinations
    without a masked form are refused before any file exists."""
    root = str(tmp_path)
    keys = write_moving_clips(root, n_key=3)
    G = handle()
    cfg = rib.AttrDict(gen=rib.hsm_gen_config(), model_height=64, model_width=64, gauss_sigma=5, skeleton_thres=0.001, foot_thres=0.001)
    inputs, poses = os.path.join(root, "inputs"), os.path.join(root, "Predict_motion")
    kw = dict(background="mci", mci_range=64, video=True)
    run = lambda name, model=G, **more: (ev.Evaluator(cfg, batch=2, chunk=2, lanes=1) if model is G else ev.Evaluator(cfg)).evaluate_from_folder(
        model, inputs, None, poses, os.path.join(root, name), **dict(kw, **more))
    for name, more in (("half", dict(mci_precision="half")), ("keys", dict(output_size="keyframes"))):
        for model in (G, Protocol(G)):
            with pytest.raises(ValueError, match="mci_person='exclude' with"):
                run(name, model=model, mci_person="exclude", **more)
        assert not os.path.exists(os.path.join(root, name))
    with pytest.raises(ValueError, match="mci_person must be"):
        run("bad", mci_person="mask")
    nat = run("nat", mci_person="exclude")
    plain, keep = run("plain"), run("keep", mci_person="keep")
    before = G.plan_batch
    G.set_plan_batch(2)                         # the reference-protocol path follows the plans the native group follows
    try:
        refw = run("ref", model=Protocol(G), mci_person="exclude")
    finally:
        G.set_plan_batch(before)
    assert len(nat) == len(refw) == len(plain) == len(keep) == 10
    read = lambda files: {os.path.relpath(x, root).split(os.sep, 1)[1]: open(x, "rb").read() for x in files}
    assert read(nat) == read(refw) and read(plain) == read(keep) and read(nat) != read(plain)
    for clip in keys:
        avi = {d: open(os.path.join(root, d, clip + "_video.avi"), "rb").read() for d in ("nat", "ref", "plain", "keep")}
        assert avi["nat"] == avi["ref"] and avi["plain"] == avi["keep"] and avi["nat"] != avi["plain"]
