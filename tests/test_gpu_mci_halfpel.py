"""rib_halfpel_refine / rib_halfpel_frames (csrc/mci.hip.h: k_mci_refine<VALID>, k_mci_frames<VALID, true>; Generator.mci_refine /
mci_frames(..., precision="half")) - the half-pel refinement of the interpolated backgrounds - against background.py's
mci_refine_host and mci_frames_host(precision="half"), bit for bit, and the folder driver with mci_precision="half".  What the
definition itself guarantees is held in tests/test_mci_halfpel_cpu.py."""
import os

import numpy as np
import pytest
import torch

import render_in_between_amd as rib
from render_in_between_amd import background as bg, evaluator as ev
from tests.mci_gpu_common import dev
from tests.test_background_cpu import moving_pair, random_pair, tie_pair
from tests.test_gpu_mci import Protocol, handle
from tests.test_mci_halfpel_cpu import LOOP_TIE_KINDS, MAXD, random_field, write_odd_clips

pytestmark = pytest.mark.gpu

RIB_ERR_INVALID = -1                                                    # include/rib.h
SIZES = [(1, 1), (7, 9), (33, 15), (67, 93), (96, 128), (40, 1030)]     # partial border blocks, a last run of fewer than 8 blocks
_CASES = {}


def case(h, w, kind="odd"):
    """(a, b, integer field per border, refined field per border) of one input, made once."""
    if (h, w, kind) not in _CASES:
        if kind == "odd":                                               # an odd pan: the refinement moves most blocks
            a, b = moving_pair(h, w, 7 if w > 20 else 1, -3 if h > 20 else 1, 9)
            fields = {m: bg.mci_field_host(a, b, 3, m) for m in bg.BORDERS}
        elif kind == "random":                                          # windows far outside the frame
            a, b = random_pair(h, w, 2)
            fields = {m: random_field(h, w, 5) for m in bg.BORDERS}
        else:                                                           # periodic: the key's lower fields decide
            a, b = tie_pair(kind, h, w)
            fields = {m: np.zeros(bg.field_shape(h, w) + (2,), np.int16) for m in bg.BORDERS}
        _CASES[h, w, kind] = (a, b, fields, {m: bg.mci_refine_host(a, b, fields[m], m) for m in bg.BORDERS})
    return _CASES[h, w, kind]


def check_refine(G, cases, border):
    """A batch of cases in one call against the definition, exactly -> the device result."""
    ta, tb, tf = dev(G, np.stack([c[0] for c in cases]), np.stack([c[1] for c in cases]), np.stack([c[2][border] for c in cases]))
    got = G.mci_refine(ta, tb, tf, border=border)
    want = np.stack([c[3][border] for c in cases])
    assert got.dtype == torch.int16 and tuple(got.shape) == want.shape and got.data_ptr() != tf.data_ptr()
    assert torch.equal(got.cpu(), torch.from_numpy(want)), (border, cases[0][0].shape, int((got.cpu().numpy() != want).any(-1).sum()))
    return got


# ---- the refinement ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("border", bg.BORDERS)
@pytest.mark.parametrize("h,w", SIZES)
def test_refine_is_the_definition(h, w, border):
    G = handle()
    moved = 0
    for kind in ("odd", "random"):
        c = case(h, w, kind)
        check_refine(G, [c], border)
        moved += int((c[3][border] != 2 * c[2][border]).any())
    assert moved or (h, w) == (1, 1)
    if (h, w) == (67, 93):                                              # [H,W,3] inputs and an [Hb,Wb,2] field give an [Hb,Wb,2] field
        c = case(h, w)
        ta, tb, tf = dev(G, c[0], c[1], c[2][border])
        assert torch.equal(G.mci_refine(ta, tb, tf, border=border).cpu(), torch.from_numpy(c[3][border]))


@pytest.mark.parametrize("border", bg.BORDERS)
def test_a_batch_is_its_segments_alone(border):
    G = handle()
    cases = [case(67, 93), case(67, 93, "random"), case(67, 93, "checker8")]
    batch = check_refine(G, cases, border)
    for i, c in enumerate(cases):
        assert torch.equal(check_refine(G, [c], border)[0], batch[i])


@pytest.mark.parametrize("border", bg.BORDERS)
def test_ties_are_decided_by_the_key(border):
    G = handle()
    cases = [case(33, 15, kind) for kind in LOOP_TIE_KINDS]
    assert any((c[3][border] != 0).any() for c in cases)
    check_refine(G, cases, border)


@pytest.mark.parametrize("border", bg.BORDERS)
def test_in_place_and_on_another_stream(border):
    G = handle()
    c = case(67, 93)
    want = torch.from_numpy(c[3][border])
    ta, tb, tf = dev(G, c[0], c[1], c[2][border])
    assert G.mci_refine(ta, tb, tf, border=border, out=tf).data_ptr() == tf.data_ptr() and torch.equal(tf.cpu(), want)       # in place
    ta, tb, tf = dev(G, np.stack([c[0]] * 2), np.stack([c[1]] * 2), np.stack([c[2][border]] * 2))
    torch.cuda.synchronize()
    st = torch.cuda.Stream(device=G.device)
    with torch.cuda.stream(st):
        got = G.mci_refine(ta, tb, tf, border=border)
        again = G.mci_refine(ta, tb, tf, border=border, out=tf)
    st.synchronize()
    assert torch.equal(got[0].cpu(), want) and torch.equal(got[1].cpu(), want) and torch.equal(again.cpu(), got.cpu())
    with pytest.raises(ValueError, match="out must be"):
        G.mci_refine(ta, tb, tf, border=border, out=tf[:1])
    with pytest.raises(ValueError, match="the field of 2 67x93 segments"):
        G.mci_refine(ta, tb, tf[:, :3], border=border)


# ---- the frames --------------------------------------------------------------------------------------------------------------------
def check_frames(G, a, b, f, s, k_first, count, border, normalised="both"):
    ta, tb, tf = dev(G, a, b, f)
    want = bg.mci_frames_host(a, b, f, s, range(k_first, k_first + count), border=border, precision="half")
    got = G.mci_frames(ta, tb, tf, s, k_first=k_first, count=count, normalised=normalised, border=border, precision="half")
    f32, u8 = got if normalised == "both" else (got, None) if normalised else (None, got)
    if u8 is not None:
        assert torch.equal(u8.cpu(), torch.from_numpy(want)), (a.shape, s, k_first, border)
    if f32 is not None:
        assert torch.equal(f32.cpu(), torch.from_numpy(bg.normalised_upload(want))), (a.shape, s, k_first, border)
    return want


@pytest.mark.parametrize("border", bg.BORDERS)
@pytest.mark.parametrize("h,w", [(67, 93), (96, 128), (40, 1030)])
def test_half_frames_are_the_definition(h, w, border):
    """W = 93: scalar stores; 128: float4 stores; 1030: a thread's second strip.  s = 8, every k; k = 0 and k = s are the key
    frames; float only and uint8 only; the doubled integer field gives precision="full"'s bytes."""
    G = handle()
    a, b, fields, refined = case(h, w)
    f, r = fields[border], refined[border]
    assert (r & 1).any()                                                # half-pel vectors are in use
    frames = check_frames(G, a, b, r, 8, 0, 9, border)
    assert np.array_equal(frames[0], a) and np.array_equal(frames[8], b)
    assert not np.array_equal(frames[3], bg.mci_frames_host(a, b, f, 8, [3], border=border)[0])
    check_frames(G, a, b, r, 8, 1, 7, border, normalised=True)
    check_frames(G, a, b, r, 8, 3, 2, border, normalised=False)
    ta, tb, tf = dev(G, a, b, f)
    full = G.mci_frames(ta, tb, tf, 8, k_first=0, count=9, normalised="both", border=border)
    half = G.mci_frames(ta, tb, 2 * tf, 8, k_first=0, count=9, normalised="both", border=border, precision="half")
    assert torch.equal(full[0], half[0]) and torch.equal(full[1], half[1])
    assert torch.equal(full[1].cpu(), torch.from_numpy(bg.mci_frames_host(a, b, f, 8, range(9), border=border)))


@pytest.mark.parametrize("border", bg.BORDERS)
def test_the_largest_rate_on_the_widest_field(border):
    G = handle()
    h, w = 67, 93
    a, b = random_pair(h, w, 4)
    r = (2 * random_field(h, w, 7).astype(np.int32) + np.random.default_rng(3).integers(-1, 2, bg.field_shape(h, w) + (2,))).astype(np.int16)
    r[0, 0], r[-1, -1], r[0, -1] = (159, -159), (-159, 159), (159, 159)
    assert np.abs(r).max() == 2 * MAXD + 1 == 159
    for k in (1, 512, 1023):
        check_frames(G, a, b, r, bg.MAX_SAMPLE_RATE, k, 1, border)
    ends = check_frames(G, a, b, r, bg.MAX_SAMPLE_RATE, 0, 1, border), check_frames(G, a, b, r, bg.MAX_SAMPLE_RATE, 1024, 1, border)
    assert np.array_equal(ends[0][0], a) and np.array_equal(ends[1][0], b)
    ends = check_frames(G, a, b, r, 1, 0, 2, border)
    assert np.array_equal(ends[0], a) and np.array_equal(ends[1], b)


@pytest.mark.parametrize("border", bg.BORDERS)
def test_an_output_off_a_16_byte_line(border):
    G = handle()
    h, w = 67, 93
    a, b, _, refined = case(h, w)
    r = refined[border]
    want = bg.mci_frames_host(a, b, r, 4, [1, 2, 3], border=border, precision="half")
    ta, tb, tr = dev(G, a, b, r)
    n = 3 * h * w * 3
    for off in (1, 7):
        buf = torch.full((off + n + 64,), 77, dtype=torch.uint8, device=G.device)
        out = buf[off:off + n].view(3, h, w, 3)
        assert out.data_ptr() % 16 == off
        G.mci_frames(ta, tb, tr, 4, normalised=False, out=out, border=border, precision="half")
        host = buf.cpu()
        assert torch.equal(host[off:off + n].view(3, h, w, 3), torch.from_numpy(want)), off
        assert (host[:off] == 77).all() and (host[off + n:] == 77).all(), off


# ---- the raw C ABI -----------------------------------------------------------------------------------------------------------------
def test_refusals_through_the_c_abi():
    G = handle()
    L = G._lib
    h, w = 40, 56
    a, b = random_pair(h, w, 1)
    ta, tb = dev(G, a, b)
    Hb, Wb = bg.field_shape(h, w)
    zero = torch.zeros((Hb, Wb, 2), dtype=torch.int16, device=G.device)

    def fresh():
        return (torch.full((Hb, Wb, 2), 77, dtype=torch.int16, device=G.device), torch.full((1, 1, h, w, 3), 9, dtype=torch.uint8, device=G.device),
                torch.full((1, 1, 3, h, w), 7.0, device=G.device))

    def refused(rc, text, sentinels):
        assert rc == RIB_ERR_INVALID and text in L.rib_last_error(G._h), (rc, text, L.rib_last_error(G._h))
        torch.cuda.synchronize()
        field, u8, f32 = sentinels
        assert (field == 77).all() and (u8 == 9).all() and (f32 == 7.0).all()          # nothing was launched
    p = lambda t: t.data_ptr()
    for bad in (2, -1, 255):
        s = fresh()
        refused(L.rib_halfpel_refine(G._h, 1, h, w, p(ta), p(tb), p(zero), p(s[0]), bad, None), b"rib_halfpel_refine: border=%d" % bad, s)
        refused(L.rib_halfpel_frames(G._h, 1, 1, h, w, p(ta), p(tb), p(zero), 4, 1, bad, p(s[2]), p(s[1]), None), b"rib_halfpel_frames: border=%d" % bad, s)
    s = fresh()
    refused(L.rib_halfpel_refine(G._h, 1, h, w, p(ta), p(tb), p(zero), None, 0, None), b"rib_halfpel_refine: null pointer", s)
    refused(L.rib_halfpel_refine(G._h, 1, h, w, p(ta), None, p(zero), p(s[0]), 0, None), b"rib_halfpel_refine: null pointer", s)
    refused(L.rib_halfpel_refine(G._h, 1, h, w, p(ta), p(tb), p(zero), p(s[0]) + 2, 0, None), b"rib_halfpel_refine: the fields must be 4-byte aligned", s)
    refused(L.rib_halfpel_refine(G._h, 0, h, w, p(ta), p(tb), p(zero), p(s[0]), 0, None), b"rib_halfpel_refine: B=0", s)
    refused(L.rib_halfpel_refine(G._h, 1, h, 16385, p(ta), p(tb), p(zero), p(s[0]), 0, None), b"rib_halfpel_refine: B=1 H=40 W=16385", s)
    refused(L.rib_halfpel_frames(G._h, 1, 1, h, w, p(ta), p(tb), p(zero), 4, 1, 0, None, None, None), b"rib_halfpel_frames: both outputs are null", s)
    refused(L.rib_halfpel_frames(G._h, 1, 1, h, w, p(ta), p(tb), None, 4, 1, 0, p(s[2]), p(s[1]), None), b"rib_halfpel_frames: null pointer", s)
    refused(L.rib_halfpel_frames(G._h, 2, 1, h, w, p(ta), p(tb), p(zero), 4, 4, 0, p(s[2]), p(s[1]), None),
            b"rib_halfpel_frames: frames 4..5 are outside the segment 0..4", s)
    refused(L.rib_halfpel_frames(G._h, 1, 1, h, w, p(ta), p(tb), p(zero), 4, -1, 0, p(s[2]), p(s[1]), None), b"rib_halfpel_frames: frames -1..-1", s)
    refused(L.rib_halfpel_frames(G._h, 1, 1, h, w, p(ta), p(tb), p(zero), 6, 1, 0, p(s[2]), p(s[1]), None), b"rib_halfpel_frames: sample_rate=6", s)
    refused(L.rib_halfpel_frames(G._h, 0, 1, h, w, p(ta), p(tb), p(zero), 4, 1, 0, p(s[2]), p(s[1]), None), b"rib_halfpel_frames: T=0", s)
    refused(L.rib_mci_frames(G._h, 2, 1, h, w, p(ta), p(tb), p(zero), 4, 4, 0, p(s[2]), p(s[1]), None),
            b"rib_mci_frames: frames 4..5 are outside the segment 0..4", s)            # the shared body keeps the first entry's texts
    # and the entries work: the raw calls give the Generator's results
    raw = torch.full((Hb, Wb, 2), 77, dtype=torch.int16, device=G.device)
    f = torch.from_numpy(random_field(h, w, 2, 9)).to(G.device)
    assert L.rib_halfpel_refine(G._h, 1, h, w, p(ta), p(tb), p(f), p(raw), 1, None) == 0
    assert L.rib_halfpel_frames(G._h, 1, 1, h, w, p(ta), p(tb), p(raw), 4, 1, 1, None, p(s[1]), None) == 0
    torch.cuda.synchronize()
    assert torch.equal(raw, G.mci_refine(ta, tb, f, border="valid"))
    assert torch.equal(s[1][0], G.mci_frames(ta, tb, raw, 4, k_first=1, count=1, normalised=False, border="valid", precision="half"))
    for bad in ("quarter", 1, None):
        with pytest.raises(ValueError, match="precision must be"):
            G.mci_frames(ta, tb, zero, 4, precision=bad)


# ---- the driver ------------------------------------------------------------------------------------------------------------------
def test_native_folder_driver_with_half_pel_precision(tmp_path):
    """background="mci", mci_border="valid", mci_precision="half" at 64 x 64, two clips of three key frames an odd number of
    pixels apart, batch 2: the native path's PNGs and .avi are the reference-protocol path's through the same Generator, byte
    for byte; two ranks write one rank's files; the default's files are an explicit "full"'s, and not "half"'s."""
    root = str(tmp_path)
    keys = write_odd_clips(root, n_key=3)
    G = handle()
    cfg = rib.AttrDict(gen=rib.hsm_gen_config(), model_height=64, model_width=64, gauss_sigma=5, skeleton_thres=0.001, foot_thres=0.001)
    inputs, poses = os.path.join(root, "inputs"), os.path.join(root, "Predict_motion")
    kw = dict(background="mci", mci_border="valid", video=True)
    run = lambda name, model=G, **more: (ev.Evaluator(cfg, batch=2, chunk=2, lanes=1) if model is G else ev.Evaluator(cfg)).evaluate_from_folder(
        model, inputs, None, poses, os.path.join(root, name), **dict(kw, **more))
    nat = run("nat", mci_precision="half")
    plain, full = run("plain"), run("full", mci_precision="full")
    two = []
    for r in (1, 0):
        two += run("two", mci_precision="half", video=False, rank=r, world=2)
    before = G.plan_batch
    G.set_plan_batch(2)                         # the reference-protocol path follows the plans the native group follows
    try:
        refw = run("ref", model=Protocol(G), mci_precision="half")
    finally:
        G.set_plan_batch(before)
    assert len(nat) == len(refw) == len(plain) == len(full) == len(two) == 10
    read = lambda files: {os.path.relpath(x, root).split(os.sep, 1)[1]: open(x, "rb").read() for x in files}
    assert read(nat) == read(refw) == read(two)
    assert read(plain) == read(full)
    for clip in keys:
        avi = {d: open(os.path.join(root, d, clip + "_video.avi"), "rb").read() for d in ("nat", "ref", "plain", "full")}
        assert avi["nat"] == avi["ref"] and avi["plain"] == avi["full"] and avi["nat"] != avi["plain"]
    # key frames pass through; a frame in between differs from full's wherever the definition's background does
    want = []
    for frames in keys.values():
        for a, b in zip(frames, frames[1:]):
            f = bg.mci_field_host(a, b, 3, border="valid")
            mid = [bg.mci_frames_host(a, b, f, 2, [1], border="valid"),
                   bg.mci_frames_host(a, b, bg.mci_refine_host(a, b, f, border="valid"), 2, [1], border="valid", precision="half")]
            want += [False, not np.array_equal(*mid)]
        want.append(False)
    assert sum(want) >= 2 and [open(x, "rb").read() != open(y, "rb").read() for x, y in zip(nat, full)] == want
