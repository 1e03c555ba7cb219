"""rib_detail_field (csrc/mci.hip.h: k_detail_search<R, VALID> and k_mci_median; Generator.mci_detail_field) - the block field
refined at the key frames' own size - against the integer definition background.mci_detail_field_host, bit for bit, and the existing
frame entries fed fields as long as it can make.  The inputs are tests/mci_detail_common.py's; the shapes are the smallest at which
the kernel can go wrong: partial blocks on both axes and a run that ends mid-workgroup (61x99), every radius 1..4 (81 candidates
over 64 lanes among them), key frames smaller than the model, and starts far outside the frame."""
import os

import numpy as np
import pytest
import torch

import render_in_between_amd as rib
from render_in_between_amd import background as bg, evaluator as ev
from tests import mci_detail_common as dc
from tests.mci_gpu_common import dev
from tests.test_gpu_mci import Protocol, handle

pytestmark = pytest.mark.gpu

RIB_ERR_INVALID = -1                                                    # include/rib.h
VARIANTS = [(b, p) for b in bg.BORDERS for p in bg.PRECISIONS]
RADIUS = [2, 3, 4, 1, 1, 4]                                             # of dc.SHAPES, in order


@pytest.mark.parametrize("case", range(len(dc.SHAPES)))
def test_field_against_the_definition(case):
    model, size, B, amp = dc.SHAPES[case]
    assert bg.detail_radius(model, size) == RADIUS[case]
    G = handle()
    ta, tb = dev(G, *dc.pairs(size, B))
    for border, precision in VARIANTS:
        want = dc.want_fields(model, size, B, amp, border, precision)
        (tf,) = dev(G, dc.random_fields(model, B, amp, precision))
        got = G.mci_detail_field(ta, tb, tf, model, border=border, precision=precision)
        assert got.dtype == torch.int16 and tuple(got.shape) == (B,) + bg.field_shape(*size) + (2,)
        assert torch.equal(got.cpu(), torch.from_numpy(want)), (border, precision)
        one = G.mci_detail_field(ta[0], tb[0], tf[0], model, border=border, precision=precision)      # [h0,w0,3] key frames: no batch axis
        assert torch.equal(one, got[0])


@pytest.mark.parametrize("case", [0, 2, 3])
def test_constant_frames_where_every_cost_ties(case):
    """One colour per key frame: the SAD of every candidate of a block is the same, so (|d|^2, dy, dx) and LAMBDA's term decide."""
    model, size, B, amp = dc.SHAPES[case]
    G = handle()
    ta, tb = dev(G, *dc.pairs(size, B, "constant"))
    for border, precision in VARIANTS:
        want = dc.want_fields(model, size, B, amp, border, precision, "constant")
        (tf,) = dev(G, dc.random_fields(model, B, amp, precision))
        got = G.mci_detail_field(ta, tb, tf, model, border=border, precision=precision)
        assert torch.equal(got.cpu(), torch.from_numpy(want)), (border, precision)


def test_a_segments_field_does_not_depend_on_the_batch():
    model, size, B, amp = dc.SHAPES[0]
    G = handle()
    a, b = dc.pairs(size, B)
    for border, precision in VARIANTS:
        f = dc.random_fields(model, B, amp, precision)
        ta, tb, tf = dev(G, a, b, f)
        all3 = G.mci_detail_field(ta, tb, tf, model, border=border, precision=precision)
        for i in range(B):
            one = G.mci_detail_field(ta[i:i + 1], tb[i:i + 1], tf[i:i + 1], model, border=border, precision=precision)
            assert torch.equal(one[0], all3[i]), (border, precision, i)


@pytest.mark.parametrize("h,w", [(128, 128), (3, 4099)])
def test_the_frame_entries_with_vectors_this_long(h, w):
    """rib_mci_frames and rib_cubic_frames (staging 0 and 1) at the key frames' size with components up to +-1268, both borders,
    against mci_frames_host: the field a refined 16x enlargement can hold, at the largest rate too."""
    G = handle()
    a, b = (x[0] for x in dc.pairs((h, w), 1))
    f = dc.long_field(h, w, 0)
    assert int(np.abs(f).max()) == bg.DETAIL_MAX_DISP == 1268
    ta, tb, tf = dev(G, a, b, f)
    for s, k_first, T in ((8, 0, 9), (1024, 1021, 3)):
        ks = range(k_first, k_first + T)
        for border in bg.BORDERS:
            for sampler, stagings in (("bilinear", (0,)), ("cubic", (0, 1))):
                want = bg.mci_frames_host(a, b, f, s, ks, border=border, sampler=sampler)
                for st in stagings:
                    got = G.mci_frames(ta, tb, tf, s, k_first=k_first, count=T, normalised=False, border=border, sampler=sampler, _staging=st)
                    assert torch.equal(got.cpu(), torch.from_numpy(want)), (s, border, sampler, st)


def test_refusals_launch_nothing():
    G = handle()
    L, H_ = G._lib, G._h
    model, size, B, amp = dc.SHAPES[0]
    (H, W), (H0, W0) = model, size
    a, b = dc.pairs(size, B)
    ta, tb, tf = dev(G, a, b, dc.random_fields(model, B, amp, "full"))
    H0b, W0b = bg.field_shape(H0, W0)
    out = torch.full((B, H0b, W0b, 2), 77, dtype=torch.int16, device=G.device)
    n = int(L.rib_detail_workspace_bytes(H_, B, H0, W0))
    assert n >= B * H0b * W0b * 4 and n % 256 == 0
    ws = torch.full((n + 16,), 9, dtype=torch.uint8, device=G.device)
    p = lambda t: t.data_ptr() if t is not None else None

    def call(B=B, H=H, W=W, H0=H0, W0=W0, a=p(ta), b=p(tb), fld=p(tf), precision=0, border=0, o=p(out), w=p(ws)):
        return L.rib_detail_field(H_, B, H, W, H0, W0, a, b, fld, precision, border, o, w, None)

    cases = [(dict(B=0), b"B=0"), (dict(B=32768), b"B=32768"), (dict(H=0), b"H=0"), (dict(W=16385), b"W=16385"), (dict(H0=0), b"H0=0"),
             (dict(W0=16385), b"W0=16385"), (dict(W0=16 * W + 1), b"within 1/16"), (dict(H0=1), b"within 1/16"), (dict(precision=2), b"precision=2"),
             (dict(precision=-1), b"precision=-1"), (dict(border=2), b"border=2"), (dict(a=None), b"null pointer"), (dict(b=None), b"null pointer"),
             (dict(fld=None), b"null pointer"), (dict(o=None), b"null pointer"), (dict(w=None), b"null pointer"), (dict(w=p(ws) + 8), b"16-byte aligned"),
             (dict(fld=p(tf) + 2), b"4-byte aligned"), (dict(o=p(out) + 2), b"4-byte aligned")]
    for kw, text in cases:
        assert call(**kw) == RIB_ERR_INVALID, kw
        assert L.rib_last_error(H_).startswith(b"rib_detail_field") and text in L.rib_last_error(H_), (kw, L.rib_last_error(H_))
    for bad in ((0, H0, W0), (B, 0, W0), (B, H0, 16385)):
        assert int(L.rib_detail_workspace_bytes(H_, *bad)) == 0
    torch.cuda.synchronize()
    assert bool((out == 77).all()) and bool((ws == 9).all())                          # nothing was launched
    with pytest.raises(ValueError, match="border must be"):
        G.mci_detail_field(ta, tb, tf, model, border="wrap")
    with pytest.raises(ValueError, match="precision must be"):
        G.mci_detail_field(ta, tb, tf, model, precision="quarter")
    with pytest.raises(ValueError, match=r"is \[3, 3, 5, 2\]"):
        G.mci_detail_field(ta, tb, tf[:, :2], model)
    with pytest.raises(ValueError, match="within 1/16"):
        G.mci_detail_field(ta, tb, tf, (2, 40))
    assert call(border=1) == 0                                                          # and the good call is accepted: the raw entry gives the Generator's result
    torch.cuda.synchronize()
    assert torch.equal(out, G.mci_detail_field(ta, tb, tf, model, border="valid"))
    assert bool((ws[n:] == 9).all())                                                    # the workspace ends where the query says


# ---- the folder driver -------------------------------------------------------------------------------------------------------------
def _tree(root):
    out = {}
    for d, _, files in os.walk(root):
        for n in files:
            out[os.path.relpath(os.path.join(d, n), root)] = open(os.path.join(d, n), "rb").read()
    return out


def test_native_folder_driver_with_the_refined_field(tmp_path):
    """64x64 model, 160x160 key frames (ratio 2.5, R = 2), two clips of three key frames whose scenes move by a number of pixels that
    is no multiple of the ratio, batch 2: under mci_detail="keyframes" the native path's PNGs and _video.avi are the reference-protocol
    path's (the host definition) through the same Generator, byte for byte, and two ranks write one rank's PNGs; they are not the
    files of mci_detail="model", which are the files of a run without the setting."""
    from tests.composite_common import write_example
    from tests.test_keyframes_size_cpu import moving_keys
    root = str(tmp_path)
    for clip, seed, step in (("clipA", 1, (6, -2)), ("clipB", 2, (-3, 7))):
        write_example(root, n_key=3, rate=4, key_hw=(160, 160), clip=clip, seed=seed)
        moving_keys(root, 3, (160, 160), clip=clip, step=step)
    inputs, poses = os.path.join(root, "inputs"), os.path.join(root, "Predict_motion")
    cfg = lambda: rib.AttrDict(gen=rib.hsm_gen_config(), model_height=64, model_width=64, gauss_sigma=5, skeleton_thres=0.001, foot_thres=0.001)
    G = handle()
    kw = dict(background="mci", output_size="keyframes", video=True)
    run = lambda name, model=G, **extra: (ev.Evaluator(cfg(), batch=2, chunk=2, lanes=1) if model is G else ev.Evaluator(cfg())).evaluate_from_folder(
        model, inputs, None, poses, os.path.join(root, name), **dict(kw, **extra))
    nat = run("nat", mci_detail="keyframes")
    plain, model = run("plain"), run("model", mci_detail="model")
    two = []
    for r in (1, 0):
        two += run("two", mci_detail="keyframes", video=False, rank=r, world=2)
    before = G.plan_batch
    G.set_plan_batch(2)                         # the reference-protocol path follows the plans the native group follows
    try:
        ref = run("ref", model=Protocol(G), mci_detail="keyframes")
    finally:
        G.set_plan_batch(before)
    assert len(nat) == len(ref) == len(plain) == len(model) == len(two) == 18
    a, b, c, d, e = (_tree(os.path.join(root, n)) for n in ("nat", "ref", "plain", "model", "two"))
    assert sorted(a) == sorted(b) == sorted(c) == sorted(d) and len(a) == 20 and "clipA_video.avi" in a
    for name in sorted(a):
        assert a[name] == b[name], name
    assert e == {n: v for n, v in a.items() if n.endswith(".png")}
    assert c == d
    assert a["clipA_video.avi"] != c["clipA_video.avi"] and a["clipB_video.avi"] != c["clipB_video.avi"]
    differing = [n for n in sorted(a) if a[n] != c[n]]
    assert len([n for n in differing if n.endswith(".png")]) >= 4      # a frame between the key frames of every segment, at the least
