"""rib_accel_field / rib_accel_frames (csrc/mci.hip.h: k_mci_accel + k_mci_median, k_accel_frames<VALID, HALF, MASKED>,
k_cubic_accel<VALID, HALF, MASKED>; Generator.mci_accel_field / mci_frames_accel) - the second-order trajectory across key frames -
against the integer definition (background.mci_accel_host / mci_frames_accel_host), bit for bit, and the folder driver's
mci_motion="quadratic".  The inputs are tests/mci_motion_common.py's; tests/test_mci_motion_cpu.py proves with
background.cubic_tile_staged that the smooth acceleration field keeps the cubic tiles staged and the rough one makes them gather."""
import os

import numpy as np
import pytest
import torch

import render_in_between_amd as rib
from render_in_between_amd import background as bg, evaluator as ev
from tests import mci_cubic_common as cc, mci_motion_common as mc
from tests.mci_gpu_common import dev
from tests.test_background_cpu import random_pair
from tests.test_gpu_mci import Protocol, handle

pytestmark = pytest.mark.gpu

RIB_ERR_INVALID = -1                                                    # include/rib.h
PRESENT = {"both": [(1, 1)] * 3, "left": [(1, 0)] * 3, "right": [(0, 1)] * 3, "none": [(0, 0)] * 3, "mixed": [(1, 1), (0, 1), (1, 0)]}


def want_accel(f, present, shift):
    return np.stack([bg.mci_accel_host(f[0, b] if hp else None, f[1, b], f[2, b] if hn else None, unit_shift=shift) for b, (hp, hn) in enumerate(present)])


@pytest.mark.parametrize("Hb,Wb", [(9, 12), (1, 1)])
@pytest.mark.parametrize("precision", bg.PRECISIONS)
def test_accel_field_against_the_definition(Hb, Wb, precision):
    """B = 3, every presence combination - through NULL pointers where no item has the neighbour, through the byte array where the
    items differ (and where they agree: the same result) - random fields at full reach: the lookups clamp at every edge."""
    G = handle()
    shift = bg.PRECISIONS.index(precision)
    f = mc.random_fields(3, Hb, Wb, cc.REACH[precision], 7)
    tp, tc, tn = dev(G, f[0], f[1], f[2])
    for name, present in PRESENT.items():
        want = want_accel(f, present, shift)
        got = G.mci_accel_field(tp, tc, tn, precision=precision, present=present)
        assert got.dtype == torch.int16 and tuple(got.shape) == (3, Hb, Wb, 2)
        assert torch.equal(got.cpu(), torch.from_numpy(want)), (name, precision)
        if name != "mixed":                 # the same through the pointers alone
            hp, hn = present[0]
            alone = G.mci_accel_field(tp if hp else None, tc, tn if hn else None, precision=precision)
            assert torch.equal(alone, got), name
    assert want_accel(f, PRESENT["both"], shift).any() and not want_accel(f, PRESENT["none"], shift).any()
    one = G.mci_accel_field(tp[1], tc[1], tn[1], precision=precision)      # an item's result does not depend on B
    assert tuple(one.shape) == (Hb, Wb, 2) and torch.equal(one, G.mci_accel_field(tp, tc, tn, precision=precision)[1])


def _segments(h, w):
    """B = 2 segments: key frames, masks, fields of both units, per accel kind the acceleration field."""
    pairs = [random_pair(h, w, 31), random_pair(h, w, 32)]
    a, b = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    ma, mb = (np.stack([cc.masks("blobs", h, w)[i], cc.masks("blobs", h, w)[1 - i]]) for i in (0, 1))
    return a, b, ma, mb


@pytest.mark.parametrize("s,firsts", [(1, [0]), (8, [6]), (1024, [1022, 511])])
@pytest.mark.parametrize("h,w", [(67, 93), (96, 128)])
def test_accel_frames_against_the_definition(h, w, s, firsts):
    """T x B = 3 x 2 (2 x 2 at s = 1) with k = s among the frames (and, at s = 1024, the frames around s / 2 where the product
    UNIT k (s - k) Acc passes 2^32), both borders, both precisions, both samplers, plain and masked, float and uint8 outputs; the
    rough acceleration field throws samples out of the frame on all four sides, the smooth one keeps cubic tiles staged."""
    G = handle()
    a, b, ma, mb = _segments(h, w)
    ta, tb, tma, tmb = dev(G, a, b, ma, mb)
    for k0 in firsts:
        T = min(3, s + 1 - k0)
        ks = range(k0, k0 + T)
        for precision in bg.PRECISIONS:
            f = np.stack([cc.field("smooth", h, w, precision), cc.field("mixed", h, w, precision)])
            (tf,) = dev(G, f)
            for kind in ("rough", "smooth"):
                acc = np.stack([mc.accel_field(kind, h, w, 1), mc.accel_field(kind, h, w, 2)[::-1, ::-1].copy()])
                (tacc,) = dev(G, acc)
                for border in bg.BORDERS:
                    for sampler in (bg.SAMPLERS if kind == "rough" else ("cubic",)):
                        for masks, tm in ((None, None), ((ma, mb), (tma, tmb))):
                            kw = dict(border=border, precision=precision, sampler=sampler)
                            want = np.stack([bg.mci_frames_accel_host(a[i], b[i], f[i], acc[i], s, ks, **kw,
                                                                      **({} if masks is None else dict(ma=ma[i], mb=mb[i]))) for i in range(2)], 1)
                            f32, u8 = G.mci_frames_accel(ta, tb, tf, tacc, s, k_first=k0, count=T, normalised="both", masks=tm, **kw)
                            assert u8.dtype == torch.uint8 and tuple(u8.shape) == (T, 2, h, w, 3) and tuple(f32.shape) == (T, 2, 3, h, w)
                            assert torch.equal(u8.cpu(), torch.from_numpy(want)), (k0, kind, kw, masks is not None)
                            assert torch.equal(f32.cpu(), torch.from_numpy(bg.normalised_upload(want))), (k0, kind, kw)
                            if k0 + T - 1 == s:
                                assert torch.equal(u8[-1], tb)
                            if s == 8 and kind == "rough":      # the acceleration matters here, and each output alone is the same
                                assert masks is not None or not np.array_equal(want[:, 0], bg.mci_frames_host(a[0], b[0], f[0], s, ks, **kw))
                                assert torch.equal(G.mci_frames_accel(ta, tb, tf, tacc, s, k_first=k0, count=T, normalised=False, masks=tm, **kw), u8)
                                assert torch.equal(G.mci_frames_accel(ta, tb, tf, tacc, s, k_first=k0, count=T, normalised=True, masks=tm, **kw), f32)


@pytest.mark.parametrize("h,w", [(67, 93), (96, 128)])
def test_zero_acceleration_gives_the_existing_entries_bytes(h, w):
    G = handle()
    a, b, ma, mb = _segments(h, w)
    ta, tb, tma, tmb = dev(G, a, b, ma, mb)
    for precision in bg.PRECISIONS:
        (tf,) = dev(G, np.stack([cc.field("smooth", h, w, precision), cc.field("mixed", h, w, precision)]))
        zero = torch.zeros_like(tf)
        for border in bg.BORDERS:
            for sampler in bg.SAMPLERS:
                kw = dict(k_first=0, count=9, normalised="both", border=border, precision=precision, sampler=sampler)
                for x, y in zip(G.mci_frames_accel(ta, tb, tf, zero, 8, **kw), G.mci_frames(ta, tb, tf, 8, **kw)):
                    assert torch.equal(x, y), kw
                for x, y in zip(G.mci_frames_accel(ta, tb, tf, zero, 8, masks=(tma, tmb), **kw), G.mci_frames_masked(ta, tb, tma, tmb, tf, 8, **kw)):
                    assert torch.equal(x, y), kw


def test_refusals_launch_nothing():
    G = handle()
    L, H_ = G._lib, G._h
    h, w = 40, 56
    Hb, Wb = bg.field_shape(h, w)
    a, b = random_pair(h, w, 18)
    ma, mb = cc.masks("blobs", h, w)
    ta, tb, tma, tmb, tf, tacc = dev(G, a, b, ma, mb, cc.field("smooth", h, w), mc.accel_field("smooth", h, w))
    f32 = torch.full((2, 1, 3, h, w), 7.0, device=G.device)
    u8 = torch.full((2, 1, h, w, 3), 9, dtype=torch.uint8, device=G.device)
    out = torch.full((1, Hb, Wb, 2), 77, dtype=torch.int16, device=G.device)
    ws = torch.empty(L.rib_accel_workspace_bytes(H_, 1, Hb, Wb), dtype=torch.uint8, device=G.device)
    p = lambda t: t.data_ptr() if t is not None else None
    odd = lambda t: t.data_ptr() + 1

    def frames(T=2, B=1, H=h, W=w, a=p(ta), b=p(tb), ma=None, mb=None, fld=p(tf), acc=p(tacc), s=4, k=1, border=0, precision=0, sampler=0, of=p(f32), ou=p(u8)):
        return L.rib_accel_frames(H_, T, B, H, W, a, b, ma, mb, fld, acc, s, k, border, precision, sampler, of, ou, None)

    def field(B=1, Hb=Hb, Wb=Wb, prev=p(tf), cur=p(tf), nxt=p(tf), present=None, half=0, o=p(out), w=p(ws)):
        return L.rib_accel_field(H_, B, Hb, Wb, prev, cur, nxt, present, half, o, w, None)

    cases = [(dict(T=0), b"T=0"), (dict(H=0), b"H=0"), (dict(W=16385), b"W=16385"), (dict(B=0), b"B=0"),                  # sizes
             (dict(s=6), b"sample_rate=6"), (dict(s=2048), b"sample_rate=2048"), (dict(s=0), b"sample_rate=0"),               # power-of-two rate
             (dict(k=4), b"outside the segment"), (dict(k=-1), b"outside the segment"),                                        # frame range
             (dict(acc=None), b"acceleration field is null"), (dict(acc=odd(tacc)), b"misaligned acceleration field"),         # accel
             (dict(ma=p(tma)), b"exactly one mask"), (dict(mb=p(tmb)), b"exactly one mask"),                                   # masks given singly
             (dict(border=2), b"border=2"), (dict(precision=2), b"precision=2"), (dict(sampler=2), b"sampler=2"), (dict(sampler=-1), b"sampler=-1"),
             (dict(a=None), b"null pointer"), (dict(fld=None), b"null pointer"), (dict(fld=odd(tf)), b"misaligned pointer"),
             (dict(of=None, ou=None), b"both outputs are null")]
    for kw, text in cases:
        assert frames(**kw) == RIB_ERR_INVALID, kw
        assert L.rib_last_error(H_).startswith(b"rib_accel_frames") and text in L.rib_last_error(H_), (kw, L.rib_last_error(H_))
    for kw, text in [(dict(B=0), b"B=0"), (dict(Hb=0), b"Hb=0"), (dict(Wb=2049), b"Wb=2049"), (dict(half=2), b"half=2"), (dict(cur=None), b"null pointer"),
                     (dict(o=None), b"null pointer"), (dict(w=None), b"null pointer"), (dict(prev=odd(tf)), b"misaligned pointer"), (dict(w=odd(ws)), b"misaligned pointer")]:
        assert field(**kw) == RIB_ERR_INVALID, kw
        assert L.rib_last_error(H_).startswith(b"rib_accel_field") and text in L.rib_last_error(H_), (kw, L.rib_last_error(H_))
    assert L.rib_accel_workspace_bytes(H_, 0, Hb, Wb) == 0 and L.rib_accel_workspace_bytes(H_, 1, 2049, 1) == 0
    torch.cuda.synchronize()
    assert bool((f32 == 7.0).all()) and bool((u8 == 9).all()) and bool((out == 77).all())      # nothing was launched
    with pytest.raises(ValueError, match="accel must be an int16 tensor"):
        G.mci_frames_accel(ta, tb, tf, None, 4)
    with pytest.raises(ValueError, match="field must be an int16 tensor"):
        G.mci_frames_accel(ta, tb, tf, tacc.to(torch.int32), 4)
    with pytest.raises(ValueError, match="the field of 1 40x56 segments"):
        G.mci_frames_accel(ta, tb, tf, tacc[:-1], 4)
    with pytest.raises(ValueError, match="present must be 1 pairs"):
        G.mci_accel_field(tf, tf, tf, present=[(1, 1), (0, 0)])
    with pytest.raises(ValueError, match="precision must be"):
        G.mci_accel_field(tf, tf, tf, precision="quarter")
    assert frames() == 0 and frames(ma=p(tma), mb=p(tmb), sampler=1, of=None) == 0 and field() == 0      # and the good calls are accepted
    torch.cuda.synchronize()
    want = bg.mci_frames_accel_host(a, b, cc.field("smooth", h, w), mc.accel_field("smooth", h, w), 4, [1, 2], sampler="cubic", ma=ma, mb=mb)
    assert torch.equal(u8[:, 0].cpu(), torch.from_numpy(want))
    f = cc.field("smooth", h, w)
    assert torch.equal(out[0].cpu(), torch.from_numpy(bg.mci_accel_host(f, f, f)))


# ---- the folder driver -------------------------------------------------------------------------------------------------------------
def _tree(root):
    out = {}
    for d, _, files in os.walk(root):
        for n in files:
            out[os.path.relpath(os.path.join(d, n), root)] = open(os.path.join(d, n), "rb").read()
    return out


def _cfg64():
    return rib.AttrDict(gen=rib.hsm_gen_config(), model_height=64, model_width=64, gauss_sigma=5, skeleton_thres=0.001, foot_thres=0.001)


def _clips(root, key_hw=(64, 64)):
    """clipA: five key frames (four segments) of a scene that accelerates by (2, -2) px per segment; clipB: two key frames, one
    segment.  Rate 4."""
    from tests.composite_common import write_example
    for clip, n_key, seed in (("clipA", 5, 1), ("clipB", 2, 2)):
        write_example(root, n_key=n_key, rate=4, key_hw=key_hw, clip=clip, seed=seed)
        mc.accelerating_keys(root, n_key, key_hw, clip)
    return os.path.join(root, "inputs"), os.path.join(root, "Predict_motion")


SETTINGS = [dict(), dict(mci_person="exclude", mci_sampler="cubic", mci_border="valid"),
            dict(output_size="keyframes", mci_detail="keyframes", mci_precision="half", key_hw=(96, 128))]


@pytest.mark.parametrize("more", SETTINGS, ids=["plain", "exclude-cubic-valid", "keyframes-detail-half"])
def test_native_folder_driver_with_quadratic_motion(tmp_path, more):
    """64 x 64, one clip of four segments and one of one segment, batch 4: under mci_motion="quadratic" the native path's PNGs and
    _video.avi are the reference-protocol path's (the host definition) through the same Generator, byte for byte; the one-segment
    clip's files are mci_motion="linear"'s, the four-segment clip's are not."""
    more = dict(more)
    root = str(tmp_path)
    inputs, poses = _clips(root, more.pop("key_hw", (64, 64)))
    G = handle()
    kw = dict(background="mci", video=True, **more)
    run = lambda name, model=G, **extra: (ev.Evaluator(_cfg64(), batch=4, chunk=2, lanes=1) if model is G else ev.Evaluator(_cfg64())).evaluate_from_folder(
        model, inputs, None, poses, os.path.join(root, name), **dict(kw, **extra))
    nat = run("nat", mci_motion="quadratic")
    lin = run("lin", mci_motion="linear")
    before = G.plan_batch
    G.set_plan_batch(4)                         # the reference-protocol path follows the plans the native group follows
    try:
        ref = run("ref", model=Protocol(G), mci_motion="quadratic")
    finally:
        G.set_plan_batch(before)
    assert len(nat) == len(ref) == len(lin) == 17 + 5
    a, b, c = _tree(os.path.join(root, "nat")), _tree(os.path.join(root, "ref")), _tree(os.path.join(root, "lin"))
    assert sorted(a) == sorted(b) == sorted(c) and len(a) == 24 and "clipA_video.avi" in a
    for name in sorted(a):
        assert a[name] == b[name], name
    for name in sorted(a):
        if name.startswith("clipB"):
            assert a[name] == c[name], name
    if "mci_person" not in more:                # (write_example's random skeleton covers most of a 64 x 64 frame: little is left to move)
        assert a["clipA_video.avi"] != c["clipA_video.avi"]
        differing = [n for n in sorted(a) if a[n] != c[n] and n.endswith(".png")]
        assert len(differing) >= 4, differing       # a frame between the key frames of every segment, at the least


def test_the_files_do_not_depend_on_the_batch_and_the_default_is_linear(tmp_path):
    """mci_motion="quadratic" with batch 1 writes batch 4's files, byte for byte (a segment reads its neighbours' key frames itself);
    a run without the setting writes the files of mci_motion="linear".  Both runs follow batch 4's kernel plan: an Evaluator makes
    the generator follow the plan of its own batch, and the plans of batch 1 and batch 4 may differ in the last uint8 step under
    any background (tests/test_gpu_parity.py) - here the one-segment clip's linear frames do - so the grouping is what is compared."""
    import contextlib
    root = str(tmp_path)
    inputs, poses = _clips(root)
    G = handle()

    @contextlib.contextmanager
    def plan_of_four(model, native):
        before = model.plan_batch
        model.set_plan_batch(4)
        try:
            yield
        finally:
            model.set_plan_batch(before)

    def run(name, batch, **extra):
        E = ev.Evaluator(_cfg64(), batch=batch, chunk=2, lanes=1)
        E._plan_policy = plan_of_four
        return E.evaluate_from_folder(G, inputs, None, poses, os.path.join(root, name), background="mci", **extra)
    four, one = run("four", 4, mci_motion="quadratic"), run("one", 1, mci_motion="quadratic")
    plain, lin = run("plain", 4), run("lin", 4, mci_motion="linear")
    assert len(four) == len(one) == len(plain) == len(lin) == 22
    a, b, c, d = (_tree(os.path.join(root, n)) for n in ("four", "one", "plain", "lin"))
    assert a == b and len(a) == 22
    assert c == d and c != a
    with pytest.raises(ValueError, match="needs mci_detail='keyframes' for now"):
        run("no", 4, mci_motion="quadratic", output_size="keyframes")
    with pytest.raises(ValueError, match="mci_motion must be"):
        run("no", 4, mci_motion="cubic")
    assert not os.path.exists(os.path.join(root, "no"))             # refused before any file is written
