"""rib_cubic_frames / rib_cubic_scaled (csrc/mci.hip.h: k_cubic_frames<VALID, HALF, MASKED>, k_cubic_scaled<VALID, HALF>;
Generator.mci_frames / mci_frames_masked / mci_frames_scaled with sampler="cubic") - the interpolated backgrounds with the 4x4 cubic
sampler - against the integer definition (background.sample_cubic and the sampler="cubic" host functions), bit for bit; every result
once with staging = 0 (the per-tile rule) and once with staging = 1 (never stage): the bytes never depend on it.  The inputs are
tests/mci_cubic_common.py's; tests/test_mci_cubic_cpu.py proves with background.cubic_tile_staged that they take both paths (smooth
fields staged, full-reach random fields direct, the mixed ones both within one launch).  The shapes are the smallest at which the
kernels can go wrong: every tap clamped (1x1, 2x3, 5x7), partial blocks with W % 4 != 0 and unaligned rows (67x93), whole tiles
(64x96), more than 256 pixels and more than 16 tiles per row (8x1040), and one row wide enough for more than 64 KB of LDS."""
import os

import numpy as np
import pytest
import torch

import render_in_between_amd as rib
from render_in_between_amd import background as bg, evaluator as ev
from tests import mci_cubic_common as cc
from tests.mci_gpu_common import dev
from tests.test_background_cpu import random_pair
from tests.test_gpu_mci import Protocol, handle

pytestmark = pytest.mark.gpu

RIB_ERR_INVALID = -1                                                    # include/rib.h
VARIANTS = [(b, p) for b in bg.BORDERS for p in bg.PRECISIONS]


def both_stagings(call):
    """call(_staging) for 0 and 1: the two results are equal; -> the first."""
    one, two = call(0), call(1)
    for x, y in zip(one if isinstance(one, tuple) else (one,), two if isinstance(two, tuple) else (two,)):
        assert torch.equal(x, y)
    return one


@pytest.mark.parametrize("h,w", cc.SIZES)
def test_frames_against_the_definition(h, w):
    """Every field kind, both borders, both precisions: frames k = 0..8 of s = 8 (the two key frames among them) in one launch,
    both outputs."""
    G = handle()
    a, b = random_pair(h, w, 11)
    ta, tb = dev(G, a, b)
    s, ks = 8, range(9)
    for kind in cc.KINDS:
        for border, precision in VARIANTS:
            want = cc.want_frames(kind, h, w, s, ks, border, precision)
            (tf,) = dev(G, cc.field(kind, h, w, precision))
            f32, u8 = both_stagings(lambda st: G.mci_frames(ta, tb, tf, s, k_first=0, count=9, normalised="both", border=border, precision=precision,
                                                            sampler="cubic", _staging=st))
            assert u8.dtype == torch.uint8 and tuple(u8.shape) == (9, h, w, 3) and f32.dtype == torch.float32 and tuple(f32.shape) == (9, 3, h, w)
            assert torch.equal(u8.cpu(), torch.from_numpy(want)), (kind, border, precision)
            assert torch.equal(f32.cpu(), torch.from_numpy(bg.normalised_upload(want))), (kind, border, precision)
            assert torch.equal(u8[0], ta) and torch.equal(u8[8], tb)
    if (h, w) in cc.WIDE:                   # the sampler matters here: the bilinear entry writes other bytes
        (tf,) = dev(G, cc.field("smooth", h, w))
        assert not torch.equal(G.mci_frames(ta, tb, tf, s, k_first=1, count=1, normalised=False),
                               G.mci_frames(ta, tb, tf, s, k_first=1, count=1, normalised=False, sampler="cubic"))


@pytest.mark.parametrize("h,w", cc.SIZES)
def test_masked_frames_against_the_definition(h, w):
    """Random blobs and an all-set mask, the person excluded: a sample is clean iff its 16 taps are clear."""
    G = handle()
    a, b = random_pair(h, w, 11)
    ta, tb = dev(G, a, b)
    s, ks = 8, range(9)
    for mk in ("blobs", "one"):
        tma, tmb = dev(G, *cc.masks(mk, h, w))
        for kind in (("smooth", "random", "mixed") if mk == "blobs" else ("mixed",)):
            for border, precision in VARIANTS:
                want = cc.want_frames(kind, h, w, s, ks, border, precision, masked=mk)
                (tf,) = dev(G, cc.field(kind, h, w, precision))
                f32, u8 = both_stagings(lambda st: G.mci_frames_masked(ta, tb, tma, tmb, tf, s, k_first=0, count=9, normalised="both", border=border,
                                                                       precision=precision, sampler="cubic", _staging=st))
                assert torch.equal(u8.cpu(), torch.from_numpy(want)), (mk, kind, border, precision)
                assert torch.equal(f32.cpu(), torch.from_numpy(bg.normalised_upload(want)))
                if mk == "blobs" and (h, w) in cc.WIDE:
                    assert not np.array_equal(want, cc.want_frames(kind, h, w, s, ks, border, precision))       # the masks matter


@pytest.mark.parametrize("s,firsts", [(1, [0]), (2, [0]), (8, [0, 6]), (1024, [0, 511, 1022])])
def test_sample_rates_and_frame_ranges(s, firsts):
    """s in {1, 2, 8, 1024}, three frames (two at s = 1) from k_first: 0 and s are among them; 67 x 93, the mixed field at full
    reach in half pixels: k * D reaches 1024 * 159 * 256."""
    G = handle()
    h, w = 67, 93
    a, b = random_pair(h, w, 12)
    f = cc.field("mixed", h, w, "half")
    ta, tb, tf = dev(G, a, b, f)
    for k0 in firsts:
        T = min(3, s + 1 - k0)
        for border in bg.BORDERS:
            want = bg.mci_frames_host(a, b, f, s, range(k0, k0 + T), border=border, precision="half", sampler="cubic")
            got = both_stagings(lambda st: G.mci_frames(ta, tb, tf, s, k_first=k0, count=T, normalised=False, border=border, precision="half",
                                                        sampler="cubic", _staging=st))
            assert torch.equal(got.cpu(), torch.from_numpy(want)), (s, k0, border)


def test_a_batch_of_two_and_each_output_alone():
    """B = 2, T = 3 (T * B = 6): two segments with different key frames, fields and masks in one launch; float only, uint8 only
    and both outputs give the same frames, and a frame does not depend on T or B."""
    G = handle()
    h, w, s = 67, 93, 4
    pairs = [random_pair(h, w, 13), random_pair(h, w, 14)]
    a, b = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    f = np.stack([cc.field("smooth", h, w), cc.field("mixed", h, w)])
    ma, mb = (np.stack([cc.masks("blobs", h, w)[i], cc.masks("blobs", h, w)[1 - i]]) for i in (0, 1))
    ta, tb, tf, tma, tmb = dev(G, a, b, f, ma, mb)
    want = np.stack([bg.mci_frames_host(a[i], b[i], f[i], s, [1, 2, 3], border="valid", sampler="cubic") for i in range(2)], 1)
    wantm = np.stack([bg.mci_frames_masked_host(a[i], b[i], ma[i], mb[i], f[i], s, [1, 2, 3], border="valid", sampler="cubic") for i in range(2)], 1)
    for st in (0, 1):
        kw = dict(k_first=1, count=3, border="valid", sampler="cubic", _staging=st)
        f32, u8 = G.mci_frames(ta, tb, tf, s, normalised="both", **kw)
        assert tuple(u8.shape) == (3, 2, h, w, 3) and torch.equal(u8.cpu(), torch.from_numpy(want))
        assert torch.equal(G.mci_frames(ta, tb, tf, s, normalised=False, **kw), u8) and torch.equal(G.mci_frames(ta, tb, tf, s, normalised=True, **kw), f32)
        assert torch.equal(f32.cpu(), torch.from_numpy(bg.normalised_upload(want)))
        m32, m8 = G.mci_frames_masked(ta, tb, tma, tmb, tf, s, normalised="both", **kw)
        assert torch.equal(m8.cpu(), torch.from_numpy(wantm)) and torch.equal(m32.cpu(), torch.from_numpy(bg.normalised_upload(wantm)))
        assert torch.equal(G.mci_frames_masked(ta, tb, tma, tmb, tf, s, normalised=False, **kw), m8)
        alone = G.mci_frames(ta[1], tb[1], tf[1], s, k_first=2, count=1, normalised=False, border="valid", sampler="cubic", _staging=st)
        assert torch.equal(alone[0], u8[1, 1])


def test_a_row_wider_than_64_kb_of_lds():
    """One row of 16384 pixels: the output row (49 KB), the weight table and the windows (and, scaled, the field row) ask for up to 97 KB
    of LDS, which the entry raises the kernel's limit for.  The scaled entry at equal sizes writes the unscaled entry's bytes."""
    G = handle()
    h, w, s = 1, 16384, 4
    a, b = random_pair(h, w, 15)
    f = cc.field("mixed", h, w)
    ta, tb, tf = dev(G, a, b, f)
    want = bg.mci_frames_host(a, b, f, s, [1, 2], border="valid", sampler="cubic")
    got = both_stagings(lambda st: G.mci_frames(ta, tb, tf, s, k_first=1, count=2, normalised=False, border="valid", sampler="cubic", _staging=st))
    assert torch.equal(got.cpu(), torch.from_numpy(want))
    sc = both_stagings(lambda st: G.mci_frames_scaled(ta, tb, tf, (h, w), s, k_first=1, count=2, border="valid", sampler="cubic", _staging=st))
    assert torch.equal(sc, got)


# model (H, W) -> key frames (h0, w0): equal sizes (the unscaled entry's bytes), enlargement with odd sides, reduction, the ratio bound.
# The blended field row always fits the LDS beside the rest (the entry raises the kernel's limit), so rib_scaled_frames' stage = 0
# path has no analogue here and needs no case.
PAIRS = [((32, 32), (32, 32)), ((32, 40), (75, 133)), ((64, 64), (20, 24)), ((4, 4), (64, 64))]


@pytest.mark.parametrize("model,size", PAIRS)
def test_scaled_against_the_definition(model, size):
    G = handle()
    B, s, k_first, T = 2, 8, 3, 3
    a0 = np.stack([random_pair(*size, 16)[0], random_pair(*size, 17)[0]])
    b0 = np.stack([random_pair(*size, 16)[1], random_pair(*size, 17)[1]])
    ta, tb = dev(G, a0, b0)
    for border, precision in VARIANTS:
        for kinds in (("random", "smooth"), ("mixed", "zero")):
            f = np.stack([cc.field(k, *model, precision) for k in kinds])
            want = np.stack([bg.mci_frames_scaled_host(a0[i], b0[i], f[i], model, s, range(k_first, k_first + T), border=border, precision=precision,
                                                       sampler="cubic") for i in range(B)], 1)
            (tf,) = dev(G, f)
            got = both_stagings(lambda st: G.mci_frames_scaled(ta, tb, tf, model, s, k_first=k_first, count=T, border=border, precision=precision,
                                                               sampler="cubic", _staging=st))
            assert got.dtype == torch.uint8 and tuple(got.shape) == (T, B) + size + (3,)
            assert torch.equal(got.cpu(), torch.from_numpy(want)), (border, precision, kinds)
            if model == size:
                same = G.mci_frames(ta, tb, tf, s, k_first=k_first, count=T, normalised=False, border=border, precision=precision, sampler="cubic")
                assert torch.equal(got, same)
    ends = G.mci_frames_scaled(ta, tb, tf, model, s, k_first=0, count=9, sampler="cubic")
    assert torch.equal(ends[0], ta) and torch.equal(ends[8], tb)


def test_refusals_launch_nothing():
    G = handle()
    L, H_ = G._lib, G._h
    h, w = 40, 56
    a, b = random_pair(h, w, 18)
    ma, mb = cc.masks("blobs", h, w)
    ta, tb, tma, tmb, tf = dev(G, a, b, ma, mb, cc.field("smooth", h, w))
    f32 = torch.full((2, 1, 3, h, w), 7.0, device=G.device)
    u8 = torch.full((2, 1, h, w, 3), 9, dtype=torch.uint8, device=G.device)
    big = torch.full((2, 1, 80, 112, 3), 9, dtype=torch.uint8, device=G.device)
    p = lambda t: t.data_ptr() if t is not None else None

    def frames(T=2, B=1, H=h, W=w, a=ta, b=tb, ma=None, mb=None, fld=tf, s=4, k=1, border=0, precision=0, staging=0, of=f32, ou=u8):
        return L.rib_cubic_frames(H_, T, B, H, W, p(a), p(b), p(ma), p(mb), p(fld), s, k, border, precision, staging, p(of), p(ou), None)

    def scaled(T=2, B=1, H=h, W=w, H0=80, W0=112, a=ta, b=tb, fld=tf, s=4, k=1, border=0, precision=0, staging=0, o=big):
        return L.rib_cubic_scaled(H_, T, B, H, W, H0, W0, p(a), p(b), p(fld), s, k, border, precision, staging, p(o), None)

    shared = [(dict(s=6), b"sample_rate=6"), (dict(s=2048), b"sample_rate=2048"), (dict(k=4), b"outside the segment"), (dict(k=-1), b"outside the segment"),
              (dict(staging=2), b"staging=2"), (dict(staging=-1), b"staging=-1"), (dict(border=2), b"border=2"), (dict(precision=2), b"precision=2"),
              (dict(T=0), b"T=0"), (dict(H=0), b"H=0"), (dict(W=16385), b"W=16385"), (dict(a=None), b"null pointer"), (dict(fld=None), b"null pointer")]
    for kw, text in shared + [(dict(ma=tma), b"exactly one mask"), (dict(mb=tmb), b"exactly one mask"), (dict(of=None, ou=None), b"both outputs are null")]:
        assert frames(**kw) == RIB_ERR_INVALID, kw
        assert L.rib_last_error(H_).startswith(b"rib_cubic_frames") and text in L.rib_last_error(H_), (kw, L.rib_last_error(H_))
    for kw, text in shared + [(dict(o=None), b"null pointer"), (dict(W0=16 * w + 1), b"within 1/16"), (dict(H0=2), b"within 1/16"), (dict(H0=0), b"H0=0")]:
        assert scaled(**kw) == RIB_ERR_INVALID, kw
        assert L.rib_last_error(H_).startswith(b"rib_cubic_scaled") and text in L.rib_last_error(H_), (kw, L.rib_last_error(H_))
    torch.cuda.synchronize()
    assert bool((f32 == 7.0).all()) and bool((u8 == 9).all()) and bool((big == 9).all())      # nothing was launched
    for bad in ("bicubic", None):
        with pytest.raises(ValueError, match="sampler must be"):
            G.mci_frames(ta, tb, tf, 4, sampler=bad)
        with pytest.raises(ValueError, match="sampler must be"):
            G.mci_frames_scaled(ta, tb, tf, (h, w), 4, sampler=bad)
    assert frames() == 0 and frames(ma=tma, mb=tmb, of=None) == 0 and scaled() == 0             # and the good calls are accepted
    torch.cuda.synchronize()
    assert torch.equal(u8[:, 0].cpu(), torch.from_numpy(bg.mci_frames_masked_host(a, b, ma, mb, cc.field("smooth", h, w), 4, [1, 2], sampler="cubic")))


# ---- the folder driver -------------------------------------------------------------------------------------------------------------
def _tree(root):
    out = {}
    for d, _, files in os.walk(root):
        for n in files:
            out[os.path.relpath(os.path.join(d, n), root)] = open(os.path.join(d, n), "rb").read()
    return out


def _cfg64():
    return rib.AttrDict(gen=rib.hsm_gen_config(), model_height=64, model_width=64, gauss_sigma=5, skeleton_thres=0.001, foot_thres=0.001)


def _clips(root, key_hw=None):
    """Two clips of three key frames at rate 4 whose scenes move by an odd number of pixels per key frame: the frames in between
    sit at fractional offsets."""
    from tests.composite_common import write_example
    from tests.test_keyframes_size_cpu import moving_keys
    hw = key_hw or (64, 64)
    for clip, seed, step in (("clipA", 1, (6, -2)), ("clipB", 2, (-2, 6))):
        write_example(root, n_key=3, rate=4, key_hw=hw, clip=clip, seed=seed)
        moving_keys(root, 3, hw, clip=clip, step=step)
    return os.path.join(root, "inputs"), os.path.join(root, "Predict_motion")


@pytest.mark.parametrize("more", [dict(), dict(mci_person="exclude"), dict(output_size="keyframes", key_hw=(96, 128))], ids=["plain", "exclude", "keyframes"])
def test_native_folder_driver_with_the_cubic_sampler(tmp_path, more):
    """64 x 64, two clips of three key frames, batch 2, mci_sampler="cubic": the native path's PNGs and _video.avi are the
    reference-protocol path's (the host definition) through the same Generator, byte for byte, and not the default sampler's."""
    more = dict(more)
    root = str(tmp_path)
    inputs, poses = _clips(root, more.pop("key_hw", None))
    G = handle()
    kw = dict(background="mci", video=True, **more)
    run = lambda name, model=G, **extra: (ev.Evaluator(_cfg64(), batch=2, chunk=2, lanes=1) if model is G else ev.Evaluator(_cfg64())).evaluate_from_folder(
        model, inputs, None, poses, os.path.join(root, name), **dict(kw, **extra))
    nat = run("nat", mci_sampler="cubic")
    plain = run("plain")
    before = G.plan_batch
    G.set_plan_batch(2)                         # the reference-protocol path follows the plans the native group follows
    try:
        ref = run("ref", model=Protocol(G), mci_sampler="cubic")
    finally:
        G.set_plan_batch(before)
    assert len(nat) == len(ref) == len(plain) == 18
    a, b, c = _tree(os.path.join(root, "nat")), _tree(os.path.join(root, "ref")), _tree(os.path.join(root, "plain"))
    assert sorted(a) == sorted(b) == sorted(c) and len(a) == 20 and "clipA_video.avi" in a
    for name in sorted(a):
        assert a[name] == b[name], name
    assert a["clipA_video.avi"] != c["clipA_video.avi"] and a["clipB_video.avi"] != c["clipB_video.avi"]
    differing = [n for n in sorted(a) if a[n] != c[n]]
    assert len([n for n in differing if n.endswith(".png")]) >= 4      # a frame between the key frames of every segment, at the least
