"""background.py's "motion" paragraph on the host: mci_accel_host / mci_frames_accel_host (mci_motion="quadratic"), the second-order
trajectory across key frames.  What the definition guarantees is asserted exactly - a zero acceleration field gives the linear
bytes; a texture at constant velocity has zero acceleration; a texture at constant acceleration gets the TRUE middle frame where the
linear definition is a pixel off - and what it only improves is measured against true frames at quarter-pixel positions."""
import inspect
import os
import re

import numpy as np
import pytest

from render_in_between_amd import background as bg
from tests import mci_cubic_common as cc, mci_motion_common as mc
from tests.test_background_cpu import random_pair

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDS = [0, 1, 2, 3, 4]


# ---- 1. zero acceleration: the linear bytes ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", [(67, 93), (96, 128)])
def test_zero_acceleration_gives_the_linear_bytes(h, w):
    a, b = random_pair(h, w, 21)
    ma, mb = cc.masks("blobs", h, w)
    for precision in bg.PRECISIONS:
        f = cc.field("mixed", h, w, precision)
        zero = np.zeros_like(f)
        for border in bg.BORDERS:
            for sampler in bg.SAMPLERS:
                for s in (1, 2, 8):
                    kw = dict(border=border, precision=precision, sampler=sampler)
                    ks = range(s + 1)
                    assert np.array_equal(bg.mci_frames_accel_host(a, b, f, zero, s, ks, **kw), bg.mci_frames_host(a, b, f, s, ks, **kw)), (kw, s)
                    assert np.array_equal(bg.mci_frames_accel_host(a, b, f, zero, s, ks, ma=ma, mb=mb, **kw),
                                          bg.mci_frames_masked_host(a, b, ma, mb, f, s, ks, **kw)), (kw, s)


def test_the_correction_in_integers():
    """c = (UNIT k (s - k) Acc + 2 s^2) >> (2 log2 s + 2) against exact rationals, at s = 1024 where the product passes 2^32; it
    vanishes at the key frames, is a / 8 in the middle and rounds to nearest (floor of + 1/2)."""
    from fractions import Fraction
    from math import floor
    acc = np.zeros((1, 1, 2), np.int16)
    for a in (-bg.ACCEL_MAX, -8, -1, 1, 3, 8, 4097, bg.ACCEL_MAX):
        acc[...] = (a, -a)
        for precision, unit in (("full", 2), ("half", 1)):
            for s in (1, 2, 8, 1024):
                for k in sorted({0, 1, s // 2, s - 1, s}):
                    cx, cy = bg.accel_correction(acc, s, k, 8, 8, precision)
                    want = lambda v: floor(Fraction(unit * k * (s - k) * v * 256, 4 * s * s) + Fraction(1, 2))
                    assert (cx == want(a)).all() and (cy == want(-a)).all(), (a, precision, s, k)
                    if k in (0, s):
                        assert not cx.any() and not cy.any()
    acc[...] = (8, 0)
    assert (bg.accel_correction(acc, 2, 1, 8, 8)[0] == 256).all()          # a = 8 px per segment^2: 1 px in the middle
    assert bg.ACCEL_MAX == 5104 < 2 ** 15


def test_accel_host_rules_on_small_fields():
    """The three lookups, block by block, against a per-block loop; None neighbours; the half-pel shift is a floor."""
    rng = np.random.default_rng(5)
    for Hb, Wb, shift, reach in ((9, 12, 0, 79), (9, 12, 1, 159), (1, 1, 0, 79), (3, 2, 1, 159)):
        fp, f, fn = mc.random_fields(1, Hb, Wb, reach, 3)[:, 0]
        for prev, nxt in ((fp, fn), (None, fn), (fp, None), (None, None)):
            raw = np.zeros((Hb, Wb, 2), np.int64)
            for by in range(Hb):
                for bx in range(Wb):
                    wx, wy = int(f[by, bx, 0]) >> shift, int(f[by, bx, 1]) >> shift
                    p = None if prev is None else prev[min(max((8 * by + 4 - 2 * wy) >> 3, 0), Hb - 1), min(max((8 * bx + 4 - 2 * wx) >> 3, 0), Wb - 1)].astype(int)
                    n = None if nxt is None else nxt[min(max((8 * by + 4 + 2 * wy) >> 3, 0), Hb - 1), min(max((8 * bx + 4 + 2 * wx) >> 3, 0), Wb - 1)].astype(int)
                    me = f[by, bx].astype(int)
                    raw[by, bx] = n - p if (p is not None and n is not None) else 2 * (n - me) if n is not None else 2 * (me - p) if p is not None else 0
            want = np.stack([bg.median3(raw[..., 0]), bg.median3(raw[..., 1])], -1)
            got = bg.mci_accel_host(prev, f, nxt, unit_shift=shift)
            assert got.dtype == np.int16 and np.array_equal(got, want), (Hb, Wb, shift)
            assert np.abs(got.astype(int)).max() <= 4 * reach
    f = np.zeros((2, 2, 2), np.int16)
    for bad in (dict(f=f.astype(np.int32)), dict(f_prev=f[:1]), dict(f_next=f.astype(np.int8)), dict(unit_shift=2), dict(f=f + 1277)):
        with pytest.raises(ValueError, match="mci_accel_host"):
            bg.mci_accel_host(**dict(dict(f_prev=None, f=f, f_next=None), **bad))
    with pytest.raises(ValueError, match="acceleration field is int16"):
        bg.mci_frames_accel_host(np.zeros((8, 8, 3), np.uint8), np.zeros((8, 8, 3), np.uint8), f[:1, :1], f[:1, :1].astype(np.int32), 2, [1])
    with pytest.raises(ValueError, match="masks are given together"):
        bg.mci_frames_accel_host(np.zeros((8, 8, 3), np.uint8), np.zeros((8, 8, 3), np.uint8), f[:1, :1], f[:1, :1], 2, [1], ma=np.zeros((8, 8), np.uint8))


# ---- 2. constant velocity: zero acceleration -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [(8, 0), (-4, 8), (8, -8)])
def test_constant_velocity_has_no_acceleration(d):
    """Four key frames of a texture that moves by the same 2 d per segment (d a multiple of 4, L = 3, 160 x 192): the acceleration
    is exactly zero on every interior block, for the middle segment and for the one-sided ends, and the frames are the linear ones."""
    step = (2 * d[0], 2 * d[1])
    for seed in SEEDS[:2]:
        keys, _, _ = mc.moving_keys(seed, [step] * 3)
        f = [bg.mci_field_host(keys[j], keys[j + 1]) for j in range(3)]
        for prev, cur, nxt, dp, dn in ((0, 1, 2, d, d), (None, 0, 1, None, d), (1, 2, None, d, None)):
            acc = bg.mci_accel_host(None if prev is None else f[prev], f[cur], None if nxt is None else f[nxt])
            g = mc.accel_blocks(dp, d, dn)
            assert g.sum() >= 4 and not acc[g].any(), (seed, d, prev, nxt)
            px = mc.exact_pixels(dp, d, dn)
            lin = bg.mci_frames_host(keys[cur], keys[cur + 1], f[cur], 4, [1, 2, 3])
            qua = bg.mci_frames_accel_host(keys[cur], keys[cur + 1], f[cur], acc, 4, [1, 2, 3])
            assert px.sum() >= 256 and np.array_equal(qua[:, px], lin[:, px])


# ---- 3. constant acceleration: the guarantee ---------------------------------------------------------------------------------------------
# Per-segment motion 8, 16, 24 px: d = 4, 8, 12, a = 8 px per segment^2 (and the same on a diagonal).  The positions of the four key
# frames are 0, 8, 24, 48 = 4 j + 4 j^2: x(t) = x_j + u t + 4 t^2 inside segment j with u = 2 d - 4, so the middle frame (t = 1/2)
# of a segment with vector d shows the scene at x_j + d - 1 where the linear definition shows x_j + d: one pixel off, everywhere.
# Measured (this test prints it): the linear middle frame differs from the truth on 99.9 .. 100.0 % of the interior pixels, in the
# horizontal and in the diagonal case, for every seed, segment and border; the quadratic one on none.
CASES = [[(8, 0), (16, 0), (24, 0)], [(8, -8), (16, -16), (24, -24)]]


@pytest.mark.parametrize("steps", CASES, ids=["horizontal", "diagonal"])
def test_constant_acceleration_is_exact(steps):
    """mci_accel_host is the scene's a on every interior block (both neighbours, and the one-sided rule at either end); the middle frame
    at s = 2 is the TRUE scene on every interior pixel, also under border="valid", and the linear definition is wrong on most of them
    (measured: on 99.9 .. 100.0 % of them in every case)."""
    ds = [(sx // 2, sy // 2) for sx, sy in steps]
    a = (steps[1][0] - steps[0][0], steps[1][1] - steps[0][1])
    for seed in SEEDS:
        keys, crop, pos = mc.moving_keys(seed, steps)
        for border in bg.BORDERS:
            f = [bg.mci_field_host(keys[j], keys[j + 1], border=border) for j in range(3)]
            # (previous, own, next) segment: the middle one with both neighbours, the first and the last with the one-sided rule
            for prev, cur, nxt in ((0, 1, 2), (None, 0, 1), (1, 2, None)):
                dp, d, dn = (None if prev is None else ds[prev]), ds[cur], (None if nxt is None else ds[nxt])
                acc = bg.mci_accel_host(None if prev is None else f[prev], f[cur], None if nxt is None else f[nxt])
                g = mc.accel_blocks(dp, d, dn)
                assert g.sum() >= 4, (steps, cur)
                assert (acc[g] == a).all(), (seed, border, cur, acc[g].tolist())
                if border == "valid" and cur != 1:
                    continue                # (the issue's valid case is the middle frame of the middle segment)
                # s = 2, k = 1: c = a / 8 = 1 px exactly; the truth is the scene at x_cur + d - a / 8
                truth = crop(int(pos[cur][0]) + d[0] - a[0] // 8, int(pos[cur][1]) + d[1] - a[1] // 8)
                px = mc.exact_pixels(dp, d, dn)
                qua = bg.mci_frames_accel_host(keys[cur], keys[cur + 1], f[cur], acc, 2, [1], border=border)[0]
                lin = bg.mci_frames_host(keys[cur], keys[cur + 1], f[cur], 2, [1], border=border)[0]
                wrong = (lin[px] != truth[px]).any(-1).mean()
                print("steps=%s seed=%d border=%s segment=%d: %d interior pixels, linear wrong on %.1f %%" % (steps, seed, border, cur, px.sum(), 100 * wrong))
                assert px.sum() >= 256 and np.array_equal(qua[px], truth[px]), (seed, border, cur)
                assert wrong > 0.5, (seed, border, cur, wrong)


# ---- 4. fractional corrections: true frames at quarter-pixel positions -------------------------------------------------------------------
# s = 4, k = 1, 3: c = 3 a / 32 px is fractional.  tests/mci_motion_common.quarter_scene: 160 x 192 frames box-downsampled 4x from one
# texture moving on a parabola, the TRUE uniform fields d = steps / 2 of the three segments (so that the trajectory is what is measured,
# not the block matcher), interior with a 32 px inset.  Measured with the committed definition (this test prints every figure):
# linear 19.6 .. 25.0 dB with either sampler, quadratic 36.9 .. 40.7 dB (bilinear) and 41.6 .. 44.7 dB (cubic); the gain of the 24 cases
# per sampler lies in 14.6 .. 18.4 dB (bilinear) and 19.4 .. 22.4 dB (cubic).  The assertion is only "greater than linear in every case".
QSTEPS = [[(8, 0), (16, 0), (24, 0)], [(8, -8), (16, -16), (24, -24)], [(24, 0), (16, 0), (8, 0)], [(0, 0), (0, 16), (0, 32)]]


def test_quarter_pixel_truth_quadratic_beats_linear():
    """s = 4, k = 1 and 3 against true frames at quarter-pixel positions: quadratic beats linear in PSNR in every case (measured
    gain: 14.6 .. 18.4 dB with the bilinear sampler, 19.4 .. 22.4 dB with the cubic one)."""
    gains = {s: [] for s in bg.SAMPLERS}
    for steps in QSTEPS:
        for seed in range(3):
            keys, mids = mc.quarter_scene(seed, steps)
            shape = bg.field_shape(mc.H, mc.W) + (2,)
            f = [np.broadcast_to(np.asarray((sx // 2, sy // 2), np.int16), shape).copy() for sx, sy in steps]
            acc = bg.mci_accel_host(f[0], f[1], f[2])
            assert (acc == (steps[2][0] - steps[1][0], steps[2][1] - steps[1][1])).all()
            assert np.array_equal(mids[0], keys[1]) and np.array_equal(mids[4], keys[2])
            for sampler in bg.SAMPLERS:
                lin = bg.mci_frames_host(keys[1], keys[2], f[1], 4, [1, 3], sampler=sampler)
                qua = bg.mci_frames_accel_host(keys[1], keys[2], f[1], acc, 4, [1, 3], sampler=sampler)
                for j, k in enumerate((1, 3)):
                    pl, pq = mc.psnr(lin[j], mids[k]), mc.psnr(qua[j], mids[k])
                    print("steps=%s seed=%d %s k=%d  PSNR linear %.2f quadratic %.2f gain %.2f dB" % (steps, seed, sampler, k, pl, pq, pq - pl))
                    gains[sampler].append(pq - pl)
                    assert pq > pl, (steps, seed, sampler, k, pl, pq)
    for s, g in gains.items():
        print("%s: gain %.2f .. %.2f dB over %d cases" % (s, min(g), max(g), len(g)))
        assert len(g) == 24


@pytest.mark.parametrize("h,w", [(67, 93), (96, 128)])
def test_the_gpu_inputs_leave_the_frame_and_take_both_tile_paths(h, w):
    """tests/test_gpu_mci_motion.py's acceleration fields: with the rough one the corrected samples leave the frame on all four sides
    and the cubic tiles gather; with the smooth one (on the smooth block field) the tiles stay staged."""
    s, k = 8, 4
    for kind, f in (("rough", cc.field("mixed", h, w)), ("smooth", cc.field("smooth", h, w))):
        pay, pax, pby, pbx = bg.sample_positions(f, s, k, h, w)
        cx, cy = bg.accel_correction(mc.accel_field(kind, h, w, 1), s, k, h, w)
        pay, pax, pby, pbx = pay + cy, pax + cx, pby + cy, pbx + cx
        share = bg.cubic_tile_staged(pay, pax, pby, pbx).mean()
        if kind == "rough":
            assert pay.min() < 0 and pax.min() < 0 and pay.max() > (h - 1) << 8 and pax.max() > (w - 1) << 8
            assert np.abs(cx).max() > 32 << 8 and share <= 0.1, share
        else:
            assert cx.any() and cy.any() and share >= 0.9, share


# ---- 5. settings -----------------------------------------------------------------------------------------------------------------------------
def test_check_motion():
    assert bg.MOTIONS == ("linear", "quadratic")
    assert bg.check_motion("dain") == "linear" and bg.check_motion("mci") == "linear" and bg.check_motion("mci", "quadratic") == "quadratic"
    for bad in ("cubic", None, 2, b"linear"):
        with pytest.raises(ValueError, match="mci_motion must be 'linear' or 'quadratic'"):
            bg.check_motion("mci", bad)
    with pytest.raises(ValueError, match="my_caller: mci_motion is a setting of background='mci'"):
        bg.check_motion("dain", "quadratic", who="my_caller")
    assert list(inspect.signature(bg.check_motion).parameters)[:3] == ["background", "mci_motion", "who"]
    with pytest.raises(ValueError, match="needs mci_detail='keyframes' for now .* rib_scaled_frames / rib_cubic_scaled is the follow-up"):
        bg.check_motion("mci", "quadratic", output_size="keyframes")
    assert bg.check_motion("mci", "quadratic", output_size="keyframes", mci_detail="keyframes") == "quadratic"
    assert bg.check_motion("mci", "linear", output_size="keyframes") == "linear"
    assert list(inspect.signature(bg.check_settings).parameters)[-1] == "mci_sampler"      # (pinned: the new setting has a check of its own)


def test_the_driver_refuses_before_any_file(tmp_path):
    import render_in_between_amd as rib
    from render_in_between_amd import evaluator as ev, inference
    cfg = rib.AttrDict(gen=rib.hsm_gen_config(), model_height=64, model_width=64, gauss_sigma=5, skeleton_thres=0.001, foot_thres=0.001)
    out = os.path.join(str(tmp_path), "out")
    call = lambda dain, **kw: ev.Evaluator(cfg).evaluate_from_folder(lambda *a: None, str(tmp_path), dain, str(tmp_path), out, **kw)
    with pytest.raises(ValueError, match="mci_motion must be"):
        call(None, background="mci", mci_motion="cubic")
    with pytest.raises(ValueError, match="mci_motion is a setting of background='mci'"):
        call(str(tmp_path), mci_motion="quadratic")
    with pytest.raises(ValueError, match="mci_motion='quadratic' with output_size='keyframes' needs mci_detail='keyframes'"):
        call(None, background="mci", mci_motion="quadratic", output_size="keyframes")
    with pytest.raises(ValueError, match="mci_person='exclude' with mci_precision='half'"):      # the existing refusals stay
        call(None, background="mci", mci_motion="quadratic", mci_person="exclude", mci_precision="half")
    assert not os.path.exists(out)
    assert inspect.signature(ev.Evaluator.evaluate_from_folder).parameters["mci_motion"].default == "linear"
    text = " ".join(inference.build_parser().format_help().split())      # (argparse wraps the lines)
    for words in ("--mci-motion", "constant velocity", "a t (1 - t) / 2", "first and last segment", "three times the field work",
                  "the 3x3 median is the only guard", "interior occlusion reasoning", "only together with --mci-detail keyframes"):
        assert words in text, words
    base = ["--input-dir", "x", "--background", "mci"]
    assert inference.parse_args(base).mci_motion == "linear"
    assert inference.parse_args(base + ["--mci-motion", "linear"]).mci_motion == "linear"
    for more in ([], ["--mci-range", "128", "--mci-border", "valid", "--mci-precision", "half", "--mci-sampler", "cubic"], ["--mci-person", "exclude"],
                 ["--output-size", "keyframes", "--mci-detail", "keyframes"]):
        assert inference.parse_args(base + ["--mci-motion", "quadratic"] + more).mci_motion == "quadratic"
    for bad in (["--input-dir", "x", "--mci-motion", "quadratic"], ["--input-dir", "x", "--mci-motion", "linear"], base + ["--mci-motion", "cubic"],
                base + ["--mci-motion", "quadratic", "--output-size", "keyframes"]):
        with pytest.raises(SystemExit):
            inference.parse_args(bad)


def test_reference_protocol_driver(tmp_path):
    """32x32 model, 5 key frames at rate 2 of a scene that accelerates, and a clip of one segment: without the setting, and with
    mci_motion="linear", the files are the same (the defaults give the files of before); "quadratic" feeds the model
    mci_frames_accel_host's frames - the middle segment with both neighbours' fields, the first with the one-sided rule - and the
    one-segment clip gets the linear files; the summary line names the setting."""
    import torch
    from render_in_between_amd import evaluator as ev, inference, resize
    from tests.composite_common import write_example
    from tests.test_composite_cpu import Recorder, cfg32, dirs_of, png
    from tests.test_driver import oracle_labels
    class Recording(Recorder):                 # ... and every call's background
        dains = []

        def __call__(self, label, label_prev, dain, prev):
            self.dains = self.dains + [dain.detach().clone()]
            return super().__call__(label, label_prev, dain, prev)
    root = str(tmp_path)
    for clip, n_key in (("clipA", 5), ("clipB", 2)):
        write_example(root, n_key=n_key, rate=2, key_hw=(32, 32), clip=clip, seed=n_key)
        mc.accelerating_keys(root, n_key, (32, 32), clip)
    inputs_dir, _, pose_dir = dirs_of(root)
    runs = {}
    for name, kw in (("plain", {}), ("linear", dict(mci_motion="linear")), ("quadratic", dict(mci_motion="quadratic"))):
        M, E = Recording(), ev.Evaluator(cfg32(), label_fn=oracle_labels)
        written = E.evaluate_from_folder(M, inputs_dir, None, pose_dir, os.path.join(root, name), background="mci", **kw)
        assert ("quadratic motion" in inference.summary_line(E)) == (name == "quadratic")
        runs[name] = ({os.path.relpath(x, os.path.join(root, name)): open(x, "rb").read() for x in written}, M)
    assert len(runs["plain"][0]) == 9 + 3 and runs["plain"][0] == runs["linear"][0]
    quad, lin = runs["quadratic"][0], runs["linear"][0]
    assert all(quad[n] == lin[n] for n in quad if n.startswith("clipB")) and any(quad[n] != lin[n] for n in quad if n.startswith("clipA"))
    keys = [resize.resize_cubic_u8(png(os.path.join(root, "inputs", "clipA", "%04d.png" % k)), 32, 32) for k in range(5)]
    f = [bg.mci_field_host(keys[k], keys[k + 1]) for k in range(4)]
    acc = [bg.mci_accel_host(f[k - 1] if k else None, f[k], f[k + 1] if k < 3 else None) for k in range(4)]
    assert any(a.any() for a in acc)
    dains = [d for d in runs["quadratic"][1].dains]
    for k in range(4):                          # the model's background of the frame in the middle of segment k
        want = bg.normalised_upload(bg.mci_frames_accel_host(keys[k], keys[k + 1], f[k], acc[k], 2, [1]))
        assert torch.equal(dains[k], torch.from_numpy(want)), k


def test_abi_is_declared_and_bound():
    from render_in_between_amd import _native
    hdr = open(os.path.join(ROOT, "include", "rib.h")).read()
    assert "size_t rib_accel_workspace_bytes(rib_handle* h, int B, int Hb, int Wb);" in hdr
    assert "int rib_accel_field(rib_handle* h, int B, int Hb, int Wb, const int16_t* prev_i16, const int16_t* cur_i16, const int16_t* next_i16," in hdr
    assert "int rib_accel_frames(rib_handle* h, int T, int B, int H, int W, const uint8_t* a_u8, const uint8_t* b_u8," in hdr
    sig = _native.SIGNATURES
    assert len(sig["rib_accel_workspace_bytes"][1]) == 4 and len(sig["rib_accel_field"][1]) == 12 and len(sig["rib_accel_frames"][1]) == 19
    src = open(os.path.join(ROOT, "render-in-between_amd", "csrc", "frame.hip")).read()
    for name in ("rib_accel_workspace_bytes", "rib_accel_field", "rib_accel_frames"):
        assert re.search(r"\n(int|size_t) %s\(rib_handle\* handle?" % name, src) or re.search(r"\n(int|size_t) %s\(rib_handle\* h" % name, src), name
    if os.path.exists(_native.LIB_PATH):
        import ctypes
        lib = ctypes.CDLL(_native.LIB_PATH)
        assert all(hasattr(lib, n) for n in ("rib_accel_workspace_bytes", "rib_accel_field", "rib_accel_frames"))
