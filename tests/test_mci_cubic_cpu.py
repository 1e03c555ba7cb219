"""The 4x4 cubic sampler of the interpolated backgrounds (no GPU): background.cubic_weights / sample_cubic / sample_clean_cubic and
sampler="cubic" of mci_frames_host, mci_frames_masked_host and mci_frames_scaled_host - the driver's mci_sampler - held to the
integer definition (a per-pixel loop restatement), to what must NOT change (whole-pixel offsets, the key frames, equal sizes), to
the quality it was built for (true frames at quarter-pixel positions), and to the staging rule the kernels follow
(background.cubic_tile_staged over the inputs of tests/test_gpu_mci_cubic.py, built in tests/mci_cubic_common.py)."""
import inspect
import os

import numpy as np
import pytest

from render_in_between_amd import background as bg
from tests import mci_cubic_common as cc
from tests.test_background_cpu import random_pair

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. the weights ----------------------------------------------------------------------------------------------------------------
def test_weights():
    w = bg.cubic_weights()
    assert w.dtype == np.int32 and w.shape == (256, 4)
    assert (w.sum(1) == 128).all()
    assert w[0].tolist() == [0, 128, 0, 0] and w[128].tolist() == [-8, 72, 72, -8]
    assert w.min() == -9 and w.max() == 128
    assert all(np.array_equal(w[256 - f], w[f][::-1]) for f in range(1, 256))      # the symmetry holds for every f (f = 0 has no partner)
    assert int(np.abs(w).sum(1).max()) == 160                                      # the docstring's int32 bound: 255 * 160^2 < 2^23
    # the formula, restated with Python integers
    for f in (1, 37, 127, 129, 255):
        n = [-f ** 3 + 512 * f * f - 65536 * f, 3 * f ** 3 - 1280 * f * f + 2 * 256 ** 3, -3 * f ** 3 + 1024 * f * f + 65536 * f, f ** 3 - 256 * f * f]
        v = [(x + (1 << 17)) >> 18 for x in n]
        v[1 if v[1] >= v[2] else 2] += 128 - sum(v)
        assert w[f].tolist() == v
        t = f / 256.0                       # and it IS Catmull-Rom, to the rounding (the residual may add one more unit)
        cr = [(-t ** 3 + 2 * t * t - t) / 2, (3 * t ** 3 - 5 * t * t + 2) / 2, (-3 * t ** 3 + 4 * t * t + t) / 2, (t ** 3 - t * t) / 2]
        assert max(abs(a - 128 * b) for a, b in zip(v, cr)) <= 1.5


# ---- 2. flat frames stay flat ----------------------------------------------------------------------------------------------------------
def test_flat_frames_stay_flat():
    rng = np.random.default_rng(1)
    py, px = rng.integers(-3000, 9000, (40, 50)).astype(np.int32), rng.integers(-3000, 9000, (40, 50)).astype(np.int32)      # far outside too
    for v in (0, 1, 127, 254, 255):
        img = np.full((13, 17, 3), v, np.uint8)
        assert (bg.sample_cubic(img, py, px) == v).all()


# ---- 3. the loop restatement -----------------------------------------------------------------------------------------------------------
def loop_sample(img, py, px):
    """One cubic sample in plain Python: (value [3], the 16 clamped taps' coordinates)."""
    h, w = img.shape[:2]
    W = bg.cubic_weights()
    wy, wx = W[py & 255], W[px & 255]
    rows = [min(max((py >> 8) - 1 + r, 0), h - 1) for r in range(4)]
    cols = [min(max((px >> 8) - 1 + c, 0), w - 1) for c in range(4)]
    out = []
    for ch in range(3):
        acc = 0
        for r in range(4):
            acc += int(wy[r]) * sum(int(wx[c]) * int(img[rows[r], cols[c], ch]) for c in range(4))
        assert abs(acc) <= 5352960
        out.append(min(max((acc + 8192) >> 14, 0), 255))
    return out, [(y, x) for y in rows for x in cols]


def loop_frames(a, b, pos, s, k, border, ma=None, mb=None):
    """Frame k from its sample positions (bg.sample_positions: the offsets are not the sampler's business), pixel by pixel."""
    h, w = a.shape[:2]
    pay, pax, pby, pbx = pos
    ls = s.bit_length() - 1
    out = np.empty((h, w, 3), np.uint8)
    for y in range(h):
        for x in range(w):
            va, ta = loop_sample(a, int(pay[y, x]), int(pax[y, x]))
            vb, tb = loop_sample(b, int(pby[y, x]), int(pbx[y, x]))
            oka = okb = True
            if ma is not None:
                oka, okb = not any(ma[t] for t in ta), not any(mb[t] for t in tb)
            if border == "valid":           # the POSITION lies inside the frame
                oka = oka and 0 <= pay[y, x] <= (h - 1) << 8 and 0 <= pax[y, x] <= (w - 1) << 8
                okb = okb and 0 <= pby[y, x] <= (h - 1) << 8 and 0 <= pbx[y, x] <= (w - 1) << 8
            if ma is not None and k in (0, s):
                oka, okb = k == 0, k == s
            for c in range(3):
                blend = ((s - k) * va[c] + k * vb[c] + s // 2) >> ls
                out[y, x, c] = blend if oka == okb else va[c] if oka else vb[c]
    return out


def test_sample_cubic_equals_the_loop():
    img = random_pair(13, 17, 2)[0]
    rng = np.random.default_rng(3)
    py, px = rng.integers(-700, 13 * 256 + 700, 300).astype(np.int32), rng.integers(-700, 17 * 256 + 700, 300).astype(np.int32)
    py[:4], px[:4] = (0, 12 << 8, -256, 3071), (0, 16 << 8, 17 << 8, 4095)
    got = bg.sample_cubic(img, py, px)
    assert got.dtype == np.int32 and got.shape == (300, 3)
    assert got.tolist() == [loop_sample(img, int(y), int(x))[0] for y, x in zip(py, px)]
    mask = rng.random((13, 17)) < 0.2
    clean = bg.sample_clean_cubic(mask, py, px)
    assert clean.tolist() == [not any(mask[t] for t in loop_sample(img, int(y), int(x))[1]) for y, x in zip(py, px)]
    assert clean.any() and not clean.all()


@pytest.mark.parametrize("precision", bg.PRECISIONS)
@pytest.mark.parametrize("border", bg.BORDERS)
def test_the_frame_functions_equal_the_loop(border, precision):
    h, w, s = 13, 17, 4
    a, b = random_pair(h, w, 4)
    f = cc.field("random", h, w, precision)
    f = (f // 8).astype(np.int16)           # +-10 px: inside, across and beyond the edges of a 13 x 17 frame
    ma, mb = (np.random.default_rng(5).random((2, h, w)) < 0.15).astype(np.uint8) * 7
    ks = [0, 1, 3, 4]
    got = bg.mci_frames_host(a, b, f, s, ks, border=border, precision=precision, sampler="cubic")
    gotm = bg.mci_frames_masked_host(a, b, ma, mb, f, s, ks, border=border, precision=precision, sampler="cubic")
    assert got.dtype == gotm.dtype == np.uint8 and got.shape == gotm.shape == (4, h, w, 3)
    one_sided = 0
    for j, k in enumerate(ks):
        pos = bg.sample_positions(f, s, k, h, w, precision)
        assert np.array_equal(got[j], loop_frames(a, b, pos, s, k, border)), k
        assert np.array_equal(gotm[j], loop_frames(a, b, pos, s, k, border, ma != 0, mb != 0)), k
        one_sided += int((got[j] != gotm[j]).any())
    assert one_sided                        # the masks matter
    # the scaled form, 13 x 17 -> 29 x 23
    a0, b0 = random_pair(29, 23, 6)
    gots = bg.mci_frames_scaled_host(a0, b0, f, (h, w), s, [1, 2], border=border, precision=precision, sampler="cubic")
    for j, k in enumerate([1, 2]):
        pos = bg.sample_positions(f, s, k, 29, 23, precision, model_hw=(h, w))
        assert np.array_equal(gots[j], loop_frames(a0, b0, pos, s, k, border)), k


def test_the_border_rule_is_the_bilinear_ones():
    """The set of one-sided pixels under border="valid" does not depend on the sampler: the rule looks at the position."""
    h, w, s = 40, 56, 4
    a, b = np.zeros((h, w, 3), np.uint8), np.full((h, w, 3), 255, np.uint8)      # a one-sided pixel is 0 or 255, a blend is neither (k = 1, 2, 3)
    f = cc.field("random", h, w)
    for k in (1, 2, 3):
        bi = bg.mci_frames_host(a, b, f, s, [k], border="valid")[0]
        cu = bg.mci_frames_host(a, b, f, s, [k], border="valid", sampler="cubic")[0]
        assert np.array_equal(bi, cu) and (bi == 0).any() and (bi == 255).any()


# ---- 4. what must not change -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("border", bg.BORDERS)
def test_whole_pixel_offsets_give_the_bilinear_bytes(border):
    h, w = 40, 56
    a, b = random_pair(h, w, 7)
    ma, mb = cc.masks("blobs", h, w)
    f = np.empty(bg.field_shape(h, w) + (2,), np.int16)
    for d, s, ks in (((6, -4), 4, [0, 1, 2, 3, 4]), ((3, -5), 2, [0, 1, 2]), ((7, 1), 8, [0, 4, 8]), ((0, 0), 8, range(9))):
        f[...] = d                          # a uniform field: 2 d k / s is whole for every k listed
        assert all((2 * c * k) % s == 0 for c in d for k in ks)
        assert np.array_equal(bg.mci_frames_host(a, b, f, s, ks, border=border, sampler="cubic"), bg.mci_frames_host(a, b, f, s, ks, border=border))
    f[...] = (5, -3)                        # in half pixels: d k / s whole
    assert np.array_equal(bg.mci_frames_host(a, b, f, 1, [0, 1], border=border, precision="half", sampler="cubic"),
                          bg.mci_frames_host(a, b, f, 1, [0, 1], border=border, precision="half"))
    # masked: the bytes agree wherever the 4x4 footprint sees what the 2x2 footprint sees - with all-zero masks everywhere
    z = np.zeros((h, w), np.uint8)
    f[...] = (6, -4)
    assert np.array_equal(bg.mci_frames_masked_host(a, b, z, z, f, 4, range(5), border=border, sampler="cubic"),
                          bg.mci_frames_host(a, b, f, 4, range(5), border=border))
    differs = (bg.mci_frames_masked_host(a, b, ma, mb, f, 4, [1], border=border, sampler="cubic")
               != bg.mci_frames_masked_host(a, b, ma, mb, f, 4, [1], border=border))[0].any(-1)
    pay, pax, pby, pbx = bg.sample_positions(f, 4, 1, h, w)
    same = (bg.sample_clean(ma != 0, pay, pax) == bg.sample_clean_cubic(ma != 0, pay, pax)) \
        & (bg.sample_clean(mb != 0, pby, pbx) == bg.sample_clean_cubic(mb != 0, pby, pbx))
    assert differs.any() and not (differs & same).any()      # only where the wider footprint sees another mask pixel: the seam moves


@pytest.mark.parametrize("precision", bg.PRECISIONS)
@pytest.mark.parametrize("border", bg.BORDERS)
def test_the_end_frames_are_the_key_frames(border, precision):
    for h, w in ((1, 1), (13, 17), (40, 56)):
        a, b = random_pair(h, w, 8)
        f = cc.field("random", h, w, precision)
        ones = np.ones((h, w), np.uint8)
        for s in (1, 4, 1024):
            out = bg.mci_frames_host(a, b, f, s, [0, s], border=border, precision=precision, sampler="cubic")
            assert np.array_equal(out[0], a) and np.array_equal(out[1], b)
            out = bg.mci_frames_masked_host(a, b, ones, ones, f, s, [0, s], border=border, precision=precision, sampler="cubic")
            assert np.array_equal(out[0], a) and np.array_equal(out[1], b)
            out = bg.mci_frames_scaled_host(a, b, f, (h, w), s, [0, s], border=border, precision=precision, sampler="cubic")
            assert np.array_equal(out[0], a) and np.array_equal(out[1], b)


@pytest.mark.parametrize("border", bg.BORDERS)
def test_scaled_at_equal_sizes_is_the_unscaled_form(border):
    for (h, w), precision in (((40, 56), "full"), ((67, 93), "half"), ((5, 7), "full")):
        a, b = random_pair(h, w, 9)
        for kind in ("random", "smooth"):
            f = cc.field(kind, h, w, precision)
            one = bg.mci_frames_host(a, b, f, 8, [1, 4, 7], border=border, precision=precision, sampler="cubic")
            assert np.array_equal(bg.mci_frames_scaled_host(a, b, f, (h, w), 8, [1, 4, 7], border=border, precision=precision, sampler="cubic"), one)


def test_the_default_is_bilinear_and_other_names_are_refused():
    a, b = random_pair(13, 17, 10)
    f = cc.field("random", 13, 17)
    z = np.zeros((13, 17), np.uint8)
    assert np.array_equal(bg.mci_frames_host(a, b, f, 4, [1], sampler="bilinear"), bg.mci_frames_host(a, b, f, 4, [1]))
    assert not np.array_equal(bg.mci_frames_host(a, b, f, 4, [1], sampler="cubic"), bg.mci_frames_host(a, b, f, 4, [1]))
    for fn, args in ((bg.mci_frames_host, (a, b, f, 4, [1])), (bg.mci_frames_masked_host, (a, b, z, z, f, 4, [1])),
                     (bg.mci_frames_scaled_host, (a, b, f, (13, 17), 4, [1]))):
        assert list(inspect.signature(fn).parameters)[-1] == "sampler" and inspect.signature(fn).parameters["sampler"].default == "bilinear"
        for bad in ("bicubic", None, 3):
            with pytest.raises(ValueError, match="sampler must be 'bilinear' or 'cubic'"):
                fn(*args, sampler=bad)


# ---- 5. quality: true frames at quarter-pixel positions -----------------------------------------------------------------------------------
# tests/mci_cubic_common.scene: 160 x 192 frames box-downsampled 4x from one texture, s = 4, five even motions, seeds 0..5, the TRUE
# uniform field m / 2, interior with a 24 px inset.  Measured with the committed definition (this test prints every figure): bilinear
# 34.5 dB on the diagonal motions and 38.0 dB on the axis-aligned ones, cubic 39.0 and 42.1 dB; the gain of the 60 cases lies in
# 3.97 .. 4.49 dB (smallest 3.972).  MARGIN is half the smallest of those gains: a sampler that lost half of what it was built for
# fails, rounding noise does not.  Sharpness (variance of second differences over the true frame's): bilinear 0.39 .. 0.65, cubic
# 0.61 .. 0.80.
MARGIN = 3.972 / 2


def test_quality_against_true_frames():
    gains, sharp = [], []
    for m in cc.QMOTIONS:
        for seed in cc.QSEEDS:
            frames, f = cc.scene(seed, m)
            bi = bg.mci_frames_host(frames[0], frames[4], f, 4, range(5))
            cu = bg.mci_frames_host(frames[0], frames[4], f, 4, range(5), sampler="cubic")
            for k in (0, 2, 4):             # whole-pixel offsets: the bilinear bytes, and k = 2 IS the truth on the interior
                assert np.array_equal(bi[k], cu[k])
            assert np.array_equal(cc.interior(cu[2]), cc.interior(frames[2]))
            for k in (1, 3):
                pb, pc = cc.psnr(bi[k], frames[k]), cc.psnr(cu[k], frames[k])
                sb, sc = cc.sharpness(bi[k], frames[k]), cc.sharpness(cu[k], frames[k])
                print("m=%s seed=%d k=%d  PSNR bilinear %.2f cubic %.2f gain %.2f dB  sharpness bilinear %.2f cubic %.2f" % (m, seed, k, pb, pc, pc - pb, sb, sc))
                gains.append(pc - pb)
                sharp.append((sb, sc))
    print("gain %.2f .. %.2f dB over %d cases; sharpness bilinear %.2f .. %.2f, cubic %.2f .. %.2f"
          % (min(gains), max(gains), len(gains), min(s[0] for s in sharp), max(s[0] for s in sharp), min(s[1] for s in sharp), max(s[1] for s in sharp)))
    assert len(gains) == 60 and min(gains) >= MARGIN
    assert all(sc > sb for sb, sc in sharp)


# ---- 6. the staging rule over the GPU tests' inputs --------------------------------------------------------------------------------------
def test_the_gpu_inputs_exercise_both_paths():
    s, ks = 8, range(9)
    seen = set()
    for precision in bg.PRECISIONS:
        for h, w in cc.WIDE:
            share = {kind: cc.staged_share(kind, h, w, precision, s, ks) for kind in cc.KINDS}
            print("%dx%d %s staged share: %s" % (h, w, precision, {k: round(v, 3) for k, v in share.items()}))
            assert share["zero"] == 1.0 and share["smooth"] >= 0.9
            assert share["random"] <= 0.1
            assert 0.1 <= share["mixed"] <= 0.9
            seen |= {share["smooth"] > 0, share["random"] < 1}
        for h, w in [x for x in cc.SIZES if x not in cc.WIDE]:      # a tile of at most 7 pixels in at most 5 rows always fits
            assert cc.staged_share("random", h, w, precision, s, ks) == 1.0
    assert seen == {True}


def test_the_staging_rule():
    z = np.zeros((2, 130), np.int32)
    X = (np.arange(130, dtype=np.int32) << 8)[None, :].repeat(2, 0)
    Y = (np.arange(2, dtype=np.int32) << 8)[:, None].repeat(130, 1)
    got = bg.cubic_tile_staged(Y, X, Y, X)
    assert got.dtype == bool and got.shape == (2, 3) and got.all()                 # at rest: 4 rows x 67 columns
    px = X.copy()
    px[0, 10] += 9 << 8                     # one pixel of tile 0 reaches 9 columns further: still 76 >= 67 + 9
    assert bg.cubic_tile_staged(Y, px, Y, X).all()
    px[0, 63] += 10 << 8                    # the tile's last pixel 10 further: 77 columns
    assert bg.cubic_tile_staged(Y, px, Y, X).tolist() == [[False, True, True], [True, True, True]]
    py = Y.copy()
    py[1, 64] -= 8 << 8                     # 4 + 8 = 12 rows: fits; one more does not - and it is key frame B's turn
    assert bg.cubic_tile_staged(Y, X, py, X).all()
    py[1, 64] -= 1
    assert bg.cubic_tile_staged(Y, X, py, X).tolist() == [[True, True, True], [True, False, True]]
    assert bg.cubic_tile_staged(Y - (500 << 8), X + (900 << 8), Y, X).all()        # far outside the frame: the rule sees unclamped taps
    assert z.shape == (2, 130) and (bg.CUBIC_TILE, bg.CUBIC_WIN_ROWS, bg.CUBIC_WIN_COLS) == (64, 12, 76)
    src = open(os.path.join(ROOT, "render-in-between_amd", "csrc", "mci.hip.h")).read()
    assert "constexpr int CUBIC_TILE = 64, CUBIC_WIN_ROWS = 12, CUBIC_WIN_COLS = 76;" in src


# ---- 7. settings, errors, the driver ---------------------------------------------------------------------------------------------------
def test_check_settings():
    ok = lambda **kw: bg.check_settings("mci", 32, "clamp", "host", **kw)
    assert ok() == ok(mci_sampler="bilinear") == ok(mci_sampler="cubic") == (3, "clamp")
    assert list(inspect.signature(bg.check_settings).parameters) == ["background", "mci_range", "mci_border", "resize_on", "who", "mci_precision",
                                                                       "mci_person", "output_size", "mci_sampler"]
    assert bg.check_settings("mci", 64, "valid", "host", "who", "half", "keep", "keyframes", mci_sampler="cubic") == (4, "valid")
    assert ok(mci_sampler="cubic", mci_person="exclude") == ok(mci_sampler="cubic", mci_precision="half", output_size="keyframes") == (3, "clamp")
    for bad in ("bicubic", None, 1, "Cubic"):
        with pytest.raises(ValueError, match="mci_sampler must be 'bilinear' or 'cubic'"):
            ok(mci_sampler=bad)
    with pytest.raises(ValueError, match="mci_sampler is a setting of background='mci'"):
        bg.check_settings("dain", 32, "clamp", "host", mci_sampler="cubic")
    with pytest.raises(ValueError, match="mci_person='exclude' with mci_precision='half'"):      # the existing refusals stay
        ok(mci_sampler="cubic", mci_person="exclude", mci_precision="half")


def test_the_driver_refuses_before_any_file(tmp_path):
    import render_in_between_amd as rib
    from render_in_between_amd import evaluator as ev, inference
    cfg = rib.AttrDict(gen=rib.hsm_gen_config(), model_height=64, model_width=64, gauss_sigma=5, skeleton_thres=0.001, foot_thres=0.001)
    out = os.path.join(str(tmp_path), "out")
    with pytest.raises(ValueError, match="mci_sampler must be"):
        ev.Evaluator(cfg).evaluate_from_folder(lambda *a: None, str(tmp_path), None, str(tmp_path), out, background="mci", mci_sampler="sharp")
    with pytest.raises(ValueError, match="mci_sampler is a setting of background='mci'"):
        ev.Evaluator(cfg).evaluate_from_folder(lambda *a: None, str(tmp_path), str(tmp_path), str(tmp_path), out, mci_sampler="cubic")
    assert not os.path.exists(out)
    text = " ".join(inference.build_parser().format_help().split())      # (argparse wraps the lines)
    for words in ("--mci-sampler", "overshoots at strong edges", "clamped", "footprint is 4x4", "seam moves by a pixel", "without interior occlusion reasoning",
                  "trained on DAIN backgrounds", "quality on real footage is unmeasured"):
        assert words in text, words
    base = ["--input-dir", "x", "--background", "mci"]
    assert inference.parse_args(base).mci_sampler == "bilinear"
    assert inference.parse_args(base + ["--mci-sampler", "bilinear"]).mci_sampler == "bilinear"
    for more in ([], ["--mci-range", "128", "--mci-border", "valid", "--mci-precision", "half", "--output-size", "keyframes"], ["--mci-person", "exclude"],
                 ["--panels", "--video", "--png-on", "gpu"]):
        assert inference.parse_args(base + ["--mci-sampler", "cubic"] + more).mci_sampler == "cubic"
    for bad in (base + ["--mci-sampler", "lanczos"], ["--input-dir", "x", "--mci-sampler", "cubic"], ["--input-dir", "x", "--mci-sampler", "bilinear"]):
        with pytest.raises(SystemExit):
            inference.parse_args(bad)


def test_driver_at_64x64_through_a_stand_in_model(tmp_path):
    """Two key frames 6 x -2 px apart at rate 4: frames 1 and 3 sit at one and a half pixels.  mci_sampler="bilinear" writes the
    default's bytes; "cubic" feeds the model the cubic definition's floats, changes frames 1..3's files and leaves the key frames'."""
    import torch
    import render_in_between_amd as rib
    from render_in_between_amd import evaluator as ev, inference, synth
    from oracle import generator_ref
    from tests.test_background_cpu import _example_without_dain
    from tests.test_driver import oracle_labels
    from tests.test_keyframes_size_cpu import moving_keys
    from tests.test_mci_range_cpu import _cfg64
    root = str(tmp_path)
    _example_without_dain(root, n_key=2, rate=4, H=64, W=64)
    moving_keys(root, 2, (64, 64), step=(6, -2))
    cfg = _cfg64()
    spec = rib.GenSpec.from_cfg(cfg.gen)
    R = generator_ref.RefGenerator(spec, synth.make_state_dict(spec, 2))
    calls = []

    class Model:
        def eval(self):
            return self

        def __call__(self, label, label_prev, dain, prev):
            calls.append(dain.clone())
            return R(label, label_prev, dain, prev)
    dirs = (os.path.join(root, "inputs"), None, os.path.join(root, "Predict_motion"))
    E = ev.Evaluator(cfg, label_fn=oracle_labels)
    runs = {}
    for name, kw in (("plain", {}), ("bilinear", dict(mci_sampler="bilinear")), ("cubic", dict(mci_sampler="cubic"))):
        del calls[:]
        written = E.evaluate_from_folder(Model(), *dirs, os.path.join(root, name), background="mci", **kw)
        assert len(written) == 5
        assert ("cubic sampler" in inference.summary_line(E)) == (name == "cubic")      # the run summary names the sampler when it is cubic
        runs[name] = ([open(x, "rb").read() for x in written], torch.cat(list(calls)))
    assert runs["plain"][0] == runs["bilinear"][0] and torch.equal(runs["plain"][1], runs["bilinear"][1])
    a, b = (E._decode_resized_u8(os.path.join(root, "inputs", "clipA", "%04d.png" % k))[0] for k in range(2))
    field = bg.mci_field_host(a, b)
    assert field.any()
    want = bg.normalised_upload(bg.mci_frames_host(a, b, field, 4, [1, 2, 3], sampler="cubic"))
    assert torch.equal(runs["cubic"][1].reshape(want.shape), torch.from_numpy(want))
    assert not torch.equal(runs["cubic"][1], runs["plain"][1])
    files, plain = runs["cubic"][0], runs["plain"][0]
    assert files[0] == plain[0] and files[4] == plain[4] and files[1] != plain[1] and files[3] != plain[3]


# ---- 8. the C ABI ------------------------------------------------------------------------------------------------------------------------
def test_abi_is_declared_bound_and_exported():
    from render_in_between_amd import _native
    hdr = open(os.path.join(ROOT, "include", "rib.h")).read()
    assert "int rib_cubic_frames(rib_handle* h, int T, int B, int H, int W, const uint8_t* a_u8, const uint8_t* b_u8," in hdr
    assert "const int16_t* field_i16, int sample_rate, int k_first, int border, int precision, int staging," in hdr
    assert "int rib_cubic_scaled(rib_handle* h, int T, int B, int H, int W, int H0, int W0, const uint8_t* a0_u8, const uint8_t* b0_u8," in hdr
    assert "It is a DIAGNOSTIC for the tests and the benches: the bytes never depend on it." in hdr
    sig = _native.SIGNATURES
    assert len(sig["rib_cubic_frames"][1]) == 18 and len(sig["rib_cubic_scaled"][1]) == 17
    assert len(sig["rib_mci_frames"][1]) == 14 and len(sig["rib_masked_frames"][1]) == 17 and len(sig["rib_scaled_frames"][1]) == 16      # pinned
    family = sorted(n for n in sig if n.startswith("rib_mci_"))
    assert family == ["rib_mci_field", "rib_mci_field_shape", "rib_mci_frames", "rib_mci_workspace_bytes"]
    src = open(os.path.join(ROOT, "render-in-between_amd", "csrc", "frame.hip")).read()
    for name in ("rib_cubic_frames", "rib_cubic_scaled"):
        assert ("\nint %s(rib_handle* h" % name) in src
    if os.path.exists(_native.LIB_PATH):                  # a built tree: the library exports them
        import ctypes
        lib = ctypes.CDLL(_native.LIB_PATH)
        assert hasattr(lib, "rib_cubic_frames") and hasattr(lib, "rib_cubic_scaled")
