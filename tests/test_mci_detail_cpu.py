"""background.mci_detail_field_host - the block field refined at the key frames' own size (the driver's mci_detail="keyframes") - held
to its properties on the CPU: it is the composition of the existing functions wherever their key holds the vectors, equal sizes
search one pixel around the field, a translating scene whose motion is NOT a multiple of the size ratio comes back exactly where
mci_frames_scaled_host cannot give it, the key and the frames' int32 arithmetic have the room they claim, and the settings, the
command line, the driver and the C ABI carry the option.  Every comparison is exact."""
import inspect
import os

import numpy as np
import pytest

from render_in_between_amd import background as bg
from tests import mci_detail_common as dc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANTS = [(b, p) for b in bg.BORDERS for p in bg.PRECISIONS]


# ---- 1. the definition is the existing functions' composition --------------------------------------------------------------------------
@pytest.mark.parametrize("model,size,B,amp", dc.SHAPES[:5])
def test_matches_the_existing_functions(model, size, B, amp):
    """start (pixel_field_scaled at the block's pixel, rounded), search(..., wide=True), median3: every candidate lies within +-79
    here (amp <= 4 model pixels at a ratio <= 8, R <= 4; pack_key_wide's |d|^2 field is made for max_disp(5) = 79), so
    pack_key_wide holds them and the winners must be the same."""
    a, b = dc.pairs(size, B)
    R = bg.detail_radius(model, size)
    for border, precision in VARIANTS:
        f = dc.random_fields(model, B, amp, precision)
        for i in range(B):
            dsx, dsy = bg.pixel_field_scaled(f[i], model, size)
            ys, xs = np.minimum(8 * np.arange((size[0] + 7) // 8) + 4, size[0] - 1), np.minimum(8 * np.arange((size[1] + 7) // 8) + 4, size[1] - 1)
            sh, rnd = (9, 256) if precision == "half" else (8, 128)
            sx, sy = ((dsx[ys][:, xs] + rnd) >> sh).astype(np.int32), ((dsy[ys][:, xs] + rnd) >> sh).astype(np.int32)
            assert max(np.abs(sx).max(), np.abs(sy).max()) + R <= bg.max_disp(bg.MAX_LEVELS)
            dx, dy = bg.search(bg.luma(a[i]), bg.luma(b[i]), sx, sy, R, wide=True, border=border)
            want = np.stack([bg.median3(dx), bg.median3(dy)], -1).astype(np.int16)
            got = bg.mci_detail_field_host(a[i], b[i], f[i], model, border=border, precision=precision)
            assert got.dtype == np.int16 and got.shape == bg.field_shape(*size) + (2,)
            assert np.array_equal(got, want), (border, precision, i)
            assert np.array_equal(got, dc.want_fields(model, size, B, amp, border, precision)[i])


def test_the_radius():
    r = bg.detail_radius
    assert [r((64, 64), (n, n)) for n in (16, 64, 65, 128, 129, 256, 257, 384, 385, 512, 1024)] == [1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 4]
    assert r((512, 512), (1080, 1920)) == 2 and r((512, 512), (720, 1280)) == 2 and r((512, 512), (512, 512)) == 1
    assert r((64, 512), (64, 1920)) == 2 and r((512, 64), (1920, 64)) == 2                # the larger axis decides
    with pytest.raises(ValueError, match="within 1/16"):
        r((16, 16), (16, 257))
    assert bg.DETAIL_MAX_RADIUS == 4 and bg.DETAIL_MAX_DISP == 79 * 16 + 4 == 1268


@pytest.mark.parametrize("border", bg.BORDERS)
def test_equal_sizes_search_one_pixel_around_the_field(border):
    """(h0, w0) == (H, W): R = 1, every start is the field's own vector where the field is constant, and the result lies within 1."""
    h, w = 40, 56
    a, b = dc.pairs((h, w), 1)
    assert bg.detail_radius((h, w), (h, w)) == 1
    for d in ((0, 0), (3, -2), (-5, 1)):
        f = np.broadcast_to(np.array(d, np.int16), bg.field_shape(h, w) + (2,)).copy()
        sx, sy = bg.detail_start(f, (h, w), (h, w))
        assert (sx == d[0]).all() and (sy == d[1]).all()
        got = bg.mci_detail_field_host(a[0], b[0], f, (h, w), border=border).astype(np.int32)
        assert np.abs(got - f).max() <= 1
        half = bg.mci_detail_field_host(a[0], b[0], (2 * f).astype(np.int16), (h, w), border=border, precision="half")
        assert np.array_equal(half, got)                                                # 2 f in half pixels starts where f does


# ---- 2. the translation guarantee ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("border", bg.BORDERS)
@pytest.mark.parametrize("index,seed", [(i, s) for i, sc in enumerate(dc.SCENES) for s in sc[3]])
def test_a_translation_that_is_no_multiple_of_the_ratio_comes_back_exactly(index, seed, border):
    """The scene translates by d0 px per side at the key frames' size, d0 no multiple of the ratio.  With a model-size field that is
    right (the recorded seeds) the refined field is d0 on every block 3 max|d0| + 16 px inside the border, every frame 1..s-1 whose
    offsets are whole pixels is the true scene on every examined pixel - and mci_frames_scaled_host on the same input differs from
    the truth on at least nine tenths of them, so the scene does need the refinement."""
    model, (h0, w0), d0, _ = dc.SCENES[index]
    assert (d0[0] * model[1]) % w0 and (d0[1] * model[0]) % h0                          # not a multiple of the ratio, on either axis
    a0, b0, true = dc.scene(index, seed)
    assert dc.model_field_is_right(index, seed, border)
    f = dc.scene_field(index, seed, border)
    F0 = bg.mci_detail_field_host(a0, b0, f, model, border=border)
    inset, s = dc.scene_inset(index), dc.SCENE_RATE
    by, bx = np.mgrid[0:F0.shape[0], 0:F0.shape[1]]
    inner = (8 * by >= inset) & (8 * by + 8 <= h0 - inset) & (8 * bx >= inset) & (8 * bx + 8 <= w0 - inset)
    assert inner.sum() > 1000
    assert int((F0[inner] != np.array(d0, np.int16)).any(-1).sum()) == 0
    ks = [k for k in range(1, s) if true(k, s) is not None]
    assert ks
    new = bg.mci_frames_host(a0, b0, F0, s, ks, border=border)
    old = bg.mci_frames_scaled_host(a0, b0, f, model, s, ks, border=border)
    sl = (slice(inset, h0 - inset), slice(inset, w0 - inset))
    for j, k in enumerate(ks):
        want = true(k, s)[sl]
        n = want.shape[0] * want.shape[1]
        wrong_new, wrong_old = int((new[j][sl] != want).any(-1).sum()), int((old[j][sl] != want).any(-1).sum())
        print("scene %d seed %d %s k=%d: %d examined pixels, wrong %d refined, %d scaled" % (index, seed, border, k, n, wrong_new, wrong_old))
        assert wrong_new == 0
        assert 10 * wrong_old >= 9 * n


# ---- 3. the room the arithmetic claims ---------------------------------------------------------------------------------------------------
def test_the_key_keeps_the_tuples_order_and_has_the_room():
    rng = np.random.default_rng(1)
    m = 1276                                                                            # 159 half pixels at ratio 16, plus the radius
    cost = rng.integers(0, 64 * 255 + 4 * 2 * m + 1, 4000)
    dx, dy = rng.integers(-m, m + 1, 4000), rng.integers(-m, m + 1, 4000)
    cost[:8], dx[:8], dy[:8] = 64 * 255 + 8 * m, [m, -m, m, -m, 0, 0, m, -m], [m, m, -m, -m, m, -m, 0, 0]
    cost[8:2000] = cost[8]                                                              # many ties on the cost: |d|^2, dy, dx decide
    key = bg.pack_key_detail(cost, dx, dy)
    assert key.dtype == np.int64 and key.min() >= 0 and key.max() < (1 << 61)
    order = sorted(range(4000), key=lambda i: (cost[i], dx[i] * dx[i] + dy[i] * dy[i], dy[i], dx[i]))
    assert np.array_equal(np.sort(key), key[order])                                     # sorted by the tuple is sorted by the key
    c, x, y = bg.unpack_key_detail(key)
    assert np.array_equal(c, cost) and np.array_equal(x, dx) and np.array_equal(y, dy)
    lo = rng.integers(-79, 80, (2, 500))                                                # where the wide key holds them: the same order
    cc = rng.integers(0, 2, 500) * 7
    assert np.array_equal(np.argsort(bg.pack_key_wide(cc, lo[0], lo[1]), kind="stable"), np.argsort(bg.pack_key_detail(cc, lo[0], lo[1]), kind="stable"))
    src = open(os.path.join(ROOT, "render-in-between_amd", "csrc", "mci.hip.h")).read()
    assert "constexpr int DETAIL_KEY_BIAS = 2048, DETAIL_MAX_R = 4;" in src and bg.DETAIL_KEY_BIAS == 2048


def test_the_frames_int32_offsets_hold_the_longest_vector():
    """mci_frames_host's largest product unit * k * D with the largest field this feature can make, at the largest rate: it fits
    the kernels' int32 (tests/test_gpu_mci_detail.py holds them to the host with such fields), and the host's offsets are the plain
    integers'."""
    assert 2 * 1024 * 1268 * 256 < 2 ** 31 and 2 * bg.MAX_SAMPLE_RATE * 1276 * (1 << bg.FIELD_FRAC_BITS) + bg.MAX_SAMPLE_RATE // 2 < 2 ** 31
    h, w, s = 16, 24, 1024
    f = np.empty(bg.field_shape(h, w) + (2,), np.int16)
    f[...] = (1268, -1268)
    Dx, Dy = bg.pixel_field(f, h, w)
    assert Dx.min() == Dx.max() == 1268 * 256 and Dy.min() == Dy.max() == -1268 * 256
    pay, pax, pby, pbx = bg.sample_positions(f, s, s - 1, h, w)
    X, Y = np.mgrid[0:h, 0:w][1] << 8, np.mgrid[0:h, 0:w][0] << 8
    wx, wy = (2 * (s - 1) * 1268 * 256 + s // 2) >> 10, (2 * (s - 1) * -1268 * 256 + s // 2) >> 10      # Python integers: no wrap
    assert np.array_equal(X - pax, np.full((h, w), wx)) and np.array_equal(Y - pay, np.full((h, w), wy))
    a, b = dc.pairs((h, w), 1)
    out = bg.mci_frames_host(a[0], b[0], f, s, [0, s], border="valid")                  # and the key frames still come back
    assert np.array_equal(out[0], a[0]) and np.array_equal(out[1], b[0])


def test_far_starts_clamp_or_keep_the_start():
    """8x8 model, 128x128 key frames, components +-79 (+-159 in half pixels): starts near +-1264, far outside the frame."""
    model, size, B, amp = dc.SHAPES[5]
    assert bg.detail_radius(model, size) == 4
    for border, precision in VARIANTS:
        f = dc.random_fields(model, B, amp, precision)[0]
        sx, sy = bg.detail_start(f, model, size, precision)
        assert max(np.abs(sx).max(), np.abs(sy).max()) >= 1200
        got = dc.want_fields(model, size, B, amp, border, precision)[0].astype(np.int32)
        assert np.abs(got).max() <= (1276 if precision == "half" else 1268)
        if border == "valid":                                                           # a start beyond the frame's side is never valid: kept
            a, b = dc.pairs(size, B)
            dx, dy = bg.search_detail(bg.luma(a[0]), bg.luma(b[0]), sx.astype(np.int32), sy.astype(np.int32), 4, "valid")
            far = (np.abs(sx) >= size[1]) | (np.abs(sy) >= size[0])
            assert far.all() and np.array_equal(dx, sx) and np.array_equal(dy, sy)


def test_input_refusals():
    a, b = dc.pairs((40, 56), 1)
    ok = np.zeros(bg.field_shape(16, 24) + (2,), np.int16)
    with pytest.raises(ValueError, match="one size"):
        bg.mci_detail_field_host(a[0], b[0][:, :-1], ok, (16, 24))
    with pytest.raises(ValueError, match=r"int16 \[2, 3, 2\]"):
        bg.mci_detail_field_host(a[0], b[0], ok[:1], (16, 24))
    with pytest.raises(ValueError, match="within 1/16"):
        bg.mci_detail_field_host(a[0], b[0], np.zeros((1, 1, 2), np.int16), (2, 3))
    for precision, lim in (("full", 79), ("half", 159)):
        bad = ok.copy()
        bad[0, 0, 1] = -lim - 1
        with pytest.raises(ValueError, match="-%d..%d" % (lim, lim)):
            bg.mci_detail_field_host(a[0], b[0], bad, (16, 24), precision=precision)
    with pytest.raises(ValueError, match="border must be"):
        bg.mci_detail_field_host(a[0], b[0], ok, (16, 24), border="wrap")
    with pytest.raises(ValueError, match="precision must be"):
        bg.mci_detail_field_host(a[0], b[0], ok, (16, 24), precision="quarter")


# ---- 4. settings, errors, the driver ---------------------------------------------------------------------------------------------------
def test_check_detail():
    """mci_detail has a check of its own, background.check_detail: check_settings keeps the parameter list it had."""
    ok = lambda **kw: bg.check_detail("mci", "keyframes", **kw)
    assert ok() == ok(mci_detail="model") == "model" and ok(mci_detail="keyframes") == "keyframes"
    assert bg.check_detail("dain", "model") == bg.check_detail("mci", "source", "model") == bg.check_detail("dain", "keyframes", "model") == "model"
    assert list(inspect.signature(bg.check_detail).parameters) == ["background", "output_size", "mci_detail", "who"]
    assert inspect.signature(bg.check_detail).parameters["mci_detail"].default == "model"
    assert list(inspect.signature(bg.check_settings).parameters) == ["background", "mci_range", "mci_border", "resize_on", "who", "mci_precision",
                                                                       "mci_person", "output_size", "mci_sampler"]
    for bad in ("full", None, 1, "Keyframes"):
        with pytest.raises(ValueError, match="mci_detail must be 'model' or 'keyframes'"):
            ok(mci_detail=bad)
    for background, size in (("mci", "model"), ("mci", "source"), ("dain", "keyframes"), ("dain", "model")):
        with pytest.raises(ValueError, match="who: mci_detail='keyframes' is a setting of background='mci' with output_size='keyframes'"):
            bg.check_detail(background, size, "keyframes", who="who")
    # the existing refusals stay check_settings': it is called with the settings it had
    with pytest.raises(ValueError, match="mci_person='exclude' with output_size='keyframes'"):
        bg.check_settings("mci", 32, "clamp", "host", mci_person="exclude", output_size="keyframes")
    with pytest.raises(ValueError, match="resize_on='gpu' is not supported"):
        bg.check_settings("mci", 32, "clamp", "gpu", output_size="keyframes")


def test_the_driver_refuses_before_any_file(tmp_path):
    import render_in_between_amd as rib
    from render_in_between_amd import evaluator as ev, inference
    cfg = rib.AttrDict(gen=rib.hsm_gen_config(), model_height=64, model_width=64, gauss_sigma=5, skeleton_thres=0.001, foot_thres=0.001)
    out = os.path.join(str(tmp_path), "out")
    call = lambda dain, **kw: ev.Evaluator(cfg).evaluate_from_folder(lambda *a: None, str(tmp_path), dain, str(tmp_path), out, **kw)
    with pytest.raises(ValueError, match="mci_detail must be"):
        call(None, background="mci", output_size="keyframes", mci_detail="fine")
    with pytest.raises(ValueError, match="mci_detail='keyframes' is a setting of background='mci' with output_size='keyframes'"):
        call(None, background="mci", mci_detail="keyframes")
    with pytest.raises(ValueError, match="mci_detail='keyframes' is a setting of background='mci'"):
        call(str(tmp_path), mci_detail="keyframes")
    with pytest.raises(ValueError, match="mci_person='exclude' with output_size='keyframes'"):      # the existing refusals stay
        call(None, background="mci", output_size="keyframes", mci_detail="keyframes", mci_person="exclude")
    with pytest.raises(ValueError, match="resize_on='gpu' is not supported"):
        ev.Evaluator(cfg, resize_on="gpu").evaluate_from_folder(lambda *a: None, str(tmp_path), None, str(tmp_path), out, background="mci",
                                                               output_size="keyframes", mci_detail="keyframes")
    assert not os.path.exists(out)
    assert inspect.signature(ev.Evaluator.evaluate_from_folder).parameters["mci_detail"].default == "model"
    text = " ".join(inference.build_parser().format_help().split())      # (argparse wraps the lines)
    for words in ("--mci-detail", "soft double image", "at most 4", "without interior occlusion reasoning", "stays wrong beyond R",
                  "capped above a size ratio of 8", "still a cubic enlargement", "quality on real footage is unmeasured"):
        assert words in text, words
    base = ["--input-dir", "x", "--background", "mci"]
    assert inference.parse_args(base).mci_detail == "model"
    assert inference.parse_args(base + ["--mci-detail", "model"]).mci_detail == "model"
    for more in ([], ["--mci-range", "128", "--mci-border", "valid", "--mci-precision", "half", "--mci-sampler", "cubic"], ["--video", "--png-on", "gpu"]):
        assert inference.parse_args(base + ["--output-size", "keyframes", "--mci-detail", "keyframes"] + more).mci_detail == "keyframes"
    for bad in (base + ["--mci-detail", "keyframes"], base + ["--output-size", "keyframes", "--mci-detail", "finer"],
                ["--input-dir", "x", "--mci-detail", "keyframes"], ["--input-dir", "x", "--mci-detail", "model"],
                base + ["--output-size", "keyframes", "--mci-detail", "keyframes", "--mci-person", "exclude"]):
        with pytest.raises(SystemExit):
            inference.parse_args(bad)


def test_reference_protocol_driver_with_the_refined_field(tmp_path):
    """32x32 model, 80x96 key frames (ratio 3, R = 2), 3 key frames at rate 2, a scene that moves by (5, -3) px per key frame - no
    multiple of the ratio: under mci_detail="keyframes" PNG i is composite_host of the model's (img, mask) over mci_frames_host's
    frame at the key frames' size with mci_detail_field_host's field; the model is called with the default's tensors; "model"
    writes the bytes a run without the setting writes, and "keyframes" other ones; the summary line names the setting."""
    import torch
    from render_in_between_amd import composite, inference, evaluator as ev, resize
    from tests.composite_common import write_example
    from tests.test_composite_cpu import Recorder, cfg32, dirs_of, png
    from tests.test_driver import oracle_labels
    from tests.test_keyframes_size_cpu import moving_keys
    root = str(tmp_path)
    n = write_example(root, n_key=3, rate=2, key_hw=(80, 96))
    moving_keys(root, 3, (80, 96), step=(5, -3))
    inputs_dir, _, pose_dir = dirs_of(root)
    runs = {}
    for name, kw in (("plain", {}), ("model", dict(mci_detail="model")), ("keyframes", dict(mci_detail="keyframes", mci_border="valid", mci_sampler="cubic")),
                     ("valid", dict(mci_border="valid", mci_sampler="cubic"))):
        M, E = Recorder(), ev.Evaluator(cfg32(), label_fn=oracle_labels)
        written = E.evaluate_from_folder(M, inputs_dir, None, pose_dir, os.path.join(root, name), background="mci", output_size="keyframes", **kw)
        assert ("field refined at the key frames' size" in inference.summary_line(E)) == (name == "keyframes")
        runs[name] = ([open(x, "rb").read() for x in written], M.calls, written)
    assert n == 5 and runs["plain"][0] == runs["model"][0]
    files, calls, written = runs["keyframes"]
    assert files != runs["valid"][0] and files[0] == runs["valid"][0][0] and files[1] != runs["valid"][0][1]
    for (i0, m0), (i1, m1) in zip(calls, runs["valid"][1]):                             # the generator sees nothing new
        assert torch.equal(i0, i1) and torch.equal(m0, m1)
    keys = [png(os.path.join(root, "inputs", "clipA", "%04d.png" % k)) for k in range(3)]
    small = [resize.resize_cubic_u8(k_, 32, 32) for k_ in keys]
    refined = False
    for k in range(2):
        field = bg.mci_field_host(small[k], small[k + 1], border="valid")
        F0 = bg.mci_detail_field_host(keys[k], keys[k + 1], field, (32, 32), border="valid")
        dsx, dsy = bg.pixel_field_scaled(field, (32, 32), (80, 96))
        refined |= bool((F0[..., 0] * 256 != dsx[4::8, 4::8]).any())
        back = bg.mci_frames_host(keys[k], keys[k + 1], F0, 2, [1], border="valid", sampler="cubic")
        img, mask = calls[k]
        assert np.array_equal(png(written[2 * k + 1]), composite.composite_host(img.numpy(), mask.numpy(), back)[0]), k
    assert refined


# ---- 5. the C ABI ------------------------------------------------------------------------------------------------------------------------
def test_abi_is_declared_bound_and_exported():
    from render_in_between_amd import _native, generator
    hdr = open(os.path.join(ROOT, "include", "rib.h")).read()
    assert "size_t rib_detail_workspace_bytes(rib_handle* h, int B, int H0, int W0);" in hdr
    assert "int rib_detail_field(rib_handle* h, int B, int H, int W, int H0, int W0, const uint8_t* a0_u8, const uint8_t* b0_u8," in hdr
    assert "const int16_t* field_i16, int precision, int border, int16_t* out_field_i16, void* workspace, void* hip_stream);" in hdr
    assert "above ratio 8 the search no longer covers the quantum" in hdr and "there is no new frame entry" in hdr
    sig = _native.SIGNATURES
    assert len(sig["rib_detail_field"][1]) == 14 and len(sig["rib_detail_workspace_bytes"][1]) == 4
    assert len(sig["rib_mci_frames"][1]) == 14 and len(sig["rib_scaled_frames"][1]) == 16 and len(sig["rib_cubic_frames"][1]) == 18      # pinned
    family = sorted(n_ for n_ in sig if n_.startswith("rib_mci_"))
    assert family == ["rib_mci_field", "rib_mci_field_shape", "rib_mci_frames", "rib_mci_workspace_bytes"]
    src = open(os.path.join(ROOT, "render-in-between_amd", "csrc", "frame.hip")).read()
    assert "\nint rib_detail_field(rib_handle* h" in src and "\nsize_t rib_detail_workspace_bytes(rib_handle* h" in src
    assert list(inspect.signature(generator.Generator.mci_detail_field).parameters) == ["self", "a0_u8", "b0_u8", "field", "model_hw", "border", "precision"]
    if os.path.exists(_native.LIB_PATH):                  # a built tree: the library exports them
        import ctypes
        lib = ctypes.CDLL(_native.LIB_PATH)
        assert hasattr(lib, "rib_detail_field") and hasattr(lib, "rib_detail_workspace_bytes")
