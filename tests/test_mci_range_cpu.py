"""The wider motion search of the interpolated backgrounds (no GPU): background.py's `levels` = 3, 4, 5 pyramid levels - the
driver's mci_range = 32, 64, 128 px of motion between key frames - held to what the definition guarantees on pure translations,
to per-pixel loops, to the default's results at levels = 3, and the folder driver's reference-protocol path on it.  The builders
of tests/test_gpu_mci_range.py's inputs live here, with the conditions those inputs must meet stated on the definition alone."""
import importlib
import os

import numpy as np
import pytest

from render_in_between_amd import background as bg, evaluator as ev
from tests.test_background_cpu import (LONG_MOTIONS, TIE_KINDS, _example_without_dain, _model, eroded, guaranteed, long_pair, moving_pair,
                                       pixels_of, random_pair, texture, tie_pair)
from tests.test_driver import oracle_labels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAD = 160                                                               # texture margin: |2 d| <= 128


# ---- levels = 3 is the default ---------------------------------------------------------------------------------------------------
def _default_inputs(h, w):
    yield "random", random_pair(h, w, 3)
    for kind in TIE_KINDS:
        yield kind, tie_pair(kind, h, w)
    for i in range(len(LONG_MOTIONS)):
        yield "long%d" % i, long_pair(h, w, i)


@pytest.mark.parametrize("h,w", [(67, 93), (96, 160)])
def test_three_levels_are_the_default(h, w):
    for name, (a, b) in _default_inputs(h, w):
        assert np.array_equal(bg.mci_field_host(a, b, levels=3), bg.mci_field_host(a, b)), name
        three, default = bg.block_field_levels(a, b, levels=3), bg.block_field_levels(a, b)
        assert len(three) == len(default) == 3
        for (x3, y3), (x, y) in zip(three, default):
            assert np.array_equal(x3, x) and np.array_equal(y3, y), name
    a, b = random_pair(h, w, 3)
    for bad in (2, 6):
        with pytest.raises(ValueError, match="levels"):
            bg.mci_field_host(a, b, levels=bad)
        with pytest.raises(ValueError, match="levels"):
            bg.block_field_levels(a, b, levels=bad)


# ---- pure translation ------------------------------------------------------------------------------------------------------------
# tests/test_background_cpu.py's argument with L levels: B is A shifted by 2 d; with d a multiple of 2^(L-1) in both components all
# L pyramids are shifted copies, the true candidate (d / 2^l on level l) costs exactly 0 wherever no sample is clamped and every
# other candidate pays the texture's SAD.  A level-0 block is exact when the (8 << (L-1))^2 pixels of its top-level ancestor,
# shifted by +d and by -d, lie inside the frame.
def guaranteed_levels(H, W, dx, dy, levels):
    """bool [Hb, Wb]: the blocks whose level-(levels-1) ancestor, shifted by +-d, lies inside the frame."""
    Hb, Wb = bg.field_shape(H, W)
    side = bg.BLOCK << (levels - 1)
    ys, xs = side * (np.arange(Hb) >> (levels - 1)), side * (np.arange(Wb) >> (levels - 1))
    oky = (ys - abs(dy) >= 0) & (ys + side - 1 + abs(dy) <= H - 1)
    okx = (xs - abs(dx) >= 0) & (xs + side - 1 + abs(dx) <= W - 1)
    return oky[:, None] & okx[None, :]


def _crops(H, W, seed):
    tex = texture(H + 2 * PAD, W + 2 * PAD, seed)
    return lambda oy, ox: np.ascontiguousarray(tex[PAD - oy:PAD - oy + H, PAD - ox:PAD - ox + W])


TRANSLATIONS = [(4, 256, 320, [(24, -16), (-32, 24), (0, 32), (-24, 0), (32, 32), (8, -8)], (0, 1, 2)),
                (5, 384, 448, [(48, -64), (-64, 32), (16, 0), (64, 64)], (0, 1))]


def test_guaranteed_levels_is_guaranteed_at_three():
    for H, W, dx, dy in ((96, 128, 12, -8), (67, 93, 4, 0), (256, 320, 24, -16)):
        assert np.array_equal(guaranteed_levels(H, W, dx, dy, 3), guaranteed(H, W, dx, dy))


@pytest.mark.parametrize("levels,H,W,shifts,seeds", TRANSLATIONS)
def test_pure_translation_beyond_the_default_range(levels, H, W, shifts, seeds):
    """Up to 64 px (four levels) and 128 px (five) between the key frames: the top-level winner on the ancestors, the raw
    level-0 field on every guaranteed block, the median-filtered field on the eroded set and the middle frame on the pixels that
    read only such blocks are exact, for every seed."""
    step = 1 << (levels - 1)
    for seed in seeds:
        crop = _crops(H, W, seed)
        for dx, dy in shifts:
            assert dx % step == 0 and dy % step == 0
            a, b, mid = crop(0, 0), crop(2 * dy, 2 * dx), crop(dy, dx)
            g = guaranteed_levels(H, W, dx, dy, levels)
            ge = eroded(g)
            assert ge.sum() >= 4, (H, W, dx, dy)
            fields = bg.block_field_levels(a, b, levels)
            assert len(fields) == levels
            anc = g[::step, ::step]
            assert anc.shape == fields[0][0].shape and anc.any()
            assert (fields[0][0][anc] * step == dx).all() and (fields[0][1][anc] * step == dy).all(), (seed, dx, dy)
            raw = np.stack(fields[-1], -1)
            assert (raw[g] == (dx, dy)).all(), (seed, dx, dy)
            f = bg.mci_field_host(a, b, levels)
            assert f.dtype == np.int16 and np.abs(f).max() <= bg.max_disp(levels)
            assert (f[ge] == (dx, dy)).all(), (seed, dx, dy)
            px = pixels_of(ge, H, W)
            out = bg.mci_frames_host(a, b, f, 2, [1])[0]
            assert px.sum() >= 256 and np.array_equal(out[px], mid[px]), (seed, dx, dy)


@pytest.mark.parametrize("dx,dy", [(24, -16), (32, 32)])
def test_three_levels_cannot_follow_that_motion(dx, dy):
    """48 x 32 px and 64 x 64 px between the key frames at 256 x 320: the default's field is wrong on more than half of the blocks
    it guarantees for motion inside its range (here: on all 768 of them, both times) - the blocks on which four levels are exact."""
    H, W = 256, 320
    crop = _crops(H, W, 0)
    a, b = crop(0, 0), crop(2 * dy, 2 * dx)
    g = guaranteed(H, W, dx, dy)
    raw = np.stack(bg.block_field_levels(a, b)[-1], -1)
    wrong = (raw[g] != (dx, dy)).any(-1)
    print("levels 3, d = (%d, %d): wrong on %d of %d guaranteed blocks" % (dx, dy, wrong.sum(), g.sum()))
    assert g.sum() >= 256 and wrong.mean() > 0.5
    g4 = guaranteed_levels(H, W, dx, dy, 4)
    assert g4.sum() >= 64 and (np.stack(bg.block_field_levels(a, b, 4)[-1], -1)[g4] == (dx, dy)).all()


# ---- the definition against loops ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(67, 93), (33, 15)])
def test_upper_pyramid_levels_and_costs_against_a_per_pixel_loop(H, W):
    a, b = texture(H, W, 7), texture(H, W, 8)
    pa, pb = bg.pyramid(bg.luma(a), 5), bg.pyramid(bg.luma(b), 5)
    shapes = [(H, W)]
    for _ in range(4):
        shapes.append(((shapes[-1][0] + 1) // 2, (shapes[-1][1] + 1) // 2))
    assert [p.shape for p in pa] == shapes and len(bg.pyramid(bg.luma(a), 4)) == 4
    assert all(np.array_equal(x, y) for x, y in zip(bg.pyramid(bg.luma(a), 4), pa)) and len(bg.pyramid(bg.luma(a))) == 3
    rng = np.random.default_rng(0)
    for lvl in (3, 4):
        src, dst = pa[lvl - 1].astype(int), pa[lvl]
        h, w = src.shape
        for y in range(dst.shape[0]):
            for x in range(dst.shape[1]):
                y1, x1 = min(2 * y + 1, h - 1), min(2 * x + 1, w - 1)
                assert dst[y, x] == (src[2 * y, 2 * x] + src[2 * y, x1] + src[y1, 2 * x] + src[y1, x1] + 2) >> 2
        ya, yb = pa[lvl], pb[lvl]
        h, w = ya.shape
        Hb, Wb = bg.field_shape(h, w)
        dx, dy = rng.integers(-5, 6, (Hb, Wb)), rng.integers(-5, 6, (Hb, Wb))
        cost = bg.block_cost(ya, yb, dx, dy)
        for by in range(Hb):
            for bx in range(Wb):
                c = bg.LAMBDA * (abs(int(dx[by, bx])) + abs(int(dy[by, bx])))
                for y in range(8 * by, min(8 * by + 8, h)):
                    for x in range(8 * bx, min(8 * bx + 8, w)):
                        va = ya[min(max(y - dy[by, bx], 0), h - 1), min(max(x - dx[by, bx], 0), w - 1)]
                        vb = yb[min(max(y + dy[by, bx], 0), h - 1), min(max(x + dx[by, bx], 0), w - 1)]
                        c += abs(int(va) - int(vb))
                assert cost[by, bx] == c
        # the full search of a top level, candidate by candidate: the minimum of the tuple
        sx = sy = np.zeros((Hb, Wb), np.int32)
        wx, wy = bg.search(ya, yb, sx, sy, bg.SEARCH_TOP, wide=True)
        nx, ny = bg.search(ya, yb, sx, sy, bg.SEARCH_TOP)
        assert np.array_equal(wx, nx) and np.array_equal(wy, ny)         # (either key: the same winner)
        for by in range(Hb):
            for bx in range(Wb):
                z = np.zeros((Hb, Wb), np.int64)
                best = min((int(bg.block_cost(ya, yb, z + ddx, z + ddy)[by, bx]), ddx * ddx + ddy * ddy, ddy, ddx)
                           for ddy in range(-4, 5) for ddx in range(-4, 5))
                assert (wx[by, bx], wy[by, bx]) == (best[3], best[2])


# ---- the wide key ------------------------------------------------------------------------------------------------------------------
def test_wide_key():
    assert [bg.max_disp(L) for L in (3, 4, 5)] == [19, 39, 79] and bg.max_disp(3) == bg.MAX_DISP
    for bad in (2, 6):
        with pytest.raises(ValueError):
            bg.max_disp(bad)
    top = (1 << 15) - 1
    assert 64 * 255 + bg.LAMBDA * 2 * bg.max_disp(5) <= top and 2 * bg.max_disp(5) ** 2 < 1 << 14 and bg.max_disp(5) < bg.WIDE_KEY_BIAS
    one = lambda v: np.full((1, 1), v, np.int64)
    for dx in (-79, 79):
        for dy in (-79, 79):
            k = bg.pack_key_wide(one(top), one(dx), one(dy))
            assert 0 <= int(k[0, 0]) < 1 << 45
            c, ux, uy = bg.unpack_key_wide(k)
            assert (int(c[0, 0]), int(ux[0, 0]), int(uy[0, 0])) == (top, dx, dy)
    rng = np.random.default_rng(5)
    n = 400
    cost = rng.integers(0, 4, n) * 5000 + rng.integers(0, 2, n)        # few distinct costs: the lower fields decide often
    dx, dy = rng.integers(-79, 80, n), rng.integers(-79, 80, n)
    dx[:40], dy[:40] = rng.integers(-2, 3, 40), rng.integers(-2, 3, 40)
    keys = bg.pack_key_wide(cost, dx, dy)
    tuples = [(int(c), int(x * x + y * y), int(y), int(x)) for c, x, y in zip(cost, dx, dy)]
    order = np.argsort(keys, kind="stable")
    assert [tuples[i] for i in order] == sorted(tuples)
    for i in range(0, n - 1):
        assert (keys[i] < keys[i + 1]) == (tuples[i] < tuples[i + 1]) and (keys[i] == keys[i + 1]) == (tuples[i] == tuples[i + 1])
    # the frames' fixed point holds the widest field at the largest rate in int32
    assert 2 * (bg.MAX_SAMPLE_RATE - 1) * (bg.max_disp(5) << bg.FIELD_FRAC_BITS) + bg.MAX_SAMPLE_RATE // 2 < 1 << 31


# ---- inputs of tests/test_gpu_mci_range.py ---------------------------------------------------------------------------------------
# (dx, dy) px between the key frames: about twice max_disp(levels), so that the field saturates in both signs of both components
WIDE_MOTIONS = {4: [(78, 0), (62, 62), (76, -78), (-62, -62)], 5: [(140, 0), (-140, 120), (0, -140), (100, 100)]}
WIDE_SIZES = [(96, 160), (67, 93)]
WIDE_TIE_KINDS = ("stripes16", "checker8", "diagonal16")
WIDE_TIE_SIZES = [(67, 93), (40, 56)]
ODD_SIZES = [(130, 250), (33, 15), (1, 1), (3, 5), (8, 8), (9, 33), (1, 40), (40, 1)]


def wide_pair(levels, h, w, i):
    dx, dy = WIDE_MOTIONS[levels][i]
    return moving_pair(h, w, dx, dy, 60 + i)


def tie_shares_levels(a, b, levels):
    """tests/test_background_cpu.py's tie_shares for `levels` levels, coarse to fine: the share of blocks whose minimal cost is
    reached by two or more candidates."""
    pa, pb = bg.pyramid(bg.luma(a), levels), bg.pyramid(bg.luma(b), levels)
    fields = bg.block_field_levels(a, b, levels)
    shares = []
    for i, lvl in enumerate(range(levels - 1, -1, -1)):
        Hb, Wb = bg.field_shape(*pa[lvl].shape)
        if i == 0:
            sx = sy = np.zeros((Hb, Wb), np.int32)
            radius = bg.SEARCH_TOP
        else:
            by, bx = np.arange(Hb) >> 1, np.arange(Wb) >> 1
            sx, sy = 2 * fields[i - 1][0][by][:, bx], 2 * fields[i - 1][1][by][:, bx]
            radius = bg.REFINE
        costs = np.stack([bg.block_cost(pa[lvl], pb[lvl], sx + ddx, sy + ddy)
                          for ddy in range(-radius, radius + 1) for ddx in range(-radius, radius + 1)])
        shares.append(float(((costs == costs.min(0)).sum(0) >= 2).mean()))
    return shares


def test_the_inputs_reach_the_widened_fields():
    h, w = WIDE_SIZES[0]
    for levels in (4, 5):
        top = bg.max_disp(levels)
        fields = [bg.mci_field_host(*wide_pair(levels, h, w, i), levels) for i in range(len(WIDE_MOTIONS[levels]))]
        for i, f in enumerate(fields):
            print("levels %d %-12s dx %d..%d dy %d..%d, share of a component >= 32: %.2f"
                  % (levels, WIDE_MOTIONS[levels][i], f[..., 0].min(), f[..., 0].max(), f[..., 1].min(), f[..., 1].max(), (np.abs(f).max(-1) >= 32).mean()))
        allf = np.stack(fields)
        assert np.abs(allf).max() == top > bg.KEY_BIAS                  # beyond what six bits hold
        for c in (0, 1):
            assert allf[..., c].min() == -top and allf[..., c].max() == top, (levels, c)
        assert max((np.abs(f).max(-1) >= 32).mean() for f in fields) >= 0.25
        # ... and with fewer levels the same inputs give other fields: the extra levels decide
        assert any(not np.array_equal(f, bg.mci_field_host(*wide_pair(levels, h, w, i), levels - 1)) for i, f in enumerate(fields))
    # ties on the new levels (3: the top of four levels, the second of five; 4: the top of five)
    h, w = WIDE_TIE_SIZES[0]
    shares = {(kind, levels): tie_shares_levels(*tie_pair(kind, h, w), levels) for kind in WIDE_TIE_KINDS for levels in (4, 5)}
    for key, s in shares.items():
        print("ties %-11s levels %d, coarse to fine: %s" % (key + (" ".join("%.2f" % v for v in s),)))
    for kind in WIDE_TIE_KINDS:
        assert shares[kind, 4][0] == 1.0, kind                          # level 3 as the top level: every block is a tie
        assert max(shares[kind, 5][:2]) == 1.0, kind                    # five levels: level 4 or level 3
    assert max(shares[kind, 5][0] for kind in WIDE_TIE_KINDS) >= 0.2 and max(shares[kind, 5][1] for kind in WIDE_TIE_KINDS) >= 0.2
    # sizes: frames smaller than one top-level block, pyramid levels of 1 x 1
    moved = 0
    for h, w in ODD_SIZES:
        a, b = random_pair(h, w, 1)
        for levels in (4, 5):
            f = bg.mci_field_host(a, b, levels)
            assert f.shape == bg.field_shape(h, w) + (2,)
            moved += bool(f.any())
    assert bg.pyramid(bg.luma(random_pair(9, 33, 1)[0]), 5)[4].shape == (1, 3) and bg.pyramid(bg.luma(random_pair(8, 8, 1)[0]), 5)[3].shape == (1, 1)
    assert moved >= 4


# ---- the driver ------------------------------------------------------------------------------------------------------------------
CLIPS = (("clipA", (48, 0), 70), ("clipB", (-40, 24), 71))          # (name, (dx, dy) px between the two key frames, seed)


def write_moving_clips(root, n_key=2, H=64, W=64):
    """Two clips of n_key key frames with one frame in between each two, no DAIN folder; a clip's key frames are crops of one
    texture 48 px (and 40 x 24 px) apart.  Returns {clip: [key frames]}."""
    from PIL import Image
    from tests.test_driver import _write_example
    import shutil
    keys = {}
    for name, (dx, dy), seed in CLIPS:
        _write_example(root, n_key=n_key, rate=2, H=H, W=W, clip=name, seed=seed)
        m = (n_key - 1) * max(abs(dx), abs(dy))
        tex = texture(H + 2 * m, W + 2 * m, seed)
        keys[name] = [np.ascontiguousarray(tex[m - k * dy:m - k * dy + H, m - k * dx:m - k * dx + W]) for k in range(n_key)]
        for k in range(n_key):
            Image.fromarray(keys[name][k]).save(os.path.join(root, "inputs", name, "%04d.png" % k))
    shutil.rmtree(os.path.join(root, "DAIN"))
    return keys


def _cfg64():
    import render_in_between_amd as rib
    from tests.test_driver import MID_CFG
    return rib.AttrDict(gen=rib.hsm_gen_config(**MID_CFG), model_height=64, model_width=64, gauss_sigma=5, skeleton_thres=0.001, foot_thres=0.001)


def test_driver_with_a_wider_range(tmp_path):
    import torch
    import render_in_between_amd as rib
    from render_in_between_amd import synth
    from oracle import generator_ref
    root = str(tmp_path)
    keys = write_moving_clips(root)
    for a, b in keys.values():                                          # the inputs: 32 and 64 px give other backgrounds
        assert not np.array_equal(bg.mci_field_host(a, b, 3), bg.mci_field_host(a, b, 4))
        f3, f4 = (bg.mci_frames_host(a, b, bg.mci_field_host(a, b, L), 2, [1]) for L in (3, 4))
        assert not np.array_equal(f3, f4)
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
    for name, kw in (("r64", dict(mci_range=64)), ("r32", dict(mci_range=32)), ("plain", {})):
        del calls[:]
        written = E.evaluate_from_folder(Model(), *dirs, os.path.join(root, name), background="mci", **kw)
        assert [os.path.relpath(x, os.path.join(root, name)) for x in written] == ["%s/f%03d.png" % (c, i) for c in ("clipA", "clipB") for i in range(3)]
        runs[name] = ([open(x, "rb").read() for x in written], list(calls))
        assert ("range %d px" % kw.get("mci_range", 32)) in importlib.import_module("render_in_between_amd.inference").summary_line(E)
    # range 64 feeds the model the four-level definition's frames
    assert len(runs["r64"][1]) == 2
    for got, name in zip(runs["r64"][1], keys):
        a, b = (E._decode_resized_u8(os.path.join(root, "inputs", name, "%04d.png" % k))[0] for k in range(2))
        assert np.array_equal(a, keys[name][0]) and np.array_equal(b, keys[name][1])
        want = bg.normalised_upload(bg.mci_frames_host(a, b, bg.mci_field_host(a, b, 4), 2, [1]))
        assert torch.equal(got[0], torch.from_numpy(want[0]))
    assert runs["r32"][0] == runs["plain"][0]                           # the default is range 32
    assert all(torch.equal(x, y) for x, y in zip(runs["r32"][1], runs["plain"][1]))
    for c in range(2):                                                  # the frame in between differs, the key frames pass through
        assert runs["r64"][0][3 * c + 1] != runs["r32"][0][3 * c + 1]
        assert runs["r64"][0][3 * c] == runs["r32"][0][3 * c] and runs["r64"][0][3 * c + 2] == runs["r32"][0][3 * c + 2]


def test_argument_errors(tmp_path):
    root = str(tmp_path)
    _example_without_dain(root, n_key=2, rate=2)
    cfg, model = _model()
    dirs = (os.path.join(root, "inputs"), None, os.path.join(root, "Predict_motion"), os.path.join(root, "out"))
    for bad in (48, 0, 256, "64", None):
        with pytest.raises(ValueError, match="mci_range must be"):
            ev.Evaluator(cfg, label_fn=oracle_labels).evaluate_from_folder(model, *dirs, background="mci", mci_range=bad)
    with pytest.raises(ValueError, match="setting of background='mci'"):
        ev.Evaluator(cfg, label_fn=oracle_labels).evaluate_from_folder(model, *dirs, mci_range=64)
    inf = importlib.import_module("render_in_between_amd.inference")
    assert inf.parse_args(["--input-dir", "x"]).mci_range == 32
    assert inf.parse_args(["--input-dir", "x", "--background", "mci"]).mci_range == 32
    for r in (32, 64, 128):
        assert inf.parse_args(["--input-dir", "x", "--background", "mci", "--mci-range", str(r)]).mci_range == r
    for bad in (["--mci-range", "64"], ["--background", "dain", "--mci-range", "32"], ["--background", "mci", "--mci-range", "48"],
                ["--background", "mci", "--mci-range", "wide"]):
        with pytest.raises(SystemExit):
            inf.parse_args(["--input-dir", "x"] + bad)
    text = " ".join(inf.build_parser().format_help().split())
    assert "--mci-range" in text and "32 (default), 64 or 128" in text and "38, 78 or 158" in text


def test_abi_is_declared_and_bound():
    from render_in_between_amd import _native
    hdr = open(os.path.join(ROOT, "include", "rib.h")).read()
    for name in ("rib_mci_workspace_bytes", "rib_mci_field"):                  # the entries that take `levels`
        assert name + "(" in hdr and name in _native.SIGNATURES
    assert "rib_mci_workspace_bytes(rib_handle* h, int B, int H, int W, int levels);" in hdr and "int levels, int border, void* workspace" in hdr
    assert len(_native.SIGNATURES["rib_mci_field"][1]) == 11 and len(_native.SIGNATURES["rib_mci_workspace_bytes"][1]) == 5
