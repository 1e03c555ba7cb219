"""The one-sided border mode of the interpolated backgrounds (no GPU): background.py's border="valid" - the driver's
mci_border - held to what the definition guarantees on pure translations (the field on EVERY block, the frames on every pixel
that has a valid sample), to per-pixel loops, to today's results under border="clamp", and the folder driver's
reference-protocol path on it.  The builders of tests/test_gpu_mci_border.py's inputs live here, with the conditions those
inputs must meet stated on the definition alone."""
import hashlib
import importlib
import os

import numpy as np
import pytest

from render_in_between_amd import background as bg, evaluator as ev
from tests.test_background_cpu import (TIE_KINDS, _example_without_dain, _model, moving_pair, random_pair, texture, tie_pair,
                                       wide_pair as strip_pair)
from tests.test_driver import oracle_labels
from tests.test_mci_range_cpu import WIDE_MOTIONS, _cfg64, guaranteed_levels, wide_pair, write_moving_clips

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAD = 160                                                               # texture margin: |2 d| <= 128


# ---- pure translation ------------------------------------------------------------------------------------------------------------
# tests/test_mci_range_cpu.py's scene: A = T(p), B = T(p - 2 d), the true frame k of s is T(p - 2 k d / s).  With d a multiple of
# 2^(L-1) all L pyramids are shifted copies, so on every level the true candidate has a SAD of exactly 0 over the pixels whose two
# samples are both inside the plane - border="valid" sums over no other pixel - and every other valid candidate pays the
# texture's SAD.  Where the plane is a whole number of 8 x 8 blocks on the top level and top-level |d| <= 4, the true candidate
# keeps n >= 4 * 8 = N / 2 pixels of every top-level block, so it is valid and wins; below, a block either has a valid start (the
# true vector, doubled: it wins again) or inherits it.  So the field is d on EVERY block, border blocks included.
TRANSLATIONS = {3: (160, 192, [(16, -16), (-16, 12)]),
                4: (256, 320, [(24, -16), (-32, 24), (0, 32), (32, 32)]),
                5: (384, 512, [(48, -64), (64, 64), (-64, 32)])}
SEEDS = (0, 1, 2, 3, 4)               # (seeds 0..24 were tried on all three rows: all 25 pass; DESIGN)
RATE = 8


def crops(H, W, seed):
    tex = texture(H + 2 * PAD, W + 2 * PAD, seed)
    return lambda oy, ox: np.ascontiguousarray(tex[PAD - oy:PAD - oy + H, PAD - ox:PAD - ox + W])


def translation_pair(H, W, dx, dy, seed):
    """(a, b): crops of one texture 2 d apart."""
    crop = crops(H, W, seed)
    return crop(0, 0), crop(2 * dy, 2 * dx)


def in_frame(H, W, oy, ox):
    """bool [H, W]: the pixels p with p + (oy, ox) inside the frame."""
    Y, X = np.mgrid[0:H, 0:W]
    return (Y + oy >= 0) & (Y + oy <= H - 1) & (X + ox >= 0) & (X + ox <= W - 1)


@pytest.mark.parametrize("levels", sorted(TRANSLATIONS))
def test_pure_translation_is_exact_up_to_the_border(levels):
    H, W, shifts = TRANSLATIONS[levels]
    step = 1 << (levels - 1)
    assert H % (bg.BLOCK * step) == 0 and W % (bg.BLOCK * step) == 0
    kept = 0
    for seed in SEEDS:
        crop = crops(H, W, seed)
        for dx, dy in shifts:
            assert dx % step == 0 and dy % step == 0 and max(abs(dx), abs(dy)) // step <= bg.SEARCH_TOP and dx % 4 == 0 and dy % 4 == 0
            a, b = crop(0, 0), crop(2 * dy, 2 * dx)
            raw = np.stack(bg.block_field_levels(a, b, levels, border="valid")[-1], -1)
            assert (raw == (dx, dy)).all(), (levels, seed, dx, dy, int((raw != (dx, dy)).any(-1).sum()))
            f = bg.mci_field_host(a, b, levels, border="valid")
            assert f.dtype == np.int16 and (f == (dx, dy)).all(), (levels, seed, dx, dy)
            # today's field is wrong on some border block of the same input
            clamp = np.stack(bg.block_field_levels(a, b, levels, border="clamp")[-1], -1)
            wrong = (clamp != (dx, dy)).any(-1)
            assert wrong[~guaranteed_levels(H, W, dx, dy, levels)].any(), (levels, seed, dx, dy)
            out = bg.mci_frames_host(a, b, f, RATE, range(1, RATE), border="valid")
            for k in range(1, RATE):
                oy, ox = 2 * k * dy // RATE, 2 * k * dx // RATE
                assert (oy * RATE, ox * RATE) == (2 * k * dy, 2 * k * dx)
                seen = in_frame(H, W, -oy, -ox) | in_frame(H, W, 2 * dy - oy, 2 * dx - ox)       # A's sample, B's sample
                assert (~seen).sum() * 10 < H * W, (levels, dx, dy, k, int((~seen).sum()))
                assert np.array_equal(out[k - 1][seen], crop(oy, ox)[seen]), (levels, seed, dx, dy, k)
            kept += 1
    assert kept == len(SEEDS) * len(shifts) and len(SEEDS) >= 5


def test_the_documented_limit_partial_top_level_blocks():
    """67 x 93 at L = 3: the top-level plane (17 x 24) is not a whole number of 8 x 8 blocks; a partial border block can have
    too few valid pairs at the true candidate and a wrong valid candidate wins.  border="valid" is then not exact - but wrong on
    no more blocks than border="clamp".  Measured, seeds 0..4, wrong blocks of 108, valid / clamp: d = (12, 0): 0 / 34-44;
    (-8, 0): 0 / 22-26; (4, 0): 0 / 10-13 (dy = 0: the partial block ROW is never short of pairs); (8, -8): 12 / 44-48;
    (-12, 12): 12 / 62-73 - the 12 are the last block row, whose level-2 ancestor is one pixel row high."""
    H, W = 67, 93
    total = [0, 0]
    for seed in SEEDS:
        for dx, dy in ((12, 0), (-8, 0), (4, 0), (8, -8), (-12, 12)):
            a, b = translation_pair(H, W, dx, dy, seed)
            wrong = [int((np.stack(bg.block_field_levels(a, b, 3, border=m)[-1], -1) != (dx, dy)).any(-1).sum()) for m in bg.BORDERS]
            print("67x93 seed %d d = (%d, %d): wrong blocks of 108, clamp %d, valid %d" % (seed, dx, dy, wrong[0], wrong[1]))
            assert wrong[1] <= wrong[0], (seed, dx, dy, wrong)
            total[0] += wrong[0]
            total[1] += wrong[1]
    assert 0 < total[1] < total[0]                                      # the limit is real, and the mode still helps


# ---- equalities with today's code --------------------------------------------------------------------------------------------------
# sha256 (first 16 hex digits) over the fields of every level, the median-filtered field and frames 0, 1, 3, 4 of s = 4, computed
# by background.py as it stood before `border` existed
BEFORE = {
    ("random", 3): "aafff10ae2e17ea3", ("random", 4): "275a1c1bd73d0de3", ("random", 5): "f228a12256f9c3c0",
    ("stripes16", 3): "5c36540b79fa4622", ("stripes16", 4): "366d1375f14ed15b", ("stripes16", 5): "81ac7a8dbe952c2c",
    ("checker8", 3): "4ec2f1c96197fc18", ("checker8", 4): "f6f40fa94d4abed9", ("checker8", 5): "67a37afeb120780d",
    ("checker8_low", 3): "e95afad04e183c7c", ("checker8_low", 4): "22eaf3ae045e7154", ("checker8_low", 5): "d8fb4a5b159f5976",
    ("stripes4", 3): "89e25a6a19d132d6", ("stripes4", 4): "66e62169b59abb55", ("stripes4", 5): "31226cc4e593f639",
    ("checker2", 3): "cf6d89cdeae6d50e", ("checker2", 4): "a11468825dc150c7", ("checker2", 5): "bde938f9aeafd94e",
    ("diagonal16", 3): "53dde95fbe1f733d", ("diagonal16", 4): "f0ddb24df20dc997", ("diagonal16", 5): "bdc841f97e8b95fe",
    ("antidiagonal16", 3): "4fbffce0d4042b06", ("antidiagonal16", 4): "efda70c365e68c53", ("antidiagonal16", 5): "d3b3095c07740eb4",
    ("flat", 3): "3b5d2a43c1e98c08", ("flat", 4): "e05b42f6b84f06bb", ("flat", 5): "476ee077c10fb21b",
}


def _existing_pairs():
    yield "random", random_pair(67, 93, 3)
    for kind in TIE_KINDS:
        yield kind, tie_pair(kind, 40, 56)
    yield "wide", strip_pair(5, 1030)


def _digest(a, b, levels, **kw):
    h = hashlib.sha256()
    for dx, dy in bg.block_field_levels(a, b, levels, **kw):
        h.update(np.ascontiguousarray(dx, dtype=np.int32).tobytes())
        h.update(np.ascontiguousarray(dy, dtype=np.int32).tobytes())
    f = bg.mci_field_host(a, b, levels, **kw)
    h.update(f.tobytes())
    h.update(bg.mci_frames_host(a, b, f, 4, [0, 1, 3, 4], **kw).tobytes())
    return h.hexdigest()[:16]


def test_clamp_is_today_byte_for_byte():
    for name, (a, b) in _existing_pairs():
        for levels in (3, 4, 5):
            d = _digest(a, b, levels, border="clamp")
            assert d == _digest(a, b, levels), (name, levels)          # the default is "clamp"
            if name != "wide":                                          # (a texture comes out of an FFT: not pinned by a digest)
                assert d == BEFORE[name, levels], (name, levels)
    a, b = random_pair(40, 56, 2)
    pa, pb = bg.pyramid(bg.luma(a)), bg.pyramid(bg.luma(b))
    z = np.zeros(bg.field_shape(*pa[2].shape), np.int32)
    for wide in (False, True):
        got, want = bg.search(pa[2], pb[2], z, z, 4, wide=wide, border="clamp"), bg.search(pa[2], pb[2], z, z, 4, wide=wide)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_valid_is_clamp_where_nothing_leaves_the_frame():
    a, b = random_pair(40, 56, 4)
    # frames: a field of zeros samples p itself in both key frames, for every k
    z = np.zeros(bg.field_shape(40, 56) + (2,), np.int16)
    ks = range(0, 9)
    assert np.array_equal(bg.mci_frames_host(a, b, z, 8, ks, border="valid"), bg.mci_frames_host(a, b, z, 8, ks))
    # zero motion: both modes find a field of zeros, and the frames are the key frame
    t = texture(64, 96, 1)
    for levels in (3, 5):
        f = bg.mci_field_host(t, t, levels, border="valid")
        assert not f.any() and np.array_equal(f, bg.mci_field_host(t, t, levels))
    assert all(np.array_equal(o, t) for o in bg.mci_frames_host(t, t, f, 4, range(5), border="valid"))
    # costs: where a candidate keeps all 64 pixels of a whole block, 64 * SAD // 64 is the SAD
    ya, yb = bg.luma(a), bg.luma(b)
    rng = np.random.default_rng(1)
    dx, dy = rng.integers(-5, 6, (5, 7)), rng.integers(-5, 6, (5, 7))
    cost, ok = bg.block_cost_valid(ya, yb, dx, dy)
    n, N = bg.valid_counts(40, 56, dx, dy)
    whole = n == 64
    assert whole[1:-1, 1:-1].all() and not whole.all() and ok[whole].all() and (N == 64).all()
    assert np.array_equal(cost[whole], bg.block_cost(ya, yb, dx, dy)[whole])
    # the end frames stay the key frames whatever the field
    a, b = wide_pair(5, 67, 93, 1)
    f = bg.mci_field_host(a, b, 5, border="valid")
    for s in (1, 8, 1024):
        ends = bg.mci_frames_host(a, b, f, s, [0, s], border="valid")
        assert np.array_equal(ends[0], a) and np.array_equal(ends[1], b)


# ---- the definition against loops ------------------------------------------------------------------------------------------------
def _loop_search(ya, yb, sx, sy, radius):
    """border="valid" as the text states it, pixel by pixel: ((dx, dy) per block, inherited mask, N per block, valid candidates
    per block, tied mask)."""
    h, w = ya.shape
    Hb, Wb = bg.field_shape(h, w)
    res = np.zeros((Hb, Wb, 2), np.int32)
    inherited, ties = np.zeros((Hb, Wb), bool), np.zeros((Hb, Wb), bool)
    Ns, nvalid = np.zeros((Hb, Wb), int), np.zeros((Hb, Wb), int)
    for by in range(Hb):
        for bx in range(Wb):
            pix = [(y, x) for y in range(8 * by, min(8 * by + 8, h)) for x in range(8 * bx, min(8 * bx + 8, w))]
            N = Ns[by, bx] = len(pix)

            def cand(dx, dy):
                both = [(y, x) for y, x in pix if 0 <= y - dy < h and 0 <= y + dy < h and 0 <= x - dx < w and 0 <= x + dx < w]
                if 4 * len(both) < N:
                    return None
                sad = sum(abs(int(ya[y - dy, x - dx]) - int(yb[y + dy, x + dx])) for y, x in both)
                return ((64 * sad) // len(both) + bg.LAMBDA * (abs(dx) + abs(dy)), dx * dx + dy * dy, dy, dx)
            s = (int(sx[by, bx]), int(sy[by, bx]))
            if cand(*s) is None:
                inherited[by, bx], res[by, bx] = True, s
                continue
            keys = [k for k in (cand(s[0] + ddx, s[1] + ddy) for ddy in range(-radius, radius + 1) for ddx in range(-radius, radius + 1))
                    if k is not None]
            best = min(keys)
            assert best[0] <= 64 * 255 + bg.LAMBDA * 2 * bg.max_disp(5) < 1 << 15
            nvalid[by, bx], ties[by, bx] = len(keys), sum(k[0] == best[0] for k in keys) >= 2
            res[by, bx] = (best[3], best[2])
    return res, inherited, Ns, nvalid, ties


def trace(a, b, levels):
    """block_field_levels(border="valid") level by level, coarse to fine, against the loop; returns the loop's masks."""
    pa, pb = bg.pyramid(bg.luma(a), levels), bg.pyramid(bg.luma(b), levels)
    fields = bg.block_field_levels(a, b, levels, border="valid")
    out = []
    for i, lvl in enumerate(range(levels - 1, -1, -1)):
        Hb, Wb = bg.field_shape(*pa[lvl].shape)
        if i == 0:
            sx = sy = np.zeros((Hb, Wb), np.int32)
            radius = bg.SEARCH_TOP
        else:
            by, bx = np.arange(Hb) >> 1, np.arange(Wb) >> 1
            sx, sy = 2 * fields[i - 1][0][by][:, bx], 2 * fields[i - 1][1][by][:, bx]
            radius = bg.REFINE
        res, inherited, N, nvalid, ties = _loop_search(pa[lvl], pb[lvl], sx, sy, radius)
        assert np.array_equal(res[..., 0], fields[i][0]) and np.array_equal(res[..., 1], fields[i][1]), (a.shape, levels, lvl)
        n0, N0 = bg.valid_counts(*pa[lvl].shape, sx, sy)
        assert np.array_equal(N0, N) and np.array_equal(4 * n0 < N0, inherited)
        out.append(dict(inherited=inherited, N=N, nvalid=nvalid, ties=ties))
    return out


INHERIT = (40, 56, 38, 0, 5)                                            # moving_pair(h, w, dx, dy, seed), three levels
ODD_SIZES = [(1, 1), (3, 5), (8, 8), (9, 33), (1, 40), (40, 1)]
BORDER_TIE_KINDS = ("stripes16", "stripes4", "checker2", "diagonal16", "antidiagonal16")


def test_rare_branches_against_a_per_pixel_loop():
    # inheritance: a 38 px pan in a 56 px frame - more than a quarter of the level-0 blocks have no valid start
    t = trace(*moving_pair(*INHERIT), 3)
    print("inherit: share per level, coarse to fine: %s" % " ".join("%.2f" % x["inherited"].mean() for x in t))
    assert not t[0]["inherited"].any() and t[2]["inherited"].mean() > 0.25 and t[1]["inherited"].any()
    # partial blocks (N < 64) on every level, next to whole ones
    t = trace(*translation_pair(67, 93, 8, -8, 0), 3)
    for x in t:
        assert (x["N"] < 64).any() and (x["N"] == 64).any()
    assert t[0]["N"].min() == 8 and sum(int(x["inherited"].sum()) for x in t) > 0      # 17 x 24: the last block row is one row high
    # every candidate but the start invalid: a 1 x 1 plane has room for d = 0 alone; and the sizes down to 1 x 1
    alone = moved = 0
    for h, w in ODD_SIZES:
        a, b = random_pair(h, w, 1)
        for levels in (3, 5):
            t = trace(a, b, levels)
            alone += sum(int((x["nvalid"] == 1).sum()) for x in t)
            f = bg.mci_field_host(a, b, levels, border="valid")
            assert f.shape == bg.field_shape(h, w) + (2,) and f.dtype == np.int16
            moved += bool(f.any())
            out = bg.mci_frames_host(a, b, f, 4, range(5), border="valid")
            assert np.array_equal(out[0], a) and np.array_equal(out[4], b)
    t = trace(*random_pair(1, 1, 1), 3)
    assert all(x["nvalid"].tolist() == [[1]] for x in t) and alone >= 10 and moved >= 4
    # ties under the normalised cost: on every level some pattern leaves a fifth of the blocks to the key's lower fields
    shares = {}
    for kind in BORDER_TIE_KINDS:
        t = trace(*tie_pair(kind, 64, 64), 3)
        shares[kind] = [float(x["ties"].mean()) for x in t]
        print("ties %-14s levels 2, 1, 0: %.2f %.2f %.2f" % ((kind,) + tuple(shares[kind])))
    for i in range(3):
        assert max(s[i] for s in shares.values()) >= 0.2, (i, shares)


def test_long_vectors_at_five_levels():
    """wide_pair (about 140 px between the key frames) at 96 x 160: vectors beyond the six-bit key, and much inheritance - where
    the coarse vector leaves the frame the finer levels keep it."""
    fields = [bg.mci_field_host(*wide_pair(5, 96, 160, i), 5, border="valid") for i in range(len(WIDE_MOTIONS[5]))]
    for (dx, dy), f in zip(WIDE_MOTIONS[5], fields):
        print("valid, levels 5 %-12s dx %d..%d dy %d..%d, share of a component >= 32: %.2f"
              % ((dx, dy), f[..., 0].min(), f[..., 0].max(), f[..., 1].min(), f[..., 1].max(), (np.abs(f).max(-1) >= 32).mean()))
    allf = np.stack(fields)
    assert bg.KEY_BIAS < np.abs(allf).max() <= bg.max_disp(5)
    assert max((np.abs(f).max(-1) >= 32).mean() for f in fields) >= 0.5
    pa = bg.pyramid(bg.luma(wide_pair(5, 96, 160, 0)[0]), 5)
    levels = bg.block_field_levels(*wide_pair(5, 96, 160, 0), 5, border="valid")
    n, N = bg.valid_counts(*pa[0].shape, *(2 * c[np.arange(12) >> 1][:, np.arange(20) >> 1] for c in levels[-2]))
    assert (4 * n < N).mean() > 0.25
    assert any(not np.array_equal(f, bg.mci_field_host(*wide_pair(5, 96, 160, i), 5)) for i, f in enumerate(fields))


def test_frames_take_the_one_valid_sample():
    """Pixel by pixel: a constant field that pushes one sample out of the frame on a strip."""
    H, W, s = 19, 27, 4
    a, b = random_pair(H, W, 6)
    f = np.zeros(bg.field_shape(H, W) + (2,), np.int16)
    f[..., 0], f[..., 1] = 5, -3
    ks = [0, 1, 2, 3, 4]
    got, clamp = bg.mci_frames_host(a, b, f, s, ks, border="valid"), bg.mci_frames_host(a, b, f, s, ks)
    one_sided = 0
    for j, k in enumerate(ks):
        for y in range(H):
            for x in range(W):
                ay, ax = y - (2 * k * -3) // s, x - (2 * k * 5) // s       # (2 k d / s is whole or a half: >> 2 of a multiple of 128)
                qa = (y * 256 - ((2 * k * -3 * 256 + 2) >> 2), x * 256 - ((2 * k * 5 * 256 + 2) >> 2))
                qb = (y * 256 + ((2 * (s - k) * -3 * 256 + 2) >> 2), x * 256 + ((2 * (s - k) * 5 * 256 + 2) >> 2))
                oka, okb = (0 <= qa[0] <= (H - 1) * 256 and 0 <= qa[1] <= (W - 1) * 256), (0 <= qb[0] <= (H - 1) * 256 and 0 <= qb[1] <= (W - 1) * 256)
                if oka == okb:
                    assert np.array_equal(got[j, y, x], clamp[j, y, x])
                else:
                    one_sided += 1
                    q, img = (qa, a) if oka else (qb, b)
                    want = bg.sample_bilinear(img, np.array([[q[0]]], np.int32), np.array([[q[1]]], np.int32))[0, 0]
                    assert np.array_equal(got[j, y, x], want), (k, y, x)
    assert one_sided > H * W // 2 and not np.array_equal(got, clamp)


# ---- inputs of tests/test_gpu_mci_border.py --------------------------------------------------------------------------------------
# the smallest multiples of 8 << (L-1) that still have interior and border blocks on every level; d as above
GPU_TRANSLATIONS = {3: (64, 96, [(12, -8), (-16, 12), (4, 16)]),
                    4: (128, 128, [(24, -16), (-32, 8), (0, 32)]),
                    5: (128, 256, [(48, -16), (-64, 32), (16, 0)])}
GPU_PARTIAL_SIZES = [(67, 93), (130, 250)]


def gpu_translation_pairs(levels):
    H, W, shifts = GPU_TRANSLATIONS[levels]
    return [translation_pair(H, W, dx, dy, 40 + i) for i, (dx, dy) in enumerate(shifts)]


def test_the_gpu_inputs_are_exact_and_differ_from_clamp():
    for levels, (H, W, shifts) in GPU_TRANSLATIONS.items():
        assert H % (8 << (levels - 1)) == 0 and W % (8 << (levels - 1)) == 0
        for (dx, dy), (a, b) in zip(shifts, gpu_translation_pairs(levels)):
            f = bg.mci_field_host(a, b, levels, border="valid")
            assert (f == (dx, dy)).all(), (levels, dx, dy)
            assert not np.array_equal(f, bg.mci_field_host(a, b, levels))
            assert not np.array_equal(bg.mci_frames_host(a, b, f, 8, [3], border="valid"), bg.mci_frames_host(a, b, f, 8, [3]))


# ---- the driver ------------------------------------------------------------------------------------------------------------------
def test_driver_with_the_valid_border(tmp_path):
    import torch
    import render_in_between_amd as rib
    from render_in_between_amd import synth
    from oracle import generator_ref
    root = str(tmp_path)
    keys = write_moving_clips(root)
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
    inf = importlib.import_module("render_in_between_amd.inference")
    runs = {}
    for name, kw in (("valid", dict(mci_border="valid")), ("clamp", dict(mci_border="clamp")), ("plain", {})):
        del calls[:]
        written = E.evaluate_from_folder(Model(), *dirs, os.path.join(root, name), background="mci", mci_range=64, **kw)
        runs[name] = ([open(x, "rb").read() for x in written], list(calls))
        assert ("range 64 px, border %s" % kw.get("mci_border", "clamp")) in inf.summary_line(E)
    assert len(runs["valid"][1]) == 2
    for got, name in zip(runs["valid"][1], keys):                       # the model is fed the definition's frames
        a, b = keys[name]
        want = bg.mci_frames_host(a, b, bg.mci_field_host(a, b, 4, border="valid"), 2, [1], border="valid")
        assert not np.array_equal(want, bg.mci_frames_host(a, b, bg.mci_field_host(a, b, 4), 2, [1]))
        assert torch.equal(got[0], torch.from_numpy(bg.normalised_upload(want)[0]))
    assert runs["clamp"][0] == runs["plain"][0]                         # the default is "clamp"
    assert all(torch.equal(x, y) for x, y in zip(runs["clamp"][1], runs["plain"][1]))
    for c in range(2):                                                  # the frame in between differs, the key frames pass through
        assert runs["valid"][0][3 * c + 1] != runs["clamp"][0][3 * c + 1]
        assert runs["valid"][0][3 * c] == runs["clamp"][0][3 * c] and runs["valid"][0][3 * c + 2] == runs["clamp"][0][3 * c + 2]


def test_argument_errors(tmp_path):
    a, b = random_pair(16, 24, 1)
    f = bg.mci_field_host(a, b)
    ya, yb = bg.luma(a), bg.luma(b)
    z = np.zeros(bg.field_shape(16, 24), np.int32)
    for bad in ("edge", "VALID", None, 1, True, b"valid", ""):
        for call in (lambda: bg.mci_field_host(a, b, 3, border=bad), lambda: bg.block_field_levels(a, b, 3, border=bad),
                     lambda: bg.search(ya, yb, z, z, 1, border=bad), lambda: bg.mci_frames_host(a, b, f, 2, [1], border=bad)):
            with pytest.raises(ValueError, match="border must be"):
                call()
    root = str(tmp_path)
    _example_without_dain(root, n_key=2, rate=2)
    cfg, model = _model()
    dirs = (os.path.join(root, "inputs"), None, os.path.join(root, "Predict_motion"), os.path.join(root, "out"))
    for bad in ("edge", "VALID", None, 1, True):
        with pytest.raises(ValueError, match="mci_border must be"):
            ev.Evaluator(cfg, label_fn=oracle_labels).evaluate_from_folder(model, *dirs, background="mci", mci_border=bad)
        with pytest.raises(ValueError, match="mci_border must be"):
            ev.Evaluator(cfg, label_fn=oracle_labels).evaluate_from_folder(model, *dirs, mci_border=bad)
    with pytest.raises(ValueError, match="mci_border is a setting of background='mci'"):
        ev.Evaluator(cfg, label_fn=oracle_labels).evaluate_from_folder(model, *dirs, mci_border="valid")
    inf = importlib.import_module("render_in_between_amd.inference")
    assert inf.parse_args(["--input-dir", "x"]).mci_border == "clamp"
    assert inf.parse_args(["--input-dir", "x", "--background", "mci"]).mci_border == "clamp"
    for m in ("clamp", "valid"):
        assert inf.parse_args(["--input-dir", "x", "--background", "mci", "--mci-range", "128", "--mci-border", m]).mci_border == m
    for bad in (["--mci-border", "valid"], ["--background", "dain", "--mci-border", "clamp"], ["--background", "mci", "--mci-border", "edge"]):
        with pytest.raises(SystemExit):
            inf.parse_args(["--input-dir", "x"] + bad)
    text = " ".join(inf.build_parser().format_help().split())
    assert "--mci-border" in text and "'clamp' (default)" in text and "no occlusion reasoning inside the frame" in text


def test_abi_is_declared_and_bound():
    from render_in_between_amd import _native
    hdr = open(os.path.join(ROOT, "include", "rib.h")).read()
    for name in ("rib_mci_field", "rib_mci_frames"):                           # the entries that take `border`
        assert name + "(" in hdr and name in _native.SIGNATURES
    assert "int levels, int border, void* workspace" in hdr and "int sample_rate, int k_first, int border, float* out_f32_nchw" in hdr
    assert len(_native.SIGNATURES["rib_mci_field"][1]) == 11 and len(_native.SIGNATURES["rib_mci_frames"][1]) == 14
