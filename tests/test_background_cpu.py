"""background.py, the integer definition of the motion-compensated background (background="mci"), and the folder driver's
reference-protocol path on it (no GPU).  Scenes: seeded band-limited random textures - two octaves of Gaussian-filtered noise,
sigma 8 px (it survives to pyramid level 2, whose Nyquist wavelength is 8 px) and sigma 2.5 px (detail inside an 8x8 block)."""
import os
import re
import socket

import numpy as np
import pytest
import torch

import render_in_between_amd as rib
from render_in_between_amd import background as bg, evaluator as ev, synth
from oracle import generator_ref
from tests.test_driver import MID_CFG, _write_example, oracle_labels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def texture(h, w, seed, sigmas=(8.0, 2.5), amps=(1.0, 0.4)):
    rng = np.random.default_rng(seed)
    fy, fx = np.fft.fftfreq(h)[:, None], np.fft.fftfreq(w)[None, :]
    t = 0
    for sigma, amp in zip(sigmas, amps):
        g = np.exp(-2 * (np.pi * sigma) ** 2 * (fy * fy + fx * fx))
        band = np.real(np.fft.ifft2(np.fft.fft2(rng.standard_normal((h, w, 3)), axes=(0, 1)) * g[..., None], axes=(0, 1)))
        t = t + amp * band / band.std()
    return np.clip(128 + 40 * t, 0, 255).astype(np.uint8)


def test_equal_key_frames_give_a_zero_field_and_the_key_frame():
    a = texture(40, 56, 1)
    f = bg.mci_field_host(a, a)
    assert f.dtype == np.int16 and f.shape == (5, 7, 2) == bg.field_shape(40, 56) + (2,) and not f.any()
    for s in (2, 4, 8):
        out = bg.mci_frames_host(a, a, f, s, range(0, s + 1))
        assert out.shape == (s + 1, 40, 56, 3) and all(np.array_equal(o, a) for o in out)


def test_flat_pair_takes_the_zero_displacement():
    """Every candidate of a flat pair costs LAMBDA * (|dx| + |dy|) and nothing else: the tuple's minimum is d = 0; with
    LAMBDA's term taken away the tie-break (dx*dx + dy*dy first) still picks it."""
    a, b = np.full((41, 57, 3), 90, np.uint8), np.full((41, 57, 3), 200, np.uint8)
    assert not bg.mci_field_host(a, b).any()
    z = np.zeros((2, 2), np.int32)
    k = [bg.pack_key(z + 7, z + dx, z + dy)[0, 0] for dy in (-1, 0, 1) for dx in (-1, 0, 1)]
    assert int(np.argmin(k)) == 4 and len(set(k)) == 9
    assert bg.pack_key(z + 7, z - 1, z + 1)[0, 0] < bg.pack_key(z + 7, z + 1, z + 1)[0, 0] < bg.pack_key(z + 8, z, z)[0, 0]


# ---- pure translation ---------------------------------------------------------------------------------------------------------
# What the definition GUARANTEES, and what the tests therefore assert on several seeds.  B is A shifted by (2 dx, 2 dy).  The
# pyramid halves a shift exactly when it is even, so with d = (dx, dy) a multiple of 4 in both components the two pyramids are
# shifted copies of each other on every level and the true candidate (d/4 at level 2, d/2 at level 1, d at level 0 - the centre
# of each refinement) has a SAD of exactly 0 wherever no sample is clamped; every other candidate pays the texture's SAD, far
# above LAMBDA's term.  A level-0 block is therefore exact when the 32 x 32 pixels of its level-2 ancestor, shifted by +d and
# by -d, lie inside the frame (its level-1 ancestor and the block itself then do too); the median keeps it when its eight
# neighbours are such blocks as well, and a pixel of the middle frame is exact when its four nearest block centres are.  For
# the issue's |.| <= 12 that is "at least four blocks from the border" (the footprint of a level-2 border block) wherever the
# frame has a whole level-2 block to spare - which at 67 x 93 (two whole level-2 block rows, 64 of 67 rows) holds for dy = 0.
# A d that is no multiple of 4 is sub-pel on the coarse levels: no candidate matches there, the winner is the nearer one in
# most blocks but not provably (measured: DESIGN), so such shifts are not asserted block by block.
SHIFTS = [(12, -8), (-12, 12), (0, -12), (8, 4), (-4, 0)]         # |.| <= 12, negative and zero components, level-2 winners up to +-3
SHIFTS_67 = [(12, 0), (-8, 0), (4, 0)]
SEEDS = [0, 1, 2, 3, 4]


def guaranteed(H, W, dx, dy):
    """bool [Hb, Wb]: the blocks whose level-2 ancestor, shifted by +-d, lies inside the frame."""
    Hb, Wb = bg.field_shape(H, W)
    ys, xs = 32 * (np.arange(Hb) >> 2), 32 * (np.arange(Wb) >> 2)
    oky = (ys - abs(dy) >= 0) & (ys + 31 + abs(dy) <= H - 1)
    okx = (xs - abs(dx) >= 0) & (xs + 31 + abs(dx) <= W - 1)
    return oky[:, None] & okx[None, :]


def eroded(g):
    p = np.pad(g, 1, mode="constant")
    return np.logical_and.reduce([p[j:j + g.shape[0], i:i + g.shape[1]] for j in range(3) for i in range(3)])


def pixels_of(g, H, W):
    """bool [H, W]: the pixels whose four nearest block centres (background.pixel_field) are all blocks of g."""
    Hb, Wb = g.shape
    ty, tx = 2 * np.arange(H) - 7, 2 * np.arange(W) - 7
    r0, r1 = np.clip(ty >> 4, 0, Hb - 1), np.clip((ty >> 4) + 1, 0, Hb - 1)
    c0, c1 = np.clip(tx >> 4, 0, Wb - 1), np.clip((tx >> 4) + 1, 0, Wb - 1)
    return g[r0][:, c0] & g[r0][:, c1] & g[r1][:, c0] & g[r1][:, c1]


@pytest.mark.parametrize("H,W,shifts", [(96, 128, SHIFTS), (67, 93, SHIFTS_67), (160, 192, SHIFTS + [(16, -16)])])
def test_pure_translation(H, W, shifts):
    """The level-0 field before the median is (dx, dy) on every guaranteed block, the median-filtered field on every guaranteed
    block whose neighbours are guaranteed, and the middle frame is A shifted by (dx, dy), exactly, on the pixels that read only
    such blocks - for every seed, including level-2 winners of +-3 and (at 160 x 192) +-4, the edge of the search."""
    for seed in SEEDS:
        tex = texture(H + 64, W + 64, seed)
        crop = lambda oy, ox: np.ascontiguousarray(tex[32 - oy:32 - oy + H, 32 - ox:32 - ox + W])
        for dx, dy in shifts:
            a, b, mid = crop(0, 0), crop(2 * dy, 2 * dx), crop(dy, dx)
            g = guaranteed(H, W, dx, dy)
            ge = eroded(g)
            assert ge.sum() >= 4, (H, W, dx, dy)                        # (never a vacuous case)
            levels = bg.block_field_levels(a, b)
            anc = g[::4, ::4]                                           # the level-2 blocks above the guaranteed ones: d / 4
            assert (levels[0][0][anc] * 4 == dx).all() and (levels[0][1][anc] * 4 == dy).all(), (seed, dx, dy)
            raw = np.stack(levels[-1], -1)
            assert (raw[g] == (dx, dy)).all(), (seed, dx, dy, raw[g].tolist())
            f = bg.mci_field_host(a, b)
            assert (f[ge] == (dx, dy)).all(), (seed, dx, dy, f[ge].tolist())
            px = pixels_of(ge, H, W)
            out = bg.mci_frames_host(a, b, f, 2, [1])[0]
            assert px.sum() >= 256 and np.array_equal(out[px], mid[px]), (seed, dx, dy)


def test_level_2_search_reaches_its_edge():
    """d = (16, -16): the level-2 winner is (4, -4), the corner of the full search, i.e. 32 px of motion between the key frames;
    the packed key holds the largest displacement the refinements can reach (MAX_DISP = 19 < KEY_BIAS)."""
    H, W, dx, dy = 160, 192, 16, -16
    tex = texture(H + 64, W + 64, 1)
    a = np.ascontiguousarray(tex[32:32 + H, 32:32 + W])
    b = np.ascontiguousarray(tex[32 - 2 * dy:32 - 2 * dy + H, 32 - 2 * dx:32 - 2 * dx + W])
    l2x, l2y = bg.block_field_levels(a, b)[0]
    assert (l2x[1:-1, 1:-1] == 4).all() and (l2y[1:-1, 1:-1] == -4).all()
    z = np.zeros((1, 1), np.int32)
    for d in (-bg.MAX_DISP, bg.MAX_DISP):
        k = bg.pack_key(z + 5, z + d, z - d)
        assert ((k & 63) - bg.KEY_BIAS == d).all() and (((k >> 6) & 63) - bg.KEY_BIAS == -d).all() and (k >> 22 == 5).all()
    assert bg.MAX_DISP == 19 < bg.KEY_BIAS and 2 * bg.MAX_DISP ** 2 < 1 << 10


def psnr(x, y):
    return 10 * np.log10(255.0 ** 2 / np.mean((x.astype(np.float64) - y.astype(np.float64)) ** 2))


def test_moving_patch_beats_the_cross_fade():
    """A 32x32 patch moving by (12, 8) over a static texture: the middle frame is nearer to the true middle frame than the
    plain cross-fade (A + B + 1) >> 1 is (the values are in DESIGN)."""
    H, W = 96, 128
    back, patch = texture(H, W, 5), texture(32, 32, 6, sigmas=(4.0, 1.5))
    frames = []
    for k in range(3):
        f = back.copy()
        f[24 + 4 * k:56 + 4 * k, 40 + 6 * k:72 + 6 * k] = patch
        frames.append(f)
    a, true_mid, b = frames
    out = bg.mci_frames_host(a, b, bg.mci_field_host(a, b), 2, [1])[0]
    fade = ((a.astype(np.int32) + b + 1) >> 1).astype(np.uint8)
    p_mci, p_fade = psnr(out, true_mid), psnr(fade, true_mid)
    print("moving patch: MCI %.2f dB, cross-fade %.2f dB" % (p_mci, p_fade))
    assert p_mci > p_fade


@pytest.mark.parametrize("H,W", [(40, 56), (41, 57)])
def test_pyramid_and_costs_against_a_per_pixel_loop(H, W):
    """The vectorised luma, pyramid, block cost, median and per-pixel field against loops that restate the definition."""
    a, b = texture(H, W, 7), texture(H, W, 8)
    ya = bg.luma(a)
    pyr = bg.pyramid(ya)
    assert [p.shape for p in pyr] == [(H, W), ((H + 1) // 2, (W + 1) // 2), (((H + 1) // 2 + 1) // 2, ((W + 1) // 2 + 1) // 2)]
    for y in range(H):
        for x in range(W):
            r, g, bl = (int(v) for v in a[y, x])
            assert ya[y, x] == (77 * r + 150 * g + 29 * bl + 128) >> 8
    for lvl in (1, 2):
        src, dst = pyr[lvl - 1].astype(int), pyr[lvl]
        h, w = src.shape
        for y in range(dst.shape[0]):
            for x in range(dst.shape[1]):
                y1, x1 = min(2 * y + 1, h - 1), min(2 * x + 1, w - 1)
                assert dst[y, x] == (src[2 * y, 2 * x] + src[2 * y, x1] + src[y1, 2 * x] + src[y1, x1] + 2) >> 2
    yb = bg.luma(b)
    Hb, Wb = bg.field_shape(H, W)
    rng = np.random.default_rng(0)
    dx, dy = rng.integers(-5, 6, (Hb, Wb)), rng.integers(-5, 6, (Hb, Wb))
    cost = bg.block_cost(ya, yb, dx, dy)
    for by in range(Hb):
        for bx in range(Wb):
            c = bg.LAMBDA * (abs(int(dx[by, bx])) + abs(int(dy[by, bx])))
            for y in range(8 * by, min(8 * by + 8, H)):
                for x in range(8 * bx, min(8 * bx + 8, W)):
                    pa = ya[min(max(y - dy[by, bx], 0), H - 1), min(max(x - dx[by, bx], 0), W - 1)]
                    pb = yb[min(max(y + dy[by, bx], 0), H - 1), min(max(x + dx[by, bx], 0), W - 1)]
                    c += abs(int(pa) - int(pb))
            assert cost[by, bx] == c
    med = bg.median3(dx)
    for by in range(Hb):
        for bx in range(Wb):
            nine = sorted(int(dx[min(max(by + j, 0), Hb - 1), min(max(bx + i, 0), Wb - 1)]) for j in (-1, 0, 1) for i in (-1, 0, 1))
            assert med[by, bx] == nine[4]
    field = np.stack([dx, dy], -1).astype(np.int16)
    Dx, _ = bg.pixel_field(field, H, W)
    for y in (0, 3, 4, H // 2, H - 1):
        for x in range(W):
            ty, tx = 2 * y - 7, 2 * x - 7
            r0, c0, fy, fx = ty // 16, tx // 16, ty % 16, tx % 16
            g = lambda r, c: int(dx[min(max(r, 0), Hb - 1), min(max(c, 0), Wb - 1)])
            assert Dx[y, x] == (16 - fy) * ((16 - fx) * g(r0, c0) + fx * g(r0, c0 + 1)) + fy * ((16 - fx) * g(r0 + 1, c0) + fx * g(r0 + 1, c0 + 1))
    # one frame, pixel by pixel
    s, k = 4, 1
    out = bg.mci_frames_host(a, b, field, s, [k])[0]
    Dx, Dy = bg.pixel_field(field, H, W)

    def tap(img, py, px, c):
        y0, x0, fy, fx = py >> 8, px >> 8, py & 255, px & 255
        v = lambda yy, xx: int(img[min(max(yy, 0), H - 1), min(max(xx, 0), W - 1), c])
        return ((256 - fy) * ((256 - fx) * v(y0, x0) + fx * v(y0, x0 + 1)) + fy * ((256 - fx) * v(y0 + 1, x0) + fx * v(y0 + 1, x0 + 1)) + 32768) >> 16
    for y in range(0, H, 5):
        for x in range(W):
            ax, ay = (2 * k * int(Dx[y, x]) + 2) >> 2, (2 * k * int(Dy[y, x]) + 2) >> 2
            bx, by = (2 * (s - k) * int(Dx[y, x]) + 2) >> 2, (2 * (s - k) * int(Dy[y, x]) + 2) >> 2
            for c in range(3):
                va, vb = tap(a, (y << 8) - ay, (x << 8) - ax, c), tap(b, (y << 8) + by, (x << 8) + bx, c)
                assert out[y, x, c] == ((s - k) * va + k * vb + 2) >> 2


def test_320x480_pair_on_the_host():
    """The host definition is vectorised: a 320x480 pair with seven frames takes well under a second here; the time is printed
    and only a bound no loaded host should miss is asserted."""
    import time
    a, b = texture(320, 480, 3), texture(320, 480, 4)
    t0 = time.perf_counter()
    bg.mci_frames_host(a, b, bg.mci_field_host(a, b), 8, range(1, 8))
    dt = time.perf_counter() - t0
    print("320x480 field + 7 frames on the host: %.2f s" % dt)
    assert dt < 60.0


# ---- inputs for the rare branches (tests/test_gpu_mci_edges.py runs the kernels on them) ----------------------------------------
# Smooth textures almost never give two candidates one cost, move by a few pixels and are a few blocks large; the kernels'
# tie order, their 6-bit displacement fields and far-clamped windows, their loops' second passes and their clamps on frames
# smaller than a tile then never decide a result.  These builders make inputs on which they do, and
# test_the_inputs_reach_the_rare_branches holds the builders to that with the definition alone.
TIE_KINDS = ("stripes16", "checker8", "checker8_low", "stripes4", "checker2", "diagonal16", "antidiagonal16", "flat")
TIE_SIZES = [(67, 93), (40, 56)]
LONG_MOTIONS = [(38, 0), (-38, 36), (0, -38), (30, 30)]          # (dx, dy) px between the key frames; 38 is outside the +-32 px search
LONG_SIZES = [(96, 160), (67, 93)]
WIDE_SIZES = [(8, 2056), (5, 1030), (16, 4100)]                  # W > 1024: the strip loop's second pass; W % 4 = 0, 2, 0
TINY_SIZES = [(1, 1), (3, 5), (7, 9), (8, 8), (9, 33), (31, 17), (33, 15), (1, 40), (40, 1)]


def _grey(plane):
    return np.ascontiguousarray(np.repeat(np.asarray(plane, np.uint8)[..., None], 3, 2))


def tie_pair(kind, h, w):
    """A periodic pattern and the same pattern shifted by half a period: many displacements match equally well."""
    Y, X = np.mgrid[0:h, 0:w]
    if kind == "stripes16":
        f = lambda o: ((X + o) % 16 < 8) * 255
        return _grey(f(0)), _grey(f(8))
    if kind in ("checker8", "checker8_low"):
        lo, hi = (0, 255) if kind == "checker8" else (100, 106)
        f = lambda o: np.where((((X + o) >> 3) + (Y >> 3)) & 1, hi, lo)
        return _grey(f(0)), _grey(f(8))
    if kind == "stripes4":
        f = lambda o: ((X + o) % 4 < 2) * 255
        return _grey(f(0)), _grey(f(2))
    if kind == "checker2":
        f = lambda o: ((((X + o) >> 1) + (Y >> 1)) & 1) * 255
        return _grey(f(0)), _grey(f(2))
    if kind == "diagonal16":
        f = lambda o: ((X + Y + o) % 16 < 8) * 200
        return _grey(f(0)), _grey(f(8))
    if kind == "antidiagonal16":
        f = lambda o: ((X - Y + o) % 16 < 8) * 200
        return _grey(f(0)), _grey(f(8))
    if kind == "flat":
        return np.full((h, w, 3), 90, np.uint8), np.full((h, w, 3), 200, np.uint8)
    raise ValueError(kind)


def tie_shares(a, b):
    """Per level (2, 1, 0): the share of blocks whose minimal cost is reached by two or more candidates, so that the lower
    fields of the packed key decide the winner.  The candidates are those of block_field_levels."""
    pa, pb = bg.pyramid(bg.luma(a)), bg.pyramid(bg.luma(b))
    levels = bg.block_field_levels(a, b)
    shares = []
    for i, lvl in enumerate(range(bg.LEVELS - 1, -1, -1)):
        Hb, Wb = bg.field_shape(*pa[lvl].shape)
        if i == 0:
            sx = sy = np.zeros((Hb, Wb), np.int32)
            radius = bg.SEARCH_TOP
        else:
            by, bx = np.arange(Hb) >> 1, np.arange(Wb) >> 1
            sx, sy = 2 * levels[i - 1][0][by][:, bx], 2 * levels[i - 1][1][by][:, bx]
            radius = bg.REFINE
        costs = np.stack([bg.block_cost(pa[lvl], pb[lvl], sx + ddx, sy + ddy)
                          for ddy in range(-radius, radius + 1) for ddx in range(-radius, radius + 1)])
        shares.append(float(((costs == costs.min(0)).sum(0) >= 2).mean()))
    return shares


def last_candidate_shares(a, b):
    """Levels 1 and 0: the share of blocks won by start + (1, 1), the last of the nine candidates - in k_mci_search<1> the only
    one whose lanes lie in the wave's upper half."""
    levels = bg.block_field_levels(a, b)
    shares = []
    for i in (1, 2):
        (dx, dy), (cx, cy) = levels[i], levels[i - 1]
        by, bx = np.arange(dx.shape[0]) >> 1, np.arange(dx.shape[1]) >> 1
        shares.append(float(((dx - 2 * cx[by][:, bx] == 1) & (dy - 2 * cy[by][:, bx] == 1)).mean()))
    return shares


def moving_pair(h, w, dx, dy, seed):
    """Two crops of one smooth texture, the second displaced by (dx, dy) px."""
    m = max(abs(dx), abs(dy), 1)
    tex = texture(h + 2 * m, w + 2 * m, seed)
    a = tex[m:m + h, m:m + w]
    b = tex[m - dy:m - dy + h, m - dx:m - dx + w]
    return np.ascontiguousarray(a), np.ascontiguousarray(b)


def long_pair(h, w, i):
    dx, dy = LONG_MOTIONS[i]
    return moving_pair(h, w, dx, dy, 20 + i)


def wide_pair(h, w):
    return moving_pair(h, w, 10, -2, 30 + h)


def random_pair(h, w, seed):
    """Unrelated random content in A and B."""
    rng = np.random.default_rng([seed, h, w])
    return rng.integers(0, 256, (h, w, 3), dtype=np.uint8), rng.integers(0, 256, (h, w, 3), dtype=np.uint8)


def test_the_inputs_reach_the_rare_branches():
    # ties: every level has an input on which a fifth of the blocks or more are decided by the key's lower fields
    h, w = TIE_SIZES[0]
    shares = {}
    for kind in TIE_KINDS:
        a, b = tie_pair(kind, h, w)
        assert a.shape == b.shape == (h, w, 3) and a.dtype == b.dtype == np.uint8
        shares[kind] = tie_shares(a, b)
        print("ties %-14s levels 2, 1, 0: %.2f %.2f %.2f" % ((kind,) + tuple(shares[kind])))
        if kind == "flat":                                              # LAMBDA's term makes d = 0 unique
            assert shares[kind] == [0.0, 0.0, 0.0] and not bg.mci_field_host(a, b).any()
    for i in range(bg.LEVELS):
        assert max(s[i] for s in shares.values()) >= 0.2, (i, shares)
    for kind in ("stripes16", "checker8", "checker8_low"):
        assert shares[kind][0] == 1.0, (kind, shares[kind])
    assert any(bg.mci_field_host(*tie_pair(kind, h, w)).any() for kind in TIE_KINDS)
    # ... and on one of them the last candidate wins a fifth of the blocks of levels 1 and 0 (on the others it never wins)
    last = last_candidate_shares(*tie_pair("antidiagonal16", h, w))
    print("ties antidiagonal16: start + (1, 1) wins %.2f %.2f of the blocks of levels 1, 0" % tuple(last))
    assert min(last) >= 0.2 and min(shares["antidiagonal16"]) >= 0.2
    # long vectors: both signs of the largest displacement in both components, and many blocks near it
    h, w = LONG_SIZES[0]
    fields = [bg.mci_field_host(*long_pair(h, w, i)) for i in range(len(LONG_MOTIONS))]
    for i, f in enumerate(fields):
        print("long %-10s dx %d..%d dy %d..%d, share of |d| >= 16: %.2f"
              % (LONG_MOTIONS[i], f[..., 0].min(), f[..., 0].max(), f[..., 1].min(), f[..., 1].max(), (np.abs(f).max(-1) >= 16).mean()))
    allf = np.stack(fields)
    assert np.abs(allf).max() == bg.MAX_DISP
    for c in (0, 1):
        assert allf[..., c].min() == -bg.MAX_DISP and allf[..., c].max() == bg.MAX_DISP, c
    assert (np.abs(allf).max(-1) >= 16).mean() >= 0.2
    # sizes: the field shapes, and a tiny frame whose field is not zero
    moved = 0
    for h, w in TINY_SIZES + WIDE_SIZES:
        a, b = random_pair(h, w, 1) if (h, w) in TINY_SIZES else wide_pair(h, w)
        f = bg.mci_field_host(a, b)
        assert f.shape == bg.field_shape(h, w) + (2,) == ((h + 7) // 8, (w + 7) // 8, 2)
        moved += bool(f.any()) and (h, w) in TINY_SIZES
    assert moved >= 1


# ---- the driver -----------------------------------------------------------------------------------------------------------------
def _cfg():
    return rib.AttrDict(gen=rib.hsm_gen_config(**MID_CFG), model_height=32, model_width=48, gauss_sigma=5,
                        skeleton_thres=0.001, foot_thres=0.001)


def _model(calls=None):
    cfg = _cfg()
    spec = rib.GenSpec.from_cfg(cfg.gen)
    R = generator_ref.RefGenerator(spec, synth.make_state_dict(spec, 2))

    class Model:                               # the reference's object protocol (tests/test_driver.py)
        def eval(self):
            return self

        def __call__(self, label, label_prev, dain, prev):
            if calls is not None:
                calls.append(dain.clone())
            return R(label, label_prev, dain, prev)
    return cfg, Model()


def _example_without_dain(root, **kw):
    import shutil
    n = _write_example(root, **kw)
    shutil.rmtree(os.path.join(root, "DAIN"))
    return n


def test_driver_end_to_end_without_a_dain_folder(tmp_path):
    from PIL import Image
    root = str(tmp_path)
    n = _example_without_dain(root, n_key=3, rate=4)
    calls = []
    cfg, model = _model(calls)
    E = ev.Evaluator(cfg, label_fn=oracle_labels)
    out = os.path.join(root, "out")
    written = E.evaluate_from_folder(model, os.path.join(root, "inputs"), None, os.path.join(root, "Predict_motion"), out, background="mci")
    assert n == 9 and [os.path.basename(w) for w in written] == ["f%03d.png" % i for i in range(9)]      # the pose files' stems
    assert sorted(os.listdir(os.path.join(out, "clipA"))) == ["f%03d.png" % i for i in range(9)]
    keys = [E._decode_resized_u8(os.path.join(root, "inputs", "clipA", "%04d.png" % k))[0] for k in range(3)]
    for k in range(3):                         # key frames pass through
        key, _ = E.load_image(os.path.join(root, "inputs", "clipA", "%04d.png" % k))
        assert np.array_equal(np.asarray(Image.open(written[4 * k])), generator_ref.quantise_uint8(key.unsqueeze(0)))
    want = []
    for k in range(2):
        u8 = bg.mci_frames_host(keys[k], keys[k + 1], bg.mci_field_host(keys[k], keys[k + 1]), 4, [1, 2, 3])
        want += list(bg.normalised_upload(u8))           # the floats the native chain reads
    assert len(calls) == 6
    for got, w in zip(calls, want):
        assert torch.equal(got[0], torch.from_numpy(w))
    assert "background mci" in __import__("importlib").import_module("render_in_between_amd.inference").summary_line(E)


def test_metrics_measure_the_interpolated_background(tmp_path):
    """--metrics under background="mci": the DAIN_* values are those of the MCI frames the model was fed, the keys keep their
    names and metrics.json says which background was measured."""
    import json
    from PIL import Image
    from render_in_between_amd import metrics as M
    root = str(tmp_path)
    n = _example_without_dain(root, n_key=2, rate=4)
    rng = np.random.default_rng(3)
    os.makedirs(os.path.join(root, "gt", "clipA"))
    for i in range(n):
        Image.fromarray(rng.integers(0, 255, (32, 48, 3), dtype=np.uint8)).save(os.path.join(root, "gt", "clipA", "g%03d.png" % i))
    cfg, model = _model()
    E = ev.Evaluator(cfg, label_fn=oracle_labels)
    out = os.path.join(root, "out")
    E.evaluate_from_folder(model, os.path.join(root, "inputs"), None, os.path.join(root, "Predict_motion"), out,
                           gt_dir=os.path.join(root, "gt"), metrics=True, background="mci")
    rep = json.load(open(os.path.join(out, "metrics.json")))
    assert rep["background"] == "mci" and rep == json.loads(json.dumps(E.metrics_report))
    per = rep["clips"]["clipA"]["per_frame"]
    assert [r["i"] for r in per] == [1, 2, 3] and {"DAIN_PSNR", "DAIN_SSIM", "OURS_PSNR", "OURS_SSIM"} <= set(per[0])
    # with a gt_dir the key frames are gt_dir's frames 0 and 4 (evaluator.py:209-212)
    ka, kb = (E._decode_resized_u8(os.path.join(root, "gt", "clipA", "g%03d.png" % i))[0] for i in (0, 4))
    u8 = bg.mci_frames_host(ka, kb, bg.mci_field_host(ka, kb), 4, [1, 2, 3])
    for j, r in enumerate(per):
        gt = E.load_image(os.path.join(root, "gt", "clipA", "g%03d.png" % r["i"]))[0].unsqueeze(0)
        p_, s_ = M.psnr_ssim(torch.from_numpy(bg.normalised_upload(u8[j])).unsqueeze(0), gt, None)
        assert r["DAIN_PSNR"] == float(p_[0]) and r["DAIN_SSIM"] == float(s_[0])
    # the default leaves metrics.json as it was: no such key
    _write_example(os.path.join(root, "d"), n_key=2, rate=2)
    os.makedirs(os.path.join(root, "d", "gt", "clipA"))
    for i in range(3):
        Image.fromarray(rng.integers(0, 255, (32, 48, 3), dtype=np.uint8)).save(os.path.join(root, "d", "gt", "clipA", "g%03d.png" % i))
    E.evaluate_from_folder(model, *(os.path.join(root, "d", x) for x in ("inputs", "DAIN", "Predict_motion")), os.path.join(root, "d", "out"),
                           gt_dir=os.path.join(root, "d", "gt"), metrics=True)
    assert "background" not in json.load(open(os.path.join(root, "d", "out", "metrics.json")))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank(rank, world, port, root, q):
    import torch.distributed as dist
    from render_in_between_amd import distributed as ribdist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    ribdist.init_process_group("gloo")
    torch.set_num_threads(2)
    cfg, model = _model()
    E = ev.Evaluator(cfg, label_fn=oracle_labels)
    written = E.evaluate_from_folder(model, os.path.join(root, "inputs"), None, os.path.join(root, "Predict_motion"),
                                     os.path.join(root, "sharded"), background="mci")
    q.put((rank, [os.path.basename(w) for w in written]))
    dist.barrier()
    dist.destroy_process_group()


def test_two_gloo_ranks_write_the_single_rank_files(tmp_path):
    import torch.multiprocessing as mp
    from PIL import Image
    root = str(tmp_path)
    n = _example_without_dain(root, n_key=4, rate=2)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank, args=(r, 2, port, root, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=300) for _ in range(2))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    (_, w0), (_, w1) = res
    assert sorted(w0 + w1) == ["f%03d.png" % i for i in range(n)] and not set(w0) & set(w1)
    cfg, model = _model()
    single = ev.Evaluator(cfg, label_fn=oracle_labels).evaluate_from_folder(
        model, os.path.join(root, "inputs"), None, os.path.join(root, "Predict_motion"), os.path.join(root, "single"), background="mci")
    for name in single:
        other = os.path.join(root, "sharded", "clipA", os.path.basename(name))
        assert np.array_equal(np.asarray(Image.open(name)), np.asarray(Image.open(other)))


def test_argument_errors(tmp_path):
    root = str(tmp_path)
    _example_without_dain(root, n_key=2, rate=2)
    cfg, model = _model()
    dirs = (os.path.join(root, "inputs"), None, os.path.join(root, "Predict_motion"), os.path.join(root, "out"))
    with pytest.raises(ValueError, match="background must be"):
        ev.Evaluator(cfg, label_fn=oracle_labels).evaluate_from_folder(model, *dirs, background="flow")
    with pytest.raises(ValueError, match="resize_on='gpu'"):
        ev.Evaluator(cfg, label_fn=oracle_labels, resize_on="gpu").evaluate_from_folder(model, *dirs, background="mci")
    os.remove(os.path.join(root, "inputs", "clipA", "0001.png"))
    with pytest.raises(ValueError, match="clipA"):
        ev.Evaluator(cfg, label_fn=oracle_labels).evaluate_from_folder(model, *dirs, background="mci")
    import importlib
    inf = importlib.import_module("render_in_between_amd.inference")
    assert inf.parse_args(["--input-dir", "x"]).background == "dain"
    assert inf.parse_args(["--input-dir", "x", "--background", "mci"]).background == "mci"
    for bad in (["--background", "flow"], ["--background", "mci", "--resize-on", "gpu"]):
        with pytest.raises(SystemExit):
            inf.parse_args(["--input-dir", "x"] + bad)
    with pytest.raises(ValueError, match="power of two"):
        bg.mci_frames_host(np.zeros((8, 8, 3), np.uint8), np.zeros((8, 8, 3), np.uint8), np.zeros((1, 1, 2), np.int16), 3, [1])


def test_default_background_is_unchanged(tmp_path):
    """background="dain" (and no argument at all) with a DAIN folder: the frames of the oracle loop of tests/test_driver.py,
    named after the DAIN files."""
    from PIL import Image
    root = str(tmp_path)
    _write_example(root, n_key=2, rate=2)
    cfg, model = _model()
    dirs = (os.path.join(root, "inputs"), os.path.join(root, "DAIN"), os.path.join(root, "Predict_motion"))
    E = ev.Evaluator(cfg, label_fn=oracle_labels)
    w_def = E.evaluate_from_folder(model, *dirs, os.path.join(root, "o1"))
    w_dain = E.evaluate_from_folder(model, *dirs, os.path.join(root, "o2"), background="dain")
    assert [os.path.basename(w) for w in w_dain] == ["f000.png", "f001.png", "f002.png"]
    for x, y in zip(w_def, w_dain):
        assert open(x, "rb").read() == open(y, "rb").read()
    k0, osz = E.load_image(os.path.join(root, "inputs", "clipA", "0000.png"))
    d1, _ = E.load_image(os.path.join(root, "DAIN", "clipA", "f001.png"))
    l1 = oracle_labels([E.load_pose(os.path.join(root, "Predict_motion", "clipA", "f001_keypoints.json"), osz)], 32, 48)[0]
    spec = rib.GenSpec.from_cfg(cfg.gen)
    R = generator_ref.RefGenerator(spec, synth.make_state_dict(spec, 2))
    img, mask = R(l1.unsqueeze(0), None, d1.unsqueeze(0), k0.unsqueeze(0))
    want = generator_ref.quantise_uint8(generator_ref.blend(img, mask, d1.unsqueeze(0)))
    assert np.array_equal(np.asarray(Image.open(w_dain[1])), want)
    assert "background DAIN frames" in __import__("importlib").import_module("render_in_between_amd.inference").summary_line(E)


def test_the_two_normalisations():
    """normalised: the host's division (what a decoded file gives, io_worker.normalised_chw); normalised_upload: the device's
    reciprocal multiplication, three float32 operations - they differ in the last bit for 111 of the 256 values."""
    from render_in_between_amd import io_worker
    u8 = np.arange(256, dtype=np.uint8).reshape(1, 256, 1).repeat(3, 2)
    assert np.array_equal(bg.normalised(u8), io_worker.normalised_chw(u8))
    up = bg.normalised_upload(u8)
    assert up.dtype == np.float32 and up.shape == (3, 1, 256)
    want = [np.float32(np.float32(np.float32(v) * np.float32(1.0 / 255.0)) - np.float32(0.5)) * np.float32(2.0) for v in range(256)]
    assert np.array_equal(up[0, 0], np.array(want, np.float32))
    assert int((up != bg.normalised(u8)).sum()) == 3 * 111 and np.abs(up - bg.normalised(u8)).max() < 2e-7


def test_abi_is_declared_and_bound():
    from render_in_between_amd import _native
    hdr = open(os.path.join(ROOT, "include", "rib.h")).read()
    for name in ("rib_mci_field_shape", "rib_mci_workspace_bytes", "rib_mci_field", "rib_mci_frames"):
        assert name + "(" in hdr and name in _native.SIGNATURES
    assert len(_native.SIGNATURES["rib_mci_frames"][1]) == 14 and len(_native.SIGNATURES["rib_mci_field"][1]) == 11
    declared = re.findall(r"^\w+ (rib_mci_\w+)\(", hdr, re.M)                 # one entry per operation, and the shape query
    assert len(declared) == 4 and set(declared) == {n for n in _native.SIGNATURES if n.startswith("rib_mci_")}
