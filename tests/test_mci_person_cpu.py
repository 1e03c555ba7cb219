"""mci_person="exclude" on the CPU: the definition (background.mci_field_masked_host / mci_frames_masked_host) keeps the person out
of the matching and out of the in-between backgrounds.

The guarantee: a textured background that pans and an opaque disc with its own motion.  With the true disc masks every pixel of
frames 1 .. s-1 that is not the disc, lies away from the frame border and whose background at least one key frame shows is
reproduced EXACTLY; the unmasked definition gets more than a thousand of them wrong per clip."""
import inspect
import os

import numpy as np
import pytest

from render_in_between_amd import background as bg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARGIN = 96


def texture(rng, height, width):
    """A blocky random texture, smoothed once (3x3 box): uint8 [height, width, 3]."""
    cells = rng.integers(0, 256, ((height + 3) // 4, (width + 3) // 4, 3))
    t = np.repeat(np.repeat(cells, 4, 0), 4, 1)[:height, :width].astype(np.int32)
    p = np.pad(t, ((1, 1), (1, 1), (0, 0)), mode="edge")
    return (sum(p[j:j + height, i:i + width] for j in range(3) for i in range(3)) // 9).astype(np.uint8)


class Scene:
    """Frame k (0..s) of the scene: the background T moves by 2 * pan and the disc by 2 * obj between k = 0 and k = s, so the
    frame in the middle shows A's p - pan and B's p + pan."""

    def __init__(self, seed, height, width, s, pan, obj, radius):
        rng = np.random.default_rng(seed)
        self.h, self.w, self.s, self.pan, self.obj, self.r = height, width, s, pan, obj, radius
        self.T = texture(rng, height + 2 * MARGIN, width + 2 * MARGIN)
        self.D = rng.integers(0, 256, (2 * radius + 1, 2 * radius + 1, 3)).astype(np.uint8)
        self.c0 = (width // 2 - obj[0], height // 2 - obj[1])       # the disc's centre at k = 0: mid-frame in the middle of the segment

    def disc(self, k):
        """bool [h, w]: the disc at time k."""
        cx, cy = self.c0[0] + 2 * self.obj[0] * k // self.s, self.c0[1] + 2 * self.obj[1] * k // self.s
        Y, X = np.mgrid[0:self.h, 0:self.w]
        return (Y - cy) ** 2 + (X - cx) ** 2 <= self.r ** 2, cx, cy

    def frame(self, k):
        assert (2 * self.pan[0] * k) % self.s == 0 and (2 * self.pan[1] * k) % self.s == 0 and (2 * self.obj[0] * k) % self.s == 0 \
            and (2 * self.obj[1] * k) % self.s == 0
        ox, oy = MARGIN + self.pan[0] - 2 * self.pan[0] * k // self.s, MARGIN + self.pan[1] - 2 * self.pan[1] * k // self.s
        f = self.T[oy:oy + self.h, ox:ox + self.w].copy()
        m, cx, cy = self.disc(k)
        Y, X = np.nonzero(m)
        f[Y, X] = self.D[Y - cy + self.r, X - cx + self.r]
        return f, m


def four_taps_clear(mask, oy, ox):
    """bool [h, w]: the pixels p whose sample at the integer position p + (oy, ox) has a clear 2x2 footprint in `mask` (the taps
    p + o, and one further right / down, clamped to the plane) - written here from the truth, not with background.sample_clean."""
    h, w = mask.shape
    Y, X = np.mgrid[0:h, 0:w]
    out = np.ones((h, w), bool)
    for ey in (0, 1):
        for ex in (0, 1):
            out &= ~mask[np.clip(Y + oy + ey, 0, h - 1), np.clip(X + ox + ex, 0, w - 1)]
    return out


# (height, width, levels, s, pan, obj, border, disc radius)
CASES = [
    (160, 192, 3, 8, (4, 0), (-8, 4), "clamp", 22),
    (160, 192, 3, 8, (8, -4), (12, 8), "valid", 22),
    (160, 192, 3, 8, (0, 0), (12, 0), "clamp", 22),
    (160, 192, 3, 4, (4, 4), (-4, 8), "valid", 22),
    (256, 320, 4, 8, (8, 8), (-24, 8), "clamp", 30),
    (131, 173, 3, 8, (4, 0), (-8, 4), "clamp", 22),
    (160, 192, 3, 4, (4, 0), (2, 0), "clamp", 22),       # a slow disc: some background is hidden in both key frames
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%dx%d-L%d-s%d-pan%s-obj%s-%s" % (c[0], c[1], c[2], c[3], c[4], c[5], c[6]))
def test_guarantee(case):
    height, width, levels, s, pan, obj, border, radius = case
    sc = Scene(CASES.index(case), height, width, s, pan, obj, radius)
    (a, ma), (b, mb) = sc.frame(0), sc.frame(s)
    ma8, mb8 = ma.astype(np.uint8) * 255, mb.astype(np.uint8)
    field = bg.mci_field_masked_host(a, b, ma8, mb8, levels, border)
    far = 3                                               # blocks from the frame edge
    inner = field[far + 1:-(far + 1), far + 1:-(far + 1)]
    assert inner.size and (inner[..., 0] == pan[0]).all() and (inner[..., 1] == pan[1]).all(), "the masked field is the pan"
    ks = list(range(1, s))
    got = bg.mci_frames_masked_host(a, b, ma8, mb8, field, s, ks, border)
    plain = bg.mci_frames_host(a, b, bg.mci_field_host(a, b, levels, border), s, ks, border)
    edge = 48 if levels == 4 else 24
    away = np.zeros((height, width), bool)
    away[edge:height - edge, edge:width - edge] = True
    examined = excluded = wrong = plain_wrong = 0
    for j, k in enumerate(ks):
        truth, disc = sc.frame(k)
        ax, ay, bx, by = 2 * pan[0] * k // s, 2 * pan[1] * k // s, 2 * pan[0] * (s - k) // s, 2 * pan[1] * (s - k) // s
        seen = four_taps_clear(ma, -ay, -ax) | four_taps_clear(mb, by, bx)
        base = away & ~disc
        sel = base & seen
        examined += int(base.sum())
        excluded += int((base & ~seen).sum())
        wrong += int((got[j] != truth).any(-1)[sel].sum())
        plain_wrong += int((np.abs(plain[j].astype(np.int32) - truth.astype(np.int32)).max(-1) > 8)[sel].sum())
    print("examined %d excluded %d wrong %d, unmasked wrong by more than 8: %d" % (examined, excluded, wrong, plain_wrong))
    assert examined > 40000 and excluded < examined // 100
    assert wrong == 0
    if case is CASES[-1]:                                 # the slow disc is here for its excluded set; its ghosts are small
        assert excluded > 0 and plain_wrong > 100
    else:
        assert plain_wrong > 1000, "the scene proves nothing: the unmasked definition is right as well"


# ---- what follows from the definition's text ------------------------------------------------------------------------------------
def _pair(h, w, seed=5, shift=(6, -2)):
    rng = np.random.default_rng([seed, h, w])
    t = texture(rng, h + 32, w + 32)
    return (np.ascontiguousarray(t[16:16 + h, 16:16 + w]),
            np.ascontiguousarray(t[16 + shift[1]:16 + shift[1] + h, 16 - shift[0]:16 - shift[0] + w]))


@pytest.mark.parametrize("h,w,levels", [(67, 93, 3), (40, 56, 4), (1, 1, 3), (9, 130, 5), (64, 96, 3)])
def test_zero_masks_under_valid_are_the_unmasked_field(h, w, levels):
    a, b = _pair(h, w)
    z = np.zeros((h, w), np.uint8)
    assert np.array_equal(bg.mci_field_masked_host(a, b, z, z, levels, "valid"), bg.mci_field_host(a, b, levels, "valid"))
    for (dx, dy, searched), (ux, uy) in zip(bg.block_field_levels_masked(a, b, z, z, levels, "valid"), bg.block_field_levels(a, b, levels, "valid")):
        assert np.array_equal(dx, ux) and np.array_equal(dy, uy)


@pytest.mark.parametrize("h,w,levels", [(64, 96, 3), (128, 64, 4), (128, 256, 5)])
def test_zero_masks_under_clamp_on_whole_blocks_are_the_unmasked_field(h, w, levels):
    """Both sides are multiples of 8 << (L-1): every block is full on every level, 64 * SAD // 64 == SAD."""
    assert h % (8 << (levels - 1)) == 0 and w % (8 << (levels - 1)) == 0
    a, b = _pair(h, w)
    z = np.zeros((h, w), np.uint8)
    assert np.array_equal(bg.mci_field_masked_host(a, b, z, z, levels, "clamp"), bg.mci_field_host(a, b, levels, "clamp"))
    assert all(s.all() for _, _, s in bg.block_field_levels_masked(a, b, z, z, levels, "clamp"))


@pytest.mark.parametrize("border", bg.BORDERS)
@pytest.mark.parametrize("precision", bg.PRECISIONS)
@pytest.mark.parametrize("h,w", [(67, 93), (1, 1), (8, 24), (33, 15)])
def test_zero_masks_give_the_unmasked_frames(h, w, border, precision):
    a, b = _pair(h, w)
    z = np.zeros((h, w), np.uint8)
    rng = np.random.default_rng(1)
    field = rng.integers(-19, 20, bg.field_shape(h, w) + (2,)).astype(np.int16)
    ks = range(0, 5)
    assert np.array_equal(bg.mci_frames_masked_host(a, b, z, z, field, 4, ks, border, precision), bg.mci_frames_host(a, b, field, 4, ks, border, precision))


@pytest.mark.parametrize("border", bg.BORDERS)
def test_all_one_masks_give_the_zero_field_and_the_cross_fade(border):
    h, w = 67, 93
    a, b = _pair(h, w)
    one = np.full((h, w), 200, np.uint8)
    field = bg.mci_field_masked_host(a, b, one, one, 4, border)
    assert not field.any()
    assert not any(s.any() for _, _, s in bg.block_field_levels_masked(a, b, one, one, 4, border))
    got = bg.mci_frames_masked_host(a, b, one, one, field, 4, range(5), border)
    fade = [((4 - k) * a.astype(np.int32) + k * b.astype(np.int32) + 2) >> 2 for k in range(5)]
    assert np.array_equal(got, np.stack(fade).astype(np.uint8)) and np.array_equal(got[0], a) and np.array_equal(got[4], b)


def test_the_key_frames_stay_whatever_their_masks():
    h, w = 40, 56
    a, b = _pair(h, w)
    rng = np.random.default_rng(3)
    ma, mb = ((rng.random((h, w)) < 0.5).astype(np.uint8) for _ in range(2))
    field = bg.mci_field_masked_host(a, b, ma, mb, 3, "valid")
    got = bg.mci_frames_masked_host(a, b, ma, mb, field, 8, [0, 8], "valid")
    assert np.array_equal(got[0], a) and np.array_equal(got[1], b)


def test_the_or_pyramid_on_odd_sizes():
    m = np.zeros((5, 7), np.uint8)
    m[4, 6] = 9                                           # the last row and column: its parents are clamped onto itself
    m[0, 1] = 1
    p = bg.mask_pyramid(m, 4)
    assert [x.shape for x in p] == [(5, 7), (3, 4), (2, 2), (1, 1)] and all(x.dtype == bool for x in p)
    want1 = np.zeros((3, 4), bool)
    want1[2, 3] = want1[0, 0] = True
    assert np.array_equal(p[0], m != 0) and np.array_equal(p[1], want1)
    assert np.array_equal(p[2], np.array([[True, False], [False, True]])) and p[3].all()
    for v in (0, 1):
        q = bg.mask_pyramid(np.full((1, 1), v, np.uint8), 5)
        assert [x.shape for x in q] == [(1, 1)] * 5 and all(bool(x[0, 0]) == bool(v) for x in q)
    # a pixel is set iff any of its clamped 2x2 parents is: against the loop
    rng = np.random.default_rng(0)
    m = rng.random((9, 11)) < 0.2
    d = bg.down2_or(m)
    for y in range(5):
        for x in range(6):
            assert d[y, x] == any(m[min(2 * y + j, 8), min(2 * x + i, 10)] for j in (0, 1) for i in (0, 1))


def test_the_fill_and_its_tie_break():
    """A hand-made flag plane of 20 x 24 blocks: a block with two equidistant sources takes the one with the smaller
    (|Dy| + |Dx|, Dy, Dx); a block with no source within 8 keeps (0, 0); searched blocks keep theirs; only searched blocks are
    sources, so a filled block never feeds another."""
    Hb, Wb = 20, 24
    searched = np.zeros((Hb, Wb), bool)
    dx, dy = np.full((Hb, Wb), 99, np.int32), np.full((Hb, Wb), 99, np.int32)      # (what an unsearched block holds must not matter)
    src = {(2, 2): (1, -1), (2, 6): (2, -2), (6, 4): (3, -3), (0, 3): (4, -4), (5, 8): (5, -5), (3, 7): (6, -6)}
    for (y, x), (vx, vy) in src.items():
        searched[y, x] = True
        dx[y, x], dy[y, x] = vx, vy
    fx, fy = bg.fill_unsearched(dx, dy, searched)
    for (y, x), (vx, vy) in src.items():
        assert (fx[y, x], fy[y, x]) == (vx, vy)
    # block (2, 4): (2, 2) and (2, 6) both at Chebyshev 2, Manhattan 2, Dy 0: Dx = -2 wins; (0, 3) is at Chebyshev 2, Manhattan 3
    assert (fx[2, 4], fy[2, 4]) == (1, -1)
    # block (4, 4): (6, 4) and (2, 2), (2, 6) at Chebyshev 2; Manhattan 2 beats 4
    assert (fx[4, 4], fy[4, 4]) == (3, -3)
    # block (4, 6): (3, 7) at Chebyshev 1
    assert (fx[4, 6], fy[4, 6]) == (6, -6)
    # block (4, 7): (3, 7) Dy = -1, Dx = 0 and (5, 8) at Chebyshev 1: Manhattan 1 beats 2
    assert (fx[4, 7], fy[4, 7]) == (6, -6)
    # block (4, 9): (5, 8) at Chebyshev 1
    assert (fx[4, 9], fy[4, 9]) == (5, -5)
    # block (1, 4): (0, 3) and (2, ...)? (0, 3): Chebyshev 1; nothing else that near
    assert (fx[1, 4], fy[1, 4]) == (4, -4)
    # Dy decides before Dx: block (1, 3) ... sources (0, 3) at (Dy, Dx) = (-1, 0) alone at Chebyshev 1
    assert (fx[1, 3], fy[1, 3]) == (4, -4)
    # equal (Chebyshev, Manhattan), different Dy: block (4, 5) sees (6, 4): (2, 3, 2, -1) and (2, 6): (2, 3, -2, 1) and (3, 7): (2, 3, -1, 2)
    assert (fx[4, 5], fy[4, 5]) == (2, -2)
    # the far corner: (19, 23) has no source within 8 - the nearest, (5, 8), is 14 away; (14, 16) is 9 from (5, 8): none either
    assert (fx[19, 23], fy[19, 23]) == (0, 0) and (fx[14, 16], fy[14, 16]) == (0, 0)
    assert (fx[13, 16], fy[13, 16]) == (5, -5)            # exactly 8 away: (5, 8) -> Chebyshev max(8, 8)
    # against the brute force, every block
    for y in range(Hb):
        for x in range(Wb):
            if searched[y, x]:
                continue
            c = sorted((max(abs(sy - y), abs(sx - x)), abs(sy - y) + abs(sx - x), sy - y, sx - x) for (sy, sx) in src
                       if max(abs(sy - y), abs(sx - x)) <= bg.FILL_RADIUS)
            want = src[(y + c[0][2], x + c[0][3])] if c else (0, 0)
            assert (fx[y, x], fy[y, x]) == want, (y, x)
    assert bg.FILL_RADIUS == 8 and bg.VALID_SHARE == 4


def test_the_searched_flag_flips_at_a_quarter():
    """One full block (N = 64): with 16 pixels left the start is valid and the block is searched; with 15 it is not."""
    rng = np.random.default_rng(2)
    ya, yb = (rng.integers(0, 256, (8, 8)).astype(np.uint8) for _ in range(2))
    z = np.zeros((1, 1), np.int32)
    order = rng.permutation(64)
    for clear, want in ((17, True), (16, True), (15, False), (0, False)):
        m = np.ones(64, bool)
        m[order[:clear]] = False
        m = m.reshape(8, 8)
        for ma, mb in ((m, np.zeros((8, 8), bool)), (np.zeros((8, 8), bool), m)):
            cost, ok, n = bg.block_cost_masked(ya, yb, ma, mb, z, z, "clamp")
            assert int(n[0, 0]) == clear and bool(ok[0, 0]) == want
            dx, dy, searched = bg.search_masked(ya, yb, ma, mb, z, z, 1, "clamp")
            assert bool(searched[0, 0]) == want
            if not want:
                assert (dx[0, 0], dy[0, 0]) == (0, 0)
    # a partial block: N = 3 * 5 = 15, 4 n >= 15 from n = 4
    ya, yb = (rng.integers(0, 256, (3, 5)).astype(np.uint8) for _ in range(2))
    for clear, want in ((4, True), (3, False)):
        m = np.ones(15, bool)
        m[:clear] = False
        _, ok, n = bg.block_cost_masked(ya, yb, m.reshape(3, 5), np.zeros((3, 5), bool), z, z, "valid")
        assert int(n[0, 0]) == clear and bool(ok[0, 0]) == want
    # the cost is the mean over the counted pixels, in 1/64: one pixel left of a full block under "clamp" at d = 0
    ya, yb = np.full((8, 8), 10, np.uint8), np.full((8, 8), 13, np.uint8)
    m = np.zeros((8, 8), bool)
    m[:6] = True
    cost, ok, n = bg.block_cost_masked(ya, yb, m, np.zeros((8, 8), bool), z, z, "clamp")
    assert int(n[0, 0]) == 16 and int(cost[0, 0]) == 64 * 3 and bool(ok[0, 0])


def test_check_settings():
    ok = lambda **kw: bg.check_settings("mci", 32, "clamp", "host", **kw)
    assert ok() == ok(mci_person="keep") == ok(mci_person="exclude") == (3, "clamp")
    assert bg.check_settings("mci", 64, "valid", "host", mci_precision="half") == (4, "valid")          # existing calls stay valid
    assert bg.check_settings("mci", 64, "valid", "host", "who", "full", "exclude") == (4, "valid")
    assert ok(mci_person="keep", mci_precision="half", output_size="keyframes") == (3, "clamp")
    assert list(inspect.signature(bg.check_settings).parameters)[:6] == ["background", "mci_range", "mci_border", "resize_on", "who", "mci_precision"]
    for bad in ("mask", None, 1, "Exclude"):
        with pytest.raises(ValueError, match="mci_person must be 'keep' or 'exclude'"):
            ok(mci_person=bad)
    with pytest.raises(ValueError, match="mci_person is a setting of background='mci'"):
        bg.check_settings("dain", 32, "clamp", "host", mci_person="exclude")
    with pytest.raises(ValueError, match="mci_person='exclude' with mci_precision='half'.*masked rib_halfpel_refine"):
        ok(mci_person="exclude", mci_precision="half")
    with pytest.raises(ValueError, match="mci_person='exclude' with output_size='keyframes'.*masked rib_scaled_frames"):
        ok(mci_person="exclude", output_size="keyframes")


def test_the_driver_refuses_before_any_file(tmp_path):
    import render_in_between_amd as rib
    from render_in_between_amd import evaluator as ev, inference
    cfg = rib.AttrDict(gen=rib.hsm_gen_config(), model_height=64, model_width=64, gauss_sigma=5, skeleton_thres=0.001, foot_thres=0.001)
    out = os.path.join(str(tmp_path), "out")
    for more in (dict(mci_precision="half"), dict(output_size="keyframes")):
        with pytest.raises(ValueError, match="mci_person='exclude' with"):
            ev.Evaluator(cfg).evaluate_from_folder(lambda *a: None, str(tmp_path), None, str(tmp_path), out, background="mci", mci_person="exclude", **more)
    with pytest.raises(ValueError, match="mci_person is a setting of background='mci'"):
        ev.Evaluator(cfg).evaluate_from_folder(lambda *a: None, str(tmp_path), str(tmp_path), str(tmp_path), out, mci_person="exclude")
    assert not os.path.exists(out)
    text = " ".join(inference.build_parser().format_help().split())      # (argparse wraps the lines)
    assert "--mci-person" in text and "coarse pose mask" in text and "hard seam" in text and "unmeasured on real footage" in text
    base = ["--input-dir", "x", "--background", "mci"]
    assert inference.parse_args(base).mci_person == "keep" and inference.parse_args(base + ["--mci-person", "exclude"]).mci_person == "exclude"
    for bad in (["--mci-person", "exclude", "--mci-precision", "half"], ["--mci-person", "exclude", "--output-size", "keyframes"],
                ["--mci-person", "mask"]):
        with pytest.raises(SystemExit):
            inference.parse_args(base + bad)
    with pytest.raises(SystemExit):
        inference.parse_args(["--input-dir", "x", "--mci-person", "exclude"])


def test_abi_is_declared_bound_and_exported():
    from render_in_between_amd import _native
    hdr = open(os.path.join(ROOT, "include", "rib.h")).read()
    assert "size_t rib_masked_workspace_bytes(rib_handle* h, int B, int H, int W, int levels);" in hdr
    assert "int rib_masked_field(rib_handle* h, int B, int H, int W, const uint8_t* a_u8, const uint8_t* b_u8, const uint8_t* ma_u8," in hdr
    assert "const uint8_t* mb_u8, int16_t* field_i16, int levels, int border, void* workspace, void* hip_stream);" in hdr
    assert "int rib_masked_frames(rib_handle* h, int T, int B, int H, int W, const uint8_t* a_u8, const uint8_t* b_u8, const uint8_t* ma_u8," in hdr
    assert "const uint8_t* mb_u8, const int16_t* field_i16, int sample_rate, int k_first, int border, int precision," in hdr
    sig = _native.SIGNATURES
    assert len(sig["rib_masked_workspace_bytes"][1]) == 5 and len(sig["rib_masked_field"][1]) == 13 and len(sig["rib_masked_frames"][1]) == 17
    assert sig["rib_masked_workspace_bytes"] == sig["rib_mci_workspace_bytes"]
    family = sorted(n for n in sig if n.startswith("rib_mci_"))
    assert family == ["rib_mci_field", "rib_mci_field_shape", "rib_mci_frames", "rib_mci_workspace_bytes"]
    assert "unless the person is excluded (`rib_masked_*`" in hdr and "rib_mci_frames' 14 arguments are pinned" in hdr
    assert "unless the person is excluded (`rib_masked_*`)" in bg.__doc__
    src = open(os.path.join(ROOT, "render-in-between_amd", "csrc", "frame.hip")).read()
    for name in ("rib_masked_workspace_bytes", "rib_masked_field", "rib_masked_frames"):
        assert ("\n%s %s(rib_handle* h" % ("size_t" if name.endswith("bytes") else "int", name)) in src
    if os.path.exists(_native.LIB_PATH):                  # a built tree: the library exports them
        import ctypes
        lib = ctypes.CDLL(_native.LIB_PATH)
        assert all(hasattr(lib, n) for n in ("rib_masked_workspace_bytes", "rib_masked_field", "rib_masked_frames"))
