"""What tests/test_mci_detail_cpu.py and tests/test_gpu_mci_detail.py share: the translating scenes whose motion is NOT a multiple of
the size ratio, the random inputs of the kernel tests, and the definition's fields, each made once and left unchanged."""
import numpy as np

from render_in_between_amd import background as bg, resize

RNG = np.random.default_rng

# ---- translating scenes ----------------------------------------------------------------------------------------------------------
# (model, key frames, d0 = (dx, dy) px per side at the key frames' size, seeds).  The seeds are recorded: for each of them the
# model-size field is right on every interior block for both borders - model_field_is_right below states "right"; they are the first
# two of seeds 0..39 that meet it (the first scene: 15 of the 40 do; the second, whose R = 1 leaves the model-size search half a model
# pixel of room, only these two).  The other seeds have a model-size vector the search cannot recover from, which this feature does
# not address.
SCENES = [((128, 160), (320, 400), (9, -4), (0, 2)),
          ((160, 192), (320, 384), (7, -3), (21, 29))]
SCENE_RATE = 8
_SCENE, _FIELD = {}, {}


def blurred_cells(h, w, seed):
    """32 px cells of random colour, Gaussian blur sigma 4 (separable, radius 12, edges repeated), noise sigma 4: uint8 [h, w, 3]."""
    r = RNG(seed)
    cells = r.integers(40, 216, ((h + 31) // 32, (w + 31) // 32, 3)).astype(np.float64)
    img = np.repeat(np.repeat(cells, 32, 0), 32, 1)[:h, :w]
    t = np.arange(-12, 13)
    g = np.exp(-t * t / (2 * 4.0 ** 2))
    g /= g.sum()
    for axis in (0, 1):
        n = img.shape[axis]
        p = np.concatenate([img.take([0] * 12, axis), img, img.take([n - 1] * 12, axis)], axis)
        img = sum(g[i] * p.take(range(i, i + n), axis) for i in range(25))
    return np.clip(img + r.normal(0, 4, img.shape), 0, 255).astype(np.uint8)


def scene(index, seed):
    """(a0, b0, true): the key frames uint8 [h0, w0, 3] of scene `index` and true(k, s), the scene's frame k of s where its offset
    is a whole pixel (None where it is not).  Frame k shows the scene displaced so that A(p - 2 k d0 / s) = frame_k(p)."""
    if (index, seed) not in _SCENE:
        _, (h0, w0), (mx, my), _ = SCENES[index]
        pad = max(abs(mx), abs(my))
        big = blurred_cells(h0 + 2 * pad, w0 + 2 * pad, seed)

        def true(k, s):
            if ((s - 2 * k) * mx) % s or ((s - 2 * k) * my) % s:
                return None
            ox, oy = (s - 2 * k) * mx // s, (s - 2 * k) * my // s
            return big[pad + oy:pad + oy + h0, pad + ox:pad + ox + w0]
        _SCENE[index, seed] = (true(0, 1), true(1, 1), true)
    return _SCENE[index, seed]


def scene_field(index, seed, border, precision="full"):
    """The model-size field of the scene's resized key frames, as the driver makes it."""
    key = (index, seed, border, precision)
    if key not in _FIELD:
        (H, W), _, _, _ = SCENES[index]
        a0, b0, _ = scene(index, seed)
        a, b = resize.resize_cubic_u8(a0, W, H), resize.resize_cubic_u8(b0, W, H)
        f = bg.mci_field_host(a, b, levels=3, border=border)
        _FIELD[key] = bg.mci_refine_host(a, b, f, border=border) if precision == "half" else f
    return _FIELD[key]


def model_field_is_right(index, seed, border):
    """The condition the seeds were picked by: on every model block that overlaps the examined region grown by two full-size blocks
    (a pixel's vector blends the four nearest block centres, and the median reads one block further), the model-size vector,
    scaled to output pixels, lies within the search radius R of d0 in both components - so does every blend of such vectors, and
    so does its rounding, d0 being whole: the search can reach d0 from every start."""
    (H, W), (h0, w0), d0, _ = SCENES[index]
    f = scene_field(index, seed, border).astype(np.int64)
    R, inset = bg.detail_radius((H, W), (h0, w0)), scene_inset(index) - 2 * bg.BLOCK
    by, bx = np.mgrid[0:f.shape[0], 0:f.shape[1]]
    near = ((8 * by + 8) * h0 > inset * H) & (8 * by * h0 < (h0 - inset) * H) & ((8 * bx + 8) * w0 > inset * W) & (8 * bx * w0 < (w0 - inset) * W)
    ex, ey = np.abs(f[..., 0] * w0 - d0[0] * W), np.abs(f[..., 1] * h0 - d0[1] * H)          # |ratio f - d0| * model side
    return bool(((ex <= R * W) & (ey <= R * H))[near].all())


def scene_inset(index):
    """3 max|d0| + 16: how far inside the border the translation guarantee is examined."""
    mx, my = SCENES[index][2]
    return 3 * max(abs(mx), abs(my)) + 16


# ---- the kernel tests' inputs ----------------------------------------------------------------------------------------------------
REACH = {"full": bg.max_disp(bg.MAX_LEVELS), "half": 2 * bg.max_disp(bg.MAX_LEVELS) + 1}      # 79, and 159 in half pixels
# model, key frames, B, the amplitude of the random field in whole model pixels (None: the full reach)
SHAPES = [((24, 40), (61, 99), 3, 3),        # ratio about 2.5, R = 2, partial blocks on both axes, a run that ends mid-workgroup
          ((16, 24), (80, 120), 1, 2),       # R = 3
          ((16, 16), (128, 120), 1, 2),      # R = 4: 81 candidates over 64 lanes
          ((40, 56), (40, 56), 1, 4),        # equal sizes, R = 1
          ((40, 56), (23, 31), 1, 4),        # key frames smaller than the model
          ((8, 8), (128, 128), 1, None)]     # components +-79 (+-159 in half): starts near +-1264, far outside the frame
_PAIRS, _RANDOM_FIELDS, _WANT = {}, {}, {}


def smooth_noise(h, w, seed):
    """Random bytes with some spatial correlation (a 3x3 box over white noise, stretched back): costs differ, ties are rare."""
    v = RNG(seed).integers(0, 256, (h + 2, w + 2, 3)).astype(np.int32)
    box = sum(v[j:j + h, i:i + w] for j in range(3) for i in range(3))
    lo, hi = box.min(), box.max()
    return ((box - lo) * 255 // max(hi - lo, 1)).astype(np.uint8)


def pairs(size, B, kind="random"):
    """(a0, b0) uint8 [B, h0, w0, 3]; kind "constant": one colour per frame, so every cost of a block ties."""
    key = (size, B, kind)
    if key not in _PAIRS:
        h0, w0 = size
        if kind == "constant":
            a = np.broadcast_to(np.array([200, 30, 90], np.uint8), (B, h0, w0, 3)).copy()
            b = np.broadcast_to(np.array([20, 210, 40], np.uint8), (B, h0, w0, 3)).copy()
        else:
            a = np.stack([smooth_noise(h0, w0, [1, h0, w0, i]) for i in range(B)])
            b = np.stack([smooth_noise(h0, w0, [2, h0, w0, i]) for i in range(B)])
        _PAIRS[key] = (a, b)
    return _PAIRS[key]


def random_fields(model, B, amp, precision):
    """int16 [B, Hb, Wb, 2], uniform over +-amp model pixels (+-(2 amp + 1) in half pixels; amp None: the full reach), both
    extremes present in every item."""
    key = (model, B, amp, precision)
    if key not in _RANDOM_FIELDS:
        Hb, Wb = bg.field_shape(*model)
        reach = REACH[precision] if amp is None else (2 * amp + 1 if precision == "half" else amp)
        f = RNG([3, model[0], model[1], B, reach]).integers(-reach, reach + 1, (B, Hb, Wb, 2)).astype(np.int16)
        f[:, 0, 0], f[:, -1, -1] = (reach, -reach), (-reach, reach)
        _RANDOM_FIELDS[key] = f
    return _RANDOM_FIELDS[key]


def want_fields(model, size, B, amp, border, precision, kind="random"):
    """The definition's fields of the fixture, item by item: int16 [B, H0b, W0b, 2]."""
    key = (model, size, B, amp, border, precision, kind)
    if key not in _WANT:
        a, b = pairs(size, B, kind)
        f = random_fields(model, B, amp, precision)
        _WANT[key] = np.stack([bg.mci_detail_field_host(a[i], b[i], f[i], model, border=border, precision=precision) for i in range(B)])
    return _WANT[key]


def long_field(h, w, seed):
    """A field for the existing frame entries with components up to +-DETAIL_MAX_DISP (1268): int16 [Hb, Wb, 2], both extremes
    present."""
    Hb, Wb = bg.field_shape(h, w)
    m = bg.DETAIL_MAX_DISP
    f = RNG([5, h, w, seed]).integers(-m, m + 1, (Hb, Wb, 2)).astype(np.int16)
    f.reshape(-1, 2)[0], f.reshape(-1, 2)[-1] = (m, -m), (-m, m)
    return f
