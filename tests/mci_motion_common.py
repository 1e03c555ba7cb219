"""What tests/test_mci_motion_cpu.py and tests/test_gpu_mci_motion.py share: scenes of four key frames on a second-order trajectory
(whole-pixel and quarter-pixel), the blocks and pixels on which the definition is exact, and random fields for the kernels."""
import numpy as np

from render_in_between_amd import background as bg
from tests.test_background_cpu import eroded, guaranteed, pixels_of, texture

H, W = 160, 192
PAD = 64                                    # the scenes' shifts stay within +-48 px


def moving_keys(seed, steps):
    """(keys, crop): keys[j], j = 0..3, uint8 [160, 192, 3] - one texture shifted by the running sum of `steps` (three (dx, dy) px, the
    motion across each segment); crop(ox, oy) is the scene at shift (ox, oy): the truth of any frame."""
    tex = texture(H + 2 * PAD, W + 2 * PAD, seed)
    crop = lambda ox, oy: np.ascontiguousarray(tex[PAD - oy:PAD - oy + H, PAD - ox:PAD - ox + W])
    pos = np.concatenate([[(0, 0)], np.cumsum(np.asarray(steps), 0)])
    return [crop(int(x), int(y)) for x, y in pos], crop, pos


def exact_blocks(d):
    """bool [Hb, Wb]: the blocks whose vector after the median is provably d (tests/test_background_cpu.py: guaranteed, eroded)."""
    return eroded(guaranteed(H, W, d[0], d[1]))


def looked_up(g, d, sign):
    """bool [Hb, Wb]: the blocks whose motion-compensated lookup (two vectors d back, sign = -1, or on, +1) lands on a block of g."""
    Hb, Wb = g.shape
    by, bx = np.mgrid[0:Hb, 0:Wb]
    return g[np.clip((8 * by + 4 + sign * 2 * d[1]) >> 3, 0, Hb - 1), np.clip((8 * bx + 4 + sign * 2 * d[0]) >> 3, 0, Wb - 1)]


def accel_blocks(d_prev, d, d_next):
    """bool [Hb, Wb]: the blocks whose acceleration after the median is provably the scene's: the block's own vector exact, the
    neighbours' fields (None: absent) exact where they are read, and the same for the eight blocks around it."""
    g = exact_blocks(d)
    if d_prev is not None:
        g = g & looked_up(exact_blocks(d_prev), d, -1)
    if d_next is not None:
        g = g & looked_up(exact_blocks(d_next), d, 1)
    return eroded(g)


def exact_pixels(d_prev, d, d_next):
    """bool [H, W]: the pixels whose four nearest blocks are exact in the field and in the acceleration."""
    return pixels_of(exact_blocks(d) & accel_blocks(d_prev, d, d_next), H, W)


# ---- quarter-pixel truth: tests/mci_cubic_common.scene's construction on a second-order trajectory ------------------------------------
QINSET = 32
_BIG = {}


def quarter_scene(seed, steps):
    """(keys, mids): one texture at four times the size, box-downsampled 4x.  keys[j], j = 0..3, the key frames at the running sum
    of `steps` (three (dx, dy) whole px; their second difference a multiple of 8 so that every position below is a whole quarter
    pixel); mids[k], k = 0..4, the TRUE frame at time k / 4 of the MIDDLE segment on the parabola through the four key frames:
    x(t) = x1 + u t + a t^2 / 2, a = steps[2] - steps[1] = steps[1] - steps[0], u = steps[1] - a / 2."""
    pad = 4 * PAD
    if seed not in _BIG:
        _BIG[seed] = texture(4 * H + 2 * pad, 4 * W + 2 * pad, 200 + seed).astype(np.int32)
    big = _BIG[seed]

    def at(qx, qy):                         # the scene shifted by (qx, qy) quarter pixels
        crop = big[pad - qy:pad - qy + 4 * H, pad - qx:pad - qx + 4 * W]
        return ((crop.reshape(H, 4, W, 4, 3).sum((1, 3)) + 8) >> 4).astype(np.uint8)
    steps = np.asarray(steps, np.int64)
    a = steps[2] - steps[1]
    assert (a == steps[1] - steps[0]).all() and (a % 8 == 0).all()
    pos = np.concatenate([[(0, 0)], np.cumsum(steps, 0)])
    keys = [at(int(4 * x), int(4 * y)) for x, y in pos]
    u = steps[1] - a // 2
    mids = []
    for k in range(5):                      # 4 x(k/4) = 4 x1 + u k + a k^2 / 8
        q = 4 * pos[1] + u * k + (a * k * k) // 8
        assert ((a * k * k) % 8 == 0).all()
        mids.append(at(int(q[0]), int(q[1])))
    return keys, mids


def psnr(x, truth):
    d = x[QINSET:-QINSET, QINSET:-QINSET].astype(np.float64) - truth[QINSET:-QINSET, QINSET:-QINSET].astype(np.float64)
    return 10 * np.log10(255.0 ** 2 / max(np.mean(d * d), 1e-12))


def accelerating_keys(root, n_key, hw, clip, a=(2, -2)):
    """Overwrites write_example's key frames (tests/composite_common.py) with crops of one blocky scene whose motion per segment grows
    by `a` px from segment to segment: key frame k is the scene at a * k (k + 1) / 2."""
    import os
    from PIL import Image
    h, w = hw
    rng = np.random.default_rng(6)
    pad = max(abs(a[0]), abs(a[1])) * n_key * (n_key + 1) // 2 + 8
    cells = rng.integers(30, 226, ((h + 2 * pad) // 6 + 1, (w + 2 * pad) // 6 + 1, 3)).astype(np.uint8)
    big = np.repeat(np.repeat(cells, 6, 0), 6, 1)
    for k in range(n_key):
        oy, ox = pad + a[1] * k * (k + 1) // 2, pad + a[0] * k * (k + 1) // 2
        Image.fromarray(np.ascontiguousarray(big[oy:oy + h, ox:ox + w])).save(os.path.join(root, "inputs", clip, "%04d.png" % k))


# ---- random inputs of the kernel tests ---------------------------------------------------------------------------------------------------
def random_fields(B, Hb, Wb, reach, seed):
    """int16 [3, B, Hb, Wb, 2]: previous, own and next fields, every component uniform over +-reach with both extremes present in
    each, so that the motion-compensated lookups clamp at every edge."""
    rng = np.random.default_rng([seed, B, Hb, Wb, reach])
    f = rng.integers(-reach, reach + 1, (3, B, Hb, Wb, 2)).astype(np.int16)
    if Hb * Wb > 1:
        f[:, :, 0, 0], f[:, :, -1, -1] = (reach, reach), (-reach, -reach)
    return f


def accel_field(kind, h, w, seed=0):
    """int16 [Hb, Wb, 2] for the frame kernels.  smooth: a slow ramp of +-32 units across the frame (c up to +-4 px in the
    middle of a segment, tiles stay staged); rough: every component uniform over +-8 * max(h, w) (c up to +-max(h, w) px: samples
    leave the frame on all four sides, and cubic tiles gather)."""
    Hb, Wb = bg.field_shape(h, w)
    by, bx = np.mgrid[0:Hb, 0:Wb]
    if kind == "smooth":
        return np.stack([np.round(32 * (2 * bx + 1 - Wb) / max(Wb, 1)), np.round(-32 * (2 * by + 1 - Hb) / max(Hb, 1))], -1).astype(np.int16)
    reach = 8 * max(h, w)
    a = np.random.default_rng([seed, h, w]).integers(-reach, reach + 1, (Hb, Wb, 2)).astype(np.int16)
    a[0, 0], a[-1, -1], a[0, -1], a[-1, 0] = (reach, reach), (-reach, -reach), (-reach, reach), (reach, -reach)
    return a
