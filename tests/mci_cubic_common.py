"""What tests/test_mci_cubic_cpu.py and tests/test_gpu_mci_cubic.py share: the builders of the cubic sampler's inputs (key frames,
fields of four kinds, masks), the quality set-up with true in-between frames, and the definition's frames, each made once."""
import numpy as np

from render_in_between_amd import background as bg
from tests.test_background_cpu import random_pair, texture

# ---- the inputs of the kernel tests -------------------------------------------------------------------------------------------------
SIZES = [(1, 1), (2, 3), (5, 7), (67, 93), (64, 96), (8, 1040)]      # every tap clamped (x3) | partial blocks, W % 4 != 0, unaligned rows |
WIDE = [(67, 93), (64, 96), (8, 1040)]                               # the vector path | more than 256 items per row, more than 16 tiles
KINDS = ("zero", "smooth", "random", "mixed")
REACH = {"full": bg.max_disp(bg.MAX_LEVELS), "half": 2 * bg.max_disp(bg.MAX_LEVELS) + 1}      # 79, and 159 in half pixels
_FIELDS, _WANT = {}, {}


def field(kind, h, w, precision="full"):
    """int16 [Hb, Wb, 2].  zero; smooth: a slow zoom about the frame's centre, 1 px (full) per 64 px; random: every component
    uniform over the full reach with both extremes present; mixed: the zoom with one wild block (full reach) per block row - per 32
    blocks of a row where the row is longer."""
    key = (kind, h, w, precision)
    if key not in _FIELDS:
        Hb, Wb = bg.field_shape(h, w)
        reach, unit = REACH[precision], 2 if precision == "half" else 1
        rng = np.random.default_rng([KINDS.index(kind), h, w, unit])
        by, bx = np.mgrid[0:Hb, 0:Wb]
        zoom = np.stack([np.round(unit * (8 * bx + 3.5 - w / 2) / 64.0), np.round(unit * (8 * by + 3.5 - h / 2) / 64.0)], -1).astype(np.int16)
        if kind == "zero":
            f = np.zeros((Hb, Wb, 2), np.int16)
        elif kind == "smooth":
            f = zoom
        elif kind == "random":
            f = rng.integers(-reach, reach + 1, (Hb, Wb, 2)).astype(np.int16)
            f[0, 0], f[-1, -1] = (reach, -reach), (-reach, reach)
        else:
            f = zoom.copy()
            for r in range(Hb):
                for c0 in range(0, Wb, 32):
                    c = c0 + (3 + 5 * r) % min(32, Wb - c0)
                    f[r, c] = [(reach, -reach), (-reach, reach)][(r + c0 // 32) % 2]
        _FIELDS[key] = f
    return _FIELDS[key]


def masks(kind, h, w):
    """(ma, mb) uint8 [h, w], nonzero = excluded (values other than 1 among them): "blobs" = random 8 x 8 cells at 0.3 and single
    pixels at 0.02; "one" = everything excluded."""
    rng = np.random.default_rng([7, h, w])
    out = []
    for _ in range(2):
        if kind == "one":
            m = np.ones((h, w), bool)
        else:
            m = np.repeat(np.repeat(rng.random(((h + 7) // 8, (w + 7) // 8)) < 0.3, 8, 0), 8, 1)[:h, :w] | (rng.random((h, w)) < 0.02)
        out.append((m * rng.integers(1, 256, (h, w))).astype(np.uint8))
    return tuple(out)


def staged_share(kind, h, w, precision, s, ks):
    """The share of tiles that background.cubic_tile_staged calls staged, over frames ks of the fixture."""
    f = field(kind, h, w, precision)
    got = [bg.cubic_tile_staged(*bg.sample_positions(f, s, k, h, w, precision)) for k in ks]
    return float(np.mean([g.mean() for g in got]))


def want_frames(kind, h, w, s, ks, border, precision, masked=None):
    """The definition's cubic frames of the fixture, made once: uint8 [len(ks), h, w, 3]."""
    key = (kind, h, w, s, tuple(ks), border, precision, masked)
    if key not in _WANT:
        a, b = random_pair(h, w, 11)
        f = field(kind, h, w, precision)
        if masked:
            _WANT[key] = bg.mci_frames_masked_host(a, b, *masks(masked, h, w), f, s, ks, border=border, precision=precision, sampler="cubic")
        else:
            _WANT[key] = bg.mci_frames_host(a, b, f, s, ks, border=border, precision=precision, sampler="cubic")
    return _WANT[key]


# ---- the quality set-up: true frames at quarter-pixel positions ------------------------------------------------------------------------
QH, QW, QS, QINSET = 160, 192, 4, 24
QMOTIONS = [(6, -2), (-10, 6), (14, 10), (2, 0), (0, -6)]            # px between the key frames, even: the true field m / 2 is whole
QSEEDS = range(6)
_SCENES, _BIG = {}, {}


def scene(seed, m):
    """(frames, field): frames[k], k = 0..4, uint8 [160, 192, 3] - one texture at four times the size, moved by k * m quarter
    pixels and box-downsampled 4x, so frame k is the TRUE frame at time k / 4 of the segment frames[0] -> frames[4]; field the true
    uniform block field m / 2."""
    if (seed, m) not in _SCENES:
        pad = 4 * max(max(abs(v) for v in mm) for mm in QMOTIONS)
        if seed not in _BIG:                # one texture per seed serves the five motions
            _BIG[seed] = texture(4 * QH + 2 * pad, 4 * QW + 2 * pad, 100 + seed).astype(np.int32)
        big = _BIG[seed]
        frames = []
        for k in range(QS + 1):
            y0, x0 = pad - k * m[1], pad - k * m[0]
            crop = big[y0:y0 + 4 * QH, x0:x0 + 4 * QW]
            frames.append(((crop.reshape(QH, 4, QW, 4, 3).sum((1, 3)) + 8) >> 4).astype(np.uint8))
        f = np.empty(bg.field_shape(QH, QW) + (2,), np.int16)
        f[...] = (m[0] // 2, m[1] // 2)
        _SCENES[seed, m] = (frames, f)
    return _SCENES[seed, m]


def interior(x):
    return x[QINSET:-QINSET, QINSET:-QINSET].astype(np.float64)


def psnr(x, truth):
    return 10 * np.log10(255.0 ** 2 / max(np.mean((interior(x) - interior(truth)) ** 2), 1e-12))


def sharpness(x, truth):
    """The variance of the second differences (both axes) of x relative to the true frame's, on the interior."""
    d2 = lambda v: np.concatenate([np.diff(v, 2, 0).ravel(), np.diff(v, 2, 1).ravel()]).var()
    return d2(interior(x)) / d2(interior(truth))
