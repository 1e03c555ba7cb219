"""Frames shared by the PNG tests (tests/test_png_cpu.py, tests/test_gpu_png.py): each case is the smallest that can break
something, as three frames [3, H, W, 3] that differ, so that the GPU test also sees that a frame's bytes do not depend on T."""
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUN_LENGTHS = (4, 5, 258, 259, 262, 263)        # behind their literal: remainders 0..3 behind a 258-chunk, and the shortest matches


def load_png():
    """render-in-between_amd/png.py as a module, without importing the package (no torch, no library)."""
    name = "_rib_png_definition"
    if name not in sys.modules:
        spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "render-in-between_amd", "png.py"))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[name] = mod
        spec.loader.exec_module(mod)
    return sys.modules[name]


def run_length_frame(order):
    """A 1 x W frame whose Sub-filtered row is zero runs of exactly RUN_LENGTHS[i] + 1 bytes (a literal and the run behind it),
    in the given order, with single non-zero bytes between them: the raw row is the running sum of that row per channel."""
    f = []
    for j, i in enumerate(order):
        f += [0] * (RUN_LENGTHS[i] + 1) + [7 + 2 * (j % 2)]
    f += [0] * (-len(f) % 3)
    f = np.array(f, np.int64)
    raw = np.zeros_like(f)
    for c in range(3):
        raw[c::3] = np.cumsum(f[c::3]) & 255
    return raw.astype(np.uint8).reshape(1, -1, 3)


def smooth(h, w, rng, phase=0.0):
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.stack([90 + 0.9 * x + 0.5 * y + phase, 128 + 60 * np.sin((x + phase) / 17.0) + 30 * np.cos(y / 9.0), 220 - 0.6 * x - 0.8 * y], -1)
    return (img + rng.normal(0, 1.2, img.shape)).clip(0, 255).astype(np.uint8)


def cases():
    """[(name, uint8 [3, H, W, 3])]: the table of the issue, in its order."""
    rng = np.random.default_rng(20261020)
    noise = lambda h, w: rng.integers(0, 256, (3, h, w, 3), dtype=np.uint8)
    out = [("1x1", noise(1, 1)), ("8x1", noise(8, 1)), ("9x5", noise(9, 5)), ("16x7", noise(16, 7))]
    zero = np.zeros((3, 17, 64, 3), np.uint8)
    zero[1] = 255                                       # frame 0 is all zero: one run cut only by the strip ends
    zero[2, 12, 40] = (1, 2, 3)
    out.append(("17x64-zero", zero))
    out.append(("runs", np.stack([run_length_frame(o) for o in ((0, 1, 2, 3, 4, 5), (5, 3, 1, 4, 2, 0), (3, 0, 5, 2, 1, 4))])))
    out.append(("24x96-noise", noise(24, 96)))
    mixed = np.empty((3, 24, 300, 3), np.uint8)
    for t in range(3):
        mixed[t, 0:8] = smooth(8, 300, rng, 11.0 * t)
        mixed[t, 8:16] = rng.integers(0, 256, (8, 300, 3), dtype=np.uint8)
        mixed[t, 16:24] = (40 + t, 90, 200)
    out.append(("24x300-mixed", mixed))
    wide = np.stack([smooth(8, 4096, rng, 5.0 * t) for t in range(3)])
    wide[:, :, 1000:2500] = rng.integers(0, 256, (3, 8, 1500, 3), dtype=np.uint8)
    wide[:, :, 3000:3800] = 17
    out.append(("8x4096-wide", wide))
    y, x = np.mgrid[0:40, 0:64]
    grad = np.stack([np.stack([(3 * x + t) & 255, (5 * y + 2 * t) & 255, (x + y + 7 * t) & 255], -1) for t in range(3)]).astype(np.uint8)
    out.append(("40x64-gradient", grad))
    return out


def filtered_host(png, img):
    """The filtered bytes of a frame, as the zlib stream holds them."""
    return png.filter_rows(img)[0].tobytes()


def idat_payload(data):
    """The concatenated IDAT data of a PNG file, and the number of IDAT chunks."""
    pos, out, count = 8, [], 0
    while pos < len(data):
        n = int.from_bytes(data[pos:pos + 4], "big")
        if data[pos + 4:pos + 8] == b"IDAT":
            out.append(data[pos + 8:pos + 8 + n])
            count += 1
        pos += 12 + n
    return b"".join(out), count
