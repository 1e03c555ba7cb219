"""The six-pane diagnostic sheet of the folder driver and the per-clip video made of it (numpy only: no torch, no GPU).

The reference's Evaluator.evaluate_from_folder(gen_vid=True) draws, per frame, Predict | Mask | Fuse over DAIN ("CAIN" in
its titles) | Ground Truth | Skeleton on a matplotlib canvas and encodes <clip>.mp4 (PGNR/utils/visualize.py make_video;
the pane bytes are tensor2images', PGNR/utils/utils.py:122-147).  This module states OUR sheet as an exact integer
definition - the layout and the titles are this project's, not matplotlib's - and writes the video as Motion-JPEG in a plain
RIFF AVI (no H.264 encoder, ffmpeg or imageio is available to this project):

    layout(H, W)          pane rectangles and the sheet size
    title_bitmap(W)       the two title bars as a 0/1 bitmap, from the glyph table below (no PIL fonts: they differ between machines)
    compose_host(...)     THE definition of the sheet's bytes; rib_panel (csrc/panel.hip.h, Generator.panel) is bit-equal to it
    write_mjpeg_avi(...)  JPEG files -> <clip>.avi; assemble(...) does it for a clip's sheet folder

Pane values: a 3-channel pane is uint8(clip(x * 0.5 + 0.5, 0, 1) * 255) in float64, truncating - the arithmetic of
rib_quantise, pinned to the reference's bytes by tests/golden/quant_ref.npz.  The 1-channel Mask pane is
uint8(float64(m) * 255.0), truncating, no clip, on all three channels (m is a sigmoid's output, in [0, 1]).  (The reference
forms that one product in float32 - a float32 array times a Python scalar - and so lands one grey level higher where
float32(m * 255) rounds up onto an integer, e.g. at m = 1 - 2^-24; the float64 product is the definition here.)
"""
from __future__ import annotations

import os
import struct

import numpy as np

GUTTER = 8                     # white border around and between the panes
TITLE_H = 24                   # title bar above each pane row
BACKGROUND = 255
TITLE_RGB = (0, 0, 255)
PANES = ("Predict", "Mask", "Fuse", "DAIN", "Ground Truth", "Skeleton")      # row 0, then row 1 (the reference's order)
AVI_MAX_BYTES = int(1.9 * 2 ** 30)                                           # plain RIFF AVI, no OpenDML: sizes are 32-bit

# 5 x 7 glyphs of the letters the titles use (upper case), one string per row, '#' = set
_GLYPHS = {
    " ": (".....", ".....", ".....", ".....", ".....", ".....", "....."),
    "A": (".###.", "#...#", "#...#", "#####", "#...#", "#...#", "#...#"),
    "C": (".###.", "#...#", "#....", "#....", "#....", "#...#", ".###."),
    "D": ("####.", "#...#", "#...#", "#...#", "#...#", "#...#", "####."),
    "E": ("#####", "#....", "#....", "####.", "#....", "#....", "#####"),
    "F": ("#####", "#....", "#....", "####.", "#....", "#....", "#...."),
    "G": (".###.", "#...#", "#....", "#.###", "#...#", "#...#", ".###."),
    "H": ("#...#", "#...#", "#...#", "#####", "#...#", "#...#", "#...#"),
    "I": (".###.", "..#..", "..#..", "..#..", "..#..", "..#..", ".###."),
    "K": ("#...#", "#..#.", "#.#..", "##...", "#.#..", "#..#.", "#...#"),
    "L": ("#....", "#....", "#....", "#....", "#....", "#....", "#####"),
    "M": ("#...#", "##.##", "#.#.#", "#.#.#", "#...#", "#...#", "#...#"),
    "N": ("#...#", "##..#", "#.#.#", "#..##", "#...#", "#...#", "#...#"),
    "O": (".###.", "#...#", "#...#", "#...#", "#...#", "#...#", ".###."),
    "P": ("####.", "#...#", "#...#", "####.", "#....", "#....", "#...."),
    "R": ("####.", "#...#", "#...#", "####.", "#.#..", "#..#.", "#...#"),
    "S": (".####", "#....", "#....", ".###.", "....#", "....#", "####."),
    "T": ("#####", "..#..", "..#..", "..#..", "..#..", "..#..", "..#.."),
    "U": ("#...#", "#...#", "#...#", "#...#", "#...#", "#...#", ".###."),
}
_GLYPH_W, _GLYPH_H, _GLYPH_SCALE = 5, 7, 2          # drawn at 10 x 14 with 2 px between letters, 5 px from the bar's top


def layout(H, W):
    """-> {"sheet": (SH, SW), "panes": [(y0, x0, H, W)] in PANES order, "titles": [(y0, TITLE_H)] of the two bars}.
    From the top: gutter, title bar, pane row 0, gutter, title bar, pane row 1, gutter; from the left: gutter, pane, gutter,
    pane, gutter, pane, gutter.  The title bars span the sheet's width."""
    H, W = int(H), int(W)
    if H < 1 or W < 1:
        raise ValueError("layout: H and W must be positive, got %dx%d" % (H, W))
    SH, SW = 2 * (H + TITLE_H) + 3 * GUTTER, 3 * W + 4 * GUTTER
    bars = [(GUTTER + r * (TITLE_H + H + GUTTER), TITLE_H) for r in range(2)]
    panes = [(bars[r][0] + TITLE_H, GUTTER + c * (W + GUTTER), H, W) for r in range(2) for c in range(3)]
    return {"sheet": (SH, SW), "panes": panes, "titles": bars}


def text_bitmap(text):
    """One line of text -> uint8 0/1 [14, n] from the glyph table (upper case)."""
    rows = [[] for _ in range(_GLYPH_H)]
    for k, ch in enumerate(text.upper()):
        if ch not in _GLYPHS:
            raise ValueError("title_bitmap: no glyph for %r" % ch)
        for y, line in enumerate(_GLYPHS[ch]):
            rows[y] += [1 if c == "#" else 0 for c in line] + ([0] if k + 1 < len(text) else [])
    a = np.array(rows, np.uint8)
    return np.repeat(np.repeat(a, _GLYPH_SCALE, 0), _GLYPH_SCALE, 1)


def title_bitmap(W, names=PANES):
    """The two title bars of a sheet of pane width W: uint8 0/1 [2, TITLE_H, SW], every pane's name centred over it (clipped
    to the pane's width when the pane is narrower than the text)."""
    SW = 3 * int(W) + 4 * GUTTER
    out = np.zeros((2, TITLE_H, SW), np.uint8)
    for k, name in enumerate(names):
        r, c = divmod(k, 3)
        t = text_bitmap(name)[:, :W]
        x0 = GUTTER + c * (W + GUTTER) + (W - t.shape[1]) // 2
        y0 = (TITLE_H - t.shape[0]) // 2
        out[r, y0:y0 + t.shape[0], x0:x0 + t.shape[1]] = t
    return out


def quantise_host(x):
    """uint8(clip(x * 0.5 + 0.5, 0, 1) * 255) in float64, truncating: [.., 3, H, W] -> uint8 [.., H, W, 3] (tensor2images)."""
    a = np.moveaxis(np.asarray(x, np.float32).astype(np.float64), -3, -1) * 0.5 + 0.5
    return (np.clip(a, 0, 1) * 255.0).astype(np.uint8)


def mask_host(m):
    """uint8(float64(m) * 255.0), truncating, no clip, on three channels: [.., 1, H, W] -> uint8 [.., H, W, 3]."""
    a = (np.moveaxis(np.asarray(m, np.float32).astype(np.float64), -3, -1) * 255.0).astype(np.int64).astype(np.uint8)
    return np.repeat(a, 3, axis=-1)


def compose_host(pred, mask, fuse, dain, gt, label, titles=None):
    """THE definition of the sheets: float32 arrays pred, fuse, dain, gt [T,3,H,W], mask [T,1,H,W], label [T,>=3,H,W]
    (channels 0..2: the skeleton image) -> uint8 [T, SH, SW, 3].  pred, mask and fuse None together: the key-frame rule
    (PGNR/models/evaluator.py:240-244: a key frame passes through) - Predict = Fuse = gt, Mask = 0.
    titles: 0/1 [2, TITLE_H, SW] (title_bitmap) or None: no text."""
    if (pred is None) != (mask is None) or (pred is None) != (fuse is None):
        raise ValueError("compose_host: pred, mask and fuse are None together (key-frame rule) or not at all")
    dain, gt, label = (np.asarray(a, np.float32) for a in (dain, gt, label))
    T, _, H, W = dain.shape
    if dain.shape != (T, 3, H, W) or gt.shape != (T, 3, H, W) or label.ndim != 4 or label.shape[0] != T or label.shape[1] < 3 \
            or label.shape[2:] != (H, W):
        raise ValueError("compose_host: dain, gt [T,3,H,W] and label [T,>=3,H,W] expected, got %s %s %s" % (dain.shape, gt.shape, label.shape))
    if pred is None:
        q_pred = q_fuse = quantise_host(gt)
        q_mask = np.zeros((T, H, W, 3), np.uint8)
    else:
        pred, mask, fuse = (np.asarray(a, np.float32) for a in (pred, mask, fuse))
        if pred.shape != (T, 3, H, W) or fuse.shape != (T, 3, H, W) or mask.shape != (T, 1, H, W):
            raise ValueError("compose_host: pred, fuse [T,3,H,W] and mask [T,1,H,W] expected, got %s %s %s" % (pred.shape, fuse.shape, mask.shape))
        q_pred, q_mask, q_fuse = quantise_host(pred), mask_host(mask), quantise_host(fuse)
    L = layout(H, W)
    SH, SW = L["sheet"]
    out = np.full((T, SH, SW, 3), BACKGROUND, np.uint8)
    for (y0, x0, _, _), q in zip(L["panes"], (q_pred, q_mask, q_fuse, quantise_host(dain), quantise_host(gt), quantise_host(label[:, :3]))):
        out[:, y0:y0 + H, x0:x0 + W] = q
    if titles is not None:
        titles = np.asarray(titles)
        if titles.shape != (2, TITLE_H, SW):
            raise ValueError("compose_host: titles must be [2, %d, %d], got %s" % (TITLE_H, SW, titles.shape))
        for r, (y0, _) in enumerate(L["titles"]):
            out[:, y0:y0 + TITLE_H][:, titles[r] != 0] = TITLE_RGB
    return out


def pane(sheet, k, H, W):
    """Pane k (PANES order, or its name) of a sheet [.., SH, SW, 3] of pane size H x W."""
    y0, x0, _, _ = layout(H, W)["panes"][PANES.index(k) if isinstance(k, str) else k]
    return sheet[..., y0:y0 + H, x0:x0 + W, :]


# ---- sheet files -----------------------------------------------------------------------------------------------------------
def sheet_dir(save_dir, clip):
    return os.path.join(save_dir, clip + "_panels")


def save_sheet(u8, jpg_name, quality=90, png_name=None):
    """One sheet uint8 [SH, SW, 3] -> its JPEG (the video's frame) and, with png_name, the lossless copy."""
    from PIL import Image
    im = Image.fromarray(u8)
    im.save(jpg_name, format="JPEG", quality=int(quality))
    if png_name is not None:
        im.save(png_name)
    return jpg_name


# ---- Motion-JPEG in a plain RIFF AVI ---------------------------------------------------------------------------------------
def _chunk(fourcc, data):
    return fourcc + struct.pack("<I", len(data)) + data + (b"\0" if len(data) & 1 else b"")


def _avi_header(n, width, height, fps, sizes):
    """The bytes in front of the first frame chunk: RIFF header, LIST hdrl (avih; LIST strl: strh vids/MJPG, strf
    BITMAPINFOHEADER) and the LIST movi header - and the file's total size."""
    fps = float(fps)
    usec = int(round(1e6 / fps))
    rate, scale = (int(fps), 1) if fps == int(fps) else (int(round(fps * 1000)), 1000)
    biggest = max(sizes) if sizes else 0
    movi = 4 + sum(8 + s + (s & 1) for s in sizes)
    avih = struct.pack("<14I", usec, int(biggest * fps), 0, 0x10, n, 0, 1, biggest, width, height, 0, 0, 0, 0)      # AVIF_HASINDEX
    strh = b"vids" + b"MJPG" + struct.pack("<IHHIIIIIIii4h", 0, 0, 0, 0, scale, rate, 0, n, biggest, -1, 0, 0, 0, min(width, 32767), min(height, 32767))
    strf = struct.pack("<IiiHH4sIiiII", 40, width, height, 1, 24, b"MJPG", width * height * 3, 0, 0, 0, 0)
    hdrl = b"LIST" + struct.pack("<I", 4 + 8 + len(avih) + 12 + 8 + len(strh) + 8 + len(strf)) + b"hdrl" + _chunk(b"avih", avih) \
        + b"LIST" + struct.pack("<I", 4 + 8 + len(strh) + 8 + len(strf)) + b"strl" + _chunk(b"strh", strh) + _chunk(b"strf", strf)
    total = 12 + len(hdrl) + 8 + movi + 8 + 16 * n
    head = b"RIFF" + struct.pack("<I", total - 8) + b"AVI " + hdrl + b"LIST" + struct.pack("<I", movi) + b"movi"
    return head, total


def avi_bytes(sizes, fps=30):
    """Size of the .avi that write_mjpeg_avi makes of JPEG files of these sizes (a pure function: nothing is read or written)."""
    return _avi_header(len(sizes), 0, 0, fps, list(sizes))[1]


def write_mjpeg_avi(paths, out, fps=30):
    """JPEG files (all of one size, in playing order) -> `out`: Motion-JPEG in a plain RIFF AVI.  hdrl (avih, one strl with
    strh vids/MJPG and a BITMAPINFOHEADER strf), movi of even-padded 00dc chunks holding the files' bytes unchanged, idx1
    (offsets from the 'movi' tag).  A file that would pass AVI_MAX_BYTES (no OpenDML) is refused before anything is written."""
    from PIL import Image
    paths = list(paths)
    if not paths:
        raise ValueError("write_mjpeg_avi: no frames")
    if not fps > 0:
        raise ValueError("write_mjpeg_avi: fps must be positive")
    sizes = [os.path.getsize(p) for p in paths]
    total = avi_bytes(sizes, fps)
    if total > AVI_MAX_BYTES:
        raise ValueError("write_mjpeg_avi: %s would take %.2f GiB, a plain RIFF AVI (no OpenDML) ends at %.1f GiB; nothing was written, "
                         "the %d sheet files stay where they are" % (out, total / 2.0 ** 30, AVI_MAX_BYTES / 2.0 ** 30, len(paths)))
    with Image.open(paths[0]) as im:
        if im.format != "JPEG":
            raise ValueError("write_mjpeg_avi: %s is not a JPEG file" % paths[0])
        width, height = im.size
    head, total = _avi_header(len(paths), width, height, fps, sizes)
    idx, pos = [], 4                                       # offsets count from the 'movi' tag
    with open(out + ".tmp", "wb") as f:
        f.write(head)
        for p, s in zip(paths, sizes):
            with open(p, "rb") as g:
                data = g.read()
            if len(data) != s:
                raise ValueError("write_mjpeg_avi: %s changed while the video was written" % p)
            f.write(_chunk(b"00dc", data))
            idx.append(struct.pack("<4sIII", b"00dc", 0x10, pos, s))          # AVIIF_KEYFRAME
            pos += 8 + s + (s & 1)
        f.write(b"idx1" + struct.pack("<I", 16 * len(idx)) + b"".join(idx))
        assert f.tell() == total
    os.replace(out + ".tmp", out)
    return out


def assemble(save_dir, clip, fps=30, keep_frames=False):
    """<save_dir>/<clip>_panels/*.jpg in index order -> <save_dir>/<clip>.avi; then the JPEG sheets are removed, and the
    folder too unless keep_frames (it then holds the lossless %04d.png sheets).  A pure function of the folder: whichever
    ranks wrote the sheets, the video is the same.  A refused video (write_mjpeg_avi) leaves every file in place."""
    d = sheet_dir(save_dir, clip)
    jpgs = [os.path.join(d, f) for f in sorted(os.listdir(d)) if f.endswith(".jpg")]
    out = write_mjpeg_avi(jpgs, os.path.join(save_dir, clip + ".avi"), fps)
    for p in jpgs:
        os.remove(p)
    if not keep_frames:
        try:
            os.rmdir(d)
        except OSError:
            pass                                                # something else lives there: leave it
    return out
