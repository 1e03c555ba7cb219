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
    jpeg_encode_host(...) THE definition of a sheet's JPEG file when the GPU encodes it (panel_encode="gpu"): baseline 4:2:0 in
                          integers only; rib_jpeg (csrc/jpeg.hip.h, Generator.jpeg) is bit-equal to it

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
    """One sheet uint8 [SH, SW, 3] -> its JPEG (the video's frame; jpg_name None: it is written elsewhere) and, with png_name,
    the lossless copy."""
    from PIL import Image
    im = Image.fromarray(u8)
    if jpg_name is not None:
        im.save(jpg_name, format="JPEG", quality=int(quality))
    if png_name is not None:
        im.save(png_name)
    return jpg_name


# ---- baseline JPEG in integers: the definition rib_jpeg is held to ---------------------------------------------------------
# ITU-T T.81 Annex K: the two quantisation tables (K.1, K.2, natural order) and the four "typical" Huffman tables (K.3 - K.6:
# 16 code-length counts, then the symbols in code order)
_JPEG_QBASE = (
    (16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99),
    (17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99)
    + (99,) * 32)
_JPEG_DC_BITS = ((0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0), (0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0))
_JPEG_DC_VALS = tuple(range(12))
_JPEG_AC_BITS = ((0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125), (0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119))
_JPEG_AC_VALS = (
    bytes.fromhex("01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738393a"
                  "434445464748494a535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aa"
                  "b2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa"),
    bytes.fromhex("000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a35363738393a"
                  "434445464748494a535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aa"
                  "b2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa"))
# position in the block (row * 8 + column) of the k-th coefficient in zig-zag order (T.81 figure A.6)
_JPEG_ZIGZAG = (0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63)
# the DCT matrix in 13 fractional bits, K[u][x] = round(8192 * c(u)/2 * cos((2x + 1) u pi / 16)), c(0) = 1/sqrt(2), c(u) = 1 otherwise:
# seven magnitudes, 4096 cos(k pi / 16) rounded for k = 1..7 (k = 4 is also row 0), written out
_JPEG_DCT = ((2896, 2896, 2896, 2896, 2896, 2896, 2896, 2896),
             (4017, 3406, 2276, 799, -799, -2276, -3406, -4017),
             (3784, 1567, -1567, -3784, -3784, -1567, 1567, 3784),
             (3406, -799, -4017, -2276, 2276, 4017, 799, -3406),
             (2896, -2896, -2896, 2896, 2896, -2896, -2896, 2896),
             (2276, -4017, 799, 3406, -3406, -799, 4017, -2276),
             (1567, -3784, 3784, -1567, -1567, 3784, -3784, 1567),
             (799, -2276, 3406, -4017, 4017, -3406, 2276, -799))
JPEG_HEADER_BYTES = 629


def jpeg_qtables(quality):
    """The two Annex K tables under the IJG quality scaling, natural order, int32 [2, 64]: scale = 5000 // q below 50, else
    200 - 2 q; entry = clamp((base * scale + 50) // 100, 1, 255).  These are the tables PIL stores for the same quality."""
    if isinstance(quality, bool) or int(quality) != quality or not 1 <= int(quality) <= 100:
        raise ValueError("jpeg: quality must be an integer in 1..100, got %r" % (quality,))
    q = int(quality)
    scale = 5000 // q if q < 50 else 200 - 2 * q
    return np.clip((np.array(_JPEG_QBASE, np.int32) * scale + 50) // 100, 1, 255).astype(np.int32)


def _jpeg_huffman(bits, vals):
    """(code, length) per symbol, uint32 [256] each (length 0: no code), by T.81 Annex C: codes of one length count up, the
    first code of the next length is the count doubled."""
    code = np.zeros(256, np.uint32)
    size = np.zeros(256, np.uint32)
    c, k = 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            code[vals[k]], size[vals[k]] = c, length
            c, k = c + 1, k + 1
        c <<= 1
    return code, size


_JPEG_HUFF = None


def _jpeg_tables():
    global _JPEG_HUFF
    if _JPEG_HUFF is None:
        _JPEG_HUFF = {"dc": [_jpeg_huffman(_JPEG_DC_BITS[c], _JPEG_DC_VALS) for c in range(2)],
                      "ac": [_jpeg_huffman(_JPEG_AC_BITS[c], _JPEG_AC_VALS[c]) for c in range(2)]}
    return _JPEG_HUFF


def jpeg_header(SH, SW, quality):
    """The JPEG_HEADER_BYTES bytes in front of the entropy-coded data: SOI, APP0 (JFIF 1.01, density 1:1, no thumbnail), DQT
    luminance, DQT chrominance (zig-zag order), SOF0 (8 bit, SH x SW, Y 2x2 table 0, Cb 1x1 table 1, Cr 1x1 table 1), DHT DC 0,
    AC 0, DC 1, AC 1, DRI (the MCUs of one MCU row), SOS (Y: tables 0/0, Cb and Cr: 1/1; Ss 0, Se 63, Ah/Al 0)."""
    q = jpeg_qtables(quality)
    zz = list(_JPEG_ZIGZAG)
    out = b"\xff\xd8" + b"\xff\xe0" + struct.pack(">H5sBBBHHBB", 16, b"JFIF\0", 1, 1, 0, 1, 1, 0, 0)
    for c in range(2):
        out += b"\xff\xdb" + struct.pack(">HB", 67, c) + bytes(int(v) for v in q[c][zz])
    out += b"\xff\xc0" + struct.pack(">HBHHB", 17, 8, SH, SW, 3) + bytes((1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1))
    for c in range(2):
        out += b"\xff\xc4" + struct.pack(">HB", 19 + 12, c) + bytes(_JPEG_DC_BITS[c]) + bytes(_JPEG_DC_VALS)
        out += b"\xff\xc4" + struct.pack(">HB", 19 + 162, 0x10 | c) + bytes(_JPEG_AC_BITS[c]) + _JPEG_AC_VALS[c]
    out += b"\xff\xdd" + struct.pack(">HH", 4, (SW + 15) // 16)
    out += b"\xff\xda" + struct.pack(">HB", 12, 3) + bytes((1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0))
    assert len(out) == JPEG_HEADER_BYTES
    return out


def jpeg_segment_bound(SW):
    """Upper bound of one restart segment's bytes, stuffing included: a block emits at most 64 symbols (one DC, 63 AC) of at
    most 16 + 11 bits (the longest code and the longest value field; the true worst case, 20 + 63 * 26 bits, is smaller), so an
    MCU row of n = 6 * ceil(SW / 16) blocks is at most 216 n bytes before the padding to a byte (216 n is whole already) and
    twice that when every byte is 0xFF and gets a zero behind it."""
    return 2 * 216 * 6 * ((int(SW) + 15) // 16)


def jpeg_max_bytes(SH, SW):
    """Upper bound of one file: header, every segment at its bound, a 2-byte RSTn between segments, EOI (rib_jpeg_max_bytes)."""
    rows = (int(SH) + 15) // 16
    return JPEG_HEADER_BYTES + rows * jpeg_segment_bound(SW) + 2 * (rows - 1) + 2


def _jpeg_size(a):
    """Number of bits of |v| (the category of T.81 tables F.1 / F.2), 0 for 0: int32 array."""
    a = np.abs(a)
    return sum((a >= (1 << k)).astype(np.int32) for k in range(12))


def jpeg_coefficients(u8, quality=90):
    """The quantised coefficients of one image uint8 [SH, SW, 3] in coding order: int32 [rows, 6 * cols, 64] - per MCU row, per
    MCU the blocks Y00 Y01 Y10 Y11 Cb Cr, each in zig-zag order.  See jpeg_encode_host for the arithmetic."""
    u8 = np.asarray(u8)
    SH, SW = u8.shape[:2]
    rows, cols = (SH + 15) // 16, (SW + 15) // 16
    p = np.pad(u8, ((0, rows * 16 - SH), (0, cols * 16 - SW), (0, 0)), mode="edge").astype(np.int32)
    r, g, b = p[..., 0], p[..., 1], p[..., 2]
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + 8421375) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + 8421375) >> 16
    half = lambda c: (c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2] + 2) >> 2
    yb = y.reshape(rows, 2, 8, cols, 2, 8).transpose(0, 3, 1, 4, 2, 5).reshape(rows, cols, 4, 8, 8)
    cbb, crb = (half(c).reshape(rows, 8, cols, 8).transpose(0, 2, 1, 3).reshape(rows, cols, 1, 8, 8) for c in (cb, cr))
    s = np.concatenate([yb, cbb, crb], axis=2).astype(np.int32) - 128                       # [rows, cols, 6, y, x]
    K = np.array(_JPEG_DCT, np.int32)
    t = (np.einsum("ux,rcbyx->rcbyu", K, s) + 512) >> 10                                    # rows of the block: 3 fractional bits stay
    F = (np.einsum("vy,rcbyu->rcbvu", K, t) + 32768) >> 16                                  # columns
    assert t.dtype == np.int32 and F.dtype == np.int32
    Q = jpeg_qtables(quality).reshape(2, 8, 8)[[0, 0, 0, 0, 1, 1]]                          # [6, 8, 8]
    q = np.sign(F) * ((np.abs(F) + (Q >> 1)) // Q)
    return q.reshape(rows, cols * 6, 64)[..., list(_JPEG_ZIGZAG)].astype(np.int32)


def _jpeg_segment(zz, st):
    """The entropy-coded bytes of one restart segment: zz int32 [n, 64], the blocks of an MCU row in coding order."""
    H = _jpeg_tables()
    n = zz.shape[0]
    comp = np.tile(np.array([0, 0, 0, 0, 1, 2]), n // 6)
    tab = (comp > 0).astype(np.int64)                                                       # Huffman table of the block
    dc = zz[:, 0].astype(np.int64)
    diff = dc.copy()
    for c in range(3):                                                                      # predictor: the component's previous block, 0 at the start
        m = np.nonzero(comp == c)[0]
        diff[m[1:]] -= dc[m[:-1]]
    cat = _jpeg_size(diff).astype(np.int64)
    dcode = np.stack([H["dc"][c][0] for c in range(2)]).astype(np.uint64)
    dsize = np.stack([H["dc"][c][1] for c in range(2)]).astype(np.int64)
    vbits = np.where(diff < 0, diff + (1 << cat) - 1, diff).astype(np.uint64)
    keys = [np.arange(n, dtype=np.int64) * 65]
    codes = [(dcode[tab, cat] << cat.astype(np.uint64)) | vbits]
    sizes = [dsize[tab, cat] + cat]
    bi, ki = np.nonzero(zz[:, 1:])                                                          # in block, then zig-zag order
    ki = ki + 1
    v = zz[bi, ki].astype(np.int64)
    first = np.ones(len(bi), bool)
    first[1:] = bi[1:] != bi[:-1]
    prev = np.where(first, 0, np.concatenate([[0], ki[:-1]]))
    run = ki - prev - 1
    nz, r = run >> 4, run & 15                                                              # ZRL symbols, then the run of the symbol
    sz = _jpeg_size(v).astype(np.int64)
    t = tab[bi]
    acode = np.stack([H["ac"][c][0] for c in range(2)]).astype(np.uint64)
    asize = np.stack([H["ac"][c][1] for c in range(2)]).astype(np.int64)
    zc, zl = acode[:, 0xF0], asize[:, 0xF0]
    rep = np.zeros((2, 4), np.uint64)
    for c in range(2):
        for j in range(1, 4):
            rep[c, j] = (rep[c, j - 1] << np.uint64(zl[c])) | zc[c]
    sym = (r << 4) | sz
    hl = asize[t, sym]
    if len(sym) and (hl == 0).any():
        raise ValueError("jpeg: an AC coefficient outside the 10 bits the tables code")
    vb = np.where(v < 0, v + (1 << sz) - 1, v).astype(np.uint64)
    keys.append(bi * 65 + ki)
    codes.append((rep[t, nz] << (hl + sz).astype(np.uint64)) | (acode[t, sym] << sz.astype(np.uint64)) | vb)
    sizes.append(nz * zl[t] + hl + sz)
    last = np.zeros(n, np.int64)
    last[bi] = ki                                                                           # the largest: ki ascends inside a block
    eob = np.nonzero(last < 63)[0]
    keys.append(eob * 65 + 64)
    codes.append(acode[tab[eob], 0])
    sizes.append(asize[tab[eob], 0])
    key, code, size = np.concatenate(keys), np.concatenate(codes), np.concatenate(sizes)
    order = np.argsort(key, kind="stable")
    code, size = code[order], size[order]
    total = int(size.sum())
    idx = np.repeat(np.arange(len(size)), size)
    pos = np.arange(total) - np.repeat(np.cumsum(size) - size, size)
    bits = ((code[idx] >> (size[idx] - 1 - pos).astype(np.uint64)) & np.uint64(1)).astype(np.uint8)
    bits = np.concatenate([bits, np.ones(-total % 8, np.uint8)])                            # the segment is padded with 1-bits
    data = np.packbits(bits)
    ff = np.nonzero(data == 0xFF)[0]
    st["stuffed"] += len(ff)
    st["zrl"] += int(nz.sum())
    st["no_eob"] += n - len(eob)
    st["max_dc_category"] = max(st["max_dc_category"], int(cat.max()))
    st["segments"] += 1
    return np.insert(data, ff + 1, 0).tobytes()


def jpeg_encode_host(u8, quality=90, stats=False):
    """THE definition of a sheet's JPEG file under panel_encode="gpu": uint8 [SH, SW, 3], any size from 1 x 1 to 65535 x 65535
    -> the bytes of a complete JFIF file (uint8 [T, SH, SW, 3] -> a list of T files; a file does not depend on its neighbours).
    rib_jpeg (csrc/jpeg.hip.h, Generator.jpeg) writes the same bytes.  stats=True: -> (bytes, {"stuffed": stuffed 0xFF bytes,
    "zrl": ZRL symbols, "no_eob": blocks whose coefficient 63 is non-zero, "max_dc_category", "segments"}).

    Format: baseline sequential DCT (SOF0), 8 bit, Y Cb Cr at 4:2:0 (MCU 16 x 16: Y00 Y01 Y10 Y11 Cb Cr), one interleaved scan,
    the Annex K quantisation tables under the IJG quality scaling (jpeg_qtables) and the four Annex K Huffman tables - what PIL
    writes by default at the same quality, up to the arithmetic below - and a restart interval of one MCU row: every MCU row is
    a byte-aligned segment with its own DC predictors, RST0..7 cycling between them.  Header: jpeg_header.  No floats anywhere:

      edge      the image is padded to multiples of 16 by repeating its last column and row; SOF0 carries the true size
      colour    Y  = ( 19595 R + 38470 G +  7471 B + 32768) >> 16
                Cb = (-11059 R - 21709 G + 32768 B + 8421375) >> 16        (8421375 = 128 * 65536 + 32767)
                Cr = ( 32768 R - 27439 G -  5329 B + 8421375) >> 16        all three in 0..255, sums non-negative
      chroma    per 2 x 2 pixels (a + b + c + d + 2) >> 2 of the Cb (Cr) values above
      shift     s = sample - 128, in -128..127
      DCT       K[u][x] = round(8192 * c(u)/2 * cos((2x+1) u pi/16)) as seven written-out integers (_JPEG_DCT); int32 throughout:
                  rows      t[y][u] = (sum_x K[u][x] s[y][x] + 512) >> 10          (arithmetic shift: floor)
                  columns   F[v][u] = (sum_y K[v][y] t[y][u] + 32768) >> 16
                bound: sum_x |K[u][x]| <= 8 * 2896 = 23168 (row 0; the other rows sum to at most 20996), so the row sums are at
                most 23168 * 128 = 2965504 < 2^22 and |t| <= 2897; the column sums are at most 23168 * 2897 + 32768 = 67150464
                < 2^27; |F| <= 1025.  DC: F[0][0] is in -1024..1016, so a DC difference is at most 2040 (category <= 11); an AC
                coefficient is at most 20996 * 23168 * 128 / 2^26 + 2 < 930 in magnitude (category <= 10).  int16 holds t and F.
      quantise  q = sign(F) * ((|F| + (Q >> 1)) // Q): to the nearest, halves away from zero
      order     zig-zag (_JPEG_ZIGZAG)
      DC        diff to the component's previous block in the segment (0 at its start); category n = bits of |diff|, 0..11; the
                category's code, then n bits: diff if diff >= 0, else diff + 2^n - 1
      AC        per non-zero coefficient: a run of r zeros before it - r >> 4 ZRL symbols (0xF0), then symbol (r & 15) << 4 | n
                and n bits as for DC; EOB (0x00) after the last one unless coefficient 63 is non-zero
      bytes     bits most significant first; the segment's last byte is filled with 1-bits; then every 0xFF byte (a filled
                last byte included) is followed by 0x00
    """
    u8 = np.asarray(u8)
    if u8.dtype != np.uint8 or u8.ndim not in (3, 4) or u8.shape[-1] != 3 or min(u8.shape[-3:-1]) < 1 or max(u8.shape[-3:-1]) > 65535:
        raise ValueError("jpeg_encode_host: uint8 [SH, SW, 3] or [T, SH, SW, 3] expected, got %s %s" % (u8.dtype, u8.shape))
    jpeg_qtables(quality)
    if u8.ndim == 4:
        res = [jpeg_encode_host(a, quality, stats) for a in u8]
        return res if not stats else ([r[0] for r in res], [r[1] for r in res])
    SH, SW = u8.shape[:2]
    zz = jpeg_coefficients(u8, quality)
    st = {"stuffed": 0, "zrl": 0, "no_eob": 0, "max_dc_category": 0, "segments": 0}
    parts = [jpeg_header(SH, SW, quality)]
    for k in range(zz.shape[0]):
        if k:
            parts.append(bytes((0xFF, 0xD0 + (k - 1) % 8)))
        parts.append(_jpeg_segment(zz[k], st))
    parts.append(b"\xff\xd9")
    data = b"".join(parts)
    return (data, st) if stats else data


def save_jpeg(data, jpg_name):
    """The bytes of a finished JPEG file -> jpg_name."""
    with open(jpg_name, "wb") as f:
        f.write(data)
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
