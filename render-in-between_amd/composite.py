"""The folder driver's frame at the SOURCE resolution: the definition (`--output-size source`).

The generator predicts a person and a blend mask at the model size; the background frame exists at the source size.  The
reference fuses at the model size and writes its frames there (PGNR/models/evaluator.py:256-258), so a 1080p clip comes
out at 512x512.  This module states the fuse at the source size,

    out = up(pred) * up(mask) + background_src * (1 - up(mask)),

in integers, so that it is exact in any evaluation order and the GPU kernel (csrc/composite.hip.h, rib_composite) can be
held to it bit for bit:

* P = panel.quantise_host(pred): the PNG quantiser, uint8(clip(x * 0.5 + 0.5, 0, 1) * 255) in float64, truncating;
* M = quantise_mask_host(mask): uint8(clip(m, 0, 1) * 255) in float64, truncating (a float32 times 255 is exact in double,
  so no product rounds up across an integer);
* Pu, Mu = resize.resize_cubic_u8(P / M, W0, H0): the 11-bit fixed-point INTER_CUBIC of the input frames, (v + 2^21) >> 22
  saturated to 0..255 - a mask overshoot clamps; equal sizes take no resize at all;
* out = (Pu * Mu + bg * (255 - Mu) + 127) // 255 in int32, per channel.

Mu = 0 gives the background's bytes, Mu = 255 gives Pu.  The person region is a cubic enlargement of a model-size prediction
and is softer than the source pixels around it; the mask has 8 bits, so a mask that never reaches 1.0 leaves up to 1/255 of
the background under the person.  This is this project's addition, not the reference's output.
"""
import numpy as np

from . import panel, resize

OUTPUT_SIZES = ("model", "source", "keyframes")      # "keyframes": background="mci" at the size of the key frame files


def check_output_size(value, who="output_size"):
    if value not in OUTPUT_SIZES:
        raise ValueError("%s: output_size must be one of %s, got %r" % (who, ", ".join(OUTPUT_SIZES), value))
    return value


def quantise_mask_host(mask):
    """uint8(clip(float64(m), 0, 1) * 255), truncating: float [.., 1, H, W] -> uint8 [.., H, W]."""
    a = np.asarray(mask, np.float32).astype(np.float64)
    if a.ndim < 3 or a.shape[-3] != 1:
        raise ValueError("quantise_mask_host: mask must be [.., 1, H, W], got %s" % (a.shape,))
    a = a.reshape(a.shape[:-3] + a.shape[-2:])
    return (np.clip(a, 0.0, 1.0) * 255.0).astype(np.uint8)


def blend_u8(p_u8, m_u8, bg_u8):
    """(P * M + bg * (255 - M) + 127) // 255 in int32: uint8 [.., H, W, 3], [.., H, W], [.., H, W, 3] -> uint8 [.., H, W, 3]."""
    m = np.asarray(m_u8).astype(np.int32)[..., None]
    v = np.asarray(p_u8).astype(np.int32) * m + np.asarray(bg_u8).astype(np.int32) * (255 - m) + 127
    return (v // 255).astype(np.uint8)


def composite_host(pred, mask, bg_u8):
    """THE definition (module docstring): pred float [n,3,H,W] in [-1,1], mask float [n,1,H,W] in [0,1] (finite), bg_u8 uint8
    [n,H0,W0,3] -> uint8 [n,H0,W0,3]."""
    pred = np.asarray(pred, np.float32)
    mask = np.asarray(mask, np.float32)
    bg = np.asarray(bg_u8)
    if bg.dtype != np.uint8 or bg.ndim != 4 or bg.shape[3] != 3:
        raise ValueError("composite_host: bg_u8 must be uint8 [n,H0,W0,3], got %s %s" % (bg.dtype, bg.shape))
    n, h0, w0, _ = bg.shape
    if pred.ndim != 4 or pred.shape[0] != n or pred.shape[1] != 3:
        raise ValueError("composite_host: pred must be [%d,3,H,W], got %s" % (n, pred.shape))
    if mask.shape != (n, 1) + pred.shape[2:]:
        raise ValueError("composite_host: mask must be %s, got %s" % ((n, 1) + pred.shape[2:], mask.shape))
    if min(n, h0, w0, pred.shape[2], pred.shape[3]) < 1:
        raise ValueError("composite_host: empty frames (pred %s, bg %s)" % (pred.shape, bg.shape))
    P = panel.quantise_host(pred)                                          # [n, H, W, 3]
    M = quantise_mask_host(mask)                                           # [n, H, W]
    out = np.empty((n, h0, w0, 3), np.uint8)
    for i in range(n):
        out[i] = blend_u8(resize.resize_cubic_u8(P[i], w0, h0), resize.resize_cubic_u8(M[i], w0, h0), bg[i])
    return out
