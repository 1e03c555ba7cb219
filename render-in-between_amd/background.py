"""Motion-compensated interpolation (MCI) of a segment's two key frames: the background source of the folder driver's
`background="mci"`, stated in integers.  It is THIS PROJECT'S interpolation, not DAIN: the reference reads one background
frame per output frame from <input>/DAIN/ (an external network with its own CUDA extension ops); the generator only
needs "a plausible frame at time t made from the two key frames", which the mask network keeps where the person is not.
The generator was trained on DAIN backgrounds; the quality of this substitute on real footage has not been measured.

The functions below ARE the definition; the HIP kernels (csrc/mci.hip.h: rib_mci_field / rib_halfpel_refine / rib_mci_frames /
rib_halfpel_frames) are held bit-equal to them (tests/test_gpu_mci.py, tests/test_gpu_mci_halfpel.py).  Every step is integer or fixed point with a stated order and stated tie-breaks:

  luma       Y = (77 R + 150 G + 29 B + 128) >> 8.
  pyramid    levels 0 (full) .. L-1, L = 3 unless asked otherwise (`levels`, below); level l+1 is ceil(h/2) x ceil(w/2), a pixel
             is (the sum of its 2x2 parents, coordinates clamped to the edge, + 2) >> 2.
  matching   bilateral block matching: one displacement d = (dx, dy) per BLOCK x BLOCK block of the INTERMEDIATE frame's grid
             (so the field has no holes), cost(d) = sum over the block's pixels p inside the image of
             |Y_A(clamp(p - d)) - Y_B(clamp(p + d))| + LAMBDA * (|dx| + |dy|).
  search     level L-1: every d in [-SEARCH_TOP, SEARCH_TOP]^2 (L = 3: +-4 at quarter size, i.e. +-32 px of motion between the
             key frames at full size: faster motion falls outside the search); every level below: start = twice the displacement
             of the coarser block that holds this block's centre (block (by >> 1, bx >> 1)), candidates
             start + [-REFINE, REFINE]^2.  The winner is the minimum of the tuple (cost, dx*dx + dy*dy, dy, dx) - packed into one
             integer (pack_key; pack_key_wide above three levels), so it does not depend on the order of evaluation.
  levels     L in 3 (the default), 4, 5: the nominal range 4 * 2^(L-1) * 2 = 32, 64 or 128 px of motion between the key frames
             (the driver's mci_range).  The level-0 field reaches max_disp(L) = 19, 39 or 79 in either component, i.e. 38, 78
             or 158 px of motion.  Nothing else changes with L; a wider search has more room for a false match on periodic
             content (LAMBDA only breaks near-ties).
  median     3x3 componentwise median over the level-0 block field, coordinates clamped at the border.
  per pixel  D(p): bilinear between the four nearest block centres (block b's centre is at 8 b + 3.5), block coordinates
             clamped at the border; the weights are exact in 1/16 per axis, so D is an exact integer in 1/256 px
             (FIELD_FRAC_BITS = 8) - no rounding.
  frame k    of a segment with sample rate s (a power of two, 0 <= k <= s): a = A sampled at p - (2k/s) D(p), b = B sampled at
             p + (2(s-k)/s) D(p); the offsets are rounded to 1/256 px (SAMPLE_FRAC_BITS = 8) as (2k D + s/2) >> log2 s and
             (2(s-k) D + s/2) >> log2 s (arithmetic shifts: floor); a sample is bilinear with edge clamp,
             (sum of the four taps times their 8-bit weight products + 2^15) >> 16, per channel;
             out = ((s-k) a + k b + s/2) >> log2 s.

  border     "clamp" (the default) is everything above.  "valid" (the driver's mci_border) is one-sided at the FRAME border, in
             two places.  Matching: a pixel p of a block counts for candidate d only when p - d and p + d both lie inside the
             plane - the rectangle |dx| <= X <= w-1-|dx|, |dy| <= Y <= h-1-|dy| cut with the block, n pixels of the block's N
             inside the plane; a candidate is valid when 4 n >= N, its cost is (64 * SAD over those n) // n + LAMBDA * (|dx| +
             |dy|) (at most 16320 + 632 < 2^15: pack_key_wide holds it, and is the key for every L), the winner the minimum
             key over the valid candidates; a block whose start candidate is not valid searches nothing and keeps its start
             (on the top level start = 0 is always valid; below it, an invalid start IS a block that, at the coarser level's
             vector, one key frame does not show).  Frames: a sample is valid when its position lies in [0, (H-1) << 8] x
             [0, (W-1) << 8] (its bilinear footprint then needs no clamp); where exactly one of the two samples is valid the
             output is that sample alone - a hard switch, with a seam where it flips; otherwise the blend above.  k = 0 and
             k = s stay A and B.  Median and per-pixel field are unchanged.

  half-pel   (mci_refine_host, the driver's mci_precision="half"; off by default).  The integer field writes the motion between the
             key frames as 2 d: even.  One more step after the median, no second median: the half-pel plane U(Y) of a luma plane
             is [2h-1, 2w-1], U[Q, P] = (Y[y0,x0] + Y[y0,x1] + Y[y1,x0] + Y[y1,x1] + 2) >> 2 with y0 = Q >> 1,
             y1 = min(y0 + (Q & 1), h-1) and the same for the column (even coordinates are Y; a half position is (a + b + 1) >> 1
             or the four-tap mean).  Every block tries h in 2 d + [-1, 1]^2, cost(h) = sum over the block's pixels p inside the
             image of |U_A(clamp(2p - h)) - U_B(clamp(2p + h))| + LAMBDA_HALF * (|hx| + |hy|), clamped to the half-pel plane
             (LAMBDA_HALF = 2: h = 2 d costs what d costs on level 0); the winner is the minimum of (cost, hx*hx + hy*hy, hy, hx)
             (pack_key_half: |h| <= 159).  border="valid": block_cost_valid's rule in half-pel coordinates - a pixel counts when
             2p - h and 2p + h both lie in [0, 2(w-1)] x [0, 2(h-1)] (ceil(|hx|/2) <= X <= w-1-ceil(|hx|/2), the same in Y: n of
             N), a candidate is valid when 4 n >= N, costs (64 * SAD over those n) // n + LAMBDA_HALF * (|hx| + |hy|), and a block
             whose start 2 d is not valid keeps 2 d.  The result is a field in HALF pixels; mci_frames_host(precision="half")
             reads it: the offsets are (k Dh + s/2) >> log2 s and ((s-k) Dh + s/2) >> log2 s, Dh the same bilinear per-pixel
             field, now in 1/256 of a half pixel - so the field 2 f gives the bytes precision="full" gives for f.  Half-pel
             samples are bilinear and therefore soft; a block whose integer vector is more than one half-pel step from the
             truth stays wrong.

  key frames' size   (mci_frames_scaled_host, the driver's output_size="keyframes"; rib_scaled_frames, tests/test_gpu_mci_scaled.py).  The
             field stays the model-size one; frame k is sampled from the key frame FILES' own pixels [h0, w0, 3]: a pixel's vector is
             the bilinear field at its centre's position in the model's block grid, scaled to output pixels by a 16.16 factor, then
             the lines of "frame k" and "border" above in output coordinates - the function's text has the four steps.  Motion
             detail finer than a model block is not followed.

  person     (mci_field_masked_host / mci_frames_masked_host, the driver's mci_person="exclude"; rib_masked_field / rib_masked_frames,
             tests/test_gpu_mci_person.py; off by default).  ma, mb uint8 [H, W], nonzero = EXCLUDED, for key frame A and B: the
             driver passes the human masks of the two key frames' poses.  Mask pyramid: level l+1 is ceil(h/2) x ceil(w/2), a pixel
             is 1 iff any of its 2x2 parents (clamped as the luma pyramid clamps them) is nonzero.  Masked cost, on every level
             and for either border: a block's pixel p counts for candidate d iff the border rule lets it count (clamp: always;
             valid: the rectangle above) and MA(clamp(p - d)) == 0 and MB(clamp(p + d)) == 0; n the counted pixels, N the block's
             pixels inside the plane; a candidate is valid iff VALID_SHARE * n >= N, costs (64 * SAD over the counted pixels) // n
             + LAMBDA * (|dx| + |dy|), the key is pack_key_wide for every L, the winner the minimum key over the valid candidates;
             a block whose start candidate is not valid is NOT SEARCHED: it keeps its start and a per-block flag says so -
             block_cost_valid / search_valid with a counted n in place of the closed-form rectangle.  Fill, on the TOP level only:
             a block that was not searched takes the vector of the SEARCHED block within Chebyshev distance FILL_RADIUS = 8 that
             minimises (max(|Dy|, |Dx|), |Dy| + |Dx|, Dy, Dx) (D = source - block, in blocks), (0, 0) if there is none; only
             searched blocks are sources, so the result does not depend on the order of evaluation.  Below the top a block that is
             not searched keeps its start - twice the coarser block's vector, by then background motion.  Median and per-pixel
             field are unchanged.  Frames: a sample is CLEAN iff the border rule calls it valid (clamp: always) and the four taps of
             its bilinear footprint in the level-0 mask of its key frame (coordinates clamped as sample_bilinear clamps them) are
             all zero; where exactly one of a pixel's two samples is clean the output is that sample alone, otherwise the blend -
             the "valid" switch with one more condition.  All-zero masks: border="valid" gives mci_field_host's field bit for bit,
             "clamp" gives it when both sides are multiples of 8 << (L-1) (every block full: 64 SAD // 64 = SAD), the frames are
             mci_frames_host's for every shape; all-one masks: the zero field and the plain cross-fade.  Only the person is
             handled, by the reference's coarse pose mask; background hidden in BOTH key frames stays a blend.

  sampler    (sampler="cubic" of the three mci_frames_*_host functions, the driver's mci_sampler; rib_cubic_frames / rib_cubic_scaled,
             tests/test_gpu_mci_cubic.py; "bilinear" by default).  A bilinear sample at a fractional position is a low-pass filter that
             disappears where the offset is a whole pixel (k = 0, k = s, often k = s / 2), so the backgrounds of a clip pulse between
             sharp and soft at the key-frame rate.  "cubic" replaces sample_bilinear by sample_cubic - 4x4 taps, Catmull-Rom (A = -1/2)
             weights in 1/128 per axis (cubic_weights, integers only), tap rows and columns clamped to the frame, acc = sum_r wy[r]
             sum_c wx[c] v[r][c], result clip((acc + 8192) >> 14, 0, 255) - and NOTHING else: offsets, blend, k = 0 / k = s, and the
             border rule (sample_valid looks at the POSITION, so the one-sided pixels are the bilinear sampler's).  Masked: a sample
             is clean iff all 16 clamped taps are clear (sample_clean_cubic): the clean / blend seam moves by a pixel.  Where every
             offset is a whole pixel the bytes are the bilinear sampler's.  Catmull-Rom overshoots at strong edges; the result is
             clamped.  cubic_tile_staged states, from the sample positions alone, which tiles the kernels read from an LDS window
             and which they gather directly; the bytes do not depend on it.

  detail     (mci_detail_field_host, the driver's mci_detail="keyframes"; rib_detail_field, tests/test_gpu_mci_detail.py; "model" by
             default).  Under "key frames' size" the block field holds whole MODEL pixels - multiples of 3.75 output pixels at
             512 -> 1920 - so the two samples of a block are misregistered by up to one quantum and the full-size background is a
             soft double image even where the model-size field is right.  One more search, at the key frames' own size: a block field
             of the full-size key frames, [ceil(h0/8), ceil(w0/8), 2] in whole OUTPUT pixels, every block started from the scaled
             model-size vector at its centre pixel and searched over start + [-R, R]^2 (detail_radius: half the quantum, at most 4)
             on the full-size lumas with the rules above (clamp / valid, the tuple's minimum; pack_key_detail holds +-1268), then
             the median.  The frames are mci_frames_host on the full-size key frames with that field, precision="full": no new
             frame function, no half-pel step at full size (below ratio 2 a model half-pel is finer than a full-size pixel).  The
             model-size floats the generator reads stay the model-size field's.  A wrong model-size vector stays wrong beyond R;
             above ratio 8 R no longer covers the quantum; no interior occlusion reasoning.

  motion     (mci_accel_host / mci_frames_accel_host, the driver's mci_motion="quadratic"; rib_accel_field / rib_accel_frames,
             tests/test_gpu_mci_motion.py; "linear" by default).  Everything above moves a segment's content at constant velocity, so
             across a clip it runs along a polyline whose velocity jumps at every key frame.  "quadratic" is the second-order
             trajectory from three fields: a block's acceleration a is the difference of the NEXT and the PREVIOUS segment's vectors,
             each read at the block the content comes from or goes to (two vectors away: motion-compensated lookups, clamped), one-
             sided (twice the difference to the segment's own vector) where a clip has no segment on one side, 0 where it has none;
             then the 3x3 median.  Frame k: Acc(p) bilinear from that block field exactly as D(p) is, and BOTH samples move by
             c = (UNIT k (s - k) Acc + 2 s^2) >> (2 log2 s + 2) - a t (1 - t) / 2 at t = k / s, zero at the key frames, a / 8 in the
             middle.  Offsets, sampler, blend, border and person rules are unchanged and act on the corrected positions; a zero
             acceleration field gives the linear bytes.  A wrong neighbour field gives a wrong correction: the median is the only guard.

No quarter-pel search, no sub-pel search on the coarse levels, nothing above second order in time, and no occlusion reasoning
beyond the frame border under border="valid" - a foreground object that covers background is not handled
unless the person is excluded (`rib_masked_*`): see DESIGN ("Motion-compensated backgrounds") for what that costs."""
from __future__ import annotations

import numpy as np

BLOCK = 8                 # block side, on every pyramid level
LEVELS = 3                # pyramid levels 0..2: the default
MIN_LEVELS, MAX_LEVELS = 3, 5             # `levels` of mci_field_host / block_field_levels
SEARCH_TOP = 4            # the top level (2 by default): full search over [-4, 4]^2
REFINE = 1                # every level below: start + [-1, 1]^2
LAMBDA = 4                # cost of one pixel of |dx| + |dy| (a block's SAD is at most 64 * 255)
FIELD_FRAC_BITS = 8       # D(p) in 1/256 px: 4 bits of bilinear weight per axis
SAMPLE_FRAC_BITS = 8      # sampling positions in 1/256 px
MAX_DISP = 2 * (2 * SEARCH_TOP + REFINE) + REFINE      # 19: the largest |dx|, |dy| of the level-0 field
KEY_BIAS = 32             # pack_key: dy + 32, dx + 32 in 6 bits each (MAX_DISP < 32)
WIDE_KEY_BIAS = 128       # pack_key_wide: dy + 128, dx + 128 in 8 bits each (max_disp(5) = 79 < 128)
MAX_SAMPLE_RATE = 1024
BORDERS = ("clamp", "valid")              # `border` of the functions below; 0 and 1 of rib_mci_field / rib_mci_frames
RANGES = {32: 3, 64: 4, 128: 5}           # the driver's mci_range (px of motion between the key frames) -> levels
VALID_SHARE = 4           # border="valid": a candidate counts when VALID_SHARE * n >= N
LAMBDA_HALF = 2           # mci_refine_host: cost of one HALF pixel of |hx| + |hy| (h = 2 d costs what d costs on level 0)
HALF_KEY_BIAS = 256       # pack_key_half: hy + 256, hx + 256 in 9 bits each (|h| <= 2 * max_disp(5) + 1 = 159)
PRECISIONS = ("full", "half")             # `precision` of mci_frames_host; the driver's mci_precision
PERSONS = ("keep", "exclude")             # the driver's mci_person: "exclude" = the *_masked_host functions with the key frames' human masks
SAMPLERS = ("bilinear", "cubic")          # `sampler` of the mci_frames_*_host functions; the driver's mci_sampler
CUBIC_TILE = 64           # cubic_tile_staged: a tile is 64 consecutive x of one output row (one wave of k_cubic_frames / k_cubic_scaled)
CUBIC_WIN_ROWS, CUBIC_WIN_COLS = 12, 76   # ... and it is staged when the taps of both its samples fit this window per key frame
FILL_RADIUS = 8           # mci_field_masked_host: a top-level block that was not searched looks this far (Chebyshev, in blocks) for a searched one
DETAILS = ("model", "keyframes")          # the driver's mci_detail: "keyframes" = mci_detail_field_host, the field refined at the key frames' size
DETAIL_MAX_RADIUS = 4     # detail_radius: at most +-4 output pixels around the scaled model-size vector (covers the quantum up to ratio 8)
DETAIL_MAX_DISP = 79 * 16 + DETAIL_MAX_RADIUS          # 1268: max_disp(5) at ratio 16, plus the radius
DETAIL_KEY_BIAS = 2048    # pack_key_detail: dy + 2048, dx + 2048 in 12 bits each (DETAIL_MAX_DISP < 2048)
MOTIONS = ("linear", "quadratic")         # the driver's mci_motion: "quadratic" = mci_accel_host / mci_frames_accel_host, the second-order trajectory


def field_shape(height, width):
    """(Hb, Wb) of the block field of a height x width frame: ceil(H/8), ceil(W/8)."""
    return (int(height) + BLOCK - 1) // BLOCK, (int(width) + BLOCK - 1) // BLOCK


def luma(u8):
    """uint8 [H, W, 3] -> uint8 [H, W]."""
    v = u8.astype(np.int32)
    return ((77 * v[..., 0] + 150 * v[..., 1] + 29 * v[..., 2] + 128) >> 8).astype(np.uint8)


def down2(y):
    """One pyramid step of a uint8 [h, w] plane."""
    h, w = y.shape
    r0, c0 = 2 * np.arange((h + 1) // 2), 2 * np.arange((w + 1) // 2)
    r1, c1 = np.minimum(r0 + 1, h - 1), np.minimum(c0 + 1, w - 1)
    v = y.astype(np.int32)
    return ((v[r0][:, c0] + v[r0][:, c1] + v[r1][:, c0] + v[r1][:, c1] + 2) >> 2).astype(np.uint8)


def check_levels(levels, who):
    if isinstance(levels, bool) or not isinstance(levels, (int, np.integer)) or not MIN_LEVELS <= levels <= MAX_LEVELS:
        raise ValueError("%s: levels must be %d..%d (a range of 32, 64 or 128 px), got %r" % (who, MIN_LEVELS, MAX_LEVELS, levels))
    return int(levels)


def check_border(border, who):
    if not isinstance(border, str) or border not in BORDERS:
        raise ValueError("%s: border must be 'clamp' or 'valid', got %r" % (who, border))
    return border


def check_precision(precision, who):
    if not isinstance(precision, str) or precision not in PRECISIONS:
        raise ValueError("%s: precision must be 'full' or 'half', got %r" % (who, precision))
    return precision


def check_sampler(sampler, who):
    if not isinstance(sampler, str) or sampler not in SAMPLERS:
        raise ValueError("%s: sampler must be 'bilinear' or 'cubic', got %r" % (who, sampler))
    return sampler


def check_settings(background, mci_range, mci_border, resize_on, who="evaluate_from_folder", mci_precision="full", mci_person="keep",
                   output_size="model", mci_sampler="bilinear"):
    """The folder driver's background settings -> (levels, border) for the functions below.
    mci_sampler: "bilinear" (the default) or "cubic" (sampler="cubic" of the mci_frames_*_host functions: sample_cubic in
    place of sample_bilinear); checked here, and the caller's to pass on.
    mci_precision: "full" (the default) or "half" (mci_refine_host after the field, mci_frames_host(precision="half")); checked
    here, and the caller's to pass on.  mci_person: "keep" (the default) or "exclude" (mci_field_masked_host /
    mci_frames_masked_host with the key frames' human masks); refused with mci_precision="half" and with output_size="keyframes",
    which have no masked form yet."""
    if not isinstance(mci_sampler, str) or mci_sampler not in SAMPLERS:
        raise ValueError("%s: mci_sampler must be 'bilinear' or 'cubic', got %r" % (who, mci_sampler))
    if background != "mci" and mci_sampler != "bilinear":
        raise ValueError("%s: mci_sampler is a setting of background='mci'" % who)
    if not isinstance(mci_person, str) or mci_person not in PERSONS:
        raise ValueError("%s: mci_person must be 'keep' or 'exclude', got %r" % (who, mci_person))
    if background != "mci" and mci_person != "keep":
        raise ValueError("%s: mci_person is a setting of background='mci'" % who)
    if mci_person == "exclude" and mci_precision == "half":
        raise ValueError("%s: mci_person='exclude' with mci_precision='half' is not supported yet (the half-pel refinement has no "
                         "masked form: a masked rib_halfpel_refine is the follow-up)" % who)
    if mci_person == "exclude" and output_size == "keyframes":
        raise ValueError("%s: mci_person='exclude' with output_size='keyframes' is not supported yet (rib_scaled_frames has no "
                         "masked form: a masked rib_scaled_frames is the follow-up)" % who)
    if background not in ("dain", "mci"):
        raise ValueError("%s: background must be 'dain' or 'mci', got %r" % (who, background))
    if background == "mci" and resize_on == "gpu":
        raise ValueError("%s: background='mci' with resize_on='gpu' is not supported (there is no DAIN list to "
                         "plan the GPU resize for)" % who)
    if mci_range not in RANGES:
        raise ValueError("%s: mci_range must be 32, 64 or 128 (px of motion between key frames), got %r" % (who, mci_range))
    if background != "mci" and mci_range != 32:
        raise ValueError("%s: mci_range is a setting of background='mci'" % who)
    if not isinstance(mci_border, str) or mci_border not in BORDERS:
        raise ValueError("%s: mci_border must be 'clamp' or 'valid', got %r" % (who, mci_border))
    if background != "mci" and mci_border != "clamp":
        raise ValueError("%s: mci_border is a setting of background='mci'" % who)
    if not isinstance(mci_precision, str) or mci_precision not in PRECISIONS:
        raise ValueError("%s: mci_precision must be 'full' or 'half', got %r" % (who, mci_precision))
    if background != "mci" and mci_precision != "full":
        raise ValueError("%s: mci_precision is a setting of background='mci'" % who)
    return RANGES[mci_range], mci_border


def check_detail(background, output_size, mci_detail="model", who="evaluate_from_folder"):
    """The folder driver's mci_detail, checked beside check_settings (whose parameter list is pinned by tests/test_mci_cubic_cpu.py, so
    the setting has a check of its own): "model" (the default) or "keyframes" (mci_detail_field_host: the block field refined at the
    key frames' own size, the frames then mci_frames_host on the full-size key frames), which needs background="mci" with
    output_size="keyframes" -> mci_detail, the caller's to pass on."""
    if not isinstance(mci_detail, str) or mci_detail not in DETAILS:
        raise ValueError("%s: mci_detail must be 'model' or 'keyframes', got %r" % (who, mci_detail))
    if mci_detail != "model" and (background != "mci" or output_size != "keyframes"):
        raise ValueError("%s: mci_detail='keyframes' is a setting of background='mci' with output_size='keyframes' (the field is "
                         "refined at the key frames' own size)" % who)
    return mci_detail


def check_motion(background, mci_motion="linear", who="evaluate_from_folder", output_size="model", mci_detail="model"):
    """The folder driver's mci_motion, checked beside check_settings and check_detail (check_settings' parameter list is pinned): "linear"
    (the default: constant velocity between two key frames) or "quadratic" (mci_accel_host / mci_frames_accel_host: the second-order
    trajectory from the neighbouring segments' fields), which needs background="mci" -> mci_motion, the caller's to pass on.
    output_size="keyframes" takes it only with mci_detail="keyframes" (the frames are then mci_frames_accel_host on the full-size key
    frames); the scaled frame functions have no acceleration yet."""
    if not isinstance(mci_motion, str) or mci_motion not in MOTIONS:
        raise ValueError("%s: mci_motion must be 'linear' or 'quadratic', got %r" % (who, mci_motion))
    if mci_motion != "linear" and background != "mci":
        raise ValueError("%s: mci_motion is a setting of background='mci'" % who)
    if mci_motion != "linear" and output_size == "keyframes" and mci_detail != "keyframes":
        raise ValueError("%s: mci_motion='quadratic' with output_size='keyframes' needs mci_detail='keyframes' for now (the scaled entries "
                         "take no acceleration: a scaled acceleration in rib_scaled_frames / rib_cubic_scaled is the follow-up)" % who)
    return mci_motion


def max_disp(levels):
    """The largest |dx|, |dy| the level-0 field of a `levels`-level search can hold: 19, 39, 79."""
    d = SEARCH_TOP
    for _ in range(check_levels(levels, "max_disp") - 1):
        d = 2 * d + REFINE
    return d


def pyramid(y, levels=LEVELS):
    out = [y]
    for _ in range(levels - 1):
        out.append(down2(out[-1]))
    return out


def pack_key(cost, dx, dy):
    """The tuple (cost, dx*dx + dy*dy, dy, dx) as one non-negative integer whose order is the tuple's order."""
    return (cost.astype(np.int64) << 22) | ((dx * dx + dy * dy).astype(np.int64) << 12) | ((dy + KEY_BIAS).astype(np.int64) << 6) \
        | (dx + KEY_BIAS).astype(np.int64)


def pack_key_wide(cost, dx, dy):
    """pack_key with room for max_disp(5): cost << 30 | (dx*dx + dy*dy) << 16 | (dy + 128) << 8 | (dx + 128), for
    cost <= 64 * 255 + 4 * 158 < 2^15, dx*dx + dy*dy <= 2 * 79^2 = 12482 < 2^14 and |dx|, |dy| <= 79 < 128.  The same order: the
    tuple's, so the same winner."""
    return (cost.astype(np.int64) << 30) | ((dx * dx + dy * dy).astype(np.int64) << 16) | ((dy + WIDE_KEY_BIAS).astype(np.int64) << 8) \
        | (dx + WIDE_KEY_BIAS).astype(np.int64)


def unpack_key_wide(key):
    """(cost, dx, dy) of a pack_key_wide key."""
    key = np.asarray(key, np.int64)
    return key >> 30, ((key & 255) - WIDE_KEY_BIAS).astype(np.int32), (((key >> 8) & 255) - WIDE_KEY_BIAS).astype(np.int32)


def pack_key_detail(cost, dx, dy):
    """pack_key_wide with room for mci_detail_field_host's vectors (whole pixels of the key frames' own size): cost << 46 |
    (dx*dx + dy*dy) << 24 | (dy + 2048) << 12 | (dx + 2048).  |dx|, |dy| <= DETAIL_MAX_DISP = 79 * 16 + 4 = 1268 from a field in
    whole pixels, and 1276 from one in half pixels (159 half pixels at ratio 16 round to 1272); so cost <= 64 * 255 + 4 * 2 * 1276 =
    26528 < 2^15, dx*dx + dy*dy <= 2 * 1276^2 = 3256352 < 2^22 and the components < 2048: 61 bits, below search_valid's "never"
    (2^62).  The same order: the tuple's, so wherever pack_key_wide holds the candidates the winner is the same."""
    return (cost.astype(np.int64) << 46) | ((dx * dx + dy * dy).astype(np.int64) << 24) | ((dy + DETAIL_KEY_BIAS).astype(np.int64) << 12) \
        | (dx + DETAIL_KEY_BIAS).astype(np.int64)


def unpack_key_detail(key):
    """(cost, dx, dy) of a pack_key_detail key."""
    key = np.asarray(key, np.int64)
    return key >> 46, ((key & 4095) - DETAIL_KEY_BIAS).astype(np.int32), (((key >> 12) & 4095) - DETAIL_KEY_BIAS).astype(np.int32)


def block_cost(ya, yb, dx, dy):
    """cost(d) of every block of one level: ya, yb uint8 [h, w]; dx, dy int [Hb, Wb] -> int64 [Hb, Wb]."""
    h, w = ya.shape
    Hb, Wb = field_shape(h, w)
    px = np.repeat(np.repeat(dx, BLOCK, 0), BLOCK, 1)[:h, :w]
    py = np.repeat(np.repeat(dy, BLOCK, 0), BLOCK, 1)[:h, :w]
    Y, X = np.mgrid[0:h, 0:w]
    a = ya[np.clip(Y - py, 0, h - 1), np.clip(X - px, 0, w - 1)].astype(np.int32)
    b = yb[np.clip(Y + py, 0, h - 1), np.clip(X + px, 0, w - 1)].astype(np.int32)
    sad = np.zeros((Hb * BLOCK, Wb * BLOCK), np.int64)
    sad[:h, :w] = np.abs(a - b)
    return sad.reshape(Hb, BLOCK, Wb, BLOCK).sum((1, 3)) + LAMBDA * (np.abs(dx) + np.abs(dy))


def valid_counts(h, w, dx, dy):
    """border="valid": (n, N) int64 [Hb, Wb] of one level - n the pixels p of each block with p - d and p + d inside the h x w
    plane (the rectangle |dx| <= X <= w-1-|dx|, |dy| <= Y <= h-1-|dy| cut with the block), N the block's pixels inside it."""
    Hb, Wb = field_shape(h, w)
    y0, x0 = BLOCK * np.arange(Hb, dtype=np.int64)[:, None], BLOCK * np.arange(Wb, dtype=np.int64)[None, :]
    y1, x1 = np.minimum(y0 + BLOCK - 1, h - 1), np.minimum(x0 + BLOCK - 1, w - 1)
    ax, ay = np.abs(dx).astype(np.int64), np.abs(dy).astype(np.int64)
    nx = np.maximum(np.minimum(x1, w - 1 - ax) - np.maximum(x0, ax) + 1, 0)
    ny = np.maximum(np.minimum(y1, h - 1 - ay) - np.maximum(y0, ay) + 1, 0)
    return nx * ny, (y1 - y0 + 1) * (x1 - x0 + 1)


def block_cost_valid(ya, yb, dx, dy):
    """border="valid": (cost, valid) of every block of one level - cost(d) = (64 * SAD over the pixels whose two samples are
    both inside the plane) // n + LAMBDA * (|dx| + |dy|), int64 [Hb, Wb] (0 where n = 0); valid = 4 n >= N, bool [Hb, Wb]."""
    h, w = ya.shape
    Hb, Wb = field_shape(h, w)
    px = np.repeat(np.repeat(dx, BLOCK, 0), BLOCK, 1)[:h, :w]
    py = np.repeat(np.repeat(dy, BLOCK, 0), BLOCK, 1)[:h, :w]
    Y, X = np.mgrid[0:h, 0:w]
    inside = (Y - py >= 0) & (Y - py <= h - 1) & (Y + py >= 0) & (Y + py <= h - 1) \
        & (X - px >= 0) & (X - px <= w - 1) & (X + px >= 0) & (X + px <= w - 1)
    a = ya[np.clip(Y - py, 0, h - 1), np.clip(X - px, 0, w - 1)].astype(np.int32)
    b = yb[np.clip(Y + py, 0, h - 1), np.clip(X + px, 0, w - 1)].astype(np.int32)
    sad = np.zeros((Hb * BLOCK, Wb * BLOCK), np.int64)
    sad[:h, :w] = np.where(inside, np.abs(a - b), 0)
    n, N = valid_counts(h, w, dx, dy)
    cost = (64 * sad.reshape(Hb, BLOCK, Wb, BLOCK).sum((1, 3))) // np.maximum(n, 1) + LAMBDA * (np.abs(dx) + np.abs(dy))
    return cost, VALID_SHARE * n >= N


def search_valid(ya, yb, sx, sy, radius):
    """search under border="valid": the minimum pack_key_wide key over the valid candidates; a block whose start candidate
    is not valid keeps its start."""
    never = np.int64(1) << 62
    best = None
    for ddy in range(-radius, radius + 1):
        for ddx in range(-radius, radius + 1):
            dx, dy = sx + ddx, sy + ddy
            cost, ok = block_cost_valid(ya, yb, dx, dy)
            key = np.where(ok, pack_key_wide(np.where(ok, cost, 0), np.where(ok, dx, 0), np.where(ok, dy, 0)), never)
            best = key if best is None else np.minimum(best, key)
    searched = block_cost_valid(ya, yb, sx, sy)[1]
    _, wx, wy = unpack_key_wide(np.where(searched, best, 0))
    return np.where(searched, wx, sx).astype(np.int32), np.where(searched, wy, sy).astype(np.int32)


def search(ya, yb, sx, sy, radius, wide=False, border="clamp"):
    """The winner of start + [-radius, radius]^2 for every block: sx, sy int [Hb, Wb] -> (dx, dy) int32 [Hb, Wb].  wide: the
    key is pack_key_wide (displacements beyond KEY_BIAS); the winner is the tuple's minimum either way.  border="valid": the
    one-sided cost over the valid candidates (always the wide key), see the module's text."""
    if check_border(border, "search") == "valid":
        return search_valid(ya, yb, sx, sy, radius)
    best = None
    pack = pack_key_wide if wide else pack_key
    for ddy in range(-radius, radius + 1):
        for ddx in range(-radius, radius + 1):
            dx, dy = sx + ddx, sy + ddy
            key = pack(block_cost(ya, yb, dx, dy), dx, dy)
            best = key if best is None else np.minimum(best, key)
    if wide:
        return unpack_key_wide(best)[1:]
    return ((best & 63) - KEY_BIAS).astype(np.int32), (((best >> 6) & 63) - KEY_BIAS).astype(np.int32)


def median3(f):
    """3x3 median of an int [Hb, Wb] plane, coordinates clamped at the border."""
    p = np.pad(f, 1, mode="edge")
    Hb, Wb = f.shape
    nine = np.stack([p[j:j + Hb, i:i + Wb] for j in range(3) for i in range(3)])
    return np.sort(nine, axis=0)[4]


def block_field_levels(a_u8, b_u8, levels=LEVELS, border="clamp"):
    """The block fields of levels L-1 .. 0 (L = levels: 3, 4 or 5) before the median: [(dx, dy)] coarse to fine (the tests look
    at them)."""
    levels = check_levels(levels, "block_field_levels")
    check_border(border, "block_field_levels")
    pa, pb = pyramid(luma(a_u8), levels), pyramid(luma(b_u8), levels)
    out = []
    dx = dy = None
    for lvl in range(levels - 1, -1, -1):
        Hb, Wb = field_shape(*pa[lvl].shape)
        if dx is None:
            sx = sy = np.zeros((Hb, Wb), np.int32)
            radius = SEARCH_TOP
        else:
            by, bx = np.arange(Hb) >> 1, np.arange(Wb) >> 1
            sx, sy = 2 * dx[by][:, bx], 2 * dy[by][:, bx]
            radius = REFINE
        dx, dy = search(pa[lvl], pb[lvl], sx, sy, radius, wide=levels > LEVELS, border=border)
        out.append((dx, dy))
    return out


def mci_field_host(a_u8, b_u8, levels=LEVELS, border="clamp"):
    """The block displacement field of a key-frame pair: a_u8, b_u8 uint8 [H, W, 3] (left and right key frame at the model
    size) -> int16 [Hb, Wb, 2], [..., 0] = dx, [..., 1] = dy, in full-size pixels of HALF the motion between the key frames
    (the intermediate frame's pixel p shows A's p - d and B's p + d).  levels: 3 (the default), 4 or 5 pyramid levels, i.e. a
    search over 32, 64 or 128 px of motion between the key frames; |dx|, |dy| <= max_disp(levels).  border: "clamp" (the
    default) or "valid", the one-sided matching at the frame border."""
    levels = check_levels(levels, "mci_field_host")
    check_border(border, "mci_field_host")
    a_u8, b_u8 = np.asarray(a_u8), np.asarray(b_u8)
    if a_u8.dtype != np.uint8 or a_u8.ndim != 3 or a_u8.shape[2] != 3 or a_u8.shape != b_u8.shape or b_u8.dtype != np.uint8:
        raise ValueError("mci_field_host: two uint8 [H, W, 3] frames of one size, got %s %s and %s %s"
                         % (a_u8.dtype, a_u8.shape, b_u8.dtype, b_u8.shape))
    dx, dy = block_field_levels(a_u8, b_u8, levels, border)[-1]
    return np.stack([median3(dx), median3(dy)], -1).astype(np.int16)


def half_plane(y):
    """U(Y): uint8 [h, w] -> uint8 [2h-1, 2w-1], the plane at half-pel positions (even coordinates are Y itself)."""
    h, w = y.shape
    Q, P = np.arange(2 * h - 1), np.arange(2 * w - 1)
    r0, c0 = Q >> 1, P >> 1
    r1, c1 = np.minimum(r0 + (Q & 1), h - 1), np.minimum(c0 + (P & 1), w - 1)
    v = y.astype(np.int32)
    return ((v[r0][:, c0] + v[r0][:, c1] + v[r1][:, c0] + v[r1][:, c1] + 2) >> 2).astype(np.uint8)


def pack_key_half(cost, hx, hy):
    """The tuple (cost, hx*hx + hy*hy, hy, hx) of a half-pel candidate as one integer in the tuple's order: cost << 34 |
    (hx*hx + hy*hy) << 18 | (hy + 256) << 9 | (hx + 256), for cost <= 64 * 255 + 2 * 318 < 2^15, hx*hx + hy*hy <= 2 * 159^2 =
    50562 < 2^16 and |hx|, |hy| <= 159 < 256."""
    return (cost.astype(np.int64) << 34) | ((hx * hx + hy * hy).astype(np.int64) << 18) | ((hy + HALF_KEY_BIAS).astype(np.int64) << 9) \
        | (hx + HALF_KEY_BIAS).astype(np.int64)


def unpack_key_half(key):
    """(cost, hx, hy) of a pack_key_half key."""
    key = np.asarray(key, np.int64)
    return key >> 34, ((key & 511) - HALF_KEY_BIAS).astype(np.int32), (((key >> 9) & 511) - HALF_KEY_BIAS).astype(np.int32)


def valid_counts_half(h, w, hx, hy):
    """valid_counts in half-pel coordinates: the pixels p with 2p - h and 2p + h inside [0, 2(w-1)] x [0, 2(h-1)] are those with
    p -+ ceil(|h| / 2) inside the plane."""
    return valid_counts(h, w, (np.abs(hx) + 1) >> 1, (np.abs(hy) + 1) >> 1)


def block_cost_half(ua, ub, hx, hy, border="clamp"):
    """(cost, valid) of the half-pel candidate (hx, hy) int [Hb, Wb] of every block: ua, ub the half-pel planes [2h-1, 2w-1].
    border="clamp": the SAD over the block's pixels, samples clamped to the half-pel plane, + LAMBDA_HALF's term; valid
    everywhere.  border="valid": block_cost_valid's rule (cost 0 where n = 0)."""
    h, w = (ua.shape[0] + 1) // 2, (ua.shape[1] + 1) // 2
    Hb, Wb = field_shape(h, w)
    px = np.repeat(np.repeat(hx, BLOCK, 0), BLOCK, 1)[:h, :w]
    py = np.repeat(np.repeat(hy, BLOCK, 0), BLOCK, 1)[:h, :w]
    Y, X = np.mgrid[0:h, 0:w]
    ay, ax, by, bx = 2 * Y - py, 2 * X - px, 2 * Y + py, 2 * X + px
    ymax, xmax = 2 * (h - 1), 2 * (w - 1)
    a = ua[np.clip(ay, 0, ymax), np.clip(ax, 0, xmax)].astype(np.int32)
    b = ub[np.clip(by, 0, ymax), np.clip(bx, 0, xmax)].astype(np.int32)
    diff = np.abs(a - b)
    penalty = LAMBDA_HALF * (np.abs(hx) + np.abs(hy))
    sad = np.zeros((Hb * BLOCK, Wb * BLOCK), np.int64)
    if border == "clamp":
        sad[:h, :w] = diff
        return sad.reshape(Hb, BLOCK, Wb, BLOCK).sum((1, 3)) + penalty, np.ones((Hb, Wb), bool)
    inside = (ay >= 0) & (ay <= ymax) & (by >= 0) & (by <= ymax) & (ax >= 0) & (ax <= xmax) & (bx >= 0) & (bx <= xmax)
    sad[:h, :w] = np.where(inside, diff, 0)
    n, N = valid_counts_half(h, w, hx, hy)
    return (64 * sad.reshape(Hb, BLOCK, Wb, BLOCK).sum((1, 3))) // np.maximum(n, 1) + penalty, VALID_SHARE * n >= N


def mci_refine_host(a_u8, b_u8, field, border="clamp"):
    """The half-pel refinement of a block field: a_u8, b_u8 uint8 [H, W, 3], field int16 [Hb, Wb, 2] of mci_field_host (any
    levels; |d| <= max_disp(5)) -> int16 [Hb, Wb, 2] in HALF pixels: for every block the minimum of (cost, hx*hx + hy*hy, hy, hx)
    over h in 2 d + [-1, 1]^2 (see the module's text); border="valid": over the valid candidates, and a block whose start 2 d is
    not valid keeps 2 d.  For mci_frames_host(precision="half")."""
    check_border(border, "mci_refine_host")
    a_u8, b_u8, field = np.asarray(a_u8), np.asarray(b_u8), np.asarray(field)
    if a_u8.dtype != np.uint8 or a_u8.ndim != 3 or a_u8.shape[2] != 3 or a_u8.shape != b_u8.shape or b_u8.dtype != np.uint8:
        raise ValueError("mci_refine_host: two uint8 [H, W, 3] frames of one size, got %s %s and %s %s"
                         % (a_u8.dtype, a_u8.shape, b_u8.dtype, b_u8.shape))
    H, W = a_u8.shape[:2]
    Hb, Wb = field_shape(H, W)
    if tuple(field.shape) != (Hb, Wb, 2) or field.dtype != np.int16:
        raise ValueError("mci_refine_host: the field of a %dx%d frame is int16 [%d, %d, 2], got %s %s" % (H, W, Hb, Wb, field.dtype, tuple(field.shape)))
    if field.size and np.abs(field.astype(np.int32)).max() > max_disp(MAX_LEVELS):
        raise ValueError("mci_refine_host: the field's components must lie in -%d..%d" % (max_disp(MAX_LEVELS), max_disp(MAX_LEVELS)))
    ua, ub = half_plane(luma(a_u8)), half_plane(luma(b_u8))
    sx, sy = 2 * field[..., 0].astype(np.int32), 2 * field[..., 1].astype(np.int32)
    never = np.int64(1) << 62
    best = None
    for ey in range(-REFINE, REFINE + 1):
        for ex in range(-REFINE, REFINE + 1):
            hx, hy = sx + ex, sy + ey
            cost, ok = block_cost_half(ua, ub, hx, hy, border)
            key = np.where(ok, pack_key_half(np.where(ok, cost, 0), hx, hy), never)
            best = key if best is None else np.minimum(best, key)
    searched = block_cost_half(ua, ub, sx, sy, border)[1]
    _, wx, wy = unpack_key_half(np.where(searched, best, 0))
    return np.stack([np.where(searched, wx, sx), np.where(searched, wy, sy)], -1).astype(np.int16)


def pixel_field(field, height, width):
    """D(p) of every pixel: int16 [Hb, Wb, 2] -> (Dx, Dy) int32 [H, W] in 1/256 px."""
    Hb, Wb = field_shape(height, width)
    if tuple(field.shape) != (Hb, Wb, 2):
        raise ValueError("mci: the field of a %dx%d frame is [%d, %d, 2], got %s" % (height, width, Hb, Wb, tuple(field.shape)))
    f = field.astype(np.int32)
    ty, tx = 2 * np.arange(height) - (BLOCK - 1), 2 * np.arange(width) - (BLOCK - 1)     # position in 1/16 block from centre 0
    r0, fy = ty >> 4, (ty & 15)[:, None, None]
    c0, fx = tx >> 4, (tx & 15)[None, :, None]
    r1, r0 = np.clip(r0 + 1, 0, Hb - 1), np.clip(r0, 0, Hb - 1)
    c1, c0 = np.clip(c0 + 1, 0, Wb - 1), np.clip(c0, 0, Wb - 1)
    d = (16 - fy) * ((16 - fx) * f[r0][:, c0] + fx * f[r0][:, c1]) + fy * ((16 - fx) * f[r1][:, c0] + fx * f[r1][:, c1])
    return d[..., 0], d[..., 1]


def sample_bilinear(img, py, px):
    """img uint8 [H, W, 3] at positions (py, px) int32 [H, W] in 1/256 px, edge clamp -> int32 [H, W, 3] in 0..255."""
    h, w = img.shape[:2]
    y0, x0 = py >> SAMPLE_FRAC_BITS, px >> SAMPLE_FRAC_BITS
    fy, fx = (py & 255)[..., None], (px & 255)[..., None]
    y1, y0 = np.clip(y0 + 1, 0, h - 1), np.clip(y0, 0, h - 1)
    x1, x0 = np.clip(x0 + 1, 0, w - 1), np.clip(x0, 0, w - 1)
    v = img.astype(np.int32)
    return ((256 - fy) * ((256 - fx) * v[y0, x0] + fx * v[y0, x1]) + fy * ((256 - fx) * v[y1, x0] + fx * v[y1, x1]) + (1 << 15)) >> 16


def cubic_weights():
    """The Catmull-Rom (A = -1/2) tap weights of sample_cubic at t = f / 256, f = 0..255, in 1/128: int32 [256, 4], integers
    only.  Numerators over 2 * 256^3: n0 = -f^3 + 512 f^2 - 65536 f, n1 = 3 f^3 - 1280 f^2 + 2 * 256^3,
    n2 = -3 f^3 + 1024 f^2 + 65536 f, n3 = f^3 - 256 f^2; w_i = (n_i + 2^17) >> 18 (arithmetic shift); the residual
    128 - sum(w) goes to w1 if w1 >= w2, else to w2.  Every row sums to 128, w[0] = (0, 128, 0, 0), w[128] = (-8, 72, 72, -8),
    the values lie in -9..128, and w[256 - f] is w[f] reversed for every f in 1..255 (tests/test_mci_cubic_cpu.py asserts all of
    it).  The kernels compute the same formula (csrc/mci.hip.h cubic_weight_row); there is no second table."""
    f = np.arange(256, dtype=np.int64)
    n = np.stack([-f ** 3 + 512 * f * f - 65536 * f, 3 * f ** 3 - 1280 * f * f + 2 * 256 ** 3,
                  -3 * f ** 3 + 1024 * f * f + 65536 * f, f ** 3 - 256 * f * f], 1)
    w = (n + (1 << 17)) >> 18
    rest = 128 - w.sum(1)
    first = w[:, 1] >= w[:, 2]
    w[:, 1] += np.where(first, rest, 0)
    w[:, 2] += np.where(first, 0, rest)
    return w.astype(np.int32)


_CUBIC_W = cubic_weights()


def sample_cubic(img, py, px):
    """img uint8 [H, W, 3] at positions (py, px) int32 [...] in 1/256 px -> int32 [..., 3] in 0..255: the 4x4 Catmull-Rom sample.
    Tap rows (py >> 8) - 1 .. + 2 and tap columns (px >> 8) - 1 .. + 2, each clamped to the frame; wy = cubic_weights()[py & 255],
    wx = cubic_weights()[px & 255]; per tap row h_r = sum_c wx[c] v[r][c], acc = sum_r wy[r] h_r, and the result is
    clip((acc + 8192) >> 14, 0, 255) per channel (Catmull-Rom overshoots at strong edges; the clip is part of the definition).
    int32 holds it: sum |w| <= 160 per axis (f = 128), so |h_r| <= 255 * 160 = 40800 and |acc| <= 255 * 160^2 = 6528000 < 2^23
    (the taps' signs cannot all favour one side: the largest |acc| an image can reach is 255 * (144^2 + 16^2) = 5352960)."""
    h, w = img.shape[:2]
    y0, x0 = py >> SAMPLE_FRAC_BITS, px >> SAMPLE_FRAC_BITS
    wy, wx = _CUBIC_W[py & 255], _CUBIC_W[px & 255]
    v = img.astype(np.int32)
    acc = 0
    for r in range(4):
        yr = np.clip(y0 - 1 + r, 0, h - 1)
        hr = 0
        for c in range(4):
            hr = hr + wx[..., c, None] * v[yr, np.clip(x0 - 1 + c, 0, w - 1)]
        acc = acc + wy[..., r, None] * hr
    return np.clip((acc + (1 << 13)) >> 14, 0, 255)


def sample_clean_cubic(mask, py, px):
    """sample_clean for sample_cubic: bool [...], the positions whose 16 taps in `mask` (bool [H, W], set = excluded; rows and
    columns clamped as sample_cubic clamps them) are all clear."""
    h, w = mask.shape
    y0, x0 = py >> SAMPLE_FRAC_BITS, px >> SAMPLE_FRAC_BITS
    hit = False
    for r in range(4):
        yr = np.clip(y0 - 1 + r, 0, h - 1)
        for c in range(4):
            hit = hit | mask[yr, np.clip(x0 - 1 + c, 0, w - 1)]
    return ~hit


def cubic_tile_staged(pay, pax, pby, pbx):
    """The staging rule of k_cubic_frames / k_cubic_scaled as a function of the sample positions alone: pay, pax (the sample of
    key frame A) and pby, pbx (of B), int [H, W] in 1/256 px, of ONE output frame -> bool [H, ceil(W / 64)], True where the tile
    (64 consecutive x of one row; the last may be short) reads its taps from the staged window, False where it gathers them
    directly.  A tile is staged iff, for each key frame, the UNCLAMPED tap rows (p >> 8) - 1 .. + 2 of its pixels span at most
    CUBIC_WIN_ROWS rows and the tap columns at most CUBIC_WIN_COLS columns.  The bytes do not depend on it."""
    pay, pax, pby, pbx = (np.asarray(v) >> SAMPLE_FRAC_BITS for v in (pay, pax, pby, pbx))
    H, W = pay.shape
    tiles = (W + CUBIC_TILE - 1) // CUBIC_TILE
    out = np.ones((H, tiles), bool)
    for t in range(tiles):
        sl = slice(t * CUBIC_TILE, min((t + 1) * CUBIC_TILE, W))
        for ty, tx in ((pay, pax), (pby, pbx)):
            out[:, t] &= (ty[:, sl].max(1) - ty[:, sl].min(1) + 4 <= CUBIC_WIN_ROWS) & (tx[:, sl].max(1) - tx[:, sl].min(1) + 4 <= CUBIC_WIN_COLS)
    return out


def sample_positions(field, sample_rate, k, height, width, precision="full", model_hw=None):
    """(pay, pax, pby, pbx) int32 [h, w] of frame k as mci_frames_host computes them (model_hw given: as mci_frames_scaled_host
    does for height x width key frames): the input of cubic_tile_staged."""
    unit = 1 if check_precision(precision, "sample_positions") == "half" else 2
    s, ls = int(sample_rate), log2_rate(sample_rate)
    Dx, Dy = pixel_field(field, height, width) if model_hw is None else pixel_field_scaled(field, model_hw, (height, width))
    Y, X = np.mgrid[0:height, 0:width]
    Y, X = (Y << SAMPLE_FRAC_BITS).astype(np.int32), (X << SAMPLE_FRAC_BITS).astype(np.int32)
    ax, ay = (unit * k * Dx + s // 2) >> ls, (unit * k * Dy + s // 2) >> ls
    bx, by = (unit * (s - k) * Dx + s // 2) >> ls, (unit * (s - k) * Dy + s // 2) >> ls
    return Y - ay, X - ax, Y + by, X + bx


def log2_rate(sample_rate):
    s = int(sample_rate)
    if s < 1 or s > MAX_SAMPLE_RATE or s & (s - 1):
        raise ValueError("mci: the sample rate must be a power of two in 1..%d, got %r" % (MAX_SAMPLE_RATE, sample_rate))
    return s.bit_length() - 1


def sample_valid(py, px, height, width):
    """border="valid": bool [H, W], the positions (1/256 px) whose bilinear footprint lies inside the frame."""
    return (py >= 0) & (py <= (height - 1) << SAMPLE_FRAC_BITS) & (px >= 0) & (px <= (width - 1) << SAMPLE_FRAC_BITS)


def mci_frames_host(a_u8, b_u8, field, sample_rate, ks, border="clamp", precision="full", sampler="bilinear"):
    """Frames ks (each 0 <= k <= sample_rate; k = 0 is A, k = sample_rate is B) of the segment between the key frames a_u8 and
    b_u8 (uint8 [H, W, 3]) from their block field (mci_field_host) -> uint8 [len(ks), H, W, 3].  border="valid": where exactly
    one of a pixel's two samples lies inside the frame the output is that sample alone.  precision="half": the field is
    mci_refine_host's, in half pixels - the offsets are k Dh / s and (s-k) Dh / s in place of 2k D / s and 2(s-k) D / s.
    sampler="cubic": sample_cubic in place of sample_bilinear and nothing else - the offsets, the blend, the border rule
    (sample_valid: the POSITION lies inside the frame; taps beyond the edge clamp) and k = 0, k = s are unchanged."""
    check_border(border, "mci_frames_host")
    unit = 1 if check_precision(precision, "mci_frames_host") == "half" else 2
    sample = sample_cubic if check_sampler(sampler, "mci_frames_host") == "cubic" else sample_bilinear
    a_u8, b_u8, field = np.asarray(a_u8), np.asarray(b_u8), np.asarray(field)
    if a_u8.dtype != np.uint8 or a_u8.ndim != 3 or a_u8.shape[2] != 3 or a_u8.shape != b_u8.shape or b_u8.dtype != np.uint8:
        raise ValueError("mci_frames_host: two uint8 [H, W, 3] frames of one size, got %s and %s" % (a_u8.shape, b_u8.shape))
    s, ls = int(sample_rate), log2_rate(sample_rate)
    H, W = a_u8.shape[:2]
    Dx, Dy = pixel_field(field, H, W)
    Y, X = np.mgrid[0:H, 0:W]
    Y, X = (Y << SAMPLE_FRAC_BITS).astype(np.int32), (X << SAMPLE_FRAC_BITS).astype(np.int32)
    out = np.empty((len(ks), H, W, 3), np.uint8)
    for j, k in enumerate(ks):
        k = int(k)
        if not 0 <= k <= s:
            raise ValueError("mci_frames_host: frame %d is outside the segment 0..%d" % (k, s))
        ax, ay = (unit * k * Dx + s // 2) >> ls, (unit * k * Dy + s // 2) >> ls
        bx, by = (unit * (s - k) * Dx + s // 2) >> ls, (unit * (s - k) * Dy + s // 2) >> ls
        a = sample(a_u8, Y - ay, X - ax)
        b = sample(b_u8, Y + by, X + bx)
        o = ((s - k) * a + k * b + s // 2) >> ls
        if border == "valid":
            oka, okb = sample_valid(Y - ay, X - ax, H, W)[..., None], sample_valid(Y + by, X + bx, H, W)[..., None]
            o = np.where(oka == okb, o, np.where(oka, a, b))
        out[j] = o.astype(np.uint8)
    return out


# ---- the person kept out (mci_person="exclude"): the module text's "person" paragraph ---------------------------------------

def check_masks(ma, mb, height, width, who):
    """ma, mb -> bool [H, W] (nonzero = excluded)."""
    ma, mb = np.asarray(ma), np.asarray(mb)
    for m in (ma, mb):
        if m.dtype != np.uint8 or tuple(m.shape) != (height, width):
            raise ValueError("%s: the masks of %dx%d key frames are uint8 [%d, %d], got %s %s" % (who, height, width, height, width, m.dtype, tuple(m.shape)))
    return ma != 0, mb != 0


def down2_or(m):
    """One step of the mask pyramid: bool [h, w] -> bool [ceil(h/2), ceil(w/2)], a pixel is set iff any of its 2x2 parents
    (clamped as down2 clamps them) is."""
    h, w = m.shape
    r0, c0 = 2 * np.arange((h + 1) // 2), 2 * np.arange((w + 1) // 2)
    r1, c1 = np.minimum(r0 + 1, h - 1), np.minimum(c0 + 1, w - 1)
    return m[r0][:, c0] | m[r0][:, c1] | m[r1][:, c0] | m[r1][:, c1]


def mask_pyramid(m, levels=LEVELS):
    """uint8 or bool [H, W] (nonzero = excluded) -> [bool planes], level 0 first."""
    out = [np.asarray(m) != 0]
    for _ in range(levels - 1):
        out.append(down2_or(out[-1]))
    return out


def block_cost_masked(ya, yb, ma, mb, dx, dy, border="clamp"):
    """(cost, valid, n) of every block of one level with the excluded pixels left out: block_cost_valid with a counted n.  A
    pixel p counts iff the border rule lets it (clamp: always; valid: p - d and p + d inside the plane) and ma(clamp(p - d)) and
    mb(clamp(p + d)) are both clear; cost = (64 * SAD over the counted pixels) // n + LAMBDA * (|dx| + |dy|) (0 where n = 0),
    valid = VALID_SHARE * n >= N, N the block's pixels inside the plane."""
    h, w = ya.shape
    Hb, Wb = field_shape(h, w)
    px = np.repeat(np.repeat(dx, BLOCK, 0), BLOCK, 1)[:h, :w]
    py = np.repeat(np.repeat(dy, BLOCK, 0), BLOCK, 1)[:h, :w]
    Y, X = np.mgrid[0:h, 0:w]
    ay, ax, by, bx = np.clip(Y - py, 0, h - 1), np.clip(X - px, 0, w - 1), np.clip(Y + py, 0, h - 1), np.clip(X + px, 0, w - 1)
    counts = ~ma[ay, ax] & ~mb[by, bx]
    if border == "valid":
        counts &= (Y - py >= 0) & (Y - py <= h - 1) & (Y + py >= 0) & (Y + py <= h - 1) \
            & (X - px >= 0) & (X - px <= w - 1) & (X + px >= 0) & (X + px <= w - 1)
    a, b = ya[ay, ax].astype(np.int32), yb[by, bx].astype(np.int32)
    sad = np.zeros((Hb * BLOCK, Wb * BLOCK), np.int64)
    sad[:h, :w] = np.where(counts, np.abs(a - b), 0)
    cnt = np.zeros((Hb * BLOCK, Wb * BLOCK), np.int64)
    cnt[:h, :w] = counts
    n = cnt.reshape(Hb, BLOCK, Wb, BLOCK).sum((1, 3))
    N = valid_counts(h, w, np.zeros_like(dx), np.zeros_like(dy))[1]
    cost = (64 * sad.reshape(Hb, BLOCK, Wb, BLOCK).sum((1, 3))) // np.maximum(n, 1) + LAMBDA * (np.abs(dx) + np.abs(dy))
    return cost, VALID_SHARE * n >= N, n


def search_masked(ya, yb, ma, mb, sx, sy, radius, border="clamp"):
    """search_valid over block_cost_masked -> (dx, dy int32 [Hb, Wb], searched bool [Hb, Wb]): the minimum pack_key_wide key over
    the valid candidates; a block whose start candidate is not valid is not searched and keeps its start."""
    never = np.int64(1) << 62
    best = None
    for ddy in range(-radius, radius + 1):
        for ddx in range(-radius, radius + 1):
            dx, dy = sx + ddx, sy + ddy
            cost, ok, _ = block_cost_masked(ya, yb, ma, mb, dx, dy, border)
            key = np.where(ok, pack_key_wide(np.where(ok, cost, 0), np.where(ok, dx, 0), np.where(ok, dy, 0)), never)
            best = key if best is None else np.minimum(best, key)
    searched = block_cost_masked(ya, yb, ma, mb, sx, sy, border)[1]
    _, wx, wy = unpack_key_wide(np.where(searched, best, 0))
    return np.where(searched, wx, sx).astype(np.int32), np.where(searched, wy, sy).astype(np.int32), searched


def fill_unsearched(dx, dy, searched, radius=FILL_RADIUS):
    """The top level's fill: a block that was not searched takes the vector of the searched block within Chebyshev distance
    `radius` that minimises (max(|Dy|, |Dx|), |Dy| + |Dx|, Dy, Dx), D = source - block; none: (0, 0).  Searched blocks keep
    theirs.  Only the INPUT's searched blocks are sources."""
    Hb, Wb = searched.shape
    ox, oy = np.where(searched, dx, 0).astype(np.int32), np.where(searched, dy, 0).astype(np.int32)
    for by, bx in zip(*np.nonzero(~searched)):
        best = None
        for sy in range(max(by - radius, 0), min(by + radius, Hb - 1) + 1):
            for sx in range(max(bx - radius, 0), min(bx + radius, Wb - 1) + 1):
                if searched[sy, sx]:
                    ddy, ddx = int(sy - by), int(sx - bx)
                    key = (max(abs(ddy), abs(ddx)), abs(ddy) + abs(ddx), ddy, ddx)
                    if best is None or key < best:
                        best = key
        if best is not None:
            ox[by, bx], oy[by, bx] = dx[by + best[2], bx + best[3]], dy[by + best[2], bx + best[3]]
    return ox, oy


def block_field_levels_masked(a_u8, b_u8, ma, mb, levels=LEVELS, border="clamp"):
    """block_field_levels with the excluded pixels left out: [(dx, dy, searched)] coarse to fine, before the median; the top
    level's (dx, dy) are those after the fill (what the level below starts from), `searched` the flags before it."""
    levels = check_levels(levels, "block_field_levels_masked")
    check_border(border, "block_field_levels_masked")
    pa, pb = pyramid(luma(a_u8), levels), pyramid(luma(b_u8), levels)
    qa, qb = mask_pyramid(ma, levels), mask_pyramid(mb, levels)
    out = []
    dx = dy = None
    for lvl in range(levels - 1, -1, -1):
        Hb, Wb = field_shape(*pa[lvl].shape)
        if dx is None:
            sx = sy = np.zeros((Hb, Wb), np.int32)
            dx, dy, searched = search_masked(pa[lvl], pb[lvl], qa[lvl], qb[lvl], sx, sy, SEARCH_TOP, border)
            dx, dy = fill_unsearched(dx, dy, searched)
        else:
            by, bx = np.arange(Hb) >> 1, np.arange(Wb) >> 1
            sx, sy = 2 * dx[by][:, bx], 2 * dy[by][:, bx]
            dx, dy, searched = search_masked(pa[lvl], pb[lvl], qa[lvl], qb[lvl], sx, sy, REFINE, border)
        out.append((dx, dy, searched))
    return out


def mci_field_masked_host(a_u8, b_u8, ma, mb, levels=LEVELS, border="clamp"):
    """mci_field_host with the person kept out of the matching: ma, mb uint8 [H, W], nonzero = excluded, for key frame A and B
    (the module text's "person" paragraph) -> int16 [Hb, Wb, 2]."""
    levels = check_levels(levels, "mci_field_masked_host")
    check_border(border, "mci_field_masked_host")
    a_u8, b_u8 = np.asarray(a_u8), np.asarray(b_u8)
    if a_u8.dtype != np.uint8 or a_u8.ndim != 3 or a_u8.shape[2] != 3 or a_u8.shape != b_u8.shape or b_u8.dtype != np.uint8:
        raise ValueError("mci_field_masked_host: two uint8 [H, W, 3] frames of one size, got %s %s and %s %s"
                         % (a_u8.dtype, a_u8.shape, b_u8.dtype, b_u8.shape))
    ma, mb = check_masks(ma, mb, a_u8.shape[0], a_u8.shape[1], "mci_field_masked_host")
    dx, dy, _ = block_field_levels_masked(a_u8, b_u8, ma, mb, levels, border)[-1]
    return np.stack([median3(dx), median3(dy)], -1).astype(np.int16)


def sample_clean(mask, py, px):
    """bool [H, W]: the positions (1/256 px) whose four bilinear taps in `mask` (bool [H, W], set = excluded; coordinates
    clamped as sample_bilinear clamps them) are all clear."""
    h, w = mask.shape
    y0, x0 = py >> SAMPLE_FRAC_BITS, px >> SAMPLE_FRAC_BITS
    y1, y0 = np.clip(y0 + 1, 0, h - 1), np.clip(y0, 0, h - 1)
    x1, x0 = np.clip(x0 + 1, 0, w - 1), np.clip(x0, 0, w - 1)
    return ~(mask[y0, x0] | mask[y0, x1] | mask[y1, x0] | mask[y1, x1])


def mci_frames_masked_host(a_u8, b_u8, ma, mb, field, sample_rate, ks, border="clamp", precision="full", sampler="bilinear"):
    """mci_frames_host with the person kept out: a sample is clean iff the border rule calls it valid (clamp: always) and
    sample_clean holds in its key frame's mask; where exactly one of a pixel's two samples is clean the output is that sample
    alone, otherwise the blend.  k = 0 and k = sample_rate stay A and B.  -> uint8 [len(ks), H, W, 3].  sampler="cubic":
    sample_cubic, and a sample is clean iff all 16 of its taps are clear (sample_clean_cubic)."""
    check_border(border, "mci_frames_masked_host")
    unit = 1 if check_precision(precision, "mci_frames_masked_host") == "half" else 2
    sample = sample_cubic if check_sampler(sampler, "mci_frames_masked_host") == "cubic" else sample_bilinear
    clean = sample_clean_cubic if sampler == "cubic" else sample_clean
    a_u8, b_u8, field = np.asarray(a_u8), np.asarray(b_u8), np.asarray(field)
    if a_u8.dtype != np.uint8 or a_u8.ndim != 3 or a_u8.shape[2] != 3 or a_u8.shape != b_u8.shape or b_u8.dtype != np.uint8:
        raise ValueError("mci_frames_masked_host: two uint8 [H, W, 3] frames of one size, got %s and %s" % (a_u8.shape, b_u8.shape))
    s, ls = int(sample_rate), log2_rate(sample_rate)
    H, W = a_u8.shape[:2]
    ma, mb = check_masks(ma, mb, H, W, "mci_frames_masked_host")
    Dx, Dy = pixel_field(field, H, W)
    Y, X = np.mgrid[0:H, 0:W]
    Y, X = (Y << SAMPLE_FRAC_BITS).astype(np.int32), (X << SAMPLE_FRAC_BITS).astype(np.int32)
    out = np.empty((len(ks), H, W, 3), np.uint8)
    for j, k in enumerate(ks):
        k = int(k)
        if not 0 <= k <= s:
            raise ValueError("mci_frames_masked_host: frame %d is outside the segment 0..%d" % (k, s))
        ax, ay = (unit * k * Dx + s // 2) >> ls, (unit * k * Dy + s // 2) >> ls
        bx, by = (unit * (s - k) * Dx + s // 2) >> ls, (unit * (s - k) * Dy + s // 2) >> ls
        a = sample(a_u8, Y - ay, X - ax)
        b = sample(b_u8, Y + by, X + bx)
        o = ((s - k) * a + k * b + s // 2) >> ls
        oka, okb = clean(ma, Y - ay, X - ax), clean(mb, Y + by, X + bx)
        if border == "valid":
            oka, okb = oka & sample_valid(Y - ay, X - ax, H, W), okb & sample_valid(Y + by, X + bx, H, W)
        oka, okb = oka[..., None], okb[..., None]
        o = np.where(oka == okb, o, np.where(oka, a, b))
        if k == 0 or k == s:                # the key frames themselves, whatever their masks
            o = a if k == 0 else b
        out[j] = o.astype(np.uint8)
    return out


SCALED_MAX_RATIO = 16     # mci_frames_scaled_host: the key frames' sides are within 1/16 .. 16 times the model's
SCALED_MAX_SIDE = 16384   # ... and every side lies in 1..16384
SCALE_FRAC_BITS = 16      # the model -> output scale factors SX, SY are 16.16


def scaled_factors(model_hw, out_hw, who="mci_frames_scaled_host"):
    """(SY, SX) of mci_frames_scaled_host, 16.16: round(h0 / H * 65536), round(w0 / W * 65536); the bounds are checked here."""
    (H, W), (h0, w0) = (int(v) for v in model_hw), (int(v) for v in out_hw)
    if not all(1 <= v <= SCALED_MAX_SIDE for v in (H, W, h0, w0)):
        raise ValueError("%s: every side must lie in 1..%d, got model %dx%d, key frames %dx%d" % (who, SCALED_MAX_SIDE, H, W, h0, w0))
    if w0 > SCALED_MAX_RATIO * W or W > SCALED_MAX_RATIO * w0 or h0 > SCALED_MAX_RATIO * H or H > SCALED_MAX_RATIO * h0:
        raise ValueError("%s: the key frames (%dx%d) must be within 1/%d .. %d times the model size (%dx%d) on each axis"
                         % (who, h0, w0, SCALED_MAX_RATIO, SCALED_MAX_RATIO, H, W))
    return ((h0 << SCALE_FRAC_BITS) + H // 2) // H, ((w0 << SCALE_FRAC_BITS) + W // 2) // W


def pixel_field_scaled(field, model_hw, out_hw):
    """D(p) of every pixel of an h0 x w0 frame from the block field of the H x W model frame, in 1/256 px of the OUTPUT frame:
    int16 [Hb, Wb, 2] -> (DSx, DSy) int32 [h0, w0].  Steps 1-3 of mci_frames_scaled_host."""
    (H, W), (h0, w0) = (int(v) for v in model_hw), (int(v) for v in out_hw)
    SY, SX = scaled_factors((H, W), (h0, w0))
    Hb, Wb = field_shape(H, W)
    if tuple(field.shape) != (Hb, Wb, 2):
        raise ValueError("mci_frames_scaled_host: the field of a %dx%d model frame is [%d, %d, 2], got %s" % (H, W, Hb, Wb, tuple(field.shape)))
    f = field.astype(np.int32)
    ty = ((2 * np.arange(h0, dtype=np.int64) + 1) * H * 16) // h0 - 128      # position in 1/256 block from centre 0
    tx = ((2 * np.arange(w0, dtype=np.int64) + 1) * W * 16) // w0 - 128
    r0, fy = ty >> 8, (ty & 255).astype(np.int32)[:, None, None]
    c0, fx = tx >> 8, (tx & 255).astype(np.int32)[None, :, None]
    r1, r0 = np.clip(r0 + 1, 0, Hb - 1), np.clip(r0, 0, Hb - 1)
    c1, c0 = np.clip(c0 + 1, 0, Wb - 1), np.clip(c0, 0, Wb - 1)
    d16 = (256 - fy) * ((256 - fx) * f[r0][:, c0] + fx * f[r0][:, c1]) + fy * ((256 - fx) * f[r1][:, c0] + fx * f[r1][:, c1])
    d8 = ((d16 + 128) >> 8).astype(np.int64)                                  # 1/256 model px
    dsx = ((d8[..., 0] * SX + (1 << 15)) >> SCALE_FRAC_BITS).astype(np.int32)
    dsy = ((d8[..., 1] * SY + (1 << 15)) >> SCALE_FRAC_BITS).astype(np.int32)
    return dsx, dsy


def mci_frames_scaled_host(a0_u8, b0_u8, field, model_hw, sample_rate, ks, border="clamp", precision="full", sampler="bilinear"):
    """mci_frames_host at the key frames' OWN size: "field at the model size, samples at the key frames' size".  a0_u8, b0_u8
    uint8 [h0, w0, 3] are the key frame files' pixels, field the int16 [Hb, Wb, 2] block field of the model-size key frames
    (mci_field_host / mci_refine_host of the H x W frames, model_hw = (H, W)) -> uint8 [len(ks), h0, w0, 3].  Per output pixel
    (Y0, X0):
      1  TX = ((2 X0 + 1) * W * 16) // w0 - 128, the pixel centre's position in 1/256 block from block centre 0 (TY with H, h0);
         c0 = TX >> 8, fx = TX & 255, c0 and c0 + 1 clamped to the field (rows the same);
      2  D16 = (256-fy) ((256-fx) f00 + fx f01) + fy ((256-fx) f10 + fx f11) per component, D8 = (D16 + 128) >> 8: 1/256 model px;
      3  SX = (w0 * 65536 + W // 2) // W (SY with h0, H), DSx = (D8x * SX + 32768) >> 16 (64-bit product): 1/256 px of the output;
      4  mci_frames_host's lines with DSx, DSy, h0, w0: offsets (unit k DS + s/2) >> log2 s, sample_bilinear, the blend, and under
         border="valid" sample_valid in output coordinates.
    With (h0, w0) == (H, W) it is mci_frames_host, byte for byte.  The sides lie in 1..16384 and within a factor 16 of the
    model's (the largest unit * k * DS then stays below 2^31).  sampler="cubic": sample_cubic in step 4, nothing else."""
    check_border(border, "mci_frames_scaled_host")
    unit = 1 if check_precision(precision, "mci_frames_scaled_host") == "half" else 2
    sample = sample_cubic if check_sampler(sampler, "mci_frames_scaled_host") == "cubic" else sample_bilinear
    a0_u8, b0_u8, field = np.asarray(a0_u8), np.asarray(b0_u8), np.asarray(field)
    if a0_u8.dtype != np.uint8 or a0_u8.ndim != 3 or a0_u8.shape[2] != 3 or a0_u8.shape != b0_u8.shape or b0_u8.dtype != np.uint8:
        raise ValueError("mci_frames_scaled_host: two uint8 [h0, w0, 3] frames of one size, got %s and %s" % (a0_u8.shape, b0_u8.shape))
    s, ls = int(sample_rate), log2_rate(sample_rate)
    h0, w0 = a0_u8.shape[:2]
    Dx, Dy = pixel_field_scaled(field, model_hw, (h0, w0))
    Y, X = np.mgrid[0:h0, 0:w0]
    Y, X = (Y << SAMPLE_FRAC_BITS).astype(np.int32), (X << SAMPLE_FRAC_BITS).astype(np.int32)
    out = np.empty((len(ks), h0, w0, 3), np.uint8)
    for j, k in enumerate(ks):
        k = int(k)
        if not 0 <= k <= s:
            raise ValueError("mci_frames_scaled_host: frame %d is outside the segment 0..%d" % (k, s))
        ax, ay = (unit * k * Dx + s // 2) >> ls, (unit * k * Dy + s // 2) >> ls
        bx, by = (unit * (s - k) * Dx + s // 2) >> ls, (unit * (s - k) * Dy + s // 2) >> ls
        a = sample(a0_u8, Y - ay, X - ax)
        b = sample(b0_u8, Y + by, X + bx)
        o = ((s - k) * a + k * b + s // 2) >> ls
        if border == "valid":
            oka, okb = sample_valid(Y - ay, X - ax, h0, w0)[..., None], sample_valid(Y + by, X + bx, h0, w0)[..., None]
            o = np.where(oka == okb, o, np.where(oka, a, b))
        out[j] = o.astype(np.uint8)
    return out


def detail_radius(model_hw, out_hw):
    """The search radius of mci_detail_field_host in output pixels: min(4, max(1, (c + 1) // 2)) with c = max(ceil(w0 / W),
    ceil(h0 / H)) - half the model-pixel quantum: 1 up to ratio 2, 2 up to 4, 3 up to 6, 4 beyond (512 -> 1920: 2).  The cap is a
    limit: above ratio 8 the search no longer covers the quantum."""
    (H, W), (h0, w0) = (int(v) for v in model_hw), (int(v) for v in out_hw)
    scaled_factors((H, W), (h0, w0), "detail_radius")
    c = max((w0 + W - 1) // W, (h0 + H - 1) // H)
    return min(DETAIL_MAX_RADIUS, max(1, (c + 1) // 2))


def detail_start(field, model_hw, out_hw, precision="full"):
    """The start vectors of mci_detail_field_host: (sx, sy) int32 [H0b, W0b], pixel_field_scaled at every full-size block's pixel
    (min(8 by + 4, h0 - 1), min(8 bx + 4, w0 - 1)), rounded to whole output pixels of d: (DS + 128) >> 8, or (DS + 256) >> 9 where
    the field is in half pixels."""
    h0, w0 = (int(v) for v in out_hw)
    H0b, W0b = field_shape(h0, w0)
    dsx, dsy = pixel_field_scaled(np.asarray(field), model_hw, (h0, w0))
    ys, xs = np.minimum(BLOCK * np.arange(H0b) + 4, h0 - 1), np.minimum(BLOCK * np.arange(W0b) + 4, w0 - 1)
    dsx, dsy = dsx[ys][:, xs], dsy[ys][:, xs]
    if check_precision(precision, "detail_start") == "half":
        return (dsx + 256) >> 9, (dsy + 256) >> 9
    return (dsx + 128) >> 8, (dsy + 128) >> 8


def search_detail(ya, yb, sx, sy, radius, border="clamp"):
    """search(..., wide=True, border) with pack_key_detail in place of pack_key_wide: the same cost functions, the same tuple, the
    same rules ("valid": the minimum over the valid candidates, and a block whose start is not valid keeps its start), room for
    |d| <= DETAIL_MAX_DISP.  Where pack_key_wide holds every candidate (|d| <= max_disp(5) = 79: its |d|^2 field has 14 bits) the winners
    are search's."""
    valid = check_border(border, "search_detail") == "valid"
    never = np.int64(1) << 62
    best = None
    for ddy in range(-radius, radius + 1):
        for ddx in range(-radius, radius + 1):
            dx, dy = sx + ddx, sy + ddy
            if valid:
                cost, ok = block_cost_valid(ya, yb, dx, dy)
                key = np.where(ok, pack_key_detail(np.where(ok, cost, 0), dx, dy), never)
            else:
                key = pack_key_detail(block_cost(ya, yb, dx, dy), dx, dy)
            best = key if best is None else np.minimum(best, key)
    if not valid:
        return unpack_key_detail(best)[1:]
    searched = block_cost_valid(ya, yb, sx, sy)[1]
    _, wx, wy = unpack_key_detail(np.where(searched, best, 0))
    return np.where(searched, wx, sx).astype(np.int32), np.where(searched, wy, sy).astype(np.int32)


def mci_detail_field_host(a0_u8, b0_u8, field, model_hw, border="clamp", precision="full"):
    """The block field of the FULL-SIZE key frames (the driver's mci_detail="keyframes"; rib_detail_field, bit-equal): a0_u8, b0_u8
    uint8 [h0, w0, 3] the key frame files' pixels, field int16 [Hb, Wb, 2] the block field of the model-size (model_hw = (H, W))
    key frames - mci_field_host's, or with precision="half" mci_refine_host's in half pixels - -> int16 [H0b, W0b, 2], H0b =
    ceil(h0 / 8), W0b = ceil(w0 / 8), in WHOLE OUTPUT pixels of half the motion: mci_field_host's meaning at that size.
      start   detail_start: the scaled per-pixel field at the block's pixel (min(8 by + 4, h0 - 1), min(8 bx + 4, w0 - 1)),
              rounded to whole pixels;
      search  start + [-R, R]^2, R = detail_radius(model_hw, (h0, w0)), on luma(a0_u8), luma(b0_u8) with the module's rules:
              "clamp" block_cost and the minimum of (cost, dx*dx + dy*dy, dy, dx); "valid" search_valid's one-sided cost,
              4 n >= N, and a block whose start is not valid keeps its start; the key is pack_key_detail;
      median  median3 per component.
    The frames at the key frames' size are mci_frames_host(a0_u8, b0_u8, F0, s, ks, border, precision="full", sampler): the
    EXISTING definition with the existing samplers - there is no new frame function, and no half-pel step at full size.  Its
    int32 offsets hold the longest vector: 2 * 1024 * 1268 * 256 < 2^31.  The field's components must lie in -79..79 (-159..159
    in half pixels), max_disp(5)'s; the result's lie within +-1268."""
    check_border(border, "mci_detail_field_host")
    half = check_precision(precision, "mci_detail_field_host") == "half"
    a0_u8, b0_u8, field = np.asarray(a0_u8), np.asarray(b0_u8), np.asarray(field)
    if a0_u8.dtype != np.uint8 or a0_u8.ndim != 3 or a0_u8.shape[2] != 3 or a0_u8.shape != b0_u8.shape or b0_u8.dtype != np.uint8:
        raise ValueError("mci_detail_field_host: two uint8 [h0, w0, 3] frames of one size, got %s %s and %s %s"
                         % (a0_u8.dtype, a0_u8.shape, b0_u8.dtype, b0_u8.shape))
    h0, w0 = a0_u8.shape[:2]
    H, W = (int(v) for v in model_hw)
    radius = detail_radius((H, W), (h0, w0))
    Hb, Wb = field_shape(H, W)
    if tuple(field.shape) != (Hb, Wb, 2) or field.dtype != np.int16:
        raise ValueError("mci_detail_field_host: the field of a %dx%d model frame is int16 [%d, %d, 2], got %s %s"
                         % (H, W, Hb, Wb, field.dtype, tuple(field.shape)))
    lim = max_disp(MAX_LEVELS) * 2 + 1 if half else max_disp(MAX_LEVELS)
    if field.size and np.abs(field.astype(np.int32)).max() > lim:
        raise ValueError("mci_detail_field_host: the field's components must lie in -%d..%d" % (lim, lim))
    sx, sy = detail_start(field, (H, W), (h0, w0), precision)
    dx, dy = search_detail(luma(a0_u8), luma(b0_u8), sx.astype(np.int32), sy.astype(np.int32), radius, border)
    return np.stack([median3(dx), median3(dy)], -1).astype(np.int16)


# ---- quadratic motion across key frames (mci_motion="quadratic"): the module text's "motion" paragraph ------------------------------

ACCEL_MAX = 4 * (DETAIL_MAX_DISP + 8)     # 5104: the largest |component| of mci_accel_host (fields within +-1276, pack_key_detail's bound)


def mci_accel_host(f_prev, f, f_next, unit_shift=0):
    """The block acceleration field of one segment (rib_accel_field, bit-equal): f int16 [Hb, Wb, 2] the segment's block field
    (mci_field_host / mci_field_masked_host / mci_detail_field_host in whole pixels, unit_shift = 0; mci_refine_host's in half pixels,
    unit_shift = 1), f_prev and f_next the fields of the segments before and after it, same shape and unit, either None ->
    int16 [Hb, Wb, 2] in the FIELD'S unit.  Per block (by, bx) with vector (fx, fy) = f[by, bx] >> unit_shift (whole pixels, floor):
      lookups  motion compensated: the previous field at block (clamp((8 by + 4 - 2 fy) >> 3), clamp((8 bx + 4 - 2 fx) >> 3)), the next
               one at (clamp((8 by + 4 + 2 fy) >> 3), clamp((8 bx + 4 + 2 fx) >> 3)) - what passes this block's centre was two vectors
               away one segment earlier, and will be two vectors on one segment later;
      both     a = next - prev: (v_next - v_prev) / 2 with v = 2 f the motion across a segment;
      one      only next: a = 2 (next - f); only prev: a = 2 (f - prev); neither: a = 0;
      median   median3 per component.
    a is the change of a segment's motion from one segment to the next in pixels (UNIT * a / 2 with mci_frames_host's UNIT).
    Bound: |a| <= 4 max|f|: 316 from max_disp(5), 636 from its half-pel field, ACCEL_MAX = 5104 from the +-1276 that pack_key_detail
    holds for the fields of the key frames' size - int16 holds it, and the fields' components must lie within +-1276."""
    f = np.asarray(f)
    if f.dtype != np.int16 or f.ndim != 3 or f.shape[2] != 2 or f.size == 0:
        raise ValueError("mci_accel_host: the field is int16 [Hb, Wb, 2], got %s %s" % (f.dtype, tuple(f.shape)))
    if unit_shift not in (0, 1):
        raise ValueError("mci_accel_host: unit_shift is 0 (whole pixels) or 1 (half pixels), got %r" % (unit_shift,))
    Hb, Wb = f.shape[:2]
    side = []
    for g in (f_prev, f_next):
        g = None if g is None else np.asarray(g)
        if g is not None and (g.dtype != np.int16 or g.shape != f.shape):
            raise ValueError("mci_accel_host: a neighbour's field is int16 %s like the segment's, got %s %s" % (tuple(f.shape), g.dtype, tuple(g.shape)))
        side.append(g)
    for g in [f] + [g for g in side if g is not None]:
        if np.abs(g.astype(np.int32)).max() > ACCEL_MAX // 4:
            raise ValueError("mci_accel_host: the fields' components must lie in -%d..%d" % (ACCEL_MAX // 4, ACCEL_MAX // 4))
    cur = f.astype(np.int32)
    wx, wy = cur[..., 0] >> unit_shift, cur[..., 1] >> unit_shift
    by, bx = np.mgrid[0:Hb, 0:Wb]

    def at(g, sign):
        return g.astype(np.int32)[np.clip((BLOCK * by + 4 + sign * 2 * wy) >> 3, 0, Hb - 1), np.clip((BLOCK * bx + 4 + sign * 2 * wx) >> 3, 0, Wb - 1)]
    prev, nxt = side
    if prev is not None and nxt is not None:
        a = at(nxt, 1) - at(prev, -1)
    elif nxt is not None:
        a = 2 * (at(nxt, 1) - cur)
    elif prev is not None:
        a = 2 * (cur - at(prev, -1))
    else:
        a = np.zeros_like(cur)
    return np.stack([median3(a[..., 0]), median3(a[..., 1])], -1).astype(np.int16)


def accel_correction(accel, sample_rate, k, height, width, precision="full"):
    """(cx, cy) int32 [H, W], 1/256 px: what mci_frames_accel_host adds to BOTH sample positions of frame k.  Acc(p) is pixel_field of
    the block acceleration field (bilinear between the block centres, exact in 1/256 of the field's unit); c = (UNIT * k * (s - k) * Acc +
    2 s^2) >> (2 log2 s + 2), the product in 64 bits, the shift arithmetic (floor): a t (1 - t) / 2 at t = k / s, rounded."""
    unit = 1 if check_precision(precision, "accel_correction") == "half" else 2
    s, ls = int(sample_rate), log2_rate(sample_rate)
    Ax, Ay = pixel_field(np.asarray(accel), height, width)
    m = np.int64(unit * int(k) * (s - int(k)))
    return tuple(((m * A.astype(np.int64) + 2 * s * s) >> (2 * ls + 2)).astype(np.int32) for A in (Ax, Ay))


def mci_frames_accel_host(a_u8, b_u8, field, accel, sample_rate, ks, border="clamp", precision="full", sampler="bilinear", ma=None, mb=None):
    """mci_frames_host (ma, mb None) / mci_frames_masked_host (both given) on a second-order trajectory (rib_accel_frames, bit-equal):
    accel int16 [Hb, Wb, 2] is mci_accel_host's field of the segment, in `field`'s unit.  A point that moves x(tau) = x0 + u tau +
    a tau^2 / 2 with x(1) - x(0) = UNIT D and passes the pixel p at t = k / s was at x(0) = p - t UNIT D + c and will be at
    x(1) = p + (1 - t) UNIT D + c, c = a t (1 - t) / 2: BOTH samples move by the same correction (accel_correction), which vanishes at
    k = 0 and k = s and is a / 8 in the middle.  A is sampled at p - off_a + c, B at p + off_b + c, off_a and off_b mci_frames_host's
    rounded offsets; the sampler, the blend, the k = 0 / k = s rule, the "valid" switch and the clean-sample switch act on those
    positions as they do there.  accel all zero: the bytes of mci_frames_host / mci_frames_masked_host, for every shape and setting.
    -> uint8 [len(ks), H, W, 3]."""
    who = "mci_frames_accel_host"
    check_border(border, who)
    unit = 1 if check_precision(precision, who) == "half" else 2
    cubic = check_sampler(sampler, who) == "cubic"
    sample = sample_cubic if cubic else sample_bilinear
    a_u8, b_u8, field, accel = np.asarray(a_u8), np.asarray(b_u8), np.asarray(field), np.asarray(accel)
    if a_u8.dtype != np.uint8 or a_u8.ndim != 3 or a_u8.shape[2] != 3 or a_u8.shape != b_u8.shape or b_u8.dtype != np.uint8:
        raise ValueError("%s: two uint8 [H, W, 3] frames of one size, got %s and %s" % (who, a_u8.shape, b_u8.shape))
    if (ma is None) != (mb is None):
        raise ValueError("%s: the masks are given together or not at all" % who)
    s, ls = int(sample_rate), log2_rate(sample_rate)
    H, W = a_u8.shape[:2]
    if accel.dtype != np.int16 or accel.shape != field.shape:
        raise ValueError("%s: the acceleration field is int16 %s like the block field, got %s %s" % (who, tuple(field.shape), accel.dtype, tuple(accel.shape)))
    masked = ma is not None
    if masked:
        ma, mb = check_masks(ma, mb, H, W, who)
        clean = sample_clean_cubic if cubic else sample_clean
    Dx, Dy = pixel_field(field, H, W)
    Y, X = np.mgrid[0:H, 0:W]
    Y, X = (Y << SAMPLE_FRAC_BITS).astype(np.int32), (X << SAMPLE_FRAC_BITS).astype(np.int32)
    out = np.empty((len(ks), H, W, 3), np.uint8)
    for j, k in enumerate(ks):
        k = int(k)
        if not 0 <= k <= s:
            raise ValueError("%s: frame %d is outside the segment 0..%d" % (who, k, s))
        cx, cy = accel_correction(accel, s, k, H, W, precision)
        pay, pax = Y - ((unit * k * Dy + s // 2) >> ls) + cy, X - ((unit * k * Dx + s // 2) >> ls) + cx
        pby, pbx = Y + ((unit * (s - k) * Dy + s // 2) >> ls) + cy, X + ((unit * (s - k) * Dx + s // 2) >> ls) + cx
        a, b = sample(a_u8, pay, pax), sample(b_u8, pby, pbx)
        o = ((s - k) * a + k * b + s // 2) >> ls
        oka = okb = np.ones((H, W), bool)
        if masked:
            oka, okb = clean(ma, pay, pax), clean(mb, pby, pbx)
        if border == "valid":
            oka, okb = oka & sample_valid(pay, pax, H, W), okb & sample_valid(pby, pbx, H, W)
        oka, okb = oka[..., None], okb[..., None]
        o = np.where(oka == okb, o, np.where(oka, a, b))
        if masked and (k == 0 or k == s):   # the key frames themselves, whatever their masks
            o = a if k == 0 else b
        out[j] = o.astype(np.uint8)
    return out


def normalised(u8):
    """ToTensor + Normalize(0.5, 0.5) of uint8 [.., H, W, 3] frames as the host computes it for a decoded file
    (io_worker.normalised_chw: a true division by 255) -> float32 [.., 3, H, W]: what the sheets' DAIN pane shows."""
    a = np.asarray(u8).astype(np.float32) / 255.0
    return np.ascontiguousarray(np.moveaxis((a - 0.5) / 0.5, -1, -3))


def normalised_upload(u8):
    """The same two operations as the native path's upload - and rib_mci_frames' float output - evaluates them on the device:
    float32(u8) times the fp32 reciprocal of 255, minus 0.5, times 2, each rounded to float32 (csrc/resize.hip.h rsz_normalise;
    it differs from the division in the last bit for 111 of the 256 values) -> float32 [.., 3, H, W].  It is what the generator
    is fed under background="mci" on EITHER path: a model behind the reference's protocol reads the very floats the native
    chain reads, so the two paths write the same files."""
    a = np.asarray(u8).astype(np.float32) * np.float32(1.0 / 255.0)
    a = (a - np.float32(0.5)) * np.float32(2.0)
    return np.ascontiguousarray(np.moveaxis(a, -1, -3))
