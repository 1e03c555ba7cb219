#!/usr/bin/env python3
"""The interpolated background at the key frames' own size on its own: rib_scaled_frames (Generator.mci_frames_scaled) on one unit
- T frames of B segments, the field of H x W model frames, the samples from H0 x W0 key frames - beside rib_mci_frames' uint8
output at the model size, for a kernel trace.

    rocprofv3 --kernel-trace --stats -d DIR -- python tools/scaled_frames_bench.py [--size 512] [--src-height 1080 --src-width 1920]
                                                     [--batch 4] [--rate 8] [--count 4] [--border clamp] [--precision full] [--reps 20]
                                                     [--sampler bilinear] [--staging 0] [--detail]

Prints one JSON line: the time of each launch between two events (median and min of --reps, after a warm-up) and each launch's
byte floor - every output byte written once, the two key frames read once - with what that floor takes at 6.3 TB/s.  The kernels'
own times are the k_scaled_frames and k_mci_frames rows of the trace.  The key frames are a smooth synthetic scene and its
translate, the field is rib_mci_field's (rib_halfpel_refine's with --precision half) of their model-size resize.
--sampler cubic: AFTER the two launches above, the same unit through rib_cubic_scaled (k_cubic_scaled in the same trace, beside
k_scaled_frames' rows); --staging 1 is that entry's diagnostic "never stage", 0 the per-tile rule.
--detail: AFTER those, the field refined at the key frames' size (rib_detail_field: k_detail_search and k_mci_median in the trace) and
the full-size frames from it through the existing entry (rib_mci_frames, or rib_cubic_frames with --sampler cubic: k_mci_frames /
k_cubic_frames at H0 x W0 beside the model-size rows); the field's floor is both full-size key frames read once.
"""
import argparse, json, os, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import render_in_between_amd as rib
from tools.mci_bench import timed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--src-height", type=int, default=1080)
    ap.add_argument("--src-width", type=int, default=1920)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--rate", type=int, default=8)
    ap.add_argument("--count", type=int, default=4, help="frames per segment in the launch (T); T * B frames in all")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--border", default="clamp", choices=("clamp", "valid"))
    ap.add_argument("--precision", default="full", choices=("full", "half"))
    ap.add_argument("--sampler", default="bilinear", choices=("bilinear", "cubic"), help="cubic: also time rib_cubic_scaled on the same unit")
    ap.add_argument("--detail", action="store_true", help="also time rib_detail_field and the full-size frames from its field (mci_detail='keyframes')")
    ap.add_argument("--staging", type=int, default=0, choices=(0, 1), help="with --sampler cubic: 0 = the per-tile staging rule, 1 = never stage")
    a = ap.parse_args()
    H = W = a.size
    H0, W0, B, s, T = a.src_height, a.src_width, a.batch, a.rate, a.count
    G = rib.Generator(rib.hsm_gen_config()).eval()                 # no weights needed: these kernels read none
    g = torch.Generator(device="cuda").manual_seed(0)
    m = 64                                     # margin of the scene around the key frames: the second crop moves by (m/2, -3m/8)
    big = torch.nn.functional.interpolate(torch.rand(B, 3, (H0 + 2 * m) // 16, (W0 + 2 * m) // 16, device="cuda", generator=g) * 255,
                                          size=(H0 + 2 * m, W0 + 2 * m), mode="bilinear", align_corners=False)
    big = (big + torch.rand(B, 3, H0 + 2 * m, W0 + 2 * m, device="cuda", generator=g) * 24).clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1)
    ka0, kb0 = big[:, m:m + H0, m:m + W0].contiguous(), big[:, m - 3 * m // 8:m - 3 * m // 8 + H0, m + m // 2:m + m // 2 + W0].contiguous()
    ka, kb = G.resize_u8(ka0, W, H), G.resize_u8(kb0, W, H)
    field = G.mci_field(ka, kb, border=a.border)
    if a.precision == "half":
        field = G.mci_refine(ka, kb, field, border=a.border)
    kw = dict(border=a.border, precision=a.precision)
    big_out = torch.empty(T, B, H0, W0, 3, dtype=torch.uint8, device="cuda")
    small_out = torch.empty(T, B, H, W, 3, dtype=torch.uint8, device="cuda")
    sms = timed(lambda: G.mci_frames_scaled(ka0, kb0, field, (H, W), s, k_first=1, count=T, out=big_out, **kw), a.reps)
    mms = timed(lambda: G.mci_frames(ka, kb, field, s, k_first=1, count=T, normalised=False, out=small_out, **kw), a.reps)
    floor = lambda h, w: 3 * h * w * T * B + 2 * 3 * h * w * B
    extra = {}
    if a.sampler == "cubic":
        from render_in_between_amd import background as bg
        cms = timed(lambda: G.mci_frames_scaled(ka0, kb0, field, (H, W), s, k_first=1, count=T, out=big_out, sampler="cubic", _staging=a.staging, **kw), a.reps)
        f0 = field[0].cpu().numpy()
        share = [float(bg.cubic_tile_staged(*bg.sample_positions(f0, s, k, H0, W0, a.precision, model_hw=(H, W))).mean()) for k in range(1, 1 + T)]
        extra = {"sampler": "cubic", "staging": a.staging, "cubic_scaled_event_us_median": round(cms[len(cms) // 2] * 1e3, 2),
                 "cubic_scaled_event_us_min": round(cms[0] * 1e3, 2), "cubic_tiles_staged_by_the_rule": round(sum(share) / len(share), 3)}
    if a.detail:
        from render_in_between_amd import background as bg
        R = bg.detail_radius((H, W), (H0, W0))
        dms = timed(lambda: G.mci_detail_field(ka0, kb0, field, (H, W), **kw), a.reps)
        field0 = G.mci_detail_field(ka0, kb0, field, (H, W), **kw)
        fms = timed(lambda: G.mci_frames(ka0, kb0, field0, s, k_first=1, count=T, normalised=False, out=big_out, border=a.border, sampler=a.sampler,
                                         _staging=a.staging), a.reps)
        blocks = field0.shape[1] * field0.shape[2]
        extra.update({"detail_radius": R, "detail_blocks_per_segment": blocks, "detail_candidates": (2 * R + 1) ** 2,
                      "detail_field_event_us_median": round(dms[len(dms) // 2] * 1e3, 2), "detail_field_event_us_min": round(dms[0] * 1e3, 2),
                      "detail_field_floor_bytes": 2 * 3 * H0 * W0 * B, "detail_field_floor_us_at_6.3TB/s": round(2 * 3 * H0 * W0 * B / 6.3e12 * 1e6, 2),
                      "detail_frames_event_us_median": round(fms[len(fms) // 2] * 1e3, 2), "detail_frames_event_us_min": round(fms[0] * 1e3, 2),
                      "detail_field_max_abs": int(field0.abs().max())})
    print(json.dumps({"height": H, "width": W, "src_height": H0, "src_width": W0, "batch": B, "rate": s, "frames": T * B, "border": a.border,
                      "precision": a.precision,
                      "scaled_event_us_median": round(sms[len(sms) // 2] * 1e3, 2), "scaled_event_us_min": round(sms[0] * 1e3, 2),
                      "scaled_floor_bytes": floor(H0, W0), "scaled_floor_us_at_6.3TB/s": round(floor(H0, W0) / 6.3e12 * 1e6, 2),
                      "model_u8_event_us_median": round(mms[len(mms) // 2] * 1e3, 2), "model_u8_event_us_min": round(mms[0] * 1e3, 2),
                      "model_u8_floor_bytes": floor(H, W), "model_u8_floor_us_at_6.3TB/s": round(floor(H, W) / 6.3e12 * 1e6, 2),
                      "field_nonzero_fraction": round(float((field != 0).float().mean()), 3), "field_max_abs": int(field.abs().max()), **extra}))


if __name__ == "__main__":
    main()
