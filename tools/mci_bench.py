#!/usr/bin/env python3
"""The motion-compensated background on its own: rib_mci_field and rib_mci_frames (Generator.mci_field / mci_frames) on one
unit - B segments of H x W at sample rate s - for a kernel trace.

    rocprofv3 --kernel-trace --stats -d DIR -- python tools/mci_bench.py [--size 512] [--batch 4] [--rate 8] [--reps 20] [--u8] [--levels 3] [--border clamp] [--precision full] [--person]
                                                     [--sampler bilinear] [--staging 0]

--levels 3 (the default), 4 or 5: the pyramid levels of the field's search, the driver's --mci-range 32, 64 or 128; the scene's
motion between the key frames grows with it (a quarter of that range in x, 3/16 in y).  --border valid: the one-sided border mode
(the driver's --mci-border; k_mci_search<R, true> and k_mci_frames<true> in the trace).  --precision half (the driver's
--mci-precision): the refine launch (rib_halfpel_refine, k_mci_refine in the trace) is timed beside the field, and the frames are
rib_halfpel_frames's from the refined field (k_mci_frames<.., true>); the default times what it always timed.
--person (the driver's --mci-person exclude): AFTER everything above, the same unit through rib_masked_field / rib_masked_frames
(Generator.mci_field_masked / mci_frames_masked) with an upright ellipse per key frame as the excluded pixels, a sixth of the
width wide and moved by an eighth of the width between the key frames - k_mci_mask_pyramid, k_mci_search<R, .., true>, k_mci_fill
and k_mci_frames<.., .., true> in the same trace, beside the unmasked rows; not with --precision half.
--sampler cubic (the driver's --mci-sampler): AFTER everything above, the same frames launch through rib_cubic_frames (k_cubic_frames
in the same trace, beside k_mci_frames' rows; with --person also its masked form); --staging 1 passes that entry's diagnostic
"never stage" (every tile gathers its taps directly), 0 is the per-tile rule.  The JSON then also holds the share of tiles the
rule stages on this field (background.cubic_tile_staged, on the host, segment 0).
--mci-motion quadratic (the driver's --mci-motion): AFTER everything above, what that setting adds per group - the fields of the
segment and of the segments before and after it in ONE call over 3 B pairs (the scene moves by half the segment's motion before it
and by the same motion after it; with --precision half the refine launch over the same 3 B), rib_accel_field (k_mci_accel and one
more k_mci_median in the trace) - and the frames through rib_accel_frames (k_accel_frames beside k_mci_frames' rows; with --sampler
cubic also k_cubic_accel beside k_cubic_frames').

Prints one JSON line: the wall time of the field's launches (levels + 2: five by default) and of the frames launch between two events (median of
--reps, after a warm-up), the frames launch's byte floor (12 bytes of float32 out per pixel and frame, 3 more with --u8, the
two key frames once) and what that floor takes at 6.3 TB/s.  The kernels' own times are the k_mci_luma_pyramid, k_mci_search,
k_mci_median and k_mci_frames rows of the trace's kernel statistics.  The key frames are a smooth synthetic scene and its
translate, so that the search does real work.
"""
import argparse, json, os, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import render_in_between_amd as rib


def timed(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    ms.sort()
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--height", type=int, default=0)
    ap.add_argument("--width", type=int, default=0)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--rate", type=int, default=8)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--u8", action="store_true", help="also write the uint8 NHWC frames (the sheets' DAIN pane)")
    ap.add_argument("--levels", type=int, default=3, choices=(3, 4, 5), help="pyramid levels of the search (--mci-range 32, 64, 128)")
    ap.add_argument("--border", default="clamp", choices=("clamp", "valid"), help="the border mode (--mci-border)")
    ap.add_argument("--precision", default="full", choices=("full", "half"), help="the field's unit (--mci-precision): half also times the refine launch")
    ap.add_argument("--person", action="store_true", help="also time the masked entries (--mci-person exclude) on the same unit")
    ap.add_argument("--sampler", default="bilinear", choices=("bilinear", "cubic"), help="cubic: also time rib_cubic_frames on the same unit (--mci-sampler)")
    ap.add_argument("--staging", type=int, default=0, choices=(0, 1), help="with --sampler cubic: 0 = the per-tile staging rule, 1 = never stage (a diagnostic)")
    ap.add_argument("--mci-motion", default="linear", choices=("linear", "quadratic"),
                    help="quadratic: also time the three segments' fields in one call, rib_accel_field and rib_accel_frames on the same unit (--mci-motion)")
    a = ap.parse_args()
    if a.person and a.precision == "half":
        ap.error("--person times the whole-pixel masked entries: not with --precision half")
    kw = {} if a.border == "clamp" else {"border": a.border}       # (clamp: the calls of before the mode existed)
    H, W, B, s = a.height or a.size, a.width or a.size, a.batch, a.rate
    m = 16 << (a.levels - 3)                   # margin of the scene around the key frames: the second crop moves by (m/2, -3m/8)
    G = rib.Generator(rib.hsm_gen_config()).eval()                 # no weights needed: these kernels read none
    g = torch.Generator(device="cuda").manual_seed(0)
    big = torch.nn.functional.interpolate(torch.rand(B, 3, (H + 2 * m) // 8, (W + 2 * m) // 8, device="cuda", generator=g) * 255,
                                          size=(H + 2 * m, W + 2 * m), mode="bilinear", align_corners=False)
    big = (big + torch.rand(B, 3, H + 2 * m, W + 2 * m, device="cuda", generator=g) * 24).clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1)
    ka, kb = big[:, m:m + H, m:m + W].contiguous(), big[:, m - 3 * m // 8:m - 3 * m // 8 + H, m + m // 2:m + m // 2 + W].contiguous()
    field = G.mci_field(ka, kb, a.levels, **kw)
    half, fkw, extra = a.precision == "half", dict(kw), {}
    if half:
        whole = field
        field = G.mci_refine(ka, kb, whole, **kw)
        fkw["precision"] = "half"
        nms = timed(lambda: G.mci_refine(ka, kb, whole, **kw), a.reps)
        extra = {"refine_event_us_median": round(nms[len(nms) // 2] * 1e3, 2), "refine_event_us_min": round(nms[0] * 1e3, 2),
                 "refined_odd_fraction": round(float(((field & 1) != 0).any(-1).float().mean()), 3)}
    T = s - 1
    f32 = torch.empty(T, B, 3, H, W, dtype=torch.float32, device="cuda")
    u8 = torch.empty(T, B, H, W, 3, dtype=torch.uint8, device="cuda") if a.u8 else None
    fms = timed(lambda: G.mci_field(ka, kb, a.levels, **kw), a.reps)
    rms = timed(lambda: G.mci_frames(ka, kb, field, s, normalised="both" if a.u8 else True, out=(f32, u8) if a.u8 else f32, **fkw), a.reps)
    floor = (12 + (3 if a.u8 else 0)) * H * W * T * B + 2 * 3 * H * W * B
    if a.person:
        Y, X = torch.meshgrid(torch.arange(H, device="cuda"), torch.arange(W, device="cuda"), indexing="ij")
        oval = lambda cx: ((((X - cx) * 12 // W) ** 2 + ((Y - H // 2) * 3 // H) ** 2) <= 1).to(torch.uint8).expand(B, H, W).contiguous()
        qa, qb = oval(W // 2 - W // 16), oval(W // 2 + W // 16)
        mfield = G.mci_field_masked(ka, kb, qa, qb, a.levels, **kw)
        pms = timed(lambda: G.mci_field_masked(ka, kb, qa, qb, a.levels, **kw), a.reps)
        qms = timed(lambda: G.mci_frames_masked(ka, kb, qa, qb, mfield, s, normalised="both" if a.u8 else True, out=(f32, u8) if a.u8 else f32, **kw), a.reps)
        extra.update({"person": True, "excluded_fraction": round(float((qa != 0).float().mean()), 3),
                      "masked_field_event_us_median": round(pms[len(pms) // 2] * 1e3, 2), "masked_field_event_us_min": round(pms[0] * 1e3, 2),
                      "masked_frames_event_us_median": round(qms[len(qms) // 2] * 1e3, 2), "masked_frames_event_us_min": round(qms[0] * 1e3, 2),
                      "masked_field_differs_fraction": round(float((mfield != field).any(-1).float().mean()), 3)})
    if a.sampler == "cubic":
        from render_in_between_amd import background as bg
        ckw = dict(fkw, sampler="cubic", _staging=a.staging)
        cms = timed(lambda: G.mci_frames(ka, kb, field, s, normalised="both" if a.u8 else True, out=(f32, u8) if a.u8 else f32, **ckw), a.reps)
        f0 = field[0].cpu().numpy()
        share = [float(bg.cubic_tile_staged(*bg.sample_positions(f0, s, k, H, W, a.precision)).mean()) for k in range(1, s)]
        extra.update({"sampler": "cubic", "staging": a.staging, "cubic_frames_event_us_median": round(cms[len(cms) // 2] * 1e3, 2),
                      "cubic_frames_event_us_min": round(cms[0] * 1e3, 2), "cubic_tiles_staged_by_the_rule": round(sum(share) / len(share), 3)})
        if a.person:
            xms = timed(lambda: G.mci_frames_masked(ka, kb, qa, qb, mfield, s, normalised="both" if a.u8 else True, out=(f32, u8) if a.u8 else f32,
                                                    **dict(kw, sampler="cubic", _staging=a.staging)), a.reps)
            extra.update({"cubic_masked_frames_event_us_median": round(xms[len(xms) // 2] * 1e3, 2), "cubic_masked_frames_event_us_min": round(xms[0] * 1e3, 2)})
    if a.mci_motion == "quadratic":
        # the key frames before and after: the scene moved by half the segment's motion before it and by the same motion after it
        kp = big[:, m + 3 * m // 16:m + 3 * m // 16 + H, m - m // 4:m - m // 4 + W].contiguous()
        kn = big[:, m - 3 * m // 4:m - 3 * m // 4 + H, m + m:m + m + W].contiguous()
        pa, pb = torch.cat([ka, kp, kb]), torch.cat([kb, ka, kn])      # own | before | after: one batched call per entry, as the driver's

        def three_fields():
            f3 = G.mci_field(pa, pb, a.levels, **kw)
            return G.mci_refine(pa, pb, f3, out=f3, **kw) if half else f3
        f3 = three_fields()
        accel = G.mci_accel_field(f3[B:2 * B], f3[:B], f3[2 * B:], precision=a.precision)
        tms = timed(three_fields, a.reps)
        ams = timed(lambda: G.mci_accel_field(f3[B:2 * B], f3[:B], f3[2 * B:], precision=a.precision), a.reps)
        out = dict(normalised="both" if a.u8 else True, out=(f32, u8) if a.u8 else f32)
        qms = timed(lambda: G.mci_frames_accel(ka, kb, f3[:B], accel, s, **out, **fkw), a.reps)
        extra.update({"mci_motion": "quadratic", "three_fields_event_us_median": round(tms[len(tms) // 2] * 1e3, 2), "three_fields_event_us_min": round(tms[0] * 1e3, 2),
                      "accel_field_event_us_median": round(ams[len(ams) // 2] * 1e3, 2), "accel_field_event_us_min": round(ams[0] * 1e3, 2),
                      "accel_frames_event_us_median": round(qms[len(qms) // 2] * 1e3, 2), "accel_frames_event_us_min": round(qms[0] * 1e3, 2),
                      "accel_nonzero_fraction": round(float((accel != 0).float().mean()), 3), "accel_max_abs": int(accel.abs().max())})
        if a.sampler == "cubic":
            yms = timed(lambda: G.mci_frames_accel(ka, kb, f3[:B], accel, s, **out, **dict(fkw, sampler="cubic")), a.reps)
            extra.update({"cubic_accel_frames_event_us_median": round(yms[len(yms) // 2] * 1e3, 2), "cubic_accel_frames_event_us_min": round(yms[0] * 1e3, 2)})
    print(json.dumps({"height": H, "width": W, "batch": B, "rate": s, "levels": a.levels, "border": a.border, "precision": a.precision, "frames": T * B, "u8": a.u8,
                      "field_event_us_median": round(fms[len(fms) // 2] * 1e3, 2), "field_event_us_min": round(fms[0] * 1e3, 2),
                      "frames_event_us_median": round(rms[len(rms) // 2] * 1e3, 2), "frames_event_us_min": round(rms[0] * 1e3, 2),
                      "frames_floor_bytes": floor, "frames_floor_us_at_6.3TB/s": round(floor / 6.3e12 * 1e6, 2),
                      "field_nonzero_fraction": round(float((field != 0).float().mean()), 3), "field_max_abs": int(field.abs().max()), **extra}))


if __name__ == "__main__":
    main()
