#!/usr/bin/env python3
"""The source-size composite on its own: rib_composite (Generator.composite) against the composition of the existing entries it
replaces, on the same inputs, for a kernel trace.

    rocprofv3 --kernel-trace --stats -d DIR -- python tools/composite_bench.py [--size 512] [--src-width 1920 --src-height 1080]
                                                                               [--frames 16] [--reps 20] [--only fused|composed]

Prints one JSON line: the wall time between two events (median and minimum of --reps, after a warm-up) of the fused launch
("fused_*") and of the composition ("composed_*": rib_quantise, the mask to uint8 on three channels, two rib_resize_cubic
launches and an integer blend in torch), whether the two wrote the same bytes, and the fused launch's byte floor - the float
patch read once (4 planes), the background read and the output written - with what that floor takes at 6.3 TB/s.  The kernels'
own times are the rows of the trace's kernel statistics: k_composite against k_quantise, k_resize_cubic_u8 (two calls per
repetition) and torch's elementwise kernels.  --only times one side alone, so that a trace holds nothing else.
The inputs are smooth synthetic frames and a soft-edged disc as the mask; the kernel's work does not depend on the values.
"""
import argparse, json, os, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import render_in_between_amd as rib
from tools.panel_bench import timed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--height", type=int, default=0)
    ap.add_argument("--width", type=int, default=0)
    ap.add_argument("--src-width", type=int, default=1920)
    ap.add_argument("--src-height", type=int, default=1080)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only", default="both", choices=("both", "fused", "composed"))
    a = ap.parse_args()
    H, W, H0, W0, T = a.height or a.size, a.width or a.size, a.src_height, a.src_width, a.frames
    G = rib.Generator(rib.hsm_gen_config()).eval()                 # no weights needed: the kernel reads none
    g = torch.Generator(device="cuda").manual_seed(0)
    pred = torch.nn.functional.interpolate(torch.rand(T, 3, max(H // 16, 2), max(W // 16, 2), device="cuda", generator=g) * 2.4 - 1.2,
                                           size=(H, W), mode="bilinear", align_corners=False).contiguous()
    yy, xx = torch.meshgrid(torch.arange(H, device="cuda"), torch.arange(W, device="cuda"), indexing="ij")
    r = torch.sqrt((yy - H / 2.0) ** 2 + (xx - W / 2.0) ** 2)
    mask = ((min(H, W) / 3.0 - r) / 8.0).clamp(0, 1).to(torch.float32).expand(T, 1, H, W).contiguous()
    bg = torch.randint(0, 256, (T, H0, W0, 3), dtype=torch.uint8, device="cuda", generator=g)
    fused_out, composed_out = torch.empty_like(bg), torch.empty_like(bg)
    P = torch.empty(T, H, W, 3, dtype=torch.uint8, device="cuda")
    Pu, Mu = torch.empty_like(bg), torch.empty_like(bg)

    def fused():
        G.composite(pred, mask, bg, out=fused_out)

    def composed():
        G.quantise(pred, out=P)
        M = (mask.double().clamp(0, 1) * 255.0).to(torch.uint8).permute(0, 2, 3, 1).expand(-1, -1, -1, 3).contiguous()
        G.resize_u8(P, W0, H0, out=Pu)
        G.resize_u8(M, W0, H0, out=Mu)
        m = Mu.int()
        composed_out.copy_((Pu.int() * m + bg.int() * (255 - m) + 127) // 255)

    res = {"height": H, "width": W, "src_height": H0, "src_width": W0, "frames": T}
    if a.only in ("both", "fused"):
        res["fused_event_us_median"], res["fused_event_us_min"] = timed(fused, a.reps)
    if a.only in ("both", "composed"):
        res["composed_event_us_median"], res["composed_event_us_min"] = timed(composed, a.reps)
    if a.only == "both":
        res["same_bytes"] = bool(torch.equal(fused_out, composed_out))
    floor = T * (4 * H * W * 4 + 2 * H0 * W0 * 3)
    res.update({"floor_bytes": floor, "floor_us_at_6.3TB/s": round(floor / 6.3e12 * 1e6, 2)})
    print(json.dumps(res))


if __name__ == "__main__":
    main()
