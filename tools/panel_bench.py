#!/usr/bin/env python3
"""The sheet kernel on its own: rib_panel (Generator.panel) on T frames of H x W, for a kernel trace.

    rocprofv3 --kernel-trace --stats -d DIR -- python tools/panel_bench.py [--size 512] [--frames 16] [--reps 20]

Prints one JSON line: the launch's wall time between two events (median of --reps, after a warm-up), its byte floor
(16 floats read + 18 bytes written per source pixel) and what that floor takes at 6.3 TB/s.  The kernel's own time is
k_panel's row of the trace's kernel statistics.
"""
import argparse, json, os, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import render_in_between_amd as rib
from render_in_between_amd import panel


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--height", type=int, default=0)
    ap.add_argument("--width", type=int, default=0)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    H, W, T = a.height or a.size, a.width or a.size, a.frames
    G = rib.Generator(rib.hsm_gen_config()).eval()                 # no weights needed: the sheet kernel reads none
    g = torch.Generator(device="cuda").manual_seed(0)
    rnd = lambda c: torch.rand(T, c, H, W, device="cuda", generator=g) * 2.4 - 1.2
    pred, fuse, dain, gt, label = rnd(3), rnd(3), rnd(3), rnd(3), rnd(G.spec.label_nc)
    mask = torch.rand(T, 1, H, W, device="cuda", generator=g)
    titles = torch.from_numpy(panel.title_bitmap(W)).cuda()
    SH, SW = panel.layout(H, W)["sheet"]
    out = torch.empty(T, SH, SW, 3, dtype=torch.uint8, device="cuda")
    for _ in range(3):
        G.panel(pred, mask, fuse, dain, gt, label, titles=titles, out=out)
    torch.cuda.synchronize()
    ms = []
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        G.panel(pred, mask, fuse, dain, gt, label, titles=titles, out=out)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    ms.sort()
    floor = (64 + 18) * H * W * T
    print(json.dumps({"height": H, "width": W, "frames": T, "sheet": [SH, SW], "event_us_median": round(ms[len(ms) // 2] * 1e3, 2),
                      "event_us_min": round(ms[0] * 1e3, 2), "floor_bytes": floor, "written_bytes": out.numel(),
                      "floor_us_at_6.3TB/s": round(floor / 6.3e12 * 1e6, 2)}))


if __name__ == "__main__":
    main()
