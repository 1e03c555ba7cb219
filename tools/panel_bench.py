#!/usr/bin/env python3
"""The sheet kernel on its own: rib_panel (Generator.panel) on T frames of H x W, for a kernel trace.

    rocprofv3 --kernel-trace --stats -d DIR -- python tools/panel_bench.py [--size 512] [--frames 16] [--reps 20] [--jpeg [--quality 90]]

Prints one JSON line: the launch's wall time between two events (median of --reps, after a warm-up), its byte floor
(16 floats read + 18 bytes written per source pixel) and what that floor takes at 6.3 TB/s.  The kernel's own time is
k_panel's row of the trace's kernel statistics.  --jpeg also times rib_jpeg (Generator.jpeg_into) on the composed sheets, on
its own pair of events: "jpeg_*" keys; its byte floor is the sheets read once and the files written twice (staging slot, file)
and read once; the kernels' own times are the k_jpeg_segments and k_jpeg_assemble rows.  The sheets are composed from smooth
synthetic frames (a noise sheet would measure the entropy coder at its worst, ten times a real sheet's bytes).
--jpeg-f32 times the encoder's float front end alone, on T smooth frames of H x W (no sheet is composed): rib_jpeg_float
(Generator.jpeg_f32_into, k_jpeg_segments<float>) against the two-launch composition rib_quantise + rib_jpeg (k_quantise,
k_jpeg_segments<unsigned char>) on the same frames, each on its own pair of events ("f32_*" and "u8_*" keys), and says whether
the two wrote the same bytes.
"""
import argparse, json, os, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import render_in_between_amd as rib
from render_in_between_amd import panel


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
    return round(ms[len(ms) // 2] * 1e3, 2), round(ms[0] * 1e3, 2)


def jpeg_f32_bench(a, G, H, W, T, g):
    x = torch.nn.functional.interpolate(torch.rand(T, 3, max(H // 16, 2), max(W // 16, 2), device="cuda", generator=g) * 2.4 - 1.2,
                                        size=(H, W), mode="bilinear", align_corners=False).contiguous()
    cap = G.jpeg_max_bytes(H, W)
    files = [torch.zeros(T * cap, dtype=torch.uint8, device="cuda") for _ in range(2)]
    lengths = [torch.zeros(T, dtype=torch.int32, device="cuda") for _ in range(2)]
    q = torch.empty(T, H, W, 3, dtype=torch.uint8, device="cuda")

    def composed():
        G.quantise(x, out=q)
        G.jpeg_into(q, files[1], lengths[1], a.quality, cap)
    f32 = timed(lambda: G.jpeg_f32_into(x, files[0], lengths[0], a.quality, cap), a.reps)
    u8 = timed(composed, a.reps)
    sizes = lengths[0].cpu().tolist()
    same = sizes == lengths[1].cpu().tolist() and all(torch.equal(files[0][t * cap:t * cap + sizes[t]], files[1][t * cap:t * cap + sizes[t]]) for t in range(T))
    print(json.dumps({"height": H, "width": W, "frames": T, "jpeg_quality": a.quality, "f32_event_us_median": f32[0], "f32_event_us_min": f32[1],
                      "u8_event_us_median": u8[0], "u8_event_us_min": u8[1], "same_bytes": bool(same), "jpeg_file_bytes_mean": sum(sizes) // T,
                      "f32_read_bytes": x.numel() * 4, "u8_read_bytes": x.numel() * 4 + q.numel(), "u8_written_bytes": q.numel()}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--height", type=int, default=0)
    ap.add_argument("--width", type=int, default=0)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--jpeg", action="store_true", help="also encode the sheets (rib_jpeg) and time that separately")
    ap.add_argument("--quality", type=int, default=90)
    ap.add_argument("--jpeg-f32", action="store_true", help="time rib_jpeg_float against rib_quantise + rib_jpeg on float frames, nothing else")
    a = ap.parse_args()
    H, W, T = a.height or a.size, a.width or a.size, a.frames
    G = rib.Generator(rib.hsm_gen_config()).eval()                 # no weights needed: the sheet kernel reads none
    g = torch.Generator(device="cuda").manual_seed(0)
    if a.jpeg:        # smooth frames: low-resolution noise, bilinearly enlarged, so that the JPEG sizes are those of pictures
        rnd = lambda c: torch.nn.functional.interpolate(torch.rand(T, c, max(H // 16, 2), max(W // 16, 2), device="cuda", generator=g) * 2.4 - 1.2,
                                                        size=(H, W), mode="bilinear", align_corners=False).contiguous()
    else:
        rnd = lambda c: torch.rand(T, c, H, W, device="cuda", generator=g) * 2.4 - 1.2
    if a.jpeg_f32:
        return jpeg_f32_bench(a, G, H, W, T, g)
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
    extra = {}
    if a.jpeg:
        cap = G.jpeg_max_bytes(SH, SW)
        files = torch.empty(T * cap, dtype=torch.uint8, device="cuda")
        lengths = torch.empty(T, dtype=torch.int32, device="cuda")
        for _ in range(3):
            G.jpeg_into(out, files, lengths, a.quality, cap)
        torch.cuda.synchronize()
        js = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            G.jpeg_into(out, files, lengths, a.quality, cap)
            e1.record()
            e1.synchronize()
            js.append(e0.elapsed_time(e1))
        js.sort()
        sizes = lengths.cpu().tolist()
        jfloor = out.numel() + 3 * sum(sizes)
        extra = {"jpeg_quality": a.quality, "jpeg_event_us_median": round(js[len(js) // 2] * 1e3, 2), "jpeg_event_us_min": round(js[0] * 1e3, 2),
                 "jpeg_file_bytes_mean": sum(sizes) // T, "jpeg_floor_bytes": jfloor, "jpeg_floor_us_at_6.3TB/s": round(jfloor / 6.3e12 * 1e6, 2)}
    print(json.dumps({"height": H, "width": W, "frames": T, "sheet": [SH, SW], "event_us_median": round(ms[len(ms) // 2] * 1e3, 2),
                      "event_us_min": round(ms[0] * 1e3, 2), "floor_bytes": floor, "written_bytes": out.numel(),
                      "floor_us_at_6.3TB/s": round(floor / 6.3e12 * 1e6, 2), **extra}))


if __name__ == "__main__":
    main()
