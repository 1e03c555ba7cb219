#!/usr/bin/env python3
"""The PNG encoder on its own: rib_png (Generator.png_into) on T frames of H x W, for a kernel trace.

    rocprofv3 --kernel-trace --stats -d DIR -- python tools/png_bench.py [--size 512 | --height 1080 --width 1920] [--frames 16]
                                                                         [--reps 20] [--content smooth|noisy|flat] [--pil-frames 4]

Prints one JSON line: the call's wall time between two events (median and minimum of --reps, after a warm-up; both launches), its
byte floor (every frame read once, every file written once) and what that floor takes at 6.3 TB/s; what PIL takes per frame on
one core at compress_level 1 and 6 (the mean over --pil-frames frames; 0 skips it) and the mean file size of all three; and
whether frame 0's file is png.encode_host's, byte for byte, and decodes to the frame in PIL.  The kernels' own times are the
k_png_strips and k_png_assemble rows of the trace's kernel statistics.
The frames are the folder driver bench's (synth.smooth_image, quantised): smooth synthetic pictures; --content noisy adds Gaussian
noise of sigma 2 to them (closer to a photograph's residuals), --content flat is one colour with a rectangle (flat graphics,
where this stream is larger than zlib's).
"""
import argparse, io, json, os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import render_in_between_amd as rib
from render_in_between_amd import png, synth
from tools.panel_bench import timed


def frames_of(content, T, H, W):
    rng = np.random.default_rng(0)
    if content == "flat":
        a = np.full((T, H, W, 3), 40, np.uint8)
        for t in range(T):
            a[t, H // 5 + t:H // 2 + t, W // 4:W // 2 + 3 * t] = (200, 30, 90)
        return a
    spec = rib.GenSpec.from_cfg(rib.hsm_gen_config())
    out = []
    for t in range(T):
        x = np.asarray(synth.smooth_image(spec, 1, H, W, 100 + t))[0]
        u8 = ((x * 0.5 + 0.5).clip(0, 1) * 255).transpose(1, 2, 0)
        if content == "noisy":
            u8 = u8 + rng.normal(0, 2.0, u8.shape)
        out.append(np.ascontiguousarray(u8.clip(0, 255).astype(np.uint8)))
    return np.ascontiguousarray(np.stack(out))


def pil_encode(u8, level):
    from PIL import Image
    buf = io.BytesIO()
    t0 = time.perf_counter()
    Image.fromarray(u8).save(buf, "PNG", compress_level=level)
    return time.perf_counter() - t0, len(buf.getvalue())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--height", type=int, default=0)
    ap.add_argument("--width", type=int, default=0)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--content", default="smooth", choices=("smooth", "noisy", "flat"))
    ap.add_argument("--pil-frames", type=int, default=4, help="frames PIL encodes at level 1 and 6 for the comparison (0: none)")
    a = ap.parse_args()
    H, W, T = a.height or a.size, a.width or a.size, a.frames
    G = rib.Generator(rib.hsm_gen_config()).eval()                 # no weights needed: the encoder reads none
    host = frames_of(a.content, T, H, W)
    x = torch.from_numpy(host).cuda()
    cap = G.png_max_bytes(H, W)
    files = torch.zeros(T * cap, dtype=torch.uint8, device="cuda")
    lengths = torch.zeros(T, dtype=torch.int32, device="cuda")
    med, low = timed(lambda: G.png_into(x, files, lengths, cap), a.reps)
    sizes = lengths.cpu().tolist()
    first = files[:sizes[0]].cpu().numpy().tobytes()
    from PIL import Image
    res = {"height": H, "width": W, "frames": T, "content": a.content, "event_us_median": med, "event_us_min": low,
           "event_us_per_frame": round(med / T, 2), "frame_bytes": H * W * 3, "file_bytes_mean": sum(sizes) // T, "cap": cap,
           "floor_bytes": T * H * W * 3 + sum(sizes), "floor_us_at_6.3TBps": round((T * H * W * 3 + sum(sizes)) / 6.3e6, 2),
           "file_to_raw": round(sum(sizes) / (T * H * W * 3), 4),
           "frame0_is_encode_host": first == png.encode_host(host[0]),
           "frame0_decodes_in_pil": bool(np.array_equal(np.asarray(Image.open(io.BytesIO(first))), host[0]))}
    for level in (1, 6):
        got = [pil_encode(host[t], level) for t in range(min(a.pil_frames, T))]
        if got:
            res["pil_level%d_ms_per_frame_one_core" % level] = round(1e3 * sum(g[0] for g in got) / len(got), 2)
            res["pil_level%d_file_bytes_mean" % level] = sum(g[1] for g in got) // len(got)
            res["gpu_file_bytes_mean_same_frames"] = sum(sizes[:len(got)]) // len(got)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
