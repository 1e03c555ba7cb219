#!/usr/bin/env python3
"""End-to-end rate of the folder driver (json + PNG in, PNG out) on a synthetic clip.

    python tools/driver_bench.py [--size 512 | --height 320 --width 480] [--keys 5] [--rate 32] [--lanes 2] [--batch B] [--chunk 4]
                                  [--src-width 1920 --src-height 1080] [--resize-on host|gpu] [--metrics [--pose-mask]] [--panels [--panel-encode host|gpu]]
                                  [--video [--frames none]] [--poses folder|keyframes] [--output-size model|source|keyframes]
                                  [--png-on host|gpu]

Writes a clip in the reference's directory layout (inputs/ DAIN/ Predict_motion/), runs
Evaluator.evaluate_from_folder twice (the first run also builds launch plans) and prints the
phase times of the second: load (decode + json), rasterise (GPU), generate (GPU chains + quantise +
one D2H copy), save (PNG encode).  --src-width / --src-height write the input frames at that size (default: the model size),
so that the driver has to resize them; --resize-on says where (Evaluator(resize_on=...)).  --metrics also writes a ground-truth
frame per frame (gt/) and measures every generated frame against it (evaluate_from_folder(metrics=True)); --pose-mask measures
under the mask drawn from each frame's pose (pose_mask=True), so that the cost of either can be read off two runs.  --panels also composes the six-pane diagnostic sheet of every frame and
writes the clip's Motion-JPEG video (evaluate_from_folder(panels=True)); --panel-encode says where its JPEG frames are encoded.
--video also writes the frames themselves as <clip>_video.avi (video=True: rib_jpeg_float on the lane's stream); --frames none
writes only that video (frames="none": no PNG is encoded, the PNG level then plays no part).  --poses keyframes runs stage 1
in the driver (poses="keyframes": a seed-defined motion transformer interpolates the key frames' poses of key_poses/, no json is
read per frame; --rate must then be a power of two); the per-clip event time of stage 1 plus the bridge is reported too.
--output-size source (with --resize-on gpu) writes the frames' files at the size of the input files (output_size="source": one
rib_composite launch per unit; the PNG encode then works on source-size frames).  --output-size keyframes (with --background mci)
does the same at the size of the key frame files (output_size="keyframes": one rib_scaled_frames launch per unit makes the
backgrounds, --src-width / --src-height say how large the key frames are).
--png-on gpu encodes the frames' PNG files on the lane's stream (png_on="gpu": rib_png, this project's own stream; --compress
then plays no part and must be left at its default); the bytes of the last run's PNG files are reported either way.
"""
import argparse, json, os, sys, tempfile, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import render_in_between_amd as rib
from render_in_between_amd import evaluator as ev, synth
from tools.raster_bench import person


def write_clip(root, n_key, rate, H, W, src_h=0, src_w=0, gt=False, dain=True):
    from PIL import Image
    rng = np.random.default_rng(0)
    n = (n_key - 1) * rate + 1
    for d in ("inputs", "DAIN", "Predict_motion") + (("gt",) if gt else ()):
        os.makedirs(os.path.join(root, d, "clip"))
    spec = rib.GenSpec.from_cfg(rib.hsm_gen_config())
    sh, sw = src_h or H, src_w or W          # the files' size; the keypoints below are in the same pixels
    def img(seed):
        a = np.asarray(synth.smooth_image(spec, 1, sh, sw, seed))[0]
        return ((a * 0.5 + 0.5).clip(0, 1) * 255).astype(np.uint8).transpose(1, 2, 0)
    for k in range(n_key):
        Image.fromarray(img(k)).save(os.path.join(root, "inputs", "clip", "%04d.png" % k))
    for i in range(n):
        if dain:                              # (background="mci" reads none: most of the time a 1080p clip takes to write)
            Image.fromarray(img(100 + i)).save(os.path.join(root, "DAIN", "clip", "f%04d.png" % i))
        if gt:
            Image.fromarray(img(1000 + i)).save(os.path.join(root, "gt", "clip", "f%04d.png" % i))
        lm, conf = person(rng, sh, sw)
        body = np.zeros((25, 3)); idx = list(range(15)) + [19, 22]
        for j, k in enumerate(idx):
            body[k] = (lm[j][0], lm[j][1], conf[j])
        hand = lambda c: [v for _ in range(21) for v in (c[0] + float(rng.normal(0, 3)), c[1] + float(rng.normal(0, 3)), 0.8)]
        doc = {"people": [{"pose_keypoints_2d": [float(v) for v in body.reshape(-1)],
                           "hand_left_keypoints_2d": hand(lm[17]), "hand_right_keypoints_2d": hand(lm[18])}]}
        with open(os.path.join(root, "Predict_motion", "clip", "f%04d_keypoints.json" % i), "w") as f:
            json.dump(doc, f)
        if i % rate == 0:                     # the key frames' detections: what poses="keyframes" starts from
            os.makedirs(os.path.join(root, "key_poses", "clip"), exist_ok=True)
            with open(os.path.join(root, "key_poses", "clip", "%04d_keypoints.json" % (i // rate)), "w") as f:
                json.dump(doc, f)
    return n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--keys", type=int, default=3)
    ap.add_argument("--rate", type=int, default=32)
    ap.add_argument("--height", type=int, default=0)
    ap.add_argument("--width", type=int, default=0)
    ap.add_argument("--lanes", type=int, default=2)
    ap.add_argument("--batch", type=int, default=0, help="segments per chain (0: the Evaluator's default for the frame size)")
    ap.add_argument("--chunk", type=int, default=4)
    ap.add_argument("--io-threads", type=int, default=0)
    ap.add_argument("--compress", type=int, default=-1, help="PNG compress level (-1: PIL's default, 6, as the reference)")
    ap.add_argument("--io-mode", default="process", choices=("process", "thread"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--dtype", default="f32")
    ap.add_argument("--src-width", type=int, default=0, help="width of the synthetic input files (0: the model width)")
    ap.add_argument("--src-height", type=int, default=0, help="height of the synthetic input files (0: the model height)")
    ap.add_argument("--resize-on", default="host", choices=("host", "gpu"), help="where the DAIN frames are resized (Evaluator(resize_on=...))")
    ap.add_argument("--metrics", action="store_true", help="measure every generated frame against a synthetic ground-truth frame (metrics=True)")
    ap.add_argument("--pose-mask", action="store_true", help="with --metrics: under the mask drawn from each frame's pose (pose_mask=True)")
    ap.add_argument("--panels", action="store_true", help="also write the diagnostic sheets and the clip's video (panels=True)")
    ap.add_argument("--panel-encode", default="host", choices=("host", "gpu"), help="with --panels: PIL in the file workers or rib_jpeg (panel_encode=...)")
    ap.add_argument("--background", default="dain", choices=("dain", "mci"),
                    help="'mci': the background frames are interpolated on the GPU from the key frames and the clip's DAIN folder is not read (background=...)")
    ap.add_argument("--mci-range", type=int, default=32, choices=(32, 64, 128), help="with --background mci: the search's range in px between key frames (mci_range=...)")
    ap.add_argument("--mci-border", default="clamp", choices=("clamp", "valid"), help="with --background mci: the border mode (mci_border=...)")
    ap.add_argument("--mci-precision", default="full", choices=("full", "half"), help="with --background mci: half-pel refinement of the field (mci_precision=...)")
    ap.add_argument("--mci-person", default="keep", choices=("keep", "exclude"),
                    help="with --background mci: the key frames' human masks are kept out of the interpolation (mci_person=...)")
    ap.add_argument("--mci-detail", default="model", choices=("model", "keyframes"),
                    help="with --background mci --output-size keyframes: refine the field at the key frames' size (mci_detail=...)")
    ap.add_argument("--mci-sampler", default="bilinear", choices=("bilinear", "cubic"),
                    help="with --background mci: the 4x4 cubic sampler for every background sample (mci_sampler=...)")
    ap.add_argument("--mci-motion", default="linear", choices=("linear", "quadratic"),
                    help="with --background mci: the second-order trajectory from the neighbouring segments' fields (mci_motion=...)")
    ap.add_argument("--video", action="store_true", help="also write the frames as <clip>_video.avi, JPEG-encoded on the GPU (video=True)")
    ap.add_argument("--frames", default="png", choices=("png", "none"), help="with --video: 'none' writes no PNG frames (frames=...)")
    ap.add_argument("--poses", default="folder", choices=("folder", "keyframes"),
                    help="'keyframes': the motion transformer interpolates the key frames' poses inside the driver (poses=...)")
    ap.add_argument("--output-size", default="model", choices=("model", "source", "keyframes"),
                    help="'source' (with --resize-on gpu): the frames' files at the input files' size, composited on the GPU; 'keyframes' "
                         "(with --background mci): the same from the key frame files, the backgrounds by rib_scaled_frames (output_size=...)")
    ap.add_argument("--png-on", default="host", choices=("host", "gpu"), help="where the frames' PNG files are encoded: PIL in the file workers or rib_png (png_on=...)")
    a = ap.parse_args()
    if a.png_on == "gpu" and (a.compress >= 0 or a.frames == "none"):
        ap.error("--png-on gpu is not combined with --compress or --frames none")
    if a.output_size == "keyframes" and a.background != "mci":
        ap.error("--output-size keyframes is a setting of --background mci")
    if a.output_size == "source" and (a.resize_on != "gpu" or a.background == "mci"):
        ap.error("--output-size source needs --resize-on gpu and is not supported with --background mci")
    if a.poses == "keyframes" and a.rate & (a.rate - 1):
        ap.error("--poses keyframes needs a power-of-two --rate")
    if a.frames == "none" and not a.video:
        ap.error("--frames none is a setting of --video")
    if a.background == "mci" and a.resize_on == "gpu":
        ap.error("--background mci with --resize-on gpu is not supported")
    if a.mci_range != 32 and a.background != "mci":
        ap.error("--mci-range is a setting of --background mci")
    if a.mci_precision != "full" and a.background != "mci":
        ap.error("--mci-precision is a setting of --background mci")
    if a.mci_person != "keep" and a.background != "mci":
        ap.error("--mci-person is a setting of --background mci")
    if a.mci_detail != "model" and (a.background != "mci" or a.output_size != "keyframes"):
        ap.error("--mci-detail keyframes is a setting of --background mci --output-size keyframes")
    if a.mci_sampler != "bilinear" and a.background != "mci":
        ap.error("--mci-sampler is a setting of --background mci")
    if a.mci_motion != "linear" and (a.background != "mci" or (a.output_size == "keyframes" and a.mci_detail != "keyframes")):
        ap.error("--mci-motion quadratic is a setting of --background mci, with --output-size keyframes only together with --mci-detail keyframes")
    if a.mci_border != "clamp" and a.background != "mci":
        ap.error("--mci-border is a setting of --background mci")
    if a.panel_encode != "host" and not a.panels:
        ap.error("--panel-encode is a setting of --panels")
    if a.pose_mask and not a.metrics:
        ap.error("--pose-mask is a setting of --metrics")
    H, W = (a.height or a.size), (a.width or a.size)
    cfg = rib.AttrDict(gen=rib.hsm_gen_config(), model_height=H, model_width=W, gauss_sigma=5, skeleton_thres=0.001, foot_thres=0.001)
    spec = rib.GenSpec.from_cfg(cfg.gen)
    G = rib.Generator(cfg.gen, compute_dtype=a.dtype).eval()
    G.load_state_dict(synth.make_state_dict(spec, 0, power_iters=3))
    with tempfile.TemporaryDirectory() as root:
        n = write_clip(root, a.keys, a.rate, H, W, a.src_height, a.src_width, gt=a.metrics, dain=a.background != "mci")
        E = ev.Evaluator(cfg, lanes=a.lanes, batch=a.batch or None, chunk=a.chunk, io_threads=a.io_threads or None,
                         png_compress_level=None if a.compress < 0 else a.compress, io_mode=a.io_mode, resize_on=a.resize_on)
        dirs = [os.path.join(root, d) for d in ("inputs", "DAIN", "Predict_motion")]
        if a.background == "mci":
            dirs[1] = None
        kw, stage1_ms = {}, None
        if a.poses == "keyframes":
            from render_in_between_amd.motion import model as mmodel, pose_io, synth as msynth
            from render_in_between_amd.motion.spec import MotionSpec
            mspec = MotionSpec()
            tr = mmodel.MotionTransformer(mspec)
            tr.load_state_dict(msynth.make_state_dict(mspec, 0))
            motion = mmodel.ModelInference(mmodel.PositionEmbeddingSine1D(mspec.pos_hidden_dim // 2, normalize=True), tr,
                                           dataset=pose_io.OpenPoseClips({}))
            dirs[2] = None
            kw = dict(poses="keyframes", key_pose_dir=os.path.join(root, "key_poses"), upsample_rate=a.rate, motion=motion)
            motion.interpolate_clip(os.path.join(root, "key_poses", "clip"), a.rate)            # warm
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            motion.interpolate_clip(os.path.join(root, "key_poses", "clip"), a.rate)
            e1.record(); e1.synchronize()
            stage1_ms = e0.elapsed_time(e1)     # host reading of the key-pose files included: the events bracket the whole call
        walls = []
        for rep in range(1 + a.reps):           # the first run also builds launch plans and pools: not counted
            t0 = time.perf_counter()
            out = E.evaluate_from_folder(G, *dirs, os.path.join(root, "out%d" % rep), gt_dir=os.path.join(root, "gt") if a.metrics else None,
                                         metrics=a.metrics, pose_mask=a.pose_mask, panels=a.panels, panel_encode=a.panel_encode,
                                         background=a.background, video=a.video, frames=a.frames, **kw,
                                         **({"output_size": a.output_size} if a.output_size != "model" else {}),
                                         **({"png_on": a.png_on} if a.png_on != "host" else {}),
                                         **({"mci_range": a.mci_range} if a.background == "mci" else {}),
                                         **({"mci_border": a.mci_border} if a.mci_border != "clamp" else {}),
                                         **({"mci_precision": a.mci_precision} if a.mci_precision != "full" else {}),
                                         **({"mci_person": a.mci_person} if a.mci_person != "keep" else {}),
                                         **({"mci_sampler": a.mci_sampler} if a.mci_sampler != "bilinear" else {}),
                                         **({"mci_detail": a.mci_detail} if a.mci_detail != "model" else {}),
                                         **({"mci_motion": a.mci_motion} if a.mci_motion != "linear" else {}))
            torch.cuda.synchronize()
            walls.append(time.perf_counter() - t0)
        tm = dict(E.timings)
        png_bytes = sum(os.path.getsize(f) for f in out if f.endswith(".png"))
        overall = dict(E.metrics_report["overall"]) if a.metrics else None
    gen = n - a.keys
    wall = sorted(walls[1:])[len(walls[1:]) // 2]
    print(json.dumps({"height": H, "width": W, "dtype": a.dtype, "frames": n, "generated": gen, "lanes": a.lanes,
                      "batch": a.batch or E.default_batch(), "chunk": a.chunk, "io_threads": E.io_threads, "io_mode": a.io_mode,
                      "cpus": len(os.sched_getaffinity(0)), "cpu_budget": ev.cpu_budget(), "png_compress_level": a.compress,
                      "src_height": a.src_height or H, "src_width": a.src_width or W, "resize_on": a.resize_on, "output_size": a.output_size, "background": a.background, "mci_range": a.mci_range if a.background == "mci" else None,
                      "mci_border": a.mci_border if a.background == "mci" else None,
                      "mci_precision": a.mci_precision if a.background == "mci" else None,
                      "mci_person": a.mci_person if a.background == "mci" else None,
                      "mci_sampler": a.mci_sampler if a.background == "mci" else None,
                      "mci_detail": a.mci_detail if a.background == "mci" else None,
                      **({"mci_motion": a.mci_motion} if a.mci_motion != "linear" else {}),
                      "metrics": a.metrics, "pose_mask": a.pose_mask, "metrics_overall": overall, "panels": a.panels, "panel_encode": a.panel_encode,
                      "video": a.video, "frames_written": a.frames, "png_on": a.png_on, "png_bytes_last_run": png_bytes, "poses": a.poses, "stage1_plus_bridge_ms_per_clip": stage1_ms,
                      "wall_s": wall, "wall_s_runs": [round(w, 4) for w in walls[1:]], "frames_per_s_end_to_end": n / wall,
                      "phase_s_last_run": {k: round(v, 4) for k, v in tm.items() if k not in ("frames", "units", "timeline", "peak_units_in_flight")},
                      "peak_units_in_flight": tm.get("peak_units_in_flight"),
                      "unit_timeline_s [decoded, enqueued, on host, written]": tm.get("timeline"),
                      "pipeline_units_last_run": tm.get("units")}))


if __name__ == "__main__":
    main()
