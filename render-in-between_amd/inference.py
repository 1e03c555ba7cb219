#!/usr/bin/env python3
"""Drop-in for PGNR/inference.py: same flags, same config keys, same directory contract.

    python render-in-between_amd/inference.py --input-dir ../example [--config configs/HSM.yaml]
                                               [--save-dir ../example] [--seed 123]

Unlike the reference it builds only what inference needs: the generator (no discriminator, VGG
perceptual loss, optimisers or h5 dataset; PGNR/models/trainer.py:61-113).

Multi-GPU (new; the reference is single-device): `--gpus N` starts N ranks, one per GPU (or launch it under
torch.distributed.run yourself).  Rank 0 reads and folds the checkpoint, the folded blob reaches the other ranks in
ONE RCCL broadcast, and the independent segments between key frames (PGNR/models/evaluator.py:240-244) of all clips
(:169-171) are dealt round-robin to the ranks; every rank writes its own frames into the same output tree.

Ground-truth metrics (new; the reference measures only in evaluate_from_dataset): `--gt-dir DIR --metrics [--mask-dir DIR | --pose-mask]`
measures every generated frame and its DAIN frame against DIR/<clip>/ (PSNR / SSIM of Evaluator.compute_metrics) and writes
<save-dir>/Generated_frames/metrics.json.  `--pose-mask` measures under the human-centric mask the reference measures under
(_generate_human_mask, drawn from each frame's own pose on the GPU; restated from OpenCV's drawing, unpinned).

Diagnostic sheets (the counterpart of the reference's gen_vid=True): `--panels [--panel-frames] [--panel-quality Q] [--panel-fps N]`
composes, per frame, Predict | Mask | Fuse over DAIN | Ground Truth | Skeleton on the GPU and writes
<save-dir>/Generated_frames/<clip>.avi (Motion-JPEG in a plain RIFF AVI: no H.264 encoder is available here; the layout and the
titles are this project's, not matplotlib's); `--panel-frames` keeps the lossless sheets in <clip>_panels/%04d.png.
`--panel-encode gpu` encodes the video's JPEG frames on the GPU (rib_jpeg: baseline 4:2:0 with PIL's tables and one restart
segment per MCU row, bit-equal to panel.jpeg_encode_host; the stream is ours, restated from ITU-T T.81, unpinned) instead of
with PIL in the file workers (`host`, the default): the files' bytes come home instead of the raw sheets.

The frames as a video (new; the reference leaves that to an external encoder): `--video [--video-fps N] [--video-quality Q]
[--video-frames]` also writes every frame of a clip, key frames included, into <save-dir>/Generated_frames/<clip>_video.avi
(Motion-JPEG in a plain RIFF AVI; a frame is panel.jpeg_encode_host of exactly the bytes its PNG holds, encoded on the GPU from
the float frames by rib_jpeg_float; `--video-frames` keeps the .jpg files in <clip>_video/).  `--frames none` (with --video) writes
only the video: no PNG is encoded and the raw frames stay on the device.  Container and stream are this project's, unpinned: PIL
is the only decoder that has read them.

Lossless frames encoded on the GPU: `--png-on gpu` (default `host`: PIL in the file workers) writes every frame PNG - key frames
included - with rib_png on the lane's stream: per strip of 8 rows a PNG filter per row, runs at distance 1 as the only matches and
the cheapest of a fixed set of Huffman tables (png.py states every byte; stream and tables are this project's, every standard
decoder reads the file).  The same names and pixels as the default run, other file bytes: typically the size of zlib level 1,
larger than level 6 on smooth content and than level 1 on flat graphics; frames up to 4096 wide.  Not with --frames none or an
explicit --png-level; --panel-frames sheets stay with the host workers.

Backgrounds without a DAIN folder: `--background mci` makes every background frame on the GPU from the segment's two key
frames - a classical motion-compensated interpolation (background.py states it in integers; rib_mci_field / rib_mci_frames) -
and never reads <input>/DAIN.  It is this project's interpolation, not DAIN: the generator was trained on DAIN backgrounds, the
quality on real footage has not been measured, and motion beyond +-32 px between key frames falls outside the search.
`--mci-range 64` or `128` (default 32) widens the search by a fourth and a fifth pyramid level: the field then reaches 78 or 158 px
of motion between key frames (38 at the default) for six or seven launches per group of segments where the default takes five.
Still no occlusion reasoning, and a wider search has more room for a false match on periodic content.
`--mci-border valid` (default `clamp`) is one-sided at the frame border: a strip that enters or leaves the frame between the two
key frames is matched on, and taken from, the key frame that shows it, where `clamp` blends it with a smear of the other key
frame's edge column.  Frame border only: a foreground object that covers background inside the frame is not handled.
`--mci-precision half` (default `full`): the search is in whole pixels, so the motion between two key frames is always written as
an even number; one more launch per group (rib_halfpel_refine) refines every block's vector by half a pixel and the frames are sampled
from that field (rib_halfpel_frames).  Half-pel samples are bilinear and soft; a block whose whole-pixel vector is more than one
half-pel step from the truth stays wrong; no quarter-pel.
`--mci-person exclude` (default `keep`): the driver knows where the person is in both key frames - it reads their poses - and the
block matcher otherwise matches person pixels against background pixels, so every in-between background carries a half-transparent
ghost of the person where key frame A has them and another where B has them.  `exclude` takes the human masks of the two key
frames' poses (rib_human_mask) as excluded pixels: they do not count in the matching (rib_masked_field), and a pixel that only one
key frame shows without the person is that key frame's sample alone (rib_masked_frames).  The limits, plainly: the mask is the
reference's coarse pose mask, so hair, loose clothing and carried objects outside it still ghost; there is a hard seam where
cleanliness flips; only the person is handled, not other moving objects; background hidden in both key frames stays a blend; the
generator and its mask network were trained on DAIN frames that show a blurred person; quality on real footage is unmeasured.
Not yet with `--mci-precision half` nor `--output-size keyframes`.
`--mci-sampler cubic` (default `bilinear`): a bilinear sample at a fractional position is a low-pass filter that disappears where
the offset is a whole pixel - at k = 0, k = s and often k = s / 2 of a segment - so the background pulses between sharp and soft at
the key-frame rate.  `cubic` takes every background sample as a 4x4 Catmull-Rom sample (rib_cubic_frames; under `--output-size
keyframes` also the full-size backgrounds, rib_cubic_scaled); frames at whole-pixel offsets keep their bytes.  It combines with every
setting above.  The limits, plainly: Catmull-Rom overshoots at strong edges and the result is clamped; with `--mci-person exclude`
the exclusion footprint is 4x4, so the clean / blend seam moves by a pixel; it is still this project's interpolation, without
interior occlusion reasoning; the generator was trained on DAIN backgrounds; quality on real footage is unmeasured.
Frames are then named after their pose files.  The default, `--background dain`, is the reference's contract.

Poses without a Predict_motion folder: `--poses keyframes --pose-dir DIR [--upsample-rate N] [--motion-config PATH]` runs stage 1
(the motion transformer, motion/inference.py) inside this command: DIR/<clip>/ holds one OpenPose json per key frame, each clip is
interpolated N-fold on the GPU and its keypoints go straight from the network's output to the frames' rasteriser tables
(ribm_openpose; motion/pose_io.py:openpose_arrays states what the json files in between would have held, bit for bit) - the
frames are the two-command run's.  <input-dir>/Predict_motion is not read.  `keyframes-linear` takes the linearly interpolated
clip (stage 1's Linear_motion folder); `--save-poses` also writes <save-dir>/Predict_motion and <save-dir>/Linear_motion as stage 1's
own command does.  With `--background mci --video --frames none` one command turns key frames and their detections into the clip.

The interpolated backgrounds at the key frames' own size: `--background mci --output-size keyframes` writes the PNGs and the --video
clip at the size of the clip's key frame files (one size per clip; e.g. 1920x1080) where `--output-size model` squashes them to
the model size.  The motion field stays the model-size one; only the background pixels are sampled from the full-size key frames
(rib_scaled_frames, background.mci_frames_scaled_host) and the generated person is composited over them (rib_composite).  The one
command is then `--poses keyframes --pose-dir DIR --background mci --output-size keyframes --video --frames none`.  It is this
project's interpolation, not DAIN; the field has the model's resolution (motion detail finer than an 8x8 model block, about 30 px
at 1080p from 512, is not followed); the person is a cubic enlargement; no interior occlusion reasoning; unmeasured on real footage.
`--mci-detail keyframes` (default `model`; only with `--background mci --output-size keyframes`): the model-size field holds whole
model pixels - multiples of 3.75 output pixels at 512 -> 1920 - so a block's two samples are misregistered by up to one quantum and
the full-size background is a soft double image even where the field is right.  One more search per group, at the key frames' own
size (rib_detail_field, background.mci_detail_field_host): every 8x8 block of the full-size frame starts from the scaled model-size
vector and looks +-R whole output pixels around it (R = half the quantum, at most 4), then the median; the full-size backgrounds are
the existing frame kernels' on the full-size key frames with that field.  The model-size frames the generator reads do not change.
The limits, plainly: it is this project's interpolation, not DAIN; no interior occlusion reasoning; a model-size vector that is
wrong stays wrong beyond R; above a size ratio of 8 the radius no longer covers the quantum; whole pixels only at full size (below
ratio 2 `--mci-precision half` is finer); the person is still a cubic enlargement; real footage is unmeasured.
`--mci-motion quadratic` (default `linear`; only with `--background mci`): between two key frames everything above moves the
background at constant velocity, so its velocity jumps at every key frame while the person's poses follow curved trajectories.
With `quadratic` a segment also reads the key frames before and after it; the three motion fields give every block an acceleration
(rib_accel_field, background.mci_accel_host) and both samples of every pixel move by a t (1 - t) / 2 (rib_accel_frames,
background.mci_frames_accel_host).  The limits, plainly: second order from three fields - a wrong neighbour field gives a wrong
correction and the median is the only guard; no interior occlusion reasoning; about three times the field work per group; with
`--output-size keyframes` only together with `--mci-detail keyframes`; real footage is unmeasured.
"""
import argparse
import os
import random
import sys

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(_HERE))

import render_in_between_amd as rib                                   # noqa: E402
from render_in_between_amd.evaluator import Evaluator                 # noqa: E402


def load_generator(config, device=None, rank=0, world=1, dtype="f32"):
    """trainer.net_G with its checkpoint (PGNR/models/trainer.py:61,67; utils/utils.py:107-119).  With several
    ranks only rank 0 touches the file; the others receive the folded weights (distributed.broadcast_weights)."""
    net_G = rib.Generator(config.gen, device=device, compute_dtype=dtype)
    path = config.model_pretrain_G
    if not os.path.isfile(path):
        raise ValueError("=> No checkpoint found at '{}'".format(path))
    err = None
    if rank == 0:
        try:
            checkpoint = torch.load(path, map_location="cpu")
            print("=> Loaded checkpoint '{}'".format(path))
            net_G.load_state_dict(checkpoint)
        except Exception as e:                  # noqa: BLE001  (re-raised below, on every rank)
            if world == 1:
                raise
            err = e
    if world > 1:
        from render_in_between_amd import distributed as ribdist
        # only rank 0 touched the file: the other ranks learn here whether the broadcast will happen at all
        try:
            ribdist.agree_or_raise(err is None, "rank 0 could not load '{}': {!r}".format(path, err), net_G.device)
        except RuntimeError:
            if err is not None:
                raise err
            raise
        ms = ribdist.broadcast_weights(net_G, src=0)
        if rank == 0:
            print("=> weights broadcast to {} ranks in {:.1f} ms".format(world, ms))
    return net_G


def load_motion(path, device=None):
    """Stage 1 for --poses keyframes: the motion transformer with its checkpoint and the dataset that reads a key-pose folder
    (motion/inference.py:load_model; every rank loads the 2 M parameters itself)."""
    from render_in_between_amd.motion import inference as stage1, pose_io
    config = stage1.get_config(path)
    return stage1.load_model(config, device, dataset=pose_io.OpenPoseClips(config))


def summary_line(evaluator, rank=0, world=1):
    """One line per rank at the end of a run: what was rendered and where the wall time went.  The phases are the launch
    thread's waits (load: for decoded inputs; rasterise + generate: enqueueing the GPU work; save: the encode tail after the
    last enqueue); the file-side work itself runs in `workers` processes on `cpu_budget` cores beside them."""
    from render_in_between_amd.evaluator import cpu_budget
    tm = evaluator.timings
    wall = max(tm.get("wall", 0.0), 1e-9)
    line = ("[rank %d/%d] %d frames in %.2f s = %.1f frames/s | load %.2f s, rasterise %.2f s, generate %.2f s, save tail %.2f s | "
            "%d units, <= %d in flight | %d file workers (%s), CPU budget %d cores | PNG level %s, batch %d, %s plans | resize on %s | background %s"
            % (rank, world, tm.get("frames", 0), wall, tm.get("frames", 0) / wall, tm.get("load", 0.0), tm.get("rasterise", 0.0),
               tm.get("generate", 0.0), tm.get("save", 0.0), tm.get("units", 0), tm.get("peak_units_in_flight", 0),
               evaluator.io_threads, evaluator.io_mode, cpu_budget(),
               "reference (zlib 6)" if evaluator.png_compress_level is None else str(evaluator.png_compress_level),
               evaluator.batch or evaluator.default_batch(), "batch-invariant" if evaluator.reproducible else "per-batch",
               getattr(evaluator, "resize_on", "host"),
               {"dain": "DAIN frames", "mci": "mci (interpolated from the key frames, range %d px, border %s%s)"
                       % (getattr(evaluator, "mci_range", 32), getattr(evaluator, "mci_border", "clamp"),
                          (", half-pel" if getattr(evaluator, "mci_precision", "full") == "half" else "")
                          + (", person excluded" if getattr(evaluator, "mci_person", "keep") == "exclude" else "")
                          + (", cubic sampler" if getattr(evaluator, "mci_sampler", "bilinear") == "cubic" else "")
                          + (", field refined at the key frames' size" if getattr(evaluator, "mci_detail", "model") == "keyframes" else "")
                          + (", quadratic motion" if getattr(evaluator, "mci_motion", "linear") == "quadratic" else ""))}
               [getattr(evaluator, "background", "dain")]))
    if getattr(evaluator, "output_size", "model") == "source":
        line += " | files at the source size"
    if getattr(evaluator, "output_size", "model") == "keyframes":
        line += " | files at the key frames' size"
    rep = getattr(evaluator, "metrics_report", None)
    if "metrics" in tm and rep is not None:
        o = rep["overall"]
        line += (" | metrics over %d frames: DAIN PSNR %.4f SSIM %.6f, OURS PSNR %.4f SSIM %.6f, metric time %.2f s"
                 % (o["frames"], o["DAIN_PSNR"], o["DAIN_SSIM"], o["OURS_PSNR"], o["OURS_SSIM"], tm["metrics"]))
    return line


def main(opts):
    from render_in_between_amd import distributed as ribdist
    if opts.gpus > 1 and not ribdist.is_rank_process():
        # not a rank yet: start one process per GPU (before anything here touches the GPU) and hand back their exit code
        sys.exit(ribdist.self_launch(os.path.abspath(__file__), sys.argv[1:], opts.gpus))
    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    random.seed(opts.seed)
    np.random.seed(opts.seed)
    torch.manual_seed(opts.seed)
    config = rib.get_config(opts.config)
    config.out_dir = opts.save_dir
    config.eval_dir = opts.save_dir
    device = None
    if world > 1:
        device = torch.device("cuda", ribdist.rank_device_index())
        torch.cuda.set_device(device)
        ribdist.init_process_group(os.environ.get("RIB_DIST_BACKEND"), device)
    net_G = load_generator(config, device, rank, world, opts.dtype)
    evaluator = Evaluator(config, batch=opts.batch or None, reproducible=opts.reproducible,
                          png_compress_level=None if opts.png_level == "reference" else int(opts.png_level), resize_on=opts.resize_on)
    train_dir = os.path.join(opts.input_dir, "inputs")
    dain_dir = os.path.join(opts.input_dir, "DAIN") if opts.background == "dain" else None
    pose_dir = os.path.join(opts.input_dir, "Predict_motion") if opts.poses == "folder" else None
    poses_kw = {}
    if opts.poses != "folder":
        poses_kw = dict(poses=opts.poses, key_pose_dir=opts.pose_dir, upsample_rate=8 if opts.upsample_rate is None else opts.upsample_rate,
                        motion=load_motion(opts.motion_config or os.path.join(_HERE, "configs", "motion.yaml"), device), save_poses=opts.save_poses)
    save_dir = os.path.join(opts.save_dir, "Generated_frames")
    written = evaluator.evaluate_from_folder(net_G, train_dir, dain_dir, pose_dir, save_dir, gt_dir=opts.gt_dir, gen_vid=False,
                                             metrics=opts.metrics, mask_dir=opts.mask_dir, pose_mask=opts.pose_mask,
                                             panels=opts.panels, panel_frames=opts.panel_frames,
                                             panel_quality=90 if opts.panel_quality is None else opts.panel_quality,
                                             panel_fps=30 if opts.panel_fps is None else opts.panel_fps,
                                             panel_encode=opts.panel_encode or "host", background=opts.background, mci_range=opts.mci_range,
                                             mci_border=opts.mci_border, mci_precision=opts.mci_precision, mci_person=opts.mci_person,
                                             mci_sampler=opts.mci_sampler, mci_detail=opts.mci_detail, video=opts.video, video_fps=30 if opts.video_fps is None else opts.video_fps,
                                             video_quality=90 if opts.video_quality is None else opts.video_quality,
                                             video_frames=opts.video_frames, frames=opts.frames, output_size=opts.output_size, png_on=opts.png_on,
                                             **({"mci_motion": opts.mci_motion} if opts.mci_motion != "linear" else {}), **poses_kw)
    print(summary_line(evaluator, rank, world))
    if world > 1:
        print("[rank {}/{}] wrote {} frames".format(rank, world, len(written)))
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()


def build_parser():
    parser = argparse.ArgumentParser(description="pose-guided neural rendering inference (MI355X)")
    parser.add_argument("--config", type=str, default=os.path.join(_HERE, "configs", "HSM.yaml"), help="Path to the config file.")
    parser.add_argument("--save-dir", type=str, default="../example", help="outputs path")
    parser.add_argument("--input-dir", type=str, required=True, help="input low FPS frames and pose input")
    parser.add_argument("--seed", type=int, default=123)
    parser.add_argument("--dtype", choices=("f32", "bf16", "f16"), default="f32",
                        help="f32: the reference's arithmetic (default); bf16 / f16: 16-bit storage, ~2x the frame rate, ~1e-2 / ~1e-3 mean deviation "
                             "(not in the reference: it is fp32 only)")
    parser.add_argument("--gpus", type=int, default=1, help="ranks to start, one per GPU (not in the reference: it is single-device)")
    parser.add_argument("--batch", type=int, default=0,
                        help="independent segments rendered as one chain of that batch size (0: by frame size - 8 at 320x480, 4 at 512x512; "
                             "1: one chain per segment)")
    parser.add_argument("--png-level", default="reference",
                        help="'reference' (default): PIL's default deflate level 6, the very bytes PGNR/utils/utils.py:139-142 writes - 54 ms of "
                             "CPU per 512x512 frame, i.e. the end-to-end rate is bound by the host cores (~200 frames/s on 16); 0-9: that zlib "
                             "level - same pixels, other file bytes (1: ~2x the end-to-end rate, ~25 %% larger files)")
    parser.add_argument("--png-on", choices=("host", "gpu"), default="host",
                        help="where the frames' PNG files are encoded. 'host' (default): PIL in the file workers, at --png-level; 'gpu': the "
                             "HIP encoder (rib_png; png.py states the stream: run-length plus table-selected Huffman, this project's own) - "
                             "the same names and pixels, other file bytes, about the size of zlib level 1; not with --frames none or an "
                             "explicit --png-level")
    parser.add_argument("--reproducible", action=argparse.BooleanOptionalAction, default=True,
                        help="(default) every group size follows the kernel choices of the full group, so a frame's bytes do not depend "
                             "on segment grouping, on --gpus N or on --batch 1 vs N-rank shares; --no-reproducible lets ragged groups "
                             "run their own measured tables (frames then agree to ~1e-5, at most one uint8 step)")
    parser.add_argument("--gt-dir", type=str, default=None,
                        help="ground-truth frames, <gt-dir>/<clip>/*.png at the high frame rate (the reference's commented-out flag, "
                             "PGNR/inference.py:34): key frames and chain starts come from it, and the keypoints scale with its size")
    parser.add_argument("--metrics", action="store_true",
                        help="measure every generated frame and its DAIN frame against --gt-dir (PSNR / SSIM of compute_metrics, on the "
                             "GPU); writes <save-dir>/Generated_frames/metrics.json (not in the reference's folder driver)")
    parser.add_argument("--mask-dir", type=str, default=None,
                        help="with --metrics: <mask-dir>/<clip>/ grayscale masks at the model size (value > 127 = measured pixel)")
    parser.add_argument("--pose-mask", action="store_true",
                        help="with --metrics, instead of --mask-dir: measure under the human-centric mask the reference measures under, "
                             "drawn on the GPU from each frame's own pose json (_generate_human_mask: a disc on every joint, a thick line "
                             "on every limb; restated from OpenCV's drawing, unpinned)")
    parser.add_argument("--resize-on", choices=("host", "gpu"), default="host",
                        help="where the DAIN frames (and, with --metrics, the ground-truth frames) are resized to the model size: 'host' "
                             "(default): by the file workers, as the reference does; 'gpu': decoded at their own size and resized by the "
                             "HIP kernel, bit-exact to the host resize - the same files, less CPU per frame when the inputs are larger "
                             "than the model size (key frames stay on the host)")
    parser.add_argument("--panels", action="store_true",
                        help="also compose a six-pane diagnostic sheet per frame on the GPU (Predict, Mask, Fuse / DAIN, Ground Truth, "
                             "Skeleton) and write <save-dir>/Generated_frames/<clip>.avi, Motion-JPEG (the counterpart of the "
                             "reference's gen_vid; the frames themselves are unchanged)")
    parser.add_argument("--panel-frames", action="store_true",
                        help="with --panels: keep the lossless sheets as <clip>_panels/%%04d.png (the reference's save_frame)")
    parser.add_argument("--panel-quality", type=int, default=None, help="with --panels: JPEG quality of the video's frames, 1-100 (default 90)")
    parser.add_argument("--panel-fps", type=float, default=None, help="with --panels: frames per second of the video (default 30)")
    parser.add_argument("--panel-encode", choices=("host", "gpu"), default=None,
                        help="with --panels: where the video's JPEG frames are encoded. 'host' (default): PIL in the file workers; 'gpu': "
                             "the HIP encoder (baseline 4:2:0, PIL's tables, a restart segment per MCU row; --panel-quality applies to both)")
    parser.add_argument("--background", default="dain",
                        help="where the background frames come from. 'dain' (default): <input-dir>/DAIN/<clip>/, one frame per output "
                             "frame, as the reference; 'mci': interpolated on the GPU from each segment's two key frames (motion-compensated, "
                             "this project's, not DAIN; the generator was trained on DAIN backgrounds and the quality on real footage has "
                             "not been measured) - no DAIN folder is read, frames are named after their pose files")
    parser.add_argument("--mci-range", type=int, default=None,
                        help="with --background mci: the motion between two key frames the search covers, 32 (default), 64 or 128 px "
                             "(3, 4 or 5 pyramid levels; the field reaches 38, 78 or 158 px; five, six or seven launches per group of "
                             "segments). Fast pans and passing objects want 64 or 128; a wider search has more room for a false match "
                             "on periodic content, and there is still no occlusion reasoning; the search is in whole pixels (see --mci-precision)")
    parser.add_argument("--mci-border", default=None,
                        help="with --background mci: what happens where a sample leaves the frame. 'clamp' (default): matching and "
                             "sampling read the edge pixel; 'valid': one-sided at the frame border - a block is matched on the pixels both "
                             "key frames show, a pixel that only one key frame shows is that key frame's sample alone (a hard switch), so a "
                             "strip entering or leaving the frame shows its content, not a smear. Frame border only: no occlusion "
                             "reasoning inside the frame")
    parser.add_argument("--mci-precision", default=None,
                        help="with --background mci: the unit of the motion field. 'full' (default): whole pixels, so the motion between "
                             "two key frames is an even number of pixels; 'half': one more launch per group refines every block's vector "
                             "by half a pixel (bilinear half-pel samples, soft; a block more than one half-pel step from the truth stays "
                             "wrong; no quarter-pel)")
    parser.add_argument("--mci-person", default=None,
                        help="with --background mci: 'keep' (default): the person's pixels take part in the matching, and every "
                             "in-between background carries a ghost of the person at both key frames' positions; 'exclude': the human "
                             "masks of the two key frames' poses are kept out of the matching, and a pixel that only one key frame shows "
                             "without the person is that key frame's sample alone. The mask is the reference's coarse pose mask (hair, "
                             "loose clothing and carried objects outside it still ghost); a hard seam where cleanliness flips; only the "
                             "person, not other moving objects; background hidden in both key frames stays a blend; the generator was "
                             "trained on DAIN frames that show a blurred person; unmeasured on real footage. Not yet with "
                             "--mci-precision half (no masked refinement) nor --output-size keyframes (no masked rib_scaled_frames)")
    parser.add_argument("--mci-sampler", default=None,
                        help="with --background mci: 'bilinear' (default): the in-between backgrounds turn soft wherever the offset is "
                             "fractional and sharp where it is whole, so they pulse at the key-frame rate; 'cubic': every background "
                             "sample is a 4x4 Catmull-Rom sample (with --output-size keyframes also the full-size backgrounds); frames "
                             "at whole-pixel offsets keep their bytes. Works with every other --mci-* setting. Catmull-Rom overshoots "
                             "at strong edges and the result is clamped; with --mci-person exclude the exclusion footprint is 4x4, so "
                             "the clean/blend seam moves by a pixel; still this project's interpolation, without interior occlusion "
                             "reasoning; the generator was trained on DAIN backgrounds; quality on real footage is unmeasured")
    parser.add_argument("--mci-motion", default=None,
                        help="with --background mci: 'linear' (default): between two key frames the background moves at constant "
                             "velocity, so across the clip its velocity jumps at every key frame and the person - whose poses follow "
                             "curved trajectories - slides against it; 'quadratic': the fields of the segments before and after give "
                             "every 8x8 block an acceleration a and both samples of a pixel move by a t (1 - t) / 2 (a / 8 in the "
                             "middle of a segment). A clip's first and last segment use the one-sided difference, a clip of one "
                             "segment gets the linear files. About three times the field work per group. Second order from three "
                             "fields: a wrong neighbour field gives a wrong correction and the 3x3 median is the only guard; still no "
                             "interior occlusion reasoning; with --output-size keyframes only together with --mci-detail keyframes; "
                             "quality on real footage is unmeasured")
    parser.add_argument("--mci-detail", default=None,
                        help="with --background mci --output-size keyframes: 'model' (default): the full-size backgrounds follow the "
                             "model-size motion field, whose vectors are whole model pixels (multiples of 3.75 output pixels at 512 -> "
                             "1920), so a block's two samples are misregistered by up to one quantum - a soft double image; 'keyframes': "
                             "one more search per group at the key frames' own size refines every 8x8 full-size block's vector by up to "
                             "+-R whole output pixels (R = half the quantum, at most 4), and the existing frame kernels sample the "
                             "full-size key frames with that field. Still this project's interpolation, without interior occlusion "
                             "reasoning; a wrong model-size vector stays wrong beyond R; the radius is capped above a size ratio of 8; "
                             "the person is still a cubic enlargement; quality on real footage is unmeasured")
    parser.add_argument("--video", action="store_true",
                        help="also write every frame of a clip, key frames included, as <save-dir>/Generated_frames/<clip>_video.avi "
                             "(Motion-JPEG; a frame is the JPEG of exactly the bytes its PNG holds, encoded on the GPU)")
    parser.add_argument("--video-fps", type=float, default=None, help="with --video: frames per second of the video (default 30)")
    parser.add_argument("--video-quality", type=int, default=None, help="with --video: JPEG quality of the video's frames, 1-100 (default 90)")
    parser.add_argument("--video-frames", action="store_true", help="with --video: keep the frames' JPEG files as <clip>_video/%%04d.jpg")
    parser.add_argument("--frames", choices=("png", "none"), default="png",
                        help="'png' (default): the reference's folder of PNG frames; 'none' (only with --video): the video is the only "
                             "output - no PNG is encoded or written, the raw frames are not downloaded")
    parser.add_argument("--output-size", choices=("model", "source", "keyframes"), default="model",
                        help="'model' (default): every file at the model size, as the reference; 'source' (needs --resize-on gpu): the "
                             "PNGs and the --video clip at the size of the clip's DAIN frames - the background keeps every source pixel, "
                             "the generated person is a cubic enlargement of the model-size prediction (softer than its surroundings and "
                             "than the key frames, which are their files' own pixels), blended on the GPU in one launch; --metrics and "
                             "--panels stay at the model size; not with --background mci; 'keyframes' (a setting of --background mci): "
                             "the same at the key frames' size - the PNGs and the --video clip at the size of the clip's key frame files, "
                             "the interpolated background sampled from the full-size key frames with the model-size motion field (motion "
                             "detail finer than an 8x8 model block is not followed), the person composited over it")
    parser.add_argument("--poses", default="folder",
                        help="where the frames' poses come from. 'folder' (default): <input-dir>/Predict_motion/<clip>/, one OpenPose json per "
                             "output frame, as the reference (written by motion/inference.py); 'keyframes': --pose-dir holds one json per KEY "
                             "frame and the motion transformer interpolates them inside this command - the same frames, no Predict_motion "
                             "folder; 'keyframes-linear': the same from the linearly interpolated poses (stage 1's Linear_motion)")
    parser.add_argument("--pose-dir", type=str, default=None, help="with --poses keyframes*: <pose-dir>/<clip>/*.json, the key frames' OpenPose detections")
    parser.add_argument("--upsample-rate", type=int, default=None, help="with --poses keyframes*: output frames per key-frame interval, a power of two (default 8)")
    parser.add_argument("--motion-config", type=str, default=None, help="with --poses keyframes*: stage 1's config file (default configs/motion.yaml)")
    parser.add_argument("--save-poses", action="store_true",
                        help="with --poses keyframes*: also write <save-dir>/Predict_motion/<clip>/ and <save-dir>/Linear_motion/<clip>/, the "
                             "json files of stage 1's own command (for inspection; nothing reads them)")
    return parser


def parse_args(argv=None):
    parser = build_parser()
    opts = parser.parse_args(argv)
    if opts.png_level != "reference" and opts.png_level not in [str(i) for i in range(10)]:
        parser.error("--png-level must be 'reference' or a zlib level 0-9")
    if opts.png_on == "gpu" and opts.png_level != "reference":
        parser.error("--png-on gpu writes this project's own stream: --png-level is a setting of the host encoder")
    if opts.png_on == "gpu" and opts.frames != "png":
        parser.error("--png-on gpu encodes the frames' PNG files: not with --frames %s" % opts.frames)
    if opts.background not in ("dain", "mci"):
        parser.error("--background must be 'dain' or 'mci', got %r" % (opts.background,))
    if opts.poses not in ("folder", "keyframes", "keyframes-linear"):
        parser.error("--poses must be 'folder', 'keyframes' or 'keyframes-linear', got %r" % (opts.poses,))
    if opts.poses == "folder" and (opts.pose_dir is not None or opts.upsample_rate is not None or opts.motion_config is not None or opts.save_poses):
        parser.error("--pose-dir, --upsample-rate, --motion-config and --save-poses are settings of --poses keyframes / keyframes-linear")
    if opts.poses != "folder" and opts.pose_dir is None:
        parser.error("--poses %s needs --pose-dir (the key frames' OpenPose json folders)" % opts.poses)
    if opts.upsample_rate is not None and (opts.upsample_rate < 1 or opts.upsample_rate & (opts.upsample_rate - 1)):
        parser.error("--upsample-rate must be a power of two")
    if opts.mci_range is not None and opts.background != "mci":
        parser.error("--mci-range is a setting of --background mci")
    if opts.mci_range not in (None, 32, 64, 128):
        parser.error("--mci-range must be 32, 64 or 128, got %r" % (opts.mci_range,))
    opts.mci_range = 32 if opts.mci_range is None else opts.mci_range
    if opts.mci_border is not None and opts.background != "mci":
        parser.error("--mci-border is a setting of --background mci")
    if opts.mci_border not in (None, "clamp", "valid"):
        parser.error("--mci-border must be 'clamp' or 'valid', got %r" % (opts.mci_border,))
    opts.mci_border = "clamp" if opts.mci_border is None else opts.mci_border
    if opts.mci_precision is not None and opts.background != "mci":
        parser.error("--mci-precision is a setting of --background mci")
    if opts.mci_precision not in (None, "full", "half"):
        parser.error("--mci-precision must be 'full' or 'half', got %r" % (opts.mci_precision,))
    opts.mci_precision = "full" if opts.mci_precision is None else opts.mci_precision
    if opts.mci_person is not None and opts.background != "mci":
        parser.error("--mci-person is a setting of --background mci")
    if opts.mci_person not in (None, "keep", "exclude"):
        parser.error("--mci-person must be 'keep' or 'exclude', got %r" % (opts.mci_person,))
    opts.mci_person = "keep" if opts.mci_person is None else opts.mci_person
    if opts.mci_sampler is not None and opts.background != "mci":
        parser.error("--mci-sampler is a setting of --background mci")
    if opts.mci_sampler not in (None, "bilinear", "cubic"):
        parser.error("--mci-sampler must be 'bilinear' or 'cubic', got %r" % (opts.mci_sampler,))
    opts.mci_sampler = "bilinear" if opts.mci_sampler is None else opts.mci_sampler
    if opts.mci_detail not in (None, "model", "keyframes"):
        parser.error("--mci-detail must be 'model' or 'keyframes', got %r" % (opts.mci_detail,))
    if opts.mci_detail is not None and opts.background != "mci":
        parser.error("--mci-detail is a setting of --background mci")
    if opts.mci_detail == "keyframes" and opts.output_size != "keyframes":
        parser.error("--mci-detail keyframes needs --output-size keyframes (the field is refined at the key frames' own size)")
    opts.mci_detail = "model" if opts.mci_detail is None else opts.mci_detail
    if opts.mci_motion not in (None, "linear", "quadratic"):
        parser.error("--mci-motion must be 'linear' or 'quadratic', got %r" % (opts.mci_motion,))
    if opts.mci_motion is not None and opts.background != "mci":
        parser.error("--mci-motion is a setting of --background mci")
    if opts.mci_motion == "quadratic" and opts.output_size == "keyframes" and opts.mci_detail != "keyframes":
        parser.error("--mci-motion quadratic with --output-size keyframes needs --mci-detail keyframes for now (the scaled entries take no "
                     "acceleration: a scaled acceleration in rib_scaled_frames / rib_cubic_scaled is the follow-up)")
    opts.mci_motion = "linear" if opts.mci_motion is None else opts.mci_motion
    if opts.mci_person == "exclude" and opts.mci_precision == "half":
        parser.error("--mci-person exclude with --mci-precision half is not supported yet: the half-pel refinement has no masked form "
                     "(a masked rib_halfpel_refine is the follow-up)")
    if opts.mci_person == "exclude" and opts.output_size == "keyframes":
        parser.error("--mci-person exclude with --output-size keyframes is not supported yet: rib_scaled_frames has no masked form "
                     "(the follow-up)")
    if opts.background == "mci" and opts.resize_on == "gpu":
        parser.error("--background mci with --resize-on gpu is not supported (there is no DAIN list to plan the GPU resize for)")
    if opts.output_size == "source" and opts.background == "mci":
        parser.error("--output-size source with --background mci is not supported: the interpolation runs at the model size; "
                     "use --output-size keyframes")
    if opts.output_size == "keyframes" and opts.background != "mci":
        parser.error("--output-size keyframes is a setting of --background mci (the size of the key frame files); with DAIN frames "
                     "use --output-size source")
    if opts.output_size == "source" and opts.resize_on != "gpu":
        parser.error("--output-size source needs --resize-on gpu: the background frames' source-size bytes are on the device only there")
    if opts.metrics and opts.gt_dir is None:
        parser.error("--metrics needs --gt-dir (the ground-truth frames)")
    if opts.mask_dir is not None and not opts.metrics:
        parser.error("--mask-dir is a setting of --metrics")
    if opts.pose_mask and not opts.metrics:
        parser.error("--pose-mask is a setting of --metrics")
    if opts.pose_mask and opts.mask_dir is not None:
        parser.error("--pose-mask and --mask-dir are two sources of the one mask: give one of them")
    if not opts.panels and (opts.panel_frames or opts.panel_quality is not None or opts.panel_fps is not None or opts.panel_encode is not None):
        parser.error("--panel-frames, --panel-quality, --panel-fps and --panel-encode are settings of --panels")
    if opts.panel_quality is not None and not 1 <= opts.panel_quality <= 100:
        parser.error("--panel-quality must be in 1..100")
    if opts.panel_fps is not None and not opts.panel_fps > 0:
        parser.error("--panel-fps must be positive")
    if opts.frames == "none" and not opts.video:
        parser.error("--frames none writes nothing unless --video is given")
    if not opts.video and (opts.video_frames or opts.video_quality is not None or opts.video_fps is not None):
        parser.error("--video-fps, --video-quality and --video-frames are settings of --video")
    if opts.video_quality is not None and not 1 <= opts.video_quality <= 100:
        parser.error("--video-quality must be in 1..100")
    if opts.video_fps is not None and not opts.video_fps > 0:
        parser.error("--video-fps must be positive")
    return opts


if __name__ == "__main__":
    main(parse_args())
