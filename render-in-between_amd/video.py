"""The folder driver's product as a video: every frame of a clip - key frames included - as a Motion-JPEG AVI next to (or, with
frames="none", instead of) the PNG folder (evaluate_from_folder(video=True), inference.py --video).

Definition.  Frame i of <save_dir>/<clip>_video.avi is panel.jpeg_encode_host(u8_i, quality), where u8_i is exactly the uint8
HWC array the driver writes as frame i's PNG: tensor2images of the fused frame (panel.quantise_host) for an in-between frame and
of the key frame's tensor for a key frame.  So decoding Generated_frames/<clip>/NAME.png and encoding it with the host
definition gives the video's frame, byte for byte.  No arithmetic is stated here: the only new statement is the composition
jpeg_encode_host(quantise_host(x)) of a float frame x (frame_host), which rib_jpeg_float (csrc/jpeg.hip.h, Generator.jpeg_f32)
evaluates on the GPU without the uint8 copy in between.

Files.  The rank that rendered frame i writes <save_dir>/<clip>_video/%04d.jpg; once every rank is done, rank 0 muxes the folder
into <clip>_video.avi with panel.write_mjpeg_avi (assemble) and removes the .jpg files unless they were asked for.  <clip>.avi
stays the name of the diagnostic sheets' video (panels=True).

Unpinned: the container is this project's RIFF writer and the stream this project's restatement of ITU-T T.81; PIL is the only
decoder that has read either here, no player has opened the file.
"""
import os

from . import panel


def video_dir(save_dir, clip):
    return os.path.join(save_dir, clip + "_video")


def frame_name(save_dir, clip, i):
    return os.path.join(video_dir(save_dir, clip), "%04d.jpg" % i)


def avi_name(save_dir, clip):
    return os.path.join(save_dir, clip + "_video.avi")


def check_settings(video, video_fps, video_quality, video_frames, frames, who="evaluate_from_folder", error=ValueError):
    """The argument rules of the driver and of the command line, stated once."""
    if frames not in ("png", "none"):
        raise error("%s: frames must be 'png' or 'none', got %r" % (who, frames))
    if not video:
        if frames == "none":
            raise error("%s: frames='none' writes nothing unless video=True" % who)
        if video_frames or video_quality != 90 or video_fps != 30:
            raise error("%s: video_fps, video_quality and video_frames are settings of video=True" % who)
        return
    if isinstance(video_quality, bool) or int(video_quality) != video_quality or not 1 <= int(video_quality) <= 100:
        raise error("%s: video_quality must be an integer in 1..100, got %r" % (who, video_quality))
    if not float(video_fps) > 0:
        raise error("%s: video_fps must be positive, got %r" % (who, video_fps))


def frame_host(x, quality=90):
    """THE definition of a video frame from a float frame x [3, H, W] in [-1, 1]: jpeg_encode_host(quantise_host(x))."""
    return panel.jpeg_encode_host(panel.quantise_host(x), quality)


def save_frame_host(u8, jpg_name, quality=90):
    """A frame's uint8 [H, W, 3] array - the one its PNG holds - -> its video frame's file (the host path of the driver)."""
    return panel.save_jpeg(panel.jpeg_encode_host(u8, quality), jpg_name)


def assemble(save_dir, clip, fps=30, keep_frames=False):
    """<save_dir>/<clip>_video/*.jpg in index order -> <save_dir>/<clip>_video.avi; then, unless keep_frames, the .jpg files
    and the folder are removed.  A pure function of the folder: whichever ranks wrote the frames, the video is the same.  A
    refused video (panel.write_mjpeg_avi: beyond AVI_MAX_BYTES) leaves every file in place."""
    d = video_dir(save_dir, clip)
    jpgs = [os.path.join(d, f) for f in sorted(os.listdir(d)) if f.endswith(".jpg")]
    out = panel.write_mjpeg_avi(jpgs, avi_name(save_dir, clip), fps)
    if not keep_frames:
        for p in jpgs:
            os.remove(p)
        try:
            os.rmdir(d)
        except OSError:
            pass                                                # something else lives there: leave it
    return out
