"""Sequence driver: the build's restatement of Evaluator.evaluate_from_folder
(PGNR/models/evaluator.py:165-269) on top of the MI355X generator.

Directory contract (PGNR/inference.py:30-35): <input>/inputs/<clip>/*.png are the low-FPS key
frames, <input>/DAIN/<clip>/*.png the interpolated background frames, <input>/Predict_motion/
<clip>/*.json the high-FPS OpenPose joints; frames are written to
<save>/Generated_frames/<clip>/<dain-name>.png.

Differences from the reference, none of which change a pixel:
  * a segment (the frames between two key frames) runs as ONE device-side chain
    (rib_chain): `prev` never leaves HBM and there is no per-frame .cpu() sync
    (evaluator.py:260-262 syncs every frame);
  * the output quantisation runs on the GPU (rib_quantise);
  * the label maps of a whole segment are drawn on the GPU in one call (rib_rasterise) instead of
    per frame with scipy / numpy loops on the host (evaluator.py:221-229);
  * independent segments of equal length are BATCHED: up to `batch` of them run as one chain of batch B
    (rib_chain(T, B, ..): sample b of every step is segment b's frame), which is what fills the 256 CUs on
    the 32x32 / 64x64 maps; a chain is cut into time chunks of `chunk` steps whose first `prev`
    is the previous chunk's last fused frame on the device, so that decode, GPU work and PNG encode of
    different chunks overlap (a unit of the pipeline is `chunk` x B frames);
  * file decode / json -> rasteriser tables / PNG encode run in a pool of worker PROCESSES (io_worker.py) that read
    and write the frames in page-locked shared memory: the decoded frames of a chunk go up and its quantised
    frames come back in one asynchronous copy each, and the three phases are pipelined over chunks (SURVEY 8 row
    f-1: at hundreds of frames/s the per-frame .cpu() + PNG encode of evaluator.py:260-266 is the wall - and at PIL's
    default zlib level, the bytes the reference writes, it still is: 54 ms of CPU per 512x512 frame);
  * multi-GPU: the independent units (the segments between key frames, evaluator.py:240-244, over all clips,
    :169-171) are dealt round-robin to the ranks of the process group (distributed.shard_units); every rank
    decodes, renders and writes only its own frames, with no communication after the weight broadcast.

Ground-truth metrics (metrics=True with a gt_dir; the reference measures in evaluate_from_dataset, evaluator.py:113-134): every
non-key frame (i % sample_rate != 0; at sample_rate 2 exactly the reference's rule, :116) is measured twice against gt_dir's
frame i - its fused frame (OURS) and its DAIN frame (DAIN) - with compute_metrics' PSNR / SSIM (metrics.py), optionally under
a mask: files from mask_dir/<clip>/, or (pose_mask=True) the human-centric mask the reference measures under, drawn from the
frame's own pose (rasterise.human_mask; on the native path by the HIP kernel behind Generator.human_mask, from the peak table the
unit already carries).  The native path decodes the GT frame in the frame's own decode task, measures on the GPU
(rib_quality) right after the unit's chain and brings the per-frame values home in the unit's one device-to-host copy.
<save_dir>/metrics.json reports every clip (the reference keeps only the last clip's dict) and the mean over all frames.
"""
from __future__ import annotations

import collections
import contextlib
import math
import os
import time
from concurrent.futures import ThreadPoolExecutor
from typing import List

import numpy as np
import torch

from . import background as _background
from . import composite as _composite
from . import io_worker, rasterise
from . import metrics as _metrics
from . import panel as _panel
from . import resize as _resize
from . import video as _video


def sample_rate_of(num_pose: int, num_key: int) -> int:
    """evaluator.py:190."""
    return 2 ** int(np.log2((num_pose - 1) / (num_key - 1)))


def split_segments(seq_len: int, sample_rate: int):
    """Frame indices: key frames (i % sample_rate == 0) pass through unchanged
    (evaluator.py:240-244); each run of generated frames between them is one independent
    autoregressive segment starting from the preceding key frame."""
    keys = [i for i in range(seq_len) if i % sample_rate == 0]
    segs = []
    for k in keys:
        frames = [i for i in range(k + 1, min(k + sample_rate, seq_len))]
        if frames:
            segs.append((k, frames))
    return keys, segs


_PROC_POOLS = {}
# A task whose worker process died never completes under multiprocessing.Pool (the pool replaces the worker, not the task):
# every wait on file-side work is bounded, so that a lost task ends the call with an error instead of hanging it.
IO_TIMEOUT_S = 300.0
# Windows of the pipeline, in units (a unit = chunk x B frames): decode runs at most DECODE_AHEAD units ahead of the unit being
# enqueued, and at most MAX_UNITS_IN_FLIGHT units are enqueued but not yet written - host and device memory are bounded by the
# windows, not by the length of the clip.
DECODE_AHEAD = int(os.environ.get("RIB_DECODE_AHEAD", "6"))
MAX_UNITS_IN_FLIGHT = int(os.environ.get("RIB_MAX_UNITS_IN_FLIGHT", "10"))


class _ProcessPool:
    """n worker processes with a concurrent.futures face (submit -> Future).  forkserver: the workers are forked from a clean
    server process that never saw the GPU (a plain fork of a process with an initialised HIP runtime is not safe), with this
    package's file-side module preloaded so that a fork is cheap.  multiprocessing would also re-run the parent's __main__
    script in every worker ("__mp_main__": for a driver script that means importing torch 32 times, which is what made the first
    version of this pool 3x slower than threads); the workers only ever run io_worker functions, so __main__ is hidden
    while they are started - multiprocessing.Pool starts all of them in its constructor."""

    def __init__(self, n):
        import multiprocessing as mp
        import sys
        ctx = mp.get_context("forkserver")
        ctx.set_forkserver_preload(["render_in_between_amd.io_worker", "PIL.Image", "PIL.PngImagePlugin", "scipy.optimize"])
        main = sys.modules.get("__main__")
        saved = {k: getattr(main, k) for k in ("__file__", "__spec__") if hasattr(main, k)}
        # one BLAS / OpenMP thread per worker (io_worker.warm says why); the variables are read when the forkserver imports numpy
        threads_env = {k: os.environ.get(k) for k in ("OPENBLAS_NUM_THREADS", "OMP_NUM_THREADS", "MKL_NUM_THREADS")}
        try:
            if hasattr(main, "__file__"):
                del main.__file__
            if main is not None:
                main.__spec__ = None
            for k in threads_env:
                os.environ[k] = "1"
            self._pool = ctx.Pool(n, initializer=io_worker.warm)
        finally:
            for k, v in saved.items():
                setattr(main, k, v)
            for k, v in threads_env.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v
        self.n = n

    def submit(self, fn, *args, **kw):
        from concurrent.futures import Future
        fut = Future()
        fut.set_running_or_notify_cancel()
        self._pool.apply_async(fn, args, kw, callback=fut.set_result, error_callback=fut.set_exception)
        return fut

    def shutdown(self):
        self._pool.terminate()


class _ShmBlock:
    """A block of POSIX shared memory that worker processes open by name (io_worker._attach) and that is also page-locked
    for the GPU (hipHostRegister), so that the upload of decoded frames and the download of quantised frames are asynchronous
    copies straight out of / into the memory the workers write / read.  `t`: the block as a flat uint8 tensor."""

    def __init__(self, nbytes):
        from multiprocessing import shared_memory
        self.nbytes = int(nbytes)
        self.shm = shared_memory.SharedMemory(create=True, size=self.nbytes)
        self.name = self.shm.name
        # tmpfs hands out pages on first touch, and a touch beyond what /dev/shm has left is a bus error in whichever process
        # makes it (a decode worker, typically): reserve the pages now, so that exhaustion is an OSError here
        try:
            os.posix_fallocate(self.shm._fd, 0, self.nbytes)
        except (AttributeError, OSError) as e:
            if isinstance(e, OSError):
                self.shm.close(); self.shm.unlink(); self.shm = None
                raise MemoryError("Evaluator: /dev/shm cannot hold a %.1f MB staging block (%s); use io_mode='thread' or a larger /dev/shm"
                                  % (self.nbytes / 1e6, e)) from e
        self.t = torch.from_numpy(np.ndarray((self.nbytes,), np.uint8, buffer=self.shm.buf))
        self.pinned = False
        if torch.cuda.is_available():
            try:
                self.pinned = int(torch.cuda.cudart().cudaHostRegister(self.t.data_ptr(), self.nbytes, 0)) == 0
            except Exception:                                   # noqa: BLE001 (not pinned: the copies are synchronous, still correct)
                self.pinned = False

    def close(self):
        if self.shm is None:
            return
        if self.pinned:
            try:
                torch.cuda.cudart().cudaHostUnregister(self.t.data_ptr())
            except Exception:                                   # noqa: BLE001
                pass
        self.t = None
        try:
            self.shm.close()
            self.shm.unlink()
        except Exception:                                       # noqa: BLE001
            pass
        self.shm = None


_SHM_FREE = {}          # nbytes -> [idle _ShmBlock]: blocks are reused across units and calls (creating + page-locking one costs ms)
_SHM_ALL = []


_SHM_GRAIN = 1 << 20          # block sizes are rounded up to this: ragged groups / tail chunks then share a few size classes
_SHM_KEEP = DECODE_AHEAD + MAX_UNITS_IN_FLIGHT + 4      # idle blocks kept per size class (the pipeline's windows); the rest is released


def _shm_get(nbytes):
    nbytes = (int(nbytes) + _SHM_GRAIN - 1) // _SHM_GRAIN * _SHM_GRAIN
    free = _SHM_FREE.get(nbytes)
    if free:
        return free.pop()
    if not _SHM_ALL:
        import atexit
        atexit.register(_shm_close_all)
    blk = _ShmBlock(nbytes)
    _SHM_ALL.append(blk)
    return blk


def _shm_put(blk):
    """Back to the free list.  Nothing is unmapped here: while a call is running, tensor views of the block may still be
    referenced (a unit's staging dict, the default arguments of a finisher that is still on the stack), and closing the
    mapping under them turns a later access into a segfault instead of an exception.  Surplus blocks are
    released by _shm_trim() at the end of evaluate_from_folder, when no unit is alive."""
    _SHM_FREE.setdefault(blk.nbytes, []).append(blk)


def _shm_trim():
    """Release the idle blocks beyond _SHM_KEEP per size class (unregister, unmap, unlink).  Worker processes drop their own
    attachment of an unlinked block the next time they attach a new one (io_worker._attach)."""
    for free in _SHM_FREE.values():
        while len(free) > _SHM_KEEP:
            blk = free.pop()
            _SHM_ALL.remove(blk)
            blk.close()


def _shm_close_all():
    for blk in _SHM_ALL:
        blk.close()
    _SHM_ALL.clear()
    _SHM_FREE.clear()


def block_layout(sections):
    """The layout of a unit's staging block or download buffer: sections = [(name, nbytes)] in buffer order ->
    ({name: (offset, nbytes)}, total bytes).  Every section starts on a multiple of 256 - any dtype may be viewed there, on
    the device and in a shared block - and a section of no bytes is left out."""
    table, end = {}, 0
    for name, nbytes in sections:
        if nbytes:
            off = (end + 255) // 256 * 256
            table[name] = (off, nbytes)
            end = off + nbytes
    return table, end


def spec_bytes(spec):
    """A block's spec [(name, dtype, shape, on)] as block_layout's sections: a section that is off takes no bytes."""
    return [(name, math.prod(shape) * dtype.itemsize if on else 0) for name, dtype, shape, on in spec]


def section_views(flat, spec, table):
    """The typed views of a buffer laid out by `table`, on the device or on the host: {name: view} over every section of the
    spec, None where the table has no such section."""
    views = dict.fromkeys(name for name, _, _, _ in spec)
    for name, dtype, shape, _ in spec:
        if name in table:
            off, nbytes = table[name]
            views[name] = flat[off:off + nbytes].view(dtype).view(shape)
    return views


def staging_spec(Tc, Bc, model_hw, src_dain=None, src_gt=None, want_gt=False, masks=False, keys=False, mci=False, mci_keys=False,
                 src_keys=None, mci_keys_src=None, mci_quad=False):
    """The spec of a unit's staging block, which the decode tasks fill and upload() sends to the GPU (DESIGN 4e has the table):
    Tc time steps of Bc segments at the model size (H, W).  src_dain / src_gt: (w0, h0) at which that list is staged for the
    GPU resize (resize_on="gpu"), None: the model size; want_gt, masks: ground-truth frames / masks are staged; keys: a first
    chunk under panels, the DAIN frames of the key frames it starts from; mci: background="mci", no DAIN bytes at all;
    mci_keys: its first chunk, the group's left and right key frames.  src_keys: (w0, h0) - a first chunk under
    output_size="source" with video, the key frames it starts from at the output size, for their video files; the section
    `key_src` exists in the spec only then.  mci_keys_src: (w0, h0) - a group's first chunk under output_size="keyframes", its
    left and right key frames' own pixels for rib_scaled_frames; the section `mci_keys_src` exists only then, after `key_src`.
    mci_quad: mci_motion="quadratic" - both key-frame sections hold FOUR key frames per member: left, right, the one before the left
    and the one after the right (MCI_KEY_ROLES; where the clip has none, the left / right one again)."""
    H, W = model_hw
    (wd, hd), (wg, hg) = src_dain or (W, H), src_gt or (W, H)
    nk = len(MCI_KEY_ROLES) if mci_quad else 2
    spec = (("dain", torch.uint8, (Tc, Bc, hd, wd, 3), not mci),
            ("gt", torch.uint8, (Tc, Bc, hg, wg, 3), want_gt),
            ("mask", torch.uint8, (Tc, Bc, H, W), masks),
            ("key", torch.uint8, (Bc, H, W, 3), keys and not mci),
            ("mci_keys", torch.uint8, (nk, Bc, H, W, 3), mci and mci_keys))
    if src_keys is not None:
        spec += (("key_src", torch.uint8, (Bc, src_keys[1], src_keys[0], 3), True),)
    if mci_keys_src is not None:
        spec += (("mci_keys_src", torch.uint8, (nk, Bc, mci_keys_src[1], mci_keys_src[0], 3), True),)
    return spec


MCI_KEY_ROLES = (0, 1, -1, 2)               # the key frames of a member's `mci_keys` / `mci_keys_src`, in segments from its left key frame


def mci_key_frames(k, sample_rate, seq_len, quad):
    """The key frames a segment starting at frame k stages for its backgrounds, in the sections' order: [left, right], and under
    mci_motion="quadratic" also the key frame before and the one after (MCI_KEY_ROLES) -> ([frame index], (has_prev, has_next)).
    A neighbour the clip does not have stands in as the left / right key frame itself and is flagged absent."""
    roles = MCI_KEY_ROLES if quad else MCI_KEY_ROLES[:2]
    has = (k - sample_rate >= 0, k + 2 * sample_rate <= seq_len - 1)
    idx = [k + r * sample_rate for r in roles]
    if quad:
        idx[2], idx[3] = (idx[2] if has[0] else k), (idx[3] if has[1] else k + sample_rate)
    return idx, has


def _process_pool(n):
    """One pool of n worker processes per size for the whole process (Evaluators come and go; 32 interpreters should not)."""
    pool = _PROC_POOLS.get(n)
    if pool is None:
        import atexit
        pool = _PROC_POOLS[n] = _ProcessPool(n)
        atexit.register(pool.shutdown)
    return pool


def cpu_budget():
    """CPUs this process can actually use: the affinity mask, capped by the cgroup's CPU quota (a GPU box of the pool shows 256
    CPUs and grants 16 cores' worth of time: more file workers than that only take turns - profiles/r04_encode_probe.txt)."""
    try:
        n = len(os.sched_getaffinity(0))
    except AttributeError:
        n = os.cpu_count() or 1
    for path in ("/sys/fs/cgroup/cpu.max", ):
        try:
            with open(path) as f:
                quota, period = f.read().split()[:2]
            if quota != "max":
                n = min(n, max(1, int(int(quota) / int(period))))
        except (OSError, ValueError):
            pass
    try:                                                        # cgroup v1
        with open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us") as f:
            quota = int(f.read())
        with open("/sys/fs/cgroup/cpu/cpu.cfs_period_us") as f:
            period = int(f.read())
        if quota > 0 and period > 0:
            n = min(n, max(1, quota // period))
    except (OSError, ValueError):
        pass
    return n


def _shm_free_bytes():
    """Bytes /dev/shm can still hand out, plus the staging blocks this process already holds (they are reused, not allocated again)."""
    try:
        st = os.statvfs("/dev/shm")
        free = st.f_bavail * st.f_frsize
    except OSError:
        free = 0
    return free + sum(b.nbytes for b in _SHM_ALL)


def shm_windows_bytes(unit_bytes):
    """Shared staging memory the pipeline's windows need when one unit stages `unit_bytes`."""
    return (DECODE_AHEAD + MAX_UNITS_IN_FLIGHT + 4) * int(unit_bytes)


def plan_gpu_resize(dain_sizes, gt_sizes, model_size, slots_per_unit, mask=False, shm_free=None, out_slot_bytes=0):
    """Which frame lists of a clip does Evaluator(resize_on="gpu") stage at their SOURCE size for the GPU resize
    (rib_resize_cubic), and which fall back to the host resize?  A pure function of sizes and budgets.
    dain_sizes / gt_sizes: [(w0, h0)] header sizes of the clip's DAIN frames / measured ground-truth frames (gt_sizes None: no
    metrics); model_size (W, H); slots_per_unit: frames of one pipeline unit (chunk x batch); mask: a mask is staged per slot
    too; shm_free: bytes the shared staging blocks may take (None: staging is not in shared memory, no budget applies);
    out_slot_bytes: bytes per slot by which the unit's download block, which lies in the same shared memory, exceeds the model
    size's (output_size="source": a frame at the source size), counted over the same windows.
    -> ({"DAIN": (w0, h0) or None, "GT": (w0, h0) or None}, [(list name, reason)]): the source size of each list that goes to
    the GPU (None: host resize) and one reason per list that was asked for and falls back.
    Rules: the sizes inside a list must be uniform (the two lists may differ from each other); then the unit's staging block
    at the real per-slot bytes must fit the pipeline's windows in shm_free - if it does not, the GT list goes back to the model
    size first, then the DAIN list."""
    W, H = model_size
    src, why = {"DAIN": None, "GT": None}, []
    for name, sizes in (("DAIN", dain_sizes), ("GT", gt_sizes)):
        if sizes is None:
            continue
        kinds = sorted(set(tuple(s_) for s_ in sizes))
        if len(kinds) == 1:
            src[name] = kinds[0]
        elif kinds:
            why.append((name, "mixed frame sizes (%s)" % ", ".join("%dx%d" % k for k in kinds[:4])))
    if shm_free is not None:
        def need():
            per_slot = sum((s_[0] * s_[1] if s_ is not None else W * H) * 3 for n_, s_ in src.items() if n_ == "DAIN" or gt_sizes is not None)
            return shm_windows_bytes(slots_per_unit * (per_slot + (W * H if mask else 0) + out_slot_bytes))
        for name in ("GT", "DAIN"):
            if src[name] is not None and need() > shm_free:
                why.append((name, "the staging windows at %dx%d need %.0f MB of shared memory, %.0f MB are free"
                            % (src[name][0], src[name][1], need() / 1e6, shm_free / 1e6)))
                src[name] = None
    return src, why


def normalise_exact(u8):
    """ToTensor + Normalize(0.5, 0.5) of uint8 [.., H, W, 3] frames on their device, bit-equal to what the HOST computes
    (io_worker.normalised_chw: float32(u8) / 255 correctly rounded, then (a - 0.5) / 0.5) -> float32 [.., 3, H, W], contiguous.
    torch evaluates `x / 255.0` on the GPU as a multiplication by the fp32 reciprocal, which differs from the division in the
    last bit for 111 of the 256 values (csrc/resize.hip.h) - invisible to the generator, but the truncating quantiser turns it
    into a grey level, and the sheets' DAIN / Ground Truth panes are held to the bytes tensor2images makes of the host's
    tensor.  The quotient is formed in float64 and rounded once: n / 255 is never within 2^-9 ulp of a float32 rounding
    boundary (its binary expansion repeats n's 8 bits), so the result is the correctly rounded float32 quotient whichever
    way the float64 division is carried out."""
    a = (u8.to(torch.float64) / 255.0).to(torch.float32)
    return ((a - 0.5) / 0.5).movedim(-1, -3).contiguous()


def _list(d, exts):
    return [os.path.join(d, f) for f in sorted(os.listdir(d)) if f.endswith(exts)]


class Evaluator:
    def __init__(self, cfg, lanes=2, label_fn=None, png_compress_level=None, resize="cv2", batch=None, chunk=4, io_threads=None,
                 io_mode="process", reproducible=True, resize_on="host"):
        """batch: independent segments of equal length rendered as ONE chain of that batch size (None: by frame size,
        `default_batch`; 1: every segment on its own, the round-1..3 behaviour).
        reproducible (default True): every chain of the call - full groups, the ragged last group of a clip, a rank's
        smaller share in a multi-GPU run - follows the kernel choices of ONE batch size, the group size
        (Generator.set_plan_batch / rib_set_plan_batch): a frame's bytes do not depend on which segments were rendered
        beside it, so N ranks write what one rank writes ("rank r's frames == single-GPU frames bit-for-bit").
        False: every group size runs its own measured table (a ragged group of 1-3 segments is then a little faster and its
        frames differ from the batched ones by ~1e-5, i.e. at most one uint8 step on ~2e-3 of the pixels).
        chunk: time steps per rib_chain call (the pipeline's unit is chunk x B frames); 0 = whole segments.
        lanes: independent chains kept in flight on one GPU, each on its own HIP stream with
        its own generator handle (the frames inside a segment stay strictly sequential).
        io_threads: decode / encode workers (None: the CPUs this process may run on, divided by the ranks of the job
        sharing the host and by the cgroup's CPU quota (cpu_budget), minus one for the launch thread, at most 48).
        io_mode: "process" (default) runs the file-side work of the native pipeline - decode, json -> rasteriser tables,
        PNG encode - in a pool of worker processes shared by all Evaluators of this process (io_worker.py), so that it
        cannot hold the interpreter lock of the thread that enqueues the GPU work; "thread": a thread pool (rounds 1-3).
        A model that only speaks the reference's call protocol, or a label_fn, always uses threads.
        label_fn(frames, H, W) -> [T, 22, H, W]: rasteriser override for models that only speak the
        reference's call protocol (the tests pass the CPU oracle); by default the model's GPU
        rasteriser is used and a model without one is an error (no host fallback).
        resize: "cv2" = OpenCV INTER_CUBIC restated (resize.py; what the reference's A.Resize computes), "pil" = PIL BICUBIC.
        resize_on: "host" (default): the file workers resize every frame (resize.py); "gpu": the DAIN frames - and under
        metrics=True the ground-truth frames - are decoded at their own size and resized by the model's HIP kernel
        (Generator.resize_u8 / rib_resize_cubic, bit-exact to the host function, so the files are the same); needs
        resize="cv2" and a native model.  Key frames are resized on the host either way.  A clip whose list has mixed sizes,
        or whose source-size staging does not fit /dev/shm, falls back to the host resize for that list and says so."""
        if resize not in ("cv2", "pil"):
            raise ValueError("resize must be 'cv2' or 'pil'")
        if resize_on not in ("host", "gpu"):
            raise ValueError("resize_on must be 'host' or 'gpu'")
        if resize_on == "gpu" and resize != "cv2":
            raise ValueError("resize_on='gpu' needs resize='cv2' (PIL's BICUBIC is not on the GPU)")
        self.resize_on = resize_on
        if io_mode not in ("process", "thread"):
            raise ValueError("io_mode must be 'process' or 'thread'")
        self.io_mode = io_mode
        self.reproducible = bool(reproducible)
        self.resize = resize
        self.cfg = cfg
        self.lanes = max(1, int(lanes))
        self.label_fn = label_fn
        # PNG compression: None = PIL's default (zlib level 6), which is what the reference's Image.save(name) writes
        # (PGNR/utils/utils.py:139-142) - byte-identical files; a lower level trades file size for encode time
        self.png_compress_level = png_compress_level
        self.batch = None if batch is None else max(1, int(batch))
        self.chunk = max(0, int(chunk))
        ncpu = cpu_budget()
        # N ranks on one host share its cores: LOCAL_WORLD_SIZE (torchrun) or WORLD_SIZE ranks each take their part, and one
        # core per rank stays with the launch thread (5 k launches per 31-frame segment); more workers than cores only slow it
        ranks = max(1, int(os.environ.get("LOCAL_WORLD_SIZE", os.environ.get("WORLD_SIZE", "1")) or 1))
        self.io_threads = max(1, int(io_threads)) if io_threads else max(1, min(48, ncpu // ranks - 1))
        self._pool = None                                   # created on first use, kept across calls (thread start-up is ~2 ms each)
        self._finishers = None
        self.timings = {}                                   # seconds per phase of the last evaluate_from_folder
        self.metrics = None                                 # per-frame ground-truth records of the last call with metrics=True
        self.metrics_report = None                          # ... and the report written to <save_dir>/metrics.json
        self.height = cfg.model_height                      # HSM_auto_dataset.py:55-56
        self.width = cfg.model_width
        self.gauss_sigma = getattr(cfg, "gauss_sigma", 5)
        self.skeleton_thres = getattr(cfg, "skeleton_thres", 0.001)
        self.foot_thres = getattr(cfg, "foot_thres", 0.001)

    def _shm_fits(self, frames_per_slot=1.0):
        """Is there room in /dev/shm for the pipeline's windows of shared staging blocks?  (A container may mount 64 MB there,
        and a write beyond it is a bus error, not an exception: the file-side work then stays on threads, with a warning.)
        frames_per_slot: staged frames per output frame (metrics: DAIN + GT frame + mask)."""
        unit = int(max(1, self.chunk) * (self.batch or self.default_batch()) * self.height * self.width * 3 * frames_per_slot)
        need = shm_windows_bytes(unit)
        free = _shm_free_bytes()
        if free < need:
            import warnings
            warnings.warn("Evaluator: /dev/shm has %.0f MB free, the shared staging blocks of the worker processes need %.0f MB: "
                          "falling back to io_mode='thread'" % (free / 1e6, need / 1e6))
            return False
        return True

    def default_batch(self):
        """Segments per chain when the caller did not say: enough samples to fill 256 CUs on the deep (1/16-resolution,
        512-channel) layers without growing the working set past the MALL - 8 at the reference's 320x480, 4 at 512x512
        (measured: profiles/r04_driver.jsonl, r04_other_shapes.jsonl)."""
        px = self.height * self.width
        return 8 if px <= 320 * 480 else (4 if px <= 512 * 512 else (2 if px <= 1024 * 1024 else 1))

    @staticmethod
    def group_segments(segs, batch):
        """[(key, frames)] -> [[segment index, ..]]: runs of up to `batch` segments of EQUAL length, in segment order
        (a chain of batch B advances all its samples together, so they must have the same number of steps)."""
        groups, open_by_len = [], {}
        for si, (_, frames) in enumerate(segs):
            g = open_by_len.get(len(frames))
            if g is None:
                g = open_by_len[len(frames)] = []
                groups.append(g)
            g.append(si)
            if len(g) >= batch:
                del open_by_len[len(frames)]
        return groups

    def _lanes(self, model, nsegs):
        """(generator, stream) pairs for concurrent segments; None for single-lane / non-native models."""
        if self.lanes <= 1 or nsegs <= 1 or not hasattr(model, "clone"):
            return None
        ver = getattr(model, "weights_version", 0)
        cache = getattr(self, "_lane_cache", None)
        if cache is None or cache[0] is not model:
            gens = [model] + [model.clone() for _ in range(self.lanes - 1)]
            self._lane_cache = cache = (model, [(g, torch.cuda.Stream(device=model.device)) for g in gens], ver)
        elif cache[2] != ver:
            # the model got new weights (load_state_dict / import_weights) since the lanes were cloned: refresh the
            # clones' blobs, or segments would alternate between old and new weights
            blob = model.export_weights()
            for g, _ in cache[1][1:]:
                g.import_weights(blob)
            torch.cuda.current_stream(model.device).synchronize()
            self._lane_cache = cache = (model, cache[1], ver)
        for g, _ in cache[1][1:]:
            if hasattr(g, "set_plan_batch"):
                g.set_plan_batch(model.plan_batch)              # clones made by an earlier call may follow another policy
            if getattr(g, "_graph_replay", False):
                g.set_graph_replay(False)                       # (_plan_policy: no replay in the folder driver)
        return cache[1][:max(1, min(self.lanes, nsegs))]

    # ---- per-frame host pre-processing (evaluator.py:205-235) --------------------------------
    def _decode_resized_u8(self, path):
        """PIL decode -> RGB uint8 HWC at the model size.  `resize="cv2"` (default): OpenCV's 8-bit INTER_CUBIC restated
        in resize.py (what the reference's albumentations `A.Resize(interpolation=cv2.INTER_CUBIC)` computes: A = -0.75,
        no low-pass on reduction; unpinned, cv2 is not in this image); `resize="pil"`: PIL's BICUBIC (round 1)."""
        return io_worker.decode_resized_u8(path, self.width, self.height, self.resize)

    def load_image(self, path):
        """PIL open -> resize to the model size (cubic) -> [-1,1] CHW (ToTensor + Normalize(.5,.5));
        PGNR/models/evaluator.py:205-221 with `get_alb_transform` (:18-26)."""
        u8, size0 = self._decode_resized_u8(path)
        a = u8.astype(np.float32) / 255.0
        return torch.from_numpy((a - 0.5) / 0.5).permute(2, 0, 1).contiguous(), size0

    def load_image_u8(self, path):
        """The same decode + resize, left as uint8 HWC: the pipeline uploads a quarter of the bytes and
        applies ToTensor + Normalize(.5,.5) on the GPU (the same two fp32 operations, bit-identical)."""
        u8, size0 = self._decode_resized_u8(path)
        return torch.from_numpy(u8.copy()), size0

    def load_pose(self, json_path, orig_size):
        """json -> (landmarks, conf) in model-size pixels: the keypoints follow the image resize
        (A.Resize keypoint rule, evaluator.py:24-26,219)."""
        return io_worker.scaled_pose(json_path, orig_size, self.width, self.height)

    def make_labels(self, model, frames):
        """[(landmarks, conf)] -> [T, 22, H, W] label maps: 3-ch skeleton image in [-1,1] + 19
        heat-maps in [0,1] (evaluator.py:221-229,250)."""
        if self.label_fn is not None:
            return self.label_fn(frames, self.height, self.width)
        if not hasattr(model, "rasterise"):
            raise RuntimeError("this model has no GPU rasteriser (rib_rasterise); pass Evaluator(label_fn=...)")
        return rasterise.rasterise_labels(model, frames, self.height, self.width, self.gauss_sigma,
                                          self.skeleton_thres, self.foot_thres)

    @contextlib.contextmanager
    def _plan_policy(self, model, native):
        """reproducible: for the length of a call the generator (and, through Generator.clone, its lane clones) follows the
        kernel choices of the group size at every batch; the handle gets its own setting back afterwards.
        Graph replay (RIB_GRAPH=1 / set_graph_replay) is off for the call: every unit of the pipeline brings fresh label / DAIN
        tensors, i.e. other pointers, so each chain would capture and instantiate a graph of its own and none would ever
        replay - the launch-by-launch path is the faster one here; `bench.py --mode clips --graph` is where a
        segment is replayed."""
        if not (native and hasattr(model, "set_plan_batch")):
            yield
            return
        before = model.plan_batch
        graph = bool(getattr(model, "_graph_replay", False))
        model.set_plan_batch((self.batch or self.default_batch()) if self.reproducible else 0)
        if graph:
            model.set_graph_replay(False)
        try:
            yield
        finally:
            model.set_plan_batch(before)
            if graph:
                model.set_graph_replay(True)

    # ---- ground-truth metrics (evaluator.py:149-163) ------------------------------------------------
    def compute_metrics(self, pred, target, mask=None):
        """The reference's compute_metrics: frames [B,3,H,W] in [-1,1], mask [B,H,W] or None -> batch-mean (PSNR, SSIM) as 0-d
        tensors (piq's psnr(data_range=1, reduction='mean') and ssim(data_range=1), restated in metrics.py).  Device tensors
        are measured by the HIP kernels of the last native model this Evaluator drove, CPU tensors by the torch statement."""
        p, s_ = _metrics.psnr_ssim(pred, target, mask, model=getattr(self, "_quality_model", None))
        return p.mean(), s_.mean()

    # ---- the driver ------------------------------------------------------------------------------
    @torch.no_grad()
    def evaluate_from_folder(self, model, train_dir, dain_dir, pose_dir, save_dir, gt_dir=None, gen_vid=False,
                             rank=None, world=None, metrics=False, mask_dir=None, pose_mask=False,
                             panels=False, panel_frames=False, panel_quality=90, panel_fps=30, panel_encode="host",
                             background="dain", mci_range=32, video=False, video_fps=30, video_quality=90, video_frames=False, frames="png",
                             poses="folder", key_pose_dir=None, upsample_rate=8, motion=None, save_poses=False, mci_border="clamp",
                             mci_precision="full", output_size="model", png_on="host", mci_person="keep", mci_sampler="bilinear", mci_detail="model",
                             mci_motion="linear"):
        """rank / world: this process's share of the independent units (default: the torch.distributed process
        group when one is initialised, else everything).  Returns the frames THIS rank wrote.
        The call is one `_FolderPipeline` (below): plan a clip -> decode -> upload -> render -> sink, pipelined over units
        of `chunk` x B frames; the launch thread only enqueues, decode of later units and encode of finished ones overlap
        the GPU work.
        metrics=True (needs gt_dir): every non-key frame is measured against gt_dir's frame i, fused (OURS) and DAIN frame,
        optionally under mask_dir/<clip>/ masks (grayscale at the model size, > 127 -> 1); the per-frame records of all ranks
        end up in self.metrics and <save_dir>/metrics.json (written by rank 0).  metrics=False changes nothing.
        pose_mask=True (with metrics, instead of mask_dir): the mask of a measured frame is the reference's human-centric mask
        (_generate_human_mask restated from OpenCV's drawing, unpinned: rasterise.human_mask) of that frame's pose - on the
        native path drawn by rib_human_mask on the upload stream, next to the label rasterisation; nothing is staged for it.
        panels=True: every frame i - key frames included - also gets a six-pane diagnostic sheet (panel.py: Predict | Mask | Fuse
        over DAIN | Ground Truth | Skeleton; the Ground Truth pane is gt_dir's frame i, else the segment's left key frame),
        written by whichever rank rendered the frame to <save_dir>/<clip>_panels/%04d.jpg (JPEG quality panel_quality) and, with
        panel_frames, losslessly to %04d.png.  On the native path the sheets are composed by rib_panel on the lane's stream
        and ride home in the unit's one copy; a model that only speaks the reference's protocol goes through
        panel.compose_host.  Rank 0 then muxes <save_dir>/<clip>.avi (Motion-JPEG, panel_fps frames/s; panel.assemble) from the
        folder, removes the JPEG sheets and - unless panel_frames - the folder.  (Ranks without a process group cannot know when
        the others are done: the caller runs panel.assemble once they are.)  panels=False changes nothing.
        panel_encode="gpu" (with panels; default "host": PIL in the file workers, the files of before): the sheets' JPEG files
        are panel.jpeg_encode_host's bytes - baseline 4:2:0 with the tables PIL uses, one restart segment per MCU row, stated in
        integers - written on the native path by rib_jpeg right behind rib_panel: the lengths ride home in the unit's copy, the
        finisher then fetches exactly the files' bytes and writes %04d.jpg itself, no worker and no PIL involved; the raw sheets
        stay on the device unless panel_frames wants the lossless copies.  A model behind the reference's protocol encodes
        with jpeg_encode_host on the host: the same files.
        background="mci" (default "dain": one background frame per output frame from dain_dir, as the reference): the
        background frames are a motion-compensated interpolation of each segment's two key frames (background.py states it in
        integers; this project's interpolation, NOT DAIN - the generator was trained on DAIN backgrounds, the quality on real
        footage has not been measured, and motion beyond +-32 px between key frames falls outside the search).
        mci_range=64 or 128 (default 32; a setting of background="mci") widens that search to +-64 or +-128 px by a fourth and a
        fifth pyramid level (background.mci_field_host's levels = 4, 5): one more short launch per level and group, and more
        room for a false match on periodic content.  mci_border="valid" (default "clamp"; a setting of background="mci") makes
        matching and sampling one-sided at the FRAME border (background.py's border="valid"): a strip that only one key frame
        shows is taken from that key frame alone, not blended with a smear of the other's edge; occlusion inside the frame (a
        foreground object covering background) is not handled unless the person is excluded: mci_person="exclude" (default
        "keep"; a setting of background="mci") takes the human masks of a segment's two key frames' poses (rasterise.human_mask; on
        the native path rib_human_mask on the upload stream, once per group where the field is made) as EXCLUDED pixels: they do
        not count in the block matching (background.mci_field_masked_host; rib_masked_field), and where exactly one of a pixel's
        two samples avoids them the background is that sample alone (mci_frames_masked_host; rib_masked_frames).  The mask is
        the reference's coarse pose mask - hair, loose clothing and carried objects outside it still ghost; there is a hard
        seam where cleanliness flips; only the person is handled; background hidden in both key frames stays a blend; a key
        frame without a detected person has an all-zero mask.  It is refused with mci_precision="half" (the refinement has no
        masked form yet) and with output_size="keyframes" (rib_scaled_frames has none).  mci_precision="half" (default "full"; a setting of
        background="mci"): the integer field writes the motion between the key frames as an even number of pixels; one more
        launch per group (rib_halfpel_refine; background.mci_refine_host) refines every block's vector by half a pixel and the frames
        are sampled from that field (rib_halfpel_frames; mci_frames_host(precision="half")).  Half-pel samples are bilinear and
        soft, and a block whose integer vector is more than one half-pel step from the truth stays wrong.
        mci_sampler="cubic" (default "bilinear"; a setting of background="mci", legal with every combination above): every
        background sample is a 4x4 Catmull-Rom sample (background.sample_cubic; rib_cubic_frames / rib_cubic_scaled) in place of the
        bilinear one - the model-size floats the chain reads AND, under output_size="keyframes", the full-size backgrounds.  Frames
        whose offsets are whole pixels (k = 0, k = s, often k = s / 2) keep their bytes; the others no longer turn soft, so the
        background stops pulsing at the key-frame rate.  Catmull-Rom overshoots at strong edges (the result is clamped); the
        exclusion footprint of mci_person="exclude" is 4x4, so the clean / blend seam moves by a pixel; it is still this project's
        interpolation without interior occlusion reasoning, the generator was trained on DAIN backgrounds, and the quality on
        real footage is unmeasured.
        mci_detail="keyframes" (default "model"; only with background="mci" and output_size="keyframes"): the model-size field holds
        whole model pixels, so at full size a block's two samples are misregistered by up to one quantum (3.75 px at 512 -> 1920);
        one more search per group at the key frames' own size (rib_detail_field; background.mci_detail_field_host) refines every 8x8
        full-size block's vector by up to +-detail_radius whole output pixels, and the full-size backgrounds are the existing frame
        entry's (rib_mci_frames / rib_cubic_frames; mci_frames_host) on the full-size key frames with that field.  The model-size
        floats the chain reads are unchanged.  A wrong model-size vector stays wrong beyond the radius, which is capped at 4 (above a
        size ratio of 8 it no longer covers the quantum); no interior occlusion reasoning; unmeasured on real footage.
        mci_motion="quadratic" (default "linear"; a setting of background="mci"): between two key frames the background no longer moves
        at constant velocity.  A segment (k, k + s) also reads the key frames k - s and k + 2 s where the clip has them (decoded by
        the rank that renders the segment, so the files do not depend on ranks or grouping); the fields of the segments before and
        after come from the same field entry (with mci_person="exclude" from their own key frames' pose masks, with
        mci_precision="half" refined, with mci_detail="keyframes" refined at the key frames' size), all three in one batched call; one
        rib_accel_field per group (background.mci_accel_host) makes the block acceleration, and every unit's frames come from
        rib_accel_frames (mci_frames_accel_host): both samples of a pixel move by a t (1 - t) / 2.  A clip's first and last segment use
        the one-sided difference; a clip of one segment has zero acceleration and gets the linear files byte for byte.  About three
        times the field work per group.  Second order from three fields: a wrong neighbour field gives a wrong correction, the 3x3
        median is the only guard; no interior occlusion reasoning; unmeasured on real footage.  Refused for now with
        output_size="keyframes" unless mci_detail="keyframes" (the scaled entries rib_scaled_frames / rib_cubic_scaled take no
        acceleration yet).  dain_dir may be
        None and is never listed or read; a frame's file is named after its pose file (stem without a trailing "_keypoints").
        On the native path the field is made once per group of segments (rib_mci_field) and every unit's frames by one launch
        (rib_mci_frames) on the upload stream - no DAIN bytes are staged or decoded; a model behind the reference's protocol is
        fed mci_frames_host, normalised as the native upload normalises (background.normalised_upload): the same files.  The DAIN_* metrics and the sheets' DAIN pane then show the MCI frames.
        video=True: every frame i of a clip - key frames included - is also written as a JPEG file, <save_dir>/<clip>_video/%04d.jpg
        (quality video_quality), by whichever rank rendered it, and rank 0 then muxes <save_dir>/<clip>_video.avi (Motion-JPEG,
        video_fps frames/s; video.assemble) and removes the .jpg files unless video_frames keeps them.  (<clip>.avi stays the
        sheets' video; both may be asked for.  Ranks without a process group: the caller runs video.assemble.)  A frame's file is
        panel.jpeg_encode_host of exactly the uint8 array its PNG holds (video.py).  On the native path a unit's fused frames are
        encoded from their float tensors by one rib_jpeg_float on the lane's stream (a first chunk's key frames by another), the
        lengths ride home in the unit's one copy and the finisher fetches exactly the files' bytes and writes them: no worker,
        no PIL.  A model behind the reference's protocol encodes with jpeg_encode_host on the host: the same files.
        frames="none" (only with video=True; default "png"): no frame PNG is encoded, staged or written and the frames' raw bytes
        stay on the device; the call returns the names of the .jpg files this rank wrote.  video=False changes nothing.
        poses="keyframes" (default "folder": one OpenPose json per output frame under pose_dir/<clip>/, what stage 1's own
        command writes): stage 1 runs here.  key_pose_dir/<clip>/ holds one OpenPose json per KEY frame; `motion` is the
        motion model (motion.model.ModelInference built with its dataset: motion/inference.py:load_model(config, dataset=...));
        plan_clip interpolates the clip upsample_rate-fold (a power of two) with ModelInference.interpolate_clip - one forward
        pass, one bridge launch (ribm_openpose), one copy home per clip, run by every rank for itself - and frame i's decode
        task gets row i of that [L, 19, 3] array where it got a json path: exactly the array rasterise.read_json_keypoint
        returns for the file stage 1's command would have written (motion.pose_io.openpose_arrays), so every output is the
        two-command run's.  pose_dir may be None and is never listed, read or written; the clips are key_pose_dir's folders.
        Under background="mci" frame i is named "%06d" % i, the stem stage 1's command gives its file.  "keyframes-linear":
        the same from the linearly interpolated clip (stage 1's Linear_motion folder).  save_poses=True also writes
        <save_dir>/../Predict_motion/<clip>/ and Linear_motion/<clip>/ - beside save_dir, where stage 1's command run with
        the same --save-dir puts them - through that command's own motion2openpose (rank 0; for inspection).
        output_size="source" (default "model": every file at the model size, as the reference): the frames' PNGs and the video
        are written at the clip's SOURCE size, the uniform size (w0, h0) of its DAIN frames: an in-between frame is
        composite.composite_host of the chain's predicted image and blend mask and the DAIN file's own pixels - the person is
        a cubic enlargement of the model-size prediction (soft), the background keeps every source pixel - and a key frame is
        the key-frame file's own pixels (resize.resize_cubic_u8 to (w0, h0) if its size differs).  The chain itself, the
        metrics and the sheets stay at the model size.  On the native path this needs resize_on="gpu" (the source-size bytes
        are on the device only there): one rib_composite launch fills the `frames` section of the unit's download buffer, and
        with video the files come from rib_jpeg on those bytes; a clip whose DAIN list the plan sends back to the host resize
        (mixed sizes, shared-memory budget) is an error before any of its files is written.  A model behind the reference's
        protocol decodes each DAIN file once more at its own size and goes through composite_host, and its generator is fed the
        background floats the native chain reads (background.normalised_upload, as under background="mci"): the same files.
        background="mci" is not supported with it (the interpolation runs at the model size): that is output_size="keyframes".
        output_size="keyframes" (a setting of background="mci"): the same at the key frames' size - the files are written at
        the uniform size (w0, h0) of the clip's key frame files (a clip with mixed sizes is an error before any of its files is
        written; so is one whose larger blocks do not fit the shared memory).  The field stays exactly the model-size one
        (mci_field_host / mci_refine_host of the host-resized keys) and the chain reads the floats it reads under "model"; only
        the background pixels are sampled from the full-size key frames (background.mci_frames_scaled_host: the field at the
        model size, the samples at the key frames' size), an in-between frame is composite_host of the chain's image and mask
        over them and a key frame is its file's own pixels.  On the native path a group's first chunk also stages the key
        files' own pixels (`mci_keys_src`), one rib_scaled_frames launch per unit on the upload stream makes the unit's
        backgrounds, and render, composite, PNG workers and video are the code of "source".  It is this project's
        interpolation, not DAIN; motion detail finer than an 8x8 model block is not followed; the person is a cubic
        enlargement; no interior occlusion reasoning; unmeasured on real footage.
        png_on="gpu" (default "host": PIL in the worker processes, every file and launch as before): on the native path every
        frame PNG this rank writes - key frames included - is encoded on the lane's stream by rib_png from the device uint8
        frame the host workers would have been handed (rib_quantise's bytes at the model size, rib_composite's under
        output_size="source" / "keyframes", a key frame's own bytes), in the units and the order video=True encodes them; the
        lengths ride home in the unit's one copy (`png_len`), the finisher fetches exactly the files' bytes and writes them
        under the PNG's name, and no raw frame is staged or copied home for the PNG workers.  A file is png.encode_host of the
        pixels the default run's PNG holds: the same names and pixels, this project's stream (png.py), not the reference's
        bytes; W <= 4096.  Not with a model behind the reference's protocol, frames="none" or an explicit PNG level; the
        sheets' lossless copies (panel_frames) stay with the host workers, video=True may be combined and is unchanged."""
        if png_on not in ("host", "gpu"):
            raise ValueError("evaluate_from_folder: png_on must be 'host' or 'gpu', got %r" % (png_on,))
        if png_on == "gpu":
            if frames != "png":
                raise ValueError("evaluate_from_folder: png_on='gpu' encodes the frames' PNG files: not with frames=%r" % (frames,))
            if self.png_compress_level is not None:
                raise ValueError("evaluate_from_folder: png_on='gpu' writes this project's own stream (png.py): an explicit PNG level "
                                 "(png_compress_level=%r) is a setting of the host encoder" % (self.png_compress_level,))
            if not (hasattr(model, "chain") and hasattr(model, "quantise") and hasattr(model, "png_into")):
                raise ValueError("evaluate_from_folder: png_on='gpu' needs the native path (rib_png): this model only speaks the "
                                 "reference's protocol")
        if poses not in ("folder", "keyframes", "keyframes-linear"):
            raise ValueError("evaluate_from_folder: poses must be 'folder', 'keyframes' or 'keyframes-linear', got %r" % (poses,))
        if poses == "folder" and (key_pose_dir is not None or upsample_rate != 8 or motion is not None or save_poses):
            raise ValueError("evaluate_from_folder: key_pose_dir, upsample_rate, motion and save_poses are settings of poses='keyframes' / 'keyframes-linear'")
        if poses != "folder":
            if key_pose_dir is None:
                raise ValueError("evaluate_from_folder: poses=%r needs key_pose_dir (one OpenPose json per key frame)" % (poses,))
            if motion is None or not hasattr(motion, "interpolate_clip"):
                raise ValueError("evaluate_from_folder: poses=%r needs motion= (the motion model, motion.model.ModelInference)" % (poses,))
            if not (isinstance(upsample_rate, int) and upsample_rate >= 1 and upsample_rate & (upsample_rate - 1) == 0):
                raise ValueError("evaluate_from_folder: upsample_rate must be a power of two, got %r" % (upsample_rate,))
        _composite.check_output_size(output_size, "evaluate_from_folder")
        _background.check_detail(background, output_size, mci_detail)
        _background.check_motion(background, mci_motion, output_size=output_size, mci_detail=mci_detail)
        mci_levels, mci_border = _background.check_settings(background, mci_range, mci_border, self.resize_on, mci_precision=mci_precision,
                                                            mci_person=mci_person, output_size=output_size, mci_sampler=mci_sampler)
        if output_size == "source" and background == "mci":
            raise ValueError("evaluate_from_folder: output_size='source' with background='mci' is not supported: the interpolation "
                             "runs at the model size (a source-size interpolation is a follow-up); use output_size='keyframes'")
        if output_size == "keyframes" and background != "mci":
            raise ValueError("evaluate_from_folder: output_size='keyframes' is a setting of background='mci' (the size of the key "
                             "frame files); with DAIN frames use output_size='source'")
        if gen_vid:
            # the reference also writes <save_dir>/<clip>.mp4 (evaluator.py:267-269, utils.make_video) from a matplotlib canvas
            # through an H.264 encoder; neither is built, and silently ignoring the flag would drop an output the caller asked for
            raise NotImplementedError("evaluate_from_folder: gen_vid (the matplotlib / mp4 video) is not supported; panels=True "
                                      "writes the six-pane sheets as <save_dir>/<clip>.avi, video=True the frames themselves as "
                                      "<save_dir>/<clip>_video.avi")
        if panel_encode not in ("host", "gpu"):
            raise ValueError("evaluate_from_folder: panel_encode must be 'host' or 'gpu', got %r" % (panel_encode,))
        if not panels and (panel_frames or panel_quality != 90 or panel_fps != 30 or panel_encode != "host"):
            raise ValueError("evaluate_from_folder: panel_frames, panel_quality, panel_fps and panel_encode are settings of panels=True")
        if panels and not (1 <= int(panel_quality) <= 100 and float(panel_fps) > 0):
            raise ValueError("evaluate_from_folder: panel_quality must be in 1..100 and panel_fps positive")
        _video.check_settings(video, video_fps, video_quality, video_frames, frames)
        if metrics and gt_dir is None:
            raise ValueError("evaluate_from_folder: metrics=True needs gt_dir (the ground-truth frames)")
        if mask_dir is not None and not metrics:
            raise ValueError("evaluate_from_folder: mask_dir is a setting of metrics=True")
        if pose_mask and not metrics:
            raise ValueError("evaluate_from_folder: pose_mask is a setting of metrics=True")
        if pose_mask and mask_dir is not None:
            raise ValueError("evaluate_from_folder: pose_mask and mask_dir are two sources of the one mask: give one of them")
        if rank is None or world is None:
            import torch.distributed as dist
            rank, world = (dist.get_rank(), dist.get_world_size()) if dist.is_available() and dist.is_initialized() else (0, 1)
        model.eval()
        if self._pool is None:
            self._pool = ThreadPoolExecutor(self.io_threads)          # decode + encode workers
            self._finishers = ThreadPoolExecutor(max(4, self.lanes + 2))  # wait for a unit's copy, then fan out its encodes
        self.metrics = self.metrics_report = None
        pipe = _FolderPipeline(self, model, rank, world, gt_dir, metrics=bool(metrics), mask_dir=mask_dir, pose_mask=bool(pose_mask),
                               panels=bool(panels), panel_frames=bool(panel_frames), panel_quality=int(panel_quality),
                               panel_encode=panel_encode, background=background, mci_levels=mci_levels, mci_border=mci_border, mci_precision=mci_precision, mci_person=mci_person, mci_sampler=mci_sampler, mci_detail=mci_detail, video=bool(video), video_quality=int(video_quality),
                               video_frames=bool(video_frames), write_png=frames == "png", output_size=output_size, png_gpu=png_on == "gpu", mci_motion=mci_motion,
                               key_poses=None if poses == "folder" else (motion, key_pose_dir, upsample_rate, poses == "keyframes-linear", bool(save_poses)))
        self.background, self.mci_range, self.mci_border, self.mci_precision = background, mci_range, mci_border, mci_precision
        self.mci_person, self.mci_sampler, self.mci_detail, self.mci_motion = mci_person, mci_sampler, mci_detail, mci_motion
        self.output_size = output_size
        self.timings = pipe.tm
        if metrics and pipe.native:
            self._quality_model = model
        try:
            with self._plan_policy(model, pipe.native):
                clips_dir = pose_dir if poses == "folder" else key_pose_dir
                for sub in [f for f in sorted(os.listdir(clips_dir)) if os.path.isdir(os.path.join(clips_dir, f))]:
                    print("Evaluating {} .....".format(sub))
                    clip = pipe.plan_clip(sub, train_dir, dain_dir, pose_dir, save_dir)
                    if pipe.native:
                        pipe.run_native(clip)
                    else:
                        pipe.run_reference(clip)
                    clip = None
                written = pipe.drain()
            if metrics:
                self.metrics, self.metrics_report = pipe.report(save_dir)
            if panels:
                pipe.assemble_panels(save_dir, panel_fps)
            if video:
                pipe.assemble_video(save_dir, video_fps)
            return written
        finally:
            del pipe                 # the units' tensor views of the shared blocks die with it ...
            _shm_trim()              # ... so the surplus blocks can be unmapped


class _Clip:
    """What this rank renders of one clip, and where every frame's pieces are while the clip is in the pipeline."""

    def __init__(self, names, dain_list, image_list, pose_list, gtlist, sample_rate, keys, segs, units, sub="", measure=False,
                 mask_list=None):
        self.sub = sub                      # the clip's directory name
        self.measure = measure              # metrics: every generated frame is measured against gtlist[i]
        self.mask_list = mask_list          # metrics: mask file of every frame index, or None
        self.records = {}                   # metrics: frame index -> {i, file, DAIN_PSNR, DAIN_SSIM, OURS_PSNR, OURS_SSIM}
        self.meas = {}                      # metrics: unit -> (GT frames [Tc*B,3,H,W], masks [Tc*B,H,W] or None) on the device
        self.names = names                  # output file of every frame index
        self.dain_list, self.image_list, self.pose_list, self.gtlist = dain_list, image_list, pose_list, gtlist
        self.sample_rate = sample_rate
        self.keys = keys                    # this rank's key frames (they pass through, evaluator.py:240-244)
        self.segs = segs                    # this rank's segments [(key, [frame indices])]
        self.units = units                  # native path: [(group, [segment indices], c0, c1)] - a unit is a time chunk of a group
        # unit -> {"blk": the shared block (worker processes) or None, "table": its block_layout, "views": the sections of
        # staging_spec, page-locked; the decoders fill them in place}
        self.staged = {}
        self.slot = {}                      # frame index -> (unit, t, b): where its DAIN frame goes
        self.loads = {}                     # frame index -> future of (dain | None, key frame | None, pose or rasteriser tables)
        self.futs = {}                      # frame index -> future of its file name, or (unit future, position in the unit)
        self.opened = 0                     # units whose staging block and decode tasks exist
        self.prev_of = {}                   # group -> last fused frames [B,3,H,W] on its lane
        # resize_on="gpu": (w0, h0) at which the DAIN / GT frames are staged for the GPU resize; None: resized on the host
        self.src_dain = self.src_gt = None
        # panels: the sheets' folder; GT frames are staged for the Ground Truth pane whenever a gt_dir is given (want_gt: staged,
        # measured or not); the key frames of a first chunk belong to its unit (key_slot: key frame index -> (unit, b)), whose
        # block has their DAIN frames in its `key` section; key_of: group -> its key frames [B,3,H,W] on the device (the Ground
        # Truth pane without a gt_dir); pan: unit -> what upload() prepared for the unit's sheets
        self.panel_dir = None
        self.want_gt = measure
        self.key_slot, self.key_of, self.pan = {}, {}, {}
        self.sheet_futs = []                # futures of sheet files that ride in no unit's sink
        # background="mci": key frame index -> its uint8 HWC bytes as decoded and resized (filled by the decode tasks);
        # group -> (left keys, right keys uint8 [B,H,W,3], field int16 [B,Hb,Wb,2]) on the device, made in the group's first
        # chunk and kept for its later chunks beside prev_of (output_size="keyframes": + the left and right keys' own pixels uint8
        # [B,h0,w0,3], else None, None); both are released at the end of run_native / run_reference
        self.key_u8, self.mci_of = {}, {}
        # video: the folder of the frames' .jpg files; out_names: what drain() reports for every frame index - the PNG, or under
        # frames="none" the .jpg
        self.video_dir = None
        self.out_names = names
        # output_size="source" / "keyframes": (w0, h0) of the clip's files, the uniform size of its DAIN frames / of its key frame
        # files (under "keyframes" src_of's staged frames are rib_scaled_frames' backgrounds); key_src: key frame index ->
        # future of its uint8 HWC pixels at that size (the key file's own, resized only if its size differs); src_of: unit ->
        # (the staged DAIN frames uint8 [Tc,B,h0,w0,3], a first chunk's key frames uint8 [B,h0,w0,3] or None) on the device
        self.out_size = None
        self.key_src, self.src_of = {}, {}

    def sheet_names(self, i, png):
        """(jpg, png or None) of frame i's sheet."""
        base = os.path.join(self.panel_dir, "%04d" % i)
        return base + ".jpg", (base + ".png" if png else None)

    def video_name(self, i):
        return os.path.join(self.video_dir, "%04d.jpg" % i)

    def ref_image(self, i):
        """evaluator.py:209-212: the "gt" image of frame i is gtlist[i] when a gt_dir is given, else the key frame of its
        segment; the keypoints go through A.Resize together with THAT image (:219), i.e. they scale by its size."""
        return self.gtlist[i] if self.gtlist is not None else self.image_list[i // self.sample_rate]

    def unit_frames(self, ui):
        _, members, c0, c1 = self.units[ui]
        return [self.segs[si][1][t] for t in range(c0, c1) for si in members]      # (t, b) order


class _FolderPipeline:
    """One evaluate_from_folder call as explicit stages over units (a unit = `chunk` time steps of a group of up to B segments):

        plan_clip   directory listing -> this rank's key frames, segments, groups and units
        decode      open_units / submit_load: staging block per unit, one decode task per frame (threads or worker processes)
        upload      DAIN frames + label rasterisation + ToTensor/Normalize (resize_on="gpu": + the cubic resize) on the upload stream
        render      the unit's batched chain, the quantiser and ONE device-to-host copy on the lane's stream
        sink        when the copy has landed: PNG encodes, blocks back to the free lists

    Windows: decode runs DECODE_AHEAD units ahead of the unit being enqueued; at most MAX_UNITS_IN_FLIGHT units (of any clip)
    are enqueued but not yet written - a unit holds its label maps and frames on the device and a shared output block on the
    host until its files exist, and the GPU renders faster than PNGs get written.  Every stage can be driven on its own
    (tests/test_driver.py)."""

    def __init__(self, ev, model, rank, world, gt_dir, metrics=False, mask_dir=None, pose_mask=False,
                 panels=False, panel_frames=False, panel_quality=90, panel_encode="host", background="dain", mci_levels=3,
                 video=False, video_quality=90, video_frames=False, write_png=True, key_poses=None, mci_border="clamp", mci_precision="full",
                 output_size="model", png_gpu=False, mci_person="keep", mci_sampler="bilinear", mci_detail="model", mci_motion="linear"):
        # composite.py: the frames' files at the clip's own size - the DAIN frames' ("source") or, under background="mci", the key
        # frame files' ("keyframes": keysize; the backgrounds are then rib_scaled_frames', everything after them is "source"'s code)
        self.source = output_size in ("source", "keyframes")
        self.keysize = output_size == "keyframes"
        self.mci, self.mci_levels = background == "mci", mci_levels      # (levels: background.mci_field_host's, from mci_range)
        self.mci_border = mci_border        # background.py's border
        self.mci_half = mci_precision == "half"      # background.py's precision: the field is refined once per group, in half pixels
        self.mci_exclude = mci_person == "exclude"   # background.py's "person": the key frames' human masks keep the person out
        self.mci_sampler = mci_sampler               # background.py's sampler: "cubic" = sample_cubic / rib_cubic_* for every background sample
        self.mci_detail = mci_detail == "keyframes"  # background.py's "detail": the field refined at the key frames' size (output_size="keyframes" only)
        self.mci_quad = mci_motion == "quadratic"    # background.py's "motion": the neighbouring segments' fields give every block an acceleration
        # poses="keyframes": (motion model, key-pose folder, upsample rate, take the linear clip, also write the json folders)
        self.key_poses = key_poses
        # video: the frames' JPEG files (video.py); write_png False (frames="none"): they are the only files of a frame
        self.video, self.video_quality, self.video_frames, self.write_png = video, video_quality, video_frames, write_png
        # png_on="gpu": the frames' PNG files come from rib_png on the lane's stream (png.py); stage_png: the raw frames go home
        # for the PNG workers
        self.png_gpu = png_gpu
        self.stage_png = write_png and not png_gpu
        self.ev, self.model, self.rank, self.world, self.gt_dir = ev, model, rank, world, gt_dir
        self.metrics, self.mask_dir, self.pose_mask = metrics, mask_dir, pose_mask
        self.panels, self.panel_frames, self.panel_quality = panels, panel_frames, panel_quality
        self.native = hasattr(model, "chain") and hasattr(model, "quantise")
        if self.native and metrics and not hasattr(model, "quality"):
            raise RuntimeError("metrics=True: this model has no GPU quality kernel (rib_quality)")
        if self.native and pose_mask and not hasattr(model, "human_mask"):
            raise RuntimeError("pose_mask=True: this model has no GPU mask kernel (rib_human_mask)")
        if ev.resize_on == "gpu" and not (self.native and hasattr(model, "resize_u8")):
            raise RuntimeError("resize_on='gpu': this model has no GPU resize kernel (rib_resize_cubic)")
        if self.native and panels and not hasattr(model, "panel"):
            raise RuntimeError("panels=True: this model has no GPU sheet kernel (rib_panel)")
        if self.native and self.mci and not hasattr(model, "mci_frames"):
            raise RuntimeError("background='mci': this model has no GPU interpolation kernels (rib_mci_field / rib_mci_frames)")
        if self.native and self.mci_exclude and not (hasattr(model, "mci_frames_masked") and hasattr(model, "human_mask")):
            raise RuntimeError("mci_person='exclude': this model has no GPU kernels for it (rib_masked_field / rib_masked_frames / rib_human_mask)")
        if self.native and self.mci_half and not hasattr(model, "mci_refine"):
            raise RuntimeError("mci_precision='half': this model has no GPU refinement kernel (rib_halfpel_refine)")
        self.jpeg_gpu = panels and panel_encode == "gpu"     # the sheets' JPEG files are jpeg_encode_host's bytes (rib_jpeg on the native path)
        if self.native and self.jpeg_gpu and not hasattr(model, "jpeg_into"):
            raise RuntimeError("panel_encode='gpu': this model has no GPU JPEG kernels (rib_jpeg)")
        if self.native and video and not hasattr(model, "jpeg_f32_into"):
            raise RuntimeError("video=True: this model has no GPU JPEG kernels for float frames (rib_jpeg_float)")
        if self.keysize and self.native and not hasattr(model, "mci_frames_scaled"):
            raise RuntimeError("output_size='keyframes': this model has no GPU kernel for the key frames' size (rib_scaled_frames)")
        if self.mci_detail and self.native and not hasattr(model, "mci_detail_field"):
            raise RuntimeError("mci_detail='keyframes': this model has no GPU kernel for the full-size field (rib_detail_field)")
        if self.mci_quad and self.native and not (hasattr(model, "mci_accel_field") and hasattr(model, "mci_frames_accel")):
            raise RuntimeError("mci_motion='quadratic': this model has no GPU kernels for it (rib_accel_field / rib_accel_frames)")
        if self.source and self.native:
            if ev.resize_on != "gpu" and not self.keysize:
                raise ValueError("output_size='source' needs resize_on='gpu' on the native path: the background frames' source-size "
                                 "bytes are on the device only there (Evaluator(resize_on='gpu'), inference.py --resize-on gpu)")
            if not hasattr(model, "composite"):
                raise RuntimeError("output_size='source': this model has no GPU composite kernel (rib_composite)")
            if video and not hasattr(model, "jpeg_into"):
                raise RuntimeError("output_size='source' with video=True: this model has no GPU JPEG kernels (rib_jpeg)")
        self.gpu_labels = self.native and ev.label_fn is None and hasattr(model, "rasterise")
        per_slot = (1.0 + (1.0 if (metrics or (panels and gt_dir is not None)) else 0.0) + (1.0 / 3 if mask_dir is not None else 0.0))
        if self.mci_quad:                    # a first chunk stages four key frames per member where the budget's frame per slot holds `chunk`
            per_slot += max(0.0, float(len(MCI_KEY_ROLES)) / max(1, ev.chunk) - 1.0)
        if panels:                           # a unit's download block also carries its sheets (six panes and the borders per frame)
            sh, sw = _panel.layout(ev.height, ev.width)["sheet"]
            if not self.jpeg_gpu or panel_frames:                # (under panel_encode="gpu" only the lossless copies need the raw sheets)
                per_slot += 2.0 * sh * sw / (ev.height * ev.width)
            self.sheet_hw = (sh, sw)
            self.titles = _panel.title_bitmap(ev.width)
            self.titles_dev = None           # ... on the device, uploaded once (native path)
        self.per_slot = per_slot
        self.procs = _process_pool(ev.io_threads) if (self.native and ev.io_mode == "process" and ev._shm_fits(per_slot)) else None
        self.pool, self.finishers = ev._pool, ev._finishers
        self.level = ev.png_compress_level
        self.tm = {"load": 0.0, "rasterise": 0.0, "generate": 0.0, "save": 0.0, "frames": 0, "peak_units_in_flight": 0}
        if metrics:
            self.tm["metrics"] = 0.0             # launch thread: enqueueing the measurements (native) or measuring (reference), + the report
        self.t_wall = time.perf_counter()
        self.unit = 0                        # running index of independent units over all clips (the round-robin deal)
        self.inflight = collections.deque()  # sink futures of the units enqueued but not yet written (call-wide window)
        self.clips = []
        self.up = None                       # the upload stream
        self._sizes = {}

    # ---- helpers --------------------------------------------------------------------------------------------------------
    def peaks_of(self, pose):
        """A decoded frame's pose -> its [19, 2] peak table: the rasteriser tables carry it; (landmarks, conf) go through peak_table."""
        if self.gpu_labels:
            return pose[1]
        return rasterise.peak_table(pose[0], pose[1], self.ev.height, self.ev.width, self.ev.skeleton_thres)

    def image_size(self, path):              # header only; the keypoints scale with THIS image
        if path not in self._sizes:
            from PIL import Image
            with Image.open(path) as im:
                self._sizes[path] = im.size
        return self._sizes[path]

    def save_q(self, q, name):               # uint8 HWC -> file, here or in a worker process
        if self.procs is not None:
            return self.procs.submit(io_worker.save_png, q, name, self.level).result(timeout=IO_TIMEOUT_S)
        return io_worker.save_png(q, name, self.level)

    @staticmethod
    def host_u8(x):                          # utils/utils.py:129-142 on the host: the uint8 HWC array of a frame's PNG
        a = np.transpose(x[0].cpu().float().numpy(), (1, 2, 0)) * np.array([0.5] * 3) + np.array([0.5] * 3)
        return (np.clip(a, 0, 1) * 255.0).astype(np.uint8)

    def save_host(self, x, name):
        return self.save_q(self.host_u8(x), name)

    def save_frame_host(self, clip, i, x):
        """Frame i's files from its float tensor x [1,3,H,W] on the host (key frames; every frame of the reference path): the
        PNG unless frames="none", and under video=True - on the reference path: the native path encodes every frame on the
        GPU - the .jpg of the same uint8 array."""
        return self.save_u8(clip, i, self.host_u8(x))

    def save_u8(self, clip, i, u8):
        """Frame i's files from the uint8 HWC array its PNG holds (save_frame_host; output_size="source": the arrays below)."""
        if self.video and not self.native:
            _video.save_frame_host(u8, clip.video_name(i), self.video_quality)
        return self.save_q(u8, clip.names[i]) if self.write_png else clip.video_name(i)

    def key_source_u8(self, clip, i):
        """output_size="source": key frame i's file as its PNG shows it - the file's own pixels, uint8 HWC, resized
        (resize.resize_cubic_u8, on the host as key frames are) only if its size is not the clip's (w0, h0)."""
        w0, h0 = clip.out_size
        u8 = io_worker.decode_u8(clip.ref_image(i))
        if (u8.shape[1], u8.shape[0]) != (w0, h0):
            u8 = _resize.resize_cubic_u8(u8, w0, h0)
        return np.array(u8)                      # (a writable copy: PIL's array is not, and the staging views copy from it)

    def save_source_host(self, clip, i, img, mask):
        """output_size="source" behind the reference's protocol: frame i's files from the model's predicted image [1,3,H,W] and
        blend mask [1,1,H,W] and the DAIN file decoded once more at its own size (composite.composite_host)."""
        bg = io_worker.decode_u8(clip.dain_list[i])
        if (bg.shape[1], bg.shape[0]) != tuple(clip.out_size):
            raise ValueError("%s is %dx%d, the clip's output size is %dx%d" % ((clip.dain_list[i], bg.shape[1], bg.shape[0]) + tuple(clip.out_size)))
        u8 = _composite.composite_host(img.detach().cpu().float().numpy(), mask.detach().cpu().float().numpy(), bg[None])[0]
        return self.save_u8(clip, i, u8)

    def save_keysize_host(self, clip, i, img, mask, bg):
        """output_size="keyframes" behind the reference's protocol: frame i's files from the model's predicted image and blend mask
        and bg uint8 [h0,w0,3], its frame of background.mci_frames_scaled_host (composite.composite_host)."""
        u8 = _composite.composite_host(img.detach().cpu().float().numpy(), mask.detach().cpu().float().numpy(), bg[None])[0]
        return self.save_u8(clip, i, u8)

    # ---- stage 0: plan ---------------------------------------------------------------------------------------------------
    def interpolate_poses(self, sub, n_key, save_dir):
        """poses="keyframes": stage 1 for one clip -> (the [19, 3] keypoint array of every frame, the sample rate).  Every rank
        runs it for itself (about a millisecond of GPU work and no communication), so the frames cannot depend on the number
        of ranks; the array comes home in one copy and its rows take the place of the json paths."""
        motion, key_pose_dir, rate, linear, save = self.key_poses
        json_dir = os.path.join(key_pose_dir, sub)
        n_pose = len(_list(json_dir, ("json",)))
        if n_pose != n_key:
            raise ValueError("poses='keyframes': clip %s has %d key-pose files and %d key frames; each key frame needs its pose"
                             % (sub, n_pose, n_key))
        folders = None
        if save and self.rank == 0:
            root = os.path.dirname(os.path.abspath(save_dir))
            folders = {"pred_dir": os.path.join(root, "Predict_motion", sub), "linear_dir": os.path.join(root, "Linear_motion", sub)}
        pred, lin = motion.interpolate_clip(json_dir, rate, save_dir=folders)
        rows = lin if linear else pred
        if len(rows) != (n_key - 1) * rate + 1:
            raise ValueError("poses='keyframes': clip %s: stage 1 returned %d frames for %d key frames at rate %d" % (sub, len(rows), n_key, rate))
        return [np.ascontiguousarray(rows[i]) for i in range(len(rows))], rate

    def plan_clip(self, sub, train_dir, dain_dir, pose_dir, save_dir):
        ev = self.ev
        frames_dir = os.path.join(save_dir, sub)
        if self.write_png:
            os.makedirs(frames_dir, exist_ok=True)
        image_list = _list(os.path.join(train_dir, sub), ("jpg", "png"))
        dain_list = None if self.mci else _list(os.path.join(dain_dir, sub), ("jpg", "png"))
        if self.mci and len(image_list) < 2:
            raise ValueError("background='mci': clip %s has %d key frame(s); a segment needs two" % (sub, len(image_list)))
        if self.key_poses is not None:
            pose_list, sample_rate = self.interpolate_poses(sub, len(image_list), save_dir)
        else:
            pose_list = _list(os.path.join(pose_dir, sub), ("json",))
            sample_rate = sample_rate_of(len(pose_list), len(image_list))
        seq_len = (len(image_list) - 1) * sample_rate + 1
        out_size = None
        if self.source and not self.keysize:      # one size per clip, read from the headers before anything of the clip is written
            kinds = sorted({tuple(self.image_size(p)) for p in dain_list[:seq_len]})
            if len(kinds) != 1:
                raise ValueError("output_size='source': clip %s: the DAIN frames have mixed sizes (%s); the clip's files need one size"
                                 % (sub, ", ".join("%dx%d" % k for k in kinds[:4])))
            out_size = kinds[0]
        if self.mci and self.key_poses is not None:      # the stems stage 1's own command gives its files
            names = [os.path.join(frames_dir, "%06d.png" % i) for i in range(seq_len)]
        elif self.mci:                       # no DAIN list to name the frames after: the pose file's stem
            def stem(path):
                base = os.path.splitext(os.path.basename(path))[0]
                return base[:-len("_keypoints")] if base.endswith("_keypoints") else base
            names = [os.path.join(frames_dir, stem(pose_list[i]) + ".png") for i in range(seq_len)]
        else:
            names = [os.path.join(frames_dir, os.path.basename(dain_list[i]))[:-4] + ".png" for i in range(seq_len)]
        gtlist = _list(os.path.join(self.gt_dir, sub), ("jpg", "png")) if self.gt_dir is not None else None
        mask_list = None
        if self.metrics:
            if len(gtlist) < seq_len:
                raise ValueError("metrics: %s has %d ground-truth frames, the clip has %d" % (os.path.join(self.gt_dir, sub), len(gtlist), seq_len))
            if self.mask_dir is not None:
                mask_list = _list(os.path.join(self.mask_dir, sub), ("jpg", "png"))
                if len(mask_list) < seq_len:
                    raise ValueError("metrics: %s has %d masks, the clip has %d frames" % (os.path.join(self.mask_dir, sub), len(mask_list), seq_len))
        if self.keysize:                     # the size of the key frame files (every rank reads all of the clip's: one answer)
            key_files = [gtlist[i] if gtlist is not None else image_list[i // sample_rate] for i in range(0, seq_len, sample_rate)]
            kinds = sorted({tuple(self.image_size(p)) for p in key_files})
            if len(kinds) != 1:
                raise ValueError("output_size='keyframes': clip %s: the key frames have mixed sizes (%s); the clip's files need one size"
                                 % (sub, ", ".join("%dx%d" % k for k in kinds[:4])))
            out_size = kinds[0]
            _background.scaled_factors((ev.height, ev.width), (out_size[1], out_size[0]), "output_size='keyframes': clip %s" % sub)
        keys, segs = split_segments(seq_len, sample_rate)
        # this rank's share: a segment is one unit of the deal and brings the key frame it starts from along (that frame is
        # decoded for the chain anyway); a key frame without a segment (the last one) is a unit of its own
        first_of = {k: si for si, (k, _) in enumerate(segs)}
        my_segs, my_keys = [], []
        for k in keys:
            if self.unit % self.world == self.rank:
                my_keys.append(k)
                if k in first_of:
                    my_segs.append(first_of[k])
            self.unit += 1
        segs = [segs[si] for si in my_segs]
        # native path: segments of equal length are grouped into batches, every (group, time chunk) is one unit of the pipeline
        # with one pinned staging buffer that the decode workers fill in place
        units = []
        if self.native:
            B_ = ev.batch or ev.default_batch()
            for gi, members in enumerate(ev.group_segments(segs, B_)):
                T = len(segs[members[0]][1])
                step = ev.chunk if ev.chunk > 0 else T
                for c0 in range(0, T, step):
                    units.append((gi, members, c0, min(T, c0 + step)))
        clip = _Clip(names, dain_list, image_list, pose_list, gtlist, sample_rate, my_keys, segs, units, sub=sub,
                     measure=self.metrics, mask_list=mask_list)
        clip.out_size = out_size
        if self.video:
            clip.video_dir = _video.video_dir(save_dir, sub)
            os.makedirs(clip.video_dir, exist_ok=True)
            if not self.write_png:
                clip.out_names = [clip.video_name(i) for i in range(seq_len)]
        if self.panels:
            if gtlist is not None and len(gtlist) < seq_len:
                raise ValueError("panels: %s has %d ground-truth frames, the clip has %d" % (os.path.join(self.gt_dir, sub), len(gtlist), seq_len))
            clip.want_gt = gtlist is not None
            clip.panel_dir = _panel.sheet_dir(save_dir, sub)
            os.makedirs(clip.panel_dir, exist_ok=True)
        if ev.resize_on == "gpu" and units:
            # the header sizes of the frames this rank stages (cached: the keypoint scaling reads the same headers)
            staged = [i for _, frames in segs for i in frames]
            slots = max((c1 - c0) * len(members) for _, members, c0, c1 in units)
            src, why = plan_gpu_resize([self.image_size(dain_list[i]) for i in staged],
                                       [self.image_size(gtlist[i]) for i in staged] if self.metrics else None,
                                       (ev.width, ev.height), slots, mask=mask_list is not None,
                                       shm_free=_shm_free_bytes() if self.procs is not None else None,
                                       out_slot_bytes=max(0, out_size[0] * out_size[1] - ev.width * ev.height) * 3
                                       if (self.source and self.stage_png) else 0)
            clip.src_dain, clip.src_gt = src["DAIN"], src["GT"]
            if self.source and clip.src_dain is None:      # never a silent change of the output's size
                raise ValueError("output_size='source': clip %s: the DAIN list falls back to the host resize, so its source-size bytes "
                                 "would not be on the device: %s" % (sub, "; ".join(r_ for n_, r_ in why if n_ == "DAIN") or "no reason given"))
            for name, reason in why:
                print("resize_on='gpu': clip {}: the {} list falls back to the host resize: {}".format(sub, name, reason))
        if self.keysize and units and self.procs is not None:
            # the blocks at the key frames' size count, as "source" counts its own: a first chunk stages both key frames of every
            # segment (with video the left ones once more), the download block a frame per slot - beside the model-size staging
            # that _shm_fits counted.  A clip that does not fit is an error, never a silent change of size
            w0, h0 = out_size
            slots = max((c1 - c0) * len(members) for _, members, c0, c1 in units)
            width = max(len(members) for _, members, _, _ in units)
            need = shm_windows_bytes(int(slots * ev.height * ev.width * 3 * self.per_slot) + ((len(MCI_KEY_ROLES) if self.mci_quad else 2) + bool(self.video or self.png_gpu)) * width * w0 * h0 * 3
                                     + (slots * w0 * h0 * 3 if self.stage_png else 0))
            free = _shm_free_bytes()
            if need > free:
                raise ValueError("output_size='keyframes': clip %s: the staging windows at %dx%d need %.0f MB of shared memory, %.0f MB "
                                 "are free (a smaller chunk or batch needs less; io_mode='thread' needs none)"
                                 % (sub, w0, h0, need / 1e6, free / 1e6))
        self.clips.append(clip)
        return clip

    # ---- stage 1: decode -------------------------------------------------------------------------------------------------
    def decode_here(self, clip, i):
        """Pre-load of frame i on a pool thread (evaluator.py:205-235)."""
        ev = self.ev
        staged_raw = i in clip.slot and clip.src_dain is not None
        if self.source and not self.native and not self.mci:
            # output_size="source" is held to the native path's files, and that path exists under resize_on="gpu" only: a model behind
            # the reference's protocol reads the very floats that chain reads (the device's normalisation, as under background="mci")
            dain = torch.from_numpy(_background.normalised_upload(ev._decode_resized_u8(clip.dain_list[i])[0]))
        else:
            dain = None if (staged_raw or self.mci) else (ev.load_image_u8 if self.native else ev.load_image)(clip.dain_list[i])[0]
        if i in clip.slot:
            ui, t, b = clip.slot[i]
            views = clip.staged[ui]["views"]
            if staged_raw:                       # resize_on="gpu": at the file's own size, straight into the slot
                io_worker.decode_raw_into(views["dain"][t, b].numpy(), 0, clip.dain_list[i], clip.src_dain)
            elif not self.mci:                   # (background="mci": nothing to stage, the background frames are made on the GPU)
                views["dain"][t, b].copy_(dain)
            dain = None
            if clip.want_gt and clip.src_gt is not None:
                io_worker.decode_raw_into(views["gt"][t, b].numpy(), 0, clip.gtlist[i], clip.src_gt)
            elif clip.want_gt:                   # the GT frame (and mask) of a measured frame, through the same resize
                views["gt"][t, b].copy_(ev.load_image_u8(clip.gtlist[i])[0])
            if clip.measure and clip.mask_list is not None:
                views["mask"][t, b].copy_(torch.from_numpy(io_worker.load_mask_u8(clip.mask_list[i], ev.width, ev.height)))
        elif i in clip.key_slot and not self.mci:        # panels: a key frame's DAIN frame, for its sheet
            ui, b = clip.key_slot[i]
            clip.staged[ui]["views"]["key"][b].copy_(dain)
            dain = None
        ref_img = clip.ref_image(i)
        if self.mci and i % clip.sample_rate == 0:       # one decode: the uint8 bytes for the interpolation, normalised for the chain
            u8 = ev._decode_resized_u8(ref_img)[0]
            clip.key_u8[i] = torch.from_numpy(u8.copy())
            gt = torch.from_numpy(io_worker.normalised_chw(u8))
        else:
            gt = ev.load_image(ref_img)[0] if i % clip.sample_rate == 0 else None
        pose = ev.load_pose(clip.pose_list[i], self.image_size(ref_img))
        if self.gpu_labels:                      # host tables of the GPU rasteriser, built here in the worker
            pose = rasterise.frame_tables(pose[0], pose[1], ev.height, ev.width, ev.skeleton_thres, ev.foot_thres)
        return dain, gt, pose

    @staticmethod
    def slot_offset(clip, ui, section, b, t=0):
        """Byte offset, in unit ui's staging block, of slot (t, b) of a section - `key` has one slot per segment, the others
        one per time step and segment - or -1 where the block has no such section.  The one place that computes a slot's offset."""
        table, (_, members, c0, c1) = clip.staged[ui]["table"], clip.units[ui]
        if section not in table:
            return -1
        off, nbytes = table[section]
        slots = len(members) * (1 if section in ("key", "key_src") else c1 - c0)
        return off + (t * len(members) + b) * (nbytes // slots)

    def decode_in_worker(self, clip, i):
        """The same pre-load in a worker process; its result is unpacked (arrays wrapped as tensors) by the pool's result thread
        as soon as it arrives.  The worker decodes the DAIN frame straight into the unit's shared staging block."""
        from concurrent.futures import Future
        ev = self.ev
        name, off, gt_off, mask_off, raw = "", -1, -1, -1, (None, None)
        if i in clip.slot:                       # a section the unit's block does not have (slot_offset: -1) is not decoded
            ui, t, b = clip.slot[i]
            name, raw = clip.staged[ui]["blk"].name, (clip.src_dain, clip.src_gt)
            off, gt_off, mask_off = (self.slot_offset(clip, ui, section, b, t) for section in ("dain", "gt", "mask"))
        elif i in clip.key_slot:                 # panels: a key frame's DAIN frame goes to the key section, at the model size
            ui, b = clip.key_slot[i]
            name, off = clip.staged[ui]["blk"].name, self.slot_offset(clip, ui, "key", b)
        src = self.procs.submit(io_worker.load_frame_shm, name, off, None if self.mci else clip.dain_list[i], clip.ref_image(i), clip.pose_list[i],
                                i % clip.sample_rate == 0, self.gpu_labels, ev.width, ev.height, ev.resize, ev.skeleton_thres, ev.foot_thres,
                                gt_offset=gt_off, mask_path=clip.mask_list[i] if mask_off >= 0 else None, mask_offset=mask_off,
                                dain_raw=raw[0], gt_raw=raw[1])
        out = Future()

        def unpack(f):
            try:
                _, gt, pose = f.result()
                if self.mci and gt is not None:          # the key frame's uint8 bytes as decoded and resized, for the interpolation
                    clip.key_u8[i] = torch.from_numpy(gt)
                out.set_result((None, torch.from_numpy(io_worker.normalised_chw(gt)) if gt is not None else None, pose))
            except BaseException as e:              # noqa: BLE001 (handed to whoever waits for the frame)
                out.set_exception(e)
        src.add_done_callback(unpack)
        return out

    def submit_load(self, clip, i):
        if i in clip.loads:
            return
        clip.loads[i] = self.decode_in_worker(clip, i) if self.procs is not None else self.pool.submit(self.decode_here, clip, i)
        # key frames pass through (evaluator.py:240-244); native path under frames="none": their only file comes from the GPU
        # (output_size="keyframes": every key frame a segment of this rank touches - the right ones too - for rib_scaled_frames)
        if self.source and (i in clip.keys or (self.keysize and i % clip.sample_rate == 0)) and i not in clip.key_src:
            clip.key_src[i] = self.pool.submit(self.key_source_u8, clip, i)
        if i in clip.keys and i not in clip.futs and (self.stage_png or not self.native):
            if self.source:                      # the key file's own pixels (the future is held here: the clip's table is cleared early)
                ks = clip.key_src[i]
                clip.futs[i] = self.finishers.submit(lambda: self.save_u8(clip, i, ks.result(timeout=IO_TIMEOUT_S)))
            else:
                clip.futs[i] = self.finishers.submit(
                    lambda: self.save_frame_host(clip, i, clip.loads[i].result(timeout=IO_TIMEOUT_S)[1].unsqueeze(0)))

    def open_units(self, clip, upto):
        """Staging block, slots and decode tasks of the units up to index `upto`: the launch thread keeps DECODE_AHEAD units open
        beyond the one it is enqueueing, so that host memory (page-locked, shared) does not grow with the clip."""
        ev = self.ev
        while clip.opened <= min(upto, len(clip.units) - 1):
            ui = clip.opened
            _, members, c0, c1 = clip.units[ui]
            # one block per unit; a later chunk under background="mci" may stage nothing at all and still gets its byte
            spec = staging_spec(c1 - c0, len(members), (ev.height, ev.width), clip.src_dain, clip.src_gt, want_gt=clip.want_gt,
                                masks=clip.mask_list is not None, keys=self.panels and c0 == 0, mci=self.mci, mci_keys=c0 == 0,
                                src_keys=clip.out_size if (self.source and (self.video or self.png_gpu) and c0 == 0) else None,
                                mci_keys_src=clip.out_size if (self.keysize and c0 == 0) else None, mci_quad=self.mci_quad)
            table, total = block_layout(spec_bytes(spec))
            # worker processes: shared with them and page-locked (size classes of 1 MB: the block may be larger than the unit)
            blk = _shm_get(max(1, total)) if self.procs is not None else None
            flat = blk.t if blk is not None else torch.empty(max(1, total), dtype=torch.uint8, pin_memory=True)
            clip.staged[ui] = {"blk": blk, "table": table, "views": section_views(flat, spec, table)}
            for b, si in enumerate(members):
                if self.panels and c0 == 0:     # (background="mci": the block has no `key` section, a key frame is its own background)
                    clip.key_slot[clip.segs[si][0]] = (ui, b)
                for t in range(c0, c1):
                    clip.slot[clip.segs[si][1][t]] = (ui, t - c0, b)
            # decode in the order the launch thread will ask for the frames: the unit's key frames first
            for i in ([clip.segs[si][0] for si in members] if c0 == 0 else []) + clip.unit_frames(ui):
                self.submit_load(clip, i)
            if self.mci and c0 == 0:            # the right key frames: decoded (not written: that is their own unit's rank)
                for si in members:              # (mci_motion="quadratic": and the key frames of the segments before and after)
                    for i in mci_key_frames(clip.segs[si][0], clip.sample_rate, len(clip.names), self.mci_quad)[0][1:]:
                        self.submit_load(clip, i)
            clip.opened += 1

    # ---- stage 2: upload -------------------------------------------------------------------------------------------------
    def wait_decoded(self, clip, ui):
        """Blocks until the unit's frames (and, for a first chunk, its key frames) are decoded: (poses or tables, key frames)."""
        _, members, c0, _ = clip.units[ui]
        got = [clip.loads[i].result(timeout=IO_TIMEOUT_S) for i in clip.unit_frames(ui)]
        gt = torch.stack([clip.loads[clip.segs[si][0]].result(timeout=IO_TIMEOUT_S)[1] for si in members]) if c0 == 0 else None
        return [g_[2] for g_ in got], gt

    def upload(self, clip, ui, g, st, poses, gt):
        """Enqueues - on the upload stream, which is idle, so that nothing waits behind the previous unit of the lane - the label
        rasterisation, the upload of the staged DAIN frames with ToTensor + Normalize(0.5, 0.5) on the GPU
        (HSM_auto_dataset.py:73-75) and the key frames; the lane joins through the returned event.  -> (lab, dn, gtd, ready)."""
        ev = self.ev
        gi, members, c0, c1 = clip.units[ui]
        Tc, Bc = c1 - c0, len(members)
        views = clip.staged[ui]["views"]        # page-locked, of the unit's block: they go back to the pool with it (sink)
        if self.up is None:
            self.up = torch.cuda.Stream(device=self.model.device)
        # panels: the label maps of a first chunk's key frames (their sheets' Skeleton pane) are drawn in the unit's own call
        key_poses = [clip.loads[clip.segs[si][0]].result(timeout=IO_TIMEOUT_S)[2] for si in members] if (self.panels and c0 == 0) else []
        with torch.cuda.stream(self.up):
            if self.gpu_labels:
                lab = rasterise.rasterise_tables(g, poses + key_poses, ev.height, ev.width, ev.gauss_sigma)
            else:
                lab = ev.make_labels(g if hasattr(g, "rasterise") else self.model, poses + key_poses)
            lab = lab.to(g.device)
            klab = lab[Tc * Bc:] if key_poses else None
            lab = lab[:Tc * Bc].reshape(Tc, Bc, *lab.shape[1:])              # [Tc,B,22,H,W]
            staged = dnu8 = None
            if self.mci:
                if c0 == 0:                    # once per group: the key frames' bytes go up and the field is made
                    ks = [clip.segs[si][0] for si in members]
                    # per member the key frames of the sections (mci_key_frames: left, right; quadratic: and the ones around them)
                    keyf = [mci_key_frames(k, clip.sample_rate, len(clip.names), self.mci_quad) for k in ks]
                    nk = len(keyf[0][0])
                    for idx, _ in keyf:
                        for i in idx[1:]:
                            clip.loads[i].result(timeout=IO_TIMEOUT_S)
                    for b, (idx, _) in enumerate(keyf):
                        for r, i in enumerate(idx):
                            views["mci_keys"][r, b].copy_(clip.key_u8[i])
                    kab = views["mci_keys"].to(g.device, non_blocking=True)
                    # the segments whose fields are made, as (left, right) rows of the sections: the group's own and, quadratic, the
                    # ones before and after it - all in ONE batched call per entry (a segment's field does not depend on the batch)
                    sides = ((0, 1), (2, 0), (1, 3)) if self.mci_quad else ((0, 1),)
                    pair = (lambda x: (torch.cat([x[i] for i, _ in sides]), torch.cat([x[j] for _, j in sides]))) if self.mci_quad else (lambda x: (x[0], x[1]))
                    pa, pb = pair(kab)
                    qab = (None, None)
                    if self.mci_exclude:        # the human masks of the key frames' poses (rib_human_mask), 1 = excluded; no person: all zero
                        pk = np.stack([self.peaks_of(clip.loads[idx[r]].result(timeout=IO_TIMEOUT_S)[2]) for r in range(nk) for idx, _ in keyf])
                        qab = (g.human_mask(pk, ev.height, ev.width) > 0).to(torch.uint8).view(nk, len(ks), ev.height, ev.width)
                        field = g.mci_field_masked(pa, pb, *pair(qab), self.mci_levels, border=self.mci_border)
                    else:
                        field = g.mci_field(pa, pb, self.mci_levels, border=self.mci_border)
                    if self.mci_half:           # one more launch behind the field's, on the same stream; in place
                        field = g.mci_refine(pa, pb, field, border=self.mci_border, out=field)
                    kab0 = (None, None)
                    if self.keysize:            # the key files' own pixels, beside the field: what the unit's backgrounds are sampled from
                        for b, (idx, _) in enumerate(keyf):
                            for r, i in enumerate(idx):
                                views["mci_keys_src"][r, b].copy_(torch.from_numpy(clip.key_src[i].result(timeout=IO_TIMEOUT_S)))
                        kab0 = views["mci_keys_src"].to(g.device, non_blocking=True)
                    field0 = None
                    if self.mci_detail:         # the field refined at the key frames' own size, once per group, behind the field (two launches)
                        field0 = g.mci_detail_field(*pair(kab0), field, (ev.height, ev.width), border=self.mci_border,
                                                    precision="half" if self.mci_half else "full")
                    accel = accel0 = None
                    if self.mci_quad:           # own | before | after -> the block acceleration (two launches), the own fields stay
                        n, present = len(ks), [has for _, has in keyf]
                        accel = g.mci_accel_field(field[n:2 * n], field[:n], field[2 * n:], precision="half" if self.mci_half else "full", present=present)
                        if self.mci_detail:
                            accel0 = g.mci_accel_field(field0[n:2 * n], field0[:n], field0[2 * n:], present=present)
                            field0 = field0[:n]
                        field = field[:n]
                    clip.mci_of[gi] = (kab[0], kab[1], field, kab0[0], kab0[1], qab[0], qab[1], field0, accel, accel0)
                ka, kb, field, ka0, kb0, qa, qb, field0, accel, accel0 = clip.mci_of[gi]
                if self.mci_quad:              # ONE launch, as below: every sample moved by the acceleration's correction
                    dn = g.mci_frames_accel(ka, kb, field, accel, clip.sample_rate, k_first=c0 + 1, count=Tc, normalised="both" if self.panels else True,
                                            border=self.mci_border, precision="half" if self.mci_half else "full", sampler=self.mci_sampler,
                                            masks=(qa, qb) if self.mci_exclude else None)
                elif self.mci_exclude:
                    dn = g.mci_frames_masked(ka, kb, qa, qb, field, clip.sample_rate, k_first=c0 + 1, count=Tc,
                                             normalised="both" if self.panels else True, border=self.mci_border, sampler=self.mci_sampler)
                else:
                    dn = g.mci_frames(ka, kb, field, clip.sample_rate, k_first=c0 + 1, count=Tc, normalised="both" if self.panels else True,
                                      border=self.mci_border, precision="half" if self.mci_half else "full", sampler=self.mci_sampler)
                if self.panels:
                    dn, dnu8 = dn
                if self.mci_detail and self.mci_quad:      # ONE launch at the key frames' size: the full-size field and its acceleration
                    staged = g.mci_frames_accel(ka0, kb0, field0, accel0, clip.sample_rate, k_first=c0 + 1, count=Tc, normalised=False,
                                                border=self.mci_border, sampler=self.mci_sampler)
                elif self.mci_detail:          # ONE launch, the existing frame entry at the key frames' size with the full-size field (whole pixels)
                    staged = g.mci_frames(ka0, kb0, field0, clip.sample_rate, k_first=c0 + 1, count=Tc, normalised=False, border=self.mci_border,
                                          sampler=self.mci_sampler)
                elif self.keysize:             # ONE launch: the unit's backgrounds uint8 [Tc,B,h0,w0,3], "source"'s staged frames
                    staged = g.mci_frames_scaled(ka0, kb0, field, (ev.height, ev.width), clip.sample_rate, k_first=c0 + 1, count=Tc,
                                                 border=self.mci_border, precision="half" if self.mci_half else "full", sampler=self.mci_sampler)
            else:
                staged = views["dain"].to(g.device, non_blocking=True)
                if clip.src_dain is not None:      # resize_on="gpu": resize + ToTensor + Normalize in one kernel (rib_resize_cubic)
                    dn = g.resize_u8(staged.flatten(0, 1), ev.width, ev.height, normalised=True).view(Tc, Bc, 3, ev.height, ev.width)
                else:
                    dn = staged.permute(0, 1, 4, 2, 3).to(torch.float32)
                    dn = ((dn / 255.0 - 0.5) / 0.5).contiguous()                      # [Tc,B,3,H,W]
            if self.source:                    # the staged frames stay as they are for the composite; a first chunk's key frames
                ksrc = None                    # go up at the output size for their video files
                if views.get("key_src") is not None:
                    for b, si in enumerate(members):
                        views["key_src"][b].copy_(torch.from_numpy(clip.key_src[clip.segs[si][0]].result(timeout=IO_TIMEOUT_S)))
                    ksrc = views["key_src"].to(g.device, non_blocking=True)
                clip.src_of[ui] = (staged, ksrc)
            gtd = gt.to(g.device) if gt is not None else None
            gtf = staged_gt = None
            if clip.want_gt:
                staged_gt = views["gt"].to(g.device, non_blocking=True)
            if clip.measure:                   # the GT frames normalised as the DAIN frames are
                if clip.src_gt is not None:
                    gtf = g.resize_u8(staged_gt.flatten(0, 1), ev.width, ev.height, normalised=True)
                else:
                    gtf = staged_gt.permute(0, 1, 4, 2, 3).to(torch.float32)
                    gtf = ((gtf / 255.0 - 0.5) / 0.5).reshape(Tc * Bc, 3, ev.height, ev.width).contiguous()
            if clip.measure:                   # masks 0/1 -> float
                mk = (views["mask"].to(g.device, non_blocking=True).to(torch.float32).reshape(Tc * Bc, ev.height, ev.width)
                      if views["mask"] is not None else None)
                if self.pose_mask:             # drawn here from the unit's own peaks (rib_human_mask): no file, no staging
                    mk = g.human_mask(np.stack([self.peaks_of(p_) for p_ in poses]), ev.height, ev.width)
                clip.meas[ui] = (gtf, mk)
            if self.panels:
                if self.titles_dev is None:
                    self.titles_dev = torch.from_numpy(self.titles).to(g.device)
                if c0 == 0:
                    clip.key_of[gi] = gtd
                # the DAIN / Ground Truth panes show the bytes tensor2images makes of the HOST's tensors (normalise_exact says why the
                # tensors the generator and the metrics read - normalised with torch's reciprocal - are not shown); frames staged at
                # their source size (resize_on="gpu") come out of the resize kernel as uint8 first
                def shown(u8, src):
                    if src is not None:
                        u8 = g.resize_u8(u8.flatten(0, 1), ev.width, ev.height)
                    return normalise_exact(u8).reshape(Tc * Bc, 3, ev.height, ev.width)
                dnp = normalise_exact(dnu8.flatten(0, 1)) if self.mci else shown(staged, clip.src_dain)
                if self.mci:                   # a key frame's background is frame k = 0 of its segment: the key frame itself
                    kdn = normalise_exact(clip.mci_of[gi][0]) if key_poses else None
                else:
                    kdn = normalise_exact(views["key"].to(g.device, non_blocking=True)) if key_poses else None
                if staged_gt is not None:
                    gtp = shown(staged_gt, clip.src_gt)
                else:                          # no gt_dir: the Ground Truth pane is the segment's left key frame (evaluator.py:209-212)
                    keys = clip.key_of[gi]
                    gtp = keys.unsqueeze(0).expand(Tc, *keys.shape).reshape(Tc * Bc, *keys.shape[1:])
                clip.pan[ui] = (gtp, klab, kdn, clip.key_of[gi], dnp)
            ready = torch.cuda.Event()
            ready.record(self.up)
        for t_ in (lab, dn, gtd) + tuple(clip.meas.get(ui, ())) + tuple(clip.pan.get(ui, ())) + tuple(clip.src_of.get(ui, ())):
            if t_ is not None:
                t_.record_stream(st)
        return lab, dn, gtd, ready

    # ---- stage 3: render -------------------------------------------------------------------------------------------------
    def render(self, clip, ui, g, st, lab, dn, gtd, ready):
        """The unit's chain (evaluator.py:240-244,252: a segment starts from its key frame; inside it prev <- fused frame), then
        everything the unit sends home - in ONE device buffer of named sections (block_layout; DESIGN 4e has the table),
        filled by the quantiser, rib_quality, rib_panel and the two JPEG encoders, each under its option - and ONE asynchronous
        copy into page-locked host memory, all on the lane's stream.  Returns the record the sink reads: the same keys for
        every unit, None where the unit has no such section."""
        gi, members, c0, _ = clip.units[ui]
        with torch.cuda.stream(st):
            st.wait_event(ready)
            imgs, masks, fz = g.chain(gtd if c0 == 0 else clip.prev_of[gi], lab, dn, want_all=self.panels or self.source)      # fz [Tc,B,3,H,W]
            clip.prev_of[gi] = fz[-1]
            t0 = time.perf_counter()
            n, H, W = fz.shape[0] * fz.shape[1], fz.shape[3], fz.shape[4]
            frames = fz.reshape(n, 3, H, W)
            gtp, klab, kdn, keys, dnp = clip.pan.pop(ui) if self.panels else (None,) * 5
            nk = kdn.shape[0] if kdn is not None else 0          # panels: a first chunk also draws the key frames it starts from
            SH, SW = self.sheet_hw if self.panels else (0, 0)
            home = self.panels and (not self.jpeg_gpu or self.panel_frames)     # the raw sheets travel home
            # output_size="source": the frames' files are at the clip's (w0, h0); the chain, the metrics and the sheets stay at H x W
            W0, H0 = clip.out_size if self.source else (W, H)
            spec = (("frames", torch.uint8, (n, H0, W0, 3), self.stage_png),
                    ("qual", torch.float32, (4, n), clip.measure),       # OURS PSNR, OURS SSIM, DAIN PSNR, DAIN SSIM
                    ("sheet_len", torch.int32, (n + nk,), self.jpeg_gpu),        # (jpeg_gpu implies panels)
                    ("video_len", torch.int32, (self.video_count(clip, ui),), self.video),
                    ("png_len", torch.int32, (self.file_count(clip, ui),), self.png_gpu),
                    ("sheets", torch.uint8, (n + nk, SH, SW, 3), home))
            table, total = block_layout(spec_bytes(spec))
            assert total, "a unit sends something home: frames, metrics, sheets or a video"
            buf = torch.empty(total, dtype=torch.uint8, device=g.device)
            dev = section_views(buf, spec, table)
            keep = [fz, lab, dn, gtd, buf]
            shown = None
            if self.source:                      # one launch: quantise, enlarge and blend over the staged frames' own pixels
                staged, ksrc = clip.src_of.pop(ui)
                shown = dev["frames"] if self.stage_png else torch.empty((n, H0, W0, 3), dtype=torch.uint8, device=g.device)
                g.composite(imgs.reshape(n, 3, H, W), masks.reshape(n, 1, H, W), staged.flatten(0, 1), out=shown)
                keep += [imgs, masks, staged, ksrc, shown]
            elif self.stage_png:
                g.quantise(frames, out=dev["frames"])
            if clip.measure:
                gtf, mk = clip.meas.pop(ui)
                g.quality(frames, gtf, mk, out=dev["qual"][0:2])
                g.quality(dn.reshape(n, 3, H, W), gtf, mk, out=dev["qual"][2:4])
                keep += [gtf, mk]
            jpeg = vid = pngs = None
            if self.png_gpu:                     # the frames' PNG files from the bytes the workers would have been handed
                u8 = shown if self.source else g.quantise(frames)
                if c0 != 0:
                    ku8 = None
                elif self.source:
                    ku8 = ksrc.contiguous()
                else:                            # a key frame passes through: the bytes of its tensor (save_frame_host)
                    ku8 = g.quantise(gtd.to(torch.float32).contiguous())
                pngs = self.encode_png(g, u8, ku8, dev["png_len"])
                keep += [u8, ku8, pngs]
            if self.panels:                      # under panel_encode="gpu" without panel_frames the sheets stay on the device
                sheets = dev["sheets"] if home else torch.empty((n + nk, SH, SW, 3), dtype=torch.uint8, device=g.device)
                g.panel(imgs.reshape(n, 3, H, W), masks.reshape(n, 1, H, W), frames, dnp, gtp, lab.reshape(n, *lab.shape[2:]),
                        titles=self.titles_dev, out=sheets[:n])
                if nk:
                    g.panel(None, None, None, kdn, keys, klab, titles=self.titles_dev, out=sheets[n:])
                keep += [imgs, masks, gtp, klab, kdn, keys, dnp]
                if self.jpeg_gpu:
                    jpeg = self.encode_jpeg(g, sheets, dev["sheet_len"])
                    keep += [sheets, jpeg]
            if self.video and self.source:
                vid = self.encode_video_u8(g, shown, ksrc, dev["video_len"])
                keep += [vid]
            elif self.video:
                vid = self.encode_video(clip, ui, g, frames, gtd, dev["video_len"])
                keep += [vid]
            out_blk = _shm_get(total) if self.procs is not None else None       # shared with the encode workers, page-locked
            flat = out_blk.t[:total] if out_blk is not None else torch.empty(total, dtype=torch.uint8, pin_memory=True)
            flat.copy_(buf, non_blocking=True)
            done = torch.cuda.Event()
            done.record(st)
            if self.panels:
                self.tm["panels"] = self.tm.get("panels", 0.0) + time.perf_counter() - t0
            elif clip.measure:
                self.tm["metrics"] += time.perf_counter() - t0
        host = section_views(flat, spec, table)
        # the files of the two encoders stay on the device until the sink knows their lengths: (files, cap, lengths on the host)
        # frames_off / sheets_off: where the file workers find those two sections in the shared block
        return {"done": done, "out_blk": out_blk, "keep": tuple(keep),
                "frames": host["frames"], "qual": host["qual"], "sheets": host["sheets"],
                "frames_off": table["frames"][0] if "frames" in table else None, "frame_hw": (H0, W0),
                "sheets_off": table["sheets"][0] if "sheets" in table else None,
                "jpeg": jpeg + (host["sheet_len"],) if jpeg else None, "video": vid + (host["video_len"],) if vid else None,
                "png": pngs + (host["png_len"],) if pngs else None,
                "sheet_frames": clip.unit_frames(ui) + ([clip.segs[si][0] for si in members] if nk else []) if self.panels else None}

    @staticmethod
    def file_count(clip, ui):
        """video / png_on="gpu": the files a unit encodes per kind - its frames and, in a first chunk, the key frames it starts from."""
        _, members, c0, c1 = clip.units[ui]
        return (c1 - c0) * len(members) + (len(members) if c0 == 0 else 0)

    def video_count(self, clip, ui):
        """video: the files a unit encodes (file_count; else 0)."""
        return self.file_count(clip, ui) if self.video else 0

    def video_frames_of(self, clip, ui):
        """The frame indices of a unit's video files, in the order encode_video writes them."""
        _, members, c0, _ = clip.units[ui]
        return clip.unit_frames(ui) + ([clip.segs[si][0] for si in members] if c0 == 0 else [])

    def encode_video(self, clip, ui, g, frames, gtd, lengths):
        """video=True, on the lane's stream: rib_jpeg_float of the unit's fused frames float [n,3,H,W] and - in a first chunk - of
        the key frames gtd [B,3,H,W] it starts from, one call each -> (files, cap): file j at files[j * cap:], its size in
        lengths[j] (int32 on the device, a view of the unit's download buffer).  cap is the proven bound (rib_jpeg_max_bytes)."""
        n, _, H, W = frames.shape
        nk = lengths.numel() - n
        cap = g.jpeg_max_bytes(H, W)
        files = torch.empty((n + nk) * cap, dtype=torch.uint8, device=g.device)
        g.jpeg_f32_into(frames.to(torch.float32).contiguous(), files[:n * cap], lengths[:n], self.video_quality, cap)
        if nk:
            g.jpeg_f32_into(gtd.to(torch.float32).contiguous(), files[n * cap:], lengths[n:], self.video_quality, cap)
        return files, cap

    def encode_video_u8(self, g, shown, ksrc, lengths):
        """video=True under output_size="source", on the lane's stream: rib_jpeg of the unit's frames uint8 [n,H0,W0,3] - the
        very bytes of their PNGs - and, in a first chunk, of the key frames ksrc uint8 [B,H0,W0,3] it starts from, one call
        each -> (files, cap) as encode_video's."""
        n, H0, W0, _ = shown.shape
        nk = lengths.numel() - n
        cap = g.jpeg_max_bytes(H0, W0)
        files = torch.empty((n + nk) * cap, dtype=torch.uint8, device=g.device)
        g.jpeg_into(shown, files[:n * cap], lengths[:n], self.video_quality, cap)
        if nk:
            g.jpeg_into(ksrc.contiguous(), files[n * cap:], lengths[n:], self.video_quality, cap)
        return files, cap

    def encode_png(self, g, u8, ku8, lengths):
        """png_on="gpu", on the lane's stream: rib_png of the unit's frames uint8 [n,H0,W0,3] and - in a first chunk - of the key
        frames ku8 uint8 [B,H0,W0,3] it starts from (else None), one call each -> (files, cap) as encode_video's.  cap is the
        proven bound (rib_png_max_bytes): no frame can be refused."""
        n, H0, W0, _ = u8.shape
        nk = lengths.numel() - n
        cap = g.png_max_bytes(H0, W0)
        files = torch.empty((n + nk) * cap, dtype=torch.uint8, device=g.device)
        g.png_into(u8, files[:n * cap], lengths[:n], cap)
        if nk:
            g.png_into(ku8, files[n * cap:], lengths[n:], cap)
        return files, cap

    def save_sheets(self, clip, frames, sheets, out_blk=None, off=0):
        """Submits the encodes of the sheets of `frames` (uint8 [n, SH, SW, 3] on the host; out_blk: the shared block they lie
        in, from byte `off`) -> futures.  panel_encode="gpu": only the lossless copies are left to encode (panel_frames)."""
        SH, SW = self.sheet_hw
        names = [clip.sheet_names(i, self.panel_frames) for i in frames]
        if self.jpeg_gpu:
            names = [(None, png) for _, png in names]
        if out_blk is not None:
            return [self.procs.submit(io_worker.save_sheet_shm, out_blk.name, off + j * SH * SW * 3, SH, SW,
                                      *names[j], self.panel_quality) for j in range(len(frames))]
        sn = sheets.numpy()
        return [self.pool.submit(io_worker.save_sheet, sn[j], *names[j], self.panel_quality) for j in range(len(frames))]

    def encode_jpeg(self, g, sheets, lengths):
        """panel_encode="gpu", on the lane's stream: rib_jpeg of the sheets uint8 [n, SH, SW, 3] on the device -> (files, cap):
        frame j's file at files[j * cap:], its size in lengths[j] (int32 [n] on the device, a view of the unit's download
        buffer).  cap is the proven bound of a file (rib_jpeg_max_bytes): no frame can be refused."""
        SH, SW = self.sheet_hw
        cap = g.jpeg_max_bytes(SH, SW)
        files = torch.empty(sheets.shape[0] * cap, dtype=torch.uint8, device=g.device)
        g.jpeg_into(sheets, files, lengths, self.panel_quality, cap)
        return files, cap

    # the three kinds of files that are encoded on the GPU: (the option and entry a refusal names, what a file is, its name)
    FILE_KINDS = {"sheet": ("panel_encode='gpu': rib_jpeg", "sheet", lambda clip, i: clip.sheet_names(i, False)[0]),
                  "video": ("video=True: rib_jpeg_float", "frame", lambda clip, i: clip.video_name(i)),
                  "png": ("png_on='gpu': rib_png", "frame", lambda clip, i: clip.names[i])}

    def fetch_files(self, clip, frames, enc, kind="sheet"):
        """On a finisher thread once the unit's copy is home: enc = (files, cap, lengths on the host) of one encoder - exactly the
        files' bytes come home and are written by this thread: no worker, no PIL.  kind (FILE_KINDS): "sheet", the sheets'
        %04d.jpg (panel_encode="gpu"); "video", the frames' own .jpg in the clip's video folder (encode_video); "png", the
        frames' PNG files under their own names (png_on="gpu", encode_png).  A zero length raises, naming the frame."""
        files, cap, lengths = enc
        what, noun, name_of = self.FILE_KINDS[kind]
        sizes = [int(v) for v in lengths.tolist()]
        if not all(0 < v <= cap for v in sizes):
            bad = [name_of(clip, i) for i, v in zip(frames, sizes) if not 0 < v <= cap]
            raise RuntimeError("%s refused a %s: %s (lengths %s, cap %d)" % (what, noun, ", ".join(bad), sizes, cap))
        with torch.cuda.stream(self.copy_stream(files.device)):
            host = [files[j * cap:j * cap + sizes[j]].cpu() for j in range(len(frames))]     # each returns when its bytes are home
        return [_panel.save_jpeg(host[j].numpy().tobytes(), name_of(clip, i)) for j, i in enumerate(frames)]

    def copy_stream(self, device):
        """The stream of the finishers' exact-size file copies (one per device): the lane's work they read is complete."""
        streams = self.__dict__.setdefault("_copy_streams", {})
        if device not in streams:
            streams[device] = torch.cuda.Stream(device)
        return streams[device]

    def loose_keys(self, clip, g, st):
        """panels / video: the sheets and the video files of this rank's key frames that start no segment of its own (a clip's
        last key frame; every key frame of a rank that renders nothing): a small unit of their own - labels, one rib_panel
        launch in key-frame mode, the two encoders - whose download is laid out and copied as a unit's is (render)."""
        ev = self.ev
        started = {k for k, _ in clip.segs}
        loose = [k for k in clip.keys if k not in started]
        if not loose:
            return
        got = [clip.loads[k].result(timeout=IO_TIMEOUT_S) for k in loose]
        n, (SH, SW) = len(loose), self.sheet_hw if self.panels else (0, 0)
        home = self.panels and (not self.jpeg_gpu or self.panel_frames)     # the raw sheets travel home
        spec = (("sheet_len", torch.int32, (n,), self.jpeg_gpu), ("video_len", torch.int32, (n,), self.video),
                ("png_len", torch.int32, (n,), self.png_gpu), ("sheets", torch.uint8, (n, SH, SW, 3), home))
        table, total = block_layout(spec_bytes(spec))
        if self.panels and self.mci:             # a key frame's background is the key frame itself (frame k = 0 of the interpolation)
            dains = [clip.key_u8[k] for k in loose]
        elif self.panels:
            dains = list(self.pool.map(lambda k: ev.load_image_u8(clip.dain_list[k])[0], loose))
        with torch.cuda.stream(st):
            buf = torch.empty(total, dtype=torch.uint8, device=g.device)
            dev = section_views(buf, spec, table)
            keys = torch.stack([g_[1] for g_ in got]).to(g.device, torch.float32).contiguous()
            keep, jpeg, vid, pngs = [buf, keys], None, None, None
            if self.panels:
                poses = [g_[2] for g_ in got]
                if self.gpu_labels:
                    klab = rasterise.rasterise_tables(g, poses, ev.height, ev.width, ev.gauss_sigma)
                else:
                    klab = ev.make_labels(g if hasattr(g, "rasterise") else self.model, poses).to(g.device)
                if self.titles_dev is None:
                    self.titles_dev = torch.from_numpy(self.titles).to(g.device)
                kdn = normalise_exact(torch.stack(dains).to(g.device))
                sheets = dev["sheets"] if home else torch.empty((n, SH, SW, 3), dtype=torch.uint8, device=g.device)
                g.panel(None, None, None, kdn, keys, klab, titles=self.titles_dev, out=sheets)
                keep += [sheets, kdn, klab]
                if self.jpeg_gpu:                # the files of both encoders stay on the device until their lengths are home
                    jpeg = self.encode_jpeg(g, sheets, dev["sheet_len"])
            ku8 = None
            if (self.video or self.png_gpu) and self.source:       # the key files' own pixels at the clip's output size
                ku8 = torch.from_numpy(np.stack([clip.key_src[k].result(timeout=IO_TIMEOUT_S) for k in loose])).to(g.device)
                keep += [ku8]
            if self.png_gpu:
                pngs = self.encode_png(g, ku8 if self.source else g.quantise(keys), None, dev["png_len"])
                keep += [pngs]
            if self.video and self.source:
                cap = g.jpeg_max_bytes(*ku8.shape[1:3])
                vid = (torch.empty(n * cap, dtype=torch.uint8, device=g.device), cap)
                g.jpeg_into(ku8, vid[0], dev["video_len"], self.video_quality, cap)
            elif self.video:
                cap = g.jpeg_max_bytes(*keys.shape[2:])
                vid = (torch.empty(n * cap, dtype=torch.uint8, device=g.device), cap)
                g.jpeg_f32_into(keys, vid[0], dev["video_len"], self.video_quality, cap)
            out_blk = _shm_get(total) if self.procs is not None else None
            flat = out_blk.t[:total] if out_blk is not None else torch.empty(total, dtype=torch.uint8, pin_memory=True)
            flat.copy_(buf, non_blocking=True)
            done = torch.cuda.Event()
            done.record(st)
        host = section_views(flat, spec, table)

        def finish(keep=keep):
            done.synchronize()
            if jpeg is not None:
                self.fetch_files(clip, loose, jpeg + (host["sheet_len"],))
            names = self.fetch_files(clip, loose, vid + (host["video_len"],), "video") if vid is not None else None
            if pngs is not None:                 # (png_on="gpu" implies frames="png": the names reported are the PNGs')
                names = self.fetch_files(clip, loose, pngs + (host["png_len"],), "png")
            if home:
                for f in self.save_sheets(clip, loose, host["sheets"], out_blk, table["sheets"][0]):
                    f.result(timeout=IO_TIMEOUT_S)
            if out_blk is not None:
                _shm_put(out_blk)
            return names                         # frames="none": the .jpg names of the loose key frames, in order; png_on="gpu": the PNGs'
        fut = self.finishers.submit(finish)
        clip.sheet_futs.append(fut)
        if (self.video and not self.write_png) or self.png_gpu:
            for j, k in enumerate(loose):
                clip.futs[k] = (fut, j)

    # ---- stage 4: sink ---------------------------------------------------------------------------------------------------
    def sink(self, clip, ui, r, t_loaded, t_enq):
        """Runs on a finisher thread: waits for the unit's copy, hands the staging block back, fans the PNG encodes out and
        returns the written names in unit order.  `r["keep"]` keeps the unit's device tensors alive until then."""
        ev = self.ev
        out_frames = clip.unit_frames(ui)
        r["done"].synchronize()                 # the chain, the quantiser and the download are done: so is the upload
        # per unit: inputs decoded, launches enqueued, results on the host, files written (seconds since the call began)
        mark = [round(t_loaded, 4), round(t_enq, 4), round(time.perf_counter() - self.t_wall, 4)]
        self.tm.setdefault("timeline", []).append(mark)
        if r["qual"] is not None:               # the unit's per-frame metrics rode in the same copy
            self.record(clip, out_frames, r["qual"].numpy().astype(np.float64))
        in_blk = clip.staged.pop(ui)["blk"]     # the record holds every view of the block: they go before the block does
        if in_blk is not None:
            _shm_put(in_blk)
        out_blk = r["out_blk"]
        # panels: the JPEG (and PNG) encodes of the unit's sheets fan out beside the PNG encodes of its frames
        sheet_fs = self.save_sheets(clip, r["sheet_frames"], r["sheets"], out_blk, r["sheets_off"]) if r["sheets"] is not None else []
        fs = []
        if self.stage_png and out_blk is not None:      # the workers read frame j in the block, from the section's offset on
            (fh, fw), off = r["frame_hw"], r["frames_off"]
            fsz = fh * fw * 3
            fs = [self.procs.submit(io_worker.save_png_shm, out_blk.name, off + j * fsz, fh, fw, clip.names[out_frames[j]], self.level)
                  for j in range(len(out_frames))]
        elif self.stage_png:
            qn = r["frames"].numpy()
            fs = [self.pool.submit(self.save_q, qn[j], clip.names[out_frames[j]]) for j in range(len(out_frames))]
        # panel_encode="gpu" / video: the files' bytes come home now that their lengths have, while the workers encode the PNGs
        if r["jpeg"] is not None:
            self.fetch_files(clip, r["sheet_frames"], r["jpeg"])
        vres = self.fetch_files(clip, self.video_frames_of(clip, ui), r["video"], "video") if r["video"] is not None else None
        pres = self.fetch_files(clip, self.video_frames_of(clip, ui), r["png"], "png") if r["png"] is not None else None
        res = [f.result(timeout=IO_TIMEOUT_S) for f in fs]
        for f in sheet_fs:
            f.result(timeout=IO_TIMEOUT_S)
        r["frames"] = r["qual"] = r["sheets"] = r["jpeg"] = r["video"] = r["png"] = None       # (the views of the block go before the block does)
        if out_blk is not None:
            _shm_put(out_blk)
        r["keep"] = None
        mark.append(round(time.perf_counter() - self.t_wall, 4))
        if self.png_gpu:
            return pres                         # the PNG names, the unit's frames and then its key frames
        return res if self.write_png else vres      # frames="none": the .jpg names, the unit's frames and then its key frames

    # ---- drivers ---------------------------------------------------------------------------------------------------------
    def run_native(self, clip):
        tm = self.tm
        ngroups = len({u[0] for u in clip.units})
        lanes = self.ev._lanes(self.model, ngroups)
        for ui, (gi, members, c0, c1) in enumerate(clip.units):
            self.open_units(clip, ui + DECODE_AHEAD)
            while len(self.inflight) >= MAX_UNITS_IN_FLIGHT:      # back-pressure (call-wide window): wait for the oldest unit's files
                self.inflight.popleft().result(timeout=IO_TIMEOUT_S)
            g, st = lanes[gi % len(lanes)] if lanes else (self.model, torch.cuda.current_stream(self.model.device))
            t0 = time.perf_counter()
            poses, gt = self.wait_decoded(clip, ui)
            t1 = time.perf_counter()
            lab, dn, gtd, ready = self.upload(clip, ui, g, st, poses, gt)
            t2 = time.perf_counter()
            r = self.render(clip, ui, g, st, lab, dn, gtd, ready)
            t3 = time.perf_counter()
            tm["load"] += t1 - t0
            tm["rasterise"] += t2 - t1
            tm["generate"] += t3 - t2
            seg_fut = self.finishers.submit(self.sink, clip, ui, r, t1 - self.t_wall, t3 - self.t_wall)
            self.inflight.append(seg_fut)
            tm["peak_units_in_flight"] = max(tm["peak_units_in_flight"], len(self.inflight))
            for j, i in enumerate(clip.unit_frames(ui) if self.stage_png else self.video_frames_of(clip, ui)):
                clip.futs[i] = (seg_fut, j)
        for k in clip.keys:
            self.submit_load(clip, k)
        if self.panels or self.video or self.png_gpu:
            self.loose_keys(clip, *(lanes[0] if lanes else (self.model, torch.cuda.current_stream(self.model.device))))
        tm["units"] = tm.get("units", 0) + len(clip.units)
        tm["frames"] += len(clip.futs)
        # background="mci": the groups' key frames and fields are only read by launches already enqueued on the upload stream,
        # where they were allocated: released with the clip (pipe.clips keeps the _Clip itself until drain)
        clip.mci_of.clear()
        clip.key_u8.clear()
        clip.key_src.clear()

    @property
    def sheet_saver(self):
        """The host encoder of a sheet on the reference path: PIL, or under panel_encode="gpu" the definition the GPU encoder
        is held to (panel.jpeg_encode_host) - the same files as the native path writes."""
        return io_worker.save_sheet_defined if self.jpeg_gpu else io_worker.save_sheet

    def quadratic_host(self, clip, k, ks):
        """mci_motion="quadratic" by the host definition, for the segment that starts at key frame k: the fields of the segment and of
        the ones before and after it (every setting as the linear path applies it), background.mci_accel_host, and frames ks by
        mci_frames_accel_host -> (uint8 [len(ks), H, W, 3] at the model size, the same at the key files' size under
        mci_detail="keyframes", else None)."""
        ev, s, B = self.ev, clip.sample_rate, _background
        idx, has = mci_key_frames(k, s, len(clip.names), True)
        pose = {i: clip.loads[i].result(timeout=IO_TIMEOUT_S)[2] for i in set(idx)}
        key = {i: clip.key_u8[i].numpy() for i in pose}
        msk = {i: rasterise.human_mask(self.peaks_of(p), ev.height, ev.width).astype(np.uint8) for i, p in pose.items()} if self.mci_exclude else {}
        src = {i: clip.key_src[i].result(timeout=IO_TIMEOUT_S) for i in pose} if self.mci_detail else {}
        prec = "half" if self.mci_half else "full"

        def fields(i, j):                        # of the segment between key frames i and j: (model size, key files' size or None)
            if self.mci_exclude:
                f = B.mci_field_masked_host(key[i], key[j], msk[i], msk[j], self.mci_levels, border=self.mci_border)
            else:
                f = B.mci_field_host(key[i], key[j], self.mci_levels, border=self.mci_border)
            if self.mci_half:
                f = B.mci_refine_host(key[i], key[j], f, border=self.mci_border)
            return f, B.mci_detail_field_host(src[i], src[j], f, (ev.height, ev.width), border=self.mci_border, precision=prec) if self.mci_detail else None
        own = fields(idx[0], idx[1])
        prev = fields(idx[2], idx[0]) if has[0] else (None, None)
        nxt = fields(idx[1], idx[3]) if has[1] else (None, None)
        masks = dict(ma=msk[idx[0]], mb=msk[idx[1]]) if self.mci_exclude else {}
        u8 = B.mci_frames_accel_host(key[idx[0]], key[idx[1]], own[0], B.mci_accel_host(prev[0], own[0], nxt[0], unit_shift=int(self.mci_half)), s, ks,
                                     border=self.mci_border, precision=prec, sampler=self.mci_sampler, **masks)
        if not self.mci_detail:
            return u8, None
        return u8, B.mci_frames_accel_host(src[idx[0]], src[idx[1]], own[1], B.mci_accel_host(prev[1], own[1], nxt[1]), s, ks, border=self.mci_border,
                                           sampler=self.mci_sampler)

    def run_reference(self, clip):
        """Any callable that only speaks the reference's protocol (img, mask = model(label, None, dain, prev)): frame by frame."""
        ev, tm, model = self.ev, self.tm, self.model
        # decoded, written by their own rank: the right key frames (quadratic: and those of the segments before and after)
        right = {i for k, _ in clip.segs for i in mci_key_frames(k, clip.sample_rate, len(clip.names), self.mci_quad)[0]} if self.mci else set()
        for i in sorted(set(clip.keys) | right | {i for _, frames in clip.segs for i in frames}):
            self.submit_load(clip, i)
        for k, frames in clip.segs:
            t0 = time.perf_counter()
            got = [clip.loads[i].result() for i in frames]
            gt = clip.loads[k].result()[1].unsqueeze(0)
            if self.mci:
                clip.loads[k + clip.sample_rate].result()
            t1 = time.perf_counter()
            tm["load"] += t1 - t0
            poses = [g[2] for g in got]
            if self.mci:                         # the host definition of the background frames (background.py)
                ka, kb = clip.key_u8[k].numpy(), clip.key_u8[k + clip.sample_rate].numpy()
                if self.mci_quad:                # three segments' fields, the acceleration, the frames: every setting in one place
                    u8, bg0 = self.quadratic_host(clip, k, [i - k for i in frames])
                elif self.mci_exclude:           # the host statement of the two key frames' human masks, 1 = excluded
                    qa, qb = (rasterise.human_mask(self.peaks_of(clip.loads[j].result()[2]), ev.height, ev.width).astype(np.uint8)
                              for j in (k, k + clip.sample_rate))
                    field = _background.mci_field_masked_host(ka, kb, qa, qb, self.mci_levels, border=self.mci_border)
                    u8 = _background.mci_frames_masked_host(ka, kb, qa, qb, field, clip.sample_rate, [i - k for i in frames], border=self.mci_border,
                                                            sampler=self.mci_sampler)
                else:
                    field = _background.mci_field_host(ka, kb, self.mci_levels, border=self.mci_border)
                    if self.mci_half:
                        field = _background.mci_refine_host(ka, kb, field, border=self.mci_border)
                    u8 = _background.mci_frames_host(ka, kb, field, clip.sample_rate, [i - k for i in frames], border=self.mci_border,
                                                     precision="half" if self.mci_half else "full", sampler=self.mci_sampler)
                # the floats the native chain reads (the device's normalisation, stated on the host); the sheets' DAIN pane
                # shows the host's normalisation, as the native path's does (normalise_exact)
                dn = torch.from_numpy(_background.normalised_upload(u8)).unsqueeze(1)
                dn_shown = torch.from_numpy(_background.normalised(u8)).unsqueeze(1)
                if self.mci_quad:
                    pass                         # (bg0 is quadratic_host's)
                elif self.mci_detail:            # the field refined at the key files' own size, then the existing frame definition there
                    ka0, kb0 = (clip.key_src[j].result(timeout=IO_TIMEOUT_S) for j in (k, k + clip.sample_rate))
                    field0 = _background.mci_detail_field_host(ka0, kb0, field, (ev.height, ev.width), border=self.mci_border,
                                                               precision="half" if self.mci_half else "full")
                    bg0 = _background.mci_frames_host(ka0, kb0, field0, clip.sample_rate, [i - k for i in frames], border=self.mci_border,
                                                      sampler=self.mci_sampler)
                elif self.keysize:               # the same field, the samples from the key files' own pixels: the files' backgrounds
                    bg0 = _background.mci_frames_scaled_host(clip.key_src[k].result(timeout=IO_TIMEOUT_S),
                                                             clip.key_src[k + clip.sample_rate].result(timeout=IO_TIMEOUT_S), field,
                                                             (ev.height, ev.width), clip.sample_rate, [i - k for i in frames],
                                                             border=self.mci_border, precision="half" if self.mci_half else "full",
                                                             sampler=self.mci_sampler)
            else:
                dn = dn_shown = torch.stack([g[0] for g in got]).unsqueeze(1)
            lab = ev.make_labels(model, poses).unsqueeze(1)
            t2 = time.perf_counter()
            prev, outs, shown = gt, [], []
            for t in range(len(frames)):
                img, mask = model(lab[t], None, dn[t], prev)
                prev = img * mask.repeat(1, 3, 1, 1) + dn[t].to(img.device) * (1 - mask.repeat(1, 3, 1, 1))
                outs.append(prev)
                shown.append((img, mask))
            tm["rasterise"] += t2 - t1
            tm["generate"] += time.perf_counter() - t2
            for t, i in enumerate(frames):
                if self.keysize:                 # composite_host of the frame's (img, mask) over its full-size interpolated background
                    clip.futs[i] = self.pool.submit(self.save_keysize_host, clip, i, *shown[t], bg0[t])
                elif self.source:                # composite_host of the frame's (img, mask) over the DAIN file's own pixels
                    clip.futs[i] = self.pool.submit(self.save_source_host, clip, i, *shown[t])
                else:
                    clip.futs[i] = self.pool.submit(self.save_frame_host, clip, i, outs[t])
            if self.panels:                      # the host statement of the sheet (panel.compose_host), a segment at a time
                def host(xs):
                    return torch.cat([x.detach().cpu().float() for x in xs]).numpy()
                gtp = [ev.load_image(clip.gtlist[i])[0].unsqueeze(0) for i in frames] if clip.gtlist is not None else [gt] * len(frames)
                sheets = _panel.compose_host(host([p_[0] for p_ in shown]), host([p_[1] for p_ in shown]), host(outs), host(list(dn_shown)),
                                             host(gtp), host(list(lab)), self.titles)
                for t, i in enumerate(frames):
                    clip.sheet_futs.append(self.pool.submit(self.sheet_saver, sheets[t], *clip.sheet_names(i, self.panel_frames), self.panel_quality))
            if clip.measure:                     # the torch statement of the metric (metrics.py), frame by frame
                t3 = time.perf_counter()
                vals = np.zeros((4, len(frames)))
                for t, i in enumerate(frames):
                    gt_i = ev.load_image(clip.gtlist[i])[0].unsqueeze(0)
                    mk = (torch.from_numpy(io_worker.load_mask_u8(clip.mask_list[i], ev.width, ev.height)).float().unsqueeze(0)
                          if clip.mask_list is not None else None)
                    if self.pose_mask:           # the host statement of the mask, from this frame's pose
                        mk = torch.from_numpy(rasterise.human_mask(self.peaks_of(poses[t]), ev.height, ev.width)).float().unsqueeze(0)
                    for row, x in ((0, outs[t]), (2, dn[t])):
                        p_, s_ = _metrics.psnr_ssim(x.detach().cpu().float(), gt_i, mk)
                        vals[row, t], vals[row + 1, t] = float(p_[0]), float(s_[0])
                self.record(clip, frames, vals)
                tm["metrics"] += time.perf_counter() - t3
        if self.panels:                          # the key frames' sheets: the key-frame rule
            for k in clip.keys:
                dain, key, pose = clip.loads[k].result()
                if self.mci:                     # frame k = 0 of the interpolation: the key frame itself
                    dain = key
                klab = ev.make_labels(model, [pose]).detach().cpu().float().numpy()
                sheet = _panel.compose_host(None, None, None, dain.unsqueeze(0).numpy(), key.unsqueeze(0).numpy(), klab, self.titles)[0]
                clip.sheet_futs.append(self.pool.submit(self.sheet_saver, sheet, *clip.sheet_names(k, self.panel_frames), self.panel_quality))
        tm["units"] = tm.get("units", 0)
        tm["frames"] += len(clip.futs)
        clip.key_u8.clear()
        clip.key_src.clear()

    # ---- metrics ---------------------------------------------------------------------------------------------------------
    @staticmethod
    def record(clip, frames, vals):
        """vals [4, len(frames)]: OURS PSNR, OURS SSIM, DAIN PSNR, DAIN SSIM of each frame -> clip.records."""
        for j, i in enumerate(frames):
            clip.records[i] = {"i": int(i), "file": os.path.basename(clip.names[i]),
                               "DAIN_PSNR": float(vals[2, j]), "DAIN_SSIM": float(vals[3, j]),
                               "OURS_PSNR": float(vals[0, j]), "OURS_SSIM": float(vals[1, j])}

    def report(self, save_dir):
        """After drain(): the per-frame records of every rank (all_gather_object under a process group; rank 0 writes
        <save_dir>/metrics.json) -> (records [{clip, i, file, 4 values}] in clip and frame order, the report dict)."""
        import json
        t0 = time.perf_counter()
        mine = [dict(r, clip=clip.sub) for clip in self.clips for _, r in sorted(clip.records.items())]
        rows = [mine]
        import torch.distributed as dist
        grouped = self.world > 1 and dist.is_available() and dist.is_initialized()
        if grouped:
            rows = [None] * dist.get_world_size()
            dist.all_gather_object(rows, mine)
        order = {c.sub: k for k, c in enumerate(self.clips)}
        recs = sorted((r for part in rows for r in part), key=lambda r: (order.get(r["clip"], len(order)), r["clip"], r["i"]))
        clips = {}
        for r in recs:
            clips.setdefault(r["clip"], []).append({k: v for k, v in r.items() if k != "clip"})
        rep = {"protocol": dict(_metrics.PROTOCOL,
                                measured_frames="every non-key frame (i % sample_rate != 0): its fused frame (OURS) and its DAIN "
                                                "frame (DAIN) against gt_dir's frame i; at sample_rate 2 the reference's rule "
                                                "(PGNR/models/evaluator.py:116)",
                                mask=("mask_dir/<clip>/ grayscale at the model size, value > 127 -> 1" if self.mask_dir is not None
                                      else (_metrics.POSE_MASK if self.pose_mask else None)),
                                clips_reported="every clip (the reference returns only the last clip's dict: it is overwritten per clip)"),
               "clips": {c: dict(_metrics.mean_record(pf), frames=len(pf), per_frame=pf) for c, pf in clips.items()},
               "overall": dict(_metrics.mean_record(recs), frames=len(recs))}
        if self.mci:                             # the DAIN_* values measure the interpolated background (the keys keep their names)
            rep["background"] = "mci"
        if self.rank == 0 or not grouped:
            name = "metrics.json" if (self.world == 1 or grouped) else "metrics_rank%d.json" % self.rank
            os.makedirs(save_dir, exist_ok=True)
            with open(os.path.join(save_dir, name), "w") as f:
                json.dump(rep, f, indent=1)
        self.tm["metrics"] = self.tm.get("metrics", 0.0) + time.perf_counter() - t0
        return recs, rep

    def assemble_panels(self, save_dir, fps):
        """After drain(): every rank's sheets are in <save_dir>/<clip>_panels/ - rank 0 (after a barrier, under a process group)
        makes <save_dir>/<clip>.avi of each clip's folder (panel.assemble).  Ranks dealt by hand (rank / world arguments without a
        process group) cannot know when the others are done: the caller assembles."""
        t0 = time.perf_counter()
        import torch.distributed as dist
        grouped = self.world > 1 and dist.is_available() and dist.is_initialized()
        if grouped:
            dist.barrier()
        if self.world == 1 or (grouped and self.rank == 0):
            for clip in self.clips:
                _panel.assemble(save_dir, clip.sub, fps, keep_frames=self.panel_frames)
        self.tm["panels"] = self.tm.get("panels", 0.0) + time.perf_counter() - t0

    def assemble_video(self, save_dir, fps):
        """After drain(): every rank's frame files are in <save_dir>/<clip>_video/ - rank 0 (after a barrier, under a process
        group) makes <save_dir>/<clip>_video.avi of each clip's folder (video.assemble).  Ranks dealt by hand cannot know when
        the others are done: the caller assembles."""
        t0 = time.perf_counter()
        import torch.distributed as dist
        grouped = self.world > 1 and dist.is_available() and dist.is_initialized()
        if grouped:
            dist.barrier()
        if self.world == 1 or (grouped and self.rank == 0):
            for clip in self.clips:
                _video.assemble(save_dir, clip.sub, fps, keep_frames=self.video_frames)
        self.tm["video"] = self.tm.get("video", 0.0) + time.perf_counter() - t0

    def drain(self):
        """Waits for every file of the call, in frame order as the reference writes them; returns the names this rank wrote."""
        written: List[str] = []
        t5 = time.perf_counter()
        for clip in self.clips:
            for i, name in enumerate(clip.out_names):
                if i not in clip.futs:
                    continue                                                       # another rank's frame
                f = clip.futs[i]
                res = f[0].result()[f[1]] if isinstance(f, tuple) else f.result()
                assert res == name
                written.append(name)
            for f in clip.sheet_futs:                                              # panels: sheets that rode in no unit's sink
                f.result()
        self.tm["save"] = time.perf_counter() - t5                                 # tail: encodes still running after the last enqueue
        self.tm["wall"] = time.perf_counter() - self.t_wall
        return written
