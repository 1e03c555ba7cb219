"""Drop-in host-side mirror of the reference ``Generator`` object protocol
(PGNR/models/generator.py:35-234 as used by PGNR/models/trainer.py:61,67 and
PGNR/models/evaluator.py:170,255):

    net_G = Generator(cfg.gen)            # same ctor argument
    net_G.load_state_dict(state_dict)     # same 372-tensor checkpoint, strict
    net_G.eval()
    img, mask = net_G(label, label_prev, img_fake, img_prev)

All compute happens in hand-written HIP kernels behind the C ABI of
include/rib.h; this class only validates arguments, owns the workspace tensor
and passes device pointers.  No CPU fallback exists: constructing a Generator
without a GPU or without the built library raises.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional

import numpy as np
import torch

from . import _native
from .config import GenSpec


def _ptr(t: Optional[torch.Tensor]):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


class Generator:
    def __init__(self, gen_cfg, device=None, use_tuning=True, compute_dtype="f32", products="f32"):
        """compute_dtype: 'f32' (exact-fp32 matrix cores; the reference's arithmetic), 'bf16' (bf16 storage and
        matrix-core operands, fp32 accumulate / statistics; BASELINE config 3) or 'f16' (the same 16-bit kernels
        with IEEE half elements: ~10x closer to fp32 than bf16 at the same speed).
        products (fp32 mode only, opt-in): 'f32' = exact-fp32 products everywhere (default); 'bf16x3' = the plain GEMMs of
        the frame form every product from six bf16 matrix-core products of three-way split operands (include/rib.h,
        rib_set_products): fp32-grade, not the reference's arithmetic."""
        if compute_dtype not in ("f32", "bf16", "f16"):
            raise ValueError("compute_dtype must be 'f32', 'bf16' or 'f16'")
        if products not in ("f32", "bf16x3"):
            raise ValueError("products must be 'f32' or 'bf16x3'")
        if products != "f32" and compute_dtype != "f32":
            raise ValueError("products='bf16x3' is an option of the fp32 mode")
        self.compute_dtype = compute_dtype
        self.products = products
        self.spec = GenSpec.from_cfg(gen_cfg)
        self._tuning = None
        self._use_tuning = use_tuning
        self.gen_cfg = gen_cfg
        if not torch.cuda.is_available():
            raise RuntimeError("render_in_between_amd.Generator needs a ROCm GPU (MI355X); "
                               "there is no CPU path")
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device())
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("Generator device must be a GPU, got %s" % (self.device,))
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self._lib = _native.lib()
        s = self.spec
        cfg = _native.RibConfig(
            label_nc=s.label_nc, image_nc=s.image_nc, num_filters=s.num_filters,
            max_num_filters=s.max_num_filters, num_layers=s.num_layers,
            num_down_img=s.num_down_img, emb_filters=s.emb_filters,
            emb_max_filters=s.emb_max_filters, emb_down=s.emb_down,
            mask_filters=s.mask_filters, mask_max_filters=s.mask_max_filters,
            mask_down=s.mask_down, mask_res_blocks=s.mask_res_blocks)
        h = C.c_void_p()
        rc = self._lib.rib_create(C.byref(cfg), self.device.index, C.byref(h))
        if rc != 0:
            msg = self._lib.rib_last_error(None)
            raise (NotImplementedError if rc == -2 else _native.RibError)(
                *(("rib_create: " + msg.decode(),) if rc == -2 else (rc, msg.decode())))
        self._h = h
        _native.check(h, self._lib.rib_set_compute_dtype(h, {"f32": 0, "bf16": 1, "f16": 3}[compute_dtype]))
        _native.check(h, self._lib.rib_set_products(h, {"f32": 0, "bf16x3": 1}[products]))
        self._ws: Dict[tuple, torch.Tensor] = {}
        self._plan_batch = 0
        self._tuned: Dict[tuple, int] = {}      # (B,H,W) -> launches whose variant came from the measured table
        self._applied: Dict[tuple, int] = {}    # (TB,H,W) whose table entries have been pinned on the handle -> how many
        self.training = False
        self._graph_replay = bool(int(__import__("os").environ.get("RIB_GRAPH", "0") or 0))
        self.weights_version = 0        # bumped by load_state_dict / import_weights (Evaluator's lane clones follow it)
        self._warned_copy = False

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            self._lib.rib_destroy(h)
            self._h = None

    # ---- nn.Module-protocol no-ops the reference driver calls ----------------------------
    def eval(self):
        self.training = False
        return self

    def train(self, mode=True):
        if mode:
            raise NotImplementedError("the MI355X path is inference-only")
        return self.eval()

    def to(self, device=None, *a, **k):
        if device is not None and torch.device(device).type == "cuda":
            idx = torch.device(device).index
            if idx is not None and idx != self.device.index:
                raise RuntimeError("a Generator handle is bound to one GPU; construct it on %s" % device)
        return self

    def cuda(self, device=None):
        return self.to("cuda" if device is None else device)

    # ---- checkpoint surface ---------------------------------------------------------------
    def expected_tensors(self):
        """[(name, shape, used)] exactly as the native loader expects them."""
        out = []
        name = C.c_char_p(); ndim = C.c_int(); dims = (C.c_int64 * 4)(); used = C.c_int()
        for i in range(self._lib.rib_num_tensors(self._h)):
            _native.check(self._h, self._lib.rib_tensor_info(self._h, i, C.byref(name), C.byref(ndim), dims, C.byref(used)))
            out.append((name.value.decode(), tuple(dims[j] for j in range(ndim.value)), bool(used.value)))
        return out

    def load_state_dict(self, state_dict, strict=True):
        """Same contract as nn.Module.load_state_dict(strict=True) on the
        reference generator (PGNR/utils/utils.py:107-119): every reference key
        must be present with its shape; unknown keys are an error."""
        if "state_dict" in state_dict and not torch.is_tensor(state_dict["state_dict"]):
            state_dict = state_dict["state_dict"]                      # utils.py:115-116
        sd = {k.replace("module.", ""): v for k, v in state_dict.items()}   # utils.py:101-105
        expected = {n for n, _, _ in self.expected_tensors()}
        if strict:
            missing = sorted(expected - set(sd))
            unexpected = sorted(set(sd) - expected)
            if missing or unexpected:
                raise RuntimeError("Error(s) in loading state_dict for Generator:\n\tMissing key(s): %s\n\t"
                                   "Unexpected key(s): %s" % (missing[:8], unexpected[:8]))
        for k, v in sd.items():
            if k not in expected:
                continue
            t = v.detach().to("cpu", torch.float32).contiguous()
            dims = (C.c_int64 * max(t.dim(), 1))(*t.shape)
            _native.check(self._h, self._lib.rib_set_tensor(self._h, k.encode(), C.c_void_p(t.data_ptr()), t.dim(), dims))
        with torch.cuda.device(self.device):
            _native.check(self._h, self._lib.rib_finalize_weights(self._h))
        self.weights_version += 1
        if self.compute_dtype == "f16":
            self.assert_finite_probe()
        return self

    def assert_finite_probe(self, size=64, seed=0):
        """IEEE half ends at 65504.  rib_finalize_weights refuses a checkpoint whose FOLDED FILTERS leave that range; this
        checks the ACTIVATIONS: one small forward on full-range inputs (frames uniform in [-1, 1], label maps in their value
        ranges) must come out finite - the condition encoder is five convolutions with no normalisation between them, the one
        place where a trained checkpoint's larger filters can compound.  Raises FloatingPointError (the f16 mode must fail
        loudly, not render NaN frames); called by load_state_dict in the f16 mode."""
        m = 1 << max(self.spec.num_down_img + 1, self.spec.mask_down, self.spec.emb_down)
        hw = max(size // m, 1) * m
        g = torch.Generator().manual_seed(seed)
        label = torch.cat([torch.rand(1, 3, hw, hw, generator=g) * 2 - 1, torch.rand(1, self.spec.label_nc - 3, hw, hw, generator=g)], dim=1)
        fake, prev = torch.rand(1, self.spec.image_nc, hw, hw, generator=g) * 2 - 1, torch.rand(1, self.spec.image_nc, hw, hw, generator=g) * 2 - 1
        img, mask = self(label.to(self.device), None, fake.to(self.device), prev.to(self.device))
        if not (bool(torch.isfinite(img).all()) and bool(torch.isfinite(mask).all())):
            raise FloatingPointError("compute_dtype='%s': this checkpoint's activations leave the 16-bit format's range (non-finite output on "
                                     "a %dx%d probe frame); use compute_dtype='bf16' (same speed, fp32's range) or 'f32'" % (self.compute_dtype, hw, hw))
        return True

    # ---- multi-GPU weight hand-off (one RCCL broadcast of the folded blob) -----------------
    def export_weights(self) -> torch.Tensor:
        n = self._lib.rib_weights_bytes(self._h)
        buf = torch.empty(n // 4, dtype=torch.float32, device=self.device)
        _native.check(self._h, self._lib.rib_export_weights(self._h, _ptr(buf), n, self._stream()))
        return buf

    def clone(self) -> "Generator":
        """A second handle on the same device with the same folded weights (device-to-device copy
        of the blob): used to keep several independent segments in flight on separate HIP streams
        (a handle is single-stream)."""
        g = Generator(self.gen_cfg, device=self.device, use_tuning=self._use_tuning, compute_dtype=self.compute_dtype,
                      products=self.products)
        g.set_plan_batch(self._plan_batch)
        blob = self.export_weights()
        g.import_weights(blob)
        torch.cuda.current_stream(self.device).synchronize()
        return g

    def weights_numel(self) -> int:
        return self._lib.rib_weights_bytes(self._h) // 4

    def import_weights(self, buf: torch.Tensor):
        assert buf.is_cuda and buf.dtype == torch.float32 and buf.is_contiguous()
        _native.check(self._h, self._lib.rib_import_weights(self._h, _ptr(buf), buf.numel() * 4, self._stream()))
        self.weights_version += 1
        return self

    # ---- forward ----------------------------------------------------------------------------
    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def set_plan_batch(self, n):
        """Batch-invariant launch plans (rib_set_plan_batch, include/rib.h): with n > 0 every plan, whatever its batch, follows
        the kernel choices of batch n, so a sample's frames are bit-identical in every grouping (B = 1, a ragged group of 3,
        a full group); 0 = every batch its own choices (the default of a handle; fastest for a single call)."""
        n = max(0, int(n))
        if n != self._plan_batch:
            _native.check(self._h, self._lib.rib_set_plan_batch(self._h, n))
            self._plan_batch = n
            self._ws.clear()                     # the workspace a shape needs follows the plans
            self.__dict__.pop("_chain_ws", None)
            self.__dict__.pop("_chain_out", None)
        return self

    @property
    def plan_batch(self):
        return self._plan_batch

    def _workspace(self, B, H, W):
        key = (B, H, W)
        ws = self._ws.get(key)
        if ws is None:
            TB = self._plan_batch or B           # the batch whose measured choices this shape's plans follow
            if self._use_tuning:
                from . import tuning
                if self._tuning is None:
                    self._tuning = tuning.load(dtype=self.compute_dtype)
                if (TB, H, W) not in self._applied:      # once per followed shape: re-pinning drops the plans that follow it
                    self._applied[(TB, H, W)] = tuning.apply(self._lib, self._h, self._tuning, TB, H, W, dtype=self.compute_dtype)
                self._tuned[key] = self._applied[(TB, H, W)]
            n = self._lib.rib_workspace_bytes(self._h, B, H, W)
            if n == 0 and self._use_tuning and self._tuning.get("%d,%d,%d" % (TB, H, W)):
                # a stale tuning entry must never break the path: drop it and use the cost model
                for op in self._tuning["%d,%d,%d" % (TB, H, W)]:
                    self._lib.rib_set_choice(self._h, TB, H, W, op.encode(), -1, 1)
                self._applied[(TB, H, W)] = self._tuned[key] = 0
                # erasing the choices of (TB, H, W) rebuilds EVERY plan that follows TB, other batch sizes included: the
                # workspaces cached for them were sized under the old choices (rib_forward / rib_chain reject a workspace
                # smaller than the current plan needs, so a stale one could only fail loudly - but it need not fail at all)
                self._ws.clear()
                self.__dict__.pop("_chain_ws", None)
                self.__dict__.pop("_chain_out", None)
                n = self._lib.rib_workspace_bytes(self._h, B, H, W)
            if n == 0:
                _native.check(self._h, -1)
            ws = torch.empty(n, dtype=torch.uint8, device=self.device)
            self._ws[key] = ws
        return ws

    def _prep(self, t, ch, name, shape=None):
        if not torch.is_tensor(t) or t.dim() != 4 or t.shape[1] != ch:
            raise ValueError("%s must be a [B,%d,H,W] tensor, got %s" % (name, ch, tuple(getattr(t, "shape", ()))))
        if shape is not None and (t.shape[0], t.shape[2], t.shape[3]) != shape:
            raise ValueError("%s has shape %s, expected B,H,W = %s" % (name, tuple(t.shape), shape))
        if t.device != self.device or t.dtype != torch.float32 or not t.is_contiguous():
            if not self._warned_copy:
                # the reference driver keeps results['fuse'] on the CPU (evaluator.py:252): fed to this object unchanged
                # that is a host-to-device copy per frame; say so once instead of hiding it
                import warnings
                warnings.warn("Generator: %s arrived as %s/%s%s and is copied to %s float32 contiguous on every call; keep "
                              "the tensors on the GPU (or use Generator.chain) to avoid a per-frame copy"
                              % (name, t.device, str(t.dtype).replace("torch.", ""), "" if t.is_contiguous() else "/strided", self.device))
                self._warned_copy = True
            t = t.to(self.device, torch.float32)
        return t.contiguous()

    def __call__(self, label, label_prev, img_fake, img_prev):
        """img_final, mask = G(label, label_prev, img_fake, img_prev)
        (generator.py:181-234).  ``label_prev`` is accepted and ignored — the
        reference never reads it; it may be None."""
        s = self.spec
        label = self._prep(label, s.label_nc, "label")
        B, _, H, W = label.shape
        img_fake = self._prep(img_fake, s.image_nc, "img_fake", (B, H, W))
        img_prev = self._prep(img_prev, s.image_nc, "img_prev", (B, H, W))
        ws = self._workspace(B, H, W)
        img = torch.empty((B, s.image_nc, H, W), dtype=torch.float32, device=self.device)
        mask = torch.empty((B, 1, H, W), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _native.check(self._h, self._lib.rib_forward(
                self._h, B, H, W, _ptr(label), _ptr(img_fake), _ptr(img_prev), _ptr(img), _ptr(mask),
                _ptr(ws), ws.numel(), self._stream()))
        return img, mask

    forward = __call__

    def forward_blend(self, label, label_prev, img_fake, img_prev):
        """(img, mask, fuse): the forward plus the driver's blend fuse = img*mask + img_fake*(1-mask)
        (evaluator.py:256-258) in one call; the mask head's kernel writes the fused frame."""
        s = self.spec
        label = self._prep(label, s.label_nc, "label")
        B, _, H, W = label.shape
        img_fake = self._prep(img_fake, s.image_nc, "img_fake", (B, H, W))
        img_prev = self._prep(img_prev, s.image_nc, "img_prev", (B, H, W))
        ws = self._workspace(B, H, W)
        img = torch.empty((B, s.image_nc, H, W), dtype=torch.float32, device=self.device)
        fuse = torch.empty_like(img)
        mask = torch.empty((B, 1, H, W), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _native.check(self._h, self._lib.rib_forward_blend(
                self._h, B, H, W, _ptr(label), _ptr(img_fake), _ptr(img_prev), _ptr(img), _ptr(mask), _ptr(fuse),
                _ptr(ws), ws.numel(), self._stream()))
        return img, mask, fuse

    def chain(self, key_frame, labels, dains, want_all=True):
        """One autoregressive segment on device (evaluator.py:238-262):
        labels [T,B,label_nc,H,W], dains [T,B,image_nc,H,W], key_frame
        [B,image_nc,H,W] -> (imgs, masks, fuses); prev never leaves HBM."""
        s = self.spec
        T = labels.shape[0]
        B, H, W = labels.shape[1], labels.shape[3], labels.shape[4]
        labels = labels.to(self.device, torch.float32).contiguous()
        dains = dains.to(self.device, torch.float32).contiguous()
        key_frame = self._prep(key_frame, s.image_nc, "key_frame", (B, H, W))
        assert labels.shape == (T, B, s.label_nc, H, W) and dains.shape == (T, B, s.image_nc, H, W)
        ws = self._workspace(B, H, W)
        need = int(self._lib.rib_chain_workspace_bytes(self._h, T, B, H, W))      # + the batched label-only launches
        if need > ws.numel():
            # one grow-only buffer per batch size: the chunks of a segment differ in T (8, 8, 8, 7) and share it
            cache = self.__dict__.setdefault("_chain_ws", {})
            cws = cache.get((B, H, W))
            if cws is None or cws.numel() < need:
                cache.pop((B, H, W), None)
                cws = cache[(B, H, W)] = torch.empty(need, dtype=torch.uint8, device=self.device)
            ws = cws
        if self._graph_replay:
            # a replayed graph writes where it was captured: two alternating output sets per shape (the previous call's frames
            # stay valid while the next call runs - a chunked segment reads its `prev` from them), overwritten two calls later
            ring = self.__dict__.setdefault("_chain_out", {}).setdefault((T, B, H, W, bool(want_all)), {"n": 0, "sets": []})
            if len(ring["sets"]) < 2:
                fz = torch.empty((T, B, s.image_nc, H, W), dtype=torch.float32, device=self.device)
                ring["sets"].append((torch.empty_like(fz) if want_all else None,
                                     torch.empty((T, B, 1, H, W), dtype=torch.float32, device=self.device) if want_all else None, fz))
            imgs, masks, fuses = ring["sets"][ring["n"] % len(ring["sets"])] if len(ring["sets"]) == 2 else ring["sets"][-1]
            ring["n"] += 1
        else:
            fuses = torch.empty((T, B, s.image_nc, H, W), dtype=torch.float32, device=self.device)
            imgs = torch.empty_like(fuses) if want_all else None
            masks = torch.empty((T, B, 1, H, W), dtype=torch.float32, device=self.device) if want_all else None
        with torch.cuda.device(self.device):
            _native.check(self._h, self._lib.rib_chain(
                self._h, T, B, H, W, _ptr(key_frame), _ptr(labels), _ptr(dains), _ptr(imgs), _ptr(masks),
                _ptr(fuses), _ptr(ws), ws.numel(), self._stream()))
        return imgs, masks, fuses

    def set_wino_in_staging(self, on=True):
        """Staged Winograd input transforms (rib_set_wino_in_staging, include/rib.h): on by default; off runs the unstaged
        kernels, which write the same bits.  Rebuilds the launch plans; the workspace a shape needs stays the same."""
        _native.check(self._h, self._lib.rib_set_wino_in_staging(self._h, 1 if on else 0))
        return self

    def set_graph_replay(self, on=True):
        """rib_chain as ONE HIP graph launch per (shape, tensors): see include/rib.h.  Also on with RIB_GRAPH=1."""
        _native.check(self._h, self._lib.rib_set_graph_replay(self._h, 1 if on else 0))
        self._graph_replay = bool(on)
        self.__dict__.pop("_chain_out", None)
        return self

    def graph_stats(self):
        cap, rep = C.c_int64(), C.c_int64()
        _native.check(self._h, self._lib.rib_graph_stats(self._h, C.byref(cap), C.byref(rep)))
        return {"captures": cap.value, "replays": rep.value}

    # ---- driver-side ops ----------------------------------------------------------------------
    def blend(self, img, mask, dain):
        img = img.to(self.device, torch.float32).contiguous(); mask = mask.to(self.device, torch.float32).contiguous()
        dain = dain.to(self.device, torch.float32).contiguous()
        B, Cc, H, W = img.shape
        out = torch.empty_like(img)
        _native.check(self._h, self._lib.rib_blend(self._h, B, Cc, H, W, _ptr(img), _ptr(mask), _ptr(dain), _ptr(out), self._stream()))
        return out

    def quantise(self, img, out=None):
        """out: optional contiguous uint8 [B,H,W,C] destination on the device (e.g. a view of a larger buffer)."""
        img = img.to(self.device, torch.float32).contiguous()
        B, Cc, H, W = img.shape
        if out is None:
            out = torch.empty((B, H, W, Cc), dtype=torch.uint8, device=self.device)
        assert out.shape == (B, H, W, Cc) and out.dtype == torch.uint8 and out.is_contiguous() and out.device == self.device
        _native.check(self._h, self._lib.rib_quantise(self._h, B, Cc, H, W, _ptr(img), _ptr(out), self._stream()))
        return out

    def quality(self, pred, target, mask=None, out=None):
        """Masked PSNR / SSIM of B frames against ground truth (rib_quality; metrics.py states the metric):
        pred, target [B,3,H,W] in [-1,1], mask [B,H,W] or None -> (psnr[B], ssim[B]) float32 device tensors, enqueued on
        the current stream.  out: optional float32 [2,B] device destination (row 0 PSNR, row 1 SSIM)."""
        pred = self._prep(pred, 3, "pred")
        B, Cc, H, W = pred.shape
        target = self._prep(target, 3, "target", (B, H, W))
        if mask is not None:
            if tuple(mask.shape) != (B, H, W):
                raise ValueError("mask must be [B,H,W] = %s, got %s" % ((B, H, W), tuple(mask.shape)))
            mask = mask.to(self.device, torch.float32).contiguous()
        n = self._lib.rib_quality_workspace_bytes(self._h, B, H, W)
        if n == 0:
            from .metrics import downsample_factor
            f = downsample_factor(H, W)
            raise ValueError("SSIM: the frame is %dx%d after %dx downsampling, smaller than the 11x11 window" % (H // f, W // f, f))
        cache = self.__dict__.setdefault("_quality_ws", {})
        ws = cache.get((B, H, W))
        if ws is None:
            ws = cache[(B, H, W)] = torch.empty(n, dtype=torch.uint8, device=self.device)
        if out is None:
            out = torch.empty((2, B), dtype=torch.float32, device=self.device)
        assert out.shape == (2, B) and out.dtype == torch.float32 and out.is_contiguous() and out.device == self.device
        with torch.cuda.device(self.device):
            _native.check(self._h, self._lib.rib_quality(
                self._h, B, Cc, H, W, _ptr(pred), _ptr(target), _ptr(mask), _ptr(out[0]), _ptr(out[1]),
                _ptr(ws), ws.numel(), self._stream()))
        return out[0], out[1]

    def _cubic_tables(self, H0, W0, height, width):
        """The device tap tables ix, cx [width,4], iy, cy [height,4] of a cubic resize H0 x W0 -> height x width
        (resize._cubic_taps), as four pointers; built once per size pair and kept on the device."""
        cache = self.__dict__.setdefault("_resize_taps", {})
        taps = cache.get((H0, W0, height, width))
        if taps is None:
            from .resize import _cubic_taps
            import numpy as np
            (ix, cx), (iy, cy) = _cubic_taps(width, W0), _cubic_taps(height, H0)
            host = np.concatenate([a.astype(np.int32).reshape(-1) for a in (ix, cx, iy, cy)])
            # (kept for the life of the handle: a few KB per size pair, and a launch enqueued on another stream may still read it)
            taps = cache[(H0, W0, height, width)] = torch.from_numpy(host).to(self.device)
        nx, ny = width * 4 * 4, height * 4 * 4            # bytes of one table of each axis
        base = taps.data_ptr()
        return [C.c_void_p(base + o) for o in (0, nx, 2 * nx, 2 * nx + ny)]

    def resize_u8(self, frames_u8, width, height, normalised=False, out=None):
        """The folder driver's frame resize on the GPU (rib_resize_cubic): uint8 [N,H0,W0,3] (or [H0,W0,3]) on this device
        -> uint8 [N,height,width,3] (or [height,width,3]), bit-exact to resize.resize_cubic_u8; normalised=True: float32
        [N,3,height,width] holding ToTensor + Normalize(0.5, 0.5) of it, ((u8 / 255.0 - 0.5) / 0.5) as torch evaluates it
        on the device.  A frame already at the target size comes back as a copy (or normalised).  The tap tables of
        resize._cubic_taps are built once per (H0, W0, height, width) and kept on the device.  Enqueued on the current
        stream.  out: optional contiguous destination of the result's shape and dtype."""
        if not torch.is_tensor(frames_u8) or frames_u8.dtype != torch.uint8 or frames_u8.dim() not in (3, 4) or frames_u8.shape[-1] != 3:
            raise ValueError("frames_u8 must be a uint8 [N,H0,W0,3] or [H0,W0,3] tensor, got %s %s"
                             % (getattr(frames_u8, "dtype", type(frames_u8)), tuple(getattr(frames_u8, "shape", ()))))
        if frames_u8.device != self.device:
            raise ValueError("resize_u8: frames_u8 is on %s, the generator on %s (upload the frames first)" % (frames_u8.device, self.device))
        width, height = int(width), int(height)
        single = frames_u8.dim() == 3
        src = (frames_u8.unsqueeze(0) if single else frames_u8).contiguous()
        N, H0, W0, _ = src.shape
        if min(N, H0, W0) < 1 or width < 1 or height < 1:
            raise ValueError("resize_u8: empty frames or a non-positive target size (%s -> %dx%d)" % (tuple(src.shape), width, height))
        shape, dtype = ((N, 3, height, width), torch.float32) if normalised else ((N, height, width, 3), torch.uint8)
        if out is None:
            res = torch.empty(shape, dtype=dtype, device=self.device)
        else:
            res = out.unsqueeze(0) if (single and out.dim() == 3) else out
            if tuple(res.shape) != shape or res.dtype != dtype or not res.is_contiguous() or res.device != self.device:
                raise ValueError("resize_u8: out must be a contiguous %s %s tensor on %s" % (shape, dtype, self.device))
        tabs = self._cubic_tables(H0, W0, height, width)
        with torch.cuda.device(self.device):
            _native.check(self._h, self._lib.rib_resize_cubic(
                self._h, N, H0, W0, height, width, _ptr(src), *tabs,
                _ptr(None if normalised else res), _ptr(res if normalised else None), self._stream()))
        if out is not None:
            return out
        return res[0] if single else res

    def composite(self, pred, mask, bg_u8, out=None):
        """The fused frame at the SOURCE size on the GPU (rib_composite, csrc/composite.hip.h; composite.composite_host is the
        definition and is bit-equal): pred [n,3,H,W] in [-1,1] and mask [n,1,H,W] in [0,1] at the model size (float32; 16-bit
        tensors are converted), bg_u8 uint8 [n,H0,W0,3] at the source size, all on this device -> uint8 [n,H0,W0,3]:
        the 8-bit cubic enlargement of the quantised prediction over the background's own pixels, weighted by the enlarged
        8-bit mask.  Any size pair.  out: optional contiguous uint8 destination of bg_u8's shape at any byte offset, e.g. a
        section of a download buffer; it may be bg_u8 itself (in place).  One launch on the current stream."""
        for t, ch, name in ((pred, 3, "pred"), (mask, 1, "mask")):
            if not torch.is_tensor(t) or t.dim() != 4 or t.shape[1] != ch or t.dtype not in (torch.float32, torch.float16, torch.bfloat16):
                raise ValueError("composite: %s must be a float [n,%d,H,W] tensor, got %s %s"
                                 % (name, ch, getattr(t, "dtype", type(t)), tuple(getattr(t, "shape", ()))))
            if t.device != self.device:
                raise ValueError("composite: %s is on %s, the generator on %s" % (name, t.device, self.device))
        if not torch.is_tensor(bg_u8) or bg_u8.dtype != torch.uint8 or bg_u8.dim() != 4 or bg_u8.shape[-1] != 3:
            raise ValueError("composite: bg_u8 must be a uint8 [n,H0,W0,3] tensor, got %s %s"
                             % (getattr(bg_u8, "dtype", type(bg_u8)), tuple(getattr(bg_u8, "shape", ()))))
        if bg_u8.device != self.device:
            raise ValueError("composite: bg_u8 is on %s, the generator on %s (upload the frames first)" % (bg_u8.device, self.device))
        N, _, H, W = pred.shape
        _, H0, W0, _ = bg_u8.shape
        if tuple(mask.shape) != (N, 1, H, W) or bg_u8.shape[0] != N:
            raise ValueError("composite: pred %s, mask %s and bg_u8 %s do not describe the same frames"
                             % (tuple(pred.shape), tuple(mask.shape), tuple(bg_u8.shape)))
        if min(N, H, W, H0, W0) < 1 or N > 65535:
            raise ValueError("composite: 1 <= n <= 65535 non-empty frames (pred %s, bg_u8 %s)" % (tuple(pred.shape), tuple(bg_u8.shape)))
        pred = pred.to(torch.float32).contiguous()
        mask = mask.to(torch.float32).contiguous()
        if out is None:
            res = torch.empty((N, H0, W0, 3), dtype=torch.uint8, device=self.device)
        else:
            res = out
            if not torch.is_tensor(res) or tuple(res.shape) != (N, H0, W0, 3) or res.dtype != torch.uint8 or not res.is_contiguous() \
                    or res.device != self.device:
                raise ValueError("composite: out must be a contiguous uint8 %s tensor on %s" % ((N, H0, W0, 3), self.device))
        # in place on the caller's own frames; a background that had to be made contiguous is a copy and cannot alias out
        bg = bg_u8 if bg_u8.is_contiguous() else bg_u8.contiguous()
        tabs = self._cubic_tables(H, W, H0, W0)
        with torch.cuda.device(self.device):
            _native.check(self._h, self._lib.rib_composite(self._h, N, H, W, H0, W0, _ptr(pred), _ptr(mask), _ptr(bg), *tabs,
                                                           _ptr(res), self._stream()))
        return res

    def warp(self, img, flow):
        img = img.to(self.device, torch.float32).contiguous(); flow = flow.to(self.device, torch.float32).contiguous()
        B, Cc, H, W = img.shape
        assert flow.shape == (B, 2, H, W)
        out = torch.empty_like(img)
        _native.check(self._h, self._lib.rib_warp(self._h, B, Cc, H, W, _ptr(img), _ptr(flow), _ptr(out), self._stream()))
        return out

    def rasterise(self, strokes, peaks, weights, radius, height, width, colors=None, halfwidth=None):
        """Label maps of T frames drawn on the GPU (rib_rasterise): strokes [T, E] of
        rasterise.STROKE_DTYPE, peaks [T, P, 2] int32, weights [radius+1] fp64 (host arrays, see
        rasterise.py) -> [T, 3+P, H, W] fp32 CUDA tensor."""
        import numpy as np
        from . import rasterise as R
        strokes = np.ascontiguousarray(strokes, R.STROKE_DTYPE)
        peaks = np.ascontiguousarray(peaks, np.int32)
        weights = np.ascontiguousarray(weights, np.float64)
        colors = np.ascontiguousarray(R.POSE_COLORS if colors is None else colors, np.uint8)
        halfwidth = R.STROKE_HALFWIDTH if halfwidth is None else int(halfwidth)
        T, E = strokes.shape
        P = peaks.shape[1]
        assert peaks.shape == (T, P, 2) and colors.shape == (E, 3) and weights.shape == (radius + 1,)
        nbytes = self._lib.rib_rasterise_workspace_bytes(self._h, T, height, width, E, P, radius)
        with torch.cuda.device(self.device):
            ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            out = torch.empty((T, 3 + P, height, width), dtype=torch.float32, device=self.device)
            _native.check(self._h, self._lib.rib_rasterise(
                self._h, T, height, width, strokes.ctypes.data, E, colors.ctypes.data, halfwidth,
                peaks.ctypes.data, P, weights.ctypes.data, radius, _ptr(out), _ptr(ws), ws.numel(), self._stream()))
        return out

    def human_mask(self, peaks, height, width, out=None):
        """The human-centric mask of the ground-truth metrics drawn on the GPU (rib_human_mask; _generate_human_mask restated
        from OpenCV's drawing, unpinned - rasterise.human_mask states the definition and is bit-equal): peaks [T, n, 2] (or
        [n, 2]) int host array of rasterise.peak_table, n = 18 or 19 -> float32 0/1 [T, H, W] on this device, enqueued on the
        current stream; it is what `quality` takes as its mask.  out: optional contiguous destination of that shape."""
        import numpy as np
        from . import rasterise as R
        if torch.is_tensor(peaks):
            peaks = peaks.detach().cpu().numpy()
        peaks = np.asarray(peaks)
        if peaks.ndim == 2:
            peaks = peaks[None]
        if peaks.ndim != 3 or peaks.shape[2] != 2 or peaks.shape[0] < 1 or peaks.dtype.kind not in "iu":
            raise ValueError("human_mask: peaks must be an integer [T, n, 2] array (rasterise.peak_table), got %s %s" % (peaks.dtype, peaks.shape))
        R.mask_limbs(peaks.shape[1])                                 # 18 or 19 joints
        height, width = int(height), int(width)
        if not (1 <= height <= R.MASK_MAX_SIDE and 1 <= width <= R.MASK_MAX_SIDE):
            raise ValueError("human_mask: height and width must be in 1..%d, got %dx%d" % (R.MASK_MAX_SIDE, height, width))
        on = peaks[..., 0] >= 0
        if np.any(peaks[..., 0] >= width) or np.any(on & ((peaks[..., 1] < 0) | (peaks[..., 1] >= height))):
            raise ValueError("human_mask: a peak lies outside the %dx%d frame (peak_table gives (-1, -1) for such a joint)" % (height, width))
        peaks = np.ascontiguousarray(peaks, np.int32)
        T, n = peaks.shape[:2]
        if out is None:
            out = torch.empty((T, height, width), dtype=torch.float32, device=self.device)
        elif tuple(out.shape) != (T, height, width) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != self.device:
            raise ValueError("human_mask: out must be a contiguous float32 %s tensor on %s" % ((T, height, width), self.device))
        with torch.cuda.device(self.device):
            _native.check(self._h, self._lib.rib_human_mask(self._h, T, height, width, peaks.ctypes.data, n, _ptr(out), self._stream()))
        return out

    def panel(self, pred, mask, fuse, dain, gt, label, titles=None, out=None):
        """The six-pane diagnostic sheets of T frames composed on the GPU (rib_panel, csrc/panel.hip.h; panel.compose_host is
        the definition and is bit-equal): float32 device tensors pred, fuse, dain, gt [T,3,H,W], mask [T,1,H,W], label
        [T,label_nc,H,W] -> uint8 [T,SH,SW,3] (panel.layout), one launch on the current stream, every byte written.
        pred, mask and fuse None together: key-frame mode (Predict = Fuse = gt, Mask = 0).
        titles: 0/1 [2,24,SW] (panel.title_bitmap; a host array is uploaded once per width and kept), or None: no text.
        out: optional contiguous uint8 destination of the result's shape, e.g. a view into a larger buffer."""
        from . import panel as P
        if (pred is None) != (mask is None) or (pred is None) != (fuse is None):
            raise ValueError("panel: pred, mask and fuse are None together (key-frame mode) or not at all")
        dain = self._prep(dain, 3, "dain")
        T, _, H, W = dain.shape
        gt = self._prep(gt, 3, "gt", (T, H, W))
        if not torch.is_tensor(label) or label.dim() != 4 or label.shape[1] < 3:
            raise ValueError("panel: label must be a [T,>=3,H,W] tensor, got %s" % (tuple(getattr(label, "shape", ())),))
        label = self._prep(label, label.shape[1], "label", (T, H, W))
        if pred is not None:
            pred, fuse = self._prep(pred, 3, "pred", (T, H, W)), self._prep(fuse, 3, "fuse", (T, H, W))
            mask = self._prep(mask, 1, "mask", (T, H, W))
        SH, SW = P.layout(H, W)["sheet"]
        if titles is not None and not (torch.is_tensor(titles) and titles.device == self.device):
            import numpy as np
            host = np.ascontiguousarray(titles.cpu().numpy() if torch.is_tensor(titles) else titles)
            if host.shape != (2, P.TITLE_H, SW):
                raise ValueError("panel: titles must be [2, %d, %d], got %s" % (P.TITLE_H, SW, host.shape))
            cache = self.__dict__.setdefault("_panel_titles", {})
            key = (SW, host.tobytes())
            if key not in cache:
                cache[key] = torch.from_numpy((host != 0).astype(np.uint8)).to(self.device)
            titles = cache[key]
        if titles is not None and (tuple(titles.shape) != (2, P.TITLE_H, SW) or titles.dtype != torch.uint8 or not titles.is_contiguous()):
            raise ValueError("panel: titles must be a contiguous uint8 [2, %d, %d] tensor" % (P.TITLE_H, SW))
        if out is None:
            out = torch.empty((T, SH, SW, 3), dtype=torch.uint8, device=self.device)
        elif tuple(out.shape) != (T, SH, SW, 3) or out.dtype != torch.uint8 or not out.is_contiguous() or out.device != self.device:
            raise ValueError("panel: out must be a contiguous uint8 %s tensor on %s" % ((T, SH, SW, 3), self.device))
        with torch.cuda.device(self.device):
            _native.check(self._h, self._lib.rib_panel(
                self._h, T, H, W, label.shape[1], _ptr(pred), _ptr(mask), _ptr(fuse), _ptr(dain), _ptr(gt), _ptr(label),
                _ptr(titles), _ptr(out), self._stream()))
        return out

    # ---- motion-compensated background (background.py states both results; csrc/mci.hip.h) ------------------------------
    def _mci_pair(self, a_u8, b_u8, who):
        for x in (a_u8, b_u8):
            if not torch.is_tensor(x) or x.dtype != torch.uint8 or x.dim() not in (3, 4) or x.shape[-1] != 3:
                raise ValueError("%s: key frames must be uint8 [B,H,W,3] or [H,W,3] tensors, got %s %s"
                                 % (who, getattr(x, "dtype", type(x)), tuple(getattr(x, "shape", ()))))
            if x.device != self.device:
                raise ValueError("%s: a key frame is on %s, the generator on %s (upload the frames first)" % (who, x.device, self.device))
        if a_u8.shape != b_u8.shape:
            raise ValueError("%s: the two key frames differ in shape: %s and %s" % (who, tuple(a_u8.shape), tuple(b_u8.shape)))
        single = a_u8.dim() == 3
        a = (a_u8.unsqueeze(0) if single else a_u8).contiguous()
        b = (b_u8.unsqueeze(0) if single else b_u8).contiguous()
        if min(a.shape[:3]) < 1:
            raise ValueError("%s: empty key frames %s" % (who, tuple(a.shape)))
        return a, b, single

    def _mci_field_arg(self, field, B, H, W, who, hint=("segments", "mci_field")):
        """field int16 [B,Hb,Wb,2] (or [Hb,Wb,2]) on this device -> contiguous [B,Hb,Wb,2].  hint: what the B frames of H x W are
        called in the refusal, and the method the field comes from."""
        from .background import field_shape
        Hb, Wb = field_shape(H, W)
        if not torch.is_tensor(field) or field.dtype != torch.int16 or field.device != self.device:
            raise ValueError("%s: field must be an int16 tensor on %s (%s)" % (who, self.device, hint[1]))
        f = (field.unsqueeze(0) if field.dim() == 3 else field).contiguous()
        if tuple(f.shape) != (B, Hb, Wb, 2):
            raise ValueError("%s: the field of %d %dx%d %s is [%d, %d, %d, 2], got %s" % (who, B, H, W, hint[0], B, Hb, Wb, tuple(field.shape)))
        return f

    @staticmethod
    def _mci_span(s, k_first, count, who):
        """(k_first, T): frames k_first .. k_first + T - 1 of a segment of s steps; count None: up to s - 1."""
        k_first = int(k_first)
        T = (s - k_first) if count is None else int(count)
        if T < 1 or k_first < 0 or k_first + T - 1 > s:
            raise ValueError("%s: frames %d..%d are outside the segment 0..%d" % (who, k_first, k_first + T - 1, s))
        return k_first, T

    def mci_field(self, a_u8, b_u8, levels=3, border="clamp"):
        """The block displacement field of B key-frame pairs on the GPU (rib_mci_field; background.mci_field_host is the
        definition and is bit-equal): a_u8, b_u8 uint8 [B,H,W,3] (or [H,W,3]) on this device, the left and right key frame of
        each segment at the model size -> int16 [B,Hb,Wb,2] (or [Hb,Wb,2]), (dx, dy) per 8x8 block.  levels: 3 (the default),
        4 or 5 pyramid levels, a search over 32, 64 or 128 px of motion between the key frames.  This project's
        interpolation, not DAIN.  border: "clamp" (the default) or "valid", one-sided matching at the frame border.
        levels + 2 launches on the current stream: five by default."""
        from .background import BORDERS, check_border, check_levels, field_shape
        levels = check_levels(levels, "mci_field")
        border = BORDERS.index(check_border(border, "mci_field"))
        a, b, single = self._mci_pair(a_u8, b_u8, "mci_field")
        B, H, W, _ = a.shape
        n = int(self._lib.rib_mci_workspace_bytes(self._h, B, H, W, levels))
        if n == 0:
            raise ValueError("mci_field: B=%d H=%d W=%d: 1 <= B <= 32767, H and W in 1..16384" % (B, H, W))
        Hb, Wb = field_shape(H, W)
        with torch.cuda.device(self.device):
            ws = torch.empty(n, dtype=torch.uint8, device=self.device)      # (per call: it belongs to the stream the call is enqueued on)
            field = torch.empty((B, Hb, Wb, 2), dtype=torch.int16, device=self.device)
            _native.check(self._h, self._lib.rib_mci_field(self._h, B, H, W, _ptr(a), _ptr(b), _ptr(field), levels, border, _ptr(ws),
                                                           self._stream()))
        return field[0] if single else field

    def mci_refine(self, a_u8, b_u8, field, border="clamp", out=None):
        """The half-pel refinement of mci_field's result on the GPU (rib_halfpel_refine; background.mci_refine_host is the
        definition and is bit-equal): a_u8, b_u8 uint8 [B,H,W,3] (or [H,W,3]), field int16 [B,Hb,Wb,2] (or [Hb,Wb,2]) on this
        device, components within +-79 -> a new int16 tensor of the same shape in HALF pixels, for
        mci_frames(precision="half").  out: optional contiguous destination of the field's shape; it may be the field itself (in
        place: a block reads only its own vector).  One launch on the current stream, no workspace."""
        from .background import BORDERS, check_border, field_shape
        border = BORDERS.index(check_border(border, "mci_refine"))
        a, b, single = self._mci_pair(a_u8, b_u8, "mci_refine")
        B, H, W, _ = a.shape
        Hb, Wb = field_shape(H, W)
        f = self._mci_field_arg(field, B, H, W, "mci_refine")
        with torch.cuda.device(self.device):
            if out is None:
                res = torch.empty_like(f)
            else:
                res = out.unsqueeze(0) if (torch.is_tensor(out) and out.dim() == 3) else out
                if not torch.is_tensor(res) or tuple(res.shape) != (B, Hb, Wb, 2) or res.dtype != torch.int16 or not res.is_contiguous() or res.device != self.device:
                    raise ValueError("mci_refine: out must be a contiguous int16 %s tensor on %s" % ((B, Hb, Wb, 2), self.device))
            _native.check(self._h, self._lib.rib_halfpel_refine(self._h, B, H, W, _ptr(a), _ptr(b), _ptr(f), _ptr(res), border, self._stream()))
        return res[0] if single else res

    def mci_detail_field(self, a0_u8, b0_u8, field, model_hw, border="clamp", precision="full"):
        """The block field refined at the key frames' OWN size on the GPU (rib_detail_field; background.mci_detail_field_host is the
        definition and is bit-equal): a0_u8, b0_u8 uint8 [B,h0,w0,3] (or [h0,w0,3]) the key frame files' pixels on this device,
        field the int16 [B,Hb,Wb,2] field of the MODEL-size key frames (mci_field, or mci_refine's in half pixels with
        precision="half"), model_hw = (H, W) -> int16 [B,ceil(h0/8),ceil(w0/8),2] in whole output pixels: every block starts from
        the scaled model-size vector at its centre and searches +-detail_radius around it on the full-size lumas, then the median.
        The frames at that size are mci_frames(a0_u8, b0_u8, F0, ..., normalised=False, precision="full", sampler=...).  Two
        launches on the current stream."""
        from .background import BORDERS, PRECISIONS, check_border, check_precision, field_shape, scaled_factors
        border = BORDERS.index(check_border(border, "mci_detail_field"))
        precision = PRECISIONS.index(check_precision(precision, "mci_detail_field"))
        a, b, single = self._mci_pair(a0_u8, b0_u8, "mci_detail_field")
        B, h0, w0, _ = a.shape
        H, W = (int(v) for v in model_hw)
        scaled_factors((H, W), (h0, w0), "mci_detail_field")
        f = self._mci_field_arg(field, B, H, W, "mci_detail_field", ("model frames", "mci_field"))
        n = int(self._lib.rib_detail_workspace_bytes(self._h, B, h0, w0))
        if n == 0:
            raise ValueError("mci_detail_field: B=%d h0=%d w0=%d: 1 <= B <= 32767, the sides in 1..16384" % (B, h0, w0))
        H0b, W0b = field_shape(h0, w0)
        with torch.cuda.device(self.device):
            ws = torch.empty(n, dtype=torch.uint8, device=self.device)      # (per call: it belongs to the stream the call is enqueued on)
            res = torch.empty((B, H0b, W0b, 2), dtype=torch.int16, device=self.device)
            _native.check(self._h, self._lib.rib_detail_field(self._h, B, H, W, h0, w0, _ptr(a), _ptr(b), _ptr(f), precision, border, _ptr(res),
                                                              _ptr(ws), self._stream()))
        return res[0] if single else res

    def mci_frames(self, a_u8, b_u8, field, sample_rate, k_first=1, count=None, normalised=True, out=None, border="clamp", precision="full",
                   sampler="bilinear", _staging=0):
        """Frames k_first .. k_first + count - 1 (count None: up to sample_rate - 1) of B segments from their key frames and
        block fields, all in one launch (rib_mci_frames; background.mci_frames_host is the definition and is bit-equal):
        a_u8, b_u8 uint8 [B,H,W,3], field int16 [B,Hb,Wb,2] (mci_field) on this device, sample_rate a power of two.
        normalised=True: float32 [T,B,3,H,W], ToTensor + Normalize(0.5, 0.5) as the folder driver's upload computes it;
        False: uint8 [T,B,H,W,3]; "both": the pair (float32, uint8).  [H,W,3] key frames give [T,3,H,W] / [T,H,W,3].
        out: optional contiguous destination (for "both": a pair).  border: "clamp" (the default) or "valid": where exactly
        one of a pixel's two samples lies inside the frame, that sample alone.  precision: "full" (the default) or "half": the
        field is mci_refine's, in half pixels (rib_halfpel_frames).  sampler: "bilinear" (the default) or "cubic": the 4x4
        Catmull-Rom sample (rib_cubic_frames; background.sample_cubic), nothing else changed; _staging (cubic only) is that
        entry's diagnostic: 0 = the per-tile rule, 1 = never stage - the bytes do not depend on it."""
        return self._mci_frames_body("mci_frames", a_u8, b_u8, None, field, sample_rate, k_first, count, normalised, out, border, precision,
                                     sampler, _staging)

    def _mci_frames_body(self, who, a_u8, b_u8, masks, field, sample_rate, k_first, count, normalised, out, border, precision, sampler, staging,
                         accel=None):
        """mci_frames (masks None), mci_frames_masked (masks = (ma, mb)) and mci_frames_accel (accel given, masks either): one check per
        argument, in one order, and one launch."""
        from .background import BORDERS, PRECISIONS, check_border, check_precision, check_sampler, log2_rate
        border = BORDERS.index(check_border(border, who))
        cubic = check_sampler(sampler, who) == "cubic"
        precision = PRECISIONS.index(check_precision(precision, who))
        a, b, single = self._mci_pair(a_u8, b_u8, who)
        B, H, W, _ = a.shape
        qa, qb = self._mci_masks(masks[0], masks[1], (B, H, W), single, who) if masks is not None else (None, None)
        log2_rate(sample_rate)
        s = int(sample_rate)
        f = self._mci_field_arg(field, B, H, W, who, ("segments", "mci_field" if masks is None else "mci_field_masked"))
        k_first, T = self._mci_span(s, k_first, count, who)
        acc = self._mci_field_arg(accel, B, H, W, who, ("segments", "mci_accel_field")) if accel is not None else None
        if normalised not in (True, False, "both"):
            raise ValueError("%s: normalised must be True, False or 'both'" % who)
        fshape, ushape = (T, B, 3, H, W), (T, B, H, W, 3)
        of, ou = (out if normalised == "both" else (out, None) if normalised else (None, out)) if out is not None else (None, None)

        def dest(t, shape, dtype):
            if t is None:
                return torch.empty(shape, dtype=dtype, device=self.device)
            v = t.unsqueeze(1) if (single and t.dim() == 4) else t
            if tuple(v.shape) != shape or v.dtype != dtype or not v.is_contiguous() or v.device != self.device:
                raise ValueError("%s: out must be a contiguous %s %s tensor on %s" % (who, shape, dtype, self.device))
            return v
        with torch.cuda.device(self.device):
            rf = dest(of, fshape, torch.float32) if normalised in (True, "both") else None
            ru = dest(ou, ushape, torch.uint8) if normalised in (False, "both") else None
            head, tail = (self._h, T, B, H, W, _ptr(a), _ptr(b)), (_ptr(rf), _ptr(ru), self._stream())
            if acc is not None:
                rc = self._lib.rib_accel_frames(*head, _ptr(qa), _ptr(qb), _ptr(f), _ptr(acc), s, k_first, border, precision, int(cubic), *tail)
            elif cubic:
                rc = self._lib.rib_cubic_frames(*head, _ptr(qa), _ptr(qb), _ptr(f), s, k_first, border, precision, int(staging), *tail)
            elif masks is not None:
                rc = self._lib.rib_masked_frames(*head, _ptr(qa), _ptr(qb), _ptr(f), s, k_first, border, precision, *tail)
            else:
                entry = self._lib.rib_halfpel_frames if precision else self._lib.rib_mci_frames
                rc = entry(*head, _ptr(f), s, k_first, border, *tail)
            _native.check(self._h, rc)
        res = tuple((r[:, 0] if single else r) for r in (rf, ru) if r is not None)
        return res if normalised == "both" else res[0]

    def _mci_masks(self, ma, mb, shape, single, who):
        """ma, mb uint8 [B,H,W] (or [H,W] beside [H,W,3] key frames) on this device, nonzero = excluded -> contiguous [B,H,W]."""
        out = []
        for m in (ma, mb):
            if not torch.is_tensor(m) or m.dtype != torch.uint8 or m.device != self.device:
                raise ValueError("%s: a mask must be a uint8 tensor on %s, got %s" % (who, self.device, getattr(m, "dtype", type(m))))
            m = m.unsqueeze(0) if (single and m.dim() == 2) else m
            if tuple(m.shape) != tuple(shape):
                raise ValueError("%s: the masks of %s key frames are uint8 %s, got %s" % (who, tuple(shape) + (3,), tuple(shape), tuple(m.shape)))
            out.append(m.contiguous())
        return out

    def mci_field_masked(self, a_u8, b_u8, ma, mb, levels=3, border="clamp"):
        """mci_field with the person kept out of the matching (rib_masked_field; background.mci_field_masked_host is the
        definition and is bit-equal): ma, mb uint8 [B,H,W] (or [H,W]) on this device, nonzero = excluded, for the left and the
        right key frame -> int16 [B,Hb,Wb,2] (or [Hb,Wb,2]).  levels + 4 launches on the current stream."""
        from .background import BORDERS, check_border, check_levels, field_shape
        levels = check_levels(levels, "mci_field_masked")
        border = BORDERS.index(check_border(border, "mci_field_masked"))
        a, b, single = self._mci_pair(a_u8, b_u8, "mci_field_masked")
        B, H, W, _ = a.shape
        qa, qb = self._mci_masks(ma, mb, (B, H, W), single, "mci_field_masked")
        n = int(self._lib.rib_masked_workspace_bytes(self._h, B, H, W, levels))
        if n == 0:
            raise ValueError("mci_field_masked: B=%d H=%d W=%d: 1 <= B <= 32767, H and W in 1..16384" % (B, H, W))
        Hb, Wb = field_shape(H, W)
        with torch.cuda.device(self.device):
            ws = torch.empty(n, dtype=torch.uint8, device=self.device)      # (per call: it belongs to the stream the call is enqueued on)
            field = torch.empty((B, Hb, Wb, 2), dtype=torch.int16, device=self.device)
            _native.check(self._h, self._lib.rib_masked_field(self._h, B, H, W, _ptr(a), _ptr(b), _ptr(qa), _ptr(qb), _ptr(field), levels,
                                                              border, _ptr(ws), self._stream()))
        return field[0] if single else field

    def mci_frames_masked(self, a_u8, b_u8, ma, mb, field, sample_rate, k_first=1, count=None, normalised=True, out=None, border="clamp",
                          precision="full", sampler="bilinear", _staging=0):
        """mci_frames with the person kept out (rib_masked_frames; background.mci_frames_masked_host is the definition and is
        bit-equal): ma, mb uint8 [B,H,W] (or [H,W]) on this device, nonzero = excluded; where exactly one of a pixel's two samples
        is clean - valid under `border`, and the four taps of its footprint in its key frame's mask all zero - the output is that
        sample alone.  Everything else - field, frames, normalised (True, False, "both"), out, precision, sampler, _staging - is
        mci_frames'; sampler="cubic" (rib_cubic_frames with the masks): a sample is clean iff all 16 of its taps are clear."""
        return self._mci_frames_body("mci_frames_masked", a_u8, b_u8, (ma, mb), field, sample_rate, k_first, count, normalised, out, border,
                                     precision, sampler, _staging)

    def mci_accel_field(self, prev, cur, next, precision="full", present=None):
        """The block acceleration field of B segments on the GPU (rib_accel_field; background.mci_accel_host is the definition and is
        bit-equal): cur int16 [B,Hb,Wb,2] (or [Hb,Wb,2]) the segments' block fields on this device (mci_field, mci_field_masked,
        mci_detail_field; mci_refine's with precision="half"), prev and next the fields of the segments before and after each, same
        shape, either None (no segment has one).  present: None, or B pairs (has_prev, has_next) - a uint8 [B,2] tensor on this device
        or a host sequence, uploaded - for a batch whose members differ; a neighbour that is absent for an item is not read there.
        -> int16 of cur's shape, in the fields' unit, for mci_frames_accel.  Two launches on the current stream."""
        from .background import PRECISIONS, check_precision
        half = PRECISIONS.index(check_precision(precision, "mci_accel_field"))
        if not torch.is_tensor(cur) or cur.dim() not in (3, 4) or min(cur.shape) < 1:
            raise ValueError("mci_accel_field: the field must be an int16 [B,Hb,Wb,2] or [Hb,Wb,2] tensor, got %s" % (tuple(getattr(cur, "shape", ())),))
        single = cur.dim() == 3
        B, Hb, Wb = (1,) + tuple(cur.shape[:2]) if single else tuple(cur.shape[:3])
        f = self._mci_field_arg(cur, B, 8 * Hb, 8 * Wb, "mci_accel_field")
        fp, fn = (None if g is None else self._mci_field_arg(g, B, 8 * Hb, 8 * Wb, "mci_accel_field", ("segments", "the neighbouring segment")) for g in (prev, next))
        if present is not None:
            if not torch.is_tensor(present):
                present = torch.tensor([[int(bool(v)) for v in pair] for pair in present], dtype=torch.uint8).reshape(-1, 2).to(self.device)
            if tuple(present.shape) != (B, 2) or present.dtype != torch.uint8 or present.device != self.device:
                raise ValueError("mci_accel_field: present must be %d pairs (has_prev, has_next): uint8 [%d, 2] on %s" % (B, B, self.device))
            present = present.contiguous()
        n = int(self._lib.rib_accel_workspace_bytes(self._h, B, Hb, Wb))
        if n == 0:
            raise ValueError("mci_accel_field: B=%d Hb=%d Wb=%d: 1 <= B <= 32767, Hb and Wb in 1..2048" % (B, Hb, Wb))
        with torch.cuda.device(self.device):
            ws = torch.empty(n, dtype=torch.uint8, device=self.device)      # (per call: it belongs to the stream the call is enqueued on)
            res = torch.empty_like(f)
            _native.check(self._h, self._lib.rib_accel_field(self._h, B, Hb, Wb, _ptr(fp), _ptr(f), _ptr(fn), _ptr(present), half, _ptr(res),
                                                             _ptr(ws), self._stream()))
        return res[0] if single else res

    def mci_frames_accel(self, a_u8, b_u8, field, accel, sample_rate, k_first=1, count=None, normalised=True, out=None, border="clamp",
                         precision="full", sampler="bilinear", masks=None):
        """mci_frames / mci_frames_masked on a second-order trajectory, one launch (rib_accel_frames; background.mci_frames_accel_host is
        the definition and is bit-equal): accel int16 [B,Hb,Wb,2] is mci_accel_field's result for the same segments, in `field`'s unit;
        both of a pixel's samples move by c = accel * t (1 - t) / 2 at t = k / sample_rate.  masks: None (the person is kept) or
        (ma, mb) as mci_frames_masked's.  Everything else - field, frames, normalised (True, False, "both"), out, border, precision,
        sampler - is mci_frames'; an all-zero accel gives its bytes."""
        if accel is None:
            raise ValueError("mci_frames_accel: accel must be an int16 tensor on %s (mci_accel_field)" % (self.device,))
        return self._mci_frames_body("mci_frames_accel", a_u8, b_u8, masks, field, sample_rate, k_first, count, normalised, out, border, precision,
                                     sampler, 0, accel=accel)

    def mci_frames_scaled(self, a0_u8, b0_u8, field, model_hw, sample_rate, k_first=0, count=None, border="clamp", precision="full", out=None,
                          sampler="bilinear", _staging=0):
        """mci_frames' uint8 frames at the key frames' OWN size, one launch (rib_scaled_frames; background.mci_frames_scaled_host
        is the definition and is bit-equal): a0_u8, b0_u8 uint8 [B,h0,w0,3] (or [h0,w0,3]) are the key frame files' pixels on
        this device, field the int16 [B,Hb,Wb,2] field of the MODEL-size key frames (mci_field, or mci_refine with
        precision="half"), model_hw = (H, W) that model size -> uint8 [T,B,h0,w0,3] ([T,h0,w0,3]), frames k_first ..
        k_first + count - 1 (count None: up to sample_rate - 1).  The field is read at the model's resolution, the pixels are
        sampled from the full-size key frames; with (h0, w0) == (H, W) the bytes are mci_frames'.  Sides in 1..16384, each axis
        within 1/16 .. 16 times the model's.  out: optional contiguous uint8 destination, any byte offset.  sampler="cubic":
        rib_cubic_scaled (background.sample_cubic in place of the bilinear sample); _staging is its diagnostic, as mci_frames'."""
        from .background import BORDERS, PRECISIONS, check_border, check_precision, check_sampler, log2_rate, scaled_factors
        border = BORDERS.index(check_border(border, "mci_frames_scaled"))
        cubic = check_sampler(sampler, "mci_frames_scaled") == "cubic"
        precision = PRECISIONS.index(check_precision(precision, "mci_frames_scaled"))
        a, b, single = self._mci_pair(a0_u8, b0_u8, "mci_frames_scaled")
        B, h0, w0, _ = a.shape
        H, W = (int(v) for v in model_hw)
        scaled_factors((H, W), (h0, w0), "mci_frames_scaled")
        log2_rate(sample_rate)
        s = int(sample_rate)
        f = self._mci_field_arg(field, B, H, W, "mci_frames_scaled", ("model frames", "mci_field"))
        k_first, T = self._mci_span(s, k_first, count, "mci_frames_scaled")
        shape = (T, B, h0, w0, 3)
        with torch.cuda.device(self.device):
            if out is None:
                res = torch.empty(shape, dtype=torch.uint8, device=self.device)
            else:
                res = out.unsqueeze(1) if (single and torch.is_tensor(out) and out.dim() == 4) else out
                if not torch.is_tensor(res) or tuple(res.shape) != shape or res.dtype != torch.uint8 or not res.is_contiguous() or res.device != self.device:
                    raise ValueError("mci_frames_scaled: out must be a contiguous uint8 %s tensor on %s" % (shape, self.device))
            if cubic:
                _native.check(self._h, self._lib.rib_cubic_scaled(self._h, T, B, H, W, h0, w0, _ptr(a), _ptr(b), _ptr(f), s, k_first, border,
                                                                  precision, int(_staging), _ptr(res), self._stream()))
            else:
                _native.check(self._h, self._lib.rib_scaled_frames(self._h, T, B, H, W, h0, w0, _ptr(a), _ptr(b), _ptr(f), s, k_first, border,
                                                                   precision, _ptr(res), self._stream()))
        return res[:, 0] if single else res

    def jpeg_max_bytes(self, height, width):
        """Upper bound of one JPEG file of a height x width image, header included (rib_jpeg_max_bytes; panel.jpeg_max_bytes)."""
        n = int(self._lib.rib_jpeg_max_bytes(int(height), int(width)))
        if n == 0:
            raise ValueError("jpeg: height and width must be in 1..65535, got %dx%d" % (height, width))
        return n

    def jpeg_into(self, sheets_u8, dst, lengths, quality=90, cap=None):
        """The lower-level form of jpeg(): encodes uint8 [T,SH,SW,3] on this device into the caller's buffers and only enqueues
        (two launches on the current stream, no synchronisation).  dst: a contiguous 1-D uint8 device tensor of at least
        T * cap bytes, any byte alignment - frame t's file starts at dst[t * cap]; lengths: a contiguous int32 [T] device
        tensor receiving each file's size.  cap (default dst.numel() // T) below jpeg_max_bytes(SH, SW) is allowed: a frame
        whose file would not fit writes nothing and gets length 0, which the caller has to check once the lengths are home.
        Bytes of a frame's cap behind its length are not written.  -> cap."""
        if not torch.is_tensor(sheets_u8) or sheets_u8.dim() != 4 or sheets_u8.shape[-1] != 3 or sheets_u8.dtype != torch.uint8 \
                or sheets_u8.device != self.device or not sheets_u8.is_contiguous():
            raise ValueError("jpeg: sheets must be a contiguous uint8 [T,SH,SW,3] tensor on %s" % (self.device,))
        T, SH, SW, _ = sheets_u8.shape
        if isinstance(quality, bool) or int(quality) != quality or not 1 <= int(quality) <= 100:
            raise ValueError("jpeg: quality must be an integer in 1..100, got %r" % (quality,))
        self.jpeg_max_bytes(SH, SW)
        if T < 1 or T > 65535:
            raise ValueError("jpeg: 1 <= T <= 65535 frames, got %d" % T)
        if dst.dim() != 1 or dst.dtype != torch.uint8 or dst.device != self.device or not dst.is_contiguous():
            raise ValueError("jpeg: dst must be a contiguous 1-D uint8 tensor on %s" % (self.device,))
        if tuple(lengths.shape) != (T,) or lengths.dtype != torch.int32 or lengths.device != self.device or not lengths.is_contiguous():
            raise ValueError("jpeg: lengths must be a contiguous int32 [%d] tensor on %s" % (T, self.device))
        cap = dst.numel() // T if cap is None else int(cap)
        from . import panel as P
        if cap < P.JPEG_HEADER_BYTES + 2 or cap >= 2 ** 31 or T * cap > dst.numel():
            raise ValueError("jpeg: cap=%d: at least the %d-byte header and EOI, below 2 GiB, and T * cap within dst (%d bytes)"
                             % (cap, P.JPEG_HEADER_BYTES, dst.numel()))
        n = int(self._lib.rib_jpeg_workspace_bytes(self._h, T, SH, SW))
        cache = self.__dict__.setdefault("_jpeg_ws", {})
        ws = cache.get((T, SH, SW))
        if ws is None:
            ws = cache[(T, SH, SW)] = torch.empty(n, dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            _native.check(self._h, self._lib.rib_jpeg(self._h, T, SH, SW, _ptr(sheets_u8), int(quality), _ptr(dst), cap, _ptr(lengths),
                                                      _ptr(ws), self._stream()))
        return cap

    def jpeg(self, sheets_u8, quality=90):
        """Baseline JPEG files of T images on the GPU (rib_jpeg, csrc/jpeg.hip.h; panel.jpeg_encode_host is the definition and is
        bit-equal): uint8 [T,SH,SW,3] on this device -> list of T bytes objects.  Every file has jpeg_max_bytes(SH, SW) of
        room, so none is refused; the lengths come home first, then exactly the files' bytes."""
        if not torch.is_tensor(sheets_u8) or sheets_u8.dim() != 4:
            raise ValueError("jpeg: sheets must be a uint8 [T,SH,SW,3] tensor")
        T, SH, SW, _ = sheets_u8.shape
        cap = self.jpeg_max_bytes(SH, SW)
        dst = torch.empty(T * cap, dtype=torch.uint8, device=self.device)
        lengths = torch.empty(T, dtype=torch.int32, device=self.device)
        self.jpeg_into(sheets_u8, dst, lengths, quality, cap)
        n = lengths.cpu().tolist()
        if not all(v > 0 for v in n):
            raise RuntimeError("jpeg: a frame exceeded rib_jpeg_max_bytes (%d bytes): the staging bound is wrong" % cap)
        return [dst[t * cap:t * cap + n[t]].cpu().numpy().tobytes() for t in range(T)]

    def png_max_bytes(self, height, width):
        """Upper bound of one PNG file of a height x width frame (rib_png_max_bytes; png.max_bytes)."""
        n = int(self._lib.rib_png_max_bytes(int(height), int(width)))
        if n == 0:
            raise ValueError("png: height must be in 1..65535 and width in 1..4096, got %dx%d" % (height, width))
        return n

    def png_into(self, frames_u8, dst, lengths, cap=None, tables=None):
        """The lower-level form of png(): encodes uint8 [T,H,W,3] on this device into the caller's buffers and only enqueues (two
        launches on the current stream, no synchronisation).  dst: a contiguous 1-D uint8 device tensor of at least T * cap
        bytes, any byte alignment - frame t's file starts at dst[t * cap]; lengths: a contiguous int32 [T] device tensor
        receiving each file's size.  cap (default dst.numel() // T) below png_max_bytes(H, W) is allowed: a frame whose file
        would not fit writes nothing and gets length 0, which the caller has to check once the lengths are home.  Bytes of a
        frame's cap behind its length are not written.  tables: uint8 [K, 286] code lengths, by default png.TABLES (the library
        validates them and keeps their device copy on the handle).  -> cap."""
        if not torch.is_tensor(frames_u8) or frames_u8.dim() != 4 or frames_u8.shape[-1] != 3 or frames_u8.dtype != torch.uint8 \
                or frames_u8.device != self.device or not frames_u8.is_contiguous():
            raise ValueError("png: frames must be a contiguous uint8 [T,H,W,3] tensor on %s" % (self.device,))
        T, H, W, _ = frames_u8.shape
        self.png_max_bytes(H, W)
        if T < 1 or T > 65535:
            raise ValueError("png: 1 <= T <= 65535 frames, got %d" % T)
        if dst.dim() != 1 or dst.dtype != torch.uint8 or dst.device != self.device or not dst.is_contiguous():
            raise ValueError("png: dst must be a contiguous 1-D uint8 tensor on %s" % (self.device,))
        if tuple(lengths.shape) != (T,) or lengths.dtype != torch.int32 or lengths.device != self.device or not lengths.is_contiguous():
            raise ValueError("png: lengths must be a contiguous int32 [%d] tensor on %s" % (T, self.device))
        cap = dst.numel() // T if cap is None else int(cap)
        if cap < 1 or cap >= 2 ** 31 or T * cap > dst.numel():
            raise ValueError("png: cap=%d: at least 1, below 2 GiB, and T * cap within dst (%d bytes)" % (cap, dst.numel()))
        if tables is None:
            from . import png as _png
            tables = _png.TABLES
        tables = np.ascontiguousarray(tables)
        if tables.dtype != np.uint8 or tables.ndim != 2 or tables.shape[1] != 286:
            raise ValueError("png: tables must be a uint8 [K, 286] array")
        n = int(self._lib.rib_png_workspace_bytes(self._h, T, H, W))
        cache = self.__dict__.setdefault("_png_ws", {})
        ws = cache.get((T, H, W))
        if ws is None:
            ws = cache[(T, H, W)] = torch.empty(n, dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            _native.check(self._h, self._lib.rib_png(self._h, T, H, W, _ptr(frames_u8), tables.ctypes.data, int(tables.shape[0]), _ptr(dst),
                                                     cap, _ptr(lengths), _ptr(ws), self._stream()))
        return cap

    def png(self, frames_u8, tables=None):
        """Lossless PNG files of T frames on the GPU (rib_png, csrc/png.hip.h; png.encode_host is the definition and is bit-equal):
        uint8 [T,H,W,3] on this device -> list of T bytes objects.  Every file has png_max_bytes(H, W) of room, so none is
        refused; the lengths come home first, then exactly the files' bytes."""
        if not torch.is_tensor(frames_u8) or frames_u8.dim() != 4:
            raise ValueError("png: frames must be a uint8 [T,H,W,3] tensor")
        T, H, W, _ = frames_u8.shape
        cap = self.png_max_bytes(H, W)
        dst = torch.empty(T * cap, dtype=torch.uint8, device=self.device)
        lengths = torch.empty(T, dtype=torch.int32, device=self.device)
        self.png_into(frames_u8, dst, lengths, cap, tables)
        n = lengths.cpu().tolist()
        if not all(v > 0 for v in n):
            raise RuntimeError("png: a frame exceeded rib_png_max_bytes (%d bytes): the bound is wrong" % cap)
        return [dst[t * cap:t * cap + n[t]].cpu().numpy().tobytes() for t in range(T)]

    def jpeg_f32_into(self, frames, dst, lengths, quality=90, cap=None):
        """jpeg_into() for the frames the chain produces (rib_jpeg_float): float32 [T,3,H,W] in [-1, 1], contiguous, on this device
        - the files of jpeg_into(quantise(frames), ...) without the uint8 copy in between.  dst, lengths, cap, the refusal of a
        frame that does not fit and the return value are jpeg_into's."""
        if not torch.is_tensor(frames) or frames.dim() != 4 or frames.shape[1] != 3 or frames.dtype != torch.float32 \
                or frames.device != self.device or not frames.is_contiguous():
            raise ValueError("jpeg_f32: frames must be a contiguous float32 [T,3,H,W] tensor on %s" % (self.device,))
        T, _, H, W = frames.shape
        if isinstance(quality, bool) or int(quality) != quality or not 1 <= int(quality) <= 100:
            raise ValueError("jpeg_f32: quality must be an integer in 1..100, got %r" % (quality,))
        self.jpeg_max_bytes(H, W)
        if T < 1 or T > 65535:
            raise ValueError("jpeg_f32: 1 <= T <= 65535 frames, got %d" % T)
        if dst.dim() != 1 or dst.dtype != torch.uint8 or dst.device != self.device or not dst.is_contiguous():
            raise ValueError("jpeg_f32: dst must be a contiguous 1-D uint8 tensor on %s" % (self.device,))
        if tuple(lengths.shape) != (T,) or lengths.dtype != torch.int32 or lengths.device != self.device or not lengths.is_contiguous():
            raise ValueError("jpeg_f32: lengths must be a contiguous int32 [%d] tensor on %s" % (T, self.device))
        cap = dst.numel() // T if cap is None else int(cap)
        from . import panel as P
        if cap < P.JPEG_HEADER_BYTES + 2 or cap >= 2 ** 31 or T * cap > dst.numel():
            raise ValueError("jpeg_f32: cap=%d: at least the %d-byte header and EOI, below 2 GiB, and T * cap within dst (%d bytes)"
                             % (cap, P.JPEG_HEADER_BYTES, dst.numel()))
        n = int(self._lib.rib_jpeg_workspace_bytes(self._h, T, H, W))
        cache = self.__dict__.setdefault("_jpeg_ws", {})         # shared with jpeg_into: the workspace of a shape is the same
        ws = cache.get((T, H, W))
        if ws is None:
            ws = cache[(T, H, W)] = torch.empty(n, dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            _native.check(self._h, self._lib.rib_jpeg_float(self._h, T, H, W, _ptr(frames), int(quality), _ptr(dst), cap, _ptr(lengths),
                                                          _ptr(ws), self._stream()))
        return cap

    def jpeg_f32(self, frames, quality=90):
        """Baseline JPEG files of T float frames on the GPU (rib_jpeg_float): float32 [T,3,H,W] in [-1, 1] on this device -> list of
        T bytes objects, panel.jpeg_encode_host(panel.quantise_host(frames)) byte for byte (= jpeg(quantise(frames)))."""
        if not torch.is_tensor(frames) or frames.dim() != 4:
            raise ValueError("jpeg_f32: frames must be a float32 [T,3,H,W] tensor")
        T, _, H, W = frames.shape
        cap = self.jpeg_max_bytes(H, W)
        dst = torch.empty(T * cap, dtype=torch.uint8, device=self.device)
        lengths = torch.empty(T, dtype=torch.int32, device=self.device)
        self.jpeg_f32_into(frames, dst, lengths, quality, cap)
        n = lengths.cpu().tolist()
        if not all(v > 0 for v in n):
            raise RuntimeError("jpeg_f32: a frame exceeded rib_jpeg_max_bytes (%d bytes): the staging bound is wrong" % cap)
        return [dst[t * cap:t * cap + n[t]].cpu().numpy().tobytes() for t in range(T)]

    # ---- introspection / measurement -----------------------------------------------------------
    def enable_taps(self, on=True):
        """Debug: keep every tapped intermediate intact until the end of a forward (buffers with disjoint lifetimes
        share workspace bytes otherwise).  Rebuilds the launch plans; call before the forward whose taps are read."""
        _native.check(self._h, self._lib.rib_set_debug_taps(self._h, 1 if on else 0))
        self._ws.clear()
        return self

    def read_taps(self, B, H, W):
        """Intermediate activations of the LAST forward at this shape (run after enable_taps()), as NCHW CPU tensors."""
        ws = self._workspace(B, H, W)
        out = {}
        name = C.c_char_p(); ch = C.c_int(); th = C.c_int(); tw = C.c_int()
        for i in range(self._lib.rib_num_taps(self._h, B, H, W)):
            _native.check(self._h, self._lib.rib_tap_info(self._h, B, H, W, i, C.byref(name), C.byref(ch), C.byref(th), C.byref(tw)))
            dst = torch.empty((B, ch.value, th.value, tw.value), dtype=torch.float32, device=self.device)
            _native.check(self._h, self._lib.rib_read_tap(self._h, B, H, W, i, _ptr(ws), _ptr(dst), self._stream()))
            out[name.value.decode()] = dst.cpu()
        return out

    def profile_begin(self, kernels=False):
        """kernels=False: one event in front of every launch (the classes add up to the profiled step, event cost included);
        kernels=True: a (start, stop) pair bound to every dispatch - the kernels' own execution times, as rocprofv3 reports them."""
        _native.check(self._h, (self._lib.rib_profile_begin_kernels if kernels else self._lib.rib_profile_begin)(self._h))

    def profile_collect(self):
        n = len(_native.KC_NAMES)
        launches = (C.c_int64 * n)(); ms = (C.c_double * n)()
        _native.check(self._h, self._lib.rib_profile_collect(self._h, launches, ms))
        return {k: {"launches": int(launches[i]), "ms": float(ms[i])} for i, k in enumerate(_native.KC_NAMES)}

    def forward_flops(self, B, H, W):
        n = len(_native.KC_NAMES)
        fl = (C.c_double * n)()
        _native.check(self._h, self._lib.rib_forward_flops(self._h, B, H, W, fl))
        return {k: float(fl[i]) for i, k in enumerate(_native.KC_NAMES)}

    def tuned_ops(self, B, H, W):
        """How many launches of this shape run a measured choice (0: the analytic cost model decides everything)."""
        self._workspace(B, H, W)
        return self._tuned.get((B, H, W), 0)

    def num_launches(self, B, H, W):
        return self._lib.rib_num_launches(self._h, B, H, W)

    def launch_info(self, B, H, W):
        """The launch plan of a shape: [{name, class (index into _native.KC_NAMES), grid, tile, flops}]."""
        self._workspace(B, H, W)                       # pins the tuned choices of this shape first
        buf = C.create_string_buffer(512)
        out = []
        for i in range(self._lib.rib_num_launches(self._h, B, H, W)):
            _native.check(self._h, self._lib.rib_debug_launch_info(self._h, B, H, W, i, buf, 512))
            name, kclass, grid, tile, flops, nbytes = buf.value.decode().split("|")
            out.append({"name": name, "class": int(kclass), "grid": grid, "tile": tile, "flops": float(flops), "bytes": float(nbytes)})
        return out
