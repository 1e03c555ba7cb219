/*
 * rib.h — C ABI of the MI355X-native pose-guided generator ("Render-In-Between" hot path).
 *
 * The reference (azuxmioy/Render-In-Between) is pure Python and has no FFI layer: its boundary for
 * this path is the Python object protocol between the sequence driver and the generator module
 * (Pose_Guided_Neural_Rendering, abbreviated PGNR below).  Every entry point cites the reference
 * interface it replaces.  All functions return 0 on success or a negative rib_status; no C++
 * exception crosses this boundary.  rib_last_error() gives the message of the last failure.
 *
 * Ownership: the caller owns every tensor and the workspace; a handle owns only the weight blob
 * and its launch plans.  A handle is bound to one device, is single-stream and not re-entrant
 * (one handle per GPU / process).  Every launch of an entry point is enqueued, in order, on the caller's
 * stream; the handle owns no streams or events.
 * Synchronisation: rib_finalize_weights(), rib_read_tap() and rib_profile_collect() synchronise; rib_import_weights()
 * waits for its stream once (it reads the blob's 64-byte header back before accepting it); and the FIRST call that
 * needs the launch plan of a new (B,H,W) - rib_workspace_bytes / rib_forward / rib_chain / the introspection calls -
 * may allocate device memory for Winograd-domain filter sets and synchronise the device while it computes them
 * (one-time work per shape; query rib_workspace_bytes() up front to keep it out of a timed or captured region).
 * Steady-state calls of every other entry point only enqueue.
 *
 * Tensors at the boundary are dense fp32 NCHW on the handle's device, exactly what the reference
 * generator takes and returns (PGNR/models/evaluator.py:250-255).
 */
#ifndef RIB_H
#define RIB_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rib_handle rib_handle;

typedef enum {
  RIB_OK = 0,
  RIB_ERR_INVALID = -1,      /* bad argument / unsupported shape */
  RIB_ERR_UNSUPPORTED = -2,  /* generator variant the path does not implement */
  RIB_ERR_STATE = -3,        /* e.g. forward before weights are loaded */
  RIB_ERR_MISSING = -4,      /* a required checkpoint tensor was never set */
  RIB_ERR_HIP = -5,          /* a HIP runtime call failed */
  RIB_ERR_WORKSPACE = -6     /* workspace too small */
} rib_status;

/* Resolved hyper-parameters of Generator(gen_cfg): the keys PGNR/models/generator.py:46-65,
 * 317-324, 431-440 reads from configs/HSM.yaml:35-67 (after getattr defaults). */
typedef struct {
  int32_t label_nc;          /* gen.input_label_nc   (22) */
  int32_t image_nc;          /* gen.input_image_nc   (3)  */
  int32_t num_filters;       /* gen.num_filters      (16) */
  int32_t max_num_filters;   /* gen.max_num_filters  (512) */
  int32_t num_layers;        /* gen.num_layers       (6)  */
  int32_t num_down_img;      /* gen.num_downsamples_img, default 4 (generator.py:50) */
  int32_t emb_filters;       /* gen.embed.num_filters      (64)  */
  int32_t emb_max_filters;   /* gen.embed.max_num_filters  (512) */
  int32_t emb_down;          /* gen.embed.num_downsamples  (4)   */
  int32_t mask_filters;      /* gen.mask.num_filters       (32)  */
  int32_t mask_max_filters;  /* gen.mask.max_num_filters   (512) */
  int32_t mask_down;         /* gen.mask.num_downsamples   (3)   */
  int32_t mask_res_blocks;   /* gen.mask.num_res_blocks    (4)   */
} rib_config;

/* ---- construction: replaces Generator(cfg.gen).to(device) (PGNR/models/trainer.py:61) ---- */
int rib_create(const rib_config* cfg, int device, rib_handle** out);
void rib_destroy(rib_handle* h);
/* h may be NULL: message of the last failed rib_create on this thread. */
const char* rib_last_error(const rib_handle* h);

/* ---- weights: replaces load_state_dict(net_G, path) (PGNR/utils/utils.py:107-119) ----
 * The handle speaks the reference checkpoint's vocabulary: the caller hands over the raw
 * state-dict tensors by their reference names ('down_0.conv_block_0.layers.conv.weight_orig',
 * '...weight_u', '...layers.norm.mlps.0.0.layers.conv.weight', ...).  rib_finalize_weights()
 * folds the eval-mode spectral norm  W = W_orig / (u . W_mat v)  (hook of
 * PGNR/models/layers/weight_norm.py:84-85), re-lays the filters out for the kernels and uploads
 * one contiguous device blob.  Tensors of modules the forward never calls (label_embedding.*,
 * conv_mask.*) are accepted and ignored; unknown names are an error (strict load). */
int rib_num_tensors(const rib_handle* h);
int rib_tensor_info(const rib_handle* h, int idx, const char** name, int* ndim, int64_t dims[4],
                    int* used);
int rib_set_tensor(rib_handle* h, const char* name, const float* host_data, int ndim,
                   const int64_t* dims);
int rib_finalize_weights(rib_handle* h);
/* The folded device blob, for the one RCCL broadcast of the multi-GPU path: rank 0 finalizes and
 * exports the blob into a caller-owned device buffer, the caller broadcasts that buffer
 * (torch.distributed / RCCL over xGMI), every other rank imports it.  Both copies are
 * device-to-device and asynchronous on the given stream. */
size_t rib_weights_bytes(const rib_handle* h);
int rib_export_weights(rib_handle* h, void* dst_device, size_t bytes, void* hip_stream);
int rib_import_weights(rib_handle* h, const void* src_device, size_t bytes, void* hip_stream);

/* ---- storage type and arithmetic of the matrix-core contractions (no reference counterpart: the reference is
 * fp32 only; PGNR/models/trainer.py:51 builds a plain fp32 module).
 *   RIB_DTYPE_F32 (default)  fp32 activations and filters, exact-fp32 MFMA (v_mfma_f32_32x32x2_f32): the mode every
 *                            parity claim and the bench headline are made in.
 *   RIB_DTYPE_BF16           BASELINE.json configs[2]: bf16 NHWC activations and bf16 filters in HBM and LDS, bf16
 *                            MFMA operands (v_mfma_f32_32x32x16_bf16), fp32 accumulation, fp32 InstanceNorm statistics
 *                            and SPADE arithmetic; the caller's tensors stay fp32 NCHW.
 *   RIB_DTYPE_F16            the same 16-bit storage layouts and kernels with IEEE half elements
 *                            (v_mfma_f32_32x32x16_f16): 11 significant bits instead of 8 at the same speed.  The bf16
 *                            mode's deviation from fp32 (1e-1 max / 8e-3 mean on a [-1,1] frame) is the format's, not the
 *                            kernels' (DESIGN 6); half brings it to ~1e-2 / 1e-3, and the network's activations and
 *                            filters sit well inside half's range (finite outputs are asserted by the tests).
 * The mode decides the weight-blob layout (16-bit filter copies are appended): set it before
 * rib_finalize_weights / rib_import_weights (a handle that still holds the state-dict tensors re-folds by itself;
 * tuned choices pinned with rib_set_choice are dropped, they name kernels of the other mode).  Blobs are
 * exchangeable only between handles of the same mode and layout: the blob starts with a 64-byte header (magic,
 * mode, size, a hash of the layout offsets) that rib_import_weights checks. ---- */
enum { RIB_DTYPE_F32 = 0, RIB_DTYPE_BF16 = 1, RIB_DTYPE_F16 = 3 };   /* (2 was round 2's retired split-bf16 mode) */
int rib_set_compute_dtype(rib_handle* h, int dtype);

/* ---- arithmetic of the GEMM-shaped launches in RIB_DTYPE_F32 mode (no reference counterpart; OPT-IN, round 6).
 *   RIB_PRODUCTS_F32 (default)  exact-fp32 matrix-core products everywhere: the reference's arithmetic, the mode every parity
 *                               claim and the bench headline are made in.
 *   RIB_PRODUCTS_BF16X3         the plain GEMMs of the frame (k_gemm_dma: the Winograd-domain GEMMs of the deep 3x3 layers and the
 *                               gamma/beta GEMM of a condition level) split every fp32 operand value into three bf16 numbers
 *                               (hi + mid + lo, exact) in registers and form a product from six bf16 matrix-core products
 *                               accumulated in fp32 (dropped cross terms < 2^-24 |a b|).  Storage, layouts, the weight blob
 *                               and every other kernel are unchanged.  Against an fp64 GEMM it is no less accurate than the
 *                               exact-fp32 MFMA chain (rms error 0.4-0.9x: fewer roundings of the running sum), but it is
 *                               not the reference's arithmetic: results differ from the default's by fp32 rounding noise.
 * Takes effect at the next launch (plans and tuned choices are shared between the two); ignored by the 16-bit modes. ---- */
enum { RIB_PRODUCTS_F32 = 0, RIB_PRODUCTS_BF16X3 = 1 };
int rib_set_products(rib_handle* h, int products);

/* ---- forward: replaces  img, mask = net_G(label, label_prev, img_fake, img_prev)
 *      (PGNR/models/generator.py:181-234; call site PGNR/models/evaluator.py:255) ----
 * label [B,label_nc,H,W], img_fake/img_prev [B,image_nc,H,W] -> img [B,image_nc,H,W] (tanh),
 * mask [B,1,H,W] (sigmoid).  label_prev is dead in the reference and has no
 * parameter.  H and W must be multiples of 2^max(num_down_img, mask_down). */
size_t rib_workspace_bytes(rib_handle* h, int B, int H, int W);
int rib_forward(rib_handle* h, int B, int H, int W, const float* label, const float* img_fake,
                const float* img_prev, float* img, float* mask, void* workspace,
                size_t workspace_bytes, void* hip_stream);
/* The same forward with the driver's blend fused in: fuse = img*mask + img_fake*(1-mask), mask broadcast over the
 * image channels (PGNR/models/evaluator.py:256-258), written by the kernel that computes the mask.  fuse [B,3,H,W]
 * fp32 NCHW device memory; may be null (then this IS rib_forward). */
int rib_forward_blend(rib_handle* h, int B, int H, int W, const float* label, const float* img_fake,
                      const float* img_prev, float* img, float* mask, float* fuse,
                      void* workspace, size_t workspace_bytes, void* hip_stream);

/* ---- autoregressive segment: replaces the inference loop body of
 *      Evaluator.evaluate_from_folder (PGNR/models/evaluator.py:238-262) ----
 * prev <- key_frame; for t in 0..T-1:
 *   img_t, mask_t = G(labels[t], ., dains[t], prev); fuse_t = img_t*mask_t + dains[t]*(1-mask_t);
 *   prev <- fuse_t.
 * labels [T,B,label_nc,H,W], dains [T,B,image_nc,H,W], key_frame [B,image_nc,H,W];
 * outputs imgs/fuses [T,B,image_nc,H,W], masks [T,B,1,H,W]; imgs and masks may be NULL. */
/* Workspace for a T-frame rib_chain: rib_workspace_bytes plus room for the label-only launches of the whole
 * segment at batch T*B (they run once per chain instead of once per frame).  A caller that passes only
 * rib_workspace_bytes still gets a correct chain with per-frame label work. */
size_t rib_chain_workspace_bytes(rib_handle* h, int T, int B, int H, int W);
int rib_chain(rib_handle* h, int T, int B, int H, int W, const float* key_frame,
              const float* labels, const float* dains, float* imgs, float* masks, float* fuses,
              void* workspace, size_t workspace_bytes, void* hip_stream);

/* fuse = img*mask + dain*(1-mask) (PGNR/models/evaluator.py:256-258); n = B*H*W pixels. */
int rib_blend(rib_handle* h, int B, int C, int H, int W, const float* img, const float* mask,
              const float* dain, float* fuse, void* hip_stream);
/* uint8 HWC frame = uint8(clip(x*0.5+0.5,0,1)*255), truncating (PGNR/utils/utils.py:129-142). */
int rib_quantise(rib_handle* h, int B, int C, int H, int W, const float* img_nchw,
                 uint8_t* out_nhwc, void* hip_stream);
/* ---- quality metrics against ground truth (PGNR/models/evaluator.py:149-163, piq defaults; restated from piq, unpinned) ----
 * Masked PSNR / SSIM of B frames: pred, target NCHW fp32 in [-1,1] (C = 3); mask [B,H,W] in [0,1] or NULL.
 * x = clamp(pred*0.5+0.5, 0, 1)*mask (likewise y); psnr[b] = -10 log10(mean (x-y)^2 + 1e-8) at full resolution;
 * ssim[b] = mean of the 11x11 gaussian (sigma 1.5, valid) SSIM map after f x f average pooling, f = max(1, round(min(H,W)/256)).
 * Per-frame results on the device; the pooled side must be at least 11 (RIB_ERR_INVALID otherwise, as piq raises).
 * Deterministic: no atomics, a frame's values do not depend on B.  The workspace is sized for C = 3; 0 = invalid shape. */
size_t rib_quality_workspace_bytes(rib_handle* h, int B, int H, int W);
int rib_quality(rib_handle* h, int B, int C, int H, int W, const float* pred, const float* target,
                const float* mask, float* psnr, float* ssim, void* workspace, size_t workspace_bytes, void* hip_stream);
/* ---- frame resize of the folder driver (PGNR/models/evaluator.py:18-26,219-221) ----
 * The reference resizes every frame to the model size with A.Resize(interpolation=cv2.INTER_CUBIC) on the host.  This is
 * OpenCV's 8-bit INTER_CUBIC as resize.py restates it, for N frames of one source size: src uint8 NHWC [N,H0,W0,3] (C = 3
 * is part of the entry) -> H x W.  ix, cx [W,4] and iy, cy [H,4] int32 device arrays: the clamped tap indices and the
 * 11-bit fixed-point coefficients of each output column / row, made on the host (resize._cubic_taps; the float32 weight
 * arithmetic is not restated on the device).  v = sum_j cy[j] * (sum_i cx[i] * src[iy[j]][ix[i]]) in int32, then
 * (v + 2^21) >> 22 saturated to 0..255: integer only, so bit-exact to the host function whatever the summation order.
 * Outputs, either may be NULL but not both: out_u8_nhwc [N,H,W,3] uint8, and out_f32_nchw [N,3,H,W] fp32 holding
 * ToTensor + Normalize(0.5, 0.5) of it, (u8 / 255 - 0.5) / 0.5, bit-identical to that expression evaluated by torch on
 * the device (a division by a host scalar is a multiplication by its fp32 reciprocal there).  H0 == H and W0 == W is
 * allowed (a copy / the normalisation alone).  Indices outside the source are clamped.  One launch, no workspace, no
 * atomics: a frame's bytes do not depend on N.  Sizes < 1, N > 65535, a NULL input or both outputs NULL: RIB_ERR_INVALID. */
int rib_resize_cubic(rib_handle* h, int N, int H0, int W0, int H, int W, const uint8_t* src_u8_nhwc,
                        const int32_t* ix, const int32_t* cx, const int32_t* iy, const int32_t* cy,
                        uint8_t* out_u8_nhwc, float* out_f32_nchw, void* hip_stream);
/* ---- the frame at the source resolution (this project's addition: the reference writes its frames at the model size) ----
 * The fuse of N frames at the SOURCE size H0 x W0, from the model-size prediction and blend mask and the source-size
 * background: pred fp32 NCHW [N,3,H,W] in [-1,1], mask fp32 [N,1,H,W] in [0,1] (finite, as for rib_quantise), bg uint8 NHWC
 * [N,H0,W0,3] -> out uint8 NHWC [N,H0,W0,3].  composite.py (composite_host) states the result in integers and the kernel is
 * bit-equal to it: P = uint8(clip(pred*0.5+0.5, 0, 1)*255) (rib_quantise's arithmetic), M = uint8(clip(mask, 0, 1)*255), both
 * in double and truncating; Pu, Mu = rib_resize_cubic's resize of P and M from H x W to H0 x W0 (a mask overshoot saturates);
 * out = (Pu*Mu + bg*(255 - Mu) + 127) / 255 in int32 per channel.  M = 0 keeps the background's bytes, M = 255 gives Pu.
 * ix, cx [W0,4] and iy, cy [H0,4] int32 device arrays: the tap tables of resize._cubic_taps(W0, W) and (H0, H), made on the
 * host as for rib_resize_cubic (the float32 weight arithmetic is not restated on the device); indices outside the input are
 * clamped.  Every size pair is allowed: enlargement, H0 == H and W0 == W (no resampling: the taps are the identity) and
 * reduction on either axis (strong reductions take a slower path of the same kernel).  pred and mask 4-byte aligned; bg and
 * out at any byte alignment.  out == bg (in place) is allowed: a pixel reads no background byte but its own; any other
 * overlap is not.  One launch, no workspace, no atomics, integer arithmetic only after the two quantisers: a frame's bytes
 * do not depend on N.  Sizes < 1, N outside 1..65535, a frame of 2 GiB or more, a NULL pointer: RIB_ERR_INVALID with a
 * rib_last_error text, and nothing is launched. */
int rib_composite(rib_handle* h, int N, int H, int W, int H0, int W0,
                  const float* pred_f32_nchw, const float* mask_f32_n1hw, const uint8_t* bg_u8_nhwc,
                  const int32_t* ix, const int32_t* cx, const int32_t* iy, const int32_t* cy,
                  uint8_t* out_u8_nhwc, void* hip_stream);
/* ---- label-map rasterisation --------------------------------------------------
 * Replaces, per frame, Dataset._generate_skeleton + _generate_pose_map
 * (PGNR/datasets/HSM_auto_dataset.py:205-251; drawing rules PGNR/utils/keypoint2img.py:36-88,132-147)
 * as called from the inference pre-load loop (PGNR/models/evaluator.py:221-229,250): writes the
 * 22-channel label [3-ch limb drawing in [-1,1] | n_maps gaussian joint maps in [0,1]] of T frames
 * straight into device memory.  The host keeps what is file parsing and scalar work: reading the
 * OpenPose json, thresholding the joints and fitting one line per limb (interpPoints,
 * keypoint2img.py:66-88); the pixels are produced here, bit-identical to the reference.
 *
 * rib_stroke: one limb of one frame.  n = int(x1 - x0) samples of np.linspace(int(x0), int(x1), n)
 * (sample k = k*step + start, the last one = stop), each mapped through a*x + b; swap = 1 when the
 * line was fitted with the roles of x and y exchanged.  n = 0: limb not drawn.
 * peaks: (x, y) = (int(x), int(y)) of each joint's one-hot, x = -1 when the joint is off.
 * weights: the radius+1 half of scipy's normalised gaussian kernel (weights[d] = tap +-d).
 * All four tables are HOST pointers (a few KB per frame): they are copied into page-locked staging memory of the handle
 * before the call returns and go to the workspace in one asynchronous copy on `stream` - the call only enqueues. */
typedef struct rib_stroke {
  int32_t n, swap;
  double start, step, stop, a, b;
} rib_stroke;
size_t rib_rasterise_workspace_bytes(rib_handle* h, int T, int H, int W, int n_edges, int n_maps, int radius);
int rib_rasterise(rib_handle* h, int T, int H, int W,
                  const rib_stroke* strokes, int n_edges, const uint8_t* colors_rgb, int stroke_halfwidth,
                  const int32_t* peaks, int n_maps, const double* weights, int radius,
                  float* labels, void* workspace, size_t workspace_bytes, void* hip_stream);
/* ---- pose mask of the ground-truth metrics ----
 * The reference measures PSNR / SSIM under the human-centric mask that _generate_human_mask draws from the frame's own
 * keypoints (PGNR/datasets/HSM_auto_dataset.py:254-334, used at :390; PGNR/models/evaluator.py:118,122): cv2.circle, filled,
 * on every valid joint (radius 30 on joint 0, 15 elsewhere) and cv2.line on every limb whose two joints are valid
 * (thickness t = 30 for head / arms / legs, 40 for the three body lines; head (0,1), hand (1,2)(2,3)(3,4)(1,5)(5,6)(6,7),
 * legs (8,9)(9,10)(10,11)(8,12)(12,13)(13,14), body (1,8)(2,9)(5,12), and for 19 joints also (4,18)(7,17)(11,16)(14,15)).
 * Restated from OpenCV's drawing, unpinned (cv2 is not in this image); the definition is an exact integer one with OpenCV's
 * structure.  Pixel (px, py) of frame t is 1.0 iff one of these holds, else 0.0:
 *   disc   (px-Px)^2 + (py-Py)^2 <= R*R + R  for a valid joint P (R = 30 / 15) or an end point of a drawn limb (R = t/2);
 *   slab   for a drawn limb A -> B with A != B, d = B-A, L2 = d.d, v = (px,py)-A, h = t/2:
 *          0 <= v.d <= L2  and  4 (vx*dy - vy*dx)^2 <= (2h+1)^2 * L2
 * i.e. the pixel centre lies within R + 1/2 of the point / within h + 1/2 of the segment: OpenCV sets the pixels on the ideal
 * outline.  rasterise.human_mask is the same statement on the host, bit for bit (integers only, no floating point).
 * peaks: HOST pointer [T][n_joints][2], the convention of the rasteriser's peaks ((x, y), x = -1: joint off); it is copied
 * to page-locked staging memory of the handle before the call returns and sent on `stream`: the call only enqueues.
 * mask [T,H,W] fp32 on the device, every element written; it is what the quality entry takes as its mask.  One launch, no
 * atomics, no workspace: a frame's bytes do not depend on T.  n_joints other than 18 / 19, T < 1 (or > 65535), H or W
 * outside 1..16384, a peak outside the frame, NULL pointers: RIB_ERR_INVALID with a rib_last_error text. */
int rib_human_mask(rib_handle* h, int T, int H, int W, const int32_t* peaks, int n_joints,
                   float* mask /* [T,H,W] device */, void* hip_stream);
/* ---- six-pane diagnostic sheet of the folder driver (PGNR/models/evaluator.py:260-269, utils/visualize.py make_video) ----
 * T sheets in one launch: row 0 Predict | Mask | Fuse, row 1 DAIN | Ground Truth | Skeleton, each pane H x W, 8 px of white
 * (255) around and between the panes and a 24 px title bar over each pane row: out uint8 [T,SH,SW,3] with
 * SH = 2 (H + 24) + 3 * 8, SW = 3 W + 4 * 8, every byte written by the launch (nothing has to be cleared).  The layout and
 * the titles are this project's, not matplotlib's; panel.py (layout, compose_host) states the sheet on the host, bit-equal.
 * Inputs fp32 NCHW on the device: pred, fuse, dain, gt [T,3,H,W], mask [T,1,H,W], label [T,label_nc,H,W] (channels 0..2 are
 * the skeleton image; label_nc >= 3).  A 3-channel pane holds uint8(clip(x*0.5+0.5,0,1)*255) - the arithmetic of
 * rib_quantise, evaluated by the same device function; the Mask pane uint8(double(m)*255.0), truncating, no clip (m in
 * [0,1]), on all three channels (tensor2images, PGNR/utils/utils.py:122-147).
 * pred, mask and fuse may be NULL together: key-frame mode, Predict = Fuse = gt and Mask = 0 (evaluator.py:240-244).
 * titles: uint8 0/1 [2,24,SW] on the device or NULL; a set pixel of title bar r is drawn (0,0,255).
 * Enqueues one launch on `stream`, no synchronisation, no workspace, no atomics: a sheet's bytes do not depend on T.
 * T outside 1..65535, H outside 1..16384, W outside 1..4096, label_nc < 3, a sheet of 2 GiB or more, a NULL dain / gt / label /
 * out, or only some of pred / mask / fuse NULL: RIB_ERR_INVALID with a rib_last_error text, nothing launched. */
int rib_panel(rib_handle* h, int T, int H, int W, int label_nc, const float* pred, const float* mask, const float* fuse,
              const float* dain, const float* gt, const float* label, const uint8_t* titles, uint8_t* out, void* hip_stream);
/* ---- baseline JPEG of the diagnostic sheets, encoded on the GPU (the video frames of evaluate_from_folder(panels=True)) ----
 * T images uint8 NHWC [T,H,W,3] on the device -> T complete JFIF files: baseline sequential DCT (SOF0), 8 bit, Y Cb Cr 4:2:0
 * (MCU 16 x 16: Y00 Y01 Y10 Y11 Cb Cr), one interleaved scan, the Annex K quantisation tables of ITU-T T.81 under the IJG
 * quality scaling (quality 1..100) and the four Annex K Huffman tables - the tables PIL writes by default - with a restart
 * interval of one MCU row (DRI = ceil(W/16); RST0..7 cycle), which is what makes the encoder parallel.  Sizes that are no
 * multiple of 16 repeat the last column and row.  The stream is this project's, restated from T.81, unpinned: panel.py
 * (jpeg_encode_host) states every byte in integer arithmetic - fixed-point colour conversion, a 13-bit integer DCT with a
 * rounding shift per pass, division to the nearest with halves away from zero - and the kernels are bit-equal to it.
 * Frame t's file starts at dst + t * dst_stride and lengths[t] (device, int32) receives its size.  rib_jpeg_max_bytes(H, W)
 * is an upper bound of one file, header included (a block codes at most 64 symbols of at most 16 + 11 bits, every byte may be
 * stuffed); with dst_stride >= rib_jpeg_max_bytes no frame is refused.  A smaller dst_stride (at least the 629-byte header
 * and EOI) is allowed: a frame whose file would not fit writes nothing and gets lengths[t] = 0 - the call only enqueues and
 * returns RIB_OK, the caller reads the refusal from lengths.  Bytes of a frame's stride behind lengths[t] are not written.
 * workspace: rib_jpeg_workspace_bytes(h, T, H, W) bytes on the device, 16-byte aligned (one staging slot per restart segment,
 * sized by the same bound, and the segment lengths); nothing has to be cleared.
 * Enqueues two launches on `stream` (segments; lengths scan + assembly), no synchronisation, no atomics on global memory, no
 * floats: a frame's bytes do not depend on T.  T outside 1..65535, H or W outside 1..65535, quality outside 1..100, a
 * dst_stride below 631 or of 2 GiB or more, a NULL or misaligned pointer: RIB_ERR_INVALID with a rib_last_error text, nothing
 * launched (the two size queries return 0). */
size_t rib_jpeg_workspace_bytes(rib_handle* h, int T, int H, int W);
size_t rib_jpeg_max_bytes(int H, int W);
int rib_jpeg(rib_handle* h, int T, int H, int W, const uint8_t* src_u8_nhwc, int quality,
             uint8_t* dst, size_t dst_stride, int32_t* lengths, void* workspace, void* hip_stream);
/* rib_jpeg_float: the same files from the frames the chain produces - fp32 NCHW [T,3,H,W] in [-1, 1], 4-byte aligned - without the
 * uint8 copy in between: byte for byte rib_jpeg(rib_quantise(src)), i.e. panel.jpeg_encode_host(panel.quantise_host(src)).
 * Only the kernel's first step differs (the three channel planes are read, float4 where a row segment is 16-byte aligned and
 * whole, and quantised with rib_quantise's arithmetic); the contract is rib_jpeg's: the same two size queries, the same
 * workspace, refusals and errors, two launches, no atomics, a frame's bytes independent of T. */
int rib_jpeg_float(rib_handle* h, int T, int H, int W, const float* src_f32_nchw, int quality,
                 uint8_t* dst, size_t dst_stride, int32_t* lengths, void* workspace, void* hip_stream);
/* ---- lossless PNG of the folder driver's frames, encoded on the GPU (evaluate_from_folder(png_on="gpu")) ----
 * T images uint8 NHWC [T,H,W,3] on the device -> T complete PNG files: 8 bit, colour type 2, no interlace; a zlib stream cut
 * into one IDAT chunk for its two header bytes (78 01), one IDAT chunk per strip of 8 image rows (the last strip may be
 * shorter) and one IDAT chunk for the Adler-32, so that every chunk CRC is one strip's own business.  Per row the one of the
 * five PNG filters with the smallest sum of |int8(filtered byte)| (a tie: the lower type; "above" is the raw row, also across
 * strips); per strip one dynamic-Huffman deflate block whose only matches are runs at distance 1 (a run of R equal bytes: a
 * literal, then lengths min(m, 258) while m >= 4, then m literals) and whose literal/length code is the cheapest of K given
 * tables, header included (a tie: the lower k); a strip that is not the last ends with an empty stored block, so every strip
 * is whole bytes.  The stream and the tables are this project's; png.py (encode_host) states every byte in integers, and the
 * kernels are bit-equal to it.  No LZ77 search, no tree built on the device, no checksum that spans workgroups.
 * code_lengths: HOST uint8 [K][286], 1 <= K <= 16; every table a complete prefix code (Kraft sum exactly 1) with lengths in
 * 1..15, every length of table 0 at most 9.  The library validates them, builds the canonical codes (RFC 1951 3.2.2) and the
 * block headers with png.py's rule on the host and keeps the device copy on the handle; they are uploaded again only when
 * their bytes change (the upload is ordered on `stream`).
 * Frame t's file starts at dst + t * dst_stride and lengths[t] (device, int32) receives its size.  rib_png_max_bytes(H, W) is an
 * upper bound of one file (table 0 prices a literal at <= 9 bits and a match of >= 4 bytes at <= 9 + 5 + 1 bits; png.py
 * max_bytes); with dst_stride >= rib_png_max_bytes no frame is refused.  A smaller dst_stride is allowed: a frame whose file
 * would not fit writes nothing and gets lengths[t] = 0 - the call only enqueues and returns RIB_OK, the caller reads the
 * refusal from lengths.  Bytes of a frame's stride behind lengths[t] are not written.
 * workspace: rib_png_workspace_bytes(h, T, H, W) bytes on the device, 16-byte aligned (one staging slot per strip, sized by
 * the same bound, and four words per strip: length, chunk CRC, Adler A, Adler B); nothing has to be cleared.
 * Enqueues two launches on `stream` (strips; lengths scan + Adler combination + assembly), no synchronisation, no atomics on
 * global memory, no floats: a frame's bytes do not depend on T.  T outside 1..65535, H outside 1..65535, W outside 1..4096, a
 * dst_stride of 0 or of 2 GiB or more, a NULL or misaligned pointer, K outside 1..16 or an invalid table: RIB_ERR_INVALID with
 * a rib_last_error text, nothing launched (the two size queries return 0). */
size_t rib_png_max_bytes(int H, int W);
size_t rib_png_workspace_bytes(rib_handle* h, int T, int H, int W);
int rib_png(rib_handle* h, int T, int H, int W, const uint8_t* src_u8_nhwc,
            const uint8_t* code_lengths /* HOST [K][286] */, int K,
            uint8_t* dst, size_t dst_stride, int32_t* lengths, void* workspace, void* hip_stream);

/* ---- motion-compensated interpolation (MCI) of a segment's two key frames: the folder driver's background="mci" ----
 * This project's interpolation, NOT DAIN (the reference reads one DAIN frame per output frame; DAIN is an external network with
 * its own CUDA ops): the generator was trained on DAIN backgrounds and the quality of this substitute on real footage has not
 * been measured.  background.py (mci_field_host, mci_frames_host) states both results in integers - luma, a pyramid of
 * L levels, bilateral 8x8 block matching (full search over [-4,4]^2 on the top level - with L = 3 at quarter size, i.e. +-32 px
 * of motion between the key frames; +-1 refinements on every level below; the minimum of (cost, dx^2+dy^2, dy, dx)), a 3x3 median,
 * a bilinear per-pixel field in 1/256 px, two fixed-point bilinear samples and a blend - and the kernels are bit-equal to it.
 * No occlusion reasoning inside the frame unless the person is excluded (`rib_masked_*`, below).  The search itself is in whole pixels; rib_halfpel_refine (below) adds one half-pel step.
 * rib_mci_field: a_u8, b_u8 uint8 NHWC [B,H,W,3] on the device (left and right key frame of B segments at the model size) ->
 * field_i16 int16 [B,Hb,Wb,2] on the device, (dx, dy) per 8x8 block of the intermediate frame (rib_mci_field_shape:
 * Hb = ceil(H/8), Wb = ceil(W/8)); once per segment.  levels: L = 3, 4 or 5 pyramid levels (the driver's --mci-range 32, 64, 128:
 * the nominal range 4 * 2^(L-1) * 2 px between the key frames); the field's components reach 19, 39 or 79, i.e. 38, 78 or 158 px
 * of motion between the key frames, and a wider search has more room for a false match on periodic content.  border (the
 * driver's --mci-border; background.py's border=): 0 = "clamp", samples clamped to the edge; 1 = "valid", one-sided at the FRAME
 * border: a block's pixel counts for a candidate d only when p - d and p + d both lie inside the level's plane (n pixels, a
 * closed-form rectangle, of the block's N); a candidate is valid when 4 n >= N, costs (64 * SAD over those n) / n +
 * LAMBDA (|dx| + |dy|), the winner is the minimum key over the valid candidates, and a block whose start candidate is not valid
 * keeps its start.  workspace: rib_mci_workspace_bytes(h, B, H, W, levels) bytes on the device, 16-byte aligned, nothing to
 * clear.  L + 2 launches on `stream` (luma + pyramid, one search per level, median: five, six, seven; an added launch took
 * 6.7 - 7.3 us on an MI355X at 512x512, B = 4, the field 54 / 61 / 69 us of kernel time: profiles/r12_mci_range.txt), the same
 * for either border; no atomics, no synchronisation: a segment's field does not depend on B.
 * rib_mci_frames: frames k_first .. k_first + T - 1 (0 <= k <= sample_rate, a power of two <= 1024; k = 0 is A, k = sample_rate
 * is B) of all B segments in ONE launch, from the field of any L: out_f32_nchw float32 [T,B,3,H,W], ((u8 / 255 - 0.5) / 0.5)
 * exactly as the driver's upload computes it (the arithmetic of rib_resize_cubic's float output), and / or out_u8_nhwc uint8
 * [T,B,H,W,3]; a NULL output is not wanted (both NULL is an error).  border: 0 = the blend of the two clamped samples; 1 = a
 * sample is valid when its position lies in [0, (H-1) << 8] x [0, (W-1) << 8], and where exactly one of the two samples is
 * valid the output is that sample alone (a hard switch), otherwise the blend.  Interior occlusion - a foreground object
 * covering background - is NOT handled unless the person is excluded (`rib_masked_*`).  Every element written; a frame's bytes do not depend on T or B.
 * levels outside 3..5, border outside {0, 1}, B outside 1..32767, B * Hb * Wb >= 2^30, T < 1, T * B > 65535, H or W outside
 * 1..16384, a bad sample_rate or frame range, NULL or misaligned pointers: RIB_ERR_INVALID with a rib_last_error text, nothing
 * launched (the size query returns 0).
 * rib_halfpel_refine (the driver's --mci-precision half; background.mci_refine_host, bit-equal): the integer field writes the motion
 * between the key frames as 2 d, an even number of pixels; this turns field_i16 (rib_mci_field's, any L) into field_half_i16,
 * int16 [B,Hb,Wb,2] in HALF pixels: per block the minimum of (cost, hx^2+hy^2, hy, hx) over h in 2 d + [-1,1]^2, cost = the SAD of
 * the half-pel planes (a half position is the rounded mean of its two or four pixels) at clamp(2p - h) in A and clamp(2p + h) in
 * B + 2 (|hx| + |hy|); border = 1: rib_mci_field's one-sided rule in half-pel coordinates (a block whose start 2 d is not valid
 * keeps 2 d).  ONE launch on `stream`, luma computed from the RGB bytes: no workspace, nothing of rib_mci_field's workspace is
 * read; no atomics, a segment's result does not depend on B.  field_half_i16 == field_i16 (in place) is allowed; both 4-byte
 * aligned.  Components beyond +-79 (no rib_mci_field result has them) cannot be refused without reading the device: such input
 * is undefined - the kernel clamps it to +-79, so nothing is read out of bounds.  Half-pel samples are bilinear and therefore
 * soft; a block whose integer vector is more than one half-pel step from the truth stays wrong; no quarter-pel, no sub-pel search
 * on the coarse levels.
 * rib_halfpel_frames: rib_mci_frames for a field in half pixels (offsets k D / s and (s-k) D / s): the same host body, the same
 * kernel template, the same contract and refusals; the field 2 f gives the bytes rib_mci_frames gives for f.  It is an entry of
 * its own only because rib_mci_frames' 14 arguments are pinned by existing callers and tests; folding it into rib_mci_frames as
 * a `precision` argument is the follow-up (one entry per operation).  The two entries are named rib_halfpel_*, not rib_mci_*: the
 * rib_mci_* family is held at four entries (one per operation and the shape query) by the suite, and the fold brings it back to that.
 * Both: border outside {0, 1}, bad B, H, W, T, sample rate or frame range, NULL or misaligned pointers: RIB_ERR_INVALID with a
 * rib_last_error text, nothing launched.
 * rib_scaled_frames (the driver's --output-size keyframes; background.mci_frames_scaled_host, bit-equal): rib_mci_frames' uint8
 * frames at the key frames' OWN size - "field at the model size, samples at the key frames' size".  a0_u8, b0_u8 uint8 NHWC
 * [B,H0,W0,3] are the key frame files' pixels, field_i16 the [B,Hb,Wb,2] field of the H x W MODEL-size key frames (Hb = ceil(H/8),
 * Wb = ceil(W/8); rib_mci_field's with precision = 0, rib_halfpel_refine's with precision = 1) -> out_u8_nhwc uint8
 * [T,B,H0,W0,3], any byte alignment.  Per output pixel (Y0, X0): (1) TX = ((2 X0 + 1) * 16 W) / W0 - 128 is its centre's position in
 * 1/256 block from block centre 0 (TY with H, H0), c0 = TX >> 8, fx = TX & 255, c0 and c0 + 1 clamped to the field; (2) D16 = the
 * bilinear sum of the four vectors with the 8-bit weights, D8 = (D16 + 128) >> 8 in 1/256 model px; (3) DSx = (D8x * SX + 32768) >>
 * 16 with SX = (W0 * 65536 + W / 2) / W (SY with H0, H; a 64-bit product) in 1/256 px of the output; (4) rib_mci_frames' offsets,
 * samples, blend and border = 1 rule with DS, H0, W0.  With (H0, W0) == (H, W) the bytes are rib_mci_frames'.  There is no float
 * output: the generator is fed rib_mci_frames' floats at the model size.  ONE launch on `stream`, no workspace, no atomics, no
 * synchronisation; every byte written; a frame's bytes do not depend on T or B.  rib_mci_frames' refusals, and also: H0 or W0
 * outside 1..16384, W0 > 16 W, W > 16 W0 (the same for the heights: beyond a ratio of 16 an offset could leave int32), precision
 * outside {0, 1}, out NULL: RIB_ERR_INVALID with a rib_last_error text that names the entry, nothing launched.  The field has the
 * model's resolution - motion detail finer than an 8x8 model block is not followed - and, as above, interior occlusion is not handled.
 * rib_masked_workspace_bytes / rib_masked_field / rib_masked_frames (the driver's --mci-person exclude; background.mci_field_masked_host
 * and mci_frames_masked_host, bit-equal): rib_mci_field and rib_mci_frames with the person kept out.  ma_u8, mb_u8 uint8 [B,H,W] on
 * the device, nonzero = EXCLUDED, for key frame A and key frame B (the driver passes rib_human_mask of the two key frames' poses).
 * Field: an OR pyramid of the masks (a pixel is set iff any of its 2x2 clamped parents is); on every level and for either border a
 * block's pixel p counts for candidate d iff the border rule lets it count and MA(clamp(p - d)) == 0 and MB(clamp(p + d)) == 0 (n
 * counted pixels of the block's N); a candidate is valid iff 4 n >= N, costs (64 * SAD over the counted pixels) / n + LAMBDA (|dx| +
 * |dy|), the winner is the minimum key over the valid candidates, and a block whose start candidate is not valid is not searched
 * and keeps its start.  On the TOP level such a block then takes the vector of the searched block within Chebyshev distance 8 that
 * minimises (max(|Dy|,|Dx|), |Dy|+|Dx|, Dy, Dx), or (0, 0); below it, it keeps twice the coarser block's vector.  Median and
 * per-pixel field are rib_mci_field's.  workspace: rib_masked_workspace_bytes(h, B, H, W, levels) bytes on the device (rib_mci_field's
 * plus the mask planes, one plane of flags and the top level's field before the fill), 16-byte aligned, nothing to clear.  L + 4
 * launches on `stream` (rib_mci_field's, the mask pyramid and the fill); no atomics, no synchronisation, a segment's field does not
 * depend on B.  Frames: a sample is clean iff the border rule calls it valid (border = 0: always) and the four taps of its bilinear
 * footprint in its key frame's mask, clamped as the sample's taps are, are all zero; where exactly one of a pixel's two samples is
 * clean the output is that sample alone (a hard switch, with a seam where it flips), otherwise the blend; k = 0 and k = sample_rate
 * stay A and B.  precision: 0 = the field in whole pixels (rib_mci_frames), 1 = in half pixels (rib_halfpel_frames) - here an
 * argument, not a second entry.  ONE launch, both outputs as rib_mci_frames', a frame's bytes do not depend on T or B.  With
 * all-zero masks the frames are rib_mci_frames' and, under border = 1, the field rib_mci_field's.  The refusals are those of the
 * unmasked entries, and also: a NULL mask, precision outside {0, 1}: RIB_ERR_INVALID with a rib_last_error text that names the
 * entry, nothing launched (the size query returns 0).  The three are named rib_masked_*, not rib_mci_*: that family stays at four.
 * Only the masked pixels are kept out: background hidden in BOTH key frames stays a blend, and other moving objects are not handled. */
size_t rib_masked_workspace_bytes(rib_handle* h, int B, int H, int W, int levels);
int rib_masked_field(rib_handle* h, int B, int H, int W, const uint8_t* a_u8, const uint8_t* b_u8, const uint8_t* ma_u8,
                     const uint8_t* mb_u8, int16_t* field_i16, int levels, int border, void* workspace, void* hip_stream);
int rib_masked_frames(rib_handle* h, int T, int B, int H, int W, const uint8_t* a_u8, const uint8_t* b_u8, const uint8_t* ma_u8,
                      const uint8_t* mb_u8, const int16_t* field_i16, int sample_rate, int k_first, int border, int precision,
                      float* out_f32_nchw, uint8_t* out_u8_nhwc, void* hip_stream);
int rib_scaled_frames(rib_handle* h, int T, int B, int H, int W, int H0, int W0, const uint8_t* a0_u8, const uint8_t* b0_u8,
                      const int16_t* field_i16, int sample_rate, int k_first, int border, int precision, uint8_t* out_u8_nhwc,
                      void* hip_stream);
/* rib_cubic_frames / rib_cubic_scaled (the driver's --mci-sampler cubic; background.sample_cubic and the sampler="cubic" forms of
 * mci_frames_host, mci_frames_masked_host and mci_frames_scaled_host, bit-equal): the frames of rib_mci_frames / rib_halfpel_frames /
 * rib_masked_frames and of rib_scaled_frames with every bilinear sample replaced by a 4x4 Catmull-Rom (A = -1/2) sample and NOTHING
 * else changed - offsets, blend, k = 0 / k = s, both outputs, alignment and the "ONE launch, no workspace" contract are theirs.
 * The sample at (py, px) in 1/256 px: tap rows (py >> 8) - 1 .. + 2, tap columns (px >> 8) - 1 .. + 2, each clamped to the frame;
 * weights in 1/128 per axis from f = p & 255 by integers: n0 = -f^3 + 512 f^2 - 65536 f, n1 = 3 f^3 - 1280 f^2 + 2 * 256^3,
 * n2 = -3 f^3 + 1024 f^2 + 65536 f, n3 = f^3 - 256 f^2, w_i = (n_i + 2^17) >> 18, the residual 128 - sum(w) added to the larger of
 * w1, w2 (w1 on a tie); acc = sum_r wy[r] * (sum_c wx[c] * tap[r][c]) (|acc| < 2^23), result clip((acc + 8192) >> 14, 0, 255): the
 * Catmull-Rom kernel overshoots at strong edges and the result is clamped.  border = 1: the rule is rib_mci_frames' (the sample's POSITION
 * lies inside the frame; taps beyond the edge clamp), so the one-sided pixels are the bilinear entry's.  ma_u8, mb_u8 as
 * rib_masked_frames' - both NULL: the person is kept; both given: a sample is clean iff all 16 clamped taps are clear (the clean /
 * blend seam moves by a pixel against the 2x2 footprint's); exactly one NULL: RIB_ERR_INVALID.  precision: 0 = the field in
 * whole pixels, 1 = in half pixels.  Where every offset is a whole pixel (k = 0, k = s, often k = s / 2) the bytes are the
 * bilinear entries'.
 * staging: 0 = a tile (64 consecutive x of one output row, one wave) whose taps fit a 12 x 76 window per key frame reads them from LDS,
 * staged with one dword load per pixel, and every other tile gathers them directly (background.cubic_tile_staged states the rule);
 * 1 = never stage.  It is a DIAGNOSTIC for the tests and the benches: the bytes never depend on it.
 * The refusals are rib_masked_frames' / rib_scaled_frames' (sides 1..16384, sample_rate a power of two <= 1024, the frame range,
 * border and precision in {0, 1}, the scaled form's ratio of 16, NULL or misaligned pointers, both outputs NULL), and also staging
 * outside {0, 1}: RIB_ERR_INVALID with a rib_last_error text that begins with the entry's name, nothing launched.  Named rib_cubic_*,
 * not rib_mci_*: that family stays at four.  This is still this project's interpolation: no interior occlusion reasoning. */
int rib_cubic_frames(rib_handle* h, int T, int B, int H, int W, const uint8_t* a_u8, const uint8_t* b_u8,
                     const uint8_t* ma_u8, const uint8_t* mb_u8,   /* both NULL: the person is kept; exactly one NULL: invalid */
                     const int16_t* field_i16, int sample_rate, int k_first, int border, int precision, int staging,
                     float* out_f32_nchw, uint8_t* out_u8_nhwc, void* hip_stream);
int rib_cubic_scaled(rib_handle* h, int T, int B, int H, int W, int H0, int W0, const uint8_t* a0_u8, const uint8_t* b0_u8,
                     const int16_t* field_i16, int sample_rate, int k_first, int border, int precision, int staging,
                     uint8_t* out_u8_nhwc, void* hip_stream);
/* rib_detail_workspace_bytes / rib_detail_field (the driver's --mci-detail keyframes; background.mci_detail_field_host, bit-equal): the block
 * field REFINED AT THE KEY FRAMES' OWN SIZE.  Under rib_scaled_frames the field holds whole MODEL pixels - multiples of 3.75 output pixels
 * at 512 -> 1920 - so a block's two samples are misregistered by up to one quantum.  a0_u8, b0_u8 uint8 NHWC [B,H0,W0,3] are the key frame
 * files' pixels, field_i16 the [B,Hb,Wb,2] field of the H x W MODEL-size key frames (rib_mci_field's with precision = 0,
 * rib_halfpel_refine's in half pixels with precision = 1) -> out_field_i16 int16 [B,H0b,W0b,2], H0b = ceil(H0/8), W0b = ceil(W0/8): a block
 * field of the FULL-SIZE frames in WHOLE OUTPUT pixels of half the motion, rib_mci_field's meaning at that size.  Per block (by, bx):
 * start = rib_scaled_frames' steps (1)-(3) at the pixel (min(8 by + 4, H0 - 1), min(8 bx + 4, W0 - 1)), rounded to whole pixels as (DS +
 * 128) >> 8 (precision = 1: (DS + 256) >> 9); the winner of start + [-R, R]^2 on the full-size lumas under rib_mci_field's rules (border =
 * 0: the clamped SAD + 4 (|dx| + |dy|), the minimum of (cost, dx^2+dy^2, dy, dx); border = 1: the one-sided cost over the candidates with
 * 4 n >= N, and a block whose start is not valid keeps its start), R = min(4, max(1, (c + 1) / 2)), c = max(ceil(W0/W), ceil(H0/H)) - half
 * the model-pixel quantum: 1 up to ratio 2, 2 up to 4, 3 up to 6, 4 beyond; above ratio 8 the search no longer covers the quantum; then
 * rib_mci_field's 3x3 median.  The key is 64-bit with 12 bits per component: components reach 79 * 16 + 4 = 1268 (1276 from half pixels).
 * The frames at the key frames' size are rib_mci_frames / rib_cubic_frames on (a0_u8, b0_u8, out_field_i16) at H0 x W0: the existing
 * entries (2 * 1024 * 1276 * 256 < 2^31); there is no new frame entry and no half-pel step at full size.  workspace:
 * rib_detail_workspace_bytes(h, B, H0, W0) bytes on the device, 16-byte aligned, nothing to clear - the field before the median and
 * nothing else; it must not overlap out_field_i16.  TWO launches on `stream` (the search, which computes every start itself and the luma
 * while staging, and the median); no atomics, no synchronisation, a segment's field does not depend on B.  Model-size components beyond
 * +-79 (+-159 in half pixels) cannot be refused without reading the device: the kernel clamps them, nothing is read out of bounds.
 * B outside 1..32767, a side outside 1..16384, B * ceil(H0/8) * ceil(W0/8) >= 2^30, W0 > 16 W, W > 16 W0 (the same for the heights),
 * precision or border outside {0, 1}, NULL or misaligned pointers (fields 4-byte, workspace 16-byte): RIB_ERR_INVALID with a rib_last_error
 * text that names the entry, nothing launched (the size query returns 0).  Named rib_detail_*, not rib_mci_*: that family stays at four.
 * This is still this project's interpolation: no interior occlusion reasoning, and a wrong model-size vector stays wrong beyond R. */
size_t rib_detail_workspace_bytes(rib_handle* h, int B, int H0, int W0);
int rib_detail_field(rib_handle* h, int B, int H, int W, int H0, int W0, const uint8_t* a0_u8, const uint8_t* b0_u8,
                     const int16_t* field_i16, int precision, int border, int16_t* out_field_i16, void* workspace, void* hip_stream);
/* rib_accel_workspace_bytes / rib_accel_field / rib_accel_frames (the driver's --mci-motion quadratic; background.mci_accel_host and
 * mci_frames_accel_host, bit-equal): the second-order trajectory across key frames.  The entries above move a segment's content at
 * constant velocity; these read the neighbouring segments' fields as well.
 * Field: cur_i16 int16 [B,Hb,Wb,2] the block fields of B segments (any of the field entries above: the entry takes the FIELD's
 * shape, so it serves the model-size fields and rib_detail_field's alike), prev_i16 / next_i16 the fields of the segments before and after
 * each, same shape and unit; half: 0 = whole pixels, 1 = half pixels (rib_halfpel_refine's).  Which neighbours exist: a NULL prev_i16
 * (next_i16) says no item has one; present_u8, NULL or uint8 [B,2] on the device, says it per item - present[2 b] nonzero: item b has a
 * previous segment, present[2 b + 1]: a next one (the planes of absent neighbours are not read) - for groups whose members differ;
 * NULL: every item has each neighbour whose pointer is given.  Per block (by, bx) with (fx, fy) = cur >> half (floor): prev is read at
 * block (clamp((8 by + 4 - 2 fy) >> 3), clamp((8 bx + 4 - 2 fx) >> 3)), next at (clamp((8 by + 4 + 2 fy) >> 3), clamp((8 bx + 4 + 2 fx)
 * >> 3)); both: a = next - prev; only next: 2 (next - cur); only prev: 2 (cur - prev); neither: 0; then rib_mci_field's 3x3 median ->
 * accel_i16 int16 [B,Hb,Wb,2] in the fields' unit (|a| <= 4 max|field|: 5104 at most, for components within +-1276).  workspace:
 * rib_accel_workspace_bytes(h, B, Hb, Wb) bytes on the device, 16-byte aligned, nothing to clear (the field before the median); it must
 * not overlap accel_i16.  TWO launches on `stream`; no atomics, no synchronisation, an item's result does not depend on B.  B outside
 * 1..32767, Hb or Wb outside 1..2048, B * Hb * Wb >= 2^30, half outside {0, 1}, cur, accel or workspace NULL, a misaligned pointer:
 * RIB_ERR_INVALID with a rib_last_error text that names the entry, nothing launched (the size query returns 0).
 * Frames: rib_mci_frames' arguments, contract and outputs with accel_i16 (the field above, for the same B segments), and as arguments
 * what the other frame entries are named for: precision (0 whole, 1 half pixels: field_i16's AND accel_i16's unit), sampler (0 bilinear,
 * 1 rib_cubic_frames' 4x4 sample, staged per tile by its rule on the CORRECTED positions), ma_u8 / mb_u8 (both NULL: the person is kept;
 * both given: rib_masked_frames' / rib_cubic_frames' clean-sample rule).  Acc(p) is bilinear from accel_i16 exactly as D(p) is from
 * field_i16 (1/256 of the unit); with UNIT = 2 (precision 0) or 1, c = (UNIT * k * (s - k) * Acc + 2 s^2) >> (2 log2 s + 2), a 64-bit
 * product and an arithmetic shift; A is sampled at p - off_a + c and B at p + off_b + c, off_a, off_b rib_mci_frames' rounded offsets:
 * BOTH samples move by c, which is 0 at k = 0 and k = s and a / 8 in the middle.  Blend, border = 1 and the masks act on those
 * positions.  An all-zero accel_i16 gives the bytes of rib_mci_frames / rib_halfpel_frames / rib_masked_frames / rib_cubic_frames.  ONE
 * launch, no workspace; a frame's bytes do not depend on T or B.  The refusals, each RIB_ERR_INVALID with a rib_last_error text that
 * names the entry, nothing launched: rib_mci_frames' (sizes, sample_rate a power of two <= 1024, the frame range, border, NULL or
 * misaligned pointers, both outputs NULL), precision or sampler outside {0, 1}, accel_i16 NULL or misaligned, exactly one mask NULL.
 * Named rib_accel_*, not rib_mci_*: that family stays at four.  Second order from three fields: a wrong neighbour field gives a wrong
 * correction, the median is the only guard, and there is still no interior occlusion reasoning. */
size_t rib_accel_workspace_bytes(rib_handle* h, int B, int Hb, int Wb);
int rib_accel_field(rib_handle* h, int B, int Hb, int Wb, const int16_t* prev_i16, const int16_t* cur_i16, const int16_t* next_i16,
                    const uint8_t* present_u8, int half, int16_t* accel_i16, void* workspace, void* hip_stream);
int rib_accel_frames(rib_handle* h, int T, int B, int H, int W, const uint8_t* a_u8, const uint8_t* b_u8,
                     const uint8_t* ma_u8, const uint8_t* mb_u8,   /* both NULL: the person is kept; exactly one NULL: invalid */
                     const int16_t* field_i16, const int16_t* accel_i16, int sample_rate, int k_first, int border, int precision,
                     int sampler, float* out_f32_nchw, uint8_t* out_u8_nhwc, void* hip_stream);
void rib_mci_field_shape(int H, int W, int* Hb, int* Wb);
size_t rib_mci_workspace_bytes(rib_handle* h, int B, int H, int W, int levels);
int rib_mci_field(rib_handle* h, int B, int H, int W, const uint8_t* a_u8, const uint8_t* b_u8, int16_t* field_i16,
                  int levels, int border, void* workspace, void* hip_stream);
int rib_mci_frames(rib_handle* h, int T, int B, int H, int W, const uint8_t* a_u8, const uint8_t* b_u8, const int16_t* field_i16,
                   int sample_rate, int k_first, int border, float* out_f32_nchw, uint8_t* out_u8_nhwc, void* hip_stream);
int rib_halfpel_refine(rib_handle* h, int B, int H, int W, const uint8_t* a_u8, const uint8_t* b_u8,
                   const int16_t* field_i16, int16_t* field_half_i16, int border, void* hip_stream);
int rib_halfpel_frames(rib_handle* h, int T, int B, int H, int W, const uint8_t* a_u8, const uint8_t* b_u8,
                        const int16_t* field_half_i16, int sample_rate, int k_first, int border,
                        float* out_f32_nchw, uint8_t* out_u8_nhwc, void* hip_stream);

/* Extension op named by the north star but absent from the reference: bilinear
 * flow-grid warp, semantics of torch.nn.functional.grid_sample(img, base+flow*2/(size-1),
 * 'bilinear', padding_mode='border', align_corners=True).  flow [B,2,H,W] in pixels (x,y). */
int rib_warp(rib_handle* h, int B, int C, int H, int W, const float* img, const float* flow,
             float* out, void* hip_stream);

/* ---- introspection for parity tests (no reference counterpart) ----
 * After a rib_forward on `workspace`, intermediate activations can be read back as NCHW - the reference-side
 * equivalent is a forward hook on a leaf module.  The plan gives buffers with disjoint lifetimes
 * the same workspace bytes, so taps must be switched on BEFORE the forward: rib_set_debug_taps(h, 1) keeps every
 * tapped activation intact until the end of the forward (and rebuilds the launch plans). */
int rib_set_debug_taps(rib_handle* h, int enable);
int rib_num_taps(rib_handle* h, int B, int H, int W);
int rib_tap_info(rib_handle* h, int B, int H, int W, int idx, const char** name, int* C, int* th,
                 int* tw);
int rib_read_tap(rib_handle* h, int B, int H, int W, int idx, const void* workspace,
                 float* dst_nchw_device, void* hip_stream);

/* ---- measurement: per-kernel-class device time with HIP events on the caller's stream ----
 * rib_profile_begin() makes subsequent forwards record ONE event in front of every launch and one behind the
 * last (slower; never enable inside a timed region).  A launch is charged the time from its event to the next
 * one, so the classes add up to the forward's time on the stream, dispatch gaps included.
 * rib_profile_collect() synchronises and returns, per class, the number of launches and total milliseconds
 * since begin.  RIB_KC_CONVAUX holds the launches that are part of computing a convolution of class
 * RIB_KC_IGEMM but are not matrix-core kernels: the Winograd input / output transforms and the split-K slab
 * sums - a convolution's time is IGEMM + CONVAUX. */
enum { RIB_KC_IGEMM = 0, RIB_KC_SPADE = 1, RIB_KC_STATS = 2, RIB_KC_POOL = 3, RIB_KC_ELTWISE = 4,
       RIB_KC_PACK = 5, RIB_KC_CONVAUX = 6, RIB_KC_COUNT = 7 };
int rib_profile_begin(rib_handle* h);
/* rib_profile_begin_kernels(): the same bookkeeping, but every launch carries a (start, stop) event pair bound to the
 * dispatch itself (hipExtLaunchKernelGGL): rib_profile_collect() then returns the kernels' OWN execution times from the
 * queue's timestamps - the durations rocprofv3 --kernel-trace reports, with no event packet between two launches; the
 * classes no longer add up to the step (the dependent-launch gaps belong to no kernel). */
int rib_profile_begin_kernels(rib_handle* h);
int rib_profile_collect(rib_handle* h, int64_t launches[RIB_KC_COUNT], double ms[RIB_KC_COUNT]);
/* Algorithmic FLOPs (2*MAC) one rib_forward spends in class RIB_KC_IGEMM / RIB_KC_SPADE. */
int rib_forward_flops(rib_handle* h, int B, int H, int W, double flops[RIB_KC_COUNT]);
int rib_num_launches(rib_handle* h, int B, int H, int W);

/* ---- tuning hooks (tools/autotune.py): the launch plan picks, per convolution, one of a small set
 * of tile geometries and a split-K factor from an analytic cost model; a measured choice can be
 * pinned per (B,H,W, op name).  geom = {FRW,WM,WN,MF,NF,BK,STRIDE,KS,UPS,SPADE,KW,TB} (KW: wave
 * groups per workgroup, in-workgroup split-K; TB: filter slices staged per barrier). ---- */
int rib_num_variants(void);
int rib_variant_info(int idx, int geom[12]);   /* returns the precision of the instantiation (0 fp32, 1 bf16, 2 half), <0 on error */
int rib_set_choice(rib_handle* h, int B, int H, int W, const char* op_name, int variant_idx, int ksplit);
int rib_time_op(rib_handle* h, int B, int H, int W, const char* op_name, const float* label,
                const float* img_fake, const float* img_prev, float* img, float* mask, void* workspace,
                size_t workspace_bytes, int iters, void* hip_stream, double* usec);

/* ---- graph replay of rib_chain (no reference counterpart; a host-side option).  With it on (or RIB_GRAPH=1 in the
 * environment at rib_create), the first rib_chain call with a given (T,B,H,W) AND a given set of pointers captures the
 * segment's launches into one HIP graph and every later call with the same arguments is ONE hipGraphLaunch on the
 * caller's stream (which must not be the NULL stream - that one cannot be captured and keeps the launch-by-launch
 * path); calls with other tensors capture their own graph (at most 8 are kept, least recently used first out).
 * Same kernels, parameters and order: frames are bit-identical to the launch-by-launch path (tested).  Meant for hosts
 * that drive many GPUs from few cores, where enqueueing ~130 launches per frame per GPU becomes the limiter.
 * rib_graph_stats: how many calls captured / replayed since rib_create.
 * A captured segment holds the plans' kernels and parameters, so every call that changes them - rib_set_choice,
 * rib_set_plan_batch, rib_set_products, rib_set_compute_dtype, rib_set_debug_taps, rib_finalize_weights / rib_import_weights,
 * turning replay off - destroys the handle's captured graphs first, and so does the eviction of the least recently used one:
 * these calls BLOCK the host until the handle's device is idle (hipDeviceSynchronize: a graph may still be running on any
 * stream it was replayed on) whenever captured graphs exist.  With no captured graph they do not synchronise. ---- */
int rib_set_graph_replay(rib_handle* h, int enable);
int rib_graph_stats(rib_handle* h, int64_t* captures, int64_t* replays);

/* ---- batch-invariant launch plans (no reference counterpart: the reference renders one frame per call,
 * PGNR/models/evaluator.py:238-262, so its frames cannot depend on a grouping).  By default every batch size has its own
 * kernel choices (measured table or cost model: tile variant, split-K, Winograd tile, fused / level-wise SPADE), and a
 * sample rendered in a batch of 4 differs from the same sample rendered alone by ~1e-5 (other summation order).
 * rib_set_plan_batch(h, n) with n > 0 makes every plan built afterwards, whatever its batch, follow the choices of batch n:
 * a launch only grows in its per-sample grid dimension, a sample's arithmetic is the same in every grouping, and the
 * frames of rib_forward / rib_chain at B = 1, 2, 3, ... are bit-identical per sample (GPU test).  The folder driver
 * sets n to its group size, so that ragged last groups, other world sizes and --batch 1 all write the same bytes.
 * n = 0 restores the default.  Plans are rebuilt on demand; the required workspace of a shape may change with n
 * (query rib_workspace_bytes / rib_chain_workspace_bytes again). ---- */
int rib_set_plan_batch(rib_handle* h, int n);
int rib_get_plan_batch(const rib_handle* h);

/* ---- staged Winograd input transforms (no reference counterpart).  On (the default) the `.wino_in` launches of the fp32
 * plans stage each workgroup's input patch in LDS, so that every element is fetched and modulated once instead of once per
 * (tile, row) unit that reads it; off runs the unstaged kernels.  Both sides write the same bits everywhere and have the
 * same launch list and workspace; only the grids of the `.wino_in` launches differ (A/B measurements, GPU test).
 * RIB_WINO_IN_UNSTAGED=1 in the environment at rib_create starts a handle with it off.  Changing it drops the cached
 * plans and the captured chain graphs, as the other setters do. ---- */
int rib_set_wino_in_staging(rib_handle* h, int on);

/* ---- build identity (no reference counterpart: the reference is interpreted Python).  A static string
 *   "librib stamp=<lib> shards=<s0>,...,<s23> consistent=<0|1> variants=<n> frame=<f> compiler=<...>"
 * where <lib> is the content hash (csrc/build.py: sha256 over rib.hip, kernels.hip.h, rib_host.h, pixel_ops.hip.h, igemm.hip.h,
 * variants.def, variants.hip.h, igemm_shard.hip, include/rib.h + flags + compiler version) rib.o was compiled with, <si> the hash
 * shard object i carries (24 of them, csrc/variants.hip.h) and <f> the hash of frame.o (frame.hip and the kernel headers of the
 * frame utilities: rib_blend ... rib_mci_frames); consistent=1 when all shards carry the hash rib.o expected of them and frame.o was
 * compiled against the same shared headers (rib_host.h, pixel_ops.hip.h, this file) as rib.o.  bench.py
 * prints it in its JSON line; tests/test_native_host.py compares it with the hashes of the tracked tree. ---- */
const char* rib_build_info(void);

/* ---- host-only debugging (CPU tests): rib_create(cfg, device = -1, ..) builds a handle that owns
 * no device memory; it supports the tensor inventory, rib_set_tensor / rib_finalize_weights (the
 * folded blob stays on the host), plans (workspace size, launch list, FLOPs) and these readers,
 * which undo the filter re-layout so the fold can be compared with the oracle. ---- */
int rib_debug_conv_weight(rib_handle* h, const char* conv_name, float* w_oihw, float* bias);
int rib_debug_spade_weight(rib_handle* h, const char* conv_name, float* w_2c_by_cond, float* bias_2c);
int rib_debug_launch_info(rib_handle* h, int B, int H, int W, int idx, char* buf, size_t buflen);

#ifdef __cplusplus
}
#endif
#endif /* RIB_H */
