// frame.hip — the folder driver's frame utilities behind the C ABI (include/rib.h): blend, quantise, cubic resize, PSNR/SSIM,
// flow warp, source-size composite, label rasteriser, pose mask, diagnostic sheet, JPEG encoder, PNG encoder and the motion-compensated background (MCI).  The second host object of librib.so (frame.o,
// csrc/build.py).  None of these entries touches a launch plan, the weight blob or a tuned choice: of a handle they use the
// device index, the error string and the small state of rib::FrameState (rib_host.h), reached through frame_state().
//
// Launches are plain hipLaunchKernelGGL.  The generator's kernel-time profiling (rib.hip: RIB_KLAUNCH) binds an event pair to
// a dispatch only inside run_plan's loop and run_plan resets the pair before it returns; rib_forward_blend and chain_enqueue
// call rib_blend after run_plan has returned, so no launch of this file was ever a profiled one.
#include "frame_kernels.hip.h"
#include "raster.hip.h"
#include "quality.hip.h"
#include "resize.hip.h"
#include "human_mask.hip.h"
#include "panel.hip.h"
#include "jpeg.hip.h"
#include "png.hip.h"
#include "mci.hip.h"
#include "composite.hip.h"
#include "rib_host.h"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>

using namespace rib;

#if !defined(RIB_BUILD_STAMP) || !defined(RIB_SHARED_STAMP)
#error "compile through csrc/build.py (-DRIB_BUILD_STAMP / -DRIB_SHARED_STAMP: content hashes of the sources, see build.py)"
#endif
// "rib-stamp frame <hash>": what rib_build_info() reports for this object and what build.py looks for in it; and the hash of
// the headers this object shares with rib.o as it was compiled (rib_build_info compares it with rib.o's own: `consistent`)
extern "C" __attribute__((used, visibility("hidden"))) const char rib_stamp_frame[] = "rib-stamp frame " RIB_BUILD_STAMP;
extern "C" __attribute__((used, visibility("hidden"))) const char rib_frame_shared_stamp[] = RIB_SHARED_STAMP;

extern "C" {

int rib_blend(rib_handle* handle, int B, int C, int H, int W, const float* img, const float* mask,
              const float* dain, float* fuse, void* hip_stream) {
  FrameState* h = frame_state(handle);
  if (!h || !img || !mask || !dain || !fuse) return RIB_ERR_INVALID;
  if (h->device >= 0) HIP_TRY(h, hipSetDevice(h->device));
  const size_t total = (size_t)B * C * H * W;
  const unsigned blocks = (unsigned)std::min<size_t>((total + 255) / 256, 4096);
  hipLaunchKernelGGL(k_blend, dim3(blocks), dim3(256), 0, reinterpret_cast<hipStream_t>(hip_stream), img, mask, dain, fuse, C, H * W, total);
  HIP_TRY(h, hipGetLastError());
  return RIB_OK;
}

int rib_quantise(rib_handle* handle, int B, int C, int H, int W, const float* img, uint8_t* out, void* hip_stream) {
  FrameState* h = frame_state(handle);
  if (!h || !img || !out) return RIB_ERR_INVALID;
  if (h->device >= 0) HIP_TRY(h, hipSetDevice(h->device));
  const size_t total = (size_t)B * C * H * W;
  const unsigned blocks = (unsigned)std::min<size_t>((total + 255) / 256, 4096);
  hipLaunchKernelGGL(k_quantise, dim3(blocks), dim3(256), 0, reinterpret_cast<hipStream_t>(hip_stream), img, out, C, H * W, total);
  HIP_TRY(h, hipGetLastError());
  return RIB_OK;
}

int rib_resize_cubic(rib_handle* handle, int N, int H0, int W0, int H, int W, const uint8_t* src, const int32_t* ix, const int32_t* cx,
                        const int32_t* iy, const int32_t* cy, uint8_t* out_u8, float* out_f32, void* hip_stream) {
  FrameState* h = frame_state(handle);
  if (!h) return RIB_ERR_INVALID;
  if (!src || !ix || !cx || !iy || !cy) return fail(h, RIB_ERR_INVALID, "rib_resize_cubic: null pointer");
  if (!out_u8 && !out_f32) return fail(h, RIB_ERR_INVALID, "rib_resize_cubic: both outputs are null");
  if (N < 1 || H0 < 1 || W0 < 1 || H < 1 || W < 1 || N > 65535)
    return fail(h, RIB_ERR_INVALID, fmt("rib_resize_cubic: N=%d H0=%d W0=%d H=%d W=%d: sizes must be positive (N <= 65535)", N, H0, W0, H, W));
  if ((size_t)H0 * W0 * 3 > (size_t)INT32_MAX || (size_t)H * W * 3 > (size_t)INT32_MAX)
    return fail(h, RIB_ERR_INVALID, "rib_resize_cubic: a frame must be smaller than 2 GiB");
  if (h->device >= 0) HIP_TRY(h, hipSetDevice(h->device));
  const int tilesX = (W * 3 + RSZ_TW - 1) / RSZ_TW, tilesY = (H + RSZ_TH - 1) / RSZ_TH;
  hipLaunchKernelGGL(k_resize_cubic_u8, dim3(tilesX * tilesY, N), dim3(256), 0, reinterpret_cast<hipStream_t>(hip_stream), src,
              reinterpret_cast<const int4*>(ix), reinterpret_cast<const int4*>(cx), reinterpret_cast<const int4*>(iy),
              reinterpret_cast<const int4*>(cy), out_u8, out_f32, H0, W0, H, W, tilesX);
  HIP_TRY(h, hipGetLastError());
  return RIB_OK;
}

int rib_composite(rib_handle* handle, int N, int H, int W, int H0, int W0, const float* pred, const float* mask, const uint8_t* bg,
                  const int32_t* ix, const int32_t* cx, const int32_t* iy, const int32_t* cy, uint8_t* out, void* hip_stream) {
  FrameState* h = frame_state(handle);
  if (!h) return RIB_ERR_INVALID;
  if (!pred || !mask || !bg || !ix || !cx || !iy || !cy || !out) return fail(h, RIB_ERR_INVALID, "rib_composite: null pointer");
  if (N < 1 || H < 1 || W < 1 || H0 < 1 || W0 < 1 || N > 65535)
    return fail(h, RIB_ERR_INVALID, fmt("rib_composite: N=%d H=%d W=%d H0=%d W0=%d: sizes must be positive (N <= 65535)", N, H, W, H0, W0));
  if ((size_t)H0 * W0 * 3 > (size_t)INT32_MAX || (size_t)H * W * 3 > (size_t)INT32_MAX)
    return fail(h, RIB_ERR_INVALID, "rib_composite: a frame must be smaller than 2 GiB");
  if ((reinterpret_cast<uintptr_t>(pred) & 3) != 0 || (reinterpret_cast<uintptr_t>(mask) & 3) != 0)
    return fail(h, RIB_ERR_INVALID, "rib_composite: pred and mask must be 4-byte aligned");
  if (h->device >= 0) HIP_TRY(h, hipSetDevice(h->device));
  CompositeParams cp;
  cp.pred = pred; cp.mask = mask; cp.bg = bg; cp.out = out;
  cp.ix = reinterpret_cast<const int4*>(ix); cp.cx = reinterpret_cast<const int4*>(cx);
  cp.iy = reinterpret_cast<const int4*>(iy); cp.cy = reinterpret_cast<const int4*>(cy);
  cp.H = H; cp.W = W; cp.H0 = H0; cp.W0 = W0;
  cp.tilesX = (W0 + CMP_TW - 1) / CMP_TW;
  const int tilesY = (H0 + CMP_TH - 1) / CMP_TH;
  // the input patch of a tile, bounded from the sizes alone: kept in LDS where it fits the budget, else no patch at all
  cp.pwMax = std::min(composite_patch_bound(CMP_TW, W0, W), W);
  cp.phMax = std::min(composite_patch_bound(CMP_TH, H0, H), H);
  if (cp.pwMax > CMP_PW || cp.phMax > CMP_PH) cp.pwMax = cp.phMax = 0;
  hipLaunchKernelGGL(k_composite, dim3(cp.tilesX * tilesY, N), dim3(256), composite_lds_bytes(cp.pwMax, cp.phMax),
                     reinterpret_cast<hipStream_t>(hip_stream), cp);
  HIP_TRY(h, hipGetLastError());
  return RIB_OK;
}

// rib_quality: the pooling factor, the tile grid and the workspace of one shape (quality.hip.h)
static bool quality_shape(int H, int W, int* f, int* Hp, int* Wp, int* tilesX, int* tilesY) {
  if (H < 1 || W < 1) return false;
  *f = std::max(1, (int)std::nearbyint(std::min(H, W) / 256.0));     // Python's round: half to even (fe default mode)
  *Hp = H / *f; *Wp = W / *f;
  if (*Hp < QUAL_K || *Wp < QUAL_K) return false;
  *tilesX = (*Wp - (QUAL_K - 1) + QUAL_OW - 1) / QUAL_OW;
  *tilesY = (*Hp - (QUAL_K - 1) + QUAL_OH - 1) / QUAL_OH;
  return true;
}

static size_t quality_ws_bytes(int B, int C, int tilesX, int tilesY) {
  return align256((size_t)B * C * tilesX * tilesY * 2 * sizeof(double));
}

size_t rib_quality_workspace_bytes(rib_handle* h, int B, int H, int W) {
  int f, Hp, Wp, tx, ty;
  if (!h || B < 1 || !quality_shape(H, W, &f, &Hp, &Wp, &tx, &ty)) return 0;
  return quality_ws_bytes(B, 3, tx, ty);
}

int rib_quality(rib_handle* handle, int B, int C, int H, int W, const float* pred, const float* target, const float* mask,
                float* psnr, float* ssim, void* workspace, size_t workspace_bytes, void* hip_stream) {
  FrameState* h = frame_state(handle);
  if (!h) return RIB_ERR_INVALID;
  if (!pred || !target || !psnr || !ssim || !workspace) return fail(h, RIB_ERR_INVALID, "rib_quality: null pointer");
  int f, Hp, Wp, tilesX, tilesY;
  if (B < 1 || C < 1 || !quality_shape(H, W, &f, &Hp, &Wp, &tilesX, &tilesY))
    return fail(h, RIB_ERR_INVALID, fmt("rib_quality: B=%d C=%d H=%d W=%d: the pooled frame must be at least %d x %d", B, C, H, W, QUAL_K, QUAL_K));
  const size_t need = quality_ws_bytes(B, C, tilesX, tilesY);
  if (workspace_bytes < need) return fail(h, RIB_ERR_WORKSPACE, fmt("rib_quality: workspace %zu < required %zu bytes", workspace_bytes, need));
  if (h->device >= 0) HIP_TRY(h, hipSetDevice(h->device));
  hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
  double* partials = reinterpret_cast<double*>(workspace);
  hipLaunchKernelGGL(k_quality_tiles, dim3(tilesX * tilesY, B * C), dim3(256), 0, st, pred, target, mask, C, H, W, f, Hp, Wp, tilesX, tilesY, partials);
  HIP_TRY(h, hipGetLastError());
  hipLaunchKernelGGL(k_quality_finalize, dim3(B), dim3(256), 0, st, (const double*)partials, C, tilesX * tilesY, H, W,
              Hp - (QUAL_K - 1), Wp - (QUAL_K - 1), psnr, ssim);
  HIP_TRY(h, hipGetLastError());
  return RIB_OK;
}

int rib_warp(rib_handle* handle, int B, int C, int H, int W, const float* img, const float* flow, float* out, void* hip_stream) {
  FrameState* h = frame_state(handle);
  if (!h || !img || !flow || !out) return RIB_ERR_INVALID;
  if (h->device >= 0) HIP_TRY(h, hipSetDevice(h->device));
  if (B < 1 || C < 1 || C > 8 || H < 1 || W < 1) return fail(h, RIB_ERR_INVALID, "rib_warp: 1 <= C <= 8 channels (the staged window must fit in LDS)");
  const int tilesX = (W + WARP_TW - 1) / WARP_TW, tilesY = (H + WARP_TH - 1) / WARP_TH;
  const size_t lds = (size_t)C * WARP_WH * WARP_PITCH * sizeof(float);      // 16 KB per channel
  // k_warp's dynamic-LDS limit is raised once per HANDLE, with the handle's device current (the attribute may be kept per
  // device: a process that drives two GPUs must not leave the second one at the 64 KB default), and a failure is reported
  // by the call that met it, not cached for the life of the process
  if (!h->warp_lds_ready) {
    HIP_TRY(h, hipFuncSetAttribute(reinterpret_cast<const void*>(&k_warp), hipFuncAttributeMaxDynamicSharedMemorySize, 8 * WARP_WH * WARP_PITCH * (int)sizeof(float)));
    h->warp_lds_ready = true;
  }
  hipLaunchKernelGGL(k_warp, dim3(tilesX * tilesY, B), dim3(256), lds, reinterpret_cast<hipStream_t>(hip_stream), img, flow, out, C, H, W, tilesX, xcd_chunk_of(tilesX * tilesY));
  HIP_TRY(h, hipGetLastError());
  return RIB_OK;
}

// a peak table of rib_rasterise / rib_human_mask: x < 0 marks an absent peak, any other must lie inside the frame
static bool peaks_inside(FrameState* h, const char* entry, const int32_t* peaks, size_t n, int H, int W) {
  for (size_t i = 0; i < n; ++i) {
    const int32_t x = peaks[2 * i], y = peaks[2 * i + 1];
    if (x >= W || (x >= 0 && (y < 0 || y >= H))) { fail(h, RIB_ERR_INVALID, fmt("%s: peak %zu (%d, %d) outside the frame", entry, i, x, y)); return false; }
  }
  return true;
}

static_assert(sizeof(rib_stroke) == sizeof(RasterStroke) && sizeof(rib_stroke) == 48, "rib_stroke layout");

namespace {
struct RasterLayout { size_t strokes, colors, peaks, weights, canvas, total; };
static RasterLayout raster_layout(int T, int H, int W, int n_edges, int n_maps, int radius) {
  RasterLayout L; size_t o = 0;
  L.strokes = o; o += align256((size_t)T * n_edges * sizeof(rib_stroke));
  L.colors = o;  o += align256((size_t)n_edges * sizeof(uint32_t));
  L.peaks = o;   o += align256((size_t)T * n_maps * 2 * sizeof(int32_t));
  L.weights = o; o += align256((size_t)(radius + 1) * sizeof(double));
  L.canvas = o;  o += align256((size_t)T * H * W * sizeof(uint32_t));
  L.total = o;
  return L;
}
}  // namespace

size_t rib_rasterise_workspace_bytes(rib_handle* h, int T, int H, int W, int n_edges, int n_maps, int radius) {
  if (!h || T < 1 || H < 1 || W < 1 || n_edges < 0 || n_maps < 0 || radius < 0) return 0;
  return raster_layout(T, H, W, n_edges, n_maps, radius).total;
}

int rib_rasterise(rib_handle* handle, int T, int H, int W, const rib_stroke* strokes, int n_edges,
                  const uint8_t* colors_rgb, int stroke_halfwidth, const int32_t* peaks, int n_maps,
                  const double* weights, int radius, float* labels, void* workspace, size_t workspace_bytes,
                  void* hip_stream) {
  FrameState* h = frame_state(handle);
  if (!h) return RIB_ERR_INVALID;
  if (h->device < 0) return fail(h, RIB_ERR_INVALID, "rib_rasterise: host-only handle");
  if (T < 1 || H < 1 || W < 1 || !labels || !workspace || (n_edges > 0 && (!strokes || !colors_rgb)) ||
      (n_maps > 0 && (!peaks || !weights)))
    return fail(h, RIB_ERR_INVALID, "rib_rasterise: bad argument");
  if (3 + n_maps != h->label_nc)
    return fail(h, RIB_ERR_INVALID, fmt("rib_rasterise: 3 + %d maps != label_nc %d", n_maps, h->label_nc));
  if (H > RASTER_MAXPTS || W > RASTER_MAXPTS) return fail(h, RIB_ERR_INVALID, fmt("rib_rasterise: H, W <= %d", RASTER_MAXPTS));
  if (radius > 127 || stroke_halfwidth < 1 || stroke_halfwidth > 16) return fail(h, RIB_ERR_INVALID, "rib_rasterise: radius <= 127, 1 <= stroke half-width <= 16");
  for (size_t i = 0; i < (size_t)T * n_edges; ++i)
    if (strokes[i].n < 0 || strokes[i].n > RASTER_MAXPTS) return fail(h, RIB_ERR_INVALID, fmt("rib_rasterise: stroke %zu has %d samples", i, strokes[i].n));
  if (!peaks_inside(h, "rib_rasterise", peaks, (size_t)T * n_maps, H, W)) return RIB_ERR_INVALID;
  const RasterLayout L = raster_layout(T, H, W, n_edges, n_maps, radius);
  if (workspace_bytes < L.total) return fail(h, RIB_ERR_WORKSPACE, fmt("workspace %zu < required %zu bytes", workspace_bytes, L.total));
  hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
  char* ws = reinterpret_cast<char*>(workspace);
  HIP_TRY(h, hipSetDevice(h->device));
  // The four tables sit at the head of the workspace in one contiguous range [0, L.canvas): they are assembled in a page-locked
  // staging slot and go over in ONE asynchronous copy.  (Rounds 1-3 copied from the caller's pageable arrays and then
  // synchronised the stream so that the arrays could be reused: where the upload stream shares a hardware queue with the
  // stream a chain runs on, that wait was the previous segment's whole chain - 60 ms per call, profiles/r04_prof_driver.txt.)
  {
    StageRing::Slot* slot;
    HIP_TRY(h, h->stage.acquire(L.canvas, false, &slot));
    StageRing::Slot& rs = *slot;
    memset(rs.host, 0, L.canvas);
    if (n_edges > 0) {
      memcpy(rs.host + L.strokes, strokes, (size_t)T * n_edges * sizeof(rib_stroke));
      uint32_t* packed = reinterpret_cast<uint32_t*>(rs.host + L.colors);
      for (int e = 0; e < n_edges; ++e)
        packed[e] = (uint32_t)colors_rgb[3 * e] | ((uint32_t)colors_rgb[3 * e + 1] << 8) | ((uint32_t)colors_rgb[3 * e + 2] << 16);
    }
    if (n_maps > 0) {
      memcpy(rs.host + L.peaks, peaks, (size_t)T * n_maps * 2 * sizeof(int32_t));
      memcpy(rs.host + L.weights, weights, (size_t)(radius + 1) * sizeof(double));
    }
    HIP_TRY(h, hipMemcpyAsync(ws, rs.host, L.canvas, hipMemcpyHostToDevice, st));
    HIP_TRY(h, hipEventRecord(rs.done, st));                    // the slot is free again once this copy has left it
  }
  if (n_maps > 0) {
    HeatParams hp;
    hp.peaks = reinterpret_cast<const int32_t*>(ws + L.peaks); hp.w = reinterpret_cast<const double*>(ws + L.weights);
    hp.r = radius; hp.label = labels; hp.T = T; hp.H = H; hp.W = W; hp.nmaps = n_maps; hp.label_nc = 3 + n_maps; hp.ch0 = 3;
    hipLaunchKernelGGL(k_heatmaps, dim3((H * W + 255) / 256, n_maps, T), dim3(256), 0, st, hp);
  }
  SkelParams sp;
  sp.strokes = reinterpret_cast<const RasterStroke*>(ws + L.strokes); sp.colors = reinterpret_cast<const uint32_t*>(ws + L.colors);
  sp.nedges = n_edges; sp.canvas = reinterpret_cast<uint32_t*>(ws + L.canvas); sp.label = labels;
  sp.T = T; sp.H = H; sp.W = W; sp.label_nc = 3 + n_maps; sp.bw = stroke_halfwidth;
  hipLaunchKernelGGL(k_skeleton, dim3(T), dim3(256), 0, st, sp);
  HIP_TRY(h, hipGetLastError());
  return RIB_OK;
}

int rib_human_mask(rib_handle* handle, int T, int H, int W, const int32_t* peaks, int n_joints, float* mask, void* hip_stream) {
  FrameState* h = frame_state(handle);
  if (!h) return RIB_ERR_INVALID;
  if (h->device < 0) return fail(h, RIB_ERR_INVALID, "rib_human_mask: host-only handle");
  if (!peaks || !mask) return fail(h, RIB_ERR_INVALID, "rib_human_mask: null pointer");
  if (n_joints != 18 && n_joints != 19) return fail(h, RIB_ERR_INVALID, fmt("rib_human_mask: a pose has 18 or 19 joints, got %d", n_joints));
  if (T < 1 || T > 65535 || H < 1 || W < 1 || H > HMASK_MAX_SIDE || W > HMASK_MAX_SIDE)
    return fail(h, RIB_ERR_INVALID, fmt("rib_human_mask: T=%d H=%d W=%d: 1 <= T <= 65535, H and W in 1..%d", T, H, W, HMASK_MAX_SIDE));
  const size_t n = (size_t)T * n_joints;
  if (!peaks_inside(h, "rib_human_mask", peaks, n, H, W)) return RIB_ERR_INVALID;
  hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
  HIP_TRY(h, hipSetDevice(h->device));
  const size_t bytes = n * 2 * sizeof(int32_t);
  StageRing::Slot* slot;
  HIP_TRY(h, h->stage.acquire(bytes, true, &slot));               // with the device copy of the table: the entry takes no workspace
  StageRing::Slot& ms = *slot;
  memcpy(ms.host, peaks, bytes);
  HIP_TRY(h, hipMemcpyAsync(ms.dev, ms.host, bytes, hipMemcpyHostToDevice, st));
  MaskParams mp;
  mp.peaks = reinterpret_cast<const int32_t*>(ms.dev); mp.mask = mask; mp.T = T; mp.H = H; mp.W = W; mp.nj = n_joints;
  mp.tilesX = (W + HMASK_TW - 1) / HMASK_TW;
  mp.vec = (W % 4 == 0 && (reinterpret_cast<uintptr_t>(mask) & 15) == 0) ? 1 : 0;
  const int tilesY = (H + HMASK_TH - 1) / HMASK_TH;
  hipLaunchKernelGGL(k_human_mask, dim3(mp.tilesX * tilesY, T), dim3(256), 0, st, mp);
  HIP_TRY(h, hipGetLastError());
  HIP_TRY(h, hipEventRecord(ms.done, st));                        // after the kernel that reads the slot's device table
  return RIB_OK;
}

int rib_panel(rib_handle* handle, int T, int H, int W, int label_nc, const float* pred, const float* mask, const float* fuse,
              const float* dain, const float* gt, const float* label, const uint8_t* titles, uint8_t* out, void* hip_stream) {
  FrameState* h = frame_state(handle);
  if (!h) return RIB_ERR_INVALID;
  if (h->device < 0) return fail(h, RIB_ERR_INVALID, "rib_panel: host-only handle");
  if (!dain || !gt || !label || !out) return fail(h, RIB_ERR_INVALID, "rib_panel: null pointer");
  const int given = (pred ? 1 : 0) + (mask ? 1 : 0) + (fuse ? 1 : 0);
  if (given != 0 && given != 3) return fail(h, RIB_ERR_INVALID, "rib_panel: pred, mask and fuse are NULL together (key-frame mode) or not at all");
  if (T < 1 || T > 65535 || H < 1 || W < 1 || H > PANEL_MAX_H || W > PANEL_MAX_W || label_nc < 3)
    return fail(h, RIB_ERR_INVALID, fmt("rib_panel: T=%d H=%d W=%d label_nc=%d: 1 <= T <= 65535, H in 1..%d, W in 1..%d, label_nc >= 3",
                                        T, H, W, label_nc, PANEL_MAX_H, PANEL_MAX_W));
  PanelParams pp;
  pp.pred = pred; pp.mask = mask; pp.fuse = fuse; pp.dain = dain; pp.gt = gt; pp.label = label; pp.titles = titles; pp.out = out;
  pp.H = H; pp.W = W; pp.label_nc = label_nc;
  pp.SH = 2 * (H + PANEL_TITLE) + 3 * PANEL_GUTTER;
  pp.SW = 3 * W + 4 * PANEL_GUTTER;
  if ((size_t)pp.SH * pp.SW * 3 > (size_t)INT32_MAX) return fail(h, RIB_ERR_INVALID, "rib_panel: a sheet must be smaller than 2 GiB");
  uintptr_t bits = reinterpret_cast<uintptr_t>(dain) | reinterpret_cast<uintptr_t>(gt) | reinterpret_cast<uintptr_t>(label);
  if (pred) bits |= reinterpret_cast<uintptr_t>(pred) | reinterpret_cast<uintptr_t>(mask) | reinterpret_cast<uintptr_t>(fuse);
  pp.vec = (W % 4 == 0 && (bits & 15) == 0 && (reinterpret_cast<uintptr_t>(out) & 3) == 0) ? 1 : 0;
  HIP_TRY(h, hipSetDevice(h->device));
  const size_t lds = (size_t)pp.SW * 3 + 32;             // the row at its phase inside a 16-byte line, rounded up to whole lines
  hipLaunchKernelGGL(k_panel, dim3(pp.SH, T), dim3(256), lds, reinterpret_cast<hipStream_t>(hip_stream), pp);
  HIP_TRY(h, hipGetLastError());
  return RIB_OK;
}

size_t rib_jpeg_max_bytes(int H, int W) {
  if (H < 1 || W < 1 || H > JPEG_MAX_DIM || W > JPEG_MAX_DIM) return 0;
  const size_t rows = (size_t)(H + 15) / 16;
  return (size_t)JPEG_HEADER_BYTES + rows * jpeg_seg_bound((W + 15) / 16) + 2 * (rows - 1) + 2;
}

size_t rib_jpeg_workspace_bytes(rib_handle* h, int T, int H, int W) {
  if (!h || T < 1 || T > 65535 || H < 1 || W < 1 || H > JPEG_MAX_DIM || W > JPEG_MAX_DIM) return 0;
  const size_t segs = (size_t)T * ((size_t)(H + 15) / 16);
  return segs * jpeg_seg_bound((W + 15) / 16) + 256 + segs * sizeof(int32_t);      // the slots, then the segment lengths
}

// rib_jpeg / rib_jpeg_float: one contract, two sources (k_jpeg_segments<uint8_t> / <float>, jpeg.hip.h)
extern "C++" {
template <typename S>
static int jpeg_enqueue(const char* entry, rib_handle* handle, int T, int H, int W, const S* src, int quality, uint8_t* dst, size_t dst_stride,
                        int32_t* lengths, void* workspace, void* hip_stream) {
  FrameState* h = frame_state(handle);
  if (!h) return RIB_ERR_INVALID;
  if (h->device < 0) return fail(h, RIB_ERR_INVALID, fmt("%s: host-only handle", entry));
  if (!src || !dst || !lengths || !workspace) return fail(h, RIB_ERR_INVALID, fmt("%s: null pointer", entry));
  if (T < 1 || T > 65535 || H < 1 || W < 1 || H > JPEG_MAX_DIM || W > JPEG_MAX_DIM || quality < 1 || quality > 100)
    return fail(h, RIB_ERR_INVALID, fmt("%s: T=%d H=%d W=%d quality=%d: 1 <= T <= 65535, H and W in 1..%d, quality in 1..100",
                                        entry, T, H, W, quality, JPEG_MAX_DIM));
  if (dst_stride < (size_t)JPEG_HEADER_BYTES + 2 || dst_stride > (size_t)INT32_MAX)
    return fail(h, RIB_ERR_INVALID, fmt("%s: dst_stride=%zu: at least the header (%d bytes) and EOI, below 2 GiB", entry, dst_stride, JPEG_HEADER_BYTES));
  if ((reinterpret_cast<uintptr_t>(workspace) & 15) != 0 || (reinterpret_cast<uintptr_t>(lengths) & 3) != 0)
    return fail(h, RIB_ERR_INVALID, fmt("%s: workspace must be 16-byte aligned, lengths 4-byte aligned", entry));
  if ((reinterpret_cast<uintptr_t>(src) & (alignof(S) - 1)) != 0) return fail(h, RIB_ERR_INVALID, fmt("%s: the source must be 4-byte aligned", entry));
  JpegParamsT<S> jp;
  jp.src = src; jp.H = H; jp.W = W; jp.quality = quality;
  jp.rows = (H + 15) / 16; jp.cols = (W + 15) / 16;
  jp.slot = (uint32_t)jpeg_seg_bound(jp.cols);
  const size_t segs = (size_t)T * jp.rows;
  jp.seg = static_cast<uint8_t*>(workspace);
  jp.seglen = reinterpret_cast<int32_t*>(jp.seg + (segs * jp.slot + 255) / 256 * 256);
  JpegAssembleParams ap;
  ap.seg = jp.seg; ap.seglen = jp.seglen; ap.dst = dst; ap.lengths = lengths; ap.dst_stride = dst_stride; ap.rows = jp.rows; ap.slot = jp.slot;
  jpeg_make_header(ap.header, H, W, quality);
  HIP_TRY(h, hipSetDevice(h->device));
  hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
  hipLaunchKernelGGL((k_jpeg_segments<S>), dim3(jp.rows, T), dim3(256), 0, st, jp);
  HIP_TRY(h, hipGetLastError());
  hipLaunchKernelGGL(k_jpeg_assemble, dim3(jp.rows, T), dim3(256), 0, st, ap);
  HIP_TRY(h, hipGetLastError());
  return RIB_OK;
}
}  // extern "C++"

int rib_jpeg(rib_handle* handle, int T, int H, int W, const uint8_t* src_u8_nhwc, int quality, uint8_t* dst, size_t dst_stride,
             int32_t* lengths, void* workspace, void* hip_stream) {
  return jpeg_enqueue<uint8_t>("rib_jpeg", handle, T, H, W, src_u8_nhwc, quality, dst, dst_stride, lengths, workspace, hip_stream);
}

int rib_jpeg_float(rib_handle* handle, int T, int H, int W, const float* src_f32_nchw, int quality, uint8_t* dst, size_t dst_stride,
                 int32_t* lengths, void* workspace, void* hip_stream) {
  return jpeg_enqueue<float>("rib_jpeg_float", handle, T, H, W, src_f32_nchw, quality, dst, dst_stride, lengths, workspace, hip_stream);
}
static size_t png_strips(int H) { return ((size_t)H + PNG_STRIP_ROWS - 1) / PNG_STRIP_ROWS; }

size_t rib_png_max_bytes(int H, int W) {
  if (H < 1 || W < 1 || H > PNG_MAX_H || W > PNG_MAX_W) return 0;
  const size_t rowN = 1 + 3 * (size_t)W, full = (size_t)H / PNG_STRIP_ROWS, rest = (size_t)H % PNG_STRIP_ROWS;
  size_t total = (size_t)PNG_PREFIX_BYTES + 16 + 12 + full * (12 + png_strip_data_bound(PNG_STRIP_ROWS * rowN));
  if (rest) total += 12 + png_strip_data_bound(rest * rowN);
  return total;
}

size_t rib_png_workspace_bytes(rib_handle* h, int T, int H, int W) {
  if (!h || T < 1 || T > 65535 || H < 1 || W < 1 || H > PNG_MAX_H || W > PNG_MAX_W) return 0;
  const size_t strips = (size_t)T * png_strips(H);
  return align256(strips * png_slot_bytes(W)) + strips * 4 * sizeof(int32_t);      // the slots, then four words per strip
}

int rib_png(rib_handle* handle, int T, int H, int W, const uint8_t* src_u8_nhwc, const uint8_t* code_lengths, int K, uint8_t* dst,
            size_t dst_stride, int32_t* lengths, void* workspace, void* hip_stream) {
  FrameState* h = frame_state(handle);
  if (!h) return RIB_ERR_INVALID;
  if (h->device < 0) return fail(h, RIB_ERR_INVALID, "rib_png: host-only handle");
  if (!src_u8_nhwc || !code_lengths || !dst || !lengths || !workspace) return fail(h, RIB_ERR_INVALID, "rib_png: null pointer");
  if (T < 1 || T > 65535 || H < 1 || H > PNG_MAX_H || W < 1 || W > PNG_MAX_W)
    return fail(h, RIB_ERR_INVALID, fmt("rib_png: T=%d H=%d W=%d: 1 <= T <= 65535, 1 <= H <= %d, 1 <= W <= %d", T, H, W, PNG_MAX_H, PNG_MAX_W));
  if (dst_stride < 1 || dst_stride > (size_t)INT32_MAX) return fail(h, RIB_ERR_INVALID, fmt("rib_png: dst_stride=%zu: at least 1, below 2 GiB", dst_stride));
  if ((reinterpret_cast<uintptr_t>(workspace) & 15) != 0 || (reinterpret_cast<uintptr_t>(lengths) & 3) != 0)
    return fail(h, RIB_ERR_INVALID, "rib_png: workspace must be 16-byte aligned, lengths 4-byte aligned");
  if (K < 1 || K > PNG_MAX_TABLES) return fail(h, RIB_ERR_INVALID, fmt("rib_png: K=%d: 1 <= K <= %d tables", K, PNG_MAX_TABLES));
  HIP_TRY(h, hipSetDevice(h->device));
  hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
  PngTableState& ts = h->png;
  const std::string key(reinterpret_cast<const char*>(code_lengths), (size_t)K * PNG_NSYM);
  if (!ts.dev || ts.key != key) {                        // new tables: validate, build, upload on `stream`
    PngDeviceTables* host = static_cast<PngDeviceTables*>(malloc(sizeof(PngDeviceTables)));
    std::string why;
    if (!host || !png_build_tables(code_lengths, K, host, &why)) {
      free(host);
      return fail(h, RIB_ERR_INVALID, "rib_png: code tables: " + (host ? why : std::string("out of memory")));
    }
    ts.host_all.push_back(host);
    void* dev = nullptr;
    HIP_TRY(h, hipMalloc(&dev, sizeof(PngDeviceTables)));
    ts.dev_all.push_back(dev);
    HIP_TRY(h, hipMemcpyAsync(dev, host, sizeof(PngDeviceTables), hipMemcpyHostToDevice, st));
    ts.dev = dev;
    ts.key = key;
  }
  PngParams pp;
  pp.src = src_u8_nhwc; pp.tab = static_cast<const PngDeviceTables*>(ts.dev);
  pp.H = H; pp.W = W; pp.strips = (int)png_strips(H);
  pp.slot = (uint32_t)png_slot_bytes(W);
  const size_t strips = (size_t)T * pp.strips;
  pp.slots = static_cast<uint8_t*>(workspace);
  pp.meta = reinterpret_cast<int32_t*>(pp.slots + align256(strips * pp.slot));
  PngAssembleParams ap;
  ap.slots = pp.slots; ap.meta = pp.meta; ap.dst = dst; ap.lengths = lengths; ap.dst_stride = dst_stride;
  ap.H = H; ap.W = W; ap.strips = pp.strips; ap.slot = pp.slot;
  png_make_prefix(ap.prefix, H, W);
  const size_t lds = ((size_t)std::min(H, PNG_STRIP_ROWS) * (1 + 3 * (size_t)W) + 15) / 16 * 16;
  if (!ts.lds_ready) {                                   // once per handle, as rib_warp does: up to 98 320 bytes at W = 4096
    HIP_TRY(h, hipFuncSetAttribute(reinterpret_cast<const void*>(&k_png_strips), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)((PNG_STRIP_ROWS * (1 + 3 * (size_t)PNG_MAX_W) + 15) / 16 * 16)));
    ts.lds_ready = true;
  }
  hipLaunchKernelGGL(k_png_strips, dim3(pp.strips, T), dim3(256), lds, st, pp);
  HIP_TRY(h, hipGetLastError());
  hipLaunchKernelGGL(k_png_assemble, dim3(pp.strips, T), dim3(256), 0, st, ap);
  HIP_TRY(h, hipGetLastError());
  return RIB_OK;
}
// rib_mci_*: the workspace of one (B, H, W, levels) - the luma levels of the 2B key frames, then the block fields of the levels
// (before the median); an extra level's plane and field follow those of the level below, so three levels lie where they lay
namespace {
struct MciLayout { int h[MCI_MAX_LEVELS], w[MCI_MAX_LEVELS], Hb[MCI_MAX_LEVELS], Wb[MCI_MAX_LEVELS]; size_t y[MCI_MAX_LEVELS], f[MCI_MAX_LEVELS], total; };
static bool mci_layout(int B, int H, int W, int levels, MciLayout* L) {
  if (B < 1 || B > 32767 || H < 1 || W < 1 || H > MCI_MAX_SIDE || W > MCI_MAX_SIDE) return false;
  if (levels < MCI_MIN_LEVELS || levels > MCI_MAX_LEVELS) return false;
  size_t o = 0;
  for (int l = 0; l < levels; ++l) {
    L->h[l] = l ? (L->h[l - 1] + 1) / 2 : H; L->w[l] = l ? (L->w[l - 1] + 1) / 2 : W;
    L->Hb[l] = (L->h[l] + MCI_BLOCK - 1) / MCI_BLOCK; L->Wb[l] = (L->w[l] + MCI_BLOCK - 1) / MCI_BLOCK;
    L->y[l] = o; o += align256((size_t)2 * B * L->h[l] * L->w[l]);
  }
  if ((size_t)B * L->Hb[0] * L->Wb[0] > (size_t)INT32_MAX / 2) return false;      // block indices (and their (dx, dy) pairs) stay in int
  for (int l = 0; l < levels; ++l) { L->f[l] = o; o += align256((size_t)B * L->Hb[l] * L->Wb[l] * 2 * sizeof(int16_t)); }
  L->total = o;
  return true;
}

// rib_masked_*: rib_mci_field's workspace, then the mask planes of the levels, the searched flags (one plane, level 0's size: a
// level's flags are read - by the fill, on the top level only - before the next level writes its own) and the top level's field
// before the fill
struct MaskedLayout { MciLayout L; size_t m[MCI_MAX_LEVELS], flags, raw, total; };
static void masked_extend(int B, int levels, MaskedLayout* M) {      // M->L is mci_layout's of these levels
  const MciLayout& L = M->L;
  size_t o = L.total;
  for (int l = 0; l < levels; ++l) { M->m[l] = o; o += align256((size_t)2 * B * L.h[l] * L.w[l]); }
  M->flags = o; o += align256((size_t)B * L.Hb[0] * L.Wb[0]);
  M->raw = o; o += align256((size_t)B * L.Hb[levels - 1] * L.Wb[levels - 1] * 2 * sizeof(int16_t));
  M->total = o;
}

// rib_detail_field: the workspace holds the full-size field before the median and nothing else
static bool detail_layout(int B, int H0, int W0, int* H0b, int* W0b, size_t* bytes) {
  if (B < 1 || B > 32767 || H0 < 1 || W0 < 1 || H0 > MCI_MAX_SIDE || W0 > MCI_MAX_SIDE) return false;
  *H0b = (H0 + MCI_BLOCK - 1) / MCI_BLOCK; *W0b = (W0 + MCI_BLOCK - 1) / MCI_BLOCK;
  if ((size_t)B * *H0b * *W0b > (size_t)INT32_MAX / 2) return false;
  *bytes = align256((size_t)B * *H0b * *W0b * 2 * sizeof(int16_t));
  return true;
}

// ---- one function per rule of the rib_* entries below.  A rule's refusal stands here once; an entry lists its rules in its own
// order, chained by ||, and reports the first that fails.
constexpr int SCALED_MAX_RATIO = 16;        // background.SCALED_MAX_RATIO: the largest unit * k * DS stays below 2^31

static int refuse(FrameState* h, const std::string& msg) { return fail(h, RIB_ERR_INVALID, msg); }
static bool off_alignment(const void* p, uintptr_t mask) { return (reinterpret_cast<uintptr_t>(p) & mask) != 0; }

static int mci_handle(rib_handle* handle, const char* who, FrameState** h) {
  *h = frame_state(handle);
  if (!*h) return RIB_ERR_INVALID;
  return (*h)->device < 0 ? refuse(*h, fmt("%s: host-only handle", who)) : RIB_OK;
}
static int need_pointers(FrameState* h, const char* who, bool all) { return all ? RIB_OK : refuse(h, fmt("%s: null pointer", who)); }
static int need_an_output(FrameState* h, const char* who, const void* f32, const void* u8) {
  return f32 || u8 ? RIB_OK : refuse(h, fmt("%s: both outputs are null", who));
}
static int check_shape(FrameState* h, const char* who, int B, int H, int W, int levels, MciLayout* L) {
  if (mci_layout(B, H, W, levels, L)) return RIB_OK;
  return refuse(h, fmt("%s: B=%d H=%d W=%d: 1 <= B <= 32767, H and W in 1..%d, B * ceil(H/8) * ceil(W/8) < 2^30", who, B, H, W, MCI_MAX_SIDE));
}
static int check_frames_shape(FrameState* h, const char* who, int T, int B, int H, int W, MciLayout* L) {
  if (T >= 1 && mci_layout(B, H, W, MCI_MIN_LEVELS, L) && (size_t)T * B <= 65535) return RIB_OK;
  return refuse(h, fmt("%s: T=%d B=%d H=%d W=%d: T, B >= 1, T * B <= 65535, H and W in 1..%d, B * ceil(H/8) * ceil(W/8) < 2^30", who, T, B, H, W, MCI_MAX_SIDE));
}
static int check_keyframe_sides(FrameState* h, const char* who, int H0, int W0) {
  if (H0 >= 1 && W0 >= 1 && H0 <= MCI_MAX_SIDE && W0 <= MCI_MAX_SIDE) return RIB_OK;
  return refuse(h, fmt("%s: H0=%d W0=%d: the key frames' sides lie in 1..%d", who, H0, W0, MCI_MAX_SIDE));
}
static int check_ratio(FrameState* h, const char* who, int H, int W, int H0, int W0) {
  constexpr int R = SCALED_MAX_RATIO;
  if (W0 <= R * W && W <= R * W0 && H0 <= R * H && H <= R * H0) return RIB_OK;
  return refuse(h, fmt("%s: key frames %dx%d, model %dx%d: each axis within 1/%d .. %d times the model's", who, H0, W0, H, W, R, R));
}
static int check_rate(FrameState* h, const char* who, int sample_rate) {
  if (sample_rate >= 1 && sample_rate <= MCI_MAX_RATE && (sample_rate & (sample_rate - 1)) == 0) return RIB_OK;
  return refuse(h, fmt("%s: sample_rate=%d: a power of two in 1..%d", who, sample_rate, MCI_MAX_RATE));
}
static int check_span(FrameState* h, const char* who, int T, int sample_rate, int k_first) {
  if (k_first >= 0 && k_first + T - 1 <= sample_rate) return RIB_OK;
  return refuse(h, fmt("%s: frames %d..%d are outside the segment 0..%d", who, k_first, k_first + T - 1, sample_rate));
}
static int check_border(FrameState* h, const char* who, int border) {
  return border == 0 || border == 1 ? RIB_OK : refuse(h, fmt("%s: border=%d: 0 (clamped samples) or 1 (valid samples only)", who, border));
}
static int check_precision(FrameState* h, const char* who, int precision) {
  if (precision == 0 || precision == 1) return RIB_OK;
  return refuse(h, fmt("%s: precision=%d: 0 (the field in whole pixels) or 1 (in half pixels)", who, precision));
}
static int check_staging(FrameState* h, const char* who, int staging) {
  return staging == 0 || staging == 1 ? RIB_OK : refuse(h, fmt("%s: staging=%d: 0 (the per-tile rule) or 1 (never stage: a diagnostic)", who, staging));
}
static int check_frame_pointers(FrameState* h, const char* who, const void* field_i16, const void* out_f32) {
  return off_alignment(field_i16, 1) || off_alignment(out_f32, 3) ? refuse(h, fmt("%s: misaligned pointer", who)) : RIB_OK;
}

static int scale_16_16(int n0, int n) { return (int)(((int64_t)n0 * 65536 + n / 2) / n); }      // background.scaled_factors
// what k_scaled_frames and k_cubic_scaled want of the two sizes: the 16.16 factors, the divmods behind TX and TY, the row's room in LDS
static void scaled_geometry(int H, int W, int H0, int W0, ScaledFramesParams* fp) {
  fp->sx = scale_16_16(W0, W); fp->sy = scale_16_16(H0, H);
  fp->qax = 32 * W / W0; fp->rax = 32 * W % W0; fp->q0x = 16 * W / W0; fp->r0x = 16 * W % W0;
  fp->qay = 32 * H / H0; fp->ray = 32 * H % H0; fp->q0y = 16 * H / H0; fp->r0y = 16 * H % H0;
  fp->v_off = (W0 * 3 + 31) & ~15;          // the row at any shift 0..15, whole 16-byte lines
}

static int enqueue_median(FrameState* h, hipStream_t st, const int16_t* in, int16_t* out, int B, int Hb, int Wb) {
  const int n = B * Hb * Wb;
  hipLaunchKernelGGL(k_mci_median, dim3(std::min((n + 255) / 256, 1024)), dim3(256), 0, st, in, out, B, Hb, Wb);
  HIP_TRY(h, hipGetLastError());
  return RIB_OK;
}
}  // namespace

extern "C++" {
namespace {
// the frame kernels' parameter structs all carry the segment the same way: s, its log2 and the first frame
template <typename P>
static void set_segment(P& fp, int sample_rate, int k_first) {
  fp.s = sample_rate; fp.k_first = k_first;
  fp.ls = 0;
  while ((1 << fp.ls) < sample_rate) ++fp.ls;
}

// the cubic kernels' dynamic LDS may pass 64 KB (rows wider than about 11 000 pixels): the kernel is told so
template <typename K, typename P>
static hipError_t cubic_launch(K kernel, dim3 grid, size_t lds, hipStream_t st, const P& params) {
  if (lds > 65536) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(kernel, grid, dim3(256), lds, st, params);
  return hipGetLastError();
}
}  // namespace
}  // extern "C++"

void rib_mci_field_shape(int H, int W, int* Hb, int* Wb) {
  if (Hb) *Hb = H < 1 ? 0 : (H + MCI_BLOCK - 1) / MCI_BLOCK;
  if (Wb) *Wb = W < 1 ? 0 : (W + MCI_BLOCK - 1) / MCI_BLOCK;
}

size_t rib_mci_workspace_bytes(rib_handle* h, int B, int H, int W, int levels) {
  MciLayout L;
  if (!h || !mci_layout(B, H, W, levels, &L)) return 0;
  return L.total;
}

size_t rib_masked_workspace_bytes(rib_handle* h, int B, int H, int W, int levels) {
  MaskedLayout M;
  if (!h || !mci_layout(B, H, W, levels, &M.L)) return 0;
  masked_extend(B, levels, &M);
  return M.total;
}

// rib_mci_field / rib_masked_field: one body.  masked: ma_u8, mb_u8 are wanted, the workspace is rib_masked_workspace_bytes', and the
// mask pyramid, the <.., MASKED = true> searches with their flags and the top level's fill run as well.
static int mci_field_enqueue(const char* who, bool masked, rib_handle* handle, int B, int H, int W, const uint8_t* a_u8, const uint8_t* b_u8,
                             const uint8_t* ma_u8, const uint8_t* mb_u8, int16_t* field_i16, int levels, int border, void* workspace,
                             void* hip_stream) {
  FrameState* h;
  MaskedLayout M;
  MciLayout& L = M.L;
  int rc;
  if ((rc = mci_handle(handle, who, &h)) ||
      (rc = need_pointers(h, who, a_u8 && b_u8 && field_i16 && workspace && (!masked || (ma_u8 && mb_u8)))))
    return rc;
  if (levels < MCI_MIN_LEVELS || levels > MCI_MAX_LEVELS)
    return refuse(h, fmt("%s: levels=%d: %d..%d pyramid levels (a search over 32, 64 or 128 px)", who, levels, MCI_MIN_LEVELS, MCI_MAX_LEVELS));
  if ((rc = check_border(h, who, border)) || (rc = check_shape(h, who, B, H, W, levels, &L))) return rc;
  if (off_alignment(workspace, 15) || off_alignment(field_i16, 3))
    return refuse(h, fmt("%s: workspace must be 16-byte aligned, the field 4-byte aligned", who));
  if (masked) masked_extend(B, levels, &M);
  HIP_TRY(h, hipSetDevice(h->device));
  hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
  uint8_t* ws = static_cast<uint8_t*>(workspace);
  MciLumaParams lp;
  lp.a = a_u8; lp.b = b_u8; lp.y0 = ws + L.y[0]; lp.y1 = ws + L.y[1]; lp.y2 = ws + L.y[2];
  lp.y3 = levels > 3 ? ws + L.y[3] : nullptr; lp.y4 = levels > 4 ? ws + L.y[4] : nullptr;
  lp.B = B; lp.H = H; lp.W = W; lp.h1 = L.h[1]; lp.w1 = L.w[1]; lp.h2 = L.h[2]; lp.w2 = L.w[2]; lp.tilesX = (W + 31) / 32;
  lp.h3 = levels > 3 ? L.h[3] : 0; lp.w3 = levels > 3 ? L.w[3] : 0; lp.h4 = levels > 4 ? L.h[4] : 0; lp.w4 = levels > 4 ? L.w[4] : 0;
  const dim3 tiles(lp.tilesX * ((H + 31) / 32), 2 * B);
  hipLaunchKernelGGL(k_mci_luma_pyramid, tiles, dim3(256), 0, st, lp);
  HIP_TRY(h, hipGetLastError());
  if (masked) {
    MciMaskParams mp;
    mp.ma = ma_u8; mp.mb = mb_u8; mp.B = B; mp.levels = levels; mp.tilesX = lp.tilesX;
    for (int l = 0; l < MCI_MAX_LEVELS; ++l) {
      mp.m[l] = l < levels ? ws + M.m[l] : nullptr; mp.h[l] = l < levels ? L.h[l] : 0; mp.w[l] = l < levels ? L.w[l] : 0;
    }
    hipLaunchKernelGGL(k_mci_mask_pyramid, tiles, dim3(256), 0, st, mp);
    HIP_TRY(h, hipGetLastError());
  }
  void (*const search[2][2][2])(MciSearchParams) = {      // [masked][border][top level]
      {{k_mci_search<1, false, false>, k_mci_search<MCI_TOP_R, false, false>}, {k_mci_search<1, true, false>, k_mci_search<MCI_TOP_R, true, false>}},
      {{k_mci_search<1, false, true>, k_mci_search<MCI_TOP_R, false, true>}, {k_mci_search<1, true, true>, k_mci_search<MCI_TOP_R, true, true>}}};
  const int top = levels - 1;
  for (int l = top; l >= 0; --l) {
    MciSearchParams sp;
    sp.y = ws + L.y[l]; sp.coarse = l == top ? nullptr : reinterpret_cast<const int16_t*>(ws + L.f[l + 1]);
    sp.out = reinterpret_cast<int16_t*>(ws + (masked && l == top ? M.raw : L.f[l]));
    sp.B = B; sp.h = L.h[l]; sp.w = L.w[l]; sp.Hb = L.Hb[l]; sp.Wb = L.Wb[l];
    sp.Hbc = l == top ? 1 : L.Hb[l + 1]; sp.Wbc = l == top ? 1 : L.Wb[l + 1];
    sp.m = masked ? ws + M.m[l] : nullptr; sp.searched = masked ? ws + M.flags : nullptr;
    const dim3 grid((sp.Hb * sp.Wb + MCI_RUN - 1) / MCI_RUN, B);
    hipLaunchKernelGGL(search[masked][border][l == top], grid, dim3(256), 0, st, sp);
    HIP_TRY(h, hipGetLastError());
    if (masked && l == top) {               // the fill reads the raw field and the flags, and writes the field the level below starts from
      const int nt = B * sp.Hb * sp.Wb;
      hipLaunchKernelGGL(k_mci_fill, dim3(std::min((nt + 255) / 256, 1024)), dim3(256), 0, st, reinterpret_cast<const int16_t*>(ws + M.raw),
                         static_cast<const uint8_t*>(ws + M.flags), reinterpret_cast<int16_t*>(ws + L.f[top]), B, sp.Hb, sp.Wb);
      HIP_TRY(h, hipGetLastError());
    }
  }
  return enqueue_median(h, st, reinterpret_cast<const int16_t*>(ws + L.f[0]), field_i16, B, L.Hb[0], L.Wb[0]);
}

int rib_mci_field(rib_handle* handle, int B, int H, int W, const uint8_t* a_u8, const uint8_t* b_u8, int16_t* field_i16,
                  int levels, int border, void* workspace, void* hip_stream) {
  return mci_field_enqueue("rib_mci_field", false, handle, B, H, W, a_u8, b_u8, nullptr, nullptr, field_i16, levels, border, workspace, hip_stream);
}

int rib_masked_field(rib_handle* handle, int B, int H, int W, const uint8_t* a_u8, const uint8_t* b_u8, const uint8_t* ma_u8,
                     const uint8_t* mb_u8, int16_t* field_i16, int levels, int border, void* workspace, void* hip_stream) {
  return mci_field_enqueue("rib_masked_field", true, handle, B, H, W, a_u8, b_u8, ma_u8, mb_u8, field_i16, levels, border, workspace, hip_stream);
}

int rib_halfpel_refine(rib_handle* handle, int B, int H, int W, const uint8_t* a_u8, const uint8_t* b_u8, const int16_t* field_i16,
                   int16_t* field_half_i16, int border, void* hip_stream) {
  static const char who[] = "rib_halfpel_refine";
  FrameState* h;
  MciLayout L;
  int rc;
  if ((rc = mci_handle(handle, who, &h)) || (rc = need_pointers(h, who, a_u8 && b_u8 && field_i16 && field_half_i16)) ||
      (rc = check_border(h, who, border)) || (rc = check_shape(h, who, B, H, W, MCI_MIN_LEVELS, &L)))
    return rc;
  if (off_alignment(field_i16, 3) || off_alignment(field_half_i16, 3)) return refuse(h, fmt("%s: the fields must be 4-byte aligned", who));
  HIP_TRY(h, hipSetDevice(h->device));
  MciRefineParams rp;
  rp.a = a_u8; rp.b = b_u8; rp.field = field_i16; rp.out = field_half_i16;
  rp.B = B; rp.H = H; rp.W = W; rp.Hb = L.Hb[0]; rp.Wb = L.Wb[0];
  const dim3 grid((rp.Hb * rp.Wb + MCI_RUN - 1) / MCI_RUN, B);
  hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
  void (*const kernels[2])(MciRefineParams) = {k_mci_refine<false>, k_mci_refine<true>};
  hipLaunchKernelGGL(kernels[border], grid, dim3(256), 0, st, rp);
  HIP_TRY(h, hipGetLastError());
  return RIB_OK;
}

// rib_detail_field: the block field of the FULL-SIZE key frames (background.mci_detail_field_host)
size_t rib_detail_workspace_bytes(rib_handle* h, int B, int H0, int W0) {
  int H0b, W0b;
  size_t n;
  if (!h || !detail_layout(B, H0, W0, &H0b, &W0b, &n)) return 0;
  return n;
}

int rib_detail_field(rib_handle* handle, int B, int H, int W, int H0, int W0, const uint8_t* a0_u8, const uint8_t* b0_u8,
                     const int16_t* field_i16, int precision, int border, int16_t* out_field_i16, void* workspace, void* hip_stream) {
  static const char who[] = "rib_detail_field";
  FrameState* h;
  MciLayout L;
  int rc, H0b, W0b;
  size_t bytes;
  if ((rc = mci_handle(handle, who, &h)) || (rc = need_pointers(h, who, a0_u8 && b0_u8 && field_i16 && out_field_i16 && workspace)) ||
      (rc = check_shape(h, who, B, H, W, MCI_MIN_LEVELS, &L)))
    return rc;
  if (!detail_layout(B, H0, W0, &H0b, &W0b, &bytes))
    return refuse(h, fmt("%s: B=%d H0=%d W0=%d: the key frames' sides lie in 1..%d, B * ceil(H0/8) * ceil(W0/8) < 2^30", who, B, H0, W0, MCI_MAX_SIDE));
  if ((rc = check_ratio(h, who, H, W, H0, W0)) || (rc = check_precision(h, who, precision)) || (rc = check_border(h, who, border))) return rc;
  if (off_alignment(workspace, 15) || off_alignment(field_i16, 3) || off_alignment(out_field_i16, 3))
    return refuse(h, fmt("%s: workspace must be 16-byte aligned, the fields 4-byte aligned", who));
  HIP_TRY(h, hipSetDevice(h->device));
  hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
  DetailSearchParams sp;
  sp.a = a0_u8; sp.b = b0_u8; sp.field = field_i16; sp.out = static_cast<int16_t*>(workspace);
  sp.B = B; sp.H = H; sp.W = W; sp.H0 = H0; sp.W0 = W0; sp.Hb = L.Hb[0]; sp.Wb = L.Wb[0]; sp.H0b = H0b; sp.W0b = W0b;
  sp.sx = scale_16_16(W0, W); sp.sy = scale_16_16(H0, H);
  sp.half = precision;
  const int c = std::max((W0 + W - 1) / W, (H0 + H - 1) / H);
  const int radius = std::min(DETAIL_MAX_R, std::max(1, (c + 1) / 2));      // background.detail_radius
  const dim3 grid((H0b * W0b + MCI_RUN - 1) / MCI_RUN, B);
  void (*const kernels[2][DETAIL_MAX_R])(DetailSearchParams) = {
      {k_detail_search<1, false>, k_detail_search<2, false>, k_detail_search<3, false>, k_detail_search<4, false>},
      {k_detail_search<1, true>, k_detail_search<2, true>, k_detail_search<3, true>, k_detail_search<4, true>}};
  hipLaunchKernelGGL(kernels[border][radius - 1], grid, dim3(256), 0, st, sp);
  HIP_TRY(h, hipGetLastError());
  return enqueue_median(h, st, static_cast<const int16_t*>(workspace), out_field_i16, B, H0b, W0b);
}

// rib_mci_frames / rib_halfpel_frames: one body, one kernel template; half: the field is rib_halfpel_refine's, in half pixels
// rib_masked_frames: the same body again; masked: ma_u8, mb_u8 are wanted, and the kernel is <.., MASKED = true>
static int mci_frames_enqueue(const char* who, bool half, rib_handle* handle, int T, int B, int H, int W, const uint8_t* a_u8, const uint8_t* b_u8,
                              const int16_t* field_i16, int sample_rate, int k_first, int border, float* out_f32_nchw, uint8_t* out_u8_nhwc,
                              void* hip_stream, bool masked = false, const uint8_t* ma_u8 = nullptr, const uint8_t* mb_u8 = nullptr) {
  FrameState* h;
  MciLayout L;
  int rc;
  if ((rc = mci_handle(handle, who, &h)) || (rc = need_pointers(h, who, a_u8 && b_u8 && field_i16 && (!masked || (ma_u8 && mb_u8)))) ||
      (rc = need_an_output(h, who, out_f32_nchw, out_u8_nhwc)) || (rc = check_frames_shape(h, who, T, B, H, W, &L)) ||
      (rc = check_rate(h, who, sample_rate)) || (rc = check_span(h, who, T, sample_rate, k_first)) || (rc = check_border(h, who, border)) ||
      (rc = check_frame_pointers(h, who, field_i16, out_f32_nchw)))
    return rc;
  MciFramesParams fp;
  fp.a = a_u8; fp.b = b_u8; fp.field = field_i16; fp.out_f32 = out_f32_nchw; fp.out_u8 = out_u8_nhwc;
  fp.T = T; fp.B = B; fp.H = H; fp.W = W; fp.Hb = L.Hb[0]; fp.Wb = L.Wb[0];
  set_segment(fp, sample_rate, k_first);
  fp.vec = (W % 4 == 0 && !off_alignment(out_f32_nchw, 15) && !off_alignment(out_u8_nhwc, 3)) ? 1 : 0;
  fp.ma = ma_u8; fp.mb = mb_u8;
  HIP_TRY(h, hipSetDevice(h->device));
  const size_t lds = out_u8_nhwc ? (size_t)W * 3 + 32 : 0;
  void (*const kernels[2][2][2])(MciFramesParams) = {      // [masked][half][border]
      {{k_mci_frames<false, false, false>, k_mci_frames<true, false, false>}, {k_mci_frames<false, true, false>, k_mci_frames<true, true, false>}},
      {{k_mci_frames<false, false, true>, k_mci_frames<true, false, true>}, {k_mci_frames<false, true, true>, k_mci_frames<true, true, true>}}};
  hipLaunchKernelGGL(kernels[masked][half][border], dim3(H, T * B), dim3(256), lds, reinterpret_cast<hipStream_t>(hip_stream), fp);
  HIP_TRY(h, hipGetLastError());
  return RIB_OK;
}

int rib_mci_frames(rib_handle* handle, int T, int B, int H, int W, const uint8_t* a_u8, const uint8_t* b_u8, const int16_t* field_i16,
                   int sample_rate, int k_first, int border, float* out_f32_nchw, uint8_t* out_u8_nhwc, void* hip_stream) {
  return mci_frames_enqueue("rib_mci_frames", false, handle, T, B, H, W, a_u8, b_u8, field_i16, sample_rate, k_first, border, out_f32_nchw,
                            out_u8_nhwc, hip_stream);
}

int rib_halfpel_frames(rib_handle* handle, int T, int B, int H, int W, const uint8_t* a_u8, const uint8_t* b_u8, const int16_t* field_half_i16,
                        int sample_rate, int k_first, int border, float* out_f32_nchw, uint8_t* out_u8_nhwc, void* hip_stream) {
  return mci_frames_enqueue("rib_halfpel_frames", true, handle, T, B, H, W, a_u8, b_u8, field_half_i16, sample_rate, k_first, border,
                            out_f32_nchw, out_u8_nhwc, hip_stream);
}

int rib_masked_frames(rib_handle* handle, int T, int B, int H, int W, const uint8_t* a_u8, const uint8_t* b_u8, const uint8_t* ma_u8,
                      const uint8_t* mb_u8, const int16_t* field_i16, int sample_rate, int k_first, int border, int precision,
                      float* out_f32_nchw, uint8_t* out_u8_nhwc, void* hip_stream) {
  FrameState* h = frame_state(handle);
  if (!h) return RIB_ERR_INVALID;
  if (int rc = check_precision(h, "rib_masked_frames", precision)) return rc;      // (this entry's first rule, before host-only, as it always was)
  return mci_frames_enqueue("rib_masked_frames", precision == 1, handle, T, B, H, W, a_u8, b_u8, field_i16, sample_rate, k_first, border,
                            out_f32_nchw, out_u8_nhwc, hip_stream, true, ma_u8, mb_u8);
}

// rib_scaled_frames / rib_cubic_scaled: the rules they share, in their order (staging = 0 where the entry has none), and what of
// ScaledFramesParams follows from the shapes and the segment
static int scaled_checks(const char* who, rib_handle* handle, int T, int B, int H, int W, int H0, int W0, bool pointers, const int16_t* field_i16,
                         int sample_rate, int k_first, int border, int precision, int staging, FrameState** hp, ScaledFramesParams* fp) {
  MciLayout L;
  int rc;
  if ((rc = mci_handle(handle, who, hp))) return rc;
  FrameState* h = *hp;
  if ((rc = need_pointers(h, who, pointers)) || (rc = check_frames_shape(h, who, T, B, H, W, &L)) || (rc = check_keyframe_sides(h, who, H0, W0)) ||
      (rc = check_ratio(h, who, H, W, H0, W0)) || (rc = check_rate(h, who, sample_rate)) || (rc = check_span(h, who, T, sample_rate, k_first)) ||
      (rc = check_border(h, who, border)) || (rc = check_precision(h, who, precision)) || (rc = check_staging(h, who, staging)) ||
      (rc = check_frame_pointers(h, who, field_i16, nullptr)))
    return rc;
  fp->T = T; fp->B = B; fp->H0 = H0; fp->W0 = W0; fp->Hb = L.Hb[0]; fp->Wb = L.Wb[0];
  set_segment(*fp, sample_rate, k_first);
  scaled_geometry(H, W, H0, W0, fp);
  return RIB_OK;
}

// rib_scaled_frames: rib_mci_frames' uint8 output at the key frames' own size H0 x W0 from the MODEL-size (H x W) field
int rib_scaled_frames(rib_handle* handle, int T, int B, int H, int W, int H0, int W0, const uint8_t* a0_u8, const uint8_t* b0_u8,
                      const int16_t* field_i16, int sample_rate, int k_first, int border, int precision, uint8_t* out_u8_nhwc,
                      void* hip_stream) {
  static const char who[] = "rib_scaled_frames";
  FrameState* h;
  ScaledFramesParams fp;
  int rc;
  if ((rc = scaled_checks(who, handle, T, B, H, W, H0, W0, a0_u8 && b0_u8 && field_i16 && out_u8_nhwc, field_i16, sample_rate, k_first, border,
                          precision, 0, &h, &fp)))
    return rc;
  fp.a = a0_u8; fp.b = b0_u8; fp.field = field_i16; fp.out = out_u8_nhwc;
  fp.vec = (W0 % 4 == 0 && !off_alignment(out_u8_nhwc, 3)) ? 1 : 0;
  const size_t with_field = (size_t)fp.v_off + (size_t)fp.Wb * sizeof(int2);
  fp.stage = with_field <= 65536 ? 1 : 0;
  const size_t lds = fp.stage ? with_field : (size_t)fp.v_off;
  HIP_TRY(h, hipSetDevice(h->device));
  void (*const kernels[2][2])(ScaledFramesParams) = {      // [precision][border]
      {k_scaled_frames<false, false>, k_scaled_frames<true, false>}, {k_scaled_frames<false, true>, k_scaled_frames<true, true>}};
  hipLaunchKernelGGL(kernels[precision][border], dim3(H0, T * B), dim3(256), lds, reinterpret_cast<hipStream_t>(hip_stream), fp);
  HIP_TRY(h, hipGetLastError());
  return RIB_OK;
}

// rib_cubic_frames / rib_cubic_scaled: the 4x4 cubic sampler (background.sample_cubic) behind rib_mci_frames' / rib_halfpel_frames' /
// rib_masked_frames' and rib_scaled_frames' contracts.  The dynamic LDS is the output row, [the blended field row,] the 2 KB weight
// table and - staging = 0 - the four waves' windows.

int rib_cubic_frames(rib_handle* handle, int T, int B, int H, int W, const uint8_t* a_u8, const uint8_t* b_u8, const uint8_t* ma_u8,
                     const uint8_t* mb_u8, const int16_t* field_i16, int sample_rate, int k_first, int border, int precision, int staging,
                     float* out_f32_nchw, uint8_t* out_u8_nhwc, void* hip_stream) {
  static const char who[] = "rib_cubic_frames";
  FrameState* h;
  MciLayout L;
  int rc;
  if ((rc = mci_handle(handle, who, &h)) || (rc = need_pointers(h, who, a_u8 && b_u8 && field_i16))) return rc;
  if ((ma_u8 == nullptr) != (mb_u8 == nullptr))
    return refuse(h, fmt("%s: exactly one mask is null (both: the person is excluded; neither: kept)", who));
  if ((rc = need_an_output(h, who, out_f32_nchw, out_u8_nhwc)) || (rc = check_frames_shape(h, who, T, B, H, W, &L)) ||
      (rc = check_rate(h, who, sample_rate)) || (rc = check_span(h, who, T, sample_rate, k_first)) || (rc = check_border(h, who, border)) ||
      (rc = check_precision(h, who, precision)) || (rc = check_staging(h, who, staging)) ||
      (rc = check_frame_pointers(h, who, field_i16, out_f32_nchw)))
    return rc;
  CubicFramesParams fp;
  fp.a = a_u8; fp.b = b_u8; fp.ma = ma_u8; fp.mb = mb_u8; fp.field = field_i16; fp.out_f32 = out_f32_nchw; fp.out_u8 = out_u8_nhwc;
  fp.T = T; fp.B = B; fp.H = H; fp.W = W; fp.Hb = L.Hb[0]; fp.Wb = L.Wb[0];
  set_segment(fp, sample_rate, k_first);
  fp.stage = staging == 0 ? 1 : 0;
  fp.w_off = out_u8_nhwc ? (W * 3 + 32 + 15) & ~15 : 0;
  const size_t lds = (size_t)fp.w_off + CUBIC_WTAB_BYTES + (fp.stage ? CUBIC_WIN_BYTES : 0);
  HIP_TRY(h, hipSetDevice(h->device));
  void (*const kernels[2][2][2])(CubicFramesParams) = {      // [masked][precision][border]
      {{k_cubic_frames<false, false, false>, k_cubic_frames<true, false, false>}, {k_cubic_frames<false, true, false>, k_cubic_frames<true, true, false>}},
      {{k_cubic_frames<false, false, true>, k_cubic_frames<true, false, true>}, {k_cubic_frames<false, true, true>, k_cubic_frames<true, true, true>}}};
  const hipError_t e = cubic_launch(kernels[ma_u8 != nullptr][precision][border], dim3(H, T * B), lds, reinterpret_cast<hipStream_t>(hip_stream), fp);
  HIP_TRY(h, e);
  return RIB_OK;
}

int rib_cubic_scaled(rib_handle* handle, int T, int B, int H, int W, int H0, int W0, const uint8_t* a0_u8, const uint8_t* b0_u8,
                     const int16_t* field_i16, int sample_rate, int k_first, int border, int precision, int staging, uint8_t* out_u8_nhwc,
                     void* hip_stream) {
  static const char who[] = "rib_cubic_scaled";
  FrameState* h;
  CubicScaledParams cp;
  ScaledFramesParams& fp = cp.f;
  int rc;
  if ((rc = scaled_checks(who, handle, T, B, H, W, H0, W0, a0_u8 && b0_u8 && field_i16 && out_u8_nhwc, field_i16, sample_rate, k_first, border,
                          precision, staging, &h, &fp)))
    return rc;
  fp.a = a0_u8; fp.b = b0_u8; fp.field = field_i16; fp.out = out_u8_nhwc;
  fp.vec = 0;
  fp.stage = 1;                            // the blended field row always has room: at most 49 168 + 16 384 + 2 048 + 29 184 bytes of the CU's 160 KB
  cp.w_off = fp.v_off + ((fp.Wb * (int)sizeof(int2) + 15) & ~15);
  cp.stage_win = staging == 0 ? 1 : 0;
  const size_t lds = (size_t)cp.w_off + CUBIC_WTAB_BYTES + (cp.stage_win ? CUBIC_WIN_BYTES : 0);
  HIP_TRY(h, hipSetDevice(h->device));
  void (*const kernels[2][2])(CubicScaledParams) = {      // [precision][border]
      {k_cubic_scaled<false, false>, k_cubic_scaled<true, false>}, {k_cubic_scaled<false, true>, k_cubic_scaled<true, true>}};
  const hipError_t e = cubic_launch(kernels[precision][border], dim3(H0, T * B), lds, reinterpret_cast<hipStream_t>(hip_stream), cp);
  HIP_TRY(h, e);
  return RIB_OK;
}

// rib_accel_field / rib_accel_frames: the second-order trajectory across key frames (background.mci_accel_host / mci_frames_accel_host).
// The field entry takes block-field shapes, not frame sizes: it serves the model-size fields and rib_detail_field's alike.
static bool accel_layout(int B, int Hb, int Wb, size_t* bytes) {
  constexpr int MAX_BLOCKS = MCI_MAX_SIDE / MCI_BLOCK;
  if (B < 1 || B > 32767 || Hb < 1 || Wb < 1 || Hb > MAX_BLOCKS || Wb > MAX_BLOCKS || (size_t)B * Hb * Wb > (size_t)INT32_MAX / 2) return false;
  *bytes = align256((size_t)B * Hb * Wb * 2 * sizeof(int16_t));
  return true;
}

size_t rib_accel_workspace_bytes(rib_handle* h, int B, int Hb, int Wb) {
  size_t n;
  return h && accel_layout(B, Hb, Wb, &n) ? n : 0;
}

int rib_accel_field(rib_handle* handle, int B, int Hb, int Wb, const int16_t* prev_i16, const int16_t* cur_i16, const int16_t* next_i16,
                    const uint8_t* present_u8, int half, int16_t* accel_i16, void* workspace, void* hip_stream) {
  static const char who[] = "rib_accel_field";
  FrameState* h;
  size_t bytes;
  int rc;
  if ((rc = mci_handle(handle, who, &h)) || (rc = need_pointers(h, who, cur_i16 && accel_i16 && workspace))) return rc;
  if (!accel_layout(B, Hb, Wb, &bytes))
    return refuse(h, fmt("%s: B=%d Hb=%d Wb=%d: 1 <= B <= 32767, Hb and Wb in 1..%d, B * Hb * Wb < 2^30", who, B, Hb, Wb, MCI_MAX_SIDE / MCI_BLOCK));
  if (half != 0 && half != 1) return refuse(h, fmt("%s: half=%d: 0 (the fields in whole pixels) or 1 (in half pixels)", who, half));
  if (off_alignment(prev_i16, 1) || off_alignment(cur_i16, 1) || off_alignment(next_i16, 1) || off_alignment(accel_i16, 1) || off_alignment(workspace, 15))
    return refuse(h, fmt("%s: misaligned pointer", who));
  HIP_TRY(h, hipSetDevice(h->device));
  hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
  MciAccelParams ap;
  ap.prev = prev_i16; ap.cur = cur_i16; ap.next = next_i16; ap.present = present_u8; ap.out = static_cast<int16_t*>(workspace);
  ap.B = B; ap.Hb = Hb; ap.Wb = Wb; ap.shift = half;
  hipLaunchKernelGGL(k_mci_accel, dim3(std::min((B * Hb * Wb + 255) / 256, 1024)), dim3(256), 0, st, ap);
  HIP_TRY(h, hipGetLastError());
  return enqueue_median(h, st, static_cast<const int16_t*>(workspace), accel_i16, B, Hb, Wb);
}

static int check_sampler(FrameState* h, const char* who, int sampler) {
  return sampler == 0 || sampler == 1 ? RIB_OK : refuse(h, fmt("%s: sampler=%d: 0 (bilinear) or 1 (the 4x4 cubic sample)", who, sampler));
}
static int check_accel_pointer(FrameState* h, const char* who, const void* accel_i16) {
  if (!accel_i16) return refuse(h, fmt("%s: the acceleration field is null (rib_accel_field makes it)", who));
  return off_alignment(accel_i16, 1) ? refuse(h, fmt("%s: misaligned acceleration field", who)) : RIB_OK;
}
static int check_mask_pair(FrameState* h, const char* who, const void* ma_u8, const void* mb_u8) {
  if ((ma_u8 == nullptr) == (mb_u8 == nullptr)) return RIB_OK;
  return refuse(h, fmt("%s: exactly one mask is null (both: the person is excluded; neither: kept)", who));
}

int rib_accel_frames(rib_handle* handle, int T, int B, int H, int W, const uint8_t* a_u8, const uint8_t* b_u8, const uint8_t* ma_u8,
                     const uint8_t* mb_u8, const int16_t* field_i16, const int16_t* accel_i16, int sample_rate, int k_first, int border,
                     int precision, int sampler, float* out_f32_nchw, uint8_t* out_u8_nhwc, void* hip_stream) {
  static const char who[] = "rib_accel_frames";
  FrameState* h;
  MciLayout L;
  int rc;
  if ((rc = mci_handle(handle, who, &h)) || (rc = need_pointers(h, who, a_u8 && b_u8 && field_i16)) ||
      (rc = need_an_output(h, who, out_f32_nchw, out_u8_nhwc)) || (rc = check_frames_shape(h, who, T, B, H, W, &L)) ||
      (rc = check_rate(h, who, sample_rate)) || (rc = check_span(h, who, T, sample_rate, k_first)) || (rc = check_border(h, who, border)) ||
      (rc = check_precision(h, who, precision)) || (rc = check_sampler(h, who, sampler)) || (rc = check_accel_pointer(h, who, accel_i16)) ||
      (rc = check_mask_pair(h, who, ma_u8, mb_u8)) || (rc = check_frame_pointers(h, who, field_i16, out_f32_nchw)))
    return rc;
  const bool masked = ma_u8 != nullptr;
  hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
  HIP_TRY(h, hipSetDevice(h->device));
  if (sampler == 1) {
    CubicAccelParams ap;
    CubicFramesParams& fp = ap.f;
    fp.a = a_u8; fp.b = b_u8; fp.ma = ma_u8; fp.mb = mb_u8; fp.field = field_i16; fp.out_f32 = out_f32_nchw; fp.out_u8 = out_u8_nhwc;
    fp.T = T; fp.B = B; fp.H = H; fp.W = W; fp.Hb = L.Hb[0]; fp.Wb = L.Wb[0];
    set_segment(fp, sample_rate, k_first);
    fp.stage = 1;
    fp.w_off = out_u8_nhwc ? (W * 3 + 32 + 15) & ~15 : 0;
    ap.accel = accel_i16;
    const size_t lds = (size_t)fp.w_off + CUBIC_WTAB_BYTES + CUBIC_WIN_BYTES;
    void (*const kernels[2][2][2])(CubicAccelParams) = {      // [masked][precision][border]
        {{k_cubic_accel<false, false, false>, k_cubic_accel<true, false, false>}, {k_cubic_accel<false, true, false>, k_cubic_accel<true, true, false>}},
        {{k_cubic_accel<false, false, true>, k_cubic_accel<true, false, true>}, {k_cubic_accel<false, true, true>, k_cubic_accel<true, true, true>}}};
    HIP_TRY(h, cubic_launch(kernels[masked][precision][border], dim3(H, T * B), lds, st, ap));
    return RIB_OK;
  }
  AccelFramesParams ap;
  MciFramesParams& fp = ap.f;
  fp.a = a_u8; fp.b = b_u8; fp.field = field_i16; fp.out_f32 = out_f32_nchw; fp.out_u8 = out_u8_nhwc;
  fp.T = T; fp.B = B; fp.H = H; fp.W = W; fp.Hb = L.Hb[0]; fp.Wb = L.Wb[0];
  set_segment(fp, sample_rate, k_first);
  fp.vec = (W % 4 == 0 && !off_alignment(out_f32_nchw, 15) && !off_alignment(out_u8_nhwc, 3)) ? 1 : 0;
  fp.ma = ma_u8; fp.mb = mb_u8;
  ap.accel = accel_i16;
  const size_t lds = out_u8_nhwc ? (size_t)W * 3 + 32 : 0;
  void (*const kernels[2][2][2])(AccelFramesParams) = {      // [masked][precision][border]
      {{k_accel_frames<false, false, false>, k_accel_frames<true, false, false>}, {k_accel_frames<false, true, false>, k_accel_frames<true, true, false>}},
      {{k_accel_frames<false, false, true>, k_accel_frames<true, false, true>}, {k_accel_frames<false, true, true>, k_accel_frames<true, true, true>}}};
  hipLaunchKernelGGL(kernels[masked][precision][border], dim3(H, T * B), dim3(256), lds, st, ap);
  HIP_TRY(h, hipGetLastError());
  return RIB_OK;
}
}  // extern "C"
