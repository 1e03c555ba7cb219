// panel.hip.h — the six-pane diagnostic sheet of the folder driver, composed on the GPU (rib_panel, include/rib.h).
//
// The reference's evaluate_from_folder(gen_vid=True) shows, per frame, Predict | Mask | Fuse over DAIN | Ground Truth |
// Skeleton (PGNR/utils/visualize.py make_video, pane bytes by tensor2images, PGNR/utils/utils.py:122-147).  panel.py states
// our sheet as an exact integer definition (layout, compose_host); this kernel writes the same bytes from the fp32 NCHW
// tensors the unit already holds on the device, so that one finished uint8 sheet per frame is all that travels home.
//
//   sheet   2 rows x 3 panes of H x W, PANEL_GUTTER px of white (255) around and between them, a PANEL_TITLE px title bar
//           over each pane row: SH = 2 (H + 24) + 3 * 8, SW = 3 W + 4 * 8, uint8 HWC.
//   panes   3-channel panes: quantise_u8 (pixel_ops.hip.h, the arithmetic of rib_quantise); the 1-channel Mask pane:
//           uint8(double(m) * 255.0), truncating, no clip, on all three channels; Skeleton: label channels 0..2.
//   titles  optional 0/1 bitmap [2, 24, SW] (made on the host from panel.py's glyph table): a set pixel is (0, 0, 255).
//   key     pred == mask == fuse == NULL: Predict and Fuse show gt, Mask is 0 (a key frame passes through the driver).
//
//   k_panel grid (SH, T): a workgroup owns ONE row of one sheet (9 W + 96 bytes) and writes all of it - gutters, title
//           bar, panes; nothing is cleared beforehand.  The row is built in LDS and stored from there:
//             1. the LDS row is filled with 255 (16-byte writes);
//             2. pane rows: a thread takes 4 consecutive x of one pane - one float4 per channel plane (the planes are
//                x-contiguous: 16 lanes cover a 256-byte run of a plane), quantises, and writes the 12 interleaved bytes
//                as three dwords into LDS; title rows: a thread per sheet pixel that is set in the bitmap;
//             3. the row leaves as 16-byte stores that are contiguous across the wave (1 KiB per instruction).  The LDS
//                row starts at the global row's own phase inside a 16-byte line (row bytes are a multiple of 16 only
//                when W % 16 == 0), so an aligned 16-byte line of LDS is an aligned 16-byte line of global memory; the
//                partial lines at the two ends of a row go out as bytes (they belong to the neighbouring rows' blocks).
//           W % 4 != 0 or a pointer off its 16-byte / 4-byte alignment takes scalar loads and byte LDS writes.
//
// Per source pixel the launch reads 16 floats (pred 3, mask 1, fuse 3, dain 3, gt 3, label 3) and writes 18 bytes.
// One launch, no atomics, no workspace: a sheet's bytes do not depend on T.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pixel_ops.hip.h"

namespace rib {

constexpr int PANEL_GUTTER = 8, PANEL_TITLE = 24;      // panel.py GUTTER, TITLE_H
constexpr int PANEL_MAX_W = 4096, PANEL_MAX_H = 16384; // the LDS row: 9 * 4096 + 128 bytes < 64 KB

struct PanelParams {
  const float *pred, *mask, *fuse, *dain, *gt, *label;  // pred / mask / fuse all null: key-frame mode
  const uint8_t* titles;                                // [2, PANEL_TITLE, SW] 0/1, or null
  uint8_t* out;                                         // [T, SH, SW, 3]
  int H, W, label_nc, SH, SW;
  int vec;                                              // float4 loads + dword LDS writes are aligned
};

__device__ inline uint8_t panel_mask_u8(float m) { return (uint8_t)(int)((double)m * 255.0); }

// four consecutive x of one plane row; x0 + j >= W reads nothing (0)
__device__ inline void panel_load4(const float* row, int x0, int W, int vec, float v[4]) {
  if (vec) {
    const float4 f = *reinterpret_cast<const float4*>(row + x0);
    v[0] = f.x; v[1] = f.y; v[2] = f.z; v[3] = f.w;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = x0 + j < W ? row[x0 + j] : 0.0f;
  }
}

__global__ __launch_bounds__(256) void k_panel(PanelParams p) {
  extern __shared__ __attribute__((aligned(16))) uint8_t s_panel[];
  const int sy = blockIdx.x, t = blockIdx.y;
  const int H = p.H, W = p.W;
  const int rowbytes = p.SW * 3;
  uint8_t* grow = p.out + ((size_t)t * p.SH + sy) * (size_t)rowbytes;
  const int shift = (int)(reinterpret_cast<uintptr_t>(grow) & 15);
  uint8_t* srow = s_panel + shift;
  const int nlines = (shift + rowbytes + 15) >> 4;
  for (int j = threadIdx.x; j < nlines; j += 256) reinterpret_cast<uint4*>(s_panel)[j] = make_uint4(~0u, ~0u, ~0u, ~0u);
  __syncthreads();
  const int band = PANEL_TITLE + H + PANEL_GUTTER;      // title bar + panes + the gutter below them
  const int rel = sy - PANEL_GUTTER;
  const int r = rel >= 0 ? rel / band : 2;
  const int yy = rel - r * band;
  if (r < 2 && yy < PANEL_TITLE) {
    if (p.titles) {
      const uint8_t* bits = p.titles + (size_t)(r * PANEL_TITLE + yy) * p.SW;
      for (int sx = threadIdx.x; sx < p.SW; sx += 256)
        if (bits[sx]) { srow[sx * 3] = 0; srow[sx * 3 + 1] = 0; }      // (0, 0, 255)
    }
  } else if (r < 2 && yy < PANEL_TITLE + H) {
    const int y = yy - PANEL_TITLE;
    const bool key = p.pred == nullptr;
    const size_t HW = (size_t)H * W;
    const int W4 = (W + 3) >> 2;
    for (int item = threadIdx.x; item < 3 * W4; item += 256) {
      const int pc = item / W4, x0 = (item - pc * W4) * 4;
      const int pane = r * 3 + pc;
      uint8_t b[12];
      if (pane == 1) {                                  // Mask: one plane on three channels
        float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (!key) panel_load4(p.mask + (size_t)t * HW + (size_t)y * W, x0, W, p.vec, v);
#pragma unroll
        for (int j = 0; j < 4; ++j) b[j * 3] = b[j * 3 + 1] = b[j * 3 + 2] = key ? (uint8_t)0 : panel_mask_u8(v[j]);
      } else {
        const float* src = pane == 0 ? (key ? p.gt : p.pred) : pane == 2 ? (key ? p.gt : p.fuse) : pane == 3 ? p.dain : pane == 4 ? p.gt : p.label;
        const size_t frame = (size_t)t * (pane == 5 ? p.label_nc : 3) * HW;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          float v[4];
          panel_load4(src + frame + c * HW + (size_t)y * W, x0, W, p.vec, v);
#pragma unroll
          for (int j = 0; j < 4; ++j) b[j * 3 + c] = quantise_u8(v[j]);
        }
      }
      uint8_t* dst = srow + (PANEL_GUTTER + pc * (W + PANEL_GUTTER) + x0) * 3;
      if (p.vec) {
#pragma unroll
        for (int d = 0; d < 3; ++d)
          reinterpret_cast<uint32_t*>(dst)[d] = (uint32_t)b[4 * d] | ((uint32_t)b[4 * d + 1] << 8) | ((uint32_t)b[4 * d + 2] << 16) | ((uint32_t)b[4 * d + 3] << 24);
      } else {
        const int nb = min(4, W - x0) * 3;
#pragma unroll
        for (int j = 0; j < 12; ++j)
          if (j < nb) dst[j] = b[j];
      }
    }
  }
  __syncthreads();
  uint8_t* gline = grow - shift;                        // 16-byte aligned; only bytes [shift, shift + rowbytes) are this row's
  for (int j = threadIdx.x; j < nlines; j += 256) {
    const int lo = j * 16;
    if (lo >= shift && lo + 16 <= shift + rowbytes) {
      *reinterpret_cast<uint4*>(gline + lo) = reinterpret_cast<const uint4*>(s_panel)[j];
    } else {
      for (int k = max(lo, shift); k < min(lo + 16, shift + rowbytes); ++k) gline[k] = s_panel[k];
    }
  }
}

}  // namespace rib
