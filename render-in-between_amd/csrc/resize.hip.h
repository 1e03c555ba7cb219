// resize.hip.h — 8-bit cubic frame resize of the folder driver on the GPU (rib_resize_cubic, include/rib.h).
//
// The reference resizes every frame to the model size with albumentations' A.Resize(interpolation=cv2.INTER_CUBIC)
// (PGNR/models/evaluator.py:18-26, applied at :219-221); resize.py restates OpenCV's 8-bit INTER_CUBIC on the host and
// this kernel computes exactly what resize.resize_cubic_u8 computes.  The per-axis tap tables - clamped source indices
// [dst, 4] and 11-bit fixed-point coefficients [dst, 4], both int32 - are made on the host by resize._cubic_taps and
// uploaded: the float32 weight arithmetic is not restated here.  What is left is integer arithmetic, and integer
// addition is order-free, so the result does not depend on how the 16 taps are summed.
//
//   k_resize_cubic_u8   grid (tiles, N).  A workgroup of 4 waves owns RSZ_TH output rows by 64 columns of one frame; a
//                       lane owns one column and RSZ_TH / 4 rows.  A column is one BYTE of the interleaved output row
//                       (x * 3 + c): the three channels of a pixel sit in neighbouring lanes, so the 16 byte loads of a
//                       lane gather, per wave instruction, from a span of about 64 * scale source bytes (one to three
//                       128-byte lines when reducing 2-4x) and the uint8 store is one contiguous 64-byte segment.  The
//                       column's four taps live in registers for all of the lane's rows, the tile's row taps in LDS
//                       (every lane of a wave reads the same word: a broadcast).  The source footprint of a tile is
//                       sparse when reducing, so the taps are gathered straight from global memory / L2.
//                       (Measured against the other mapping, a lane per PIXEL looping over its three channels, on 16 frames
//                       1920x1080 -> 512x512 with the fp32 output: 109.8 us against 108.7 us median of 20 launches, inside
//                       the 1 % spread of either; this one is kept for its contiguous uint8 store.)
//                       Outputs, either or both: uint8 NHWC (what resize_cubic_u8 returns) and fp32 NCHW holding
//                       ToTensor + Normalize(0.5, 0.5) of it (below).
//
// One launch per call, no atomics, no workspace beyond the tables: a frame's bytes do not depend on N or on the run.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rib {

#define RSZ_TW 64                    // output tile: 64 byte columns (one per lane of a wave) ...
#define RSZ_TH 16                    // ... by 16 rows, 4 per wave
#define RSZ_COEF_BITS 11             // resize.py _COEF_BITS (OpenCV INTER_RESIZE_COEF_BITS)

// ToTensor + Normalize(0.5, 0.5) of one uint8 value as the folder driver's upload computes it with torch on the device,
// ((float(u8) / 255.0 - 0.5) / 0.5): three separately rounded fp32 operations, nothing contracted into an FMA.  torch
// evaluates a division by a host scalar on the device as a multiplication by the scalar's reciprocal rounded to fp32
// (float(1.0 / 255.0), and 2.0f for 0.5, which is exact), so that is what is written here: a true division by 255
// differs from it in the last bit for some of the 256 values (tests/test_gpu_resize.py holds all 256 to torch).
__device__ inline float rsz_normalise(int u8) {
#pragma clang fp contract(off)
  const float inv255 = (float)(1.0 / 255.0);
  float f = (float)u8 * inv255;
  f = f - 0.5f;
  return f * 2.0f;
}

// src [N, H0, W0, 3] uint8; ix, cx [W, 4] and iy, cy [H, 4] int32 (resize._cubic_taps); out_u8 [N, H, W, 3] uint8 or null;
// out_f32 [N, 3, H, W] fp32 or null.
__global__ __launch_bounds__(256) void k_resize_cubic_u8(const uint8_t* __restrict__ src, const int4* __restrict__ ix,
                                                          const int4* __restrict__ cx, const int4* __restrict__ iy,
                                                          const int4* __restrict__ cy, uint8_t* __restrict__ out_u8,
                                                          float* __restrict__ out_f32, int H0, int W0, int H, int W, int tilesX) {
  __shared__ int4 s_iy[RSZ_TH], s_cy[RSZ_TH];
  const int tx = blockIdx.x % tilesX, ty = blockIdx.x / tilesX;
  const int n = blockIdx.y;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int y0 = ty * RSZ_TH;
  if (threadIdx.x < RSZ_TH) {
    const int y = min(y0 + (int)threadIdx.x, H - 1);          // (rows past the frame are never read back)
    s_iy[threadIdx.x] = iy[y];
    s_cy[threadIdx.x] = cy[y];
  }
  __syncthreads();
  const int col = tx * RSZ_TW + lane;                         // byte column of the interleaved output row: x * 3 + c
  if (col >= W * 3) return;
  const int x = col / 3, c = col - x * 3;
  const int4 tix = ix[x], tcx = cx[x];
  // (the tables come clamped from resize._cubic_taps; clamping again keeps a bad table of a C caller inside the frame)
  const int o0 = min(max(tix.x, 0), W0 - 1) * 3 + c, o1 = min(max(tix.y, 0), W0 - 1) * 3 + c;
  const int o2 = min(max(tix.z, 0), W0 - 1) * 3 + c, o3 = min(max(tix.w, 0), W0 - 1) * 3 + c;
  const size_t pitch = (size_t)W0 * 3;
  const uint8_t* frame = src + (size_t)n * H0 * pitch;
#pragma unroll
  for (int r = 0; r < RSZ_TH / 4; ++r) {
    const int ry = wave * (RSZ_TH / 4) + r;
    const int y = y0 + ry;
    if (y >= H) break;
    const int4 tiy = s_iy[ry], tcy = s_cy[ry];
    const int rows[4] = {min(max(tiy.x, 0), H0 - 1), min(max(tiy.y, 0), H0 - 1), min(max(tiy.z, 0), H0 - 1), min(max(tiy.w, 0), H0 - 1)};
    const int wy[4] = {tcy.x, tcy.y, tcy.z, tcy.w};
    // exact in int32 as in OpenCV: |v| <= 255 * (1.375 * 2048)^2 < 2^31, which also covers v + 2^21 below
    int v = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const uint8_t* p = frame + (size_t)rows[j] * pitch;
      const int hsum = tcx.x * (int)p[o0] + tcx.y * (int)p[o1] + tcx.z * (int)p[o2] + tcx.w * (int)p[o3];
      v += wy[j] * hsum;
    }
    v = (v + (1 << (2 * RSZ_COEF_BITS - 1))) >> (2 * RSZ_COEF_BITS);          // FixedPtCast<int, uchar, 22>: arithmetic shift
    v = min(max(v, 0), 255);
    if (out_u8) out_u8[((size_t)n * H + y) * ((size_t)W * 3) + col] = (uint8_t)v;
    if (out_f32) out_f32[(((size_t)n * 3 + c) * H + y) * (size_t)W + x] = rsz_normalise(v);
  }
}

}  // namespace rib
